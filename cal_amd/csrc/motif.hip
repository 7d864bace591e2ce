// Exact motif matching: the embeddings of small connected patterns in every graph of a batch, the device operator behind
// cal_amd/motif.py (motif_match; contains / isomorphic / where).  The contract -- graph semantics, match order, roots, steps and
// budget, the outputs -- is in cal_hip.h.  Integers only: this file has no floating point.
//
// cal_motif_match, k_motif_match: one workgroup of 256 threads per target graph, for all P patterns.
//  * the adjacency is a 256 x 256 bit matrix in LDS, four 64-bit words per row (8 KB), built once from the graph's columns with
//    64-bit LDS OR-atomics (a duplicate column or the reverse column sets a set bit again: the order cannot show).
//  * the launcher plans every pattern on the host (match order, parents, adjacency by position) and passes the plans by value,
//    as kernel arguments; the workgroup copies them to LDS.
//  * a set cell (u, w) of the matrix is a root.  The rows are cut into items of 16 cells (of one cell in a graph of at most 64
//    nodes, where every cell can have a lane of its own); a lane that has no root in hand
//    takes the next item from a counter in LDS (an integer atomic) and the next set cell of its item, so the roots are dealt
//    as lanes come free and ONE loop holds both the dealing and the search: the lanes of a wave step together whatever their
//    roots, and a wave lasts as long as its longest lane, not as the sum of its longest roots.  A workgroup lasts at least as
//    long as its longest root: a root is not split, its steps are counted in the order of the search.
//  * a lane searches below its root alone, depth first: the images so far are the bytes of ONE 64-bit word in pattern-node
//    order (the key of `first`, node 0 in the top byte), the cursors of the positions 2 .. 7 nine bits each of another, so
//    the stack stays in registers; the next neighbour of the parent's image is found with count-trailing-zeros on the row's
//    words; the adjacency tests of a candidate are independent LDS reads, issued together (any byte of the key is a valid
//    row, so the reads need no guard) and combined without a branch.
//  * the LAST position is not walked: its candidates are the parent's row, the ones that fit are that row ANDed with the rows
//    the pattern wants adjacent (and with the complements of the others, when induced), less the images and the wrong labels
//    (a bit row per position, made with ballots); two population counts give the steps and the embeddings, the lowest bit
//    the smallest key, and a budget that ends inside the row keeps its first few bits.  The leaves are most of a search.
//  * all P patterns run in the same loop: an item is a pattern and a piece of a row, the items are dealt pattern by pattern, and
//    a lane keeps its pattern's plan in registers (the plans, the labels by position and the label rows wait in LDS).  So the
//    workgroup lasts as long as the longest root of any pattern, not as the sum over the patterns of their longest roots, and
//    there is no barrier between patterns.
//  * count and truncated are integer sums and first an unsigned 64-bit minimum: a lane keeps them in registers while it stays
//    with a pattern and hands them in with 64-bit LDS atomics (add, min) when it moves on.  Integer sums and a minimum: the
//    order cannot show.  No global atomics but the ignored-column count.
#include "cal_hip.h"
#include "segment.hpp"

namespace cal {
namespace {

typedef unsigned long long u64;

constexpr int kMotifNT = 256;                        // threads of a workgroup
constexpr int kMotifP = CAL_MOTIF_MAX_PATTERNS;
// (kMotifN, kMotifK, MotifPlan -- one pattern, planned -- and motif_plan, the planner the launcher runs on the host: rules.hpp)

struct MotifArgs {
    const int64_t* ei;         // [2, E]
    int64_t E, N;
    const int64_t* ptr;        // [B + 1]
    const int64_t* eptr;       // [B + 1]
    const int64_t* lab;        // [N] or null
    const int64_t* plab;       // [PN] or null
    int64_t P, budget;
    int induced;
    int64_t* count;            // [B, P]
    int64_t* trunc;            // [B, P]
    int32_t* first;            // [B, P, 8]
    int64_t* tgt_edges;        // [B]
    int64_t* pat_edges;        // [P]
    u64* totals;               // [1]
    MotifPlan plan[kMotifP];
};
static_assert(sizeof(MotifArgs) <= 4096, "the plans travel as kernel arguments");

// the pattern a lane is working on, in registers
struct MotifPat {
    u64 order, padj;
    uint32_t parent;
    int k;
};

__device__ __forceinline__ bool adj_bit(const u64* adj, int a, int b) { return (adj[a * 4 + (b >> 6)] >> (b & 63)) & 1ull; }

// the lowest set bit of row `a` at or above s (0 <= s <= 256); 256: none
__device__ __forceinline__ int next_neighbour(const u64* adj, int a, int s) {
    for (int w = s >> 6; w < 4; ++w) {
        u64 m = adj[a * 4 + w];
        if (w == (s >> 6)) m &= ~0ull << (s & 63);
        if (m) return w * 64 + __builtin_ctzll(m);
    }
    return kMotifN;
}

// may v take position d?  key holds the images of the positions before d.
__device__ __forceinline__ bool motif_fits(const u64* adj, const MotifPat& q, const int64_t* tlab, const int64_t* plab, bool labelled,
                                           int induced, u64 key, int d, int v) {
    bool ok = !labelled || tlab[v] == plab[d];
    const unsigned need = (unsigned)(q.padj >> (8 * d)) & 0xFFu;
#pragma unroll
    for (int j = 0; j < kMotifK - 1; ++j) {                           // (position d <= 7 has at most 7 before it)
        const int x = (int)(key >> (56 - 8 * (int)((q.order >> (8 * j)) & 0xFF))) & 0xFF;
        const bool a = adj_bit(adj, v, x);                            // (j >= d: a stale or blank byte, still a row of adj)
        ok &= j >= d || (x != v && ((need >> j) & 1u ? a : !(induced && a)));
    }
    return ok;
}

// The LAST position, all its candidates at once.  The neighbours of the parent's image are the steps (as many as the budget
// still allows, in ascending id); the ones among them that fit -- a few ANDs of rows of the matrix -- are the embeddings, the
// lowest of them the smallest key below this prefix.  lmask: the nodes that carry the position's label (null: no labels).
// -> true: the budget cut the row short, the root stops.
__device__ __forceinline__ bool motif_last(const u64* adj, const u64* lmask, const MotifPat& q, int induced, u64 key, int d,
                                           u64 budget, u64& steps, u64& cnt, u64& best) {
    const int pd = (int)(q.parent >> (3 * d)) & 7;
    const int px = (int)(key >> (56 - 8 * (int)((q.order >> (8 * pd)) & 0xFF))) & 0xFF;
    const unsigned need = (unsigned)(q.padj >> (8 * d)) & 0xFFu;
    u64 row[4], ok[4];
#pragma unroll
    for (int w = 0; w < 4; ++w) ok[w] = row[w] = adj[px * 4 + w];
#pragma unroll
    for (int j = 0; j < kMotifK - 1; ++j) {                           // (j >= d: a stale or blank byte, still a row of adj)
        const int x = (int)(key >> (56 - 8 * (int)((q.order >> (8 * j)) & 0xFF))) & 0xFF;
        const bool wanted = (need >> j) & 1u;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const u64 r = adj[x * 4 + w];
            u64 m = wanted ? r : (induced ? ~r : ~0ull);
            m &= ~((u64)((x >> 6) == w) << (x & 63));                 // an image is used
            ok[w] &= j < d ? m : ~0ull;
        }
    }
    if (lmask) {
#pragma unroll
        for (int w = 0; w < 4; ++w) ok[w] &= lmask[w];
    }
    const u64 total = __popcll(row[0]) + __popcll(row[1]) + __popcll(row[2]) + __popcll(row[3]);
    const bool cut = steps + total > budget;
    if (cut) {                                                        // only the first budget - steps neighbours are tried
        u64 allow = budget - steps;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const u64 c = __popcll(row[w]);
            u64 keep = ~0ull;
            if (allow >= c) {
                allow -= c;
            } else {
                u64 m = row[w];
                keep = 0;
                for (; allow; --allow) {
                    keep |= m & (~m + 1);
                    m &= m - 1;
                }
            }
            ok[w] &= keep;
        }
        steps = budget;
    } else {
        steps += total;
    }
    const int c = __popcll(ok[0]) + __popcll(ok[1]) + __popcll(ok[2]) + __popcll(ok[3]);
    if (c) {
        const int v = ok[0] ? __builtin_ctzll(ok[0]) : ok[1] ? 64 + __builtin_ctzll(ok[1]) : ok[2] ? 128 + __builtin_ctzll(ok[2])
                                                                                              : 192 + __builtin_ctzll(ok[3]);
        const int shd = 56 - 8 * (int)((q.order >> (8 * d)) & 0xFF);
        const u64 nk = (key & ~(0xFFull << shd)) | ((u64)v << shd);
        cnt += (u64)c;
        best = nk < best ? nk : best;
    }
    return cut;
}

// grid B, kMotifNT threads
__global__ void __launch_bounds__(kMotifNT) k_motif_match(MotifArgs a) {
    __shared__ u64 adj[kMotifN * 4];
    __shared__ int64_t tlab[kMotifN];
    __shared__ MotifPlan plan[kMotifP];
    __shared__ int64_t plab[kMotifP][kMotifK];                        // the patterns' labels, by position
    __shared__ u64 lmask[kMotifP][kMotifK][4];                        // per position: the nodes that carry its label, as a bit row
    __shared__ u64 acc[kMotifP][3];                                   // per pattern: count, truncated, the smallest key
    __shared__ long long red[kMotifNT / 64];
    __shared__ int next_item;
    constexpr int NT = kMotifNT;
    const int64_t g = blockIdx.x, N = a.N, E = a.E;
    const int P = (int)a.P;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t nlo, n64, elo, m;
    seg_clamp(a.ptr, g, N, nlo, n64);
    seg_clamp(a.eptr, g, E, elo, m);
    const bool skip = n64 > kMotifN;                                  // (uniform)
    const int n = skip ? 0 : (int)n64;
    for (int i = tid; i < kMotifN * 4; i += NT) adj[i] = 0;
    for (int i = tid; i < P; i += NT) {
        plan[i] = a.plan[i];
        acc[i][0] = 0;
        acc[i][1] = 0;
        acc[i][2] = ~0ull;
        if (g == 0) a.pat_edges[i] = a.plan[i].edges;
    }
    if (tid == 0) next_item = 0;
    __syncthreads();
    int64_t ign = 0;
    for (int64_t e = tid; e < m; e += NT) {
        const int64_t u = a.ei[elo + e] - nlo, v = a.ei[E + elo + e] - nlo;
        if (!(u >= 0 && u < n64 && v >= 0 && v < n64)) {
            ++ign;
        } else if (!skip && u != v) {
            atomicOr(&adj[(int)u * 4 + ((int)v >> 6)], 1ull << ((int)v & 63));
            atomicOr(&adj[(int)v * 4 + ((int)u >> 6)], 1ull << ((int)u & 63));
        }
    }
    const bool labelled = a.lab != nullptr;
    if (labelled && tid < n) tlab[tid] = a.lab[nlo + tid];
    if (labelled)
        for (int i = tid; i < P * kMotifK; i += NT) {
            const MotifPlan& q = plan[i / kMotifK];
            const int d = i % kMotifK;
            if (d < q.k) plab[i / kMotifK][d] = a.plab[q.lo + (int64_t)((q.order >> (8 * d)) & 0xFF)];
        }
    ign = wg_sum<NT>(ign, red);                                       // (its barriers publish the matrix and the labels)
    if (tid == 0 && ign) atomicAdd(a.totals, (u64)ign);
    if (skip) {
        for (int64_t i = tid; i < P; i += NT) {
            a.count[g * P + i] = -1;
            a.trunc[g * P + i] = 0;
        }
        for (int64_t i = tid; i < (int64_t)P * kMotifK; i += NT) a.first[g * P * kMotifK + i] = -1;
        if (tid == 0) a.tgt_edges[g] = -1;
        return;
    }
    int64_t deg = 0;
    if (tid < n) deg = __popcll(adj[tid * 4]) + __popcll(adj[tid * 4 + 1]) + __popcll(adj[tid * 4 + 2]) + __popcll(adj[tid * 4 + 3]);
    deg = wg_sum<NT>(deg, red);
    if (tid == 0) a.tgt_edges[g] = deg >> 1;

    if (labelled && tid < kMotifN)                                    // (whole waves: NT >= kMotifN)
        for (int p = 0; p < P; ++p)
            for (int d = 0; d < plan[p].k; ++d) {
                const u64 b = __ballot(tid < n && tlab[tid] == plab[p][d]);
                if (lane == 0) lmask[p][d][wave] = b;
            }
    for (int p = 0; p < P; ++p)                                       // one node: the label-compatible nodes
        if (plan[p].k == 1 && tid < n && (!labelled || tlab[tid] == plab[p][0])) {
            atomicAdd(&acc[p][0], 1ull);
            atomicMin(&acc[p][2], ((u64)tid << 56) | (~0ull >> 8));
        }
    __syncthreads();

    // Items: a pattern and 16 cells of a row (one cell in a graph of at most 64 nodes, where every cell can have a lane of
    // its own), dealt pattern by pattern from one counter: a lane that is done with its pattern goes on with the next one.
    const u64 budget = (u64)a.budget;
    const int induced = a.induced;
    const int per = n > 64 ? 16 : n, cw = n > 64 ? 16 : 1;
    const int items = n * per, total = items * P;
    MotifPat q{0, 0, 0, 0};
    int pcur = -1, d = 0, u = 0, base = 0;                            // d = 0: no root in hand
    unsigned cells = 0;                                               // the set cells of this lane's item not yet taken
    u64 key = 0, cur = 0, steps = 0, blank = 0;                       // cur: bits [9 (d - 2), +9): where position d goes on
    u64 cnt = 0, trc = 0, best = ~0ull;                               // of pattern pcur, not yet in acc
    int sh0 = 0, sh1 = 0;
    for (;;) {
        if (d == 0) {
            if (cells == 0) {
                const int it = atomicAdd(&next_item, 1);
                const int pn = it < total ? it / items : P;           // P: the end (never pcur, which starts at -1)
                if (pn != pcur) {                                     // another pattern, or the end: hand in what was found
                    if (cnt) atomicAdd(&acc[pcur][0], cnt);
                    if (trc) atomicAdd(&acc[pcur][1], trc);
                    if (best != ~0ull) atomicMin(&acc[pcur][2], best);
                    cnt = trc = 0;
                    best = ~0ull;
                    if (pn == P) break;
                    pcur = pn;
                    q.order = plan[pn].order;
                    q.padj = plan[pn].padj;
                    q.parent = plan[pn].parent;
                    q.k = plan[pn].k;
                    blank = q.k < kMotifK ? ~0ull >> (8 * q.k) : 0ull;   // the bytes of the nodes k .. 7: 0xFF
                    sh0 = 56 - 8 * (int)(q.order & 0xFF);
                    sh1 = 56 - 8 * (int)((q.order >> 8) & 0xFF);
                }
                if (q.k < 2) continue;
                const int loc = it - pn * items;
                u = loc / per;
                base = (loc - u * per) * cw;
                cells = (unsigned)(adj[u * 4 + (base >> 6)] >> (base & 63)) & (cw == 16 ? 0xFFFFu : 1u);
                if (labelled && tlab[u] != plab[pcur][0]) cells = 0;
                continue;
            }
            const int w = base + __builtin_ctz(cells);
            cells &= cells - 1;
            if (labelled && tlab[w] != plab[pcur][1]) continue;
            key = blank | ((u64)u << sh0) | ((u64)w << sh1);          // the images, in pattern-node order
            if (q.k == 2) {
                ++cnt;
                best = key < best ? key : best;
                continue;
            }
            d = 2;
            cur = 0;
            steps = 0;
        }
        if (d == q.k - 1) {                                           // the last position: in one piece
            if (motif_last(adj, labelled ? lmask[pcur][d] : nullptr, q, induced, key, d, budget, steps, cnt, best)) {
                ++trc;
                d = 0;
            } else {
                d = d == 2 ? 0 : d - 1;
            }
            continue;
        }
        const int pd = (int)(q.parent >> (3 * d)) & 7;
        const int shp = 56 - 8 * (int)((q.order >> (8 * pd)) & 0xFF), shd = 56 - 8 * (int)((q.order >> (8 * d)) & 0xFF);
        const int cs = 9 * (d - 2);
        const int v = next_neighbour(adj, (int)(key >> shp) & 0xFF, (int)(cur >> cs) & 0x1FF);
        if (v >= kMotifN) {                                           // position d has no candidate left
            d = d == 2 ? 0 : d - 1;
            continue;
        }
        if (steps == budget) {                                        // this would be step budget + 1
            ++trc;
            d = 0;
            continue;
        }
        ++steps;
        cur = (cur & ~(0x1FFull << cs)) | ((u64)(v + 1) << cs);
        if (!motif_fits(adj, q, tlab, plab[pcur], labelled, induced, key, d, v)) continue;
        key = (key & ~(0xFFull << shd)) | ((u64)v << shd);
        ++d;
        cur &= ~(0x1FFull << (9 * (d - 2)));
    }
    __syncthreads();
    for (int p = tid; p < P; p += NT) {
        const u64 c = acc[p][0], b = acc[p][2];
        a.count[g * P + p] = (int64_t)c;
        a.trunc[g * P + p] = (int64_t)acc[p][1];
        for (int i = 0; i < kMotifK; ++i)
            a.first[(g * P + p) * kMotifK + i] = c && i < plan[p].k ? (int32_t)((b >> (56 - 8 * i)) & 0xFF) : -1;
    }
}

}  // namespace
}  // namespace cal

using namespace cal;

CAL_EXPORT int cal_motif_match(const int64_t* edge_index, int64_t E, int64_t N, const int64_t* ptr, const int64_t* edge_ptr,
                               int64_t B, const int64_t* labels, const int64_t* pat_edge_index, int64_t PE, int64_t PN,
                               const int64_t* pat_ptr, const int64_t* pat_edge_ptr, int64_t P, const int64_t* pat_labels,
                               int induced, int64_t budget, int64_t* count, int64_t* truncated, int32_t* first,
                               int64_t* tgt_edges, int64_t* pat_edges, int64_t* totals, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CAL_REQUIRE(E >= 0 && N >= 0 && B >= 0 && PE >= 0 && PN >= 0 && P >= 0, "E, N, B, PE, PN, P must be >= 0");
    CAL_REQUIRE(induced == 0 || induced == 1, "induced must be 0 or 1");
    CAL_REQUIRE(budget >= 0, "budget must be >= 0");
    CAL_REQUIRE(B <= 0x7FFFFFFF, "too many graphs");
    CAL_REQUIRE(P <= kMotifP, "more than CAL_MOTIF_MAX_PATTERNS patterns");
    CAL_REQUIRE((labels == nullptr) == (pat_labels == nullptr) || N == 0 || PN == 0, "labels and pat_labels go together");
    CAL_REQUIRE(totals, "totals is null");
    CAL_REQUIRE(P == 0 || (pat_ptr && pat_edge_ptr), "pat_ptr / pat_edge_ptr are null");
    CAL_REQUIRE(PE == 0 || pat_edge_index, "pat_edge_index is null");
    MotifArgs a{};
    for (int64_t p = 0; p < P; ++p) {
        const int64_t nlo = pat_ptr[p], nhi = pat_ptr[p + 1], elo = pat_edge_ptr[p], ehi = pat_edge_ptr[p + 1];
        CAL_REQUIRE(nlo >= 0 && nlo <= nhi && nhi <= PN && elo >= 0 && elo <= ehi && ehi <= PE, "pat_ptr / pat_edge_ptr are malformed");
        CAL_REQUIRE(motif_plan(pat_edge_index, PE, elo, ehi, nlo, nhi - nlo, a.plan[p]),
                    "a pattern must be connected and have 1 to CAL_MOTIF_MAX_PATTERN nodes");
    }
    if (hipMemsetAsync(totals, 0, sizeof(int64_t), stream) != hipSuccess) {
        set_error("cal_motif_match: hipMemsetAsync failed");
        return 1;
    }
    if (B == 0 || P == 0) return 0;
    CAL_REQUIRE(ptr && edge_ptr, "ptr / edge_ptr are null");
    CAL_REQUIRE(E == 0 || edge_index, "edge_index is null");
    CAL_REQUIRE(count && truncated && first && tgt_edges && pat_edges, "an output is null");
    const bool labelled = labels && pat_labels;
    a.ei = edge_index;
    a.E = E;
    a.N = N;
    a.ptr = ptr;
    a.eptr = edge_ptr;
    a.lab = labelled ? labels : nullptr;
    a.plab = labelled ? pat_labels : nullptr;
    a.P = P;
    a.budget = budget;
    a.induced = induced;
    a.count = count;
    a.trunc = truncated;
    a.first = first;
    a.tgt_edges = tgt_edges;
    a.pat_edges = pat_edges;
    a.totals = reinterpret_cast<u64*>(totals);
    hipLaunchKernelGGL(k_motif_match, dim3((unsigned)B), dim3(kMotifNT), 0, stream, a);
    CAL_CHECK_LAUNCH("k_motif_match");
    return 0;
}
