// Graph centralities of every graph of a batch: hop distances (farness, reach, eccentricity, distance to a marked set), Brandes'
// node and edge betweenness and PageRank, the device operator behind cal_amd/centrality.py.  The contract -- graph semantics, the
// outputs, the order of every floating-point sum -- is in cal_hip.h; the rules shared with the host twin are in rules.hpp.
//
// cal_centrality, k_centrality: one workgroup of 256 threads (kCentW = 4 waves) per graph of at most 256 nodes.
//  * the adjacency is motif.hip's 256 x 256 bit matrix in LDS (8 KB), built with 64-bit LDS OR-atomics.
//  * a wave owns the sources s = wave (mod 4), in ascending s, and runs Brandes' algorithm for one source at a time ALONE: it
//    meets the other waves at a workgroup barrier only when all its sources are done.  sigma, q = (1 + delta) / sigma and the hop
//    distances of the current source live in the wave's own 5 KB of LDS.
//  * a lane owns the nodes lane + 64 j, j = 0 .. 3, and keeps their rows (16 words), distances, sigma and delta in registers, so
//    __ballot over the wave IS word j of a frontier or a level mask: a level step is the AND of a node's row with the frontier
//    and a count-trailing-zeros walk over the result for the pull sum, in ascending neighbour id.  The levels are not stored: the
//    backward pass makes level L's mask again with a ballot of (dist == L).
//  * what one lane writes to LDS and another lane of the wave reads (sigma, q, dist) is ordered with wave_sync(): a wavefront-scope
//    fence, so that the compiler keeps the accesses in program order, and the wave barrier.
//  * farness, reach and eccentricity use the symmetry d(s, v) = d(v, s): a lane adds what its nodes see over the wave's sources, in
//    registers; betweenness the same way.  Edge betweenness: after a source's backward pass the lanes walk the graph's columns
//    and add the column's term to the WAVE's partial -- in LDS for a graph of at most kCentCap columns, in the workspace above.
//    A column belongs to the lane (column mod 64) every time, so nobody else touches its partial.
//  * at the end the four partials are added in wave order.  No floating-point atomic anywhere: two runs give the same bits.
//  * PageRank runs after the barrier on all 256 threads, thread t = node t, one barrier per iteration; the dangling mass and the
//    L1 change are the tree sum of rules.hpp (cent_tree_sum).
//  * the distance to the marked nodes (hop) is one more search without sigma, by wave 0.
#include "cal_hip.h"
#include "segment.hpp"

namespace cal {
namespace {

typedef unsigned long long u64;

constexpr int kCentNT = 64 * kCentW;                 // threads of a workgroup
constexpr int kCentN = CAL_MOTIF_MAX_NODES;
constexpr int kCentCap = CAL_CENTRALITY_LDS_COLS;    // columns whose per-wave partials (and local ends) fit in LDS
constexpr uint32_t kColNone = 0xFFFFFFFFu;           // a column that leaves its graph
static_assert(kCentNT == kCentN && kCentN == kCentSlots, "thread t is node t in the PageRank phase, one slot of the tree sum");

struct CentArgs {
    const int64_t* ei;         // [2, E]
    int64_t E, N;
    const int64_t* ptr;        // [B + 1]
    const int64_t* eptr;       // [B + 1]
    const uint8_t* src;        // [N] or null
    double alpha, tol;
    int64_t max_iter;
    int64_t *far, *reach, *ecc, *deg;   // [N]
    double *bc, *ebc, *pr;
    int32_t* pr_iters;         // [B]; null: only hop is wanted
    int32_t* hop;              // [N] or null
    int64_t* skipped;          // [B]
    u64* totals;               // [1]
    double* ws;                // [kCentW, E] or null
};

// what one lane of a wave wrote to LDS, another lane of the SAME wave may read after this
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the tree sum of the 256 slots of r (cent_tree_sum); every lane of every wave gets the same bits
__device__ __forceinline__ double tree_sum(const double* r, int lane) {
    double s = (r[lane] + r[lane + 128]) + (r[lane + 64] + r[lane + 192]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    return s;
}

// grid B, kCentNT threads
__global__ void __launch_bounds__(kCentNT) k_centrality(CentArgs a) {
    __shared__ u64 adj[kCentN * 4];
    __shared__ double sig[kCentW][kCentN];
    __shared__ double qv[kCentW][kCentN];
    __shared__ int dist[kCentW][kCentN];
    __shared__ double part[kCentW][kCentCap];
    __shared__ uint32_t cols[kCentCap];
    __shared__ long long red[kCentW];
    constexpr int NT = kCentNT;
    const int64_t g = blockIdx.x, N = a.N, E = a.E;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool cent = a.pr_iters != nullptr, hopw = a.hop != nullptr;
    int64_t nlo, n64, elo, m;
    seg_clamp(a.ptr, g, N, nlo, n64);
    seg_clamp(a.eptr, g, E, elo, m);
    const bool skip = n64 > kCentN;                                   // (uniform)
    const int n = skip ? 0 : (int)n64;
    const bool inl = m <= kCentCap;                                   // the columns' ends and partials are in LDS
    for (int i = tid; i < kCentN * 4; i += NT) adj[i] = 0;
    __syncthreads();
    int64_t ign = 0;
    for (int64_t e = tid; e < m; e += NT) {
        const int64_t u = a.ei[elo + e] - nlo, v = a.ei[E + elo + e] - nlo;
        const bool out = !(u >= 0 && u < n64 && v >= 0 && v < n64);
        if (out) {
            ++ign;
        } else if (!skip && u != v) {
            atomicOr(&adj[(int)u * 4 + ((int)v >> 6)], 1ull << ((int)v & 63));
            atomicOr(&adj[(int)v * 4 + ((int)u >> 6)], 1ull << ((int)u & 63));
        }
        if (inl && !skip) cols[e] = out ? kColNone : (uint32_t)u | ((uint32_t)v << 16);
    }
    ign = wg_sum<NT>(ign, red);                                       // (its barriers publish the matrix and the columns)
    if (tid == 0) {
        if (ign) atomicAdd(a.totals, (u64)ign);
        a.skipped[g] = skip ? 1 : 0;
    }
    if (skip) {
        const double nan = cent_skip_f64();
        for (int64_t i = tid; i < n64; i += NT) {
            if (cent) {
                a.far[nlo + i] = a.reach[nlo + i] = a.ecc[nlo + i] = a.deg[nlo + i] = kCentSkipInt;
                a.bc[nlo + i] = a.pr[nlo + i] = nan;
            }
            if (hopw) a.hop[nlo + i] = (int32_t)kCentSkipInt;
        }
        if (cent) {
            for (int64_t e = tid; e < m; e += NT) a.ebc[elo + e] = nan;
            if (tid == 0) a.pr_iters[g] = (int32_t)kCentSkipInt;
        }
        return;
    }
    const int nw = (n + 63) >> 6;                                     // words of a row, of a mask; nodes per lane

    // this lane's rows: node lane + 64 j (zero beyond the graph)
    u64 row[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int w = 0; w < 4; ++w) row[j][w] = adj[(lane + 64 * j) * 4 + w];

    // ---- the distance to the marked nodes: wave 0, levels by ballots
    if (hopw && wave == 0) {
        int d[4];
        u64 F[4] = {0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int v = lane + 64 * j;
            const bool mk = j < nw && v < n && a.src && a.src[nlo + v] != 0;
            d[j] = mk ? kCentHopSeed : kCentUnreached;
            F[j] = __ballot(mk);
        }
        for (int L = kCentHopSeed;; ++L) {
            u64 NF[4] = {0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                bool hit = false;
                if (j < nw && d[j] == kCentUnreached)
                    hit = ((row[j][0] & F[0]) | (row[j][1] & F[1]) | (row[j][2] & F[2]) | (row[j][3] & F[3])) != 0;
                if (hit) d[j] = L + 1;
                NF[j] = __ballot(hit);
            }
            if (!(NF[0] | NF[1] | NF[2] | NF[3])) break;
#pragma unroll
            for (int j = 0; j < 4; ++j) F[j] = NF[j];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (lane + 64 * j < n) a.hop[nlo + lane + 64 * j] = d[j];
    }
    if (!cent) return;

    // ---- Brandes, one source at a time per wave
    double* const sg = sig[wave];
    double* const qq = qv[wave];
    int* const ds = dist[wave];
    double* const wpart = inl ? part[wave] : a.ws + (int64_t)wave * E + elo;
    for (int64_t e = lane; e < m; e += 64) wpart[e] = 0.0;            // (column e is this lane's every time)
    int64_t farv[4] = {0, 0, 0, 0};
    int reachv[4] = {0, 0, 0, 0}, eccv[4] = {0, 0, 0, 0};
    double bcv[4] = {0.0, 0.0, 0.0, 0.0};
    for (int s = wave; s < n; s += kCentW) {
        int d[4];
        double sv[4], dl[4];
        u64 F[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int v = lane + 64 * j;
            F[j] = (s >> 6) == j ? 1ull << (s & 63) : 0ull;
            d[j] = v == s ? 0 : kCentUnreached;
            sv[j] = v == s ? 1.0 : 0.0;
            dl[j] = 0.0;
            if (j < nw) {
                sg[v] = sv[j];
                ds[v] = d[j];
            }
        }
        wave_sync();
        int maxL = 0;
        for (;;) {                                                    // forward: level maxL -> maxL + 1
            u64 NF[4] = {0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                bool hit = false;
                if (j < nw && d[j] == kCentUnreached) {
                    double sum = 0.0;
#pragma unroll
                    for (int w = 0; w < 4; ++w) {
                        u64 mm = row[j][w] & F[w];
                        while (mm) {
                            sum += sg[w * 64 + __builtin_ctzll(mm)];
                            mm &= mm - 1;
                            hit = true;
                        }
                    }
                    if (hit) {
                        d[j] = maxL + 1;
                        sv[j] = sum;
                        sg[lane + 64 * j] = sum;                      // (an unreached node: nobody reads it in this level)
                        ds[lane + 64 * j] = maxL + 1;
                    }
                }
                NF[j] = __ballot(hit);
            }
            wave_sync();
            if (!(NF[0] | NF[1] | NF[2] | NF[3])) break;
#pragma unroll
            for (int j = 0; j < 4; ++j) F[j] = NF[j];
            ++maxL;
        }
        for (int lev = maxL; lev >= 1; --lev) {                       // backward: level lev pulls from level lev + 1
            u64 M[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) M[j] = __ballot(d[j] == lev + 1);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j < nw && d[j] == lev) {
                    double acc = 0.0;
#pragma unroll
                    for (int w = 0; w < 4; ++w) {
                        u64 mm = row[j][w] & M[w];
                        while (mm) {
                            acc += sv[j] * qq[w * 64 + __builtin_ctzll(mm)];
                            mm &= mm - 1;
                        }
                    }
                    dl[j] = acc;
                    qq[lane + 64 * j] = cent_q(acc, sv[j]);
                }
            }
            wave_sync();
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (d[j] >= 0) {                                          // (the source itself: distance 0, no delta)
                farv[j] += d[j];
                reachv[j] += 1;
                eccv[j] = d[j] > eccv[j] ? d[j] : eccv[j];
                if (d[j] > 0) bcv[j] += dl[j];
            }
        for (int64_t e = lane; e < m; e += 64) {                      // the columns' terms of this source
            uint32_t c;
            if (inl) {
                c = cols[e];
            } else {
                const int64_t u = a.ei[elo + e] - nlo, v = a.ei[E + elo + e] - nlo;
                c = (u >= 0 && u < n && v >= 0 && v < n) ? (uint32_t)u | ((uint32_t)v << 16) : kColNone;
            }
            if (c == kColNone) continue;
            const int x = (int)(c & 0xFFFFu), y = (int)(c >> 16);
            const int dx = ds[x], dy = ds[y];
            if (dx >= 0 && dy == dx + 1) wpart[e] += sg[x] * qq[y];
            else if (dy >= 0 && dx == dy + 1) wpart[e] += sg[y] * qq[x];
        }
        wave_sync();                                                  // (the next source overwrites sigma, q, dist)
    }
    __syncthreads();

    // ---- the waves' partials, in wave order.  sig / qv / dist are free now: wave w leaves its nodes' sums in its own rows.
    u64* const ipk = reinterpret_cast<u64*>(qv[wave]);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int v = lane + 64 * j;
        sg[v] = bcv[j];
        ipk[v] = (u64)farv[j] | ((u64)reachv[j] << 32);
        ds[v] = eccv[j];
    }
    if (!inl) __threadfence_block();                                  // (the other waves' partials in the workspace)
    __syncthreads();
    if (tid < n) {
        a.bc[nlo + tid] = cent_join(sig[0][tid], sig[1][tid], sig[2][tid], sig[3][tid]);
        u64 pk = 0;
        int ec = 0;
#pragma unroll
        for (int w = 0; w < kCentW; ++w) {
            pk += reinterpret_cast<const u64*>(qv[w])[tid];
            ec = dist[w][tid] > ec ? dist[w][tid] : ec;
        }
        a.far[nlo + tid] = (int64_t)(pk & 0xFFFFFFFFull);
        a.reach[nlo + tid] = (int64_t)(pk >> 32);
        a.ecc[nlo + tid] = ec;
    }
    for (int64_t e = tid; e < m; e += NT) {
        if (inl) {
            a.ebc[elo + e] = cent_join(part[0][e], part[1][e], part[2][e], part[3][e]);
        } else {
            const double* p = a.ws + elo + e;
            a.ebc[elo + e] = cent_join(p[0], p[E], p[2 * E], p[3 * E]);
        }
    }
    __syncthreads();

    // ---- PageRank: thread t is node t.  pxd: x / deg, two buffers; rs[parity][0 / 1]: |x_new - x|, the dangling x.
    double(*const pxd)[kCentN] = sig;                                 // [2][256]
    double(*const rs)[kCentN] = qv;                                   // [4][256]: rs[2 * parity + kind]
    const bool in = tid < n;
    u64 r4[4];
#pragma unroll
    for (int w = 0; w < 4; ++w) r4[w] = adj[tid * 4 + w];
    const int deg = __popcll(r4[0]) + __popcll(r4[1]) + __popcll(r4[2]) + __popcll(r4[3]);
    const double dn = (double)n, degd = (double)deg;
    double x = in ? 1.0 / dn : 0.0;
    pxd[0][tid] = in && deg ? x / degd : 0.0;
    rs[3][tid] = in && !deg ? x : 0.0;
    __syncthreads();
    double dsum = tree_sum(rs[3], lane);
    int it = 0;
    for (int par = 0; it < a.max_iter && n > 0; par ^= 1) {
        double pull = 0.0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            u64 mm = r4[w];
            while (mm) {
                pull += pxd[par][w * 64 + __builtin_ctzll(mm)];
                mm &= mm - 1;
            }
        }
        const double xn = in ? cent_pr_step(a.alpha, pull, dsum, dn) : 0.0;
        pxd[par ^ 1][tid] = in && deg ? xn / degd : 0.0;
        rs[2 * par][tid] = fabs(xn - x);
        rs[2 * par + 1][tid] = in && !deg ? xn : 0.0;
        x = xn;
        __syncthreads();
        const double err = tree_sum(rs[2 * par], lane);
        dsum = tree_sum(rs[2 * par + 1], lane);
        ++it;
        if (cent_pr_done(err, a.tol)) break;                          // (the same bits in every lane: uniform)
    }
    if (in) {
        a.pr[nlo + tid] = x;
        a.deg[nlo + tid] = deg;
    }
    if (tid == 0) a.pr_iters[g] = it;
}

}  // namespace
}  // namespace cal

using namespace cal;

CAL_EXPORT int64_t cal_centrality_ws(int64_t E) {
    return E > kCentCap ? (int64_t)kCentW * E * (int64_t)sizeof(double) : 0;
}

CAL_EXPORT int cal_centrality(const int64_t* edge_index, int64_t E, int64_t N, const int64_t* ptr, const int64_t* edge_ptr,
                              int64_t B, const uint8_t* sources, double alpha, double tol, int64_t max_iter, int64_t* far,
                              int64_t* reach, int64_t* ecc, int64_t* deg, double* bc, double* ebc, double* pr, int32_t* pr_iters,
                              int32_t* hop, int64_t* skipped, int64_t* totals, void* ws, int64_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CAL_REQUIRE(E >= 0 && N >= 0 && B >= 0, "E, N, B must be >= 0");
    CAL_REQUIRE(B <= 0x7FFFFFFF, "too many graphs");
    CAL_REQUIRE(alpha >= 0.0 && alpha < 1.0, "alpha must be in [0, 1)");
    CAL_REQUIRE(tol >= 0.0 && max_iter >= 0 && max_iter <= 0x7FFFFFFF, "tol must be >= 0 and max_iter in [0, 2^31)");
    CAL_REQUIRE(totals, "totals is null");
    CAL_REQUIRE(!hop || sources || N == 0, "hop needs sources");
    if (hipMemsetAsync(totals, 0, sizeof(int64_t), stream) != hipSuccess) {
        set_error("cal_centrality: hipMemsetAsync failed");
        return 1;
    }
    if (B == 0) return 0;
    const bool cent = pr_iters != nullptr;
    CAL_REQUIRE(!cent || ((N == 0 || (far && reach && ecc && deg && bc && pr)) && (E == 0 || ebc)),
                "pr_iters is given: far, reach, ecc, deg, bc, ebc and pr must be");
    CAL_REQUIRE(cent || hop || N == 0, "nothing is asked for");
    CAL_REQUIRE(ptr && edge_ptr && skipped, "ptr / edge_ptr / skipped are null");
    CAL_REQUIRE(E == 0 || edge_index, "edge_index is null");
    const int64_t need = cent ? cal_centrality_ws(E) : 0;
    CAL_REQUIRE(need == 0 || (ws && ws_bytes >= need), "ws is smaller than cal_centrality_ws(E)");
    CentArgs a{};
    a.ei = edge_index;
    a.E = E;
    a.N = N;
    a.ptr = ptr;
    a.eptr = edge_ptr;
    a.src = sources;
    a.alpha = alpha;
    a.tol = tol;
    a.max_iter = max_iter;
    a.far = far;
    a.reach = reach;
    a.ecc = ecc;
    a.deg = deg;
    a.bc = bc;
    a.ebc = ebc;
    a.pr = pr;
    a.pr_iters = pr_iters;
    a.hop = hop;
    a.skipped = skipped;
    a.totals = reinterpret_cast<u64*>(totals);
    a.ws = need ? static_cast<double*>(ws) : nullptr;
    hipLaunchKernelGGL(k_centrality, dim3((unsigned)B), dim3(kCentNT), 0, stream, a);
    CAL_CHECK_LAUNCH("k_centrality");
    return 0;
}
