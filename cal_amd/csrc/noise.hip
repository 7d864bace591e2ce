// Structural-noise replicas: the device operator behind cal_amd/noise.py (noise curves, explanation stability), and the capped
// one-hot degree features of a batch.
//
// cal_noise_count / cal_noise_write: replica r is graph g = rep_graph[r] of the batch with a random subset of its edges deleted and
// random new edges inserted -- what SPMotif's own generator does under its `noise` knob, here on the device and with the pairing
// to the clean graph (edge_src) kept.  The full contract is in cal_hip.h; in short, with H(s, i) = splitmix64(splitmix64(s) + i):
//  * deletion: the player with representative column e_loc (inside g's segment) goes iff (H(seed ^ C_DEL, e_loc) >> 1) < rep_del[r];
//  * insertion: candidate c = 0 .. tries a - 1 is the pair (u, v) = ((h >> 32) mod n, (h & 0xffffffff) mod n), h = H(seed ^ C_ADD, c);
//    it is fresh iff u != v, the SOURCE graph has no such column and no earlier candidate is the same pair; the replica receives
//    the first a fresh candidates in candidate order, after its surviving source columns.
// Everything is integer: every output is uniquely determined.
//
// The two launches follow the protocol of rebatch.hpp.  What is particular here is the insertion, decided by the count launch,
// one workgroup per replica, candidates in chunks of one workgroup's threads:
//  * a pair is the key u n + v (directed) or min n + max (undirected, twin given).  A candidate passes when its key is neither a
//    source column's nor an accepted pair's; within the chunk a duplicate resolves to the smallest candidate index (every thread
//    compares its key with the chunk's keys in front of it, read from LDS as broadcasts); an ordered prefix count (wg_excl) over
//    the chunk's fresh candidates cuts at a.  The accepted pairs go to the replica's run of ws (int32 u, v; a pairs taken
//    from a counter in ws, the run's start kept in ws), where the write launch finds them; the loop ends as soon as a pairs are
//    accepted.
//  * source segments within kSegCap columns whose keys and accepted pairs fit the table (m + a <= kNoiseFill): an open-addressing
//    hash set of kNoiseSlots 64-bit keys in LDS (32 KB) holds the source keys and, chunk by chunk, the accepted ones.  Which slot
//    a key lands in depends on the order of the LDS atomics; whether a key is in the set does not.
//  * anything larger: every candidate of the chunk walks the segment's columns (all lanes read the same column: broadcast loads)
//    and the accepted run in ws.  Plain, and any size.
// No value that reaches an output is accumulated in an order-dependent way.
//
// cal_degree_onehot: three steps on the stream -- x_out is zeroed, the degree of node i is counted as an integer in the first
// slot of its row (integer atomics: the order cannot show), then every row is rewritten as the one-hot of min(d, F - 1).
#include "cal_hip.h"
#include "rebatch.hpp"

namespace cal {
namespace {

constexpr int kNoiseSlots = 4096;          // hash set slots (64-bit keys, 32 KB of LDS)
constexpr int kNoiseFill = 3072;           // keys it may hold: the load stays at or below 3 / 4
constexpr int64_t kNoisePairs = (int64_t)1 << 31;   // accepted pairs ws is taken to hold, at the most
constexpr uint64_t kNoKey = ~0ull;         // an empty slot; the key of a candidate that does not pass

struct NoArgs {
    const int64_t* ei;         // [2, E]
    int64_t E, N;
    const int64_t* ptr;        // [B + 1]
    const int64_t* eptr;       // [B + 1]
    int64_t B;
    const int32_t* twin;       // [E] or null (directed)
    const int64_t* rg;         // [R] graph of every replica (outside [0, B): none)
    const int64_t* rseed;      // [R]
    const int64_t* rdel;       // [R] deletion threshold
    const int64_t* radd;       // [R] insertions asked for
    int64_t R, tries;
    int64_t* added;            // [R] insertions made (count writes, write reads)
    int64_t* ptr_out;          // [R + 1]
    int64_t* eptr_out;         // [R + 1]
    int64_t* totals;           // [7]
    int64_t* cnt;              // ws [2 R]: nodes, columns of every replica
    int64_t* offs;             // ws [R]: where replica r's run of accepted pairs starts (count writes, write reads)
    unsigned long long* next;  // ws: the pairs handed out so far (zeroed in front of the count launch)
    int32_t* pairs;            // ws [2 cap]: accepted (u, v)
    int64_t cap;               // pairs ws holds
    const float* x;            // (write) [N, F] or null
    WriteOut out;              // (write)
    int ticket, nblk;
};

// (kNoiseDel, kNoiseAdd, noise_hash, NoRep, noise_replica, noise_stays, pair_key: rules.hpp)

__device__ __forceinline__ unsigned slot_of(uint64_t k) { return (unsigned)(splitmix64(k) & (kNoiseSlots - 1)); }

__device__ __forceinline__ void set_insert(unsigned long long* tab, uint64_t k) {
    unsigned s = slot_of(k);
    for (int i = 0; i < kNoiseSlots; ++i) {                       // (the fill bound keeps a slot free: the walk ends early)
        const unsigned long long old = atomicCAS(tab + s, (unsigned long long)kNoKey, (unsigned long long)k);
        if (old == kNoKey || old == k) return;
        s = (s + 1) & (kNoiseSlots - 1);
    }
}

__device__ __forceinline__ bool set_has(const unsigned long long* tab, uint64_t k) {
    unsigned s = slot_of(k);
    for (int i = 0; i < kNoiseSlots; ++i) {
        const unsigned long long cur = tab[s];
        if (cur == k) return true;
        if (cur == kNoKey) return false;
        s = (s + 1) & (kNoiseSlots - 1);
    }
    return false;
}

// grid R, NT threads
template <int NT>
__global__ void __launch_bounds__(NT) k_noise_count(NoArgs a) {
    __shared__ unsigned long long tab[kNoiseSlots];
    __shared__ unsigned long long ck[NT];
    __shared__ long long red[NT / 64];
    __shared__ int wcnt[NT / 64];
    __shared__ int last;
    __shared__ long long run;
    const int64_t r = blockIdx.x, R = a.R;
    const NoRep q = noise_replica(a, r);
    const bool und = a.twin != nullptr;
    // the replica's run of accepted pairs: a pairs from the counter.  Where a run lies depends on the order in which the
    // workgroups ask; what is written into it, and every output, does not.
    if (threadIdx.x == 0) {
        const bool asks = q.nn > 1 && q.a > 0;
        const unsigned long long ask = (unsigned long long)(q.a < kNoisePairs ? q.a : kNoisePairs);      // (R < 2^31: no overflow)
        run = asks ? (long long)atomicAdd(a.next, ask) : 0;
        a.offs[r] = run;
    }
    long long c = 0;
    for (int64_t t = threadIdx.x; t < q.em; t += NT) c += noise_stays(a, q, q.elo + t);
    const int64_t kept = wg_sum<NT>(c, red);

    // the insertions (everything below is uniform over the workgroup but the per-candidate values)
    const int64_t off = run;                                       // (wg_sum's barriers lie between the write and this read)
    const int64_t room = off < a.cap ? a.cap - off : 0;            // (ws holds the bound on the sum of the a: room >= a)
    const int64_t aeff = q.a < room ? q.a : room;                  // (a smaller ws: nothing is overrun, the walk stays bounded)
    const int64_t want = q.nn > 1 ? aeff : 0;
    const uint64_t n = (uint64_t)q.nn;
    const bool lds = q.em <= kSegCap && q.em + want <= kNoiseFill;
    int32_t* mine = a.pairs + 2 * off;
    int64_t acc = 0;
    if (want > 0) {
        if (lds) {
            for (int i = threadIdx.x; i < kNoiseSlots; i += NT) tab[i] = kNoKey;
            __syncthreads();
            for (int64_t t = threadIdx.x; t < q.em; t += NT) {
                const int64_t u = a.ei[q.elo + t] - q.nlo, v = a.ei[a.E + q.elo + t] - q.nlo;
                if (u >= 0 && u < q.nn && v >= 0 && v < q.nn && u != v) set_insert(tab, pair_key(und, (uint64_t)u, (uint64_t)v, n));
            }
            __syncthreads();
        }
        const unsigned long long total = (unsigned long long)a.tries * (unsigned long long)aeff;
        for (unsigned long long base = 0; base < total && acc < want; base += NT) {
            const unsigned long long cnd = base + threadIdx.x;
            uint64_t key = kNoKey;
            uint32_t u = 0, v = 0;
            if (cnd < total) {
                const unsigned long long h = noise_hash(q.seed ^ kNoiseAdd, cnd);
                u = (uint32_t)((h >> 32) % n);
                v = (uint32_t)((h & 0xffffffffull) % n);
                if (u != v) {
                    key = pair_key(und, u, v, n);
                    bool taken;
                    if (lds) {
                        taken = set_has(tab, key);
                    } else {
                        taken = false;
                        for (int64_t t = 0; t < q.em && !taken; ++t) {
                            const int64_t su = a.ei[q.elo + t] - q.nlo, sv = a.ei[a.E + q.elo + t] - q.nlo;
                            taken = su >= 0 && su < q.nn && sv >= 0 && sv < q.nn && su != sv &&
                                    pair_key(und, (uint64_t)su, (uint64_t)sv, n) == key;
                        }
                        for (int64_t t = 0; t < acc && !taken; ++t) {      // (written by this workgroup, chunks ago)
                            const int32_t pu = __hip_atomic_load(mine + 2 * t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                            const int32_t pv = __hip_atomic_load(mine + 2 * t + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                            taken = pair_key(und, (uint64_t)pu, (uint64_t)pv, n) == key;
                        }
                    }
                    if (taken) key = kNoKey;
                }
            }
            ck[threadIdx.x] = key;
            __syncthreads();
            bool fresh = key != kNoKey;
            for (int j = 0; j < (int)threadIdx.x && fresh; ++j) fresh = ck[j] != key;
            int tot;
            const int pos = wg_excl<NT>(fresh, wcnt, tot);
            const bool take = fresh && acc + pos < want;
            if (take) {
                mine[2 * (acc + pos)] = (int32_t)u;
                mine[2 * (acc + pos) + 1] = (int32_t)v;
                if (lds) set_insert(tab, key);
            }
            acc = acc + tot < want ? acc + tot : want;
            __syncthreads();                                       // (ck, the set and the accepted run before the next chunk)
        }
    }
    if (threadIdx.x == 0) {
        a.cnt[r] = q.nn;
        a.cnt[R + r] = kept + acc * (und ? 2 : 1);
        a.added[r] = acc;
    }
    if (!last_workgroup(a.ticket, a.nblk, &last)) return;
    scan_counts<NT>(a.cnt, a.cnt + R, R, a.ptr_out, a.eptr_out, a.totals, red);
    long long sa = 0, sh = 0;
    for (int64_t p = threadIdx.x; p < R; p += NT) {
        const long long ad = __hip_atomic_load(a.added + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int64_t w = a.radd[p];
        sa += ad;
        sh += ad < (w > 0 ? w : 0);
    }
    sa = wg_sum<NT>(sa, red);
    sh = wg_sum<NT>(sh, red);
    if (threadIdx.x == 0) {
        a.totals[5] = sa;
        a.totals[6] = sh;
    }
}

// grid ceil(Nout / kNodeChunk) node workgroups, then R column workgroups; 256 threads
__global__ void __launch_bounds__(256) k_noise_write(NoArgs a, int node_blocks) {
    __shared__ int64_t src[kNodeChunk];
    __shared__ int wcnt[4];
    if ((int)blockIdx.x < node_blocks) {
        write_nodes(
            a.out, a.ptr_out, a.R, -1, src,
            [&](int64_t r, int64_t l) -> int64_t {
                const NoRep q = noise_replica(a, r);
                return l < q.nn ? q.nlo + l : -1;
            },
            [&](int64_t s) { return a.x + s * a.out.F; });
        return;
    }
    const int64_t r = (int64_t)((int)blockIdx.x - node_blocks);
    const NoRep q = noise_replica(a, r);
    write_cols(
        a.out, a.ptr_out, a.eptr_out, r, a.ei, a.E, q.elo, q.em, wcnt, [&](int64_t e) { return noise_stays(a, q, e); },
        [&](int64_t u) { return u - q.nlo; });
    // the inserted columns: the end of the replica's run
    const int64_t off = a.offs[r] > 0 ? a.offs[r] : 0;
    const int w = a.twin ? 2 : 1;
    int64_t acc = a.added[r];
    const int64_t room = off < a.cap ? a.cap - off : 0, n0 = a.ptr_out[r], j1 = a.eptr_out[r + 1];
    acc = acc < 0 ? 0 : (acc < room ? acc : room);
    acc = acc * w <= j1 - a.eptr_out[r] ? acc : 0;                 // (an added[] changed since the count: nothing is overrun)
    const int32_t* mine = a.pairs + 2 * off;
    for (int64_t t = threadIdx.x; t < acc; t += 256) {
        const int64_t u = n0 + mine[2 * t], v = n0 + mine[2 * t + 1];
        for (int d = 0; d < w; ++d) {
            const int64_t j = j1 - (acc - t) * w + d;
            if (j >= 0 && j < a.out.Eout) {
                a.out.ei_out[j] = d ? v : u;
                a.out.ei_out[a.out.Eout + j] = d ? u : v;
                a.out.edge_src[j] = -1;
            }
        }
    }
}

constexpr int64_t kNoiseHead = 256;        // bytes of ws between the per-replica arrays and the pairs: the counter, slack

// cand bounds the sum of tries a, so ceil(cand / tries) bounds the pairs
int64_t noise_ws_need(int64_t R, int64_t cand, int64_t tries) {
    R = R > 0 ? R : 0;
    cand = cand > 0 ? cand : 0;
    tries = tries > 0 ? tries : 1;
    return 24 * R + kNoiseHead + 8 * ((cand + tries - 1) / tries);
}

#define NOISE_REQUIRE_INPUTS()                                                                                                   \
    CAL_REQUIRE(E >= 0 && N >= 0 && B >= 0 && R >= 0, "sizes must be >= 0");                                                     \
    CAL_REQUIRE(N < ((int64_t)1 << 31), "2^31 nodes or more are not supported (the accepted pairs are int32)");                  \
    CAL_REQUIRE(R <= 0x7FFFFFFF, "too many replicas");                                                                           \
    CAL_REQUIRE(tries >= 1 && tries <= (1 << 20), "tries must be in [1, 2^20]");                                                 \
    CAL_REQUIRE(R == 0 || (rep_graph && rep_seed && rep_del && rep_add && added), "rep_graph / rep_seed / rep_del / rep_add / added are null"); \
    CAL_REQUIRE(B == 0 || (ptr && edge_ptr), "ptr / edge_ptr are null");                                                         \
    CAL_REQUIRE(E == 0 || edge_index, "edge_index is null");                                                                     \
    CAL_REQUIRE(R == 0 || (ws && ws_bytes >= noise_ws_need(R, 0, 1) && (reinterpret_cast<uintptr_t>(ws) & 7) == 0),                 \
                "ws must be 8-byte aligned and hold cal_noise_ws(E, R, cand, tries) bytes")

NoArgs noise_args(const int64_t* edge_index, int64_t E, int64_t N, const int64_t* ptr, const int64_t* edge_ptr, int64_t B,
                  const int32_t* twin, const int64_t* rep_graph, const int64_t* rep_seed, const int64_t* rep_del,
                  const int64_t* rep_add, int64_t R, int64_t tries, int64_t* added, void* ws, int64_t ws_bytes) {
    NoArgs a{};
    a.ei = edge_index;
    a.E = E;
    a.N = N;
    a.ptr = ptr;
    a.eptr = edge_ptr;
    a.B = B;
    a.twin = E > 0 ? twin : nullptr;
    a.rg = rep_graph;
    a.rseed = rep_seed;
    a.rdel = rep_del;
    a.radd = rep_add;
    a.R = R;
    a.tries = tries;
    a.added = added;
    a.cnt = (int64_t*)ws;
    a.offs = (int64_t*)ws + 2 * R;
    a.next = reinterpret_cast<unsigned long long*>((int64_t*)ws + 3 * R);
    a.pairs = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(ws) + 24 * R + kNoiseHead);
    a.cap = (ws_bytes - 24 * R - kNoiseHead) / 8;
    a.cap = a.cap < kNoisePairs ? a.cap : kNoisePairs - 1;
    return a;
}

// grid ceil(E / 256): the degree of node u, counted in the first slot of its row
__global__ void __launch_bounds__(256) k_degree_count(const int64_t* ei, int64_t E, int64_t N, int64_t F, float* x_out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const int64_t u = ei[e], v = ei[E + e];
    if (u >= 0 && u < N && u != v) atomicAdd(reinterpret_cast<int*>(x_out + u * F), 1);
}

// grid ceil(N / 256): the row of node i becomes the one-hot of min(d, F - 1) (the other slots are zero already)
__global__ void __launch_bounds__(256) k_degree_onehot(int64_t N, int64_t F, float* x_out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    float* row = x_out + i * F;
    const int64_t d = *reinterpret_cast<const int*>(row);
    const int64_t c = d < F - 1 ? d : F - 1;
    row[0] = c == 0 ? 1.f : 0.f;
    if (c > 0) row[c] = 1.f;
}

}  // namespace
}  // namespace cal

using namespace cal;

CAL_EXPORT int64_t cal_noise_ws(int64_t, int64_t R, int64_t cand, int64_t tries) { return noise_ws_need(R, cand, tries); }

CAL_EXPORT int cal_noise_count(const int64_t* edge_index, int64_t E, int64_t N, const int64_t* ptr, const int64_t* edge_ptr,
                               int64_t B, const int32_t* twin, const int64_t* rep_graph, const int64_t* rep_seed,
                               const int64_t* rep_del, const int64_t* rep_add, int64_t R, int64_t tries, int64_t* added,
                               int64_t* ptr_out, int64_t* edge_ptr_out, int64_t* totals, void* ws, int64_t ws_bytes,
                               void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    NOISE_REQUIRE_INPUTS();
    CAL_REQUIRE(totals && ptr_out && edge_ptr_out, "totals / ptr_out / edge_ptr_out are null");
    if (R == 0) return zero_counts(__func__, totals, 7, ptr_out, edge_ptr_out, stream);
    NoArgs a = noise_args(edge_index, E, N, ptr, edge_ptr, B, twin, rep_graph, rep_seed, rep_del, rep_add, R, tries, added, ws,
                          ws_bytes);
    a.ptr_out = ptr_out;
    a.eptr_out = edge_ptr_out;
    a.totals = totals;
    a.ticket = next_ticket();
    a.nblk = (int)R;
    if (hipMemsetAsync(a.next, 0, sizeof(unsigned long long), stream) != hipSuccess) {
        set_error("cal_noise_count: hipMemsetAsync failed");
        return 1;
    }
    CAL_REBATCH_COUNT(k_noise_count, E / (B > 0 ? B : 1), R, stream, a);
    CAL_CHECK_LAUNCH("k_noise_count");
    return 0;
}

CAL_EXPORT int cal_noise_write(const int64_t* edge_index, int64_t E, int64_t N, const int64_t* ptr, const int64_t* edge_ptr,
                               int64_t B, const int32_t* twin, const int64_t* rep_graph, const int64_t* rep_seed,
                               const int64_t* rep_del, const int64_t* rep_add, int64_t R, int64_t tries, int64_t* added,
                               const float* x, int64_t F, const int64_t* ptr_out, const int64_t* edge_ptr_out, int64_t Nout,
                               int64_t Eout, int64_t* batch_out, float* x_out, int64_t* edge_index_out, int64_t* node_src,
                               int64_t* edge_src, void* ws, int64_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    NOISE_REQUIRE_INPUTS();
    CAL_REBATCH_REQUIRE_WRITE(R, !x_out || (F > 0 && (N == 0 || x)), "x_out needs F > 0 and x", Eout > 0 ? R : 0);
    if (R == 0 || nb + eb == 0) return 0;
    NoArgs a = noise_args(edge_index, E, N, ptr, edge_ptr, B, twin, rep_graph, rep_seed, rep_del, rep_add, R, tries, added, ws,
                          ws_bytes);
    a.x = x;
    a.ptr_out = const_cast<int64_t*>(ptr_out);
    a.eptr_out = const_cast<int64_t*>(edge_ptr_out);
    a.out = write_out(Nout, Eout, batch_out, x_out, edge_index_out, node_src, edge_src, F, x);
    hipLaunchKernelGGL(k_noise_write, dim3((unsigned)(nb + eb)), dim3(256), 0, stream, a, (int)nb);
    CAL_CHECK_LAUNCH("k_noise_write");
    return 0;
}

CAL_EXPORT int cal_degree_onehot(const int64_t* edge_index, int64_t E, int64_t N, int64_t F, float* x_out, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CAL_REQUIRE(E >= 0 && N >= 0, "E, N must be >= 0");
    CAL_REQUIRE(F >= 1 && F < (1 << 22), "F must be in [1, 2^22)");
    if (N == 0) return 0;
    CAL_REQUIRE(x_out, "x_out is null");
    CAL_REQUIRE(E == 0 || edge_index, "edge_index is null");
    CAL_REQUIRE((E + 255) / 256 <= 0x7FFFFFFF && (N + 255) / 256 <= 0x7FFFFFFF, "too many elements");
    if (hipMemsetAsync(x_out, 0, sizeof(float) * (size_t)N * (size_t)F, stream) != hipSuccess) {
        set_error("cal_degree_onehot: hipMemsetAsync failed");
        return 1;
    }
    if (E > 0) {
        hipLaunchKernelGGL(k_degree_count, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, stream, edge_index, E, N, F, x_out);
        CAL_CHECK_LAUNCH("k_degree_count");
    }
    hipLaunchKernelGGL(k_degree_onehot, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream, N, F, x_out);
    CAL_CHECK_LAUNCH("k_degree_onehot");
    return 0;
}
