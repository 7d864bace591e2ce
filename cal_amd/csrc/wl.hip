// Weisfeiler-Lehman colour refinement of a batch of graphs and the WL subtree kernel of two batches: the device operators
// behind cal_amd/wl.py (wl_refine, wl_match; the shape census of explanations).  The contract is in cal_hip.h; in short, with
// sm = splitmix64 and everything mod 2^64:
//   c_0[v] = sm(init[v] ^ C_INIT),  c_t[v] = sm(sm(sm(c_{t-1}[v] + C_SELF) + out[v]) + in[v]),
//   out[v] / in[v] the sums of sm(c_{t-1}[w] ^ C_OUT) / sm(c_{t-1}[w] ^ C_IN) over the counted columns (v, w) / (w, v),
//   hash[g, t] = h_t,  h_t = sm(h_{t-1} + sum_v sm(c_t[v] ^ C_NODE)),  h_{-1} = sm(n_g ^ C_GRAPH).
// Integers only: this file has no floating point.
//
// cal_wl_refine, k_wl_refine: one workgroup per graph runs all T rounds.
//  * a graph of at most CAP nodes: the colours of the round before, the colours being made and the two sum arrays in LDS
//    (4 x 8 CAP bytes: 64 KB at CAP = kSegCap).  Every array holds one 64-bit word per node, thread i on word i, i + NT, ..:
//    consecutive lanes on consecutive 8-byte words, no bank conflict but the scatter of the sums.  A round streams the graph's
//    columns from global memory (after the first round: from L2) and adds the two hashed neighbour colours with 64-bit LDS
//    atomics -- integer sums commute, so their order cannot show; a hub's columns queue up on one word and stay exact.
//  * a larger graph (only with max_nodes above the cap): the same rounds with row t - 1 of colors as the colours and two [N]
//    arrays of ws as the sums, every access to the sums an agent-scope atomic (they are formed in L2: a plain load could
//    be served by the CU's vector cache).
// The ignored columns are counted per graph and added to totals[0] (zeroed by a memset in front of the launch).
// Two instantiations, chosen by the host-known max_nodes: <256, 256> (8 KB, several workgroups per CU) and <1024, kSegCap>.
//
// cal_wl_match, k_wl_match: one workgroup per graph a of A, depth by depth.
//  * n_a <= CAP: the colours go to LDS, every thread counts for its colours how many are smaller / equal / equal and in
//    front (the row read as broadcasts, as twin.hip does) and writes each to its place in the sorted row.  A colour's count
//    is then the length of its run [first >= c, first > c) -- two binary searches (first_false) -- so wave w takes the
//    prototypes w, w + NW, ..: every lane looks up nodes of the prototype, the wave sums.  self_a is the sum over the nodes
//    of the count of their own colour.
//  * above the cap: every pair is compared, colours read from global memory.
// No atomics.
#include "cal_hip.h"
#include "segment.hpp"

namespace cal {
namespace {

constexpr int64_t kWlMaxT = 4096;
constexpr int64_t kWlMaxProtoNodes = 4096;
constexpr int kWlSmall = 256;              // nodes (and threads) of the small instantiation

typedef unsigned long long u64;

// sum mod 2^64 over the workgroup's NT threads, every thread gets it (two barriers).  wg_sum of segment.hpp adds signed
// words, which must not wrap; these sums do.
template <int NT>
__device__ __forceinline__ u64 wl_total(u64 v, u64* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    u64 t = 0;
#pragma unroll
    for (int i = 0; i < NT / 64; ++i) t += red[i];
    return t;
}

struct WlArgs {
    const int64_t* ei;         // [2, E]
    int64_t E, N;
    const int64_t* ptr;        // [B + 1]
    const int64_t* eptr;       // [B + 1]
    int64_t B;
    const int64_t* init;       // [N] or null
    int64_t T, max_nodes;
    u64* colors;               // [T + 1, N]
    u64* hash;                 // [B, T + 1]
    u64* totals;               // [1]
    u64* wout;                 // ws [N]  (graphs above the cap)
    u64* win;                  // ws [N]
};

// grid B, NT threads
template <int NT, int CAP>
__global__ void __launch_bounds__(NT) k_wl_refine(WlArgs a) {
    __shared__ u64 col[2][CAP];
    __shared__ u64 so[CAP];
    __shared__ u64 si[CAP];
    __shared__ u64 red[NT / 64];
    const int64_t g = blockIdx.x, N = a.N, E = a.E, T = a.T;
    int64_t nlo, n, elo, m;
    seg_clamp(a.ptr, g, N, nlo, n);
    seg_clamp(a.eptr, g, E, elo, m);

    u64 ign = 0;
    for (int64_t e = threadIdx.x; e < m; e += NT) {
        const int64_t u = a.ei[elo + e] - nlo, v = a.ei[E + elo + e] - nlo;
        ign += !(u >= 0 && u < n && v >= 0 && v < n);
    }
    ign = wl_total<NT>(ign, red);
    if (threadIdx.x == 0 && ign) atomicAdd(a.totals, ign);

    u64* hrow = a.hash + g * (T + 1);
    if (n > a.max_nodes) {                                         // (uniform) not worked on: zeros
        for (int64_t t = threadIdx.x; t <= T; t += NT) hrow[t] = 0;
        for (int64_t t = 0; t <= T; ++t)
            for (int64_t v = threadIdx.x; v < n; v += NT) a.colors[t * N + nlo + v] = 0;
        return;
    }
    const bool lds = n <= CAP;                                     // (uniform)
    for (int64_t v = threadIdx.x; v < n; v += NT) {
        const u64 c = splitmix64((a.init ? (u64)a.init[nlo + v] : 0ull) ^ kWlInit);
        a.colors[nlo + v] = c;
        if (lds) {
            col[0][v] = c;
            so[v] = 0;
            si[v] = 0;
        } else {
            __hip_atomic_store(a.wout + nlo + v, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(a.win + nlo + v, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    u64 h = splitmix64((u64)n ^ kWlGraph);
    int b = 0;                                                     // col[b]: the colours of depth t
    for (int64_t t = 0;; ++t) {
        const u64* crow = a.colors + t * N + nlo;                  // the same colours in global memory
        // every thread reads back the colours it wrote itself; wl_total's barriers then publish them and the zeroed sums
        u64 s = 0;
        for (int64_t v = threadIdx.x; v < n; v += NT) s += splitmix64((lds ? col[b][v] : crow[v]) ^ kWlNode);
        s = wl_total<NT>(s, red);
        h = splitmix64(h + s);
        if (threadIdx.x == 0) hrow[t] = h;
        if (t == T) break;
        for (int64_t e = threadIdx.x; e < m; e += NT) {
            const int64_t u = a.ei[elo + e] - nlo, v = a.ei[E + elo + e] - nlo;
            if (!(u >= 0 && u < n && v >= 0 && v < n)) continue;
            if (lds) {
                atomicAdd(&so[u], splitmix64(col[b][v] ^ kWlOut));
                atomicAdd(&si[v], splitmix64(col[b][u] ^ kWlIn));
            } else {
                atomicAdd(a.wout + nlo + u, splitmix64(crow[v] ^ kWlOut));
                atomicAdd(a.win + nlo + v, splitmix64(crow[u] ^ kWlIn));
            }
        }
        __syncthreads();
        u64* nrow = a.colors + (t + 1) * N + nlo;
        for (int64_t v = threadIdx.x; v < n; v += NT) {
            u64 c;
            if (lds) {
                c = wl_next(col[b][v], so[v], si[v]);
                col[b ^ 1][v] = c;
                so[v] = 0;
                si[v] = 0;
            } else {
                c = wl_next(crow[v], __hip_atomic_load(a.wout + nlo + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                            __hip_atomic_load(a.win + nlo + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
                __hip_atomic_store(a.wout + nlo + v, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(a.win + nlo + v, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            nrow[v] = c;
        }
        b ^= 1;
    }
}

struct WmArgs {
    const u64* ca;             // colours of A: row t at ca + t sa
    int64_t sa, Na;
    const int64_t* pa;         // [A + 1]
    int64_t A;
    const u64* cp;             // colours of P
    int64_t sp, Np;
    const int64_t* pp;         // [P + 1]
    int64_t P, T, max_nodes;
    int64_t* K;                // [A, P, T + 1]
    int64_t* self;             // [A, T + 1]
};

// grid A, NT threads
template <int NT, int CAP>
__global__ void __launch_bounds__(NT) k_wl_match(WmArgs a) {
    __shared__ __align__(16) u64 key[CAP];
    __shared__ __align__(16) u64 srt[CAP];
    __shared__ u64 red[NT / 64];
    constexpr int NW = NT / 64;
    const int64_t g = blockIdx.x, P = a.P, T = a.T;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t lo, n;
    seg_clamp(a.pa, g, a.Na, lo, n);
    if (n > a.max_nodes) {                                         // (uniform) not worked on: zeros
        for (int64_t i = threadIdx.x; i < P * (T + 1); i += NT) a.K[g * P * (T + 1) + i] = 0;
        for (int64_t t = threadIdx.x; t <= T; t += NT) a.self[g * (T + 1) + t] = 0;
        return;
    }
    const bool lds = n <= CAP;                                     // (uniform)
    for (int64_t t = 0; t <= T; ++t) {
        const u64* row = a.ca + t * a.sa + lo;
        const u64* prow = a.cp + t * a.sp;
        u64 own = 0;                                               // sum over this thread's nodes of the count of their colour
        if (lds) {
            const int nn = (int)n;
            for (int v = threadIdx.x; v < nn; v += NT) key[v] = row[v];
            __syncthreads();
            for (int v = threadIdx.x; v < nn; v += NT) {
                const u64 k = key[v];
                int ltc = 0, eqc = 0, eqb = 0;
                for (int j = 0; j < nn; ++j) {                     // (every lane the same word: a broadcast)
                    const u64 kj = key[j];
                    ltc += kj < k;
                    eqc += kj == k;
                    eqb += (kj == k) & (j < v);
                }
                srt[ltc + eqb] = k;
                own += (u64)eqc;
            }
            __syncthreads();
        } else {
            for (int64_t v = threadIdx.x; v < n; v += NT) {
                const u64 k = row[v];
                for (int64_t j = 0; j < n; ++j) own += row[j] == k;
            }
        }
        for (int64_t p = wave; p < P; p += NW) {
            int64_t plo, pn;
            seg_clamp(a.pp, p, a.Np, plo, pn);
            long long cnt = 0;
            for (int64_t w = lane; w < pn; w += 64) {
                const u64 c = prow[plo + w];
                if (lds) {
                    const int nn = (int)n;
                    cnt += first_false(srt, nn, [c](u64 x) { return x <= c; }) - first_false(srt, nn, [c](u64 x) { return x < c; });
                } else {
                    for (int64_t j = 0; j < n; ++j) cnt += row[j] == c;
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
            if (lane == 0) a.K[(g * P + p) * (T + 1) + t] = cnt;
        }
        own = wl_total<NT>(own, red);                              // (its barriers: the rows are free for the next depth)
        if (threadIdx.x == 0) a.self[g * (T + 1) + t] = (int64_t)own;
    }
}

int64_t wl_ws_need(int64_t N) { return 16 * (N > 0 ? N : 0) + 16; }

}  // namespace
}  // namespace cal

using namespace cal;

CAL_EXPORT int64_t cal_wl_ws(int64_t N, int64_t, int64_t) { return wl_ws_need(N); }

CAL_EXPORT int cal_wl_refine(const int64_t* edge_index, int64_t E, int64_t N, const int64_t* ptr, const int64_t* edge_ptr,
                             int64_t B, const int64_t* init, int64_t T, int64_t max_nodes, int64_t* colors, int64_t* hash,
                             int64_t* totals, void* ws, int64_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CAL_REQUIRE(E >= 0 && N >= 0 && B >= 0 && max_nodes >= 0, "E, N, B, max_nodes must be >= 0");
    CAL_REQUIRE(T >= 0 && T <= kWlMaxT, "T must be in [0, 4096]");
    CAL_REQUIRE(B <= 0x7FFFFFFF, "too many graphs");
    CAL_REQUIRE(totals, "totals is null");
    if (hipMemsetAsync(totals, 0, sizeof(int64_t), stream) != hipSuccess) {
        set_error("cal_wl_refine: hipMemsetAsync failed");
        return 1;
    }
    if (B == 0) return 0;
    CAL_REQUIRE(ptr && edge_ptr && hash, "ptr / edge_ptr / hash are null");
    CAL_REQUIRE(E == 0 || edge_index, "edge_index is null");
    CAL_REQUIRE(N == 0 || colors, "colors is null");
    const bool large = max_nodes > kSegCap;
    CAL_REQUIRE(!large || (ws && ws_bytes >= wl_ws_need(N) && (reinterpret_cast<uintptr_t>(ws) & 7) == 0),
                "ws must be 8-byte aligned and hold cal_wl_ws(N, E, B) bytes");
    WlArgs a{edge_index, E, N, ptr, edge_ptr, B, init, T, max_nodes, reinterpret_cast<u64*>(colors), reinterpret_cast<u64*>(hash),
             reinterpret_cast<u64*>(totals), large ? (u64*)ws : nullptr, large ? (u64*)ws + N : nullptr};
    if (max_nodes <= kWlSmall)
        hipLaunchKernelGGL((k_wl_refine<kWlSmall, kWlSmall>), dim3((unsigned)B), dim3(kWlSmall), 0, stream, a);
    else
        hipLaunchKernelGGL((k_wl_refine<kSegWide, kSegCap>), dim3((unsigned)B), dim3(kSegWide), 0, stream, a);
    CAL_CHECK_LAUNCH("k_wl_refine");
    return 0;
}

CAL_EXPORT int cal_wl_match(const int64_t* colors_a, int64_t stride_a, int64_t Na, const int64_t* ptr_a, int64_t A,
                            const int64_t* colors_p, int64_t stride_p, int64_t Np, const int64_t* ptr_p, int64_t P, int64_t T,
                            int64_t max_nodes_a, int64_t* K, int64_t* self_a, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CAL_REQUIRE(Na >= 0 && A >= 0 && Np >= 0 && P >= 0 && max_nodes_a >= 0, "Na, A, Np, P, max_nodes_a must be >= 0");
    CAL_REQUIRE(T >= 0 && T <= kWlMaxT, "T must be in [0, 4096]");
    CAL_REQUIRE(Np <= kWlMaxProtoNodes, "the prototype batch has more than 4096 nodes");
    CAL_REQUIRE(stride_a >= Na && stride_p >= Np, "a row stride is shorter than its row");
    CAL_REQUIRE(A <= 0x7FFFFFFF, "too many graphs");
    if (A == 0) return 0;
    CAL_REQUIRE(ptr_a && self_a, "ptr_a / self_a are null");
    CAL_REQUIRE(P == 0 || (ptr_p && K), "ptr_p / K are null");
    CAL_REQUIRE((Na == 0 || colors_a) && (Np == 0 || colors_p), "colors_a / colors_p are null");
    WmArgs a{reinterpret_cast<const u64*>(colors_a), stride_a, Na, ptr_a, A, reinterpret_cast<const u64*>(colors_p), stride_p, Np,
             ptr_p, P, T, max_nodes_a, K, self_a};
    if (max_nodes_a <= kWlSmall)
        hipLaunchKernelGGL((k_wl_match<kWlSmall, kWlSmall>), dim3((unsigned)A), dim3(kWlSmall), 0, stream, a);
    else
        hipLaunchKernelGGL((k_wl_match<kSegWide, kSegCap>), dim3((unsigned)A), dim3(kSegWide), 0, stream, a);
    CAL_CHECK_LAUNCH("k_wl_match");
    return 0;
}
