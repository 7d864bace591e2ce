// The per-segment toolkit of the explanation kernels (explain.hip, twin.hip, subgraph.hip).  A segment is one graph's run of
// edge columns or nodes, [p[g], p[g+1]) of M elements in all.  Device helpers are __device__ __forceinline__, host helpers
// plain inline: no translation unit of their own.
#pragma once
#include "common.hpp"

namespace cal {

constexpr int kSegCap = 2048;    // LDS capacity S: elements of one segment / chunk (cal_explain_lds_cap())
constexpr int kSegWide = 1024;   // threads of the widest group and of the large-segment workgroups

// (seg_clamp, segment g of p clamped into [0, M]: rules.hpp)

// sum over the nw consecutive waves from wave w0 on (this thread's group), every thread of the group gets it; all threads of
// the workgroup call it (two barriers).  Fixed order: wave butterflies, then the group's wave partials in wave order.
__device__ __forceinline__ int64_t wave_group_total(int64_t v, int w0, int nw, long long* red) {
    long long s = v;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    long long t = 0;
    for (int i = 0; i < nw; ++i) t += red[w0 + i];
    return t;
}

// ... over the G consecutive threads (whole waves) of this thread's group
__device__ __forceinline__ int64_t group_total(int64_t v, int G, long long* red) {
    return wave_group_total(v, (int)(threadIdx.x / G) * (G >> 6), G >> 6, red);
}

// ... over the workgroup's NT threads
template <int NT>
__device__ __forceinline__ int64_t wg_sum(int64_t v, long long* red) {
    return wave_group_total(v, 0, NT / 64, red);
}

// maximum over the workgroup's NT threads, every thread gets it (two barriers)
template <int NT>
__device__ __forceinline__ long long wg_max(long long v, long long* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const long long u = __shfl_xor(v, o, 64);
        v = u > v ? u : v;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    long long t = red[0];
#pragma unroll
    for (int i = 1; i < NT / 64; ++i) t = red[i] > t ? red[i] : t;
    return t;
}

// position of this thread's flag among the set flags of the workgroup's NT threads (exclusive), their count in tot;
// every thread of the workgroup calls it (two barriers)
template <int NT>
__device__ __forceinline__ int wg_excl(bool f, int* wcnt, int& tot) {
    const unsigned long long b = __ballot(f);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int pre = __popcll(b & ((1ull << lane) - 1ull));
    __syncthreads();
    if (lane == 0) wcnt[w] = __popcll(b);
    __syncthreads();
    int base = 0, t = 0;
#pragma unroll
    for (int i = 0; i < NT / 64; ++i) {
        const int v = wcnt[i];
        base += i < w ? v : 0;
        t += v;
    }
    tot = t;
    return base + pre;
}

// first index of a row of n elements at which p is false; p holds on a prefix of the row (a sorted row, a threshold)
template <class T, class Pred>
__device__ __forceinline__ int first_false(const T* s, int n, Pred p) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (p(s[mid])) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Launch geometry of a kernel that gives every segment one group of G threads and cap LDS slots: G = 64 .. kSegWide, the
// smallest power of two covering min(max_seg, S); cap = G x (elements per lane) >= min(max_seg, S); workgroups of
// NT = max(G, 256) threads hold spb = NT / G segments; grid (nblk, nch).  large: some segment may exceed S (then
// G = NT = kSegWide, cap = S) and is worked on in nch chunks of S elements.
struct SegGeom {
    int G, cap, NT, spb;
    int64_t nch, nblk;
    bool large;
    bool chunks_ok() const { return nch <= 65535; }            // (grid.y)
    bool grid_ok() const { return nblk <= 0x7FFFFFFF; }        // (grid.x)
};

inline SegGeom seg_geom(int64_t max_seg, int64_t B) {
    SegGeom q;
    q.large = max_seg > kSegCap;
    q.nch = q.large ? (max_seg + kSegCap - 1) / kSegCap : 1;
    const int eff = (int)(max_seg < kSegCap ? max_seg : kSegCap);
    q.G = 64;
    while (q.G < eff && q.G < kSegWide) q.G <<= 1;
    q.cap = (eff > 0 ? (eff + q.G - 1) / q.G : 1) * q.G;
    q.NT = q.G <= 256 ? 256 : q.G;
    q.spb = q.NT / q.G;
    q.nblk = (B + q.spb - 1) / q.spb;
    return q;
}

// KERNEL<q.NT><<<(q.nblk, q.nch), q.NT, lds, stream>>>(args..., q.G, q.cap)
#define CAL_SEG_LAUNCH(KERNEL, q, lds, stream, ...)                                                                    \
    do {                                                                                                               \
        const dim3 grid_((unsigned)(q).nblk, (unsigned)(q).nch);                                                       \
        if ((q).NT == 256) hipLaunchKernelGGL(KERNEL<256>, grid_, dim3(256), lds, stream, __VA_ARGS__, (q).G, (q).cap); \
        else if ((q).NT == 512) hipLaunchKernelGGL(KERNEL<512>, grid_, dim3(512), lds, stream, __VA_ARGS__, (q).G, (q).cap); \
        else hipLaunchKernelGGL(KERNEL<1024>, grid_, dim3(1024), lds, stream, __VA_ARGS__, (q).G, (q).cap);            \
    } while (0)

// What one group of such a kernel owns.  valid: the group has a segment (g < B), of m elements; chunk_idx = blockIdx.y.
//   bad:   the segment is longer than max_seg: not worked on (the caller marks it, in chunk 0)
//   full:  it fits the cap: finished here, by chunk 0 only
//   chunk: it is larger (m > S here: cap = S whenever max_seg > S): this group works on [ulo, ulo + un) of it
// un = 0 for a group with nothing to do.  g and chunk_idx are uniform over the group, so are all five; over the workgroup
// only when it holds one segment (spb = 1, always so on the chunked path).
struct SegUnit {
    bool bad, full, chunk;
    int64_t ulo;
    int un;
};

__device__ __forceinline__ SegUnit seg_unit(bool valid, int64_t m, int64_t max_seg, int cap, int64_t chunk_idx) {
    SegUnit u;
    u.bad = valid && m > max_seg;
    u.full = valid && !u.bad && m <= cap && chunk_idx == 0;
    u.chunk = valid && !u.bad && m > cap;
    u.ulo = u.chunk ? chunk_idx * kSegCap : 0;
    u.un = u.full ? (int)m : (u.chunk && u.ulo < m ? (int)(m - u.ulo < kSegCap ? m - u.ulo : kSegCap) : 0);
    return u;
}

}  // namespace cal
