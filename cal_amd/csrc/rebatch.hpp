// The count / scan / write toolkit of the batch builders (splice.hip, occlude.hip, coalition.hip, noise.hip, subset.hip): operators
// that make a new batch of R result graphs out of the graphs of an old one.  Device helpers are __device__ __forceinline__, host
// helpers plain inline or macros: no kernel and no translation unit of their own.  (Occlusion, coalitions and subsets share their
// two kernels as well: restrict.hpp, on top of this.)
//
// The protocol, two launches with the caller's one read-back of totals between them:
//  * the count launch, one workgroup per result graph, leaves every result graph's node and column count in ws.  The workgroup
//    that finishes last (last_workgroup: one atomicInc per workgroup on a wrapping counter, nothing else) scans the R counts
//    into ptr_out / edge_ptr_out and writes totals (scan_counts): the integer result does not depend on which workgroup that is,
//    and no output value is accumulated atomically.
//  * the write launch, 256 threads: its first ceil(Nout / kNodeChunk) workgroups take kNodeChunk result nodes each
//    (write_nodes: the result graph by binary search in ptr_out, batch_out / node_src, then the feature rows of the chunk:
//    16 bytes per lane when F % 4 == 0 and every base is 16-byte aligned, else element by element); the column workgroups
//    follow, for the replica builders one per replica (write_cols).
// twin.hip uses the completion ticket alone.
#pragma once
#include <atomic>

#include "segment.hpp"

namespace cal {

constexpr int kNodeChunk = 256;            // result nodes of one node workgroup (one per thread in the index phase)
constexpr int kTickets = 64;               // concurrent ticketed launches (on different streams) that may be in flight

// ---- the completion ticket -----------------------------------------------------------------------------------------------------
namespace {                                // (anonymous: every translation unit has its own slots and call counter)
__device__ unsigned int g_ticket[kTickets];   // zero at load; atomicInc wraps each back to zero
std::atomic<unsigned> g_ticket_calls{0};

// the slot of this translation unit's next ticketed launch
inline int next_ticket() { return (int)(g_ticket_calls.fetch_add(1) % kTickets); }

// true in every thread of the one workgroup, of the launch's nblk, that arrives last: what the others wrote to global memory
// before their call is visible to it (agent-scope loads).  flag is one int of LDS; every thread of the workgroup calls it.
__device__ __forceinline__ bool last_workgroup(int slot, int nblk, int* flag) {
    if (threadIdx.x == 0) {
        __threadfence();
        *flag = atomicInc(&g_ticket[slot], (unsigned)(nblk - 1)) == (unsigned)(nblk - 1);
    }
    __syncthreads();
    if (!*flag) return false;
    __threadfence();
    return true;
}
}  // namespace

// ---- the scan of the counts ----------------------------------------------------------------------------------------------------
// exclusive prefix of v over the workgroup's NT threads in thread order, the workgroup's sum in tot (two barriers)
template <int NT>
__device__ __forceinline__ long long wg_excl_sum(long long v, long long* red, long long& tot) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    long long inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const long long u = __shfl_up(inc, o, 64);
        if (lane >= o) inc += u;
    }
    __syncthreads();
    if (lane == 63) red[w] = inc;
    __syncthreads();
    long long base = 0, t = 0;
#pragma unroll
    for (int i = 0; i < NT / 64; ++i) {
        const long long r = red[i];
        base += i < w ? r : 0;
        t += r;
    }
    tot = t;
    return base + inc - v;
}

// The last workgroup's scan over the R result graphs, nodes[] / cols[] their counts as the other workgroups left them: thread t
// owns the run [t L, (t + 1) L).  ptr_out / eptr_out [R + 1]: the exclusive sums; totals[0..4]: nodes, columns, the largest
// node count, the largest column count, result graphs without a node.
template <int NT>
__device__ __forceinline__ void scan_counts(const int64_t* nodes, const int64_t* cols, int64_t R, int64_t* ptr_out,
                                            int64_t* eptr_out, int64_t* totals, long long* red) {
    const int64_t L = (R + NT - 1) / NT, lo = (int64_t)threadIdx.x * L, hi = lo + L < R ? lo + L : R;
    long long sn = 0, se = 0, mn = 0, me = 0, empty = 0;
    for (int64_t p = lo; p < hi; ++p) {
        const long long n = __hip_atomic_load(nodes + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const long long e = __hip_atomic_load(cols + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        sn += n;
        se += e;
        mn = n > mn ? n : mn;
        me = e > me ? e : me;
        empty += n == 0;
    }
    long long tn, te;
    long long on = wg_excl_sum<NT>(sn, red, tn), oe = wg_excl_sum<NT>(se, red, te);
    for (int64_t p = lo; p < hi; ++p) {
        ptr_out[p] = on;
        eptr_out[p] = oe;
        on += __hip_atomic_load(nodes + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        oe += __hip_atomic_load(cols + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    mn = wg_max<NT>(mn, red);
    me = wg_max<NT>(me, red);
    empty = wg_sum<NT>(empty, red);
    if (threadIdx.x == 0) {
        ptr_out[R] = tn;
        eptr_out[R] = te;
        totals[0] = tn;
        totals[1] = te;
        totals[2] = mn;
        totals[3] = me;
        totals[4] = empty;
    }
}

// ---- the write launch ----------------------------------------------------------------------------------------------------------
// what a write launch fills, the part of the kernel arguments the builders share
struct WriteOut {
    int64_t Nout, Eout;        // totals[0], totals[1] as the caller read them
    int64_t* batch_out;        // [Nout]
    float* x_out;              // [Nout, F] or null
    int64_t* ei_out;           // [2, Eout]
    int64_t* node_src;         // [Nout]
    int64_t* edge_src;         // [Eout]
    int64_t F;
    int vec;                   // the 16-byte row copy applies
};

// the 16-byte row copy applies: rows of F floats from xa (and xb, if any) to x_out
inline bool rows_vec(const float* x_out, int64_t F, const float* xa, const float* xb = nullptr) {
    return x_out && F % 4 == 0 &&
           ((reinterpret_cast<uintptr_t>(xa) | reinterpret_cast<uintptr_t>(xb) | reinterpret_cast<uintptr_t>(x_out)) & 15) == 0;
}

inline WriteOut write_out(int64_t Nout, int64_t Eout, int64_t* batch_out, float* x_out, int64_t* ei_out, int64_t* node_src,
                          int64_t* edge_src, int64_t F, const float* xa, const float* xb = nullptr) {
    return WriteOut{Nout, Eout, batch_out, x_out, ei_out, node_src, edge_src, F, rows_vec(x_out, F, xa, xb) ? 1 : 0};
}

// last index q in [0, n) with p[q] <= i; p non-decreasing with p[0] = 0 <= i (the result graph that owns element i, empty ones
// skipped)
template <class T>
__device__ __forceinline__ int64_t owner(const T* p, int64_t n, int64_t i) {
    int64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (p[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// Node workgroup blockIdx.x of a write launch (256 threads): the result nodes [blockIdx.x kNodeChunk, ...).  code(r, l) is the
// source row code of node l of result graph r, none where there is no such node: it goes to node_src as it is; row(code) is
// the base of that source row.  src: kNodeChunk slots of LDS.
template <class Code, class Row>
__device__ __forceinline__ void write_nodes(const WriteOut& o, const int64_t* ptr_out, int64_t R, int64_t none, int64_t* src,
                                            Code code, Row row) {
    const int64_t i0 = (int64_t)blockIdx.x * kNodeChunk, i = i0 + threadIdx.x;
    int64_t s = none;
    if (i < o.Nout) {
        const int64_t r = owner(ptr_out, R + 1, i);
        if (r < R) {
            s = code(r, i - ptr_out[r]);
            if (s != none) {
                o.batch_out[i] = r;
                o.node_src[i] = s;
            }
        }
    }
    if (!o.x_out) return;
    src[threadIdx.x] = s;
    __syncthreads();
    const int64_t left = o.Nout - i0;
    const unsigned rows = (unsigned)(left < kNodeChunk ? left : kNodeChunk);
    if (o.vec) {
        const unsigned F4 = (unsigned)(o.F >> 2), n = rows * F4;
        float4* out = reinterpret_cast<float4*>(o.x_out) + i0 * F4;
        for (unsigned t = threadIdx.x; t < n; t += 256) {
            const unsigned rr = t / F4, c = t - rr * F4;
            const int64_t sr = src[rr];
            if (sr == none) continue;
            out[t] = reinterpret_cast<const float4*>(row(sr))[c];
        }
    } else {
        const unsigned F = (unsigned)o.F, n = rows * F;
        float* out = o.x_out + i0 * o.F;
        for (unsigned t = threadIdx.x; t < n; t += 256) {
            const unsigned rr = t / F, c = t - rr * F;
            const int64_t sr = src[rr];
            if (sr == none) continue;
            out[t] = row(sr)[c];
        }
    }
}

// The column workgroup of replica r (256 threads): walks the source columns [elo, elo + em) of (ei, E) in chunks and writes the
// ones with stays(e), in order, at eptr_out[r] on; local(u) is the new local id of endpoint u.  em is uniform over the
// workgroup; wcnt: 4 ints of LDS.
template <class Stays, class Local>
__device__ __forceinline__ void write_cols(const WriteOut& o, const int64_t* ptr_out, const int64_t* eptr_out, int64_t r,
                                           const int64_t* ei, int64_t E, int64_t elo, int64_t em, int* wcnt, Stays stays,
                                           Local local) {
    const int64_t n0 = ptr_out[r], j0 = eptr_out[r], j1 = eptr_out[r + 1] < o.Eout ? eptr_out[r + 1] : o.Eout;
    int64_t carry = 0;
    for (int64_t base = 0; base < em; base += 256) {
        const int64_t e = elo + base + threadIdx.x;
        const bool f = base + threadIdx.x < em && stays(e);
        int t;
        const int pos = wg_excl<256>(f, wcnt, t);
        const int64_t j = j0 + carry + pos;
        if (f && j < j1) {
            o.ei_out[j] = n0 + local(ei[e]);
            o.ei_out[o.Eout + j] = n0 + local(ei[E + e]);
            o.edge_src[j] = e;
        }
        carry += t;
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
// the count entry point's answer without a result graph: totals[0 .. n) and the two offsets' first entries are zero
inline int zero_counts(const char* entry, int64_t* totals, int n, int64_t* ptr_out, int64_t* eptr_out, hipStream_t stream) {
    if (hipMemsetAsync(totals, 0, n * sizeof(int64_t), stream) != hipSuccess ||
        hipMemsetAsync(ptr_out, 0, sizeof(int64_t), stream) != hipSuccess ||
        hipMemsetAsync(eptr_out, 0, sizeof(int64_t), stream) != hipSuccess) {
        set_error("%s: hipMemsetAsync failed", entry);
        return 1;
    }
    return 0;
}

// KERNEL<NT><<<n, NT, 0, stream>>>(a): wide workgroups once the average source graph (avg columns) has more columns than a
// 256-thread workgroup walks in a few chunks
#define CAL_REBATCH_COUNT(KERNEL, avg, n, stream, a)                                                                             \
    do {                                                                                                                         \
        if ((avg) > 2048) hipLaunchKernelGGL(KERNEL<1024>, dim3((unsigned)(n)), dim3(1024), 0, stream, a);                       \
        else hipLaunchKernelGGL(KERNEL<256>, dim3((unsigned)(n)), dim3(256), 0, stream, a);                                      \
    } while (0)

// The checks of a write entry point on what it fills (CAL_REQUIRE names the entry point), x_ok / x_msg its own on the features;
// then nb, eb: the node and column (col_blocks) workgroups of the launch.
#define CAL_REBATCH_REQUIRE_WRITE(R, x_ok, x_msg, col_blocks)                                                                    \
    CAL_REQUIRE(Nout >= 0 && Eout >= 0 && F >= 0 && F < (1 << 22), "Nout, Eout must be >= 0 and 0 <= F < 2^22");                 \
    CAL_REQUIRE(R == 0 || (ptr_out && edge_ptr_out), "ptr_out / edge_ptr_out are null");                                         \
    CAL_REQUIRE(Nout == 0 || (batch_out && node_src), "batch_out / node_src are null");                                          \
    CAL_REQUIRE(Eout == 0 || (edge_index_out && edge_src), "edge_index_out / edge_src are null");                                \
    CAL_REQUIRE(x_ok, x_msg);                                                                                                    \
    const int64_t nb = (Nout + kNodeChunk - 1) / kNodeChunk, eb = (col_blocks);                                                  \
    CAL_REQUIRE(nb + eb <= 0x7FFFFFFF, "too many elements")

}  // namespace cal
