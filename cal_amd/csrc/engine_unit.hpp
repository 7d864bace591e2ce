// The protocol between engine.hip and its side units -- the translation units that hold a step-engine kernel outside engine.hip's
// code object (gconv_fwd_att.hip, gconv_bwd_att.hip, gconv_bwd_seq.hip).  Host code only.  A side unit includes this header at
// global scope, in front of the unnamed namespace that holds its copy of the engine's headers; engine.hip includes it too, so one
// declaration checks both the definition and the call of every entry.
//
// An entry takes the launch site, the engine's structures as untyped pointer + size (the two files compile the same headers into
// different namespaces: same layout, other types) and the kernel's scalar arguments.  It returns 0, 2 when a structure is not the
// one the unit was compiled with, 3 when the unit's build does not hold the kernel asked for.
// (namespace calunit and not cal: inside a side unit `cal` is the copy in its unnamed namespace)
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stddef.h>
#include <string.h>

namespace calunit {

// Where a kernel goes: grid, stream, and the two events a profiled dispatch is stamped with (its start and end), or null.
struct LaunchSite { dim3 grid; hipStream_t st; hipEvent_t e0, e1; };

template <typename... P, typename... A>
inline void launch(void (*kern)(P...), const LaunchSite& at, dim3 block, A&&... a) {
    if (at.e0) hipExtLaunchKernelGGL(kern, at.grid, block, 0, at.st, at.e0, at.e1, 0, static_cast<P>(a)...);
    else hipLaunchKernelGGL(kern, at.grid, block, 0, at.st, static_cast<P>(a)...);
}

// An untyped structure argument into its typed local; false when the caller's structure is not this unit's.
template <typename T>
inline bool take(T& dst, const void* src, size_t bytes) {
    if (bytes != sizeof(T)) return false;
    memcpy(&dst, src, sizeof(T));
    return true;
}

}  // namespace calunit

extern "C" {
// gconv_fwd_att.hip: k_gconv_fwd_att, the last backbone layer's per-graph forward with the attention forward as its tail; grid (graphs, 2 slices)
int cal_launch_gconv_fwd_att(const calunit::LaunchSite& at, const void* csr, size_t csr_bytes, const int* gptr, const int* eptr, const void* branches,
                             size_t branches_bytes, int relu, float loop_w, int H, int K, int* status, const void* att, size_t att_bytes);
// gconv_bwd_att.hip: k_gconv_bwd_att, the ATT mode of the per-graph GCNConv backward; grid (graphs, slices)
int cal_launch_gconv_bwd_att(const calunit::LaunchSite& at, const void* csr, size_t csr_bytes, const int* gptr, const int* eptr, const void* branches,
                             size_t branches_bytes, float loop_w, int N, int H, int K, int* status, const void* att, size_t att_bytes);
// gconv_bwd_seq.hip: the k_gconv_bwd instantiations that run the dX' and dW products one after the other (CAL_GCB_ORDER).
// sel: 1 = two branches (POOL), 2 = packed tiles (POOL only), 4 = dOut given (MODE 0; otherwise UP), 8 = LEAN
int cal_launch_gconv_bwd_seq(const calunit::LaunchSite& at, int sel, const void* csr, size_t csr_bytes, const int* gptr, const int* eptr,
                             const void* branches, size_t branches_bytes, float loop_w, int N, int H, int K, int* status);
// finish_plan.hip: k_finish_plan, the step's final commit (FinishArgs) beside the graph plan of the next batch (ChainPlan; B = 0: none) with
// the counters' in / out words (ChainCtl); 1-D grid of ChainCtl::nplan plan blocks + the commit's blocks, 256 threads
int cal_launch_finish_plan(const calunit::LaunchSite& at, const void* finish, size_t finish_bytes, float* grad, const void* plan, size_t plan_bytes,
                           const void* ctl, size_t ctl_bytes);
}

// A unit's accessor of ITS copies of the clock buffers (engine_kernels.hpp): marks 0 .. 3 to out, 4 .. 7 to outx, 8192 values each
#ifdef CAL_BLK_CLOCKS
#define CAL_UNIT_BLK_CLOCKS(name)                                                                                                \
    extern "C" __attribute__((visibility("default"))) int name(long long* out, long long* outx) {                                \
        const int rc = (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(cal::g_blk_clk), sizeof(long long) * 8192);                      \
        return rc ? rc : (int)hipMemcpyFromSymbol(outx, HIP_SYMBOL(cal::g_blk_clk_x), sizeof(long long) * 8192);                 \
    }
#else
#define CAL_UNIT_BLK_CLOCKS(name)
#endif
