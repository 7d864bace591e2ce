// The instantiations of k_gconv_bwd (engine_gconv_bwd.hpp) that run the two products behind P1 one after the other
// (-DCAL_GCB_ORDER=1, the default: the four non-LEAN ones; 2: the LEAN ones too, a measuring build); launched by gconv_bwd of
// engine.hip through cal_launch_gconv_bwd_seq.  With -DCAL_GCB_ORDER=0 this file holds no kernel.
//
// A translation unit, and so a code object, of its own for the reason gconv_bwd_att.hip is one: compiled inside engine.hip the
// shorter kernels moved every kernel behind them, and steps that never launch them measured up to 0.45 % slower than the parent
// (profiles/r10/ab_bwd_order.txt).  engine.hip keeps its order-0 text of all eight instantiations -- its device code is what it
// was, byte for byte -- and launches the LEAN ones itself.  Internal linkage and untyped structure arguments as in
// gconv_bwd_att.hip.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <string.h>

#define CAL_GCB_UNIT              // this unit takes the build's order of the two products (engine_gconv_bwd.hpp)
namespace {
#include "engine_kernels.hpp"
#include "engine_readout.hpp"
#include "engine_gconv.hpp"
#include "engine_gconv_bwd.hpp"
}  // namespace

// sel: 1 = two branches (POOL), 2 = packed tiles (POOL only), 4 = dOut given (MODE 0; otherwise UP), 8 = LEAN.  e0 / e1: events
// stamped with the dispatch's start and end (a profiled launch), or null.  Returns 0; 2 when the caller's structures are not the
// ones this file was compiled with; 3 when this build does not hold the instantiation.
extern "C" int cal_launch_gconv_bwd_seq(int sel, unsigned gx, unsigned gy, unsigned gz, hipStream_t st, hipEvent_t e0, hipEvent_t e1, const void* csr,
                                        size_t csr_bytes, const int* gptr, const int* eptr, const void* branches, size_t branches_bytes, float loop_w,
                                        int N, int H, int K, int* status) {
    using namespace cal;
    if (csr_bytes != sizeof(CSR) || branches_bytes != sizeof(GconvBwdBranch2)) return 2;
#if CAL_GCB_ORDER == 0
    return 3;
#else
    CSR g; GconvBwdBranch2 bb;
    memcpy(&g, csr, sizeof(g)); memcpy(&bb, branches, sizeof(bb));
    void (*kern)(const CSR, const int*, const int*, const GconvBwdBranch2, float, int, int, int, int*) = nullptr;
    switch (sel) {
        case 1: kern = k_gconv_bwd<true, 2>; break;
        case 3: kern = k_gconv_bwd<true, 2, true>; break;
        case 4: kern = k_gconv_bwd<false, 0>; break;
        case 0: kern = k_gconv_bwd<false, 1>; break;
#if CAL_GCB_ORDER == 2
        case 9: kern = k_gconv_bwd<true, 2, false, true>; break;
        case 11: kern = k_gconv_bwd<true, 2, true, true>; break;
        case 12: kern = k_gconv_bwd<false, 0, false, true>; break;
        case 8: kern = k_gconv_bwd<false, 1, false, true>; break;
#endif
        default: return 3;
    }
    const dim3 grid(gx, gy, gz);
    if (e0) hipExtLaunchKernelGGL(kern, grid, dim3(GB_NT), 0, st, e0, e1, 0, g, gptr, eptr, bb, loop_w, N, H, K, status);
    else hipLaunchKernelGGL(kern, grid, dim3(GB_NT), 0, st, g, gptr, eptr, bb, loop_w, N, H, K, status);
    return 0;
#endif
}

#ifdef CAL_BLK_CLOCKS
// this translation unit's copies of the clock buffers (engine_kernels.hpp): marks 0 .. 3 to out, 4 .. 7 to outx, 8192 values each
extern "C" __attribute__((visibility("default"))) int cal_debug_blk_clocks_seq(long long* out, long long* outx) {
    const int rc = (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(cal::g_blk_clk), sizeof(long long) * 8192);
    return rc ? rc : (int)hipMemcpyFromSymbol(outx, HIP_SYMBOL(cal::g_blk_clk_x), sizeof(long long) * 8192);
}
#endif
