// The instantiations of k_gconv_bwd (engine_gconv_bwd.hpp) that run the two products behind P1 one after the other
// (-DCAL_GCB_ORDER=1, the default: the four non-LEAN ones; 2: the LEAN ones too, a measuring build); launched by gconv_bwd of
// engine.hip through cal_launch_gconv_bwd_seq.  With -DCAL_GCB_ORDER=0 this file holds no kernel.
//
// A translation unit, and so a code object, of its own for the reason gconv_bwd_att.hip is one: compiled inside engine.hip the
// shorter kernels moved every kernel behind them, and steps that never launch them measured up to 0.45 % slower than the parent
// (profiles/r10/ab_bwd_order.txt): a kernel whose length changes moves what follows it, whatever fixes the order.  engine.hip
// keeps its order-0 text of all eight instantiations and launches the LEAN ones itself.  Internal linkage as in
// gconv_bwd_att.hip; the entry follows engine_unit.hpp.
#include <stdint.h>
#include "engine_unit.hpp"

#define CAL_GCB_UNIT              // this unit takes the build's order of the two products (engine_gconv_bwd.hpp)
namespace {
#include "engine_kernels.hpp"
#include "engine_readout.hpp"
#include "engine_gconv.hpp"
#include "engine_gconv_bwd.hpp"
}  // namespace

// sel and the return codes: engine_unit.hpp
extern "C" int cal_launch_gconv_bwd_seq(const calunit::LaunchSite& at, int sel, const void* csr, size_t csr_bytes, const int* gptr, const int* eptr,
                                        const void* branches, size_t branches_bytes, float loop_w, int N, int H, int K, int* status) {
    using namespace cal;
    CSR g; GconvBwdBranch2 bb;
    if (!calunit::take(g, csr, csr_bytes) || !calunit::take(bb, branches, branches_bytes)) return 2;
#if CAL_GCB_ORDER == 0
    return 3;
#else
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
    calunit::launch(kern, at, dim3(GB_NT), g, gptr, eptr, bb, loop_w, N, H, K, status);
    return 0;
#endif
}

CAL_UNIT_BLK_CLOCKS(cal_debug_blk_clocks_seq)
