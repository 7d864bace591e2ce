// k_gconv_fwd_att: the last backbone layer's per-graph GCNConv forward (the body of k_gconv_fwd<false, 64, 512>, engine_gconv.hpp
// compiled with CAL_GCF_ATT_UNIT) with the per-graph attention forward as its tail (engine_attfwd_fold.hpp); launched by
// fwd_backbone of engine.hip through cal_launch_gconv_fwd_att when Route::att_fwd_fold is set.
//
// A translation unit, and so a code object, of its own for the reason gconv_bwd_att.hip is one: a new kernel inside engine.hip moves
// the kernels behind it, and steps that never launch it measured slower.  The engine's headers are included
// inside an unnamed namespace (they define their non-template kernels without `inline`); what crosses to engine.hip is the one
// entry declared in engine_unit.hpp.
#include <stdint.h>
#include "engine_unit.hpp"

#define CAL_GCF_ATT_UNIT          // engine_gconv.hpp: the kernel is k_gconv_fwd_att, with the attention operands and tail
namespace {
#include "engine_kernels.hpp"
#include "engine_readout.hpp"
#include "engine_gconv.hpp"
}  // namespace

extern "C" int cal_launch_gconv_fwd_att(const calunit::LaunchSite& at, const void* csr, size_t csr_bytes, const int* gptr, const int* eptr,
                                        const void* branches, size_t branches_bytes, int relu, float loop_w, int H, int K, int* status,
                                        const void* att, size_t att_bytes) {
    using namespace cal;
    CSR g; GconvBranch2 bb; AttFwdFoldArgs fa;
    if (!calunit::take(g, csr, csr_bytes) || !calunit::take(bb, branches, branches_bytes) || !calunit::take(fa, att, att_bytes)) return 2;
    calunit::launch(k_gconv_fwd_att<false, 64, 512, false>, at, dim3(512), g, gptr, eptr, bb, relu, loop_w, H, K, status, fa);
    return 0;
}

CAL_UNIT_BLK_CLOCKS(cal_debug_blk_clocks_fwd_att)
