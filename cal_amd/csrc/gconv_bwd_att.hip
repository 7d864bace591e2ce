// k_gconv_bwd_att: the ATT mode of the per-graph GCNConv backward (engine_gconv_bwd_body.hpp with MODE 3) -- the last backbone
// layer's backward with the per-graph attention backward (engine_attphases.hpp) run while it stages; launched by bwd_att of
// engine.hip through cal_launch_gconv_bwd_att.
//
// A translation unit, and so a code object, of its own ON PURPOSE: inside engine.hip the kernel (25 KB of text) moved the kernels
// of the step engine behind it, and steps that never launch it measured 0.2-0.6 % slower although they ran the instructions they
// ran before (profiles/r9/ab_attfold.txt).  engine_order.hpp fixes the ORDER of engine.hip's kernels; a
// kernel added there, or one whose length changes, still moves every kernel behind it.  Here it moves none.
//
// The engine's headers define their non-template kernels without `inline`, so a second translation unit that includes them
// defines those kernels a second time.  They are included inside an unnamed namespace: every definition of this file has internal
// linkage, and what crosses to engine.hip is the one entry declared in engine_unit.hpp.
#include <stdint.h>
#include "engine_unit.hpp"

#define CAL_GCB_UNIT              // this unit takes the build's order of the two products (engine_gconv_bwd.hpp)
namespace {
#include "engine_kernels.hpp"
#include "engine_readout.hpp"
#include "engine_gconv.hpp"
#include "engine_gconv_bwd.hpp"
#include "engine_attbwd.hpp"      // AttBwdGraphArgs

namespace cal {
__global__ void __launch_bounds__(GB_NT, 1) k_gconv_bwd_att(const CSR g, const int* __restrict__ gptr, const int* __restrict__ eptr,
                                                           const GconvBwdBranch2 bb, float loop_w, int N, int H,
                                                           int K, int* __restrict__ status, const AttBwdGraphArgs ga) {
    constexpr bool RS = false, TILED = false, LEAN = false;
    constexpr int MODE = 3;
#include "engine_gconv_bwd_body.hpp"
}
}  // namespace cal
}  // namespace

extern "C" int cal_launch_gconv_bwd_att(const calunit::LaunchSite& at, const void* csr, size_t csr_bytes, const int* gptr, const int* eptr,
                                        const void* branches, size_t branches_bytes, float loop_w, int N, int H, int K, int* status,
                                        const void* att, size_t att_bytes) {
    using namespace cal;
    CSR g; GconvBwdBranch2 bb; AttBwdGraphArgs ga;
    if (!calunit::take(g, csr, csr_bytes) || !calunit::take(bb, branches, branches_bytes) || !calunit::take(ga, att, att_bytes)) return 2;
    calunit::launch(k_gconv_bwd_att, at, dim3(GB_NT), g, gptr, eptr, bb, loop_w, N, H, K, status, ga);
    return 0;
}

CAL_UNIT_BLK_CLOCKS(cal_debug_blk_clocks_att)
