// k_gconv_bwd_att: the ATT mode of the per-graph GCNConv backward (engine_gconv_bwd_body.hpp with MODE 3) -- the last backbone
// layer's backward with the per-graph attention backward (engine_attphases.hpp) run while it stages; launched by bwd_att of
// engine.hip through launch_gconv_bwd_att.
//
// A translation unit, and so a code object, of its own ON PURPOSE: inside engine.hip the kernel (25 KB of text) moved the kernels
// of the step engine behind it, and steps that never launch it measured 0.2-0.6 % slower although they ran the instructions they
// ran before (profiles/r9/ab_attfold.txt).  Here, engine.hip's device code is what it was, byte for byte.
//
// The engine's headers define their non-template kernels without `inline`, so a second translation unit that includes them
// defines those kernels a second time.  They are included inside an unnamed namespace: every definition of this file has internal
// linkage, and what crosses to engine.hip is one function whose structure arguments travel as untyped pointers (same headers,
// same layout; the sizes are checked on both sides).
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

// e0 / e1: events stamped with the dispatch's start and end (a profiled launch), or null.  Returns 0, or 2 when the caller's
// structures are not the ones this file was compiled with.
extern "C" int cal_launch_gconv_bwd_att(unsigned gx, unsigned gy, hipStream_t st, hipEvent_t e0, hipEvent_t e1, const void* csr, size_t csr_bytes,
                                        const int* gptr, const int* eptr, const void* branches, size_t branches_bytes, float loop_w, int N, int H,
                                        int K, int* status, const void* att, size_t att_bytes) {
    using namespace cal;
    if (csr_bytes != sizeof(CSR) || branches_bytes != sizeof(GconvBwdBranch2) || att_bytes != sizeof(AttBwdGraphArgs)) return 2;
    CSR g; GconvBwdBranch2 bb; AttBwdGraphArgs ga;
    memcpy(&g, csr, sizeof(g)); memcpy(&bb, branches, sizeof(bb)); memcpy(&ga, att, sizeof(ga));
    const dim3 grid(gx, gy, 1);
    if (e0) hipExtLaunchKernelGGL(k_gconv_bwd_att, grid, dim3(GB_NT), 0, st, e0, e1, 0, g, gptr, eptr, bb, loop_w, N, H, K, status, ga);
    else hipLaunchKernelGGL(k_gconv_bwd_att, grid, dim3(GB_NT), 0, st, g, gptr, eptr, bb, loop_w, N, H, K, status, ga);
    return 0;
}

#ifdef CAL_BLK_CLOCKS
// this translation unit's copies of the clock buffers (engine_kernels.hpp): marks 0 .. 3 to out, 4 .. 7 to outx, 8192 values each
extern "C" __attribute__((visibility("default"))) int cal_debug_blk_clocks_att(long long* out, long long* outx) {
    const int rc = (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(cal::g_blk_clk), sizeof(long long) * 8192);
    return rc ? rc : (int)hipMemcpyFromSymbol(outx, HIP_SYMBOL(cal::g_blk_clk_x), sizeof(long long) * 8192);
}
#endif
