// k_gconv_fwd_att: the last backbone layer's per-graph GCNConv forward (the body of k_gconv_fwd<false, 64, 512>, engine_gconv.hpp
// compiled with CAL_GCF_ATT_UNIT) with the per-graph attention forward as its tail (engine_attfwd_fold.hpp); launched by
// fwd_backbone of engine.hip through cal_launch_gconv_fwd_att when Route::att_fwd_fold is set.
//
// A translation unit, and so a code object, of its own for the reason gconv_bwd_att.hip is one: a new kernel inside engine.hip moves
// the kernels behind it, and steps that never launch it measured slower.  Here, engine.hip's device code is
// what it was.  The engine's headers are included inside an unnamed namespace (they define their non-template kernels without
// `inline`); what crosses to engine.hip is one function whose structure arguments travel as untyped pointers, sizes checked.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <string.h>

#define CAL_GCF_ATT_UNIT          // engine_gconv.hpp: the kernel is k_gconv_fwd_att, with the attention operands and tail
namespace {
#include "engine_kernels.hpp"
#include "engine_readout.hpp"
#include "engine_gconv.hpp"
}  // namespace

// e0 / e1: events stamped with the dispatch's start and end (a profiled launch), or null.  Returns 0, or 2 when the caller's
// structures are not the ones this file was compiled with.  Grid (graphs, 2 slices), 512 threads.
extern "C" int cal_launch_gconv_fwd_att(unsigned gx, hipStream_t st, hipEvent_t e0, hipEvent_t e1, const void* csr, size_t csr_bytes,
                                        const int* gptr, const int* eptr, const void* branches, size_t branches_bytes, int relu, float loop_w,
                                        int H, int K, int* status, const void* att, size_t att_bytes) {
    using namespace cal;
    if (csr_bytes != sizeof(CSR) || branches_bytes != sizeof(GconvBranch2) || att_bytes != sizeof(AttFwdFoldArgs)) return 2;
    CSR g; GconvBranch2 bb; AttFwdFoldArgs fa;
    memcpy(&g, csr, sizeof(g)); memcpy(&bb, branches, sizeof(bb)); memcpy(&fa, att, sizeof(fa));
    const dim3 grid(gx, 2, 1);
    auto kern = k_gconv_fwd_att<false, 64, 512, false>;
    if (e0) hipExtLaunchKernelGGL(kern, grid, dim3(512), 0, st, e0, e1, 0, g, gptr, eptr, bb, relu, loop_w, H, K, status, fa);
    else hipLaunchKernelGGL(kern, grid, dim3(512), 0, st, g, gptr, eptr, bb, relu, loop_w, H, K, status, fa);
    return 0;
}

#ifdef CAL_BLK_CLOCKS
// this translation unit's copies of the clock buffers (engine_kernels.hpp): marks 0 .. 3 to out, 4 .. 7 to outx, 8192 values each
extern "C" __attribute__((visibility("default"))) int cal_debug_blk_clocks_fwd_att(long long* out, long long* outx) {
    const int rc = (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(cal::g_blk_clk), sizeof(long long) * 8192);
    return rc ? rc : (int)hipMemcpyFromSymbol(outx, HIP_SYMBOL(cal::g_blk_clk_x), sizeof(long long) * 8192);
}
#endif
