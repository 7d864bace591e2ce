// Test hook: one flat problem description -> GemmArgs / GemmProb / Xform / BNRef (engine.hpp) -> one of the GEMM launchers.
// tests/test_gpu_gemm_contract.py drives every operand transform, epilogue, sum mode, batch and split of the four kernel
// files through it; cal_gemm / cal_gemm_ks can express only plain operands, bias and ReLU.  The hook adds no logic: the
// description is copied field by field the way engine.hip fills it (memset to zero, the sizes and leading dimensions of
// gemm_args, gemm_set_split), and the selection rules are the launchers' own.  No twin in the host library.
//
// Split-K: the slices are left as slabs (slab z of problem b at C_b + z * M * ldc, as the engine's grad_slabs hands them to
// k_finish); the caller sums them.  k_splitk_reduce is NOT run here.
//
// Layout of the description (all arrays in HOST memory; pointers inside pv are DEVICE pointers, 0 = null):
//   iv[0..7]                  transA, transB, M, N, K, relu, nbatch (1..3), split (0: one slice, 1: splitk_for as grad_slabs)
//   iv[8 + 24 b + ..]         problem b: 0 xa.rs_stride, 1 xb.rs_stride, 2 aux_rs_stride, 3 has_aux, 4 st_ss,
//                             then three BatchNorm blocks of 5 at 5 (xa.bn), 10 (xb.bn), 15 (aux_bn):
//                                 + 0 present (xa / xb: has_bn), 1 rows (inv_n = 1 / rows, unbias = rows / (rows - 1)),
//                                 + 2 update, 3 use_running, 4 ss
//   pv[40 b + ..]             problem b: 0 A, 1 B, 2 C, 3 bias, 4 xa.rs, 5 xb.rs, 6 st_sum, 7 st_sq, 8 aux, 9 aux_rs,
//                             10 dot_sum, 11 dot_prod, 12 parts, then three BatchNorm blocks of 7 at 13, 20, 27:
//                                 + 0 sum, 1 sq, 2 gamma, 3 beta, 4 run_mean, 5 run_var, 6 num_batches_tracked
//   dv[0]                     eps of every BatchNorm
#include "engine.hpp"
#include <cstring>

using namespace cal;

namespace {

constexpr int IV_HEAD = 8, IV_PROB = 24, PV_PROB = 40;

BNRef probe_bn(const int64_t* iv, void* const* pv, double eps) {
    BNRef r;
    memset(&r, 0, sizeof(r));
    const int rows = (int)iv[1];
    r.sum = (const double*)pv[0]; r.sq = (const double*)pv[1];
    r.gamma = (const float*)pv[2]; r.beta = (const float*)pv[3];
    r.inv_n = 1.0 / (double)(rows > 0 ? rows : 1); r.eps = (float)eps;
    r.run_mean = (float*)pv[4]; r.run_var = (float*)pv[5]; r.nbt = (int64_t*)pv[6];
    r.unbias = rows > 1 ? (float)rows / (float)(rows - 1) : 1.f;
    r.update = (int)iv[2];
    r.use_running = (int)iv[3];
    r.ss = (int)iv[4];
    return r;
}

// 0 = filled, else the description is malformed
int probe_fill(const int64_t* iv, void* const* pv, const double* dv, GemmArgs& a, bool& transA, bool& transB, int& nbatch) {
    memset(&a, 0, sizeof(a));
    transA = iv[0] != 0; transB = iv[1] != 0;
    for (int i = 2; i <= 4; ++i)
        if (iv[i] < 0 || iv[i] >= (1ll << 31)) return 1;
    a.M = (int)iv[2]; a.N = (int)iv[3]; a.K = (int)iv[4];
    a.lda = transA ? a.M : a.K; a.ldb = transB ? a.K : a.N; a.ldc = a.N;
    a.relu = (int)iv[5];
    nbatch = (int)iv[6];
    if (nbatch < 1 || nbatch > 3) return 1;
    gemm_set_split(a, iv[7] ? splitk_for(a.M, a.N, a.K, nbatch) : 1);
    for (int b = 0; b < nbatch; ++b) {
        const int64_t* ib = iv + IV_HEAD + IV_PROB * b;
        void* const* pb = pv + PV_PROB * b;
        GemmProb& p = a.p[b];
        p.A = (const float*)pb[0]; p.B = (const float*)pb[1]; p.C = (float*)pb[2]; p.bias = (const float*)pb[3];
        p.xa.rs = (const float*)pb[4]; p.xa.rs_stride = (int)ib[0];
        p.xb.rs = (const float*)pb[5]; p.xb.rs_stride = (int)ib[1];
        p.st_sum = (double*)pb[6]; p.st_sq = (double*)pb[7];
        p.aux = (const float*)pb[8]; p.aux_rs = (const float*)pb[9]; p.aux_rs_stride = (int)ib[2];
        p.has_aux = (int)ib[3];
        p.dot_sum = (double*)pb[10]; p.dot_prod = (double*)pb[11];
        p.parts = (double*)pb[12];
        p.st_ss = (int)ib[4];
        p.xa.has_bn = (int)ib[5];
        if (p.xa.has_bn) p.xa.bn = probe_bn(ib + 5, pb + 13, dv[0]);
        p.xb.has_bn = (int)ib[10];
        if (p.xb.has_bn) p.xb.bn = probe_bn(ib + 10, pb + 20, dv[0]);
        if (ib[15]) p.aux_bn = probe_bn(ib + 15, pb + 27, dv[0]);
    }
    return 0;
}

}  // namespace

// What a caller needs to size its buffers, from the launchers' own rules: out[0] split-K factor (splitk_for), out[1] slices
// and out[2] slice length after gemm_set_split with that factor, out[3] partial rows per problem of launch_gemm
// (gemm_row_tiles; hasC = 0: a statistics-only launch), out[4] of launch_gemm_ks (gemm_ks_row_tiles), out[5] NSTRIPE.
CAL_EXPORT int cal_gemm_probe_plan(int64_t M, int64_t N, int64_t K, int nbatch, int hasC, int64_t* out) {
    CAL_REQUIRE(M >= 0 && N >= 0 && K >= 0 && M < (1ll << 31) && N < (1ll << 31) && K < (1ll << 31), "sizes out of range");
    GemmArgs a;
    memset(&a, 0, sizeof(a));
    a.M = (int)M; a.N = (int)N; a.K = (int)K;
    const int S = splitk_for(M, N, K, nbatch);
    gemm_set_split(a, S);
    out[0] = S; out[1] = a.nsplit; out[2] = a.kchunk;
    out[3] = gemm_row_tiles(a.M, a.N, a.K, hasC != 0);
    out[4] = gemm_ks_row_tiles(a.M);
    out[5] = NSTRIPE;
    return 0;
}

// sel: 0 launch_gemm, 1 launch_gemm_ks, 2 launch_gemm_big alone, 3 launch_gemm_wres alone, 4 launch_gemm_dual (iv / pv: the
// NT set ax, iv2 / pv2: the TN set aw; null otherwise).  Returns 0 = launched, 1 = the launch itself failed, 2 = refused (a
// malformed description, or the launcher's own refusal; cal_last_error has the message), 3 = the kernel of an "alone"
// selector declined the launch (nothing ran).
CAL_EXPORT int cal_gemm_probe(int sel, const int64_t* iv, void* const* pv, const int64_t* iv2, void* const* pv2,
                              const double* dv, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    GemmArgs a, a2;
    bool ta, tb, ta2, tb2;
    int nb, nb2;
    CAL_REQUIRE(iv && pv && dv, "description missing");
    CAL_REQUIRE(probe_fill(iv, pv, dv, a, ta, tb, nb) == 0, "malformed description");
    if (sel == 0) return launch_gemm(ta, tb, a, nb, stream);
    if (sel == 1) {
        CAL_REQUIRE(!ta && a.nsplit == 1, "the K-split kernel takes neither transA nor split-K");
        return launch_gemm_ks(tb, a, nb, stream);
    }
    if (sel == 2 || sel == 3) {
        const int r = sel == 2 ? launch_gemm_big(ta, tb, a, nb, stream) : launch_gemm_wres(ta, tb, a, nb, stream);
        if (r < 0) return 2;
        if (r == 0) { set_error("cal_gemm_probe: %s declined the launch", sel == 2 ? "launch_gemm_big" : "launch_gemm_wres"); return 3; }
        return 0;
    }
    if (sel == 4) {
        CAL_REQUIRE(iv2 && pv2, "second description missing");
        CAL_REQUIRE(probe_fill(iv2, pv2, dv, a2, ta2, tb2, nb2) == 0, "malformed description");
        CAL_REQUIRE(!ta && tb && ta2 && !tb2, "the dual launch is NT + TN");
        return launch_gemm_dual(a, nb, a2, nb2, stream);
    }
    set_error("cal_gemm_probe: unknown selector %d", sel);
    return 2;
}
