// The operand-tile and epilogue vocabulary of the node-level GEMM kernels (gemm.hip 64 x 64, gemm_big.hip 128 x 128, gemm_ks.hip
// K split over waves, gemm_wres.hip weight-resident): one definition of what the contract of engine.hpp (GemmArgs / GemmProb)
// asks of every one of them.  The K loops and their scheduling stay in the kernels.
//
//   basics      gc_f32x16, mma_row (engine_mma.hpp), pin4, BK
//   operands    tile_load<T, KC, MODE>, tile_store<T, KC, MODE, XF>     T x 32 operand tile: global -> registers -> LDS
//               xform_tables<KC, T, ST>                                 BatchNorm scale / shift tables of a transformed operand
//   epilogue    EpiAux<NS> (load, pin, scale)                           aux values + row scales of the BN-backward dot sums
//               epi_walk                                                bias, ReLU, store, the two fp64 column sums of one accumulator
//               stat_fold, stat_commit, stat_commit1                    lane halves -> LDS, partial row or (striped) atomics
//   host        xform_class, gemm_xa_class, gemm_operands_plain_aligned, with_xa
#pragma once
#include "engine_mma.hpp"
#include <type_traits>

namespace cal {

constexpr int BK = 32;    // K step of the tile kernels (BK = 64 measured slower in gemm.hip: 9.6 vs 8.8 us at K = 128)

__device__ __forceinline__ void pin4(float4& v) { asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w)); }

// ---- operand tiles ------------------------------------------------------------------------------------------------------
// The operand is logically X[mn][k] (mn = row of A / column of B), the tile T x BK, 256 threads.
//   KC = true : memory is [mn][k] row-major (k contiguous)  -> transposing LDS store, row stride T + 1
//   KC = false: memory is [k][mn] row-major (mn contiguous) -> direct 16 B LDS store, row stride T + 4
// MODE 0 = interior tile: unconditional 16 B loads.
// MODE 1 = ragged in mn only (last row / column tile; K range whole, 16 B aligned, and for !KC operands mn_end % 4 == 0):
//          16 B loads from a CLAMPED row / column group.  The rows or columns past the end then hold copies of valid data,
//          which only ever reach accumulator rows / columns the epilogue never stores -- no zeroing, same speed as an
//          interior tile (the scalar path made the one ragged workgroup of a [7315,128] launch the critical path: 18 us
//          against 5.6 us for its 229 neighbours).
// MODE 2 = anything else: every element from a clamped (always valid) address, zeroed at store time.
// MODE 3 = MODE 1 with a ragged K range on a !KC operand (gemm_big.hip: K = node rows of a weight gradient): the k row is
//          clamped too, and k rows past the end are zeroed as whole float4 at store time.
// No divergent control flow in any mode.
template <int T> constexpr int tile_nq() { return T * BK / 4 / 256; }      // float4 per thread per operand tile
template <int T, bool KC> constexpr int tile_ld() { return KC ? T + 1 : T + 4; }

template <int T, bool KC, int MODE>
__device__ __forceinline__ void tile_load(float4 (&r)[tile_nq<T>()], const float* __restrict__ p, int ld, int mn0, int mn_end,
                                          int k0, int k_end) {
#pragma unroll
    for (int q = 0; q < tile_nq<T>(); ++q) {
        const int f = threadIdx.x + q * 256;
        const int mn = KC ? f / (BK / 4) : (f % (T / 4)) * 4;
        const int k = KC ? (f % (BK / 4)) * 4 : f / (T / 4);
        if (MODE == 0) {
            r[q] = KC ? *reinterpret_cast<const float4*>(p + (size_t)(mn0 + mn) * ld + k0 + k)
                      : *reinterpret_cast<const float4*>(p + (size_t)(k0 + k) * ld + mn0 + mn);
        } else if (MODE == 1 || MODE == 3) {
            const int kr = MODE == 3 ? min(k0 + k, k_end - 1) : k0 + k;
            r[q] = KC ? *reinterpret_cast<const float4*>(p + (size_t)min(mn0 + mn, mn_end - 1) * ld + k0 + k)
                      : *reinterpret_cast<const float4*>(p + (size_t)kr * ld + min(mn0 + mn, mn_end - 4));
        } else if (KC) {
            const float* row = p + (size_t)min(mn0 + mn, mn_end - 1) * ld;
            const int kl = k_end - 1;
            r[q] = make_float4(row[min(k0 + k, kl)], row[min(k0 + k + 1, kl)], row[min(k0 + k + 2, kl)], row[min(k0 + k + 3, kl)]);
        } else {
            const float* row = p + (size_t)min(k0 + k, k_end - 1) * ld;
            const int ml = mn_end - 1;
            r[q] = make_float4(row[min(mn0 + mn, ml)], row[min(mn0 + mn + 1, ml)], row[min(mn0 + mn + 2, ml)], row[min(mn0 + mn + 3, ml)]);
        }
    }
}

// XF: 0 = plain, 1 = BN scale/shift on the feature axis, 2 = per-storage-row scale, then BN.
// sc/sh: LDS tables indexed by (k - kb) for KC operands and by the tile-local mn for !KC ones.
template <int T, bool KC, int MODE, int XF>
__device__ __forceinline__ void tile_store(const float4 (&r)[tile_nq<T>()], float* __restrict__ s, int mn0, int mn_end, int k0,
                                           int k_end, int kb, const float* __restrict__ rsp, int rs_stride,
                                           const float* sc, const float* sh) {
    constexpr int LD = tile_ld<T, KC>();
#pragma unroll
    for (int q = 0; q < tile_nq<T>(); ++q) {
        const int f = threadIdx.x + q * 256;
        const int mn = KC ? f / (BK / 4) : (f % (T / 4)) * 4;
        const int k = KC ? (f % (BK / 4)) * 4 : f / (T / 4);
        float v[4] = {r[q].x, r[q].y, r[q].z, r[q].w};
        if (XF > 0) {
            float rs = 1.f;
            if (XF == 2) rs = rsp[(size_t)(KC ? min(mn0 + mn, mn_end - 1) : min(k0 + k, k_end - 1)) * rs_stride];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int fi = KC ? (k0 + k + j - kb) : (mn + j);     // feature index into the tables
                v[j] = fmaf(XF == 2 ? rs * v[j] : v[j], sc[fi], sh[fi]);
            }
        }
        if (MODE == 2) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool ok = KC ? (mn0 + mn < mn_end && k0 + k + j < k_end) : (k0 + k < k_end && mn0 + mn + j < mn_end);
                v[j] = ok ? v[j] : 0.f;
            }
        }
        if (KC) {
            s[(k + 0) * LD + mn] = v[0]; s[(k + 1) * LD + mn] = v[1];
            s[(k + 2) * LD + mn] = v[2]; s[(k + 3) * LD + mn] = v[3];
        } else {
            const bool ok = MODE != 3 || k0 + k < k_end;
            *reinterpret_cast<float4*>(s + k * LD + mn) = ok ? make_float4(v[0], v[1], v[2], v[3]) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
}

// BN scale / shift tables of a transformed operand: features [kb, ke) of a KC operand, the tile's min(T, mn_end - mn0)
// features from mn0 of a !KC one (the table's tail zero-filled up to T).  ST: striped reader of the statistics (engine.hpp).
// upd: this workgroup is the one that updates the BatchNorm's running statistics.  256 threads; the caller synchronises.
template <bool KC, int T, bool ST>
__device__ __forceinline__ void xform_tables(const BNRef& bn, float* sc, float* sh, int kb, int ke, int mn0, int mn_end, bool upd) {
    const int cnt = KC ? (ke - kb) : min(T, mn_end - mn0);
    const int c0 = KC ? kb : mn0;
    for (int t = threadIdx.x; t < cnt; t += 256) {
        bn_scale_shift<ST>(bn, c0 + t, sc[t], sh[t]);
        if (bn.update && upd) bn_update_running<ST>(bn, c0 + t);
    }
    if (!KC) for (int t = cnt + threadIdx.x; t < T; t += 256) { sc[t] = 0.f; sh[t] = 0.f; }
}

// ---- epilogue -----------------------------------------------------------------------------------------------------------
// C/D layout of the 32x32 MFMA: lane (li, lk) holds column li of the rows mma_row(r, lk), r = 0..15.
//
// aux values of the BN-backward dot sums for the 16 rows of NS accumulators side by side (columns col[0..NS)), and the rows'
// scales, as ONE batch of unconditional loads on clamped rows (no scale: the aux pointer again, stride 0, value ignored);
// a per-row `if (aux_rs)` made every row a load, a branch and a dependent second load.  load, (the caller's other loads),
// pin, scale -- in that order, so that nothing waits before everything is requested.
template <int NS>
struct EpiAux {
    float v[NS][16], rs[16];
    __device__ __forceinline__ void load(const GemmProb& pr, int rbase, int lk, int M, int N, const int (&col)[NS]) {
        const bool has_rs = pr.aux_rs != nullptr;
        const float* rsp = has_rs ? pr.aux_rs : pr.aux;
        const size_t rstr = has_rs ? (size_t)pr.aux_rs_stride : 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const size_t row = (size_t)min(mma_row(r, lk, rbase), M - 1);
            rs[r] = rsp[row * rstr];
#pragma unroll
            for (int sn = 0; sn < NS; ++sn) v[sn][r] = pr.aux[row * N + col[sn]];
        }
    }
    __device__ __forceinline__ void pin() {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            asm volatile("" : "+v"(rs[r]));
#pragma unroll
            for (int sn = 0; sn < NS; ++sn) asm volatile("" : "+v"(v[sn][r]));
        }
    }
    __device__ __forceinline__ void scale(const GemmProb& pr) {
        const bool has_rs = pr.aux_rs != nullptr;
#pragma unroll
        for (int r = 0; r < 16; ++r)
#pragma unroll
            for (int sn = 0; sn < NS; ++sn) v[sn][r] *= has_rs ? rs[r] : 1.f;
    }
};

// One accumulator: bias (bv), ReLU, store to C (may be null), column statistics (want_st) or dot sums against the
// normalised aux values (want_dot) into s1 / s2.  interior: no per-element guards, the 16 stores stream out.
__device__ __forceinline__ void epi_walk(const gc_f32x16& acc, const float (&aux)[16], float bv, float amean, float arstd, int relu,
                                         float* C, int ldc, int rbase, int lk, int col, int M, bool interior, bool cok,
                                         bool want_st, bool want_dot, double& s1, double& s2) {
    auto emit = [&](int r, int row) {
        float v = acc[r] + bv;
        if (relu) v = fmaxf(v, 0.f);
        if (C) C[(size_t)row * ldc + col] = v;
        if (want_st) { s1 += (double)v; s2 += (double)v * (double)v; }
        if (want_dot) {
            const float xn = (aux[r] - amean) * arstd;
            s1 += (double)v;
            s2 += (double)v * (double)xn;
        }
    };
    if (interior) {
#pragma unroll
        for (int r = 0; r < 16; ++r) emit(r, mma_row(r, lk, rbase));
    } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = mma_row(r, lk, rbase);
            if (row < M && cok) emit(r, row);
        }
    }
}

// the two lane halves of a wave (rows 4 lk ..) added; lane half 0 leaves the wave's column sums in slot[0 / 1][li]
__device__ __forceinline__ void stat_fold(double& s1, double& s2, double (&slot)[2][32], int li, int lk) {
    s1 += __shfl_xor(s1, 32, 64);
    s2 += __shfl_xor(s2, 32, 64);
    if (lk == 0) { slot[0][li] = s1; slot[1][li] = s2; }
}
// One of a workgroup's two column sums (which = 0 / 1) leaves: as the partial row of its row tile, parts[row tiles][2][N],
// or added atomically into the row tile's plane of the site's accumulator (engine.hpp; plane 0 for every tile at st_ss == 0,
// which is what every launch on k_gemm_big and k_wres has: engine.hip gemm_stats stripes only the k_gemm / k_gemm_ks launches).
__device__ __forceinline__ void stat_commit1(const GemmProb& pr, bool want_st, int which, int row_tile, int N, int col, double t) {
    if (pr.parts) pr.parts[((size_t)row_tile * 2 + which) * N + col] = t;
    else atomicAdd((which ? (want_st ? pr.st_sq : pr.dot_prod) : (want_st ? pr.st_sum : pr.dot_sum)) + (size_t)(row_tile % NSTRIPE) * pr.st_ss + col, t);
}
__device__ __forceinline__ void stat_commit(const GemmProb& pr, bool want_st, int row_tile, int N, int col, double t1, double t2) {
    if (pr.parts) {
        pr.parts[((size_t)row_tile * 2 + 0) * N + col] = t1;
        pr.parts[((size_t)row_tile * 2 + 1) * N + col] = t2;
    } else {
        const size_t po = (size_t)(row_tile % NSTRIPE) * pr.st_ss + col;
        atomicAdd((want_st ? pr.st_sum : pr.dot_sum) + po, t1);
        atomicAdd((want_st ? pr.st_sq : pr.dot_prod) + po, t2);
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------
// operand-transform class: 0 = plain, 1 = BN, 2 = row scale + BN (a row scale without BN is not instantiated anywhere)
inline int xform_class(const Xform& x) { return x.has_bn ? (x.rs ? 2 : 1) : 0; }
// ... of operand A over a batch; -1 = mixed
inline int gemm_xa_class(const GemmArgs& a, int nbatch) {
    int x = -1;
    for (int b = 0; b < nbatch; ++b) {
        const int m = xform_class(a.p[b].xa);
        if (x >= 0 && x != m) return -1;
        x = m;
    }
    return x;
}
// both operands 16-byte aligned with leading dimensions to match, no transform on B, no row scale without BN on A
inline bool gemm_operands_plain_aligned(const GemmArgs& a, int nbatch) {
    bool ok = a.lda % 4 == 0 && a.ldb % 4 == 0;
    for (int b = 0; b < nbatch; ++b)
        ok = ok && aligned16(a.p[b].A) && aligned16(a.p[b].B) && !a.p[b].xb.has_bn && !a.p[b].xb.rs && !(a.p[b].xa.rs && !a.p[b].xa.has_bn);
    return ok;
}
// f(std::integral_constant<int, xa>) for xa in 0..2 (as engine.hip's with_g)
template <typename F>
void with_xa(int xa, F f) {
    if (xa == 0) f(std::integral_constant<int, 0>());
    else if (xa == 1) f(std::integral_constant<int, 1>());
    else f(std::integral_constant<int, 2>());
}

}  // namespace cal
