// All-pairs intervention readout: the eval-mode `co` head (model.py:145-164) on EVERY pair of an objects row xo_g (B of them) and
// a trivial row xc_j (a bank of M), i.e. the backdoor adjustment P(Y | do(C)) = sum_s P(Y | C, s) P(s) summed exactly.
//
//   logp(g, j) = log_softmax(fc2(bn2(relu(fc1(bn1(x))))))      x = xc_j + xo_g (add) | cat(xc_j, xo_g) (cat)
//   p_do[g, c] = (1 / M) sum_j exp(logp(g, j)[c])              hits[g]  = #{j : argmax_c logp(g, j) == ref[g]} (lowest class on ties)
//   p_min[g]   = min_j exp(logp(g, j)[ref[g]])                 j_min[g] = the lowest j attaining it
//
// Both BatchNorms are affine in eval mode, so the pre-activation of fc1 splits into A[g] + Cb[j] (A: the xo part and every
// constant; Cb: the xc part; cat: the two column blocks of fc1_co.weight, each with its half of the BN scale) and bn2 folds into
// fc2 (W2f, b2f).  Neither [B M, H] nor a B M x H x H product exists.  THREE launches, no synchronisation, no read-back:
//
//  1. k_iv_fold   folds the parameters and forms A [B, HP] and Cb^T [HP, MP] (HP = H rounded up to 4, MP = M rounded up to 64, the
//                 padding zero): 32 x 128 output tiles, one 32 x 32 MFMA tile per wave (mma_rowk of engine_mma.hpp), operands
//                 staged through LDS with the BN scale applied on the way in; the constants are one more stretch of the
//                 reduction (the BN shift against the whole weight row).  One more workgroup writes W2f / b2f.
//  2. k_iv_pairs  one workgroup = 4 waves = 64 partners x 4 GB graphs.  Lane <-> partner, wave <-> GB graphs held as GB x CP
//                 accumulators (CP = C rounded up to 4, 8, 16, 32, 64; GB CP = 32, 64 at CP = 64).  The reduction runs in slices of
//                 64: the Cb^T slice [64 k][64 j] (conflict-free 4-byte reads, lane = bank), the workgroup's A rows and W2f are
//                 staged in LDS (22 .. 33 KB: four or more workgroups per CU at every shape); A and W2f are read as 16-byte
//                 broadcasts.  Per pair and k: one add, one max, C FMAs.  Then the softmax per pair, and the chunk's 64 partners
//                 are reduced inside the wave in a fixed order (DPP adds, a ballot for the hits and for the lowest j of the
//                 minimum) into one partial row per (chunk, graph).
//  3. k_iv_finish sums the chunks' partial rows in chunk order in fp64 (fp32 inside a chunk of 64), takes the minimum with the
//                 lowest j, and writes the sentinels (hits 0, p_min NaN, j_min -1) where ref is null or outside [0, C).
//
// No value is accumulated atomically and there is no ticket: two calls on the same inputs give the same bits.
//
// VALU, not MFMA, for the H x C contraction: on gfx950 the fp32 MFMA rate equals the fp32 vector rate (64 FLOP / clk / SIMD), so a
// matrix tile only pays when its columns are used.  A tile is 16 or 32 columns wide; at C <= 8 three quarters or more of it would
// multiply padding, and the add-ReLU that produces the A operand is VALU work either way (and would have to be laid out as an
// MFMA operand first).  On the VALU the pair costs 2 + C operations per k with no padding beyond CP.  At C = 64 (GB = 1) the
// kernel is bound by its LDS broadcasts instead (65 16-byte reads per 4 k against 264 VALU operations, four waves on one LDS);
// that corner is correct and tested, not tuned.
// LDS against occupancy: slicing the reduction keeps the workgroup at 22 .. 33 KB whatever H is (the whole Cb tile alone would be
// 64 KB at H = 256), so a CU holds 4 .. 7 workgroups by LDS (three waves per SIMD by registers) and a workgroup's two barriers per slice overlap with its neighbours' work.
#include "engine_mma.hpp"

namespace cal {
namespace {

constexpr int IV_J = 64;       // partners per chunk (one per lane)
constexpr int IV_KS = 64;      // reduction slice staged in LDS
constexpr int IV_LD = 36;      // row stride of the fold's LDS tiles (= 4 mod 32: conflict-free 16-byte reads)

struct IvBn { const float *w, *b, *mean, *var; float eps; };

struct IvArgs {
    const float *xo, *xc;
    int64_t B, M;
    int H, C, HP, CP, cat;
    int64_t MP;
    IvBn bn1, bn2;
    const float *W1, *b1, *W2, *b2;
    const int64_t* ref;
    float *p_do, *p_min, *logp_pairs;
    int32_t *hits, *j_min;
    // workspace
    float *w2f, *b2f, *A, *cbT, *part_p, *part_min;
    int32_t *part_hits, *part_j;
    int64_t ntA, ntC, nch;
};

__device__ __forceinline__ float bn_scale(const IvBn& bn, int k) { return bn.w[k] / sqrtf(bn.var[k] + bn.eps); }
__device__ __forceinline__ float bn_shift(const IvBn& bn, int k) { return bn.b[k] - bn.mean[k] * bn_scale(bn, k); }

// grid (ntA + ntC + 1, ceil(H / 128)), 256 threads.  Row tile bx < ntA: A rows; < ntA + ntC: Cb rows; the last: W2f / b2f.
__global__ void __launch_bounds__(256) k_iv_fold(IvArgs a) {
    __shared__ __align__(16) float xs[32 * IV_LD];
    __shared__ __align__(16) float ws[128 * IV_LD];
    const int t = threadIdx.x, H = a.H, HP = a.HP;
    const int64_t bx = blockIdx.x;
    if (bx == a.ntA + a.ntC) {
        if (blockIdx.y != 0) return;
        for (int i = t; i < a.CP * HP; i += 256) {
            const int c = i / HP, k = i % HP;
            a.w2f[i] = (c < a.C && k < H) ? a.W2[(size_t)c * H + k] * bn_scale(a.bn2, k) : 0.f;
        }
        if (t < a.CP) {
            float s = 0.f;
            if (t < a.C) {
                s = a.b2[t];
                for (int k = 0; k < H; ++k) s = fmaf(a.W2[(size_t)t * H + k], bn_shift(a.bn2, k), s);
            }
            a.b2f[t] = s;
        }
        return;
    }
    const bool isA = bx < a.ntA;
    const int64_t r0 = (isA ? bx : bx - a.ntA) * 32, nrows = isA ? a.B : a.M;
    const float* src = isA ? a.xo : a.xc;
    const int Kin = a.cat ? 2 * H : H, koff = (isA && a.cat) ? H : 0;
    const int Kred = isA ? H + Kin : H;               // A: the row's own stretch, then the BN shift against the whole weight row
    const int n0 = blockIdx.y * 128;
    const int wave = t >> 6, lane = t & 63, li = lane & 31, lk = lane >> 5;
    gc_f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int k0 = 0; k0 < Kred; k0 += 32) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = t + i * 256, r = idx >> 5, kk = k0 + (idx & 31);
            float v = 0.f;
            if (kk < H) {
                if (r0 + r < nrows) v = src[(size_t)(r0 + r) * H + kk] * bn_scale(a.bn1, koff + kk);
            } else if (kk < Kred) {
                v = bn_shift(a.bn1, kk - H);
            }
            xs[r * IV_LD + (idx & 31)] = v;
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int idx = t + i * 256, n = idx >> 5, kk = k0 + (idx & 31);
            float v = 0.f;
            if (n0 + n < H && kk < Kred) v = a.W1[(size_t)(n0 + n) * Kin + (kk < H ? koff + kk : kk - H)];
            ws[n * IV_LD + (idx & 31)] = v;
        }
        __syncthreads();
        if (n0 + wave * 32 < HP) mma_rowk(xs + li * IV_LD, ws + (wave * 32 + li) * IV_LD, 32, lk, acc);
        __syncthreads();
    }
    const int n = n0 + wave * 32 + li;
    if (n >= HP) return;
    const float bias = (isA && n < H) ? a.b1[n] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int64_t row = r0 + mma_row(r, lk);
        if (row >= nrows) continue;
        const float v = n < H ? acc[r] + bias : 0.f;
        if (isA) a.A[(size_t)row * HP + n] = v;
        else a.cbT[(size_t)n * a.MP + row] = v;
    }
}

// grid (nch, ceil(B / (4 GB))), 256 threads: wave w owns the graphs gb0 + w GB .. + GB, lane l the partner chunk * 64 + l
template <int CP, int GB>
__global__ void __launch_bounds__(256) k_iv_pairs(IvArgs a) {
    __shared__ __align__(16) float cb_s[IV_KS * IV_J];
    __shared__ __align__(16) float a_s[4 * GB * IV_KS];
    __shared__ __align__(16) float w_s[CP * IV_KS];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int HP = a.HP, C = a.C;
    const int64_t chunk = blockIdx.x, j0 = chunk * IV_J, j = j0 + lane;
    const int64_t gb0 = (int64_t)blockIdx.y * (4 * GB);
    float acc[GB][CP];
#pragma unroll
    for (int g = 0; g < GB; ++g)
#pragma unroll
        for (int c = 0; c < CP; ++c) acc[g][c] = 0.f;

    for (int k0 = 0; k0 < HP; k0 += IV_KS) {
        const int kn = min(IV_KS, HP - k0);                      // (a multiple of 4)
        // Cb^T slice: rows k0 .. k0 + kn of [HP, MP], 64 columns from j0 (inside MP; columns >= M were never written: zeroed here)
        for (int i = t; i < kn * (IV_J / 4); i += 256) {
            const int k = i >> 4, q = (i & 15) * 4;
            float4 v = *reinterpret_cast<const float4*>(a.cbT + (size_t)(k0 + k) * a.MP + j0 + q);
            if (j0 + q + 0 >= a.M) v.x = 0.f;
            if (j0 + q + 1 >= a.M) v.y = 0.f;
            if (j0 + q + 2 >= a.M) v.z = 0.f;
            if (j0 + q + 3 >= a.M) v.w = 0.f;
            *reinterpret_cast<float4*>(cb_s + k * IV_J + q) = v;
        }
        for (int i = t; i < 4 * GB * (IV_KS / 4); i += 256) {
            const int r = i / (IV_KS / 4), q = (i % (IV_KS / 4)) * 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (gb0 + r < a.B && q < kn) v = *reinterpret_cast<const float4*>(a.A + (size_t)(gb0 + r) * HP + k0 + q);
            *reinterpret_cast<float4*>(a_s + r * IV_KS + q) = v;
        }
        for (int i = t; i < CP * (IV_KS / 4); i += 256) {
            const int c = i / (IV_KS / 4), q = (i % (IV_KS / 4)) * 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (q < kn) v = *reinterpret_cast<const float4*>(a.w2f + (size_t)c * HP + k0 + q);
            *reinterpret_cast<float4*>(w_s + c * IV_KS + q) = v;
        }
        __syncthreads();
        for (int k = 0; k < kn; k += 4) {
            float cb[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) cb[i] = cb_s[(k + i) * IV_J + lane];
            float h[GB][4];
#pragma unroll
            for (int g = 0; g < GB; ++g) {
                const float4 av = *reinterpret_cast<const float4*>(a_s + (wave * GB + g) * IV_KS + k);
                h[g][0] = fmaxf(av.x + cb[0], 0.f);
                h[g][1] = fmaxf(av.y + cb[1], 0.f);
                h[g][2] = fmaxf(av.z + cb[2], 0.f);
                h[g][3] = fmaxf(av.w + cb[3], 0.f);
            }
#pragma unroll
            for (int c = 0; c < CP; ++c) {
                const float4 wv = *reinterpret_cast<const float4*>(w_s + c * IV_KS + k);
#pragma unroll
                for (int g = 0; g < GB; ++g)
                    acc[g][c] = fmaf(h[g][3], wv.w, fmaf(h[g][2], wv.z, fmaf(h[g][1], wv.y, fmaf(h[g][0], wv.x, acc[g][c]))));
            }
        }
        __syncthreads();
    }

    const bool jv = j < a.M;
    float b2[CP];
#pragma unroll
    for (int c = 0; c < CP; ++c) b2[c] = a.b2f[c];
#pragma unroll
    for (int g = 0; g < GB; ++g) {
        const int64_t gg = gb0 + wave * GB + g;                  // (uniform over the wave)
        if (gg >= a.B) continue;
        int64_t rf = a.ref ? a.ref[gg] : -1;
        if (rf < 0 || rf >= C) rf = -1;
        float mx = -INFINITY;
        int arg = 0;
#pragma unroll
        for (int c = 0; c < CP; ++c) {
            acc[g][c] += b2[c];
            if (c < C && acc[g][c] > mx) { mx = acc[g][c]; arg = c; }
        }
        float se = 0.f;
#pragma unroll
        for (int c = 0; c < CP; ++c) if (c < C) se += expf(acc[g][c] - mx);
        const float lse = mx + logf(se);
        float keep = 0.f, pr = INFINITY;
#pragma unroll
        for (int c = 0; c < CP; ++c) {
            if (c >= C) continue;                                 // (uniform)
            const float lp = acc[g][c] - lse;
            if (jv && a.logp_pairs) a.logp_pairs[((size_t)gg * a.M + j) * C + c] = lp;
            const float p = jv ? expf(lp) : 0.f;
            if (c == rf && jv) pr = p;
            const float s = group_sum<64>(p);                     // every lane: the chunk's sum, fixed order
            if (lane == c) keep = s;
        }
        if (lane < C) a.part_p[((size_t)chunk * a.B + gg) * CP + lane] = keep;
        const unsigned long long hit = __ballot(jv && arg == (int)rf);
        const float mn = -group_max<64>(-pr);
        const unsigned long long at = __ballot(jv && pr == mn);
        if (lane == 0) {
            const size_t o = (size_t)chunk * a.B + gg;
            a.part_hits[o] = __popcll(hit);
            a.part_min[o] = mn;
            a.part_j[o] = at ? (int32_t)(j0 + __ffsll((long long)at) - 1) : -1;
        }
    }
}

// grid ceil(B (C + 1) / 256): thread (g, c < C) sums column c of the chunks' rows in fp64; thread (g, C) combines the scalars
__global__ void __launch_bounds__(256) k_iv_finish(IvArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int C = a.C;
    if (i >= a.B * (C + 1)) return;
    const int64_t g = i / (C + 1);
    const int c = (int)(i % (C + 1));
    if (c < C) {
        double s = 0.0;
        for (int64_t ch = 0; ch < a.nch; ++ch) s += (double)a.part_p[((size_t)ch * a.B + g) * a.CP + c];
        a.p_do[(size_t)g * C + c] = (float)(s / (double)a.M);
        return;
    }
    const int64_t rf = a.ref ? a.ref[g] : -1;
    if (rf < 0 || rf >= C) {
        a.hits[g] = 0;
        a.p_min[g] = __builtin_nanf("");
        a.j_min[g] = -1;
        return;
    }
    int64_t h = 0;
    float mn = INFINITY;
    int32_t jm = -1;
    for (int64_t ch = 0; ch < a.nch; ++ch) {
        const size_t o = (size_t)ch * a.B + g;
        h += a.part_hits[o];
        const float m = a.part_min[o];
        if (m < mn || jm < 0) { mn = m; jm = a.part_j[o]; }
    }
    a.hits[g] = (int32_t)h;
    a.p_min[g] = mn;
    a.j_min[g] = jm;
}

inline int iv_cp(int64_t C) { return C <= 4 ? 4 : C <= 8 ? 8 : C <= 16 ? 16 : C <= 32 ? 32 : 64; }
inline int iv_gb(int CP) { return CP == 64 ? 1 : 32 / CP; }

struct IvLayout { int64_t w2f, b2f, A, cbT, part_p, part_min, part_hits, part_j, total; int HP, CP; int64_t MP, nch; };

inline IvLayout iv_layout(int64_t B, int64_t M, int64_t H, int64_t C) {
    IvLayout l;
    l.HP = (int)((H + 3) & ~(int64_t)3);
    l.CP = iv_cp(C);
    l.nch = (M + IV_J - 1) / IV_J;
    l.MP = l.nch * IV_J;
    int64_t o = 0;
    auto take = [&](int64_t n) { const int64_t at = o; o += (n + 3) & ~(int64_t)3; return at; };
    l.w2f = take((int64_t)l.CP * l.HP);
    l.b2f = take(64);
    l.A = take(B * l.HP);
    l.cbT = take((int64_t)l.HP * l.MP);
    l.part_p = take(l.nch * B * l.CP);
    l.part_min = take(l.nch * B);
    l.part_hits = take(l.nch * B);
    l.part_j = take(l.nch * B);
    l.total = o;
    return l;
}

}  // namespace
}  // namespace cal

using namespace cal;

CAL_EXPORT int64_t cal_intervene_ws(int64_t B, int64_t M, int64_t H, int64_t C) {
    if (B < 0 || M < 1 || H < 1 || H > 256 || C < 2 || C > 64) return 0;
    return 4 * iv_layout(B, M, H, C).total + 256;
}

CAL_EXPORT int cal_intervene_pairs(const float* xo, int64_t B, const float* xc, int64_t M, int64_t H, int64_t C, int cat,
                                   const float* bn1_w, const float* bn1_b, const float* bn1_mean, const float* bn1_var, float bn1_eps,
                                   const float* fc1_w, const float* fc1_b, const float* bn2_w, const float* bn2_b,
                                   const float* bn2_mean, const float* bn2_var, float bn2_eps, const float* fc2_w,
                                   const float* fc2_b, const int64_t* ref, float* p_do, int32_t* hits, float* p_min,
                                   int32_t* j_min, float* logp_pairs, void* ws, int64_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CAL_REQUIRE(B >= 0, "B must be >= 0");
    CAL_REQUIRE(M >= 1, "the bank is empty (M must be >= 1)");
    CAL_REQUIRE(H >= 1 && H <= 256, "H must be in [1, 256]");
    CAL_REQUIRE(C >= 2 && C <= 64, "C must be in [2, 64]");
    if (B == 0) return 0;
    CAL_REQUIRE(xo && xc && p_do && hits && p_min && j_min, "xo / xc / an output is null");
    CAL_REQUIRE(bn1_w && bn1_b && bn1_mean && bn1_var && fc1_w && fc1_b && bn2_w && bn2_b && bn2_mean && bn2_var && fc2_w && fc2_b,
                "a parameter of the co head is null");
    CAL_REQUIRE(ws && ws_bytes >= cal_intervene_ws(B, M, H, C) && (reinterpret_cast<uintptr_t>(ws) & 15) == 0,
                "ws must be 16-byte aligned and hold cal_intervene_ws(B, M, H, C) bytes");
    const IvLayout l = iv_layout(B, M, H, C);
    const int GB = iv_gb(l.CP);
    const int64_t nby = (B + 4 * GB - 1) / (4 * GB);
    CAL_REQUIRE(nby <= 65535, "B too large (at most 65535 graph blocks per call)");
    CAL_REQUIRE(l.nch <= 0x7FFFFFFF && (B + 31) / 32 + (M + 31) / 32 + 1 <= 0x7FFFFFFF && B * (C + 1) / 256 + 1 <= 0x7FFFFFFF,
                "B or M too large");
    float* w = (float*)ws;
    IvArgs a;
    a.xo = xo; a.xc = xc; a.B = B; a.M = M; a.H = (int)H; a.C = (int)C; a.HP = l.HP; a.CP = l.CP; a.cat = cat ? 1 : 0; a.MP = l.MP;
    a.bn1 = IvBn{bn1_w, bn1_b, bn1_mean, bn1_var, bn1_eps};
    a.bn2 = IvBn{bn2_w, bn2_b, bn2_mean, bn2_var, bn2_eps};
    a.W1 = fc1_w; a.b1 = fc1_b; a.W2 = fc2_w; a.b2 = fc2_b; a.ref = ref;
    a.p_do = p_do; a.p_min = p_min; a.logp_pairs = logp_pairs; a.hits = hits; a.j_min = j_min;
    a.w2f = w + l.w2f; a.b2f = w + l.b2f; a.A = w + l.A; a.cbT = w + l.cbT; a.part_p = w + l.part_p; a.part_min = w + l.part_min;
    a.part_hits = (int32_t*)(w + l.part_hits); a.part_j = (int32_t*)(w + l.part_j);
    a.ntA = (B + 31) / 32; a.ntC = (M + 31) / 32; a.nch = l.nch;
    hipLaunchKernelGGL(k_iv_fold, dim3((unsigned)(a.ntA + a.ntC + 1), (unsigned)((H + 127) / 128)), dim3(256), 0, stream, a);
    CAL_CHECK_LAUNCH("k_iv_fold");
    const dim3 grid((unsigned)l.nch, (unsigned)nby);
    switch (l.CP) {
        case 4: hipLaunchKernelGGL((k_iv_pairs<4, 8>), grid, dim3(256), 0, stream, a); break;
        case 8: hipLaunchKernelGGL((k_iv_pairs<8, 4>), grid, dim3(256), 0, stream, a); break;
        case 16: hipLaunchKernelGGL((k_iv_pairs<16, 2>), grid, dim3(256), 0, stream, a); break;
        case 32: hipLaunchKernelGGL((k_iv_pairs<32, 1>), grid, dim3(256), 0, stream, a); break;
        default: hipLaunchKernelGGL((k_iv_pairs<64, 1>), grid, dim3(256), 0, stream, a); break;
    }
    CAL_CHECK_LAUNCH("k_iv_pairs");
    hipLaunchKernelGGL(k_iv_finish, dim3((unsigned)((B * (C + 1) + 255) / 256)), dim3(256), 0, stream, a);
    CAL_CHECK_LAUNCH("k_iv_finish");
    return 0;
}
