// Soft edge masks (cal_amd/gradient.py): the two pieces of hot path the operator-level masked forward needs besides the GCN
// normalisation backward (gcn.hip) -- the gradient of a weighted plain sum w.r.t. its per-column weights (GINConv), and a GATConv
// whose edge softmax carries a per-column mask m >= 0 and returns d m.
//
// Both are gather-bound row kernels.  Every output element has one writer and a fixed summation order (no atomics, no
// communication between workgroups, every loop bounded by a row length or a width known at launch), so two calls on the same
// inputs give the same bits.  The masked GAT is ONE general path (any K <= 64, any D, scalar loads: no alignment demand), kept
// apart from gat.hip, whose specialised paths are pinned by their own contract tests (DESIGN.md "masked GATConv").
#include "cal_hip.h"
#include "common.hpp"

namespace cal {
namespace {


// butterfly sum / max over the lane offsets lo, 2 lo, ... < hi (powers of two): every lane of the span ends with the same bits
__device__ __forceinline__ float span_sum(float v, int lo, int hi) {
    for (int o = lo; o < hi; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float span_max(float v, int lo, int hi) {
    for (int o = lo; o < hi; o <<= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// ---- out[e] = <a[col[e], :], b[row[e], :]>, 0 for a self-loop column: d/dw_e of out_i = sum_{j -> i} w_ji x_j (+ loop) with
// a = the upstream gradient and b = the input.  One group of G lanes per column, VEC floats per lane and sweep.
template <int VEC>
__global__ void __launch_bounds__(256) k_edge_dot(const int* __restrict__ row32, const int* __restrict__ col32,
                                                  const float* __restrict__ a, const float* __restrict__ b,
                                                  float* __restrict__ out, int64_t E, int H, int G) {
    using V = Vec<VEC>;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t e = t / G;
    const int l = (int)(t % G);
    const bool live = e < E;
    float p = 0.f;
    bool loop = true;
    if (live) {
        const int r = row32[e], c = col32[e];
        loop = r == c;
        if (!loop) {
            const float* ap = a + (size_t)c * H;
            const float* bp = b + (size_t)r * H;
            for (int x = l * VEC; x < H; x += G * VEC) p += V::ld(ap + x).dot(V::ld(bp + x));
        }
    }
    p = span_sum(p, 1, G);
    if (live && l == 0) out[e] = loop ? 0.f : p;
}

// ---- masked GATConv ---------------------------------------------------------------------------------------------------------
// a_dst[i,k] = <z[i,k,:], att[k,:D]>, a_src[i,k] = <z[i,k,:], att[k,D:]>
__global__ void __launch_bounds__(256) k_gatm_scores(const float* __restrict__ z, const float* __restrict__ att,
                                                     float* __restrict__ adst, float* __restrict__ asrc, int64_t NK, int K, int D) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= NK) return;
    const int k = (int)(t % K);
    const float* zp = z + (size_t)t * D;
    const float* ad = att + (size_t)k * 2 * D;
    float sd = 0.f, ss = 0.f;
    for (int d = 0; d < D; ++d) { const float v = zp[d]; sd = fmaf(v, ad[d], sd); ss = fmaf(v, ad[D + d], ss); }
    adst[t] = sd;
    asrc[t] = ss;
}

// One wave per destination row.  Per head: max over the loop and the slots with m > 0, den = sum m exp(e - max) + 1e-16 (slots over
// the lanes); lane k keeps head k's pair.  Then the weighted sum with the columns over the lanes, 64 at a time.
__global__ void __launch_bounds__(256) k_gatm_fwd(const int* __restrict__ rowptr, const int* __restrict__ nbr, const int* __restrict__ eid,
                                                  const float* __restrict__ z, const float* __restrict__ bias, int relu, float slope,
                                                  const float* __restrict__ m, float* __restrict__ out, const float* __restrict__ adst,
                                                  const float* __restrict__ asrc, float* __restrict__ mx, float* __restrict__ den,
                                                  int N, int K, int D) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= N) return;                                       // (a whole wave)
    const int s0 = rowptr[i], s1 = rowptr[i + 1];
    const int H = K * D;
    float m_mine = 0.f, d_mine = 1.f;
    for (int k = 0; k < K; ++k) {
        const float ad = adst[(size_t)i * K + k];
        const float eself = lrelu(ad + asrc[(size_t)i * K + k], slope);
        float mv = eself;
        for (int s = s0 + lane; s < s1; s += 64)
            if (m[eid[s]] > 0.f) mv = fmaxf(mv, lrelu(ad + asrc[(size_t)nbr[s] * K + k], slope));
        mv = span_max(mv, 1, 64);
        float sum = 0.f;
        for (int s = s0 + lane; s < s1; s += 64) {
            const float ms = m[eid[s]];
            if (ms > 0.f) sum = fmaf(ms, expf(lrelu(ad + asrc[(size_t)nbr[s] * K + k], slope) - mv), sum);
        }
        sum = span_sum(sum, 1, 64);
        const float dn = sum + expf(eself - mv) + 1e-16f;
        if (lane == k) { m_mine = mv; d_mine = dn; mx[(size_t)i * K + k] = mv; den[(size_t)i * K + k] = dn; }
    }
    for (int c0 = 0; c0 < H; c0 += 64) {
        const int c = c0 + lane;
        const bool live = c < H;
        const int k = live ? c / D : 0;
        const float mk = __shfl(m_mine, k, 64), dk = __shfl(d_mine, k, 64);
        if (!live) continue;
        const float ad = adst[(size_t)i * K + k];
        float acc = 0.f;
        for (int s = s0; s < s1; ++s) {
            const float ms = m[eid[s]];
            if (ms > 0.f) {
                const int j = nbr[s];
                acc = fmaf(ms * expf(lrelu(ad + asrc[(size_t)j * K + k], slope) - mk), z[(size_t)j * H + c], acc);
            }
        }
        acc = fmaf(expf(lrelu(ad + asrc[(size_t)i * K + k], slope) - mk), z[(size_t)i * H + c], acc);
        float v = acc / dk + (bias ? bias[c] : 0.f);
        if (relu) v = fmaxf(v, 0.f);
        out[(size_t)i * H + c] = v;
    }
}

// Destination view, one wave per row, G lanes per slot (64 / G slots at a time).  With c_s = <g_i, z_j>_k, alpha_s = m_s q_s,
// q_s = exp(e_s - max) / den and S = sum_s alpha_s c_s:  d e_s = alpha_s (c_s - S) (max is a constant), written times the
// LeakyReLU slope into draw[id, k] (id = the column, E + i for the loop), and dm[col] = sum_k q_s (c_s - S).
__global__ void __launch_bounds__(256) k_gatm_bwd_dst(const int* __restrict__ rowptr, const int* __restrict__ nbr, const int* __restrict__ eid,
                                                      const float* __restrict__ z, const float* __restrict__ adst,
                                                      const float* __restrict__ asrc, const float* __restrict__ mx,
                                                      const float* __restrict__ den, const float* __restrict__ gout, float slope,
                                                      const float* __restrict__ m, float* __restrict__ draw, float* __restrict__ dm,
                                                      int N, int64_t E, int K, int D, int G) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= N) return;                                       // (a whole wave)
    const int s0 = rowptr[i], s1 = rowptr[i + 1];
    const int H = K * D, ngrp = 64 / G, grp = lane / G, gl = lane % G;
    const int nit = (s1 - s0 + 1 + ngrp - 1) / ngrp;
    const float* gi = gout + (size_t)i * H;
    float s_mine = 0.f;
    for (int k = 0; k < K; ++k) {
        const float ad = adst[(size_t)i * K + k], mk = mx[(size_t)i * K + k], dk = den[(size_t)i * K + k];
        float sp = 0.f;
        for (int it = 0; it < nit; ++it) {
            const int s = s0 + it * ngrp + grp;
            const bool valid = s <= s1, self = s >= s1;
            const int j = valid && !self ? nbr[s] : i;
            const float* zj = z + (size_t)j * H + (size_t)k * D;
            float dot = 0.f;
            for (int d = gl; d < D; d += G) dot = fmaf(gi[k * D + d], zj[d], dot);
            dot = span_sum(dot, 1, G);
            const float ms = valid && !self ? m[eid[s]] : 1.f;
            const float alpha = ms > 0.f ? ms * expf(lrelu(ad + asrc[(size_t)j * K + k], slope) - mk) / dk : 0.f;
            if (valid) sp = fmaf(alpha, dot, sp);
        }
        const float S = span_sum(sp, G, 64);
        if (lane == k) s_mine = S;
    }
    for (int it = 0; it < nit; ++it) {
        const int s = s0 + it * ngrp + grp;
        const bool valid = s <= s1, self = s >= s1;
        const int j = valid && !self ? nbr[s] : i;
        const int64_t id = valid && !self ? (int64_t)eid[s] : E + i;
        const float ms = valid && !self ? m[id] : 1.f;
        float dmacc = 0.f;
        for (int k = 0; k < K; ++k) {
            const float ad = adst[(size_t)i * K + k], mk = mx[(size_t)i * K + k], dk = den[(size_t)i * K + k];
            const float S = __shfl(s_mine, k, 64);
            const float* zj = z + (size_t)j * H + (size_t)k * D;
            float dot = 0.f;
            for (int d = gl; d < D; d += G) dot = fmaf(gi[k * D + d], zj[d], dot);
            dot = span_sum(dot, 1, G);
            const float raw = ad + asrc[(size_t)j * K + k];
            const float q = expf(lrelu(raw, slope) - mk) / dk;
            const float alpha = ms > 0.f ? ms * q : 0.f;
            if (valid && gl == 0) draw[(size_t)id * K + k] = alpha * (dot - S) * (raw > 0.f ? 1.f : slope);
            dmacc += q * (dot - S);
        }
        if (valid && !self && gl == 0) dm[id] = dmacc;
    }
}

// Source view, one wave per node j, the columns over the lanes: dz[j] = sum over the columns leaving j (and its loop) of
// alpha g[dst] + d a_dst[j] att[:D] + d a_src[j] att[D:], with d a_src[j] / d a_dst[j] the sums of draw over j's by-source / by-
// destination slots (each with the loop's), summed here in slot order.
__global__ void __launch_bounds__(256) k_gatm_bwd_src(const int* __restrict__ rowptr_src, const int* __restrict__ nbr_src,
                                                      const int* __restrict__ eid_src, const int* __restrict__ rowptr_dst,
                                                      const int* __restrict__ eid_dst, const float* __restrict__ att,
                                                      const float* __restrict__ adst, const float* __restrict__ asrc,
                                                      const float* __restrict__ mx, const float* __restrict__ den,
                                                      const float* __restrict__ gout, float slope, const float* __restrict__ m,
                                                      const float* __restrict__ draw, float* __restrict__ dz, int N, int64_t E, int K, int D) {
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= N) return;
    const int H = K * D;
    const int s0 = rowptr_src[j], s1 = rowptr_src[j + 1], t0 = rowptr_dst[j], t1 = rowptr_dst[j + 1];
    for (int c = lane; c < H; c += 64) {
        const int k = c / D, d = c - k * D;
        const float as = asrc[(size_t)j * K + k];
        float acc = 0.f, das = 0.f, dad = 0.f;
        for (int s = s0; s < s1; ++s) {
            const int i = nbr_src[s], e = eid_src[s];
            const float ms = m[e];
            if (ms > 0.f) {
                const float alpha = ms * expf(lrelu(adst[(size_t)i * K + k] + as, slope) - mx[(size_t)i * K + k]) / den[(size_t)i * K + k];
                acc = fmaf(alpha, gout[(size_t)i * H + c], acc);
            }
            das += draw[(size_t)e * K + k];
        }
        const float dloop = draw[(size_t)(E + j) * K + k];
        acc = fmaf(expf(lrelu(adst[(size_t)j * K + k] + as, slope) - mx[(size_t)j * K + k]) / den[(size_t)j * K + k],
                   gout[(size_t)j * H + c], acc);
        das += dloop;
        for (int s = t0; s < t1; ++s) dad += draw[(size_t)eid_dst[s] * K + k];
        dad += dloop;
        dz[(size_t)j * H + c] = fmaf(das, att[(size_t)k * 2 * D + D + d], fmaf(dad, att[(size_t)k * 2 * D + d], acc));
    }
}

inline int pow2_cover(int64_t n, int cap) {
    int g = 1;
    while (g < n && g < cap) g <<= 1;
    return g;
}

}  // namespace
}  // namespace cal

using namespace cal;

// call site: cal_amd/ops.py _GINWeightedAggregate.backward (d edge_weight of GINConv's weighted sum)
CAL_EXPORT int cal_edge_dot(const int32_t* row32, const int32_t* col32, const float* a, const float* b, float* out, int64_t N,
                            int64_t E, int64_t H, void* stream) {
    CAL_REQUIRE(N >= 0 && E >= 0 && H >= 0 && N < (1ll << 31) && E < (1ll << 31) && H < (1ll << 24), "bad sizes");
    if (E == 0) return 0;
    CAL_REQUIRE(row32 && col32 && out && (H == 0 || (a && b)), "null operand");
    const bool vec = H % 4 == 0 && aligned16(a) && aligned16(b);
    const int G = pow2_cover(vec ? H / 4 : H, 64);
    const int64_t blocks = (E * G + 255) / 256;
    CAL_REQUIRE(blocks < (1ll << 31), "too many columns for one launch");
    hipStream_t st = (hipStream_t)stream;
    if (vec) k_edge_dot<4><<<dim3((unsigned)blocks), dim3(256), 0, st>>>(row32, col32, a, b, out, E, (int)H, G);
    else k_edge_dot<1><<<dim3((unsigned)blocks), dim3(256), 0, st>>>(row32, col32, a, b, out, E, (int)H, G);
    CAL_CHECK_LAUNCH("k_edge_dot");
    return 0;
}

static int gatm_shape_ok(int64_t N, int64_t E, int64_t K, int64_t D) {
    return N >= 0 && E >= 0 && K > 0 && K <= 64 && D > 0 && K * D < (1ll << 20) && N < (1ll << 31) - 4 && E < (1ll << 31) &&
           (E + N) * K < (1ll << 40);
}

// call site: cal_amd/ops.py _GATMaskAggregate.forward
CAL_EXPORT int cal_gat_mask_fwd(const int32_t* rowptr_dst, const int32_t* nbr_dst, const int32_t* eid_dst, const float* z,
                                const float* att, const float* bias, int relu, float slope, const float* m, float* out, float* adst,
                                float* asrc, float* mx, float* den, int64_t N, int64_t E, int64_t K, int64_t D, void* stream) {
    CAL_REQUIRE(gatm_shape_ok(N, E, K, D), "bad shape (1 <= K <= 64, D >= 1)");
    if (N == 0) return 0;
    CAL_REQUIRE(rowptr_dst && z && att && out && adst && asrc && mx && den && (E == 0 || (nbr_dst && eid_dst && m)), "null operand");
    CAL_REQUIRE(z != out, "in-place aggregation is not supported");
    hipStream_t st = (hipStream_t)stream;
    k_gatm_scores<<<dim3((unsigned)cdiv(N * K, 256)), dim3(256), 0, st>>>(z, att, adst, asrc, N * K, (int)K, (int)D);
    CAL_CHECK_LAUNCH("k_gatm_scores");
    k_gatm_fwd<<<dim3((unsigned)cdiv(N, 4)), dim3(256), 0, st>>>(rowptr_dst, nbr_dst, eid_dst, z, bias, relu, slope, m, out, adst, asrc,
                                                                mx, den, (int)N, (int)K, (int)D);
    CAL_CHECK_LAUNCH("k_gatm_fwd");
    return 0;
}

// floats of workspace: d(raw score) of every slot, [(E + N), K] by column id (E + i: node i's loop)
CAL_EXPORT int64_t cal_gat_mask_bwd_ws(int64_t N, int64_t E, int64_t K, int64_t D) {
    (void)D;
    return (E + N) * K > 4 ? (E + N) * K : 4;
}

// call site: cal_amd/ops.py _GATMaskAggregate.backward
CAL_EXPORT int cal_gat_mask_bwd(const int32_t* rowptr_dst, const int32_t* nbr_dst, const int32_t* eid_dst, const int32_t* rowptr_src,
                                const int32_t* nbr_src, const int32_t* eid_src, const float* z, const float* att, const float* adst,
                                const float* asrc, const float* mx, const float* den, const float* gout, float slope, const float* m,
                                float* dz, float* dm, float* ws, int64_t N, int64_t E, int64_t K, int64_t D, void* stream) {
    CAL_REQUIRE(gatm_shape_ok(N, E, K, D), "bad shape (1 <= K <= 64, D >= 1)");
    hipStream_t st = (hipStream_t)stream;
    if (E > 0) {
        CAL_REQUIRE(dm != nullptr, "null operand");
        // columns outside the plan's CSR (input self loops) have no slot: their d m is 0; every other entry is overwritten below
        if (hipMemsetAsync(dm, 0, (size_t)E * sizeof(float), st) != hipSuccess) { set_error("cal_gat_mask_bwd: memset failed"); return 1; }
    }
    if (N == 0) return 0;
    CAL_REQUIRE(rowptr_dst && rowptr_src && z && att && adst && asrc && mx && den && gout && dz && ws &&
                (E == 0 || (nbr_dst && eid_dst && nbr_src && eid_src && m)), "null operand");
    const int G = pow2_cover(D, 64);
    k_gatm_bwd_dst<<<dim3((unsigned)cdiv(N, 4)), dim3(256), 0, st>>>(rowptr_dst, nbr_dst, eid_dst, z, adst, asrc, mx, den, gout, slope, m, ws,
                                                                    dm, (int)N, E, (int)K, (int)D, G);
    CAL_CHECK_LAUNCH("k_gatm_bwd_dst");
    k_gatm_bwd_src<<<dim3((unsigned)cdiv(N, 4)), dim3(256), 0, st>>>(rowptr_src, nbr_src, eid_src, rowptr_dst, eid_dst, att, adst, asrc, mx,
                                                                    den, gout, slope, m, ws, dz, (int)N, E, (int)K, (int)D);
    CAL_CHECK_LAUNCH("k_gatm_bwd_src");
    return 0;
}
