// Parametric edge explainer (cal_amd/pgexplain.py): a two-layer MLP on the embeddings of an edge's two
// end nodes, evaluated on gathered rows of the node projection PQ = x [W1a; W1b]^T + [b1; 0] (one cal_gemm), so that no [E, 2H]
// tensor exists at any point.
//
//   cal_edge_mlp_fwd   ONE launch: per player the gather of two or four PQ rows, add, ReLU, dot with w2, a cross-lane sum, the
//                      concrete sample, sigma, the scatter to one or two mask entries and the per-graph sums of the regularisers.
//   cal_edge_mlp_bwd   a memset and three launches: the column coefficients (k_edge_mlp_coef), the node rows of dPQ with the
//                      partials of dw2 / db2 (k_edge_mlp_rows: one wave per row, h_e recomputed), the finish of the partials.
//
// One workgroup per graph in the player kernels (the approach of maskopt.hip); every output element has one writer, the
// per-graph sums are taken in double in a fixed order, every row is summed in slot order and nothing is atomic: two calls on
// equal inputs give equal bits.
#include <math.h>

#include "cal_hip.h"
#include "common.hpp"
#include "segment.hpp"

namespace cal {
namespace {

constexpr int kMlpNT = 256;

// (what a player's z gives -- m = sigma(z), dm = m (1 - m), H(m) -- is logit_terms of rules.hpp, as in maskopt.hip;
// column_ok, mlp_rows_per_block and mlp_sizes_ok are there too)

// A group of G lanes serves one player, 256 / G players per pass of the workgroup over its graph.
template <int VEC, int G>
__global__ void __launch_bounds__(kMlpNT) k_edge_mlp_fwd(const float* __restrict__ pq, const float* __restrict__ w2,
                                                         const float* __restrict__ b2, const int32_t* __restrict__ row32,
                                                         const int32_t* __restrict__ col32, const int64_t* __restrict__ pptr,
                                                         const int32_t* __restrict__ rep, const int32_t* __restrict__ mate,
                                                         float* __restrict__ omega, float* __restrict__ zout,
                                                         float* __restrict__ mask, double* __restrict__ terms, int64_t N, int64_t E,
                                                         int Hd, int64_t P, float tau, unsigned long long seed,
                                                         unsigned long long step) {
    using V = Vec<VEC>;
    constexpr int PPB = kMlpNT / G;
    __shared__ double red[2 * (kMlpNT / 64)];
    const int grp = threadIdx.x / G, l = threadIdx.x % G;
    int64_t lo, n;
    seg_clamp(pptr, blockIdx.x, P, lo, n);
    const float bias = b2[0];
    const size_t ld = 2 * (size_t)Hd;
    double s_size = 0.0, s_ent = 0.0;
    for (int64_t i0 = 0; i0 < n; i0 += PPB) {                  // (uniform over the workgroup: every lane reaches the group sums)
        const int64_t i = i0 + grp;
        const bool act = i < n;
        const int64_t p = lo + (act ? i : 0);
        int ur, vr, ut, vt;
        const bool r_ok = act && column_ok(rep[p], row32, col32, E, N, ur, vr);
        const bool t_ok = r_ok && column_ok(mate[p], row32, col32, E, N, ut, vt);
        float ar = 0.f, at = 0.f;
        if (r_ok) {
            for (int c = l * VEC; c < Hd; c += G * VEC) {
                const V w = V::ld(w2 + c);
                V h = V::ld(pq + ur * ld + c);
                h.add(V::ld(pq + vr * ld + Hd + c));
                h.relu();
                ar += h.dot(w);
                if (t_ok) {
                    V k = V::ld(pq + ut * ld + c);
                    k.add(V::ld(pq + vt * ld + Hd + c));
                    k.relu();
                    at += k.dot(w);
                }
            }
        }
        ar = group_sum<G>(ar);
        at = group_sum<G>(at);
        if (act && l == 0) {
            float om = 0.f, z = 0.f;
            if (r_ok) {
                om = t_ok ? 0.5f * ((bias + ar) + (bias + at)) : bias + ar;
                float noise = 0.f;
                if (seed != 0ull) {
                    const unsigned long long h = splitmix64(splitmix64(seed) + ((step << 32) + (unsigned long long)p));
                    const float u = ((float)(h >> 41) + 0.5f) * (1.f / 8388608.f);      // exact, in (0, 1); so is 1 - u
                    noise = logf(u) - logf(1.f - u);
                }
                z = (noise + om) / tau;
                const Logit q = logit_terms(z);
                mask[rep[p]] = q.m;
                if (t_ok) mask[mate[p]] = q.m;
                s_size += (double)q.m;
                s_ent += (double)q.ent;
            }
            omega[p] = om;
            zout[p] = z;
        }
    }
    if (terms == nullptr) return;                             // (uniform over the grid)
    s_size = group_sum_d<64>(s_size);
    s_ent = group_sum_d<64>(s_ent);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[2 * w] = s_size; red[2 * w + 1] = s_ent; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0, b = 0.0;
        for (int k = 0; k < kMlpNT / 64; ++k) { a += red[2 * k]; b += red[2 * k + 1]; }
        terms[2 * (size_t)blockIdx.x] = a;
        terms[2 * (size_t)blockIdx.x + 1] = b;
    }
}

// c[e] of every player column (c is zeroed in front of this launch): one workgroup per graph strides over the graph's players
__global__ void __launch_bounds__(kMlpNT) k_edge_mlp_coef(const int32_t* __restrict__ row32, const int32_t* __restrict__ col32,
                                                          const int64_t* __restrict__ pptr, const int32_t* __restrict__ rep,
                                                          const int32_t* __restrict__ mate, const float* __restrict__ z,
                                                          const float* __restrict__ gmask, float* __restrict__ c, int64_t N,
                                                          int64_t E, int64_t P, float tau, float l_size, float l_ent) {
    int64_t lo, n;
    seg_clamp(pptr, blockIdx.x, P, lo, n);
    const float ent_w = n > 0 ? l_ent / (float)n : 0.f;
    for (int64_t i = threadIdx.x; i < n; i += kMlpNT) {
        const int64_t p = lo + i;
        int u, v;
        const int64_t r = rep[p], t = mate[p];
        if (!column_ok(r, row32, col32, E, N, u, v)) continue;
        const bool t_ok = column_ok(t, row32, col32, E, N, u, v);
        const float zz = z[p];
        const Logit q = logit_terms(zz);
        const float g = ((gmask[r] + (t_ok ? gmask[t] : 0.f) + (l_size - ent_w * zz)) * q.dm) / tau;
        if (t_ok) {
            c[r] = 0.5f * g;
            c[t] = 0.5f * g;
        } else {
            c[r] = g;
        }
    }
}

// The (up to) four hidden units of a lane: VEC = 4 the units 4 l .. 4 l + 3 by one 16-byte access, VEC = 1 the units l + 64 j.
template <int VEC>
struct Units {
    __device__ __forceinline__ static int unit(int l, int j) { return VEC == 4 ? 4 * l + j : l + 64 * j; }
    __device__ __forceinline__ static void ld(const float* __restrict__ p, int l, int Hd, float* o) {
        if constexpr (VEC == 4) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (4 * l < Hd) v = *reinterpret_cast<const float4*>(p + 4 * l);
            o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = l + 64 * j < Hd ? p[l + 64 * j] : 0.f;
        }
    }
    __device__ __forceinline__ static void st(float* __restrict__ p, int l, int Hd, const float* o) {
        if constexpr (VEC == 4) {
            if (4 * l < Hd) *reinterpret_cast<float4*>(p + 4 * l) = make_float4(o[0], o[1], o[2], o[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (l + 64 * j < Hd) p[l + 64 * j] = o[j];
        }
    }
};

// One CSR row of node n, summed in slot order: 64 slots' column id, coefficient and other end node are loaded at once, then
// taken one by one (wave-uniform).  SRC: the row's columns leave n (own = P_n, other = Q of the destination; dw2 and db2 are
// summed here, every column once); else they enter n (own = Q_n, other = P of the source).
template <int VEC, bool SRC>
__device__ __forceinline__ void mlp_row(const float* __restrict__ pq, const int32_t* __restrict__ ptr, const int32_t* __restrict__ eid,
                                        const int32_t* __restrict__ other, const float* __restrict__ c, const float* wk, int n, int64_t N,
                                        int64_t E, int Hd, int lane, float* acc, float* accw, float& accb) {
    using U = Units<VEC>;
    const size_t ld = 2 * (size_t)Hd;
    int beg = __builtin_amdgcn_readfirstlane(ptr[n]), end = __builtin_amdgcn_readfirstlane(ptr[n + 1]);     // (wave-uniform)
    beg = beg < 0 ? 0 : beg;
    end = end > (int)E ? (int)E : end;
    float own[4];
    U::ld(pq + (size_t)n * ld + (SRC ? 0 : Hd), lane, Hd, own);
    for (int s0 = beg; s0 < end; s0 += 64) {
        const int cnt = end - s0 < 64 ? end - s0 : 64;
        float c_l = 0.f;
        int o_l = 0;
        if (lane < cnt) {
            const int e = eid[s0 + lane];
            if (e >= 0 && e < E) {
                const int o = other[e];
                if (o >= 0 && o < N) { c_l = c[e]; o_l = o; }
            }
        }
        for (int j = 0; j < cnt; ++j) {
            const float ce = rdlane_f(c_l, j);
            if (ce == 0.f) continue;                            // (a column of no player: nothing to add)
            const int o = __builtin_amdgcn_readlane(o_l, j);
            float oth[4];
            U::ld(pq + (size_t)o * ld + (SRC ? Hd : 0), lane, Hd, oth);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float h = own[k] + oth[k];
                if (h > 0.f) {
                    acc[k] = fmaf(ce, wk[k], acc[k]);
                    if (SRC) accw[k] = fmaf(ce, h, accw[k]);
                }
            }
            if (SRC) accb += ce;
        }
    }
}

// dpq rows and the partials of dw2 / db2.  Workgroup b owns the nodes [b rpb, (b + 1) rpb), its wave w every fourth of them from
// the w-th on; part [nblocks, Hd + 4]: columns [0, Hd) dw2, column Hd db2 (the four wave partials in wave order).
template <int VEC>
__global__ void __launch_bounds__(kMlpNT) k_edge_mlp_rows(const float* __restrict__ pq, const float* __restrict__ w2,
                                                          const int32_t* __restrict__ row32, const int32_t* __restrict__ col32,
                                                          const int32_t* __restrict__ ptr_src, const int32_t* __restrict__ eid_src,
                                                          const int32_t* __restrict__ ptr_dst, const int32_t* __restrict__ eid_dst,
                                                          const float* __restrict__ c, float* __restrict__ dpq,
                                                          float* __restrict__ part, int64_t N, int64_t E, int Hd, int rpb) {
    using U = Units<VEC>;
    __shared__ float sw[kMlpNT / 64][260];
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t r0 = (int64_t)blockIdx.x * rpb, r1 = r0 + rpb < N ? r0 + rpb : N;
    const size_t ld = 2 * (size_t)Hd;
    float wk[4], accw[4] = {0.f, 0.f, 0.f, 0.f}, accb = 0.f;
    U::ld(w2, lane, Hd, wk);
    for (int64_t n = r0 + w; n < r1; n += kMlpNT / 64) {
        float ap[4] = {0.f, 0.f, 0.f, 0.f}, aq[4] = {0.f, 0.f, 0.f, 0.f};
        mlp_row<VEC, true>(pq, ptr_src, eid_src, col32, c, wk, (int)n, N, E, Hd, lane, ap, accw, accb);
        mlp_row<VEC, false>(pq, ptr_dst, eid_dst, row32, c, wk, (int)n, N, E, Hd, lane, aq, accw, accb);
        U::st(dpq + (size_t)n * ld, lane, Hd, ap);
        U::st(dpq + (size_t)n * ld + Hd, lane, Hd, aq);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int k = U::unit(lane, j);
        if (k < Hd) sw[w][k] = accw[j];
    }
    if (lane == 0) sw[w][Hd] = accb;
    __syncthreads();
    for (int k = threadIdx.x; k <= Hd; k += kMlpNT)
        part[(size_t)blockIdx.x * (Hd + 4) + k] = ((sw[0][k] + sw[1][k]) + sw[2][k]) + sw[3][k];
}

// dw2 [Hd], db2 [1] from the partials
__global__ void __launch_bounds__(256) k_edge_mlp_finish(const float* __restrict__ part, int nparts, int Hd, float* __restrict__ dw2,
                                                         float* __restrict__ db2) {
    __shared__ float red[256];
    const int c = blockIdx.x * 16 + (threadIdx.x & 15);
    const float s = finish_colsum(part, nparts, Hd + 4, c, c <= Hd, red);
    if ((threadIdx.x >> 4) != 0 || c > Hd) return;
    if (c < Hd) dw2[c] = s;
    else db2[0] = s;
}

}  // namespace
}  // namespace cal

using namespace cal;

// call site: cal_amd/ops.py _EdgeMlpMask.forward
CAL_EXPORT int cal_edge_mlp_fwd(const float* pq, const float* w2, const float* b2, const int32_t* row32, const int32_t* col32,
                                const int64_t* pptr, const int32_t* rep, const int32_t* mate, float* omega, float* z, float* mask,
                                double* terms, int64_t N, int64_t E, int64_t Hd, int64_t B, int64_t P, float tau, uint64_t seed,
                                int64_t step, void* stream) {
    CAL_REQUIRE(mlp_sizes_ok(N, E, Hd, B, P), "bad sizes (Hd: a multiple of 4 in [4, 256])");
    CAL_REQUIRE(tau > 0.f && step >= 0 && step < (1ll << 31), "tau must be > 0, step in [0, 2^31)");
    if (B == 0 || P == 0) return 0;
    CAL_REQUIRE(pq && w2 && b2 && row32 && col32 && pptr && rep && mate && omega && z && mask, "null operand");
    const bool vec_ok = aligned16(pq) && aligned16(w2);
    CAL_DISPATCH_VG((int)Hd, vec_ok, {
        hipLaunchKernelGGL((k_edge_mlp_fwd<VEC, G>), dim3((unsigned)B), dim3(kMlpNT), 0, (hipStream_t)stream, pq, w2, b2, row32, col32,
                           pptr, rep, mate, omega, z, mask, terms, N, E, (int)Hd, P, tau, (unsigned long long)seed,
                           (unsigned long long)step);
    });
    CAL_CHECK_LAUNCH("k_edge_mlp_fwd");
    return 0;
}

CAL_EXPORT int64_t cal_edge_mlp_bwd_ws(int64_t N, int64_t E, int64_t Hd) {
    // c [E] + partials
    const int64_t nb = N <= 0 ? 1 : cdiv(N, mlp_rows_per_block(N));
    return (E + 3) / 4 * 4 + nb * (Hd + 4) + 16;
}

// call site: cal_amd/ops.py _EdgeMlpMask.backward
CAL_EXPORT int cal_edge_mlp_bwd(const float* pq, const float* w2, const int32_t* row32, const int32_t* col32,
                                const int32_t* rowptr_src, const int32_t* eid_src, const int32_t* rowptr_dst, const int32_t* eid_dst,
                                const int64_t* pptr, const int32_t* rep, const int32_t* mate, const float* z, const float* gmask,
                                float* dpq, float* dw2, float* db2, float* ws, int64_t N, int64_t E, int64_t Hd, int64_t B, int64_t P,
                                float tau, float l_size, float l_ent, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CAL_REQUIRE(mlp_sizes_ok(N, E, Hd, B, P), "bad sizes (Hd: a multiple of 4 in [4, 256])");
    CAL_REQUIRE(tau > 0.f, "tau must be > 0");
    if (B == 0 || P == 0) return 0;
    CAL_REQUIRE(pq && w2 && row32 && col32 && rowptr_src && eid_src && rowptr_dst && eid_dst && pptr && rep && mate && z && gmask &&
                    dpq && dw2 && db2 && ws, "null operand");
    const int rpb = mlp_rows_per_block(N);
    const int nb = N == 0 ? 0 : cdiv(N, rpb);
    float* c = ws;
    float* part = ws + (E + 3) / 4 * 4;
    if (E > 0) {
        if (hipMemsetAsync(c, 0, (size_t)E * sizeof(float), stream) != hipSuccess) {
            set_error("cal_edge_mlp_bwd: memset failed");
            return 1;
        }
        hipLaunchKernelGGL(k_edge_mlp_coef, dim3((unsigned)B), dim3(kMlpNT), 0, stream, row32, col32, pptr, rep, mate, z, gmask, c, N, E,
                           P, tau, l_size, l_ent);
        CAL_CHECK_LAUNCH("k_edge_mlp_coef");
    }
    if (N > 0) {
        if (aligned16(pq) && aligned16(w2) && aligned16(dpq))
            hipLaunchKernelGGL((k_edge_mlp_rows<4>), dim3(nb), dim3(kMlpNT), 0, stream, pq, w2, row32, col32, rowptr_src, eid_src,
                               rowptr_dst, eid_dst, c, dpq, part, N, E, (int)Hd, rpb);
        else
            hipLaunchKernelGGL((k_edge_mlp_rows<1>), dim3(nb), dim3(kMlpNT), 0, stream, pq, w2, row32, col32, rowptr_src, eid_src,
                               rowptr_dst, eid_dst, c, dpq, part, N, E, (int)Hd, rpb);
        CAL_CHECK_LAUNCH("k_edge_mlp_rows");
    }
    hipLaunchKernelGGL(k_edge_mlp_finish, dim3(cdiv(Hd + 1, 16)), dim3(256), 0, stream, part, nb, (int)Hd, dw2, db2);
    CAL_CHECK_LAUNCH("k_edge_mlp_finish");
    return 0;
}
