// libcalhost -- HOST (CPU) implementation of the operator-level entry points of include/cal_hip.h, behind the same
// symbol names and argument lists ("each also has a host implementation behind the same symbol set
// so the boundary is testable in a GPU-less container"; BASELINE.json configs[0] is the reference's CPU plumbing run).
//
// Plain C++17 loops over the same GraphPlan structures the HIP kernels consume -- no HIP, no torch, nothing from
// oracle/.  Pointers are HOST pointers, `stream` is ignored, `ws` / `part` workspaces are accepted and left untouched.
// cal_amd selects this library by tensor residency (CPU tensors -> libcalhost, CUDA tensors -> libcalhip); data on the
// GPU never comes here and a missing libcalhip.so is an error, not a reason to run on the host.
//
// Every function cites the reference call site it stands for, like its HIP twin (cal_amd/csrc/*.hip): the formulas,
// the slot order of the plan (by edge id inside a row) and the summation order of every segment reduction are the
// same, so host and device agree to fp32 rounding.  The rules whose results the two libraries promise bit for bit -- hashes, keys,
// clamps, selection counts, plans, replica rules -- are not restated here: both sides read them from cal_amd/csrc/rules.hpp.
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <cstdlib>
#include <vector>

#include "cal_hip.h"
#include "rules.hpp"

using namespace cal;

#define HOST_EXPORT extern "C" __attribute__((visibility("default")))

namespace {

thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
#define HOST_REQUIRE(cond, msg) do { if (!(cond)) { set_error("%s: %s", __func__, msg); return 2; } } while (0)

}  // namespace

HOST_EXPORT const char* cal_last_error() { return g_err; }
HOST_EXPORT int cal_version() { return 100; }

// ---- GraphPlan (remove_self_loops / add_self_loops of GCNConv.norm, gcn_conv.py:56-63; the scatter index of
// MessagePassing.propagate, gcn_conv.py:92): counting sort of the edges by destination and by source, slots of a
// row in edge-id order, explicit self loops dropped, the N added loops implicit.
HOST_EXPORT int cal_plan_build(const int64_t* edge_index, int64_t E, int64_t N, int32_t* rowptr_dst, int32_t* nbr_dst,
                               int32_t* eid_dst, int32_t* rowptr_src, int32_t* nbr_src, int32_t* eid_src, int32_t* row32,
                               int32_t* col32, int32_t* work, int32_t* status, void*) {
    HOST_REQUIRE(N >= 0 && E >= 0 && N < (1ll << 31) && E < (1ll << 31), "N/E out of int32 range");
    (void)work;
    *status = 0;
    std::fill(rowptr_dst, rowptr_dst + N + 1, 0);
    std::fill(rowptr_src, rowptr_src + N + 1, 0);
    for (int64_t e = 0; e < E; ++e) {
        const int64_t r = edge_index[e], c = edge_index[E + e];
        if (r < 0 || r >= N || c < 0 || c >= N) {        // the reference would raise an index error
            *status |= 1;
            row32[e] = 0; col32[e] = 0;                     // treated as a dropped self loop
            continue;
        }
        row32[e] = (int32_t)r; col32[e] = (int32_t)c;
        if (r != c) { rowptr_dst[c + 1]++; rowptr_src[r + 1]++; }
    }
    for (int64_t v = 0; v < N; ++v) { rowptr_dst[v + 1] += rowptr_dst[v]; rowptr_src[v + 1] += rowptr_src[v]; }
    std::vector<int32_t> cd(rowptr_dst, rowptr_dst + N), cs(rowptr_src, rowptr_src + N);
    for (int64_t e = 0; e < E; ++e) {                       // ascending edge id = the slot order inside every row
        const int32_t r = row32[e], c = col32[e];
        if (r == c) continue;
        const int32_t p = cd[c]++, q = cs[r]++;
        nbr_dst[p] = r; eid_dst[p] = (int32_t)e;
        nbr_src[q] = c; eid_src[q] = (int32_t)e;
    }
    return 0;
}

// node offsets of every graph from the sorted `batch` vector (the Batch object of train_causal.py:174)
HOST_EXPORT int cal_graph_ptr(const int64_t* batch, int64_t N, int64_t B, int32_t* gptr, int32_t* status, void*) {
    HOST_REQUIRE(N >= 0 && B >= 0 && N < (1ll << 31), "bad sizes");
    int64_t prev = -1;
    for (int64_t i = 0; i <= N; ++i) {
        const int64_t cur = i == N ? B : batch[i];
        if (i < N && (cur < prev || cur >= B || cur < 0)) { *status |= 2; continue; }
        for (int64_t b = prev + 1; b <= cur && b <= B; ++b) gptr[b] = (int32_t)i;
        prev = cur;
    }
    return 0;
}

// ---- GCNConv.norm (gcn_conv.py:44-70): deg over the source index incl. the added loop, dis = deg^-1/2 (inf -> 0),
// norm_e = dis[row] w dis[col] in original edge order (0 on dropped self-loop edges)
HOST_EXPORT int cal_gcn_norm_fwd(const int32_t* rowptr_src, const int32_t* eid_src, const int32_t* row32, const int32_t* col32,
                                 const float* w, float loop_w, int64_t N, int64_t E, float* dis, float* norm_e, void*) {
#pragma omp parallel for schedule(static)
    for (int64_t v = 0; v < N; ++v) {
        float d = 0.f;
        if (w) for (int s = rowptr_src[v]; s < rowptr_src[v + 1]; ++s) d += w[eid_src[s]];
        else d = (float)(rowptr_src[v + 1] - rowptr_src[v]);
        d += loop_w;
        dis[v] = d == 0.f ? 0.f : 1.0f / sqrtf(d);
    }
#pragma omp parallel for schedule(static)
    for (int64_t e = 0; e < E; ++e) {
        const int r = row32[e], c = col32[e];
        norm_e[e] = r != c ? dis[r] * (w ? w[e] : 1.f) * dis[c] : 0.f;
    }
    return 0;
}

// ---- propagate + message + update (+ fused ReLU), gcn_conv.py:92-104 / model.py:95: by-destination CSR for the
// forward, by-source CSR for the gradient w.r.t. h (its transpose)
HOST_EXPORT int cal_spmm_fwd(const int32_t* rowptr, const int32_t* nbr, const int32_t* eid, const float* norm_e,
                             const float* dis, float loop_w, const float* h, const float* bias, int relu, float* out,
                             int64_t N, int64_t H, void*) {
    if (N == 0 || H == 0) return 0;
    HOST_REQUIRE(h != out, "in-place aggregation is not supported");
#pragma omp parallel for schedule(dynamic, 64)
    for (int64_t i = 0; i < N; ++i) {
        float* o = out + i * H;
        for (int64_t c = 0; c < H; ++c) o[c] = 0.f;
        for (int s = rowptr[i]; s < rowptr[i + 1]; ++s) {
            const float n = norm_e[eid[s]];
            const float* hj = h + (int64_t)nbr[s] * H;
            for (int64_t c = 0; c < H; ++c) o[c] = fmaf(n, hj[c], o[c]);
        }
        const float nself = dis[i] * loop_w * dis[i];
        const float* hi = h + i * H;
        for (int64_t c = 0; c < H; ++c) {
            float v = fmaf(nself, hi[c], o[c]);
            if (bias) v += bias[c];
            if (relu) v = v > 0.f ? v : 0.f;
            o[c] = v;
        }
    }
    return 0;
}

HOST_EXPORT int64_t cal_colsum_parts(int64_t) { return 1; }
// ReLU backward + bias gradient (gcn_conv.py:103, model.py:95): dz = dout * (y > 0), dbias = column sums of dz
HOST_EXPORT int cal_relu_bwd_colsum(const float* dout, const float* y, float* dz, float* dbias, float* part, int64_t N,
                                    int64_t H, void*) {
    (void)part;
    std::vector<double> acc(dbias ? H : 0, 0.0);
    for (int64_t r = 0; r < N; ++r)
        for (int64_t c = 0; c < H; ++c) {
            float g = dout[r * H + c];
            if (y && !(y[r * H + c] > 0.f)) g = 0.f;
            if (dz) dz[r * H + c] = g;
            if (dbias) acc[c] += g;
        }
    if (dbias) for (int64_t c = 0; c < H; ++c) dbias[c] = (float)acc[c];
    return 0;
}

// ---- gradient w.r.t. the edge weights through propagate AND through the normalisation (gcn_conv.py:63-70,97
// differentiated): gn_e[e] = <dz[col_e], h[row_e]>, gself[v] = <dz[v], h[v]>, d deg, dw in original edge order
HOST_EXPORT int cal_gcn_norm_bwd(const int32_t* rowptr_dst, const int32_t* nbr_dst, const int32_t* eid_dst,
                                 const int32_t* rowptr_src, const int32_t* nbr_src, const int32_t* eid_src, const int32_t* row32,
                                 const int32_t* col32, const float* w, const float* dis, float loop_w, const float* h,
                                 const float* dz, float* gn_e, float* gself, float* ddeg, float* dw, int64_t N, int64_t E,
                                 int64_t H, void*) {
#pragma omp parallel for schedule(dynamic, 64)
    for (int64_t i = 0; i < N; ++i) {
        const float* di = dz + i * H;
        for (int s = rowptr_dst[i]; s <= rowptr_dst[i + 1]; ++s) {
            const bool self = s == rowptr_dst[i + 1];
            const float* hj = h + (int64_t)(self ? i : nbr_dst[s]) * H;
            float p = 0.f;
            for (int64_t c = 0; c < H; ++c) p = fmaf(di[c], hj[c], p);
            if (self) gself[i] = p; else gn_e[eid_dst[s]] = p;
        }
    }
#pragma omp parallel for schedule(static)
    for (int64_t v = 0; v < N; ++v) {
        float acc = 0.f;
        for (int s = rowptr_src[v]; s < rowptr_src[v + 1]; ++s) { const int e = eid_src[s]; acc += gn_e[e] * (w ? w[e] : 1.f) * dis[nbr_src[s]]; }
        for (int s = rowptr_dst[v]; s < rowptr_dst[v + 1]; ++s) { const int e = eid_dst[s]; acc += gn_e[e] * (w ? w[e] : 1.f) * dis[nbr_dst[s]]; }
        const float d = dis[v];
        acc += 2.f * gself[v] * d * loop_w;
        ddeg[v] = -0.5f * d * d * d * acc;
    }
#pragma omp parallel for schedule(static)
    for (int64_t e = 0; e < E; ++e) {
        const int r = row32[e], c = col32[e];
        dw[e] = r != c ? gn_e[e] * dis[r] * dis[c] + ddeg[r] : 0.f;
    }
    return 0;
}

// ---- dense layers: x @ W (gcn_conv.py:75), torch.nn.Linear (model.py:46-75) and their gradients.
// C[M,N] = op(A) op(B) (+ bias[N]) (ReLU); transA: A stored [K,M]; transB: B stored [N,K]
HOST_EXPORT int64_t cal_gemm_ws(int64_t, int64_t, int64_t) { return 4; }
HOST_EXPORT int cal_gemm(int transA, int transB, const float* A, const float* B, float* C, const float* bias, int relu, float* ws,
                         int64_t M, int64_t N, int64_t K, void*) {
    (void)ws;
    if (M == 0 || N == 0) return 0;
#pragma omp parallel for schedule(static)
    for (int64_t m = 0; m < M; ++m) {
        float* c = C + m * N;
        if (transB) {                                       // B[n][k]: both operands contiguous along k
            for (int64_t n = 0; n < N; ++n) {
                const float* b = B + n * K;
                float acc = 0.f;
                if (transA) for (int64_t k = 0; k < K; ++k) acc = fmaf(A[k * M + m], b[k], acc);
                else { const float* a = A + m * K; for (int64_t k = 0; k < K; ++k) acc = fmaf(a[k], b[k], acc); }
                c[n] = acc;
            }
        } else {                                            // B[k][n]: axpy over rows of B
            for (int64_t n = 0; n < N; ++n) c[n] = 0.f;
            for (int64_t k = 0; k < K; ++k) {
                const float a = transA ? A[k * M + m] : A[m * K + k];
                const float* b = B + k * N;
                for (int64_t n = 0; n < N; ++n) c[n] = fmaf(a, b[n], c[n]);
            }
        }
        for (int64_t n = 0; n < N; ++n) {
            float v = c[n] + (bias ? bias[n] : 0.f);
            c[n] = relu ? (v > 0.f ? v : 0.f) : v;
        }
    }
    return 0;
}
HOST_EXPORT int cal_gemm_ks(int transB, const float* A, const float* B, float* C, const float* bias, int relu, int64_t M, int64_t N,
                            int64_t K, void* stream) {
    return cal_gemm(0, transB, A, B, C, bias, relu, nullptr, M, N, K, stream);
}

// ---- edge attention (model.py:97-104): softmax over 2 classes of Linear([x[row] || x[col]]) = P[row] + Q[col] + b with
// the per-node projections P = x W[:, :H]^T, Q = x W[:, H:]^T; att [2,E] (row 0 = edge_weight_c, row 1 = edge_weight_o)
HOST_EXPORT int cal_edge_att_fwd(const float* x, const float* W, const float* b, const int32_t* row32, const int32_t* col32,
                                 float* pq, float* att, int64_t N, int64_t E, int64_t H, void*) {
#pragma omp parallel for schedule(static)
    for (int64_t v = 0; v < N; ++v) {
        const float* xv = x + v * H;
        float p0 = 0.f, p1 = 0.f, q0 = 0.f, q1 = 0.f;
        for (int64_t c = 0; c < H; ++c) {
            p0 = fmaf(xv[c], W[c], p0); p1 = fmaf(xv[c], W[2 * H + c], p1);
            q0 = fmaf(xv[c], W[H + c], q0); q1 = fmaf(xv[c], W[3 * H + c], q1);
        }
        pq[4 * v] = p0; pq[4 * v + 1] = p1; pq[4 * v + 2] = q0; pq[4 * v + 3] = q1;
    }
#pragma omp parallel for schedule(static)
    for (int64_t e = 0; e < E; ++e) {
        const float* pr = pq + 4 * (int64_t)row32[e];
        const float* qc = pq + 4 * (int64_t)col32[e];
        const float l0 = pr[0] + qc[2] + b[0], l1 = pr[1] + qc[3] + b[1];
        const float m = fmaxf(l0, l1);
        const float e0 = expf(l0 - m), e1 = expf(l1 - m);
        const float inv = 1.f / (e0 + e1);
        att[e] = e0 * inv; att[E + e] = e1 * inv;
    }
    return 0;
}
HOST_EXPORT int64_t cal_edge_att_bwd_ws(int64_t, int64_t, int64_t) { return 4; }
HOST_EXPORT int cal_edge_att_bwd(const float* x, const float* W, const float* att, const float* datt, const int32_t* rowptr_src,
                                 const int32_t* eid_src, const int32_t* rowptr_dst, const int32_t* eid_dst, float* dx, int accumulate,
                                 float* dW, float* db, float* ws, int64_t N, int64_t E, int64_t H, void*) {
    (void)ws;
    // d logit_0 = a0 a1 (dA0 - dA1) per edge (d logit_1 = -d logit_0); self-loop edges are absent from the CSR and
    // their weights never reach a conv (gcn_conv.py:56)
    std::vector<float> dl(E > 0 ? E : 1);
    for (int64_t e = 0; e < E; ++e) dl[e] = att[e] * att[E + e] * (datt[e] - datt[E + e]);
    std::vector<double> aw(2 * H, 0.0);
    double sb = 0.0;
    for (int64_t v = 0; v < N; ++v) {
        float sp = 0.f, sq = 0.f;
        for (int s = rowptr_src[v]; s < rowptr_src[v + 1]; ++s) sp += dl[eid_src[s]];
        for (int s = rowptr_dst[v]; s < rowptr_dst[v + 1]; ++s) sq += dl[eid_dst[s]];
        const float* xv = x + v * H;
        float* d = dx + v * H;
        for (int64_t c = 0; c < H; ++c) {
            const float wp = W[c] - W[2 * H + c], wq = W[H + c] - W[3 * H + c];
            const float base = accumulate ? d[c] : 0.f;
            d[c] = fmaf(sq, wq, fmaf(sp, wp, base));
            aw[c] += (double)sp * xv[c];
            aw[H + c] += (double)sq * xv[c];
        }
        sb += sp;
    }
    for (int64_t c = 0; c < 2 * H; ++c) { dW[c] = (float)aw[c]; dW[2 * H + c] = -(float)aw[c]; }
    db[0] = (float)sb; db[1] = -(float)sb;
    return 0;
}

// ---- node attention + split (model.py:106-111): a = softmax2(x Wn^T + bn), xc = a0 x, xo = a1 x
HOST_EXPORT int cal_node_att_split_fwd(const float* x, const float* Wn, const float* bn, float* att_n, float* xc, float* xo, int64_t N,
                                       int64_t H, void*) {
#pragma omp parallel for schedule(static)
    for (int64_t v = 0; v < N; ++v) {
        const float* xv = x + v * H;
        float l0 = 0.f, l1 = 0.f;
        for (int64_t c = 0; c < H; ++c) { l0 = fmaf(xv[c], Wn[c], l0); l1 = fmaf(xv[c], Wn[H + c], l1); }
        l0 += bn[0]; l1 += bn[1];
        const float m = fmaxf(l0, l1);
        const float e0 = expf(l0 - m), e1 = expf(l1 - m);
        const float inv = 1.f / (e0 + e1), a0 = e0 * inv, a1 = e1 * inv;
        att_n[2 * v] = a0; att_n[2 * v + 1] = a1;
        for (int64_t c = 0; c < H; ++c) { xc[v * H + c] = a0 * xv[c]; xo[v * H + c] = a1 * xv[c]; }
    }
    return 0;
}
HOST_EXPORT int64_t cal_node_att_bwd_ws(int64_t, int64_t) { return 4; }
HOST_EXPORT int cal_node_att_split_bwd(const float* x, const float* Wn, const float* att_n, const float* dxc, const float* dxo, float* dx,
                                       float* dWn, float* dbn, float* ws, int64_t N, int64_t H, void*) {
    (void)ws;
    std::vector<double> aw(H, 0.0);
    double sb = 0.0;
    for (int64_t v = 0; v < N; ++v) {
        const float a0 = att_n[2 * v], a1 = att_n[2 * v + 1];
        const float* xv = x + v * H;
        float d0 = 0.f, d1 = 0.f;
        for (int64_t c = 0; c < H; ++c) { d0 = fmaf(dxc[v * H + c], xv[c], d0); d1 = fmaf(dxo[v * H + c], xv[c], d1); }
        const float dl0 = a0 * a1 * (d0 - d1);              // d logit_0 (softmax2 backward); d logit_1 = -dl0
        for (int64_t c = 0; c < H; ++c) {
            dx[v * H + c] = a0 * dxc[v * H + c] + a1 * dxo[v * H + c] + dl0 * (Wn[c] - Wn[H + c]);
            aw[c] += (double)dl0 * xv[c];
        }
        sb += dl0;
    }
    for (int64_t c = 0; c < H; ++c) { dWn[c] = (float)aw[c]; dWn[H + c] = -(float)aw[c]; }
    dbn[0] = (float)sb; dbn[1] = -(float)sb;
    return 0;
}

// ---- global_add_pool (model.py:115-116, 403-404): batch is sorted, so a graph is the node segment [gptr[b], gptr[b+1])
HOST_EXPORT int cal_add_pool_fwd(const float* x, const int32_t* gptr, float* out, float* part, int64_t B, int64_t H, int64_t S, void*) {
    (void)part; (void)S;
#pragma omp parallel for schedule(static)
    for (int64_t b = 0; b < B; ++b) {
        float* o = out + b * H;
        for (int64_t c = 0; c < H; ++c) o[c] = 0.f;
        for (int v = gptr[b]; v < gptr[b + 1]; ++v)
            for (int64_t c = 0; c < H; ++c) o[c] += x[(int64_t)v * H + c];
    }
    return 0;
}
HOST_EXPORT int cal_add_pool_bwd(const float* dout, const int64_t* batch, float* dx, int64_t N, int64_t H, void*) {
#pragma omp parallel for schedule(static)
    for (int64_t v = 0; v < N; ++v) memcpy(dx + v * H, dout + batch[v] * H, sizeof(float) * H);
    return 0;
}

// ---- GATConv(hidden, hidden / heads, heads, dropout = p) of PyG (call sites model.py:340,390), after z = x W:
//   a_dst[i,k] = <z[i,k,:], att[k,:D]>, a_src[j,k] = <z[j,k,:], att[k,D:]>, e = LeakyReLU(a_dst[i] + a_src[j]),
//   alpha = softmax over the incoming edges of i (input self loops dropped, one loop per node added),
//   exp(e - max) / (sum + 1e-16); alpha~ = alpha keep / (1 - p) in training; out[i,k,:] = sum_j alpha~ z[j,k,:] + bias
HOST_EXPORT int cal_gat_fwd(const int32_t* rowptr, const int32_t* nbr, const int32_t* eid, const float* z, const float* att,
                            const float* bias, int relu, float slope, float p, uint64_t seed, float* out, float* adst, float* asrc,
                            float* mx, float* den, int64_t N, int64_t E, int64_t K, int64_t D, void*) {
    HOST_REQUIRE(K > 0 && D > 0, "bad head shape");
    HOST_REQUIRE(p >= 0.f && p < 1.f, "dropout p must be in [0,1)");
    const int64_t H = K * D;
    const float inv_keep = p > 0.f ? 1.f / (1.f - p) : 1.f;
#pragma omp parallel for schedule(static)
    for (int64_t t = 0; t < N * K; ++t) {
        const int64_t k = t % K;
        const float* zp = z + t * D;
        float sd = 0.f, ss = 0.f;
        for (int64_t d = 0; d < D; ++d) { sd = fmaf(zp[d], att[k * 2 * D + d], sd); ss = fmaf(zp[d], att[k * 2 * D + D + d], ss); }
        adst[t] = sd; asrc[t] = ss;
    }
#pragma omp parallel for schedule(dynamic, 64)
    for (int64_t i = 0; i < N; ++i)
        for (int64_t k = 0; k < K; ++k) {
            const float ad = adst[i * K + k];
            const float eself = lrelu(ad + asrc[i * K + k], slope);
            float m = eself;
            for (int s = rowptr[i]; s < rowptr[i + 1]; ++s) m = fmaxf(m, lrelu(ad + asrc[(int64_t)nbr[s] * K + k], slope));
            float* o = out + i * H + k * D;
            for (int64_t d = 0; d < D; ++d) o[d] = 0.f;
            float lsum = 0.f;
            for (int s = rowptr[i]; s <= rowptr[i + 1]; ++s) {
                const bool self = s == rowptr[i + 1];
                const int64_t j = self ? i : nbr[s];
                const float pe = expf((self ? eself : lrelu(ad + asrc[j * K + k], slope)) - m);
                lsum += pe;
                const float wgt = pe * keep_scale(seed, self ? E + i : (int64_t)eid[s], (int)k, (int)K, p, inv_keep);
                const float* zj = z + j * H + k * D;
                for (int64_t d = 0; d < D; ++d) o[d] = fmaf(wgt, zj[d], o[d]);
            }
            const float dn = lsum + 1e-16f;
            for (int64_t d = 0; d < D; ++d) {
                float v = o[d] / dn + (bias ? bias[k * D + d] : 0.f);
                o[d] = relu ? (v > 0.f ? v : 0.f) : v;
            }
            mx[i * K + k] = m; den[i * K + k] = dn;
        }
    return 0;
}
HOST_EXPORT int64_t cal_gat_bwd_ws(int64_t, int64_t, int64_t, int64_t) { return 4; }
// gout: gradient at the layer output (already masked by the ReLU if one was fused).  dz [N,K*D], datt [K,2D].
HOST_EXPORT int cal_gat_bwd(const int32_t* rowptr_dst, const int32_t* nbr_dst, const int32_t* eid_dst, const int32_t* rowptr_src,
                            const int32_t* nbr_src, const int32_t* eid_src, const float* z, const float* att, const float* adst,
                            const float* asrc, const float* mx, const float* den, const float* gout, float slope, float p,
                            uint64_t seed, float* dz, float* datt, float* ws, int64_t N, int64_t E, int64_t K, int64_t D, void*) {
    (void)ws;
    const int64_t H = K * D;
    const float inv_keep = p > 0.f ? 1.f / (1.f - p) : 1.f;
    std::vector<float> draw((size_t)(E + N) * K, 0.f), dadst((size_t)N * K, 0.f), dasrc((size_t)N * K, 0.f);
    // by destination: d(raw logit) of every incoming slot (softmax + LeakyReLU backward), its row sum = d a_dst
#pragma omp parallel for schedule(dynamic, 64)
    for (int64_t i = 0; i < N; ++i)
        for (int64_t k = 0; k < K; ++k) {
            const float ad = adst[i * K + k], m = mx[i * K + k], dn = den[i * K + k];
            const float* gi = gout + i * H + k * D;
            const int s0 = rowptr_dst[i], s1 = rowptr_dst[i + 1];
            float S = 0.f;
            for (int s = s0; s <= s1; ++s) {
                const bool self = s == s1;
                const int64_t j = self ? i : nbr_dst[s], id = self ? E + i : (int64_t)eid_dst[s];
                const float* zj = z + j * H + k * D;
                float dot = 0.f;
                for (int64_t d = 0; d < D; ++d) dot = fmaf(gi[d], zj[d], dot);
                const float alpha = expf(lrelu(ad + asrc[j * K + k], slope) - m) / dn;
                const float dalpha = dot * keep_scale(seed, id, (int)k, (int)K, p, inv_keep);
                S = fmaf(alpha, dalpha, S);
                draw[id * K + k] = dalpha;
            }
            float rowsum = 0.f;
            for (int s = s0; s <= s1; ++s) {
                const bool self = s == s1;
                const int64_t j = self ? i : nbr_dst[s], id = self ? E + i : (int64_t)eid_dst[s];
                const float raw = ad + asrc[j * K + k];
                const float alpha = expf(lrelu(raw, slope) - m) / dn;
                const float dr = alpha * (draw[id * K + k] - S) * (raw > 0.f ? 1.f : slope);
                rowsum += dr;
                draw[id * K + k] = dr;
            }
            dadst[i * K + k] = rowsum;
        }
    // by source: dz[j] = sum over the edges leaving j (and its loop) of alpha~ g[dst] + d a_dst att[:D] + d a_src att[D:]
#pragma omp parallel for schedule(dynamic, 64)
    for (int64_t j = 0; j < N; ++j)
        for (int64_t k = 0; k < K; ++k) {
            const float as = asrc[j * K + k];
            float* o = dz + j * H + k * D;
            for (int64_t d = 0; d < D; ++d) o[d] = 0.f;
            float das = 0.f;
            const int s0 = rowptr_src[j], s1 = rowptr_src[j + 1];
            for (int s = s0; s <= s1; ++s) {
                const bool self = s == s1;
                const int64_t i = self ? j : nbr_src[s], id = self ? E + j : (int64_t)eid_src[s];
                const float alpha = expf(lrelu(adst[i * K + k] + as, slope) - mx[i * K + k]) / den[i * K + k];
                const float wgt = alpha * keep_scale(seed, id, (int)k, (int)K, p, inv_keep);
                const float* gi = gout + i * H + k * D;
                for (int64_t d = 0; d < D; ++d) o[d] = fmaf(wgt, gi[d], o[d]);
                das += draw[id * K + k];
            }
            dasrc[j * K + k] = das;
            const float dad = dadst[j * K + k];
            for (int64_t d = 0; d < D; ++d) o[d] = fmaf(das, att[k * 2 * D + D + d], fmaf(dad, att[k * 2 * D + d], o[d]));
        }
    // d att[k,:D] = sum_v d a_dst[v,k] z[v,k,:], d att[k,D:] = sum_v d a_src[v,k] z[v,k,:]
    std::vector<double> acc((size_t)2 * H, 0.0);
    for (int64_t v = 0; v < N; ++v)
        for (int64_t k = 0; k < K; ++k) {
            const double da = dadst[v * K + k], ds = dasrc[v * K + k];
            const float* zv = z + v * H + k * D;
            for (int64_t d = 0; d < D; ++d) { acc[k * 2 * D + d] += da * zv[d]; acc[k * 2 * D + D + d] += ds * zv[d]; }
        }
    for (int64_t c = 0; c < 2 * H; ++c) datt[c] = (float)acc[c];
    return 0;
}
// keep mask (1/0) as floats, [E + N, K]: row e < E for original edge e, row E + i for node i's loop
HOST_EXPORT int cal_gat_dropout_mask(uint64_t seed, int64_t E, int64_t N, int64_t K, float p, float* mask, void*) {
    for (int64_t t = 0; t < (E + N) * K; ++t) mask[t] = keep_scale(seed, t / K, (int)(t % K), (int)K, p, 1.f);
    return 0;
}

// ---- soft edge masks (cal_amd/csrc/softmask.hip; cal_amd/gradient.py): the same formulas, sums in slot order.
// out[e] = <a[col[e]], b[row[e]]>, exactly 0 for a self-loop column: d/dw_e of GINConv's weighted sum
HOST_EXPORT int cal_edge_dot(const int32_t* row32, const int32_t* col32, const float* a, const float* b, float* out, int64_t N,
                             int64_t E, int64_t H, void*) {
    HOST_REQUIRE(N >= 0 && E >= 0 && H >= 0, "bad sizes");
#pragma omp parallel for schedule(static)
    for (int64_t e = 0; e < E; ++e) {
        const int r = row32[e], c = col32[e];
        float p = 0.f;
        if (r != c) for (int64_t h = 0; h < H; ++h) p = fmaf(a[(int64_t)c * H + h], b[(int64_t)r * H + h], p);
        out[e] = p;
    }
    return 0;
}

// GATConv with a mask m >= 0 by column inside the edge softmax (no dropout): alpha = m exp(e - max) / (sum m exp(e - max) + 1e-16),
// the added loop at weight 1, max over the loop and the columns with m > 0
HOST_EXPORT int cal_gat_mask_fwd(const int32_t* rowptr, const int32_t* nbr, const int32_t* eid, const float* z, const float* att,
                                 const float* bias, int relu, float slope, const float* m, float* out, float* adst, float* asrc,
                                 float* mx, float* den, int64_t N, int64_t E, int64_t K, int64_t D, void*) {
    HOST_REQUIRE(N >= 0 && E >= 0 && K > 0 && K <= 64 && D > 0, "bad shape (1 <= K <= 64, D >= 1)");
    const int64_t H = K * D;
#pragma omp parallel for schedule(static)
    for (int64_t t = 0; t < N * K; ++t) {
        const int64_t k = t % K;
        const float* zp = z + t * D;
        float sd = 0.f, ss = 0.f;
        for (int64_t d = 0; d < D; ++d) { sd = fmaf(zp[d], att[k * 2 * D + d], sd); ss = fmaf(zp[d], att[k * 2 * D + D + d], ss); }
        adst[t] = sd; asrc[t] = ss;
    }
#pragma omp parallel for schedule(dynamic, 64)
    for (int64_t i = 0; i < N; ++i)
        for (int64_t k = 0; k < K; ++k) {
            const float ad = adst[i * K + k];
            const float eself = lrelu(ad + asrc[i * K + k], slope);
            float mv = eself;
            for (int s = rowptr[i]; s < rowptr[i + 1]; ++s)
                if (m[eid[s]] > 0.f) mv = fmaxf(mv, lrelu(ad + asrc[(int64_t)nbr[s] * K + k], slope));
            float* o = out + i * H + k * D;
            for (int64_t d = 0; d < D; ++d) o[d] = 0.f;
            float lsum = 0.f;
            for (int s = rowptr[i]; s <= rowptr[i + 1]; ++s) {
                const bool self = s == rowptr[i + 1];
                const int64_t j = self ? i : nbr[s];
                const float ms = self ? 1.f : m[eid[s]];
                if (!(ms > 0.f)) continue;
                const float wgt = ms * expf((self ? eself : lrelu(ad + asrc[j * K + k], slope)) - mv);
                lsum += wgt;
                const float* zj = z + j * H + k * D;
                for (int64_t d = 0; d < D; ++d) o[d] = fmaf(wgt, zj[d], o[d]);
            }
            const float dn = lsum + 1e-16f;
            for (int64_t d = 0; d < D; ++d) {
                const float v = o[d] / dn + (bias ? bias[k * D + d] : 0.f);
                o[d] = relu ? (v > 0.f ? v : 0.f) : v;
            }
            mx[i * K + k] = mv; den[i * K + k] = dn;
        }
    return 0;
}
HOST_EXPORT int64_t cal_gat_mask_bwd_ws(int64_t, int64_t, int64_t, int64_t) { return 4; }
// gout: gradient at the layer output (already masked by the ReLU if one was fused).  dz [N, K*D]; dm [E], 0 for a column
// outside the CSR (an input self loop).  max is a constant.
HOST_EXPORT int cal_gat_mask_bwd(const int32_t* rowptr_dst, const int32_t* nbr_dst, const int32_t* eid_dst, const int32_t* rowptr_src,
                                 const int32_t* nbr_src, const int32_t* eid_src, const float* z, const float* att, const float* adst,
                                 const float* asrc, const float* mx, const float* den, const float* gout, float slope, const float* m,
                                 float* dz, float* dm, float* ws, int64_t N, int64_t E, int64_t K, int64_t D, void*) {
    (void)ws;
    HOST_REQUIRE(N >= 0 && E >= 0 && K > 0 && K <= 64 && D > 0, "bad shape (1 <= K <= 64, D >= 1)");
    const int64_t H = K * D;
    std::vector<float> draw((size_t)(E + N) * K, 0.f);
    for (int64_t e = 0; e < E; ++e) dm[e] = 0.f;
#pragma omp parallel for schedule(dynamic, 64)
    for (int64_t i = 0; i < N; ++i) {
        const int s0 = rowptr_dst[i], s1 = rowptr_dst[i + 1];
        std::vector<float> S((size_t)K, 0.f);
        for (int64_t k = 0; k < K; ++k) {
            const float ad = adst[i * K + k], mk = mx[i * K + k], dn = den[i * K + k];
            const float* gi = gout + i * H + k * D;
            float acc = 0.f;
            for (int s = s0; s <= s1; ++s) {
                const bool self = s == s1;
                const int64_t j = self ? i : nbr_dst[s];
                const float ms = self ? 1.f : m[eid_dst[s]];
                if (!(ms > 0.f)) continue;
                const float* zj = z + j * H + k * D;
                float dot = 0.f;
                for (int64_t d = 0; d < D; ++d) dot = fmaf(gi[d], zj[d], dot);
                acc = fmaf(ms * expf(lrelu(ad + asrc[j * K + k], slope) - mk) / dn, dot, acc);
            }
            S[k] = acc;
        }
        for (int s = s0; s <= s1; ++s) {
            const bool self = s == s1;
            const int64_t j = self ? i : nbr_dst[s], id = self ? E + i : (int64_t)eid_dst[s];
            const float ms = self ? 1.f : m[id];
            float dmacc = 0.f;
            for (int64_t k = 0; k < K; ++k) {
                const float* gi = gout + i * H + k * D;
                const float* zj = z + j * H + k * D;
                float dot = 0.f;
                for (int64_t d = 0; d < D; ++d) dot = fmaf(gi[d], zj[d], dot);
                const float raw = adst[i * K + k] + asrc[j * K + k];
                const float q = expf(lrelu(raw, slope) - mx[i * K + k]) / den[i * K + k];
                const float alpha = ms > 0.f ? ms * q : 0.f;
                draw[id * K + k] = alpha * (dot - S[k]) * (raw > 0.f ? 1.f : slope);
                dmacc += q * (dot - S[k]);
            }
            if (!self) dm[id] = dmacc;
        }
    }
#pragma omp parallel for schedule(dynamic, 64)
    for (int64_t j = 0; j < N; ++j)
        for (int64_t k = 0; k < K; ++k) {
            const float as = asrc[j * K + k];
            float* o = dz + j * H + k * D;
            for (int64_t d = 0; d < D; ++d) o[d] = 0.f;
            float das = 0.f, dad = 0.f;
            const int s0 = rowptr_src[j], s1 = rowptr_src[j + 1];
            for (int s = s0; s <= s1; ++s) {
                const bool self = s == s1;
                const int64_t i = self ? j : nbr_src[s], id = self ? E + j : (int64_t)eid_src[s];
                const float ms = self ? 1.f : m[id];
                if (ms > 0.f) {
                    const float alpha = ms * expf(lrelu(adst[i * K + k] + as, slope) - mx[i * K + k]) / den[i * K + k];
                    const float* gi = gout + i * H + k * D;
                    for (int64_t d = 0; d < D; ++d) o[d] = fmaf(alpha, gi[d], o[d]);
                }
                das += draw[id * K + k];
            }
            for (int s = rowptr_dst[j]; s < rowptr_dst[j + 1]; ++s) dad += draw[(int64_t)eid_dst[s] * K + k];
            dad += draw[(E + j) * K + k];
            for (int64_t d = 0; d < D; ++d) o[d] = fmaf(das, att[k * 2 * D + D + d], fmaf(dad, att[k * 2 * D + d], o[d]));
        }
    return 0;
}

// ---- learned masks (cal_amd/csrc/maskopt.hip; cal_amd/maskopt.py): the same formulas in fp32, the per-graph sums in double in the
// kernel's order -- 256 strided lane partials, a butterfly per 64 of them, the four wave partials in order
namespace {
inline double lanes_total(double* v) {                        // [256], destroyed
    for (int w = 0; w < 4; ++w)
        for (int o = 32; o > 0; o >>= 1)
            for (int l = 0; l < o; ++l) v[64 * w + l] += v[64 * w + l + o];
    return ((v[0] + v[64]) + v[128]) + v[192];
}
}  // namespace

HOST_EXPORT int cal_mask_step(const int64_t* pptr, const int32_t* rep, const int32_t* mate, const float* grad, float* theta,
                              float* exp_avg, float* exp_avg_sq, float* mask, double* terms, int64_t B, int64_t P, int64_t M,
                              int32_t step, float lr, float beta1, float beta2, float eps, float l_size, float l_ent, void*) {
    HOST_REQUIRE(B >= 0 && P >= 0 && M >= 0 && step >= 0, "bad sizes");
    if (B == 0 || P == 0) return 0;
    HOST_REQUIRE(pptr && rep && mate && theta && (M == 0 || mask), "null operand");
    HOST_REQUIRE(step == 0 || (grad && exp_avg && exp_avg_sq), "a step >= 1 needs grad and both moments");
    HOST_REQUIRE(step == 0 || (beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f), "betas must be in [0, 1)");
    float step_size = 0.f, rsq2 = 1.f;
    if (step > 0) {
        step_size = (float)((double)lr / (1.0 - pow((double)beta1, (double)step)));
        rsq2 = (float)(1.0 / sqrt(1.0 - pow((double)beta2, (double)step)));
    }
    for (int64_t g = 0; g < B; ++g) {
        int64_t lo, n;
        seg_clamp(pptr, g, P, lo, n);
        const float ent_w = n > 0 ? l_ent / (float)n : 0.f;
        double s_size[256] = {0.0}, s_ent[256] = {0.0};
        for (int64_t i = 0; i < n; ++i) {
            const int64_t p = lo + i;
            const int64_t r = rep[p], t = mate[p];
            const bool r_ok = r >= 0 && r < M, t_ok = t >= 0 && t < M;
            float th = theta[p];
            Logit q = logit_terms(th);
            s_size[i & 255] += (double)q.m;
            s_ent[i & 255] += (double)q.ent;
            if (step > 0) {
                // dL/dtheta = (dL_pred/dm of the player's elements + d size/dm + d entropy/dm) dm/dtheta
                const float gr = ((r_ok ? grad[r] : 0.f) + (t_ok ? grad[t] : 0.f) + (l_size - ent_w * th)) * q.dm;
                const float m1 = beta1 * exp_avg[p] + (1.f - beta1) * gr;
                const float m2 = beta2 * exp_avg_sq[p] + (1.f - beta2) * gr * gr;
                th -= step_size * (m1 / (sqrtf(m2) * rsq2 + eps));
                exp_avg[p] = m1;
                exp_avg_sq[p] = m2;
                theta[p] = th;
                q = logit_terms(th);
            }
            if (r_ok) mask[r] = q.m;
            if (t_ok) mask[t] = q.m;
        }
        if (terms) {
            terms[2 * g] = lanes_total(s_size);
            terms[2 * g + 1] = lanes_total(s_ent);
        }
    }
    return 0;
}

// ---- parametric edge explainer (cal_amd/csrc/edgemlp.hip; cal_amd/pgexplain.py): the same formulas in fp32 -- a column's dot
// product over the hidden units in order, a node's row sums in slot order, dw2 / db2 through the kernel's per-block, per-wave
// partials -- the per-graph sums in double
namespace {
inline float column_omega(const float* pq, const float* w2, float b2, int64_t u, int64_t v, int64_t Hd) {
    float a = 0.f;
    for (int64_t k = 0; k < Hd; ++k) a = fmaf(fmaxf(pq[u * 2 * Hd + k] + pq[v * 2 * Hd + Hd + k], 0.f), w2[k], a);
    return b2 + a;
}
}  // namespace

HOST_EXPORT int cal_edge_mlp_fwd(const float* pq, const float* w2, const float* b2, const int32_t* row32, const int32_t* col32,
                                 const int64_t* pptr, const int32_t* rep, const int32_t* mate, float* omega, float* z, float* mask,
                                 double* terms, int64_t N, int64_t E, int64_t Hd, int64_t B, int64_t P, float tau, uint64_t seed,
                                 int64_t step, void*) {
    HOST_REQUIRE(mlp_sizes_ok(N, E, Hd, B, P), "bad sizes (Hd: a multiple of 4 in [4, 256])");
    HOST_REQUIRE(tau > 0.f && step >= 0 && step < (1ll << 31), "tau must be > 0, step in [0, 2^31)");
    if (B == 0 || P == 0) return 0;
    HOST_REQUIRE(pq && w2 && b2 && row32 && col32 && pptr && rep && mate && omega && z && mask, "null operand");
    for (int64_t g = 0; g < B; ++g) {
        int64_t lo, n;
        seg_clamp(pptr, g, P, lo, n);
        double s_size = 0.0, s_ent = 0.0;
        for (int64_t p = lo; p < lo + n; ++p) {
            int ur, vr, ut, vt;
            float om = 0.f, zz = 0.f;
            if (column_ok(rep[p], row32, col32, E, N, ur, vr)) {
                const bool t_ok = column_ok(mate[p], row32, col32, E, N, ut, vt);
                om = column_omega(pq, w2, b2[0], ur, vr, Hd);
                if (t_ok) om = 0.5f * (om + column_omega(pq, w2, b2[0], ut, vt, Hd));
                float noise = 0.f;
                if (seed != 0) {
                    const uint64_t h = splitmix64(splitmix64(seed) + (((uint64_t)step << 32) + (uint64_t)p));
                    const float u = ((float)(h >> 41) + 0.5f) * (1.f / 8388608.f);
                    noise = logf(u) - logf(1.f - u);
                }
                zz = (noise + om) / tau;
                const Logit q = logit_terms(zz);
                mask[rep[p]] = q.m;
                if (t_ok) mask[mate[p]] = q.m;
                s_size += (double)q.m;
                s_ent += (double)q.ent;
            }
            omega[p] = om;
            z[p] = zz;
        }
        if (terms) { terms[2 * g] = s_size; terms[2 * g + 1] = s_ent; }
    }
    return 0;
}

HOST_EXPORT int64_t cal_edge_mlp_bwd_ws(int64_t, int64_t, int64_t) { return 4; }

HOST_EXPORT int cal_edge_mlp_bwd(const float* pq, const float* w2, const int32_t* row32, const int32_t* col32,
                                 const int32_t* rowptr_src, const int32_t* eid_src, const int32_t* rowptr_dst, const int32_t* eid_dst,
                                 const int64_t* pptr, const int32_t* rep, const int32_t* mate, const float* z, const float* gmask,
                                 float* dpq, float* dw2, float* db2, float* ws, int64_t N, int64_t E, int64_t Hd, int64_t B, int64_t P,
                                 float tau, float l_size, float l_ent, void*) {
    (void)ws;
    HOST_REQUIRE(mlp_sizes_ok(N, E, Hd, B, P), "bad sizes (Hd: a multiple of 4 in [4, 256])");
    HOST_REQUIRE(tau > 0.f, "tau must be > 0");
    if (B == 0 || P == 0) return 0;
    HOST_REQUIRE(pq && w2 && row32 && col32 && rowptr_src && eid_src && rowptr_dst && eid_dst && pptr && rep && mate && z && gmask &&
                     dpq && dw2 && db2, "null operand");
    std::vector<float> c((size_t)(E > 0 ? E : 1), 0.f);
    for (int64_t g = 0; g < B; ++g) {
        int64_t lo, n;
        seg_clamp(pptr, g, P, lo, n);
        const float ent_w = n > 0 ? l_ent / (float)n : 0.f;
        for (int64_t p = lo; p < lo + n; ++p) {
            int u, v;
            const int64_t r = rep[p], t = mate[p];
            if (!column_ok(r, row32, col32, E, N, u, v)) continue;
            const bool t_ok = column_ok(t, row32, col32, E, N, u, v);
            const Logit q = logit_terms(z[p]);
            const float gr = ((gmask[r] + (t_ok ? gmask[t] : 0.f) + (l_size - ent_w * z[p])) * q.dm) / tau;
            if (t_ok) { c[r] = 0.5f * gr; c[t] = 0.5f * gr; }
            else c[r] = gr;
        }
    }
    // the kernel's partials: workgroup b owns rpb nodes, its wave w every fourth of them; a block's partial is its four waves' in
    // order, the total the blocks' in order
    const int rpb = mlp_rows_per_block(N);
    std::vector<float> tot((size_t)Hd + 1, 0.f), wave(4 * ((size_t)Hd + 1));
    for (int64_t r0 = 0; r0 < N; r0 += rpb) {
        std::fill(wave.begin(), wave.end(), 0.f);
        const int64_t r1 = r0 + rpb < N ? r0 + rpb : N;
        for (int64_t n = r0; n < r1; ++n) {
            float* aw = wave.data() + ((n - r0) & 3) * (Hd + 1);
            float* dp = dpq + n * 2 * Hd;
            std::fill(dp, dp + 2 * Hd, 0.f);
            for (int side = 0; side < 2; ++side) {
                const int32_t* ptr = side == 0 ? rowptr_src : rowptr_dst;
                const int32_t* eid = side == 0 ? eid_src : eid_dst;
                const int32_t* other = side == 0 ? col32 : row32;
                int64_t beg = ptr[n], end = ptr[n + 1];
                beg = beg < 0 ? 0 : beg;
                end = end > E ? E : end;
                const float* own = pq + n * 2 * Hd + (side == 0 ? 0 : Hd);
                for (int64_t s = beg; s < end; ++s) {
                    const int64_t e = eid[s];
                    if (e < 0 || e >= E) continue;
                    const int64_t o = other[e];
                    if (o < 0 || o >= N || c[e] == 0.f) continue;
                    const float ce = c[e];
                    const float* oth = pq + o * 2 * Hd + (side == 0 ? Hd : 0);
                    for (int64_t k = 0; k < Hd; ++k) {
                        const float h = own[k] + oth[k];
                        if (h > 0.f) {
                            dp[side * Hd + k] = fmaf(ce, w2[k], dp[side * Hd + k]);
                            if (side == 0) aw[k] = fmaf(ce, h, aw[k]);
                        }
                    }
                    if (side == 0) aw[Hd] += ce;
                }
            }
        }
        for (int64_t k = 0; k <= Hd; ++k)
            tot[k] += ((wave[k] + wave[Hd + 1 + k]) + wave[2 * (Hd + 1) + k]) + wave[3 * (Hd + 1) + k];
    }
    for (int64_t k = 0; k < Hd; ++k) dw2[k] = tot[k];
    db2[0] = tot[Hd];
    return 0;
}

// Batch.from_data_list for graphs that live in ONE host-side concatenation (train_causal.py:13-15; cal_amd/data.py::_HostConcat):
// features copied, edge_index rebased by the running node offset, batch vector and labels written.  Same entry point as
// libcalhip.so (collate.hip) -- it only ever sees host pointers, so a machine with the host library alone serves DataLoader too.
HOST_EXPORT int cal_collate_host(const float* X, const int64_t* EI, int64_t Etot, int64_t F, const int64_t* node_ptr,
                                 const int64_t* edge_ptr, const int64_t* Y, const int64_t* idx, int64_t B, float* xo,
                                 int64_t* eio, int64_t Eout, int64_t* batcho, int64_t* yo) {
    HOST_REQUIRE(X && EI && node_ptr && edge_ptr && Y && idx && xo && eio && batcho && yo && B >= 0 && F > 0, "bad arguments");
    // offsets of every member graph first (serial, B additions), then the copies -- 128 scattered graphs of a 10 MB dataset are
    // ~0.7 MB of cache-missing reads: 120 us on one core, the largest piece of a host-collated step (0.34 ms against 0.22 ms on
    // the GPU) -- over a few threads (a fixed small team: the work is 100 us, the caller's loop runs it every 0.3 ms)
    std::vector<int64_t> noff((size_t)B + 1), eoff((size_t)B + 1);
    noff[0] = 0; eoff[0] = 0;
    for (int64_t b = 0; b < B; ++b) {
        const int64_t g = idx[b];
        const int64_t nn = node_ptr[g + 1] - node_ptr[g], ne = edge_ptr[g + 1] - edge_ptr[g];
        HOST_REQUIRE(nn >= 0 && ne >= 0 && eoff[b] + ne <= Eout, "offsets out of range");
        noff[b + 1] = noff[b] + nn; eoff[b + 1] = eoff[b] + ne;
    }
    const int64_t edges = eoff[B];
    static const int team_max = [] { const char* v = getenv("CAL_HOST_COLLATE_THREADS"); const int n = v ? atoi(v) : 4; return n < 1 ? 1 : n; }();
    const int team = B >= 32 ? team_max : 1;
#pragma omp parallel for schedule(static) num_threads(team) if (team > 1)
    for (int64_t b = 0; b < B; ++b) {
        const int64_t g = idx[b];
        const int64_t nb = node_ptr[g], nn = node_ptr[g + 1] - nb, eb = edge_ptr[g], ne = edge_ptr[g + 1] - eb;
        const int64_t nodes = noff[b], e0 = eoff[b];
        std::copy(X + nb * F, X + (nb + nn) * F, xo + nodes * F);
        const int64_t* src = EI + eb;
        const int64_t* dst = EI + Etot + eb;
        for (int64_t k = 0; k < ne; ++k) { eio[e0 + k] = src[k] + nodes; eio[Eout + e0 + k] = dst[k] + nodes; }
        std::fill(batcho + nodes, batcho + nodes + nn, b);
        yo[b] = Y[g];
    }
    HOST_REQUIRE(edges == Eout, "edge count mismatch");
    return 0;
}

// ---- explanations (model.py:97-111 edge / node scores): per-segment ranking, top-k selection, motif metrics.  Same keys,
// order, k_g rule and integer rank sums as cal_amd/csrc/explain.hip, so masks, ranks and metrics agree bit for bit.
namespace {
constexpr int64_t kExplainLdsCap = 2048;
}  // namespace

HOST_EXPORT int64_t cal_explain_ws(int64_t M, int64_t) { return 8 * (M > 0 ? M : 0) + 256; }
HOST_EXPORT int64_t cal_explain_lds_cap(void) { return kExplainLdsCap; }

HOST_EXPORT int cal_explain_rank(const float* score, int64_t stride, const int64_t* seg_ptr, int64_t B, int64_t M,
                                 int64_t max_seg, double ratio, int64_t k, const uint8_t* gt, uint8_t* mask, int32_t* rank,
                                 double* metrics, void*, int64_t, void*) {
    HOST_REQUIRE(B >= 0 && M >= 0 && max_seg >= 0 && stride >= 1, "B, M, max_seg must be >= 0 and stride >= 1");
    HOST_REQUIRE(k >= -2, "k must be >= 0, -1 (ratio) or -2 (ground-truth count)");
    HOST_REQUIRE(k != -2 || gt, "k = -2 needs gt");
    HOST_REQUIRE(k != -1 || ratio >= 0.0, "k = -1 needs a ratio >= 0");
    HOST_REQUIRE(B == 0 || seg_ptr, "seg_ptr is null");
    HOST_REQUIRE(M == 0 || (score && mask && rank), "score / mask / rank are null");
    HOST_REQUIRE(max_seg < ((int64_t)1 << 30), "segments of 2^30 elements or more are not supported");
#pragma omp parallel for schedule(dynamic, 16)
    for (int64_t g = 0; g < B; ++g) {
        int64_t lo, m;
        seg_clamp(seg_ptr, g, M, lo, m);
        double* row = metrics ? metrics + 4 * g : nullptr;
        if (m > max_seg) {                                    // not ranked (max_seg must bound every segment)
            for (int64_t q = 0; q < m; ++q) { rank[lo + q] = -1; mask[lo + q] = 0; }
            if (row) for (int t = 0; t < 4; ++t) row[t] = NAN;
            continue;
        }
        std::vector<uint32_t> key(m);
        std::vector<int64_t> ord(m);
        int64_t P = 0;
        for (int64_t q = 0; q < m; ++q) {
            key[q] = score_key(score[(lo + q) * stride]);
            ord[q] = q;
            if (gt) P += gt[lo + q] != 0;
        }
        std::sort(ord.begin(), ord.end(), [&](int64_t a, int64_t b) { return key[a] != key[b] ? key[a] > key[b] : a < b; });
        const int64_t kg = sel_count(m, P, ratio, k);
        int64_t hits = 0, r2 = 0;
        for (int64_t s = 0; s < m;) {                         // runs of equal keys: [s, e)
            int64_t e = s + 1;
            while (e < m && key[ord[e]] == key[ord[s]]) ++e;
            const int64_t eq = e - s, less = m - e;
            for (int64_t p = s; p < e; ++p) {
                const int64_t i = lo + ord[p];
                rank[i] = (int32_t)p;
                mask[i] = p < kg;
                if (gt && gt[i]) { hits += p < kg; r2 += 2 * less + eq + 1; }
            }
            s = e;
        }
        if (row) {
            row[0] = (double)kg; row[1] = (double)hits; row[2] = (double)P;
            row[3] = seg_auc(m, P, r2);
        }
    }
    return 0;
}

// ---- subgraph extraction: keep masks -> the compacted (and optionally relabelled) batch, order preserved.  The same rules
// as cal_amd/csrc/subgraph.hip (an edge that leaves its graph's node range is dropped); every integer output agrees bit for bit.
HOST_EXPORT int64_t cal_subgraph_ws(int64_t N, int64_t E, int64_t B) {
    N = N > 0 ? N : 0;
    E = E > 0 ? E : 0;
    B = B > 0 ? B : 0;
    return 16 * B + 8 * N + N + E + 256;
}

HOST_EXPORT int cal_subgraph_extract(const int64_t* edge_index, int64_t E, int64_t N, const int64_t* ptr, const int64_t* edge_ptr,
                                     int64_t B, const uint8_t* edge_keep, const uint8_t* node_keep, int complement, int relabel,
                                     const float* x, int64_t F, int64_t* edge_index_out, int64_t* ptr_out, int64_t* edge_ptr_out,
                                     int64_t* batch_out, float* x_out, int64_t* node_map, int64_t* edge_map, int64_t* totals,
                                     void*, int64_t, void*) {
    HOST_REQUIRE(E >= 0 && N >= 0 && B >= 0 && F >= 0, "E, N, B, F must be >= 0");
    HOST_REQUIRE(totals && ptr_out && edge_ptr_out, "totals / ptr_out / edge_ptr_out are null");
    HOST_REQUIRE(B == 0 || (ptr && edge_ptr), "ptr / edge_ptr are null");
    HOST_REQUIRE(E == 0 || (edge_index && edge_index_out && edge_map), "edge_index / edge_index_out / edge_map are null");
    HOST_REQUIRE(!relabel || N == 0 || (node_map && batch_out), "relabel needs node_map and batch_out");
    HOST_REQUIRE(!x_out || (x && relabel && F > 0), "x_out needs x, F > 0 and relabel");
    const bool comp = complement != 0, from_edges = relabel && !node_keep;
    std::vector<uint8_t> nflag(N, 0), eflag(E, 0);
    std::vector<int64_t> newid(N, 0), src, dst;
    src.reserve(E);
    dst.reserve(E);
    int64_t nt = 0, et = 0, mn = 0, me = 0;
    for (int64_t g = 0; g < B; ++g) {
        int64_t nlo, nn, elo, em;
        seg_clamp(ptr, g, N, nlo, nn);
        seg_clamp(edge_ptr, g, E, elo, em);
        const int64_t nhi = nlo + nn, ehi = elo + em;
        if (node_keep)
            for (int64_t i = nlo; i < nhi; ++i) nflag[i] = (node_keep[i] != 0) != comp;
        else if (from_edges)
            for (int64_t i = nlo; i < nhi; ++i) nflag[i] = 0;
        for (int64_t e = elo; e < ehi; ++e) {
            const int64_t s = edge_index[e], d = edge_index[E + e];
            bool k = s >= nlo && s < nhi && d >= nlo && d < nhi;
            if (k && edge_keep) k = (edge_keep[e] != 0) != comp;
            if (k && node_keep) k = nflag[s] && nflag[d];
            eflag[e] = k;
            if (k && from_edges) nflag[s] = nflag[d] = 1;
        }
        ptr_out[g] = std::min(nt, N);
        edge_ptr_out[g] = std::min(et, E);
        int64_t nc = 0, ec = 0;
        for (int64_t i = nlo; i < nhi; ++i) {
            if (relabel && !nflag[i]) continue;
            const int64_t p = relabel ? nt + nc : i;
            ++nc;
            newid[i] = p;
            if (p >= N) continue;
            if (node_map) node_map[p] = i;
            if (batch_out) batch_out[p] = g;
            if (relabel && x_out)
                for (int64_t c = 0; c < F; ++c) x_out[p * F + c] = x[i * F + c];
        }
        for (int64_t e = elo; e < ehi; ++e) {
            if (!eflag[e]) continue;
            const int64_t p = et + ec;
            ++ec;
            if (p >= E) continue;
            const int64_t s = edge_index[e], d = edge_index[E + e];
            src.push_back(relabel ? newid[s] : s);
            dst.push_back(relabel ? newid[d] : d);
            edge_map[p] = e;
        }
        nt += nc;
        et += ec;
        mn = std::max(mn, nc);
        me = std::max(me, ec);
    }
    const int64_t Nt = std::min(nt, N), Et = std::min(et, E);
    for (int64_t p = 0; p < Et; ++p) {                         // row 1 starts at E': a contiguous [2, E']
        edge_index_out[p] = src[p];
        edge_index_out[Et + p] = dst[p];
    }
    ptr_out[B] = Nt;
    edge_ptr_out[B] = Et;
    totals[0] = Nt; totals[1] = Et; totals[2] = mn; totals[3] = me;
    return 0;
}

// ---- undirected explanations: the reverse-edge map and the ranking of edge pairs.  The same pairing rule, representatives,
// symmetrised scores and compaction order as cal_amd/csrc/twin.hip and explain.hip, so every output agrees bit for bit.
HOST_EXPORT int64_t cal_edge_twin_ws(int64_t E, int64_t B) { return 32 * (B > 0 ? B : 0) + 12 * (E > 0 ? E : 0) + 256; }

HOST_EXPORT int cal_edge_twin(const int64_t* edge_index, int64_t E, const int64_t* ptr, const int64_t* edge_ptr, int64_t B,
                              int64_t max_edges, int32_t* twin, int64_t* totals, void*, int64_t, void*) {
    HOST_REQUIRE(E >= 0 && B >= 0 && max_edges >= 0, "E, B, max_edges must be >= 0");
    HOST_REQUIRE(E < ((int64_t)1 << 31), "2^31 columns or more are not supported (twin is int32)");
    HOST_REQUIRE(totals, "totals is null");
    HOST_REQUIRE(B == 0 || (ptr && edge_ptr), "ptr / edge_ptr are null");
    HOST_REQUIRE(E == 0 || (edge_index && twin), "edge_index / twin are null");
    int64_t unp = 0, nself = 0;
    std::vector<std::pair<uint64_t, int64_t>> keys;
    for (int64_t g = 0; g < B; ++g) {
        const int64_t nlo = ptr[g], nn = std::max(ptr[g + 1] - nlo, (int64_t)0);
        int64_t elo, em;
        seg_clamp(edge_ptr, g, E, elo, em);
        const int64_t ehi = elo + em;
        if (em > max_edges) {
            for (int64_t e = elo; e < ehi; ++e) twin[e] = -1;
            unp += em;
            continue;
        }
        keys.clear();
        for (int64_t e = elo; e < ehi; ++e) {
            const int64_t u = edge_index[e], v = edge_index[E + e];
            twin[e] = -1;
            if (u < nlo || u >= nlo + nn || v < nlo || v >= nlo + nn) continue;
            if (u == v) { twin[e] = (int32_t)e; ++nself; continue; }
            keys.emplace_back(und_edge_key((uint64_t)(u - nlo), (uint64_t)(v - nlo), (uint64_t)nn, u > v), e);
        }
        std::sort(keys.begin(), keys.end());                  // by key, then column index
        for (size_t s = 0; s < keys.size();) {                 // one undirected edge: its (u < v) columns, then its (u > v) columns
            const uint64_t und = keys[s].first >> 1;
            size_t mid = s, end;
            while (mid < keys.size() && keys[mid].first == (und << 1)) ++mid;
            end = mid;
            while (end < keys.size() && keys[end].first == ((und << 1) | 1)) ++end;
            const size_t np = std::min(mid - s, end - mid);
            for (size_t j = 0; j < np; ++j) {
                twin[keys[s + j].second] = (int32_t)keys[mid + j].second;
                twin[keys[mid + j].second] = (int32_t)keys[s + j].second;
            }
            s = end;
        }
        for (int64_t e = elo; e < ehi; ++e) unp += twin[e] < 0;
    }
    totals[0] = unp;
    totals[1] = nself;
    return 0;
}

HOST_EXPORT int64_t cal_explain_pairs_ws(int64_t M, int64_t B) {
    return 14 * (M > 0 ? M : 0) + 8 * (B > 0 ? B : 0) + 512 + cal_explain_ws(M, B);
}

HOST_EXPORT int cal_explain_rank_pairs(const float* score, int64_t stride, const int64_t* seg_ptr, int64_t B, int64_t M,
                                       int64_t max_seg, double ratio, int64_t k, const uint8_t* gt, const int32_t* twin,
                                       int reduce, float* score_out, uint8_t* mask, int32_t* rank, double* metrics, void*,
                                       int64_t, void*) {
    HOST_REQUIRE(B >= 0 && M >= 0 && max_seg >= 0 && stride >= 1, "B, M, max_seg must be >= 0 and stride >= 1");
    HOST_REQUIRE(k >= -2, "k must be >= 0, -1 (ratio) or -2 (ground-truth count)");
    HOST_REQUIRE(k != -2 || gt, "k = -2 needs gt");
    HOST_REQUIRE(k != -1 || ratio >= 0.0, "k = -1 needs a ratio >= 0");
    HOST_REQUIRE(reduce >= 0 && reduce <= 2, "reduce must be 0 (mean), 1 (max) or 2 (min)");
    HOST_REQUIRE(B == 0 || seg_ptr, "seg_ptr is null");
    HOST_REQUIRE(M == 0 || (score && twin && score_out && mask && rank), "score / twin / score_out / mask / rank are null");
    HOST_REQUIRE(M < ((int64_t)1 << 31), "2^31 columns or more are not supported (twin is int32)");
    // the representatives of every segment, compacted in order into one contiguous batch of segments
    std::vector<float> cs;
    std::vector<uint8_t> cgt, cmask;
    std::vector<int32_t> crank;
    std::vector<int64_t> cptr(B + 1, 0), rep(M, -1), lens(B, 0);
    int64_t longest = 0;
    for (int64_t g = 0; g < B; ++g) {
        int64_t lo, m;
        seg_clamp(seg_ptr, g, M, lo, m);
        const int64_t hi = lo + m;
        const bool bad = m > max_seg;
        for (int64_t e = lo; e < hi; ++e) {
            int64_t t = twin[e];
            if (!(t >= lo && t < hi && t != e && twin[t] == e)) t = -1;
            float sym = score[e * stride];
            uint8_t pos = gt ? gt[e] != 0 : 0;
            if (t >= 0) {
                const float o = score[t * stride], x = e < t ? sym : o, y = e < t ? o : sym;
                if (reduce == 0) sym = (x + y) * 0.5f;
                else if (x != x || y != y) sym = NAN;
                else if (reduce == 1) sym = x >= y ? x : y;
                else sym = x <= y ? x : y;
                if (gt) pos |= gt[t] != 0;
            }
            score_out[e] = sym;
            rep[e] = t >= 0 && t < e ? t : e;
            if (bad || rep[e] != e) continue;
            cs.push_back(sym);
            cgt.push_back(pos);
        }
        // a segment that is not ranked keeps its length, so the ranking below marks it (NaN metrics)
        if (bad) { cs.resize(cs.size() + m, 0.f); cgt.resize(cgt.size() + m, 0); }
        cptr[g + 1] = (int64_t)cs.size();
        lens[g] = cptr[g + 1] - cptr[g];
        if (!bad) longest = std::max(longest, lens[g]);
    }
    const int64_t Mc = (int64_t)cs.size();
    cmask.resize(Mc);
    crank.resize(Mc);
    const int rc = cal_explain_rank(cs.data(), 1, cptr.data(), B, Mc, std::min(max_seg, std::max(longest, (int64_t)0)), ratio, k,
                                    gt ? cgt.data() : nullptr, cmask.data(), crank.data(), metrics, nullptr, 0, nullptr);
    if (rc != 0) return rc;
    for (int64_t g = 0; g < B; ++g) {
        int64_t lo, m;
        seg_clamp(seg_ptr, g, M, lo, m);
        const int64_t hi = lo + m;
        const bool bad = m > max_seg;
        int64_t p = cptr[g];
        for (int64_t e = lo; e < hi; ++e) {                    // (a representative comes before its partner)
            if (bad) { rank[e] = -1; mask[e] = 0; continue; }
            if (rep[e] == e) { rep[e] = p++; rank[e] = crank[rep[e]]; mask[e] = cmask[rep[e]]; }
            else { const int64_t r = rep[rep[e]]; rank[e] = crank[r]; mask[e] = cmask[r]; }
        }
    }
    return 0;
}

// ---- the batch builders (cal_amd/csrc/rebatch.hpp: splice, occlusion, coalition, noise and subset replicas): what their count and
// write entry points share.
namespace {
// the count side: result graph r has n nodes and m columns; finish(R) after the last one
struct BatchScan {
    int64_t* ptr_out; int64_t* edge_ptr_out; int64_t* totals;
    int64_t nt = 0, et = 0, mn = 0, me = 0, empty = 0;
    void add(int64_t r, int64_t n, int64_t m) {
        ptr_out[r] = nt;
        edge_ptr_out[r] = et;
        nt += n;
        et += m;
        mn = std::max(mn, n);
        me = std::max(me, m);
        empty += n == 0;
    }
    void finish(int64_t R) {
        ptr_out[R] = nt;
        edge_ptr_out[R] = et;
        totals[0] = nt; totals[1] = et; totals[2] = mn; totals[3] = me; totals[4] = empty;
    }
};
// the write side: the next node / column of result graph r, after begin(r); nothing is written at or beyond Nout / Eout
struct OutWriter {
    int64_t Nout, Eout, F; const int64_t* ptr_out; const int64_t* edge_ptr_out;
    int64_t* batch_out; float* x_out; int64_t* edge_index_out; int64_t* node_src; int64_t* edge_src;
    int64_t r = 0, n0 = 0, i = 0, j = 0;
    void begin(int64_t r_) { r = r_; i = n0 = ptr_out[r]; j = edge_ptr_out[r]; }
    void node(int64_t code, const float* x, int64_t s) {      // (row s of x)
        if (i >= Nout) return;
        batch_out[i] = r;
        node_src[i] = code;
        if (x_out) memcpy(x_out + i * F, x + s * F, sizeof(float) * (size_t)F);
        ++i;
    }
    void col(int64_t u, int64_t v, int64_t code) {
        if (j >= Eout) return;
        edge_index_out[j] = u;
        edge_index_out[Eout + j] = v;
        edge_src[j] = code;
        ++j;
    }
};
}  // namespace

// the checks of a write entry point on what it fills (HOST_REQUIRE names the entry point), x_ok / x_msg its own on the features;
// then W, the writer
#define HOST_REQUIRE_WRITE(R, x_ok, x_msg)                                                                                       \
    HOST_REQUIRE(Nout >= 0 && Eout >= 0 && F >= 0 && F < (1 << 22), "Nout, Eout must be >= 0 and 0 <= F < 2^22");                \
    HOST_REQUIRE(R == 0 || (ptr_out && edge_ptr_out), "ptr_out / edge_ptr_out are null");                                        \
    HOST_REQUIRE(Nout == 0 || (batch_out && node_src), "batch_out / node_src are null");                                         \
    HOST_REQUIRE(Eout == 0 || (edge_index_out && edge_src), "edge_index_out / edge_src are null");                               \
    HOST_REQUIRE(x_ok, x_msg);                                                                                                   \
    OutWriter W{Nout, Eout, F, ptr_out, edge_ptr_out, batch_out, x_out, edge_index_out, node_src, edge_src}

// ---- batch splice (cal_amd/csrc/splice.hip): the same order of nodes and columns, the same dropped columns and bridge rules, so
// every integer output agrees bit for bit.  The count leaves each pair's valid-column counts in ws, as the device does.
namespace {
struct SpliceSide {            // (the fields side_ranges and col_valid of rules.hpp read, named as splice.hip's Side)
    const int64_t* ei; int64_t E, N; const int64_t* ptr; const int64_t* eptr; int64_t B; const int64_t* pick; const int64_t* bridge;
};
inline bool splice_bridge(const SpliceSide& a, const SpliceSide& b, int64_t p, int64_t alo, int64_t an, int64_t blo, int64_t bn,
                          bool& asked) {
    const int64_t ba = a.bridge ? a.bridge[p] : -1, bb = b.bridge ? b.bridge[p] : -1;
    asked = ba >= 0 || bb >= 0;
    return ba >= 0 && bb >= 0 && ba >= alo && ba < alo + an && bb >= blo && bb < blo + bn;
}
}  // namespace

HOST_EXPORT int64_t cal_graph_splice_ws(int64_t Ea, int64_t Eb, int64_t P) {
    return 40 * (P > 0 ? P : 0) + 8 * (Ea > 0 ? Ea : 0) + 8 * (Eb > 0 ? Eb : 0) + 256;
}

#define SPLICE_REQUIRE_INPUTS()                                                                                                  \
    HOST_REQUIRE(Ea >= 0 && Na >= 0 && Ba >= 0 && Eb >= 0 && Nb >= 0 && Bb >= 0 && P >= 0, "sizes must be >= 0");                \
    HOST_REQUIRE(P == 0 || (ga && gb), "ga / gb are null");                                                                      \
    HOST_REQUIRE((Ba == 0 || (ptr_a && eptr_a)) && (Bb == 0 || (ptr_b && eptr_b)), "ptr / edge_ptr are null");                   \
    HOST_REQUIRE((Ea == 0 || eia) && (Eb == 0 || eib), "edge_index is null");                                                    \
    HOST_REQUIRE((bridge_a == nullptr) == (bridge_b == nullptr), "bridge_a and bridge_b come together");                        \
    HOST_REQUIRE(P == 0 || (ws && ws_bytes >= cal_graph_splice_ws(Ea, Eb, P)), "ws must hold cal_graph_splice_ws(Ea, Eb, P) bytes")

HOST_EXPORT int cal_graph_splice_count(const int64_t* eia, int64_t Ea, int64_t Na, const int64_t* ptr_a, const int64_t* eptr_a,
                                       int64_t Ba, const int64_t* eib, int64_t Eb, int64_t Nb, const int64_t* ptr_b,
                                       const int64_t* eptr_b, int64_t Bb, const int64_t* ga, const int64_t* gb, int64_t P,
                                       const int64_t* bridge_a, const int64_t* bridge_b, int64_t* ptr_out, int64_t* edge_ptr_out,
                                       int64_t* totals, void* ws, int64_t ws_bytes, void*) {
    SPLICE_REQUIRE_INPUTS();
    HOST_REQUIRE(totals && ptr_out && edge_ptr_out, "totals / ptr_out / edge_ptr_out are null");
    const SpliceSide A{eia, Ea, Na, ptr_a, eptr_a, Ba, ga, bridge_a}, B{eib, Eb, Nb, ptr_b, eptr_b, Bb, gb, bridge_b};
    int64_t* cnt = (int64_t*)ws;
    BatchScan scan{ptr_out, edge_ptr_out, totals};
    int64_t unput = 0;
    for (int64_t p = 0; p < P; ++p) {
        int64_t alo, an, aelo, aem, blo, bn, belo, bem, ea = 0, eb = 0;
        side_ranges(A, p, alo, an, aelo, aem);
        side_ranges(B, p, blo, bn, belo, bem);
        for (int64_t e = aelo; e < aelo + aem; ++e) ea += col_valid(A, e, alo, an);
        for (int64_t e = belo; e < belo + bem; ++e) eb += col_valid(B, e, blo, bn);
        bool asked;
        const bool put = splice_bridge(A, B, p, alo, an, blo, bn, asked);
        cnt[p] = ea;
        cnt[P + p] = eb;
        scan.add(p, an + bn, ea + eb + (put ? 2 : 0));
        unput += asked && !put;
    }
    scan.finish(P);
    totals[5] = unput;
    return 0;
}

HOST_EXPORT int cal_graph_splice_write(const int64_t* eia, int64_t Ea, int64_t Na, const int64_t* ptr_a, const int64_t* eptr_a,
                                       int64_t Ba, const int64_t* eib, int64_t Eb, int64_t Nb, const int64_t* ptr_b,
                                       const int64_t* eptr_b, int64_t Bb, const int64_t* ga, const int64_t* gb, int64_t P,
                                       const int64_t* bridge_a, const int64_t* bridge_b, const float* xa, const float* xb, int64_t F,
                                       const int64_t* ptr_out, const int64_t* edge_ptr_out, int64_t Nout, int64_t Eout,
                                       int64_t* batch_out, float* x_out, int64_t* edge_index_out, int64_t* node_src,
                                       int64_t* edge_src, void* ws, int64_t ws_bytes, void*) {
    SPLICE_REQUIRE_INPUTS();
    HOST_REQUIRE_WRITE(P, !x_out || (F > 0 && (Na == 0 || xa) && (Nb == 0 || xb)), "x_out needs F > 0, xa and xb");
    const SpliceSide A{eia, Ea, Na, ptr_a, eptr_a, Ba, ga, bridge_a}, B{eib, Eb, Nb, ptr_b, eptr_b, Bb, gb, bridge_b};
    for (int64_t p = 0; p < P; ++p) {
        int64_t alo, an, aelo, aem, blo, bn, belo, bem;
        side_ranges(A, p, alo, an, aelo, aem);
        side_ranges(B, p, blo, bn, belo, bem);
        W.begin(p);
        const int64_t n0 = W.n0;
        for (int64_t s = alo; s < alo + an; ++s) W.node(s, xa, s);
        for (int64_t s = blo; s < blo + bn; ++s) W.node(-1 - s, xb, s);
        for (int64_t e = aelo; e < aelo + aem; ++e)
            if (col_valid(A, e, alo, an)) W.col(n0 + (eia[e] - alo), n0 + (eia[Ea + e] - alo), e);
        for (int64_t e = belo; e < belo + bem; ++e)
            if (col_valid(B, e, blo, bn)) W.col(n0 + an + (eib[e] - blo), n0 + an + (eib[Eb + e] - blo), -1 - e);
        bool asked;
        if (splice_bridge(A, B, p, alo, an, blo, bn, asked)) {
            const int64_t u = n0 + (bridge_a[p] - alo), v = n0 + an + (bridge_b[p] - blo);
            W.col(u, v, CAL_SPLICE_BRIDGE);
            W.col(v, u, CAL_SPLICE_BRIDGE);
        }
    }
    return 0;
}
#undef SPLICE_REQUIRE_INPUTS

// ---- the restriction builders: occlusion, coalition and subset replicas (cal_amd/csrc/restrict.hpp with occlude.hip, coalition.hip,
// subset.hip; occlude_batch, coalition_batch, subset_batch).  One count loop and one write loop over the sources and the
// replica / node_stays / col_stays overloads of rules.hpp: the same nodes and columns in the same order as the kernels, so every
// integer output agrees bit for bit.  An entry point is its checks, its source and one call.
namespace {
template <class S>
int restrict_count(const S& s, int64_t R, int64_t* ptr_out, int64_t* edge_ptr_out, int64_t* totals) {
    std::vector<int64_t> cn((size_t)R), cm((size_t)R);
#pragma omp parallel for schedule(dynamic, 16)
    for (int64_t r = 0; r < R; ++r) {
        const auto q = replica(s, r);
        int64_t n = 0, m = 0;
        for (int64_t l = 0; l < q.nn; ++l) n += node_stays(s, q, l);
        for (int64_t e = q.elo; e < q.elo + q.em; ++e) m += col_stays(s, q, e);
        cn[(size_t)r] = n;
        cm[(size_t)r] = m;
    }
    BatchScan scan{ptr_out, edge_ptr_out, totals};
    for (int64_t r = 0; r < R; ++r) scan.add(r, cn[(size_t)r], cm[(size_t)r]);
    scan.finish(R);
    return 0;
}

template <class S>
int restrict_write(const S& s, int64_t R, const float* x, OutWriter W) {
#pragma omp parallel for schedule(dynamic, 16) firstprivate(W)
    for (int64_t r = 0; r < R; ++r) {                          // (every replica writes its own run of the outputs)
        std::vector<int64_t> local;                            // new local id of every node of the replica's graph
        const auto q = replica(s, r);
        W.begin(r);
        local.assign((size_t)q.nn, 0);
        for (int64_t l = 0; l < q.nn; ++l) {
            local[(size_t)l] = W.i - W.n0;
            if (node_stays(s, q, l)) W.node(q.nlo + l, x, q.nlo + l);
        }
        for (int64_t e = q.elo; e < q.elo + q.em; ++e)
            if (col_stays(s, q, e)) W.col(W.n0 + local[(size_t)(s.ei[e] - q.nlo)], W.n0 + local[(size_t)(s.ei[s.E + e] - q.nlo)], e);
    }
    return 0;
}
}  // namespace

// the checks the six entry points share (HOST_REQUIRE names the entry point): HEAD, then the builder's own, then TAIL
#define RESTRICT_REQUIRE_HEAD(sizes_ok)                                                                                          \
    HOST_REQUIRE(sizes_ok, "sizes must be >= 0");                                                                                \
    HOST_REQUIRE(mode == 0 || mode == 1, "mode must be 0 (edges) or 1 (nodes)")
#define RESTRICT_REQUIRE_TAIL()                                                                                                  \
    HOST_REQUIRE(B == 0 || (ptr && edge_ptr), "ptr / edge_ptr are null");                                                        \
    HOST_REQUIRE(E == 0 || edge_index, "edge_index is null");                                                                    \
    const BatchSrc batch{edge_index, E, N, ptr, edge_ptr, B, rep_graph, mode}

HOST_EXPORT int64_t cal_occlude_ws(int64_t, int64_t R) { return restrict_ws_need(R, 0, 0); }

#define OCCLUDE_REQUIRE_INPUTS()                                                                                                 \
    RESTRICT_REQUIRE_HEAD(E >= 0 && N >= 0 && B >= 0 && R >= 0);                                                                 \
    HOST_REQUIRE(R == 0 || (rep_graph && rep_elem), "rep_graph / rep_elem are null");                                            \
    RESTRICT_REQUIRE_TAIL();                                                                                                     \
    const OccSrc S = occ_src(batch, rep_elem, twin)

HOST_EXPORT int cal_occlude_count(const int64_t* edge_index, int64_t E, int64_t N, const int64_t* ptr, const int64_t* edge_ptr,
                                  int64_t B, const int64_t* rep_graph, const int64_t* rep_elem, int64_t R, int mode,
                                  const int32_t* twin, int64_t* ptr_out, int64_t* edge_ptr_out, int64_t* totals, void*, int64_t,
                                  void*) {
    OCCLUDE_REQUIRE_INPUTS();
    HOST_REQUIRE(totals && ptr_out && edge_ptr_out, "totals / ptr_out / edge_ptr_out are null");
    return restrict_count(S, R, ptr_out, edge_ptr_out, totals);
}

HOST_EXPORT int cal_occlude_write(const int64_t* edge_index, int64_t E, int64_t N, const int64_t* ptr, const int64_t* edge_ptr,
                                  int64_t B, const int64_t* rep_graph, const int64_t* rep_elem, int64_t R, int mode,
                                  const int32_t* twin, const float* x, int64_t F, const int64_t* ptr_out,
                                  const int64_t* edge_ptr_out, int64_t Nout, int64_t Eout, int64_t* batch_out, float* x_out,
                                  int64_t* edge_index_out, int64_t* node_src, int64_t* edge_src, void*, int64_t, void*) {
    OCCLUDE_REQUIRE_INPUTS();
    HOST_REQUIRE_WRITE(R, !x_out || (F > 0 && (N == 0 || x)), "x_out needs F > 0 and x");
    return restrict_write(S, R, x, W);
}
#undef OCCLUDE_REQUIRE_INPUTS

HOST_EXPORT int64_t cal_coalition_ws(int64_t, int64_t R, int64_t max_nodes, int mode) { return restrict_ws_need(R, max_nodes, mode); }

#define COALITION_REQUIRE_INPUTS()                                                                                               \
    RESTRICT_REQUIRE_HEAD(E >= 0 && N >= 0 && B >= 0 && R >= 0 && K >= 0);                                                       \
    HOST_REQUIRE(invert == 0 || invert == 1, "invert must be 0 or 1");                                                           \
    HOST_REQUIRE(max_nodes >= 0 && max_nodes <= 0x7FFFFFFF, "max_nodes must be in [0, 2^31)");                                   \
    HOST_REQUIRE(R == 0 || (rep_graph && rep_row && rep_thresh), "rep_graph / rep_row / rep_thresh are null");                   \
    HOST_REQUIRE(K == 0 || (mode == 0 ? E : N) == 0 || key, "key is null");                                                      \
    RESTRICT_REQUIRE_TAIL();                                                                                                     \
    const CoSrc S = co_src(batch, key, K, rep_row, rep_thresh, invert, max_nodes)

HOST_EXPORT int cal_coalition_count(const int64_t* edge_index, int64_t E, int64_t N, const int64_t* ptr, const int64_t* edge_ptr,
                                    int64_t B, const int32_t* key, int64_t K, const int64_t* rep_graph, const int64_t* rep_row,
                                    const int64_t* rep_thresh, int64_t R, int mode, int invert, int64_t max_nodes,
                                    int64_t* ptr_out, int64_t* edge_ptr_out, int64_t* totals, void*, int64_t, void*) {
    COALITION_REQUIRE_INPUTS();
    HOST_REQUIRE(totals && ptr_out && edge_ptr_out, "totals / ptr_out / edge_ptr_out are null");
    return restrict_count(S, R, ptr_out, edge_ptr_out, totals);
}

HOST_EXPORT int cal_coalition_write(const int64_t* edge_index, int64_t E, int64_t N, const int64_t* ptr, const int64_t* edge_ptr,
                                    int64_t B, const int32_t* key, int64_t K, const int64_t* rep_graph, const int64_t* rep_row,
                                    const int64_t* rep_thresh, int64_t R, int mode, int invert, int64_t max_nodes, const float* x,
                                    int64_t F, const int64_t* ptr_out, const int64_t* edge_ptr_out, int64_t Nout, int64_t Eout,
                                    int64_t* batch_out, float* x_out, int64_t* edge_index_out, int64_t* node_src,
                                    int64_t* edge_src, void*, int64_t, void*) {
    COALITION_REQUIRE_INPUTS();
    HOST_REQUIRE_WRITE(R, !x_out || (F > 0 && (N == 0 || x)), "x_out needs F > 0 and x");
    return restrict_write(S, R, x, W);
}
#undef COALITION_REQUIRE_INPUTS

HOST_EXPORT int64_t cal_subset_ws(int64_t, int64_t R, int64_t max_nodes, int mode) { return restrict_ws_need(R, max_nodes, mode); }

#define SUBSET_REQUIRE_INPUTS()                                                                                                  \
    RESTRICT_REQUIRE_HEAD(E >= 0 && N >= 0 && B >= 0 && R >= 0 && K >= 0 && NW >= 0);                                            \
    HOST_REQUIRE(NW <= (1 << 26), "W must be <= 2^26");                                                                          \
    HOST_REQUIRE(max_nodes >= 0 && max_nodes <= 0x7FFFFFFF, "max_nodes must be in [0, 2^31)");                                   \
    HOST_REQUIRE(R == 0 || (rep_graph && rep_row && rep_flip), "rep_graph / rep_row / rep_flip are null");                       \
    HOST_REQUIRE(K == 0 || NW == 0 || bits, "bits is null");                                                                     \
    RESTRICT_REQUIRE_TAIL();                                                                                                     \
    const SubSrc S = sub_src(batch, bits, K, NW, rep_row, rep_flip, twin, max_nodes)

HOST_EXPORT int cal_subset_count(const int64_t* edge_index, int64_t E, int64_t N, const int64_t* ptr, const int64_t* edge_ptr,
                                 int64_t B, const uint32_t* bits, int64_t K, int64_t NW, const int64_t* rep_graph,
                                 const int64_t* rep_row, const int64_t* rep_flip, int64_t R, const int32_t* twin, int mode,
                                 int64_t max_nodes, int64_t* ptr_out, int64_t* edge_ptr_out, int64_t* totals, void*, int64_t,
                                 void*) {
    SUBSET_REQUIRE_INPUTS();
    HOST_REQUIRE(totals && ptr_out && edge_ptr_out, "totals / ptr_out / edge_ptr_out are null");
    return restrict_count(S, R, ptr_out, edge_ptr_out, totals);
}

HOST_EXPORT int cal_subset_write(const int64_t* edge_index, int64_t E, int64_t N, const int64_t* ptr, const int64_t* edge_ptr,
                                 int64_t B, const uint32_t* bits, int64_t K, int64_t NW, const int64_t* rep_graph,
                                 const int64_t* rep_row, const int64_t* rep_flip, int64_t R, const int32_t* twin, int mode,
                                 int64_t max_nodes, const float* x, int64_t F, const int64_t* ptr_out,
                                 const int64_t* edge_ptr_out, int64_t Nout, int64_t Eout, int64_t* batch_out, float* x_out,
                                 int64_t* edge_index_out, int64_t* node_src, int64_t* edge_src, void*, int64_t, void*) {
    SUBSET_REQUIRE_INPUTS();
    HOST_REQUIRE_WRITE(R, !x_out || (F > 0 && (N == 0 || x)), "x_out needs F > 0 and x");
    return restrict_write(S, R, x, W);
}
#undef SUBSET_REQUIRE_INPUTS
#undef RESTRICT_REQUIRE_HEAD
#undef RESTRICT_REQUIRE_TAIL

// ---- the beam step (cal_amd/csrc/beam.hip; cal_amd/counterfactual.py): the order, the children and the duplicates of rules.hpp,
// graph by graph.
namespace {
struct BeamSrc {               // (the fields beam_parent and beam_before of rules.hpp read, named as beam.hip's BeamArgs)
    const uint32_t* bits; int beam; int64_t W; const int64_t* nst; const int64_t* rrow; const int64_t* rflip; const float* p;
    const uint8_t* flipped;
};
}  // namespace

HOST_EXPORT int cal_beam_step(const uint32_t* bits, int64_t B, int beam, int64_t W, const int64_t* n_state,
                              const int64_t* cand_ptr, const int64_t* rep_row, const int64_t* rep_flip, const float* p,
                              const uint8_t* flipped, int64_t R, const int64_t* seg_ptr, int64_t M, const int32_t* twin, int mode,
                              int64_t max_cand, uint8_t* done, uint32_t* bits_out, float* p_state_out, int64_t* n_state_out,
                              uint32_t* cf_bits, float* cf_p, int64_t* cf_cand, int32_t* status, void*) {
    HOST_REQUIRE(B >= 0 && R >= 0 && M >= 0 && B <= 0x7FFFFFFF, "sizes must be >= 0, B < 2^31");
    HOST_REQUIRE(beam >= 1 && beam <= kBeamMax, "beam must be in [1, 16]");
    HOST_REQUIRE(W >= 0 && W <= kBeamWords, "W must be in [0, 64]");
    HOST_REQUIRE(mode == 0 || mode == 1, "mode must be 0 (edges) or 1 (nodes)");
    HOST_REQUIRE(max_cand >= 0 && max_cand <= cal_explain_lds_cap(), "max_cand must be <= cal_explain_lds_cap()");
    if (B == 0) return 0;
    HOST_REQUIRE(n_state && cand_ptr && seg_ptr && done && n_state_out && status,
                 "n_state / cand_ptr / seg_ptr / done / n_state_out / status are null");
    HOST_REQUIRE(W == 0 || (bits && bits_out && cf_bits), "bits / bits_out / cf_bits are null");
    HOST_REQUIRE(p_state_out && cf_p && cf_cand, "p_state_out / cf_p / cf_cand are null");
    HOST_REQUIRE(R == 0 || (rep_row && rep_flip && p && flipped), "rep_row / rep_flip / p / flipped are null");
    const BeamSrc S{bits, beam, W, n_state, rep_row, rep_flip, p, flipped};
    if (mode != 0) twin = nullptr;
#pragma omp parallel for schedule(dynamic, 4)
    for (int64_t g = 0; g < B; ++g) {
        n_state_out[g] = 0;
        int64_t clo, cn, lo, m;
        seg_clamp(cand_ptr, g, R, clo, cn);
        if (done[g] || cn == 0) continue;
        if (cn > max_cand) {
            status[g] = 2;
            continue;
        }
        status[g] = 0;
        seg_clamp(seg_ptr, g, M, lo, m);
        std::vector<int64_t> ord((size_t)cn);
        for (int64_t c = 0; c < cn; ++c) ord[(size_t)c] = clo + c;
        std::sort(ord.begin(), ord.end(), [&](int64_t i, int64_t j) { return beam_before(S, i, j); });
        std::vector<uint32_t> child((size_t)W), kept;            // kept: the children picked so far, W words each
        auto make = [&](int64_t i) {
            const int s = beam_parent(S, g, i);
            int64_t f0, f1;
            flip_pair(rep_flip[i], lo, m, twin, f0, f1);
            if (f0 >= 32 * W) f0 = -1;                             // (an index >= 32 W toggles nothing)
            if (f1 >= 32 * W) f1 = -1;
            for (int64_t w = 0; w < W; ++w)
                child[(size_t)w] = (s < beam ? bits[(g * beam + s) * W + w] : full_word(m, W, w)) ^ flip_word(f0, f1, w);
        };
        if (flipped[ord[0]]) {
            make(ord[0]);
            for (int64_t w = 0; w < W; ++w) cf_bits[g * W + w] = child[(size_t)w];
            done[g] = 1;
            cf_p[g] = p[ord[0]];
            cf_cand[g] = ord[0];
            continue;
        }
        int64_t picked = 0;
        for (int64_t c = 0; c < cn && picked < beam; ++c) {
            make(ord[(size_t)c]);
            bool dup = false;
            for (int64_t k = 0; k < picked && !dup; ++k)
                dup = std::equal(child.begin(), child.end(), kept.begin() + (size_t)(k * W));
            if (dup) continue;
            kept.insert(kept.end(), child.begin(), child.end());
            for (int64_t w = 0; w < W; ++w) bits_out[(g * beam + picked) * W + w] = child[(size_t)w];
            p_state_out[g * beam + picked] = p[ord[(size_t)c]];
            ++picked;
        }
        n_state_out[g] = picked;
    }
    return 0;
}

// ---- structural-noise replicas (cal_amd/csrc/noise.hip; cal_amd/noise.py noise_batch): the hash, the deletions and the pair key of
// rules.hpp and the same accepted candidates in the same order, so every integer output agrees bit for bit.  Nothing is kept
// between the two calls: the write decides the insertions again.
namespace {
struct NoiseSrc {              // (the fields noise_replica and noise_stays of rules.hpp read, named as noise.hip's NoArgs)
    const int64_t* ei; int64_t E, N; const int64_t* ptr; const int64_t* eptr; int64_t B; const int32_t* twin;
    const int64_t* rg; const int64_t* rseed; const int64_t* rdel; const int64_t* radd; int64_t tries;
    // the accepted pairs of replica q, in candidate order
    void insertions(const NoRep& q, std::vector<std::pair<int64_t, int64_t>>& out) const {
        out.clear();
        const int64_t a = q.a;
        const uint64_t n = (uint64_t)q.nn;
        if (a == 0 || n <= 1) return;
        std::vector<uint64_t> taken;                           // the source pairs, sorted; then the accepted ones, unsorted
        for (int64_t e = q.elo; e < q.elo + q.em; ++e)
            if (col_valid(*this, e, q.nlo, q.nn) && ei[e] != ei[E + e])
                taken.push_back(pair_key(twin != nullptr, (uint64_t)(ei[e] - q.nlo), (uint64_t)(ei[E + e] - q.nlo), n));
        std::sort(taken.begin(), taken.end());
        const size_t ns = taken.size();
        const uint64_t total = (uint64_t)tries * (uint64_t)a;
        for (uint64_t c = 0; c < total && (int64_t)out.size() < a; ++c) {
            const uint64_t h = noise_hash(q.seed ^ kNoiseAdd, c);
            const uint64_t u = (h >> 32) % n, v = (h & 0xffffffffull) % n;
            if (u == v) continue;
            const uint64_t k = pair_key(twin != nullptr, u, v, n);
            if (std::binary_search(taken.begin(), taken.begin() + (long)ns, k)) continue;
            if (std::find(taken.begin() + (long)ns, taken.end(), k) != taken.end()) continue;
            taken.push_back(k);
            out.emplace_back((int64_t)u, (int64_t)v);
        }
    }
};
}  // namespace

HOST_EXPORT int64_t cal_noise_ws(int64_t, int64_t, int64_t, int64_t) { return 0; }

#define NOISE_REQUIRE_INPUTS()                                                                                                   \
    HOST_REQUIRE(E >= 0 && N >= 0 && B >= 0 && R >= 0, "sizes must be >= 0");                                                    \
    HOST_REQUIRE(tries >= 1 && tries <= (1 << 20), "tries must be in [1, 2^20]");                                                \
    HOST_REQUIRE(R == 0 || (rep_graph && rep_seed && rep_del && rep_add && added), "rep_graph / rep_seed / rep_del / rep_add / added are null"); \
    HOST_REQUIRE(B == 0 || (ptr && edge_ptr), "ptr / edge_ptr are null");                                                        \
    HOST_REQUIRE(E == 0 || edge_index, "edge_index is null");                                                                    \
    const NoiseSrc S{edge_index, E, N, ptr, edge_ptr, B, E > 0 ? twin : nullptr, rep_graph, rep_seed, rep_del, rep_add, tries}

HOST_EXPORT int cal_noise_count(const int64_t* edge_index, int64_t E, int64_t N, const int64_t* ptr, const int64_t* edge_ptr,
                                int64_t B, const int32_t* twin, const int64_t* rep_graph, const int64_t* rep_seed,
                                const int64_t* rep_del, const int64_t* rep_add, int64_t R, int64_t tries, int64_t* added,
                                int64_t* ptr_out, int64_t* edge_ptr_out, int64_t* totals, void*, int64_t, void*) {
    NOISE_REQUIRE_INPUTS();
    HOST_REQUIRE(totals && ptr_out && edge_ptr_out, "totals / ptr_out / edge_ptr_out are null");
    BatchScan scan{ptr_out, edge_ptr_out, totals};
    std::vector<std::pair<int64_t, int64_t>> ins;
    int64_t sum = 0, fell = 0;
    for (int64_t r = 0; r < R; ++r) {
        const NoRep q = noise_replica(S, r);
        int64_t m = 0;
        for (int64_t e = q.elo; e < q.elo + q.em; ++e) m += noise_stays(S, q, e);
        S.insertions(q, ins);
        added[r] = (int64_t)ins.size();
        sum += added[r];
        fell += added[r] < q.a;
        scan.add(r, q.nn, m + added[r] * (S.twin ? 2 : 1));
    }
    scan.finish(R);
    totals[5] = sum;
    totals[6] = fell;
    return 0;
}

HOST_EXPORT int cal_noise_write(const int64_t* edge_index, int64_t E, int64_t N, const int64_t* ptr, const int64_t* edge_ptr,
                                int64_t B, const int32_t* twin, const int64_t* rep_graph, const int64_t* rep_seed,
                                const int64_t* rep_del, const int64_t* rep_add, int64_t R, int64_t tries, int64_t* added,
                                const float* x, int64_t F, const int64_t* ptr_out, const int64_t* edge_ptr_out, int64_t Nout,
                                int64_t Eout, int64_t* batch_out, float* x_out, int64_t* edge_index_out, int64_t* node_src,
                                int64_t* edge_src, void*, int64_t, void*) {
    NOISE_REQUIRE_INPUTS();
    HOST_REQUIRE_WRITE(R, !x_out || (F > 0 && (N == 0 || x)), "x_out needs F > 0 and x");
    std::vector<std::pair<int64_t, int64_t>> ins;
    for (int64_t r = 0; r < R; ++r) {
        const NoRep q = noise_replica(S, r);
        W.begin(r);
        for (int64_t s = q.nlo; s < q.nlo + q.nn; ++s) W.node(s, x, s);
        for (int64_t e = q.elo; e < q.elo + q.em; ++e)
            if (noise_stays(S, q, e)) W.col(W.n0 + edge_index[e] - q.nlo, W.n0 + edge_index[E + e] - q.nlo, e);
        S.insertions(q, ins);
        for (const auto& p : ins) {
            W.col(W.n0 + p.first, W.n0 + p.second, -1);
            if (S.twin) W.col(W.n0 + p.second, W.n0 + p.first, -1);
        }
    }
    return 0;
}
#undef NOISE_REQUIRE_INPUTS

HOST_EXPORT int cal_degree_onehot(const int64_t* edge_index, int64_t E, int64_t N, int64_t F, float* x_out, void*) {
    HOST_REQUIRE(E >= 0 && N >= 0, "E, N must be >= 0");
    HOST_REQUIRE(F >= 1 && F < (1 << 22), "F must be in [1, 2^22)");
    if (N == 0) return 0;
    HOST_REQUIRE(x_out, "x_out is null");
    HOST_REQUIRE(E == 0 || edge_index, "edge_index is null");
    std::vector<int64_t> deg((size_t)N, 0);
    for (int64_t e = 0; e < E; ++e) {
        const int64_t u = edge_index[e];
        if (u >= 0 && u < N && u != edge_index[E + e]) ++deg[(size_t)u];
    }
    memset(x_out, 0, sizeof(float) * (size_t)N * (size_t)F);
    for (int64_t i = 0; i < N; ++i) x_out[i * F + std::min(deg[(size_t)i], F - 1)] = 1.f;
    return 0;
}

// ---- rank agreement (cal_amd/csrc/occlude.hip; cal_amd/occlude.py rank_agreement): the same ten integers per segment, here from
// two sorts per segment where the device counts all pairs.
HOST_EXPORT int64_t cal_rank_agreement_ws(int64_t, int64_t, int64_t) { return 0; }

HOST_EXPORT int cal_rank_agreement(const float* a, const float* b, int64_t M, const int64_t* seg_ptr, int64_t B, int64_t max_seg,
                                   const uint8_t* sel, int64_t k_code, double k_val, int64_t* counts, void*, int64_t, void*) {
    HOST_REQUIRE(M >= 0 && B >= 0 && max_seg >= 0, "M, B, max_seg must be >= 0");
    HOST_REQUIRE(max_seg < ((int64_t)1 << 20), "segments of 2^20 elements or more are not supported (the sums would leave int64)");
    HOST_REQUIRE(k_code >= -1, "k_code must be >= 0 or -1 (ratio)");
    HOST_REQUIRE(k_code != -1 || k_val >= 0.0, "k_code = -1 needs a ratio >= 0");
    if (B == 0) return 0;
    HOST_REQUIRE(seg_ptr && counts, "seg_ptr / counts are null");
    HOST_REQUIRE(M == 0 || (a && b), "a / b are null");
#pragma omp parallel for schedule(dynamic, 16)
    for (int64_t g = 0; g < B; ++g) {
        int64_t lo, m;
        seg_clamp(seg_ptr, g, M, lo, m);
        int64_t* row = counts + 10 * g;
        for (int t = 0; t < 10; ++t) row[t] = 0;
        if (m > max_seg) { row[0] = -1; continue; }
        std::vector<int64_t> id;                               // the elements taking part, ascending
        for (int64_t i = lo; i < lo + m; ++i)
            if ((!sel || sel[i]) && a[i] == a[i] && b[i] == b[i]) id.push_back(i);
        const int64_t n = (int64_t)id.size();
        const int64_t kg = ag_sel_count(n, k_val, k_code);
        // doubled mid-ranks and top-k membership of one vector: positions in the order value descending, then index
        std::vector<int64_t> r2[2];
        std::vector<uint8_t> top[2];
        int64_t tied[2] = {0, 0};
        for (int s = 0; s < 2; ++s) {
            const float* v = s ? b : a;
            std::vector<int64_t> ord(n);
            for (int64_t q = 0; q < n; ++q) ord[q] = q;
            std::sort(ord.begin(), ord.end(), [&](int64_t p, int64_t q) { return v[id[p]] != v[id[q]] ? v[id[p]] > v[id[q]] : p < q; });
            r2[s].assign(n, 0);
            top[s].assign(n, 0);
            for (int64_t p = 0; p < n;) {                      // runs of equal values: [p, e)
                int64_t e = p + 1;
                while (e < n && v[id[ord[e]]] == v[id[ord[p]]]) ++e;
                const int64_t eq = e - p, less = n - e;
                tied[s] += eq * (eq - 1) / 2;
                for (int64_t t = p; t < e; ++t) { r2[s][ord[t]] = 2 * less + eq + 1; top[s][ord[t]] = t < kg; }
                p = e;
            }
        }
        int64_t C = 0, D = 0, saa = 0, sbb = 0, sab = 0, inter = 0;
        for (int64_t p = 0; p < n; ++p) {
            saa += r2[0][p] * r2[0][p];
            sbb += r2[1][p] * r2[1][p];
            sab += r2[0][p] * r2[1][p];
            inter += top[0][p] && top[1][p];
            const float ap = a[id[p]], bp = b[id[p]];
            for (int64_t q = p + 1; q < n; ++q) {
                const float aq = a[id[q]], bq = b[id[q]];
                const int sa = (aq > ap) - (aq < ap), sb = (bq > bp) - (bq < bp);
                C += sa * sb > 0;
                D += sa * sb < 0;
            }
        }
        row[0] = n; row[1] = C; row[2] = D; row[3] = tied[0]; row[4] = tied[1];
        row[5] = saa; row[6] = sbb; row[7] = sab; row[8] = kg; row[9] = inter;
    }
    return 0;
}

// ---- all-pairs intervention readout (cal_amd/csrc/intervene.hip): the same folded form, dot products accumulated in fp64 ----
HOST_EXPORT int64_t cal_intervene_ws(int64_t, int64_t, int64_t, int64_t) { return 0; }

HOST_EXPORT int cal_intervene_pairs(const float* xo, int64_t B, const float* xc, int64_t M, int64_t H, int64_t C, int cat,
                                    const float* bn1_w, const float* bn1_b, const float* bn1_mean, const float* bn1_var, float bn1_eps,
                                    const float* fc1_w, const float* fc1_b, const float* bn2_w, const float* bn2_b,
                                    const float* bn2_mean, const float* bn2_var, float bn2_eps, const float* fc2_w,
                                    const float* fc2_b, const int64_t* ref, float* p_do, int32_t* hits, float* p_min,
                                    int32_t* j_min, float* logp_pairs, void*, int64_t, void*) {
    HOST_REQUIRE(B >= 0, "B must be >= 0");
    HOST_REQUIRE(M >= 1, "the bank is empty (M must be >= 1)");
    HOST_REQUIRE(H >= 1 && C >= 1, "H and C must be >= 1");
    if (B == 0) return 0;
    HOST_REQUIRE(xo && xc && p_do && hits && p_min && j_min, "xo / xc / an output is null");
    HOST_REQUIRE(bn1_w && bn1_b && bn1_mean && bn1_var && fc1_w && fc1_b && bn2_w && bn2_b && bn2_mean && bn2_var && fc2_w && fc2_b,
                 "a parameter of the co head is null");
    const int64_t Kin = cat ? 2 * H : H, koff = cat ? H : 0;
    std::vector<double> s1(Kin), t1(Kin), cst(H), b2f(C);
    std::vector<float> A((size_t)B * H), Cb((size_t)M * H), W2f((size_t)C * H);
    for (int64_t k = 0; k < Kin; ++k) {
        s1[k] = (double)bn1_w[k] / sqrt((double)bn1_var[k] + (double)bn1_eps);
        t1[k] = (double)bn1_b[k] - (double)bn1_mean[k] * s1[k];
    }
    for (int64_t n = 0; n < H; ++n) {
        double s = fc1_b[n];
        for (int64_t k = 0; k < Kin; ++k) s += (double)fc1_w[n * Kin + k] * t1[k];
        cst[n] = s;
    }
    for (int64_t c = 0; c < C; ++c) {
        double s = fc2_b[c];
        for (int64_t k = 0; k < H; ++k) {
            const double sc = (double)bn2_w[k] / sqrt((double)bn2_var[k] + (double)bn2_eps);
            W2f[c * H + k] = (float)((double)fc2_w[c * H + k] * sc);
            s += (double)fc2_w[c * H + k] * ((double)bn2_b[k] - (double)bn2_mean[k] * sc);
        }
        b2f[c] = s;
    }
#pragma omp parallel for schedule(static)
    for (int64_t r = 0; r < B + M; ++r) {
        const bool isA = r < B;
        const float* x = isA ? xo + r * H : xc + (r - B) * H;
        float* out = isA ? A.data() + r * H : Cb.data() + (r - B) * H;
        const int64_t ko = isA ? koff : 0;
        for (int64_t n = 0; n < H; ++n) {
            double s = isA ? cst[n] : 0.0;
            for (int64_t k = 0; k < H; ++k) s += (double)fc1_w[n * Kin + ko + k] * s1[ko + k] * (double)x[k];
            out[n] = (float)s;
        }
    }
#pragma omp parallel for schedule(static)
    for (int64_t g = 0; g < B; ++g) {
        std::vector<float> h(H);
        std::vector<double> z(C), ps(C, 0.0);
        const int64_t rf = (ref && ref[g] >= 0 && ref[g] < C) ? ref[g] : -1;
        int64_t nh = 0, jm = -1;
        float mn = INFINITY;
        for (int64_t j = 0; j < M; ++j) {
            for (int64_t k = 0; k < H; ++k) h[k] = std::max(A[g * H + k] + Cb[j * H + k], 0.f);
            int64_t arg = 0;
            for (int64_t c = 0; c < C; ++c) {
                double s = b2f[c];
                for (int64_t k = 0; k < H; ++k) s += (double)h[k] * (double)W2f[c * H + k];
                z[c] = s;
                if (s > z[arg]) arg = c;
            }
            double se = 0.0;
            for (int64_t c = 0; c < C; ++c) se += exp(z[c] - z[arg]);
            const double lse = z[arg] + log(se);
            for (int64_t c = 0; c < C; ++c) {
                const float lp = (float)(z[c] - lse);
                if (logp_pairs) logp_pairs[(g * M + j) * C + c] = lp;
                const float p = expf(lp);
                ps[c] += (double)p;
                if (c == rf && (p < mn || jm < 0)) { mn = p; jm = j; }
            }
            nh += arg == rf;
        }
        for (int64_t c = 0; c < C; ++c) p_do[g * C + c] = (float)(ps[c] / (double)M);
        hits[g] = rf < 0 ? 0 : (int32_t)nh;
        p_min[g] = rf < 0 ? NAN : mn;
        j_min[g] = rf < 0 ? -1 : (int32_t)jm;
    }
    return 0;
}

// ---- Weisfeiler-Lehman refinement and the WL subtree kernel (cal_amd/csrc/wl.hip; cal_amd/wl.py): the same integer formulas
// (wl_next and the constants: rules.hpp), graph by graph; the match counts colours through a sorted copy, as the device does.

HOST_EXPORT int64_t cal_wl_ws(int64_t, int64_t, int64_t) { return 0; }

HOST_EXPORT int cal_wl_refine(const int64_t* edge_index, int64_t E, int64_t N, const int64_t* ptr, const int64_t* edge_ptr,
                              int64_t B, const int64_t* init, int64_t T, int64_t max_nodes, int64_t* colors, int64_t* hash,
                              int64_t* totals, void*, int64_t, void*) {
    HOST_REQUIRE(E >= 0 && N >= 0 && B >= 0 && max_nodes >= 0, "E, N, B, max_nodes must be >= 0");
    HOST_REQUIRE(T >= 0 && T <= 4096, "T must be in [0, 4096]");
    HOST_REQUIRE(totals, "totals is null");
    totals[0] = 0;
    if (B == 0) return 0;
    HOST_REQUIRE(ptr && edge_ptr && hash, "ptr / edge_ptr / hash are null");
    HOST_REQUIRE(E == 0 || edge_index, "edge_index is null");
    HOST_REQUIRE(N == 0 || colors, "colors is null");
    uint64_t* col = reinterpret_cast<uint64_t*>(colors);
    uint64_t* hs = reinterpret_cast<uint64_t*>(hash);
    int64_t ignored = 0;
#pragma omp parallel for schedule(dynamic, 16) reduction(+ : ignored)
    for (int64_t g = 0; g < B; ++g) {
        int64_t nlo, n, elo, em;
        seg_clamp(ptr, g, N, nlo, n);
        seg_clamp(edge_ptr, g, E, elo, em);
        const int64_t nhi = nlo + n, ehi = elo + em;
        auto inside = [&](int64_t e) {
            const int64_t u = edge_index[e], v = edge_index[E + e];
            return u >= nlo && u < nhi && v >= nlo && v < nhi;
        };
        for (int64_t e = elo; e < ehi; ++e) ignored += !inside(e);
        uint64_t* hrow = hs + g * (T + 1);
        if (n > max_nodes) {
            for (int64_t t = 0; t <= T; ++t) {
                hrow[t] = 0;
                for (int64_t v = nlo; v < nhi; ++v) col[t * N + v] = 0;
            }
            continue;
        }
        for (int64_t v = nlo; v < nhi; ++v) col[v] = splitmix64((init ? (uint64_t)init[v] : 0ull) ^ kWlInit);
        std::vector<uint64_t> so((size_t)n), si((size_t)n);
        uint64_t h = splitmix64((uint64_t)n ^ kWlGraph);
        for (int64_t t = 0;; ++t) {
            const uint64_t* c = col + t * N;
            uint64_t s = 0;
            for (int64_t v = nlo; v < nhi; ++v) s += splitmix64(c[v] ^ kWlNode);
            h = splitmix64(h + s);
            hrow[t] = h;
            if (t == T) break;
            std::fill(so.begin(), so.end(), 0ull);
            std::fill(si.begin(), si.end(), 0ull);
            for (int64_t e = elo; e < ehi; ++e) {
                if (!inside(e)) continue;
                const int64_t u = edge_index[e], v = edge_index[E + e];
                so[(size_t)(u - nlo)] += splitmix64(c[v] ^ kWlOut);
                si[(size_t)(v - nlo)] += splitmix64(c[u] ^ kWlIn);
            }
            for (int64_t v = nlo; v < nhi; ++v) col[(t + 1) * N + v] = wl_next(c[v], so[(size_t)(v - nlo)], si[(size_t)(v - nlo)]);
        }
    }
    totals[0] = ignored;
    return 0;
}

HOST_EXPORT int cal_wl_match(const int64_t* colors_a, int64_t stride_a, int64_t Na, const int64_t* ptr_a, int64_t A,
                             const int64_t* colors_p, int64_t stride_p, int64_t Np, const int64_t* ptr_p, int64_t P, int64_t T,
                             int64_t max_nodes_a, int64_t* K, int64_t* self_a, void*) {
    HOST_REQUIRE(Na >= 0 && A >= 0 && Np >= 0 && P >= 0 && max_nodes_a >= 0, "Na, A, Np, P, max_nodes_a must be >= 0");
    HOST_REQUIRE(T >= 0 && T <= 4096, "T must be in [0, 4096]");
    HOST_REQUIRE(Np <= 4096, "the prototype batch has more than 4096 nodes");
    HOST_REQUIRE(stride_a >= Na && stride_p >= Np, "a row stride is shorter than its row");
    if (A == 0) return 0;
    HOST_REQUIRE(ptr_a && self_a, "ptr_a / self_a are null");
    HOST_REQUIRE(P == 0 || (ptr_p && K), "ptr_p / K are null");
    HOST_REQUIRE((Na == 0 || colors_a) && (Np == 0 || colors_p), "colors_a / colors_p are null");
    const uint64_t* ca = reinterpret_cast<const uint64_t*>(colors_a);
    const uint64_t* cp = reinterpret_cast<const uint64_t*>(colors_p);
#pragma omp parallel for schedule(dynamic, 16)
    for (int64_t g = 0; g < A; ++g) {
        int64_t lo, na;
        seg_clamp(ptr_a, g, Na, lo, na);
        const int64_t hi = lo + na;
        const bool skip = na > max_nodes_a;
        std::vector<uint64_t> srt;
        for (int64_t t = 0; t <= T; ++t) {
            int64_t own = 0;
            if (!skip) {
                srt.assign(ca + t * stride_a + lo, ca + t * stride_a + hi);
                std::sort(srt.begin(), srt.end());
                for (size_t p = 0; p < srt.size();) {
                    size_t e = p + 1;
                    while (e < srt.size() && srt[e] == srt[p]) ++e;
                    own += (int64_t)((e - p) * (e - p));
                    p = e;
                }
            }
            self_a[g * (T + 1) + t] = own;
            for (int64_t p = 0; p < P; ++p) {
                int64_t plo, np, cnt = 0;
                seg_clamp(ptr_p, p, Np, plo, np);
                for (int64_t w = plo; w < plo + np && !skip; ++w) {
                    const auto r = std::equal_range(srt.begin(), srt.end(), cp[t * stride_p + w]);
                    cnt += (int64_t)(r.second - r.first);
                }
                K[(g * P + p) * (T + 1) + t] = cnt;
            }
        }
    }
    return 0;
}

// ---- exact motif matching (cal_amd/csrc/motif.hip; cal_amd/motif.py): the plan and the key of rules.hpp, the same roots and steps,
// graph by graph.
namespace {
struct MotifGraph {
    int n;
    uint64_t adj[kMotifN][4];
    const int64_t* lab;         // the graph's labels or null
    bool has(int a, int b) const { return (adj[a][b >> 6] >> (b & 63)) & 1ull; }
    int next(int a, int s) const {                                    // the lowest neighbour of a at or above s; 256: none
        for (int w = s >> 6; w < 4; ++w) {
            uint64_t m = adj[a][w];
            if (w == (s >> 6)) m &= ~0ull << (s & 63);
            if (m) return w * 64 + __builtin_ctzll(m);
        }
        return kMotifN;
    }
};

// one pattern in one graph -> count, truncated roots, the smallest key
void motif_search(const MotifGraph& G, const MotifPlan& q, const int64_t* plab, int induced, uint64_t budget, uint64_t& cnt,
                  uint64_t& trc, uint64_t& best) {
    cnt = trc = 0;
    best = ~0ull;
    const int k = q.k, n = G.n;
    auto label_ok = [&](int v, int d) { return !G.lab || G.lab[v] == plab[q.lo + motif_node(q, d)]; };
    int img[kMotifK], cur[kMotifK];
    if (k == 1) {
        for (int v = 0; v < n; ++v)
            if (label_ok(v, 0)) {
                ++cnt;
                img[0] = v;
                best = std::min<uint64_t>(best, motif_key(q, img));
            }
        return;
    }
    for (int u = 0; u < n; ++u)
        for (int w = G.next(u, 0); w < kMotifN; w = G.next(u, w + 1)) {
            if (!label_ok(u, 0) || !label_ok(w, 1)) continue;
            img[0] = u;
            img[1] = w;
            if (k == 2) {
                ++cnt;
                best = std::min<uint64_t>(best, motif_key(q, img));
                continue;
            }
            uint64_t steps = 0;
            int d = 2;
            cur[2] = 0;
            for (;;) {
                const int v = G.next(img[motif_parent(q, d)], cur[d]);
                if (v >= kMotifN) {
                    if (d == 2) break;
                    --d;
                    continue;
                }
                if (steps == budget) {
                    ++trc;
                    break;
                }
                ++steps;
                cur[d] = v + 1;
                bool ok = label_ok(v, d);
                for (int j = 0; j < d && ok; ++j) {
                    const bool a = G.has(v, img[j]);
                    ok = img[j] != v && ((motif_adj(q, d) >> j & 1u) ? a : !(induced && a));
                }
                if (!ok) continue;
                img[d] = v;
                if (d == k - 1) {
                    ++cnt;
                    best = std::min<uint64_t>(best, motif_key(q, img));
                } else {
                    ++d;
                    cur[d] = 0;
                }
            }
        }
}
}  // namespace

HOST_EXPORT int cal_motif_match(const int64_t* edge_index, int64_t E, int64_t N, const int64_t* ptr, const int64_t* edge_ptr,
                                int64_t B, const int64_t* labels, const int64_t* pat_edge_index, int64_t PE, int64_t PN,
                                const int64_t* pat_ptr, const int64_t* pat_edge_ptr, int64_t P, const int64_t* pat_labels,
                                int induced, int64_t budget, int64_t* count, int64_t* truncated, int32_t* first,
                                int64_t* tgt_edges, int64_t* pat_edges, int64_t* totals, void*) {
    HOST_REQUIRE(E >= 0 && N >= 0 && B >= 0 && PE >= 0 && PN >= 0 && P >= 0, "E, N, B, PE, PN, P must be >= 0");
    HOST_REQUIRE(induced == 0 || induced == 1, "induced must be 0 or 1");
    HOST_REQUIRE(budget >= 0, "budget must be >= 0");
    HOST_REQUIRE(P <= CAL_MOTIF_MAX_PATTERNS, "more than CAL_MOTIF_MAX_PATTERNS patterns");
    HOST_REQUIRE((labels == nullptr) == (pat_labels == nullptr) || N == 0 || PN == 0, "labels and pat_labels go together");
    HOST_REQUIRE(totals, "totals is null");
    HOST_REQUIRE(P == 0 || (pat_ptr && pat_edge_ptr), "pat_ptr / pat_edge_ptr are null");
    HOST_REQUIRE(PE == 0 || pat_edge_index, "pat_edge_index is null");
    std::vector<MotifPlan> plan((size_t)P);
    for (int64_t p = 0; p < P; ++p) {
        const int64_t nlo = pat_ptr[p], nhi = pat_ptr[p + 1], elo = pat_edge_ptr[p], ehi = pat_edge_ptr[p + 1];
        HOST_REQUIRE(nlo >= 0 && nlo <= nhi && nhi <= PN && elo >= 0 && elo <= ehi && ehi <= PE, "pat_ptr / pat_edge_ptr are malformed");
        HOST_REQUIRE(motif_plan(pat_edge_index, PE, elo, ehi, nlo, nhi - nlo, plan[(size_t)p]),
                     "a pattern must be connected and have 1 to CAL_MOTIF_MAX_PATTERN nodes");
    }
    totals[0] = 0;
    if (B == 0 || P == 0) return 0;
    HOST_REQUIRE(ptr && edge_ptr, "ptr / edge_ptr are null");
    HOST_REQUIRE(E == 0 || edge_index, "edge_index is null");
    HOST_REQUIRE(count && truncated && first && tgt_edges && pat_edges, "an output is null");
    const bool labelled = labels && pat_labels;
    for (int64_t p = 0; p < P; ++p) pat_edges[p] = plan[(size_t)p].edges;
    int64_t ignored = 0;
#pragma omp parallel for schedule(dynamic, 1) reduction(+ : ignored)
    for (int64_t g = 0; g < B; ++g) {
        int64_t nlo, n, elo, em;
        seg_clamp(ptr, g, N, nlo, n);
        seg_clamp(edge_ptr, g, E, elo, em);
        const bool skip = n > kMotifN;
        std::vector<MotifGraph> box(1);
        MotifGraph& G = box[0];
        G.n = skip ? 0 : (int)n;
        G.lab = labelled ? labels + nlo : nullptr;
        memset(G.adj, 0, sizeof(G.adj));
        for (int64_t e = elo; e < elo + em; ++e) {
            const int64_t u = edge_index[e] - nlo, v = edge_index[E + e] - nlo;
            if (!(u >= 0 && u < n && v >= 0 && v < n)) {
                ++ignored;
            } else if (!skip && u != v) {
                G.adj[u][v >> 6] |= 1ull << (v & 63);
                G.adj[v][u >> 6] |= 1ull << (u & 63);
            }
        }
        int64_t deg = 0;
        for (int v = 0; v < G.n; ++v)
            for (int w = 0; w < 4; ++w) deg += __builtin_popcountll(G.adj[v][w]);
        tgt_edges[g] = skip ? -1 : deg / 2;
        for (int64_t p = 0; p < P; ++p) {
            const MotifPlan& q = plan[(size_t)p];
            uint64_t cnt = 0, trc = 0, best = ~0ull;
            if (!skip) motif_search(G, q, pat_labels, induced, (uint64_t)budget, cnt, trc, best);
            count[g * P + p] = skip ? -1 : (int64_t)cnt;
            truncated[g * P + p] = (int64_t)trc;
            for (int i = 0; i < kMotifK; ++i)
                first[(g * P + p) * kMotifK + i] = cnt && i < q.k ? (int32_t)((best >> (56 - 8 * i)) & 0xFF) : -1;
        }
    }
    totals[0] = ignored;
    return 0;
}

// ---- graph centralities (cal_amd/csrc/centrality.hip; cal_amd/centrality.py): the same searches and the same order of every sum
// (rules.hpp), graph by graph, over a CSR of the distinct neighbours in ascending id.  No limit on a graph's nodes.
HOST_EXPORT int64_t cal_centrality_ws(int64_t) { return 0; }

HOST_EXPORT int cal_centrality(const int64_t* edge_index, int64_t E, int64_t N, const int64_t* ptr, const int64_t* edge_ptr,
                               int64_t B, const uint8_t* sources, double alpha, double tol, int64_t max_iter, int64_t* far,
                               int64_t* reach, int64_t* ecc, int64_t* deg, double* bc, double* ebc, double* pr, int32_t* pr_iters,
                               int32_t* hop, int64_t* skipped, int64_t* totals, void*, int64_t, void*) {
    HOST_REQUIRE(E >= 0 && N >= 0 && B >= 0, "E, N, B must be >= 0");
    HOST_REQUIRE(alpha >= 0.0 && alpha < 1.0, "alpha must be in [0, 1)");
    HOST_REQUIRE(tol >= 0.0 && max_iter >= 0 && max_iter <= 0x7FFFFFFF, "tol must be >= 0 and max_iter in [0, 2^31)");
    HOST_REQUIRE(totals, "totals is null");
    HOST_REQUIRE(!hop || sources || N == 0, "hop needs sources");
    totals[0] = 0;
    if (B == 0) return 0;
    const bool cent = pr_iters != nullptr;
    HOST_REQUIRE(!cent || ((N == 0 || (far && reach && ecc && deg && bc && pr)) && (E == 0 || ebc)),
                 "pr_iters is given: far, reach, ecc, deg, bc, ebc and pr must be");
    HOST_REQUIRE(cent || hop || N == 0, "nothing is asked for");
    HOST_REQUIRE(ptr && edge_ptr && skipped, "ptr / edge_ptr / skipped are null");
    HOST_REQUIRE(E == 0 || edge_index, "edge_index is null");
    int64_t ignored = 0;
#pragma omp parallel for schedule(dynamic, 1) reduction(+ : ignored)
    for (int64_t g = 0; g < B; ++g) {
        int64_t nlo, n, elo, em;
        seg_clamp(ptr, g, N, nlo, n);
        seg_clamp(edge_ptr, g, E, elo, em);
        skipped[g] = 0;
        // the distinct neighbours of every node, ascending
        std::vector<int64_t> rp((size_t)n + 1, 0);
        std::vector<int32_t> nb;
        {
            std::vector<std::pair<int32_t, int32_t>> pairs;
            pairs.reserve((size_t)em * 2);
            for (int64_t e = elo; e < elo + em; ++e) {
                const int64_t u = edge_index[e] - nlo, v = edge_index[E + e] - nlo;
                if (!(u >= 0 && u < n && v >= 0 && v < n)) {
                    ++ignored;
                } else if (u != v) {
                    pairs.emplace_back((int32_t)u, (int32_t)v);
                    pairs.emplace_back((int32_t)v, (int32_t)u);
                }
            }
            std::sort(pairs.begin(), pairs.end());
            pairs.erase(std::unique(pairs.begin(), pairs.end()), pairs.end());
            nb.resize(pairs.size());
            for (size_t i = 0; i < pairs.size(); ++i) {
                nb[i] = pairs[i].second;
                rp[(size_t)pairs[i].first + 1]++;
            }
            for (int64_t v = 0; v < n; ++v) rp[(size_t)v + 1] += rp[(size_t)v];
        }
        std::vector<int32_t> dist((size_t)n), order;
        order.reserve((size_t)n);
        if (hop) {                                                    // levels from the marked nodes
            std::fill(dist.begin(), dist.end(), kCentUnreached);
            for (int64_t v = 0; v < n; ++v)
                if (sources && sources[nlo + v]) {
                    dist[(size_t)v] = kCentHopSeed;
                    order.push_back((int32_t)v);
                }
            for (size_t h = 0; h < order.size(); ++h) {
                const int32_t v = order[h];
                for (int64_t i = rp[(size_t)v]; i < rp[(size_t)v + 1]; ++i)
                    if (dist[(size_t)nb[(size_t)i]] == kCentUnreached) {
                        dist[(size_t)nb[(size_t)i]] = dist[(size_t)v] + 1;
                        order.push_back(nb[(size_t)i]);
                    }
            }
            for (int64_t v = 0; v < n; ++v) hop[nlo + v] = dist[(size_t)v];
        }
        if (!cent) continue;
        std::vector<double> sig((size_t)n), q((size_t)n), delta((size_t)n);
        std::vector<double> bcp((size_t)n * kCentW, 0.0), ep((size_t)em * kCentW, 0.0);
        for (int64_t v = 0; v < n; ++v) {
            far[nlo + v] = reach[nlo + v] = ecc[nlo + v] = 0;
            deg[nlo + v] = rp[(size_t)v + 1] - rp[(size_t)v];
        }
        for (int64_t s = 0; s < n; ++s) {
            const int w = cent_wave(s);
            std::fill(dist.begin(), dist.end(), kCentUnreached);
            order.clear();
            dist[(size_t)s] = 0;
            sig[(size_t)s] = 1.0;
            order.push_back((int32_t)s);
            for (size_t h = 0; h < order.size(); ++h) {               // levels; sigma pulls from the level above, ascending
                const int32_t v = order[h];
                if (h) {
                    double sum = 0.0;
                    for (int64_t i = rp[(size_t)v]; i < rp[(size_t)v + 1]; ++i)
                        if (dist[(size_t)nb[(size_t)i]] == dist[(size_t)v] - 1) sum += sig[(size_t)nb[(size_t)i]];
                    sig[(size_t)v] = sum;
                }
                for (int64_t i = rp[(size_t)v]; i < rp[(size_t)v + 1]; ++i)
                    if (dist[(size_t)nb[(size_t)i]] == kCentUnreached) {
                        dist[(size_t)nb[(size_t)i]] = dist[(size_t)v] + 1;
                        order.push_back(nb[(size_t)i]);
                    }
            }
            for (size_t h = order.size(); h-- > 1;) {                 // the deepest level first; the source is left out
                const int32_t v = order[h];
                double acc = 0.0;
                for (int64_t i = rp[(size_t)v]; i < rp[(size_t)v + 1]; ++i)
                    if (dist[(size_t)nb[(size_t)i]] == dist[(size_t)v] + 1) acc += sig[(size_t)v] * q[(size_t)nb[(size_t)i]];
                delta[(size_t)v] = acc;
                q[(size_t)v] = cent_q(acc, sig[(size_t)v]);
                bcp[(size_t)v * kCentW + w] += acc;
            }
            for (size_t h = 0; h < order.size(); ++h) {               // (d(s, v) = d(v, s))
                const int32_t v = order[h];
                far[nlo + v] += dist[(size_t)v];
                reach[nlo + v] += 1;
                ecc[nlo + v] = std::max<int64_t>(ecc[nlo + v], dist[(size_t)v]);
            }
            for (int64_t e = 0; e < em; ++e) {
                const int64_t x = edge_index[elo + e] - nlo, y = edge_index[E + elo + e] - nlo;
                if (!(x >= 0 && x < n && y >= 0 && y < n)) continue;
                const int dx = dist[(size_t)x], dy = dist[(size_t)y];
                if (dx >= 0 && dy == dx + 1) ep[(size_t)e * kCentW + w] += sig[(size_t)x] * q[(size_t)y];
                else if (dy >= 0 && dx == dy + 1) ep[(size_t)e * kCentW + w] += sig[(size_t)y] * q[(size_t)x];
            }
        }
        for (int64_t v = 0; v < n; ++v) {
            const double* p = &bcp[(size_t)v * kCentW];
            bc[nlo + v] = cent_join(p[0], p[1], p[2], p[3]);
        }
        for (int64_t e = 0; e < em; ++e) {
            const double* p = &ep[(size_t)e * kCentW];
            ebc[elo + e] = cent_join(p[0], p[1], p[2], p[3]);
        }
        // PageRank
        std::vector<double> x((size_t)n, n ? 1.0 / (double)n : 0.0), xd((size_t)n), xn((size_t)n);
        double slots[kCentSlots];
        auto tree = [&](auto term) {
            std::fill(slots, slots + kCentSlots, 0.0);
            for (int64_t v = 0; v < n; ++v) slots[v & (kCentSlots - 1)] += term(v);
            return cent_tree_sum(slots);
        };
        auto degree = [&](int64_t v) { return rp[(size_t)v + 1] - rp[(size_t)v]; };
        double dsum = tree([&](int64_t v) { return degree(v) ? 0.0 : x[(size_t)v]; });
        int32_t it = 0;
        while (it < max_iter && n > 0) {
            for (int64_t v = 0; v < n; ++v) xd[(size_t)v] = degree(v) ? x[(size_t)v] / (double)degree(v) : 0.0;
            for (int64_t v = 0; v < n; ++v) {
                double pull = 0.0;
                for (int64_t i = rp[(size_t)v]; i < rp[(size_t)v + 1]; ++i) pull += xd[(size_t)nb[(size_t)i]];
                xn[(size_t)v] = cent_pr_step(alpha, pull, dsum, (double)n);
            }
            const double err = tree([&](int64_t v) { return fabs(xn[(size_t)v] - x[(size_t)v]); });
            x.swap(xn);
            dsum = tree([&](int64_t v) { return degree(v) ? 0.0 : x[(size_t)v]; });
            ++it;
            if (cent_pr_done(err, tol)) break;
        }
        for (int64_t v = 0; v < n; ++v) pr[nlo + v] = x[(size_t)v];
        pr_iters[g] = it;
    }
    totals[0] = ignored;
    return 0;
}

// ---- nearest neighbours in embedding space (cal_amd/csrc/knn.hip): norms and dot products in fp64, rounded once to the fp32 the key
// holds; the same keys (knn_key), eligibility, k' and vote rule.  The chunking does not change the result: chunk_rows is only checked.
HOST_EXPORT int64_t cal_knn_ws(int64_t, int64_t, int64_t, int64_t) { return 0; }

HOST_EXPORT int cal_knn(const float* Q, int64_t nq, const float* X, int64_t M, int64_t H, int metric, int64_t k, const int64_t* skip,
                        const int64_t* labels, int64_t C, int32_t* idx, float* dist, int32_t* votes, int64_t chunk_rows, void*,
                        int64_t, void*) {
    HOST_REQUIRE(nq >= 0, "nq must be >= 0");
    HOST_REQUIRE(M >= 1 && M < (1ll << 31), "M must be in [1, 2^31)");
    HOST_REQUIRE(H >= 1 && k >= 1 && C >= 0, "H and k must be >= 1, C >= 0");
    HOST_REQUIRE(metric == 0 || metric == 1, "metric must be 0 (squared Euclidean) or 1 (cosine)");
    HOST_REQUIRE(chunk_rows >= 0 && chunk_rows % 32 == 0, "chunk_rows must be 0 or a positive multiple of 32");
    if (nq == 0) return 0;
    HOST_REQUIRE(Q && X && idx && dist, "Q / X / idx / dist is null");
    HOST_REQUIRE(!votes || (labels && C >= 1), "votes needs labels and C >= 1");
    auto norm2 = [H](const float* r) {
        double s = 0.0;
        for (int64_t i = 0; i < H; ++i) s += (double)r[i] * (double)r[i];
        return s;
    };
    std::vector<double> xn((size_t)M);
#pragma omp parallel for schedule(static)
    for (int64_t j = 0; j < M; ++j) xn[(size_t)j] = norm2(X + j * H);
#pragma omp parallel for schedule(static)
    for (int64_t q = 0; q < nq; ++q) {
        const float* qr = Q + q * H;
        const double qn = norm2(qr);
        const int64_t sk = skip ? skip[q] : -1, kk = knn_count(k, M, sk);
        std::vector<uint64_t> keys;
        keys.reserve((size_t)M);
        for (int64_t j = 0; j < M; ++j) {
            if (!knn_eligible(j, sk)) continue;
            const float* xr = X + j * H;
            double dot = 0.0;
            for (int64_t i = 0; i < H; ++i) dot += (double)qr[i] * (double)xr[i];
            keys.push_back(knn_key((float)knn_dist<double>(metric, qn, xn[(size_t)j], dot), (uint32_t)j));
        }
        std::partial_sort(keys.begin(), keys.begin() + kk, keys.end());
        for (int64_t c = 0; votes && c < C; ++c) votes[q * C + c] = 0;
        for (int64_t p = 0; p < k; ++p) {
            const uint64_t key = p < kk ? keys[(size_t)p] : kKnnNone;
            idx[q * k + p] = p < kk ? knn_key_idx(key) : -1;
            dist[q * k + p] = p < kk ? knn_key_dist(key) : INFINITY;
            if (votes && p < kk && knn_votes_for(labels[knn_key_idx(key)], C)) ++votes[q * C + labels[knn_key_idx(key)]];
        }
    }
    return 0;
}

// ---- k-means on embedding rows (cal_amd/csrc/kmeans.hip): norms and dot products in fp64, the distance rounded once to the fp32 the
// key holds; the same key (kmeans_key), the same -1 rule, and the order of sums of rules.hpp in fp32: a superblock's chain in
// ascending row order, the superblocks in ascending order, kmeans_mean.
HOST_EXPORT int64_t cal_kmeans_ws(int64_t, int64_t, int64_t, int64_t) { return 0; }

namespace {
// assign[j], dist[j] of the rows [j0, j1) against the K centroids C (cn: their fp64 norms)
void km_assign_rows(const float* X, int64_t j0, int64_t j1, int64_t H, const float* C, const std::vector<double>& cn, int64_t K,
                    int32_t* assign, float* dist) {
#pragma omp parallel for schedule(static)
    for (int64_t j = j0; j < j1; ++j) {
        const float* xr = X + j * H;
        double xn = 0.0;
        for (int64_t i = 0; i < H; ++i) xn += (double)xr[i] * (double)xr[i];
        uint64_t best = kKnnNone;
        for (int64_t c = 0; c < K; ++c) {
            const float* cr = C + c * H;
            double dot = 0.0;
            for (int64_t i = 0; i < H; ++i) dot += (double)xr[i] * (double)cr[i];
            const uint64_t key = kmeans_key((float)knn_dist<double>(0, xn, cn[(size_t)c], dot), (uint32_t)c);
            best = key < best ? key : best;
        }
        assign[j] = kmeans_cluster(best);
        dist[j] = knn_key_dist(best);
    }
}
std::vector<double> km_norms(const float* C, int64_t K, int64_t H) {
    std::vector<double> cn((size_t)K);
    for (int64_t c = 0; c < K; ++c) {
        double s = 0.0;
        for (int64_t i = 0; i < H; ++i) s += (double)C[c * H + i] * (double)C[c * H + i];
        cn[(size_t)c] = s;
    }
    return cn;
}
}  // namespace

HOST_EXPORT int cal_kmeans_assign(const float* X, int64_t N, int64_t H, const float* Cn, int64_t K, int32_t* assign, float* dist,
                                  void*) {
    HOST_REQUIRE(N >= 0 && N < (1ll << 31), "N must be in [0, 2^31)");
    HOST_REQUIRE(H >= 1 && K >= 1, "H and K must be >= 1");
    if (N == 0) return 0;
    HOST_REQUIRE(X && Cn && assign && dist, "X / Cn / assign / dist is null");
    km_assign_rows(X, 0, N, H, Cn, km_norms(Cn, K, H), K, assign, dist);
    return 0;
}

HOST_EXPORT int cal_kmeans(const float* X, int64_t N, int64_t H, const float* C_in, int64_t K, int64_t iters, int64_t span_rows,
                           float* C_out, int32_t* assign, int64_t* counts, double* inertia, int64_t* moved, int32_t* iters_run,
                           void*, int64_t, void*) {
    HOST_REQUIRE(N >= 0 && N < (1ll << 31), "N must be in [0, 2^31)");
    HOST_REQUIRE(H >= 1 && K >= 1, "H and K must be >= 1");
    HOST_REQUIRE(iters >= 1 && iters < INT32_MAX, "iters must be >= 1");
    HOST_REQUIRE(span_rows >= 0 && span_rows % kKmTile == 0, "span_rows must be 0 or a positive multiple of 128");
    if (N == 0) return 0;
    HOST_REQUIRE(X && C_in && C_out && assign && counts && inertia && moved && iters_run, "a tensor is null");
    const int64_t span = kmeans_span(N, span_rows), spans = kmeans_spans(N, span);
    std::vector<int32_t> now((size_t)N);
    std::vector<float> dist((size_t)N), sum((size_t)(K * H)), part((size_t)(K * H));
    std::vector<int64_t> cnt((size_t)K);
    for (int64_t it = 0; it < iters; ++it) {
        const float* C = it == 0 ? C_in : C_out;
        km_assign_rows(X, 0, N, H, C, km_norms(C, K, H), K, now.data(), dist.data());
        int64_t mv = 0;
        for (int64_t j = 0; j < N; ++j) {
            mv += now[(size_t)j] != (it == 0 ? -1 : assign[j]);
            assign[j] = now[(size_t)j];
        }
        std::fill(cnt.begin(), cnt.end(), 0);
        double in = 0.0;
        for (int64_t s = 0; s < spans; ++s) {
            std::fill(part.begin(), part.end(), 0.f);
            double pin = 0.0;
            const int64_t j1 = std::min(N, (s + 1) * span);
            for (int64_t j = s * span; j < j1; ++j) {
                const int32_t c = assign[j];
                if (c < 0) continue;
                ++cnt[(size_t)c];
                pin += (double)dist[(size_t)j];
                float* p = part.data() + (int64_t)c * H;
                const float* xr = X + j * H;
                for (int64_t h = 0; h < H; ++h) p[h] = kmeans_add(p[h], xr[h]);
            }
            if (s == 0) {
                sum = part;
                in = pin;
            } else {
                for (int64_t i = 0; i < K * H; ++i) sum[(size_t)i] = kmeans_add(sum[(size_t)i], part[(size_t)i]);
                in += pin;
            }
        }
        for (int64_t c = 0; c < K; ++c) {
            counts[c] = cnt[(size_t)c];
            for (int64_t h = 0; h < H; ++h) C_out[c * H + h] = kmeans_mean(sum[(size_t)(c * H + h)], cnt[(size_t)c], C[c * H + h]);
        }
        inertia[it] = in;
        moved[it] = mv;
        *iters_run = (int32_t)(it + 1);
        if (mv == 0) break;
    }
    return 0;
}

// ---- surrogate attributions (cal_amd/csrc/surrogate.hip): the same fit, every operation a function of the surrogate block of
// rules.hpp in the order stated there, so the results are the device library's bit for bit.  No player limit: a dense lower
// triangle per graph, OpenMP over the graphs.
namespace {
struct SurArgs {
    const int32_t* key; int64_t K, M;
    const int64_t *rptr, *rrow, *rth, *rinv;
    const double *val, *wt; int64_t R;
    const int64_t *pptr, *pel; int64_t P;
    const double *ve, *vf; int mode; double ridge;
    double *phi, *phi0, *r2; int32_t* status;
};

void sur_fit_graph(const SurArgs& a, int64_t g) {
    const double nan = __builtin_nan("");
    int64_t plo, n, rlo, S;
    seg_clamp(a.pptr, g, a.P, plo, n);
    seg_clamp(a.rptr, g, a.R, rlo, S);
    const int mode = a.mode;
    const int64_t d = sur_dim(n, mode);
    const double ve = mode == 0 ? a.ve[g] : 0.0, vf = mode == 0 ? a.vf[g] : 0.0, delta = vf - ve;
    bool bad = mode == 0 && !(sur_finite(ve) && sur_finite(vf));
    for (int64_t p = 0; p < n; ++p) bad = bad || !sur_player_ok(a.pel[plo + p], a.M);
    std::vector<double> w((size_t)S), v((size_t)S);
    for (int64_t s = 0; s < S; ++s) {
        v[(size_t)s] = a.val[rlo + s];
        w[(size_t)s] = a.wt ? a.wt[rlo + s] : 1.0;
        bad = bad || !sur_sample_ok(v[(size_t)s], w[(size_t)s]);
    }
    auto fail = [&](int st) {
        for (int64_t p = 0; p < n; ++p) a.phi[plo + p] = nan;
        a.phi0[g] = a.r2[g] = nan;
        a.status[g] = st;
    };
    if (bad) return fail(sur_status(false, true, false));
    std::vector<uint8_t> z((size_t)(S * d));
    for (int64_t s = 0; s < S; ++s) {
        const int64_t i = rlo + s;
        for (int64_t p = 0; p < n; ++p)
            z[(size_t)(s * d + p)] = sur_member(a.key, a.K, a.M, a.rrow[i], a.pel[plo + p], a.rth[i], a.rinv && a.rinv[i] != 0);
        if (mode == 1) z[(size_t)(s * d + n)] = 1;
    }
    std::vector<double> phi((size_t)n);
    double phi0 = ve;
    bool deficient = false;
    if (sur_one_player(n, mode)) {
        phi[0] = delta;
    } else if (d > 0) {
        std::vector<double> L((size_t)(d * (d + 1) / 2)), x((size_t)d), u((size_t)d);
        auto at = [&](int64_t i, int64_t j) -> double& { return L[(size_t)(i * (i + 1) / 2 + j)]; };
        for (int64_t i = 0; i < d; ++i) {
            for (int64_t j = 0; j <= i; ++j) {
                double acc = 0.0;
                for (int64_t s = 0; s < S; ++s)
                    if (z[(size_t)(s * d + i)] && z[(size_t)(s * d + j)]) acc = sur_gram_add(acc, w[(size_t)s]);
                at(i, j) = i == j ? sur_ridge(acc, a.ridge, i, n) : acc;
            }
            double acc = 0.0;
            for (int64_t s = 0; s < S; ++s)
                if (z[(size_t)(s * d + i)]) acc = sur_rhs_add(acc, w[(size_t)s], sur_y(v[(size_t)s], ve, mode));
            x[(size_t)i] = acc;
            u[(size_t)i] = 1.0;
        }
        for (int64_t j = 0; j < d && !deficient; ++j) {
            const double ajj = at(j, j);
            double dj = ajj;
            for (int64_t k = 0; k < j; ++k) dj = sur_sub(dj, at(j, k), at(j, k));
            if (!sur_pivot_ok(dj, ajj)) {
                deficient = true;
                break;
            }
            const double ljj = sur_sqrt(dj);
            at(j, j) = ljj;
            for (int64_t i = j + 1; i < d; ++i) {
                double acc = at(i, j);
                for (int64_t k = 0; k < j; ++k) acc = sur_sub(acc, at(i, k), at(j, k));
                at(i, j) = sur_div(acc, ljj);
            }
        }
        if (!deficient) {
            for (std::vector<double>* r : {&x, &u}) {
                std::vector<double>& t = *r;
                for (int64_t i = 0; i < d; ++i) {
                    double acc = t[(size_t)i];
                    for (int64_t k = 0; k < i; ++k) acc = sur_sub(acc, at(i, k), t[(size_t)k]);
                    t[(size_t)i] = sur_div(acc, at(i, i));
                }
                for (int64_t i = d - 1; i >= 0; --i) {
                    double acc = t[(size_t)i];
                    for (int64_t k = d - 1; k > i; --k) acc = sur_sub(acc, at(k, i), t[(size_t)k]);
                    t[(size_t)i] = sur_div(acc, at(i, i));
                }
            }
            if (mode == 0) {
                double sx = 0.0, su = 0.0;
                for (int64_t i = 0; i < d; ++i) {
                    sx = sx + x[(size_t)i];
                    su = su + u[(size_t)i];
                }
                for (int64_t i = 0; i < n; ++i) phi[(size_t)i] = sur_correct(x[(size_t)i], u[(size_t)i], sx, su, delta);
            } else {
                for (int64_t i = 0; i < n; ++i) phi[(size_t)i] = x[(size_t)i];
                phi0 = x[(size_t)n];
            }
        }
    }
    if (deficient && n > 0) return fail(sur_status(false, false, true));
    if (deficient) phi0 = nan;                                     // (mode 1 without a player and without weight)
    double sw = 0.0, swv = 0.0;
    for (int64_t s = 0; s < S; ++s) {
        sw = sur_gram_add(sw, w[(size_t)s]);
        swv = sur_rhs_add(swv, w[(size_t)s], v[(size_t)s]);
    }
    const double mean = sur_div(swv, sw);
    double ssr = 0.0, sst = 0.0;
    for (int64_t s = 0; s < S; ++s) {
        double fit = phi0;
        for (int64_t p = 0; p < n; ++p)
            if (z[(size_t)(s * d + p)]) fit = fit + phi[(size_t)p];
        ssr = sur_sq_add(ssr, w[(size_t)s], v[(size_t)s] - fit);
        sst = sur_sq_add(sst, w[(size_t)s], v[(size_t)s] - mean);
    }
    for (int64_t p = 0; p < n; ++p) a.phi[plo + p] = phi[(size_t)p];
    a.phi0[g] = phi0;
    a.r2[g] = sur_r2(ssr, sst);
    a.status[g] = 0;
}
}  // namespace

HOST_EXPORT int cal_surrogate_fit(const int32_t* key, int64_t K, int64_t M, const int64_t* rep_ptr, const int64_t* rep_row,
                                  const int64_t* rep_thresh, const int64_t* rep_invert, const double* value, const double* weight,
                                  int64_t R, const int64_t* pl_ptr, const int64_t* pl_elem, int64_t P, int64_t B,
                                  const double* v_empty, const double* v_full, int mode, double ridge, double* phi, double* phi0,
                                  double* r2, int32_t* status, void*) {
    HOST_REQUIRE(K >= 0 && M >= 0 && R >= 0 && P >= 0 && B >= 0, "sizes must be >= 0");
    HOST_REQUIRE(mode == 0 || mode == 1, "mode must be 0 (shap) or 1 (lime)");
    HOST_REQUIRE(ridge >= 0.0 && sur_finite(ridge), "ridge must be finite and >= 0");
    if (B == 0) return 0;
    HOST_REQUIRE(rep_ptr && pl_ptr && phi0 && r2 && status, "rep_ptr / pl_ptr / phi0 / r2 / status is null");
    HOST_REQUIRE(R == 0 || (rep_row && rep_thresh && value), "rep_row / rep_thresh / value is null");
    HOST_REQUIRE(P == 0 || (pl_elem && phi), "pl_elem / phi is null");
    HOST_REQUIRE(mode == 1 || (v_empty && v_full), "mode 0 needs v_empty and v_full");
    const SurArgs a{key, key && M > 0 ? K : 0, M, rep_ptr, rep_row, rep_thresh, rep_invert, value, weight, R, pl_ptr, pl_elem, P,
                    v_empty, v_full, mode, ridge, phi, phi0, r2, status};
#pragma omp parallel for schedule(dynamic, 1)
    for (int64_t g = 0; g < B; ++g) sur_fit_graph(a, g);
    return 0;
}
