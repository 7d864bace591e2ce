// The phases of the per-graph attention backward (engine_attbwd.hpp: model.py:97-113 differentiated, per graph) as device functions,
// for the ATT mode of the per-graph GCNConv backward (engine_gconv_bwd_body.hpp, k_gconv_bwd_att in gconv_bwd_att.hip), which runs
// them in front of the last backbone layer's backward inside that launch: the BatchNorm table of bnc / bno, the edge phase (d deg,
// dl, its sums by source and by destination through dense [source][destination] blocks in LDS), one row of the row phase, and the
// unit's partial rows of the column sums.  Same lane layout and the same arithmetic, operation for operation, as
// k_att_bwd_graph, which keeps its own text: called from there, these functions changed that kernel's length and register
// allocation, and with it the place of every kernel behind it in the step engine's code object -- which measurably moved the time
// of steps that never take the ATT mode.  A change to one side belongs in the other
// (tests/test_gpu_att_fold.py holds the two against each other, gradient by gradient).
#pragma once
#include "engine_kernels.hpp"

namespace cal {

// Column t of the BatchNorm table, from the column's striped sums (loaded and pinned by the caller), in two halves: mean / rstd of
// bnc and bno from their batch statistics (training-mode backward: never running stats), and the means of their backward sums
template <int LDB>
__device__ __forceinline__ void att_bn_stats(const AttBwdArgs& a, const StripeVal& sc, const StripeVal& qc, const StripeVal& so, const StripeVal& qo,
                                             float (*bnk_s)[LDB], int t) {
    const double inv = (double)a.bnc.inv_n;
    const double bsc = stripe_total(sc, a.bnc.ss), bqc = stripe_total(qc, a.bnc.ss);
    const double bso = stripe_total(so, a.bno.ss), bqo = stripe_total(qo, a.bno.ss);
    const double m_c = bsc * inv, v_c = bqc * inv - m_c * m_c, m_o = bso * inv, v_o = bqo * inv - m_o * m_o;
    bnk_s[0][t] = (float)m_c; bnk_s[1][t] = 1.0f / sqrtf((float)(v_c > 0.0 ? v_c : 0.0) + a.bnc.eps);
    bnk_s[2][t] = (float)m_o; bnk_s[3][t] = 1.0f / sqrtf((float)(v_o > 0.0 ? v_o : 0.0) + a.bno.eps);
}
template <int LDB>
__device__ __forceinline__ void att_bn_dsums(const AttBwdArgs& a, const StripeVal& d1c, const StripeVal& d2c, const StripeVal& d1o, const StripeVal& d2o,
                                             float (*bnk_s)[LDB], int t) {
    const double inv = (double)a.bnc.inv_n;
    bnk_s[4][t] = (float)(stripe_total(d1c, a.dss) * inv); bnk_s[5][t] = (float)(stripe_total(d2c, a.dss) * inv);
    bnk_s[6][t] = (float)(stripe_total(d1o, a.dss) * inv); bnk_s[7][t] = (float)(stripe_total(d2o, a.dss) * inv);
}

// Edge phase, behind the barrier that publishes the cleared blocks, the slots' rows (d_oth: source, d_own: destination), dis_* and
// gs_*: d deg -> dd_*, dl per edge, its sums by source -> spv_s and by destination -> sqv_s.  Ends with a barrier.
template <int LD, class IDX>
__device__ __forceinline__ void att_edge_phase(float* Tc, float* To, float* Dm, const IDX* d_oth, const IDX* d_own,
                                               const float* dis_c_s, const float* dis_o_s, const float* gs_c_s, const float* gs_o_s,
                                               float* dd_c_s, float* dd_o_s, float* spv_s, float* sqv_s,
                                               const float (&dgc)[2], const float (&dgo)[2], const float (&dwc)[2], const float (&dwo)[2],
                                               int t, int rows, int ne, float fedge, float loop_w) {
    // ---- d deg -------------------------------------------------------------------------------------------------------
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int s = t + u * 512;
        if (s < ne) {
            const int r = d_oth[s], q = d_own[s];
            atomicAdd(&Tc[r * LD + q], dgc[u] * dwc[u]);
            atomicAdd(&To[r * LD + q], dgo[u] * dwo[u]);
        }
    }
    __syncthreads();
    {   // node v, branch k, quarter p of the other endpoints: out-edges v -> j (row v) and in-edges j -> v (column v)
        const int v = t >> 3, k = (t >> 2) & 1, p = t & 3;
        const float* T = k ? To : Tc;
        const float* dsv = k ? dis_o_s : dis_c_s;
        // (unconditional over the lane's 16 columns: entries past the graph are zero, and so is their deg^-1/2; with
        //  `if (j < rows)` inside, every iteration was a branch with its own LDS round trip)
        float acc = 0.f;
        float tv[16], tw[16], dj[16];
#pragma unroll
        for (int jj = 0; jj < 16; ++jj) {
            const int j = p * 16 + jj;
            tv[jj] = T[v * LD + j]; tw[jj] = T[j * LD + v]; dj[jj] = dsv[j];
        }
#pragma unroll
        for (int jj = 0; jj < 16; ++jj) acc = fmaf(tv[jj] + tw[jj], dj[jj], acc);
        acc += __shfl_xor(acc, 1, 64);
        acc += __shfl_xor(acc, 2, 64);
        if (v < rows && p == 0) {                     // + the self loop; d deg = d(deg^-1/2) chain
            const float d = dsv[v], gsv = (k ? gs_o_s : gs_c_s)[v];
            (k ? dd_o_s : dd_c_s)[v] = -0.5f * d * d * d * (acc + 2.f * gsv * d * loop_w);
        }
    }
    __syncthreads();
    // ---- dl per edge r -> q (an input self loop carries no gradient: k_normbwd_edge), summed by source / by destination --
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int s = t + u * 512;
        if (s < ne) {
            const int r = d_oth[s], q = d_own[s];
            const float xc = dgc[u] * dis_c_s[r] * dis_c_s[q] + dd_c_s[r];
            const float xo = dgo[u] * dis_o_s[r] * dis_o_s[q] + dd_o_s[r];
            if (r != q) atomicAdd(&Dm[r * LD + q], fedge * dwc[u] * dwo[u] * (xc - xo));
        }
    }
    __syncthreads();
    {
        const int v = t >> 3, k = (t >> 2) & 1, p = t & 3;
        float acc = 0.f;
        float dv[16];
#pragma unroll
        for (int jj = 0; jj < 16; ++jj) { const int j = p * 16 + jj; dv[jj] = Dm[k ? j * LD + v : v * LD + j]; }
#pragma unroll
        for (int jj = 0; jj < 16; ++jj) acc += dv[jj];
        acc += __shfl_xor(acc, 1, 64);
        acc += __shfl_xor(acc, 2, 64);
        if (v < rows && p == 0) (k ? sqv_s : spv_s)[v] = acc;
    }
    __syncthreads();
}

// the row phase's constants of the lane's columns c .. c + VEC - 1 (cc: clamped), from the table and the pinned loads
template <int VEC, int LDB>
__device__ __forceinline__ void att_row_consts(const float (*bnk_s)[LDB], int c, int cc, bool cok, int H,
                                               float (&mc)[VEC], float (&rc)[VEC], float (&gc)[VEC], float (&m1c)[VEC], float (&m2c)[VEC],
                                               float (&mo)[VEC], float (&ro)[VEC], float (&go)[VEC], float (&m1o)[VEC], float (&m2o)[VEC],
                                               const float (&w0)[VEC], const float (&w1)[VEC], const float (&w2)[VEC], const float (&w3)[VEC],
                                               const float (&w4)[VEC], const float (&w5)[VEC], float (&wn)[VEC], float (&wp)[VEC], float (&wq)[VEC]) {
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        const bool on = cok && c + j < H;
        mc[j] = bnk_s[0][cc + j]; rc[j] = bnk_s[1][cc + j]; mo[j] = bnk_s[2][cc + j]; ro[j] = bnk_s[3][cc + j];
        gc[j] = on ? gc[j] * rc[j] : 0.f; go[j] = on ? go[j] * ro[j] : 0.f;
        m1c[j] = bnk_s[4][cc + j]; m2c[j] = bnk_s[5][cc + j];
        m1o[j] = bnk_s[6][cc + j]; m2o[j] = bnk_s[7][cc + j];
        wn[j] = on ? w0[j] - w1[j] : 0.f; wp[j] = on ? w2[j] - w3[j] : 0.f; wq[j] = on ? w4[j] - w5[j] : 0.f;
    }
}

// One row i of the row phase on the G lanes of its group (x4: the row of x; hc4 / ho4: of dXc_hat / dXo_hat, slice partials added).
// own: the lane's columns are the caller's to write -- it adds them to the column sums and st(i, o) stores their dZ values.
template <int VEC, int G, class St>
__device__ __forceinline__ void att_row_item(const AttBwdArgs& a, int relu, int i, int rend, int l, bool cok, bool own,
                                             const Vec<VEC>& x4, const Vec<VEC>& hc4, const Vec<VEC>& ho4, float a0, float a1,
                                             const float (&mc)[VEC], const float (&rc)[VEC], const float (&gc)[VEC], const float (&m1c)[VEC], const float (&m2c)[VEC],
                                             const float (&mo)[VEC], const float (&ro)[VEC], const float (&go)[VEC], const float (&m1o)[VEC], const float (&m2o)[VEC],
                                             const float (&wn)[VEC], const float (&wp)[VEC], const float (&wq)[VEC],
                                             const float* spv_s, const float* sqv_s, double (&cs)[4][VEC], double& sdl, double& ssp, St st) {
    float xv[VEC], dxc[VEC], dxo[VEC];
    float d0 = 0.f, d1 = 0.f;
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
        xv[j] = cok ? x4.get(j) : 0.f;
        const float xcn = (a0 * xv[j] - mc[j]) * rc[j], xon = (a1 * xv[j] - mo[j]) * ro[j];
        dxc[j] = cok ? gc[j] * (hc4.get(j) - m1c[j] - xcn * m2c[j]) : 0.f;
        dxo[j] = cok ? go[j] * (ho4.get(j) - m1o[j] - xon * m2o[j]) : 0.f;
        d0 = fmaf(dxc[j], xv[j], d0);
        d1 = fmaf(dxo[j], xv[j], d1);
    }
    d0 = group_sum<G>(d0); d1 = group_sum<G>(d1);
    const float dl0 = a.fnode * a0 * a1 * (d0 - d1);
    if (i < rend) {
        const float spv = spv_s[i], sqv = sqv_s[i];
        if (l == 0) { sdl += (double)dl0; ssp += (double)spv; }
        if (own) {
            float o[VEC];
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                float dx = a0 * dxc[j] + a1 * dxo[j] + dl0 * wn[j] + spv * wp[j] + sqv * wq[j];
                if (relu && !(xv[j] > 0.f)) dx = 0.f;
                o[j] = dx;
                cs[0][j] += (double)dx;
                cs[1][j] += (double)(dl0 * xv[j]);
                cs[2][j] += (double)(spv * xv[j]);
                cs[3][j] += (double)(sqv * xv[j]);
            }
            st(i, o);
        }
    }
}

// The unit's partial rows of the column sums behind d bias_L, d node_att_mlp, d edge_att_mlp, in two steps around a barrier.
// Before it: lanes of a wave that hold the same column (64 / G groups per wave) combine by shuffle; the wave's sums go to red
// (the lane's columns are rc .. rc + VEC - 1 of the caller's NC, if it owns any) and its two scalars to sc_lds.
template <int VEC, int G, int NC>
__device__ __forceinline__ void att_colsum_waves(const double (&cs)[4][VEC], double sdl, double ssp, double (*red)[4][NC], double (*sc_lds)[8],
                                                 int t, int l, int rc, bool own) {
    const int wv = t >> 6;
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            double v = cs[q][j];
            if (G < 64) for (int off = G; off < 64; off <<= 1) v += __shfl_xor(v, off, 64);
            if ((t & 63) < G && own) red[wv][q][rc + j] = v;
        }
    if (l == 0) {
        // one value per group: groups of a wave sit G lanes apart
        double s0 = sdl, s1 = ssp;
        if (G < 64) for (int off = G; off < 64; off <<= 1) { s0 += __shfl_xor(s0, off, 64); s1 += __shfl_xor(s1, off, 64); }
        if ((t & 63) == 0) { sc_lds[0][wv] = s0; sc_lds[1][wv] = s1; }
    }
}
// Behind it: lanes tt = 0 .. nt - 1 add the 8 waves (512 threads: all of them hold rows) and write the columns col0 .. col0 + ncols - 1
// of the partial rows; lane 0 also writes the two scalars (d bn0 at dWn[H], d be0 at dWe[2H]) when `scalars`.
template <int NC>
__device__ __forceinline__ void att_colsum_store(const AttBwdArgs& a, const double (*red)[4][NC], const double (*sc_lds)[8], int tt, int nt,
                                                 int col0, int ncols, int H, bool scalars) {
    for (int idx = tt; idx < 4 * ncols; idx += nt) {
        const int q = idx / ncols, rc = idx - q * ncols, col = col0 + rc;
        double tot = 0.0;
#pragma unroll
        for (int w8 = 0; w8 < 8; ++w8) tot += red[w8][q][rc];
        if (q == 0) { if (a.dbias.on()) a.dbias.add(col, tot); }
        else if (q == 1) a.dWn.add(col, tot);
        else if (q == 2) a.dWe.add(col, tot);
        else a.dWe.add(H + col, tot);
    }
    if (tt == 0 && scalars) {
        double t0 = 0.0, t1 = 0.0;
        for (int k = 0; k < 8; ++k) { t0 += sc_lds[0][k]; t1 += sc_lds[1][k]; }
        a.dWn.add(H, t0);
        a.dWe.add(2 * H, t1);
    }
}

}  // namespace cal
