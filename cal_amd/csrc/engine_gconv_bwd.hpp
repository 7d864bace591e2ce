// Per-graph fused backward of a GCN convolution of the step engine (the transpose of engine_gconv.hpp):
// with dOut = gradient w.r.t. the convolution's pre-activation output, x' = BN(rs * x) its (normalised)
// input and z = x' W,
//     dz  = A_hat^T dOut                       (gcn_conv.py:92-104 backward)
//     dX' = dz W^T  (+ the two BatchNorm-backward column sums  sum dX',  sum dX' * x_hat)
//     dW  = x'^T dz
// as ONE kernel instead of transposed aggregation -> dX GEMM + dW GEMM.  A workgroup owns one graph and a
// 64-column slice `ns` of the OUTPUT features: it aggregates only its slice of dz (dense adjacency block
// on MFMA, like the forward), multiplies it with W[:, ns]^T into a PARTIAL dX' over all K input columns
// (the H/64 slices are summed by the consumer: k_bn_bwd / k_att_bwd read both partials) and with x'^T into
// the columns `ns` of this graph's dW slab (the B slabs are summed by k_finish, as split-K slabs were).
// dz never goes to HBM and neither product re-reads it.
//
//   grid (B graphs, H / 64 slices, branches), 512 threads; graphs of at most 64 nodes / 1024 stored edges
//   (cal_engine_set_graph_bounds), K = H in {64, 128}.  LDS ~115-135 KB: one workgroup per CU, so it brings its
//   own latency hiding: 8 waves, and twice as many loads are in flight while staging.  Behind dz both products only
//   need dz.  Order 1 (CAL_GCB_ORDER below, the non-LEAN instantiations): all eight waves run the dX' product, one
//   32 x 32 tile each, then all eight the dW product -- what other workgroups and the next kernel wait for (the dX'
//   tiles, the column-sum fold, the striped atomics) leaves under dW's MFMAs, and dW's slab has no reader before
//   k_finish.  Order 0 (LEAN): waves 0-3 run dX' and its epilogue while waves 4-7 run dW.
#pragma once
#include "engine_gconv.hpp"
#include "engine_attphases.hpp"

namespace cal {

// Order of the two products behind P1, chosen at build time (-DCAL_GCB_ORDER=0|1 through CAL_HIPCC_EXTRA of build.py).
// 0: waves 0-3 run dX' and its epilogue while waves 4-7 run dW.  1: all eight waves run dX' (one 32 x 32 tile each), then all
// eight run dW, so that the dX' tiles, the column-sum fold and the striped atomics leave under dW's MFMAs instead of behind
// them.  Same results bit for bit.  The LEAN instantiations keep order 0 (their W rows are L2 reads in the dX' product, which
// order 1 doubles); 2 = order 1 in the LEAN instantiations too, a measuring build only.  The default is what the A/B of
// profiles/r10/ab_bwd_order.txt decided.
// Order 1 lives in the translation units that define CAL_GCB_UNIT in front of this header (gconv_bwd_seq.hip: the non-LEAN
// instantiations of k_gconv_bwd; gconv_bwd_att.hip: the ATT entry).  engine.hip always compiles order 0, the text it has always
// had: its k_gconv_bwd instantiations serve the LEAN launches (and every launch of an order-0 build), and its code object does
// not move when the order changes (steps that never launch these kernels lost 0.1-0.45 % when it did).
#ifndef CAL_GCB_ORDER
#define CAL_GCB_ORDER 1
#endif
#ifdef CAL_GCB_UNIT
constexpr bool GCB_SEQ = CAL_GCB_ORDER != 0, GCB_SEQ_LEAN = CAL_GCB_ORDER == 2;
#else
constexpr bool GCB_SEQ = false, GCB_SEQ_LEAN = false;
#endif

constexpr int GB_NT = 512;                // threads per workgroup
constexpr int GB_T = 64;                  // nodes per graph
constexpr int GB_E = 1024;                // stored edges per graph
constexpr int GB_LDJ = GB_T + 1;          // k-major tiles indexed by a node: adjacency block, dz^T
constexpr int GB_LDD = GC_N + 4;          // row-major [node][64 output columns]: dOut slice, dz
constexpr int GB_LDW = GC_K + 1;          // W slice transposed: Wt[n][k_in]
constexpr int GB_LDX = GC_K + 4;          // row-major [node][K]: normalised input rows

struct GconvBwdBranch {
    const float* dout;       // [N,H]
    const float* x;          // [N,K] raw layer input
    const float* W;          // [K,H]
    const float* ew;         // per-edge weight in edge-id order, or null
    const float* dis;        // [N]
    const float* rs;         // per-row scale of x, or null
    int rs_stride;
    BNRef bn;                // BatchNorm applied to rs * x (batch statistics of the forward)
    float* dxp0; float* dxp1; // [N,K] partial dX' of output-column slice 0 / 1
    float* slab;             // [B][K,H] per-graph dW
    double* dot_parts;       // [B * H/64][2K]: (sum dX', sum dX' * x_hat) partial rows
    double* dacc_sum; double* dacc_prod; int dacc_ss;    // or (non-null): added atomically into the workgroup's plane of the site's
                                                         // NSTRIPE accumulator planes (engine.hpp: stripe_sum; no finishing launch)
    const float* coef_in;    // edge coefficients dis_j * w_e in CSR-slot order, written by the forward kernel, or null
    // UP variant: dOut is not materialised.  It is the BatchNorm-backward (+ ReLU mask) of the layer ABOVE,
    //     dOut = relu'(y) * gamma_u rstd_u (dY - m1_u - y_hat m2_u),   dY = dy0 + dy1,
    // computed while the slice is staged (what k_bn_bwd would have written and this kernel read back), and its
    // per-graph column sums (the bias gradient of this convolution) go to bias_parts [B][H].
    const float* dy0; const float* dy1;      // partials of the upper layer's dX' (dy1 null when H == 64)
    const float* y;                          // [N,H] this convolution's output after ReLU = the upper BatchNorm's input
    BNRef ubn;                               // the upper BatchNorm
    const double* udot_sum; const double* udot_prod;
    double* bias_parts;
    // POOL variant (the two weighted convolutions under global_add_pool, model.py:112-116): dOut is not materialised
    // either -- dOut[v] = relu'(out[v]) * g_b with g_b = gp0[b] (+ gp1[pb], pb = iperm[b] or b) the gradient of graph b's
    // pooled row (y = the convolution's output, bias_parts as above) -- and the kernel also emits this slice's part of
    //     gn[e] = <dOut[col_e], z[row_e]>,   gself[v] = <dOut[v], z[v]>
    // (the SDDMM behind the edge-weight gradients, gcn_conv.py:63-70,97 differentiated) from LDS while P1 runs.
    const float* gp0; const float* gp1; const int* iperm;
    const float* z;          // [N,H] x' W of the forward
    float* gn; float* gself; // this branch's [E] / [N] partials of slice 0; slice 1 is gn_stride / gself_stride further
    size_t gn_stride, gself_stride;
    int gn_slot;             // gn is written in CSR-slot order (gn[eptr[b] + s], for the per-graph attention backward) instead of edge-id order
    // packed batch (TILED instantiation of the POOL variant, cal_engine_set_tiles): the unit is a tile of the consecutive
    // graphs [tile_gptr[b], tile_gptr[b + 1]); gp0 / gp1 / iperm are per GRAPH, batch [N] names the graph of every row
    const int64_t* batch;
    const int64_t* tile_gptr;
};

struct GconvBwdBranch2 { GconvBwdBranch b[2]; };
// `ga` of the body in the modes that have no attention operands (a dependent type, so that the discarded ATT blocks compile)
struct GconvBwdNoAtt {};
template <int MODE> struct GconvBwdNoAttOf { using type = GconvBwdNoAtt; };

// LEAN (MODE 0 / 1, the single-branch launches; round 5): under 80 KB of LDS and 128 registers, so TWO workgroups share a CU
// and a launch of more workgroups than CUs (a packed batch: 240 tiles x 2 slices at NCI1-like batches of 512 graphs) stops
// running as two rounds of latency chains -- the W slice is not staged (waves 0-3 read their rows of it straight from L2 as
// MFMA operands in P2: 16-byte reads of a 64 KB matrix every workgroup shares), the x_hat rows have no padding (no access to
// them is strided by a row), CSR neighbours are 16-bit.  The POOL variant (MODE 2) also holds the z rows for the SDDMM: 140 KB,
// one workgroup per CU.
// ATT (MODE 3, the last backbone layer behind the per-graph attention backward): dOut is not materialised either -- it is the dZ
// of k_att_bwd_graph (engine_attbwd.hpp), whose phases (engine_attphases.hpp) run here in front of the products: the loads of both kernels go out together
// (one CSR slot batch serves both; the W slice and rows 32-63 as a second batch behind the BatchNorm table, or the kernel spills), the edge phase's three 64 x 65 blocks live in the W / x_hat stages (whose
// registers wait, as the LEAN POOL variant's x_hat does), and the row phase walks all rows x all H columns (dl0 needs the
// full-width dots) while only the lanes of this slice's columns write dOut and add to the column sums: the partial rows of
// d bias_L / d Wn / d We are one per unit, the slices write disjoint columns, slice 0 the two scalars.  No dZ round trip, no
// launch boundary, one prologue.
// Chosen per launch (gconv_bwd in engine.hip): a launch of at most one workgroup per CU keeps the staged W slice -- with one
// workgroup on a CU the two L2 round trips of P2's operand reads are exposed (config 2: 0.2386 -> 0.2418 ms with LEAN everywhere).
template <bool RS, int MODE, bool TILED = false, bool LEAN = false>      // MODE 0: dOut given; 1: UP (from the upper layer's partials); 2: POOL (+ gn / gself)
__global__ void __launch_bounds__(GB_NT, (LEAN ? 4 : 1)) k_gconv_bwd(const CSR g, const int* __restrict__ gptr, const int* __restrict__ eptr,
                                                   const GconvBwdBranch2 bb, float loop_w, int N, int H,
                                                   int K, int* __restrict__ status) {
    static_assert(MODE != 3, "the ATT mode is the kernel k_gconv_bwd_att (gconv_bwd_att.hip)");
    [[maybe_unused]] const typename GconvBwdNoAttOf<MODE>::type ga{};    // (what the ATT blocks of the body name; they are discarded here)
#include "engine_gconv_bwd_body.hpp"
}

// ------------------------------------------------------------------------------------------------------------------
// Backward of the feature layer h0 = relu(BN0(x0) W_feat) (model.py:90-91, a GCNConv with gfn=True: no aggregation)
// per graph, fed like the UP variant above: dZ = BatchNorm_1-backward(dy0 + dy1) masked by h0 > 0 is built in LDS
// from the first backbone layer's partial dX', then
//     dW_feat (this graph's slab [F,H]) = x0_hat'^T dZ,   (sum dX0, sum dX0 * x0_hat) per feature with dX0 = dZ W_feat^T
// (the BatchNorm_0 affine gradients).  F is small (10 for SPMotif): plain FMA loops on LDS operands; replaces k_bn_bwd +
// the dual GEMM of the unfused path.  grid (B), 512 threads, graphs of at most FB_T nodes, F <= FB_F.
// ------------------------------------------------------------------------------------------------------------------
constexpr int FB_T = 64, FB_F = 64, FB_H = 128;
struct FeatBwdArgs {
    const float* dy0; const float* dy1;      // partials of the first backbone layer's dX' (dy1 null when H == 64)
    const float* y;                          // h0 [N,H]
    BNRef ubn; const double* udot_sum; const double* udot_prod;     // BatchNorm_1
    const float* x0;                         // [N,F]
    const float* W;                          // [F,H]
    BNRef bn0;
    float* slab;                             // [B][F,H]
    double* parts;                           // [B][2F]: (sum dX0, sum dX0 * x0_hat)
};
// gptr == null (round 6: graphs of 129-256 nodes behind the wide convolutions, engine_gwide.hpp): the units are uniform chunks of FB_T
// ROWS of the batch, b * FB_T .. -- nothing here looks at the graph structure (dW_feat and the two BatchNorm_0 sums are sums over
// rows), so a 240-node graph is simply four units with a slab and a partial row each.
// FMAX: the LDS arrays' feature capacity (16: 46 KB, three workgroups per CU -- SPMotif's F = 10 over 470 row chunks was two rounds
// of one workgroup per CU at 100 KB; 64: any F <= FB_F)
template <int FMAX>
__global__ void __launch_bounds__(GB_NT) k_feat_bwd(const int* __restrict__ gptr, const FeatBwdArgs a, int H, int F,
                                                  int* __restrict__ status, int N) {
    __shared__ __attribute__((aligned(16))) float Dz[FB_T * (FB_H + 4)];     // dZ rows [j][n]
    __shared__ float Xn[FB_T * FMAX];                    // x0_hat rows [j][f] (normalised, no affine)
    __shared__ __attribute__((aligned(16))) float Ws[FMAX * (FB_H + 4)];     // W_feat [f][n]
    __shared__ float um_s[FB_H], ur_s[FB_H], ug_s[FB_H], u1_s[FB_H], u2_s[FB_H];
    __shared__ float m0_s[FMAX], r0_s[FMAX], g0_s[FMAX], b0_s[FMAX];
    __shared__ float dX0[FB_T * FMAX];
    BLK_CLK(0);
    warm_kernargs<sizeof(FeatBwdArgs) + 32>();
    const int b = blockIdx.x, t = threadIdx.x, LDZ = FB_H + 4;
    const int g0 = gptr ? gptr[b] : b * FB_T, rows = gptr ? gptr[b + 1] - g0 : min(FB_T, N - g0);
    float* slab = a.slab + (size_t)b * F * H;
    double* parts = a.parts + (size_t)b * 2 * F;
    if (rows <= 0 || rows > FB_T) {
        if (rows > 0 && t == 0) atomicOr(status, 8);
        for (int i = t; i < F * H; i += GB_NT) slab[i] = 0.f;
        for (int i = t; i < 2 * F; i += GB_NT) parts[i] = 0.0;
        return;
    }
    const int H4 = H >> 2;
    // all loads first: the two partials and h0 (rows x H/4 float4 each, <= 8 per lane), x0, W, BN constants
    RoBatch<float4, 4> b0, b1, by, bwt;
    const float* d1 = a.dy1 ? a.dy1 : a.dy0;
    ro_issue<GB_NT>(b0, rows, H4, [&](int j, int c) { return *reinterpret_cast<const float4*>(a.dy0 + (size_t)(g0 + j) * H + 4 * c); });
    ro_issue<GB_NT>(b1, rows, H4, [&](int j, int c) { return *reinterpret_cast<const float4*>(d1 + (size_t)(g0 + j) * H + 4 * c); });
    ro_issue<GB_NT>(bwt, F, H4, [&](int f, int c) { return *reinterpret_cast<const float4*>(a.W + (size_t)f * H + 4 * c); });
    ro_issue<GB_NT>(by, rows, H4, [&](int j, int c) { return *reinterpret_cast<const float4*>(a.y + (size_t)(g0 + j) * H + 4 * c); });
    float xr[8];                                         // x0[g0 .. g0 + rows) is contiguous: rows * F <= 4096 floats
#pragma unroll
    for (int u = 0; u < 8; ++u) xr[u] = a.x0[(size_t)g0 * F + min(t + u * GB_NT, rows * F - 1)];
    // BatchNorm constants: unconditional loads on clamped columns, pinned with the tile loads (BNRaw, engine.hpp)
    const int uc = min(t, H - 1), fc = min(max(t - 128, 0), F - 1);
    BNRawS uraws = bn_raws_load(a.ubn, uc);              // (striped readers, engine.hpp)
    BNRaw raw0 = bn_raw_load(a.bn0, fc);
    StripeVal ud1s = stripe_load(a.udot_sum, uc, a.ubn.ss), ud2s = stripe_load(a.udot_prod, uc, a.ubn.ss);
    bn_raws_pin(uraws); bn_raw_pin(raw0);
    stripe_pin(ud1s); stripe_pin(ud2s);
    if (t < H) bn_table_upper(a.ubn, uraws, ud1s, ud2s, t, um_s, ur_s, ug_s, u1_s, u2_s);
    else if (t - 128 < F && t >= 128) {
        const int f = t - 128;
        float m1, r1;
        bn_raw_mean_rstd(a.bn0, raw0, m1, r1);
        m0_s[f] = m1; r0_s[f] = r1;
        g0_s[f] = raw0.g;
        b0_s[f] = raw0.b;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) asm volatile("" : "+v"(xr[u]));
    ro_commit<GB_NT>(bwt, F, H4, [&](int f, int c, const float4 v) { *reinterpret_cast<float4*>(Ws + f * LDZ + 4 * c) = v; });
    __syncthreads();
    {
        const bool two = a.dy1 != nullptr;
#pragma unroll
        for (int u = 0; u < 4; ++u) { ro_pin(b1.v[u]); ro_pin(by.v[u]); }
        // item (u, t) of a rows x H4 grid: walked like ro_commit does
        const int q = GB_NT / H4, r = GB_NT % H4;
        int row = t / H4, col = t % H4;
#pragma unroll
        for (int u = 0; u < 4; ++u) ro_pin(b0.v[u]);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (t + u * GB_NT < rows * H4) {
                const float4 v0 = b0.v[u], v1 = b1.v[u], yv = by.v[u];
                const int c = 4 * col;
                const float d[4] = {v0.x + (two ? v1.x : 0.f), v0.y + (two ? v1.y : 0.f), v0.z + (two ? v1.z : 0.f), v0.w + (two ? v1.w : 0.f)};
                const float yy[4] = {yv.x, yv.y, yv.z, yv.w};
                float o[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float yn = (yy[k] - um_s[c + k]) * ur_s[c + k];
                    const float g1 = ug_s[c + k] * (d[k] - u1_s[c + k] - yn * u2_s[c + k]);
                    o[k] = yy[k] > 0.f ? g1 : 0.f;
                }
                *reinterpret_cast<float4*>(Dz + row * LDZ + c) = make_float4(o[0], o[1], o[2], o[3]);
            }
            row += q; col += r;
            if (col >= H4) { col -= H4; ++row; }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = t + u * GB_NT;
            if (i < rows * F) { const int f = i % F; Xn[(i / F) * FMAX + f] = (xr[u] - m0_s[f]) * r0_s[f]; }
        }
    }
    __syncthreads();
    BLK_CLK(2);
    // dW_feat slab: output (f, 4 consecutive n), reduction over the graph's rows; x0_hat' = gamma0 x0_hat + beta0
    for (int o = t; o < F * H4; o += GB_NT) {
        const int f = o / H4, n = 4 * (o % H4);
        const float gam = g0_s[f], bet = b0_s[f];
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
        for (int j = 0; j < rows; ++j) {
            const float xv = fmaf(Xn[j * FMAX + f], gam, bet);
            const float4 d = *reinterpret_cast<const float4*>(Dz + j * LDZ + n);
            acc.x = fmaf(xv, d.x, acc.x); acc.y = fmaf(xv, d.y, acc.y); acc.z = fmaf(xv, d.z, acc.z); acc.w = fmaf(xv, d.w, acc.w);
        }
        *reinterpret_cast<float4*>(slab + (size_t)f * H + n) = acc;
    }
    BLK_CLK(3);
    // BatchNorm_0 backward sums: dX0[j][f] = <dZ[j], W[f]>: lane = (row j = t / 4, quarter qn of the H columns) keeps its
    // quarter row of dZ in registers and walks the features; then one lane per feature sums over the rows (fixed order)
    {
        const int j = (t & 255) >> 2, qn = t & 3, nq4 = H >> 4;  // float4s per quarter row (H % 16 == 0)
        const int fh = (F + 1) >> 1, f_lo = t < 256 ? 0 : fh, f_hi = t < 256 ? fh : F;     // the two halves of the block split the features
        // (reads unconditional on a clamped float4 index, masked afterwards: `k < nq4 ? read : 0` compiles to one branch with
        //  its own LDS round trip per element -- 40 serial reads in the feature loop below)
        float4 dz[FB_H / 16];
#pragma unroll
        for (int k = 0; k < FB_H / 16; ++k)
            dz[k] = *reinterpret_cast<const float4*>(Dz + min(j, rows - 1) * LDZ + 4 * (qn * nq4 + min(k, nq4 - 1)));
#pragma unroll
        for (int k = 0; k < FB_H / 16; ++k) { ro_pin(dz[k]); if (k >= nq4) dz[k] = make_float4(0.f, 0.f, 0.f, 0.f); }
        for (int f = f_lo; f < f_hi; ++f) {
            const float4* wr = reinterpret_cast<const float4*>(Ws + f * LDZ) + qn * nq4;
            float4 wv[FB_H / 16];
#pragma unroll
            for (int k = 0; k < FB_H / 16; ++k) wv[k] = wr[min(k, nq4 - 1)];
            float p = 0.f;
#pragma unroll
            for (int k = 0; k < FB_H / 16; ++k) p = dot4(dz[k], wv[k], p);
            p += __shfl_xor(p, 1, 64);
            p += __shfl_xor(p, 2, 64);
            if (qn == 0 && j < rows) dX0[j * FMAX + f] = p;
        }
    }
    __syncthreads();
    // eight lanes per feature, each over every eighth row (<= 8 terms, fp32), combined in fp64 by shuffle: one lane per
    // feature walked the graph's rows as a chain of 57 dependent LDS round trips + fp64 adds while 500 lanes idled
    {
        const int f = t >> 3, p = t & 7, fc = min(f, F - 1);
        float a1 = 0.f, a2 = 0.f;
        float dv[FB_T / 8], xv[FB_T / 8];
#pragma unroll
        for (int u = 0; u < FB_T / 8; ++u) {
            const int j = min(p + 8 * u, rows - 1);
            dv[u] = dX0[j * FMAX + fc]; xv[u] = Xn[j * FMAX + fc];
        }
#pragma unroll
        for (int u = 0; u < FB_T / 8; ++u) {
            const float v = p + 8 * u < rows ? dv[u] : 0.f;
            a1 += v; a2 = fmaf(v, xv[u], a2);
        }
        double s1 = (double)a1, s2 = (double)a2;
#pragma unroll
        for (int o = 1; o < 8; o <<= 1) { s1 += __shfl_xor(s1, o, 64); s2 += __shfl_xor(s2, o, 64); }
        if (p == 0 && f < F) { parts[f] = s1; parts[F + f] = s2; }
    }
    BLK_CLK(1);
}

// ------------------------------------------------------------------------------------------------------------------
// The same feature-layer backward on the matrix cores, for any F <= FM_F (one-hot degree features of the TU datasets:
// F = 109 / 139, datasets.py:16-20) -- and without the dX0 = dZ W_feat^T product at all.  With P = x0_hat^T dZ (this unit's
// [F,H] block) and cs = column sums of dZ, everything the layer needs is linear in P:
//     dW_feat   = (gamma0 x0_hat + beta0)^T dZ  = gamma0[f] P[f,:] + beta0[f] cs
//     sum_j dX0[j,f]            = <W[f,:], cs>            (dX0 = dZ W^T)
//     sum_j dX0[j,f] x0_hat[j,f] = <W[f,:], P[f,:]>
// so one MFMA product per unit replaces two products and a row pass.  NOBN: the layer above is not behind a BatchNorm
// (CausalGIN: h0 feeds GINConv directly): dZ = (dy0 + dy1) masked by h0 > 0.
//   grid (units), 512 threads; XU = x0 loads per lane (8: F <= 64, 20: F <= 160).
// ------------------------------------------------------------------------------------------------------------------
constexpr int FM_F = 160;
template <int XU, bool NOBN>
__global__ void __launch_bounds__(GB_NT) k_feat_bwd_mma(const int* __restrict__ gptr, const FeatBwdArgs a, int H, int F,
                                                      int* __restrict__ status) {
    constexpr int FP = XU == 8 ? 64 : FM_F, LDXN = FP + 1, LDZ = FB_H + 4;
    __shared__ __attribute__((aligned(16))) float Dz[FB_T * LDZ];           // dZ rows [j][n]
    __shared__ float Xn[FB_T * LDXN];                    // x0_hat rows [j][f] (normalised, no affine), zero beyond F / rows
    __shared__ float um_s[FB_H], ur_s[FB_H], ug_s[FB_H], u1_s[FB_H], u2_s[FB_H];
    __shared__ float m0_s[FP], r0_s[FP], g0_s[FP], b0_s[FP];
    __shared__ float cs_s[FB_H];
    __shared__ float csp[GB_NT / 64][32][4];
    __shared__ float s12[2][4][FP];                      // per column tile: partial <W[f,:], cs>, <W[f,:], P[f,:]>
    __shared__ float red_s[GB_NT / 64][2][32][33];       // per wave: the two product tiles [feature][column], summed over the columns
    BLK_CLK(0);
    warm_kernargs<sizeof(FeatBwdArgs) + 32>();
    const int b = blockIdx.x, t = threadIdx.x;
    const int g0 = gptr[b], rows = gptr[b + 1] - g0;
    float* slab = a.slab + (size_t)b * F * H;
    double* parts = a.parts + (size_t)b * 2 * F;
    if (rows <= 0 || rows > FB_T) {
        if (rows > 0 && t == 0) atomicOr(status, 8);
        for (int i = t; i < F * H; i += GB_NT) slab[i] = 0.f;
        for (int i = t; i < 2 * F; i += GB_NT) parts[i] = 0.0;
        return;
    }
    const int H4 = H >> 2, rowsP = (rows + 31) & ~31, nct = H >> 5, nft = (F + 31) >> 5;
    RoBatch<float4, 4> b0, b1, by;
    const float* d1 = a.dy1 ? a.dy1 : a.dy0;
    ro_issue<GB_NT>(b0, rows, H4, [&](int j, int c) { return *reinterpret_cast<const float4*>(a.dy0 + (size_t)(g0 + j) * H + 4 * c); });
    ro_issue<GB_NT>(b1, rows, H4, [&](int j, int c) { return *reinterpret_cast<const float4*>(d1 + (size_t)(g0 + j) * H + 4 * c); });
    ro_issue<GB_NT>(by, rows, H4, [&](int j, int c) { return *reinterpret_cast<const float4*>(a.y + (size_t)(g0 + j) * H + 4 * c); });
    float xr[XU];                                        // x0[g0 .. g0 + rows) is contiguous: rows * F floats
#pragma unroll
    for (int u = 0; u < XU; ++u) xr[u] = a.x0[(size_t)g0 * F + min(t + u * GB_NT, rows * F - 1)];
    // W rows of this wave's first output tile (the epilogue's <W[f,:], .> sums): requested now, not behind the product
    const int lane = t & 63, li = lane & 31, lk = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);
    const int ct = w % nct, fstep = (GB_NT / 64) / nct;
    float wv[16];
    auto load_w = [&](int ft) {
#pragma unroll
        for (int r = 0; r < 16; ++r) wv[r] = a.W[(size_t)min(mma_row(r, lk, ft * 32), F - 1) * H + ct * 32 + li];
    };
    load_w(w / nct);
    const int uc = min(t, H - 1), fc = min(max(t - 128, 0), F - 1);
    BNRawS uraws;
    BNRaw raw0 = bn_raw_load(a.bn0, fc);
    StripeVal ud1s, ud2s;
    if (!NOBN) { uraws = bn_raws_load(a.ubn, uc); ud1s = stripe_load(a.udot_sum, uc, a.ubn.ss); ud2s = stripe_load(a.udot_prod, uc, a.ubn.ss); bn_raws_pin(uraws); stripe_pin(ud1s); stripe_pin(ud2s); }
    bn_raw_pin(raw0);
    if (!NOBN && t < H) bn_table_upper(a.ubn, uraws, ud1s, ud2s, t, um_s, ur_s, ug_s, u1_s, u2_s);
    if (t >= 128 && t - 128 < FP) {
        const int f = t - 128;
        float m1, r1;
        bn_raw_mean_rstd(a.bn0, raw0, m1, r1);
        m0_s[f] = m1; r0_s[f] = f < F ? r1 : 0.f;
        g0_s[f] = raw0.g;
        b0_s[f] = raw0.b;
    }
#pragma unroll
    for (int u = 0; u < XU; ++u) asm volatile("" : "+v"(xr[u]));
#pragma unroll
    for (int r = 0; r < 16; ++r) asm volatile("" : "+v"(wv[r]));
    // zero the padding of the x0_hat tile (columns F .. FP of every row, rows rows .. rowsP): they are reduced over / read
    for (int i = t; i < rowsP * LDXN; i += GB_NT) Xn[i] = 0.f;
    __syncthreads();
    {
        const bool two = a.dy1 != nullptr;
#pragma unroll
        for (int u = 0; u < 4; ++u) { ro_pin(b0.v[u]); ro_pin(b1.v[u]); ro_pin(by.v[u]); }
        // item (u, t): row (t + u * 512) / H4, float4 column t % H4 (512 % H4 == 0: a lane keeps its column group)
        const int col = t % H4, c = 4 * col, rstep = GB_NT / H4;
        int row = t / H4;
        float cs[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (row < rowsP) {
                float o[4] = {0.f, 0.f, 0.f, 0.f};
                if (row < rows) {
                    const float4 v0 = b0.v[u], v1 = b1.v[u], yv = by.v[u];
                    const float d[4] = {v0.x + (two ? v1.x : 0.f), v0.y + (two ? v1.y : 0.f), v0.z + (two ? v1.z : 0.f), v0.w + (two ? v1.w : 0.f)};
                    const float yy[4] = {yv.x, yv.y, yv.z, yv.w};
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        float g1 = d[k];
                        if (!NOBN) {
                            const float yn = (yy[k] - um_s[c + k]) * ur_s[c + k];
                            g1 = ug_s[c + k] * (d[k] - u1_s[c + k] - yn * u2_s[c + k]);
                        }
                        o[k] = yy[k] > 0.f ? g1 : 0.f;
                        cs[k] += o[k];
                    }
                }
                *reinterpret_cast<float4*>(Dz + row * LDZ + c) = make_float4(o[0], o[1], o[2], o[3]);
            }
            row += rstep;
        }
        // column sums of dZ: lanes of a wave with the same column group, then the eight waves through LDS
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (H4 <= 32) cs[k] += __shfl_xor(cs[k], 32, 64);
            if (H4 <= 16) cs[k] += __shfl_xor(cs[k], 16, 64);
        }
        const int lane = t & 63;
        if (lane < H4 && lane < 32) {
#pragma unroll
            for (int k = 0; k < 4; ++k) csp[t >> 6][lane][k] = cs[k];
        }
#pragma unroll
        for (int u = 0; u < XU; ++u) {
            const int i = t + u * GB_NT;
            if (i < rows * F) { const int f = i % F; Xn[(i / F) * LDXN + f] = (xr[u] - m0_s[f]) * r0_s[f]; }
        }
    }
    __syncthreads();
    if (t < H) {
        float tot = 0.f;
#pragma unroll
        for (int k = 0; k < GB_NT / 64; ++k) tot += csp[k][t >> 2][t & 3];
        cs_s[t] = tot;
    }
    __syncthreads();
    BLK_CLK(2);
    // P = x0_hat^T dZ on the matrix cores: wave w takes column tile w % nct and the feature tiles w / nct, + 8 / nct, ..
    auto ident = [](float v) { return v; };
    for (int ft = w / nct; ft < nft; ft += fstep) {
        gc_f32x16 acc[2];
#pragma unroll
        for (int i = 0; i < 16; ++i) { acc[0][i] = 0.f; acc[1][i] = 0.f; }
        mma_kmajor<1, 1, LDXN, LDZ>(Xn + ft * 32 + li, Dz + ct * 32 + li, rowsP, lk, ident, MmaIdent(), acc);
        const int h = ct * 32 + li;
        const float csh = cs_s[h];
        float wc[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) wc[r] = wv[r];
        float p1[16], p2[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int f = mma_row(r, lk, ft * 32);
            const float pv = acc[0][r];
            acc[1][r] = fmaf(g0_s[min(f, FP - 1)], pv, b0_s[min(f, FP - 1)] * csh);         // this unit's dW_feat entry
            p1[r] = f < F ? wc[r] * csh : 0.f;
            p2[r] = f < F ? wc[r] * pv : 0.f;
        }
        // sums over the tile's 32 columns through this wave's LDS scratch: lane (which = lane / 32, feature = lane % 32) adds
        // its row (160 ds_bpermute shuffles per tile, each behind its own lgkmcnt wait, were ~4 us per tile)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int fl = mma_row(r, lk);
            red_s[w][0][fl][li] = p1[r];
            red_s[w][1][fl][li] = p2[r];
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);              // lgkmcnt(0): the wave's own LDS writes (no other wave touches red_s[w])
        {
            const float* rr = &red_s[w][lk][li][0];
            float v[32], tot = 0.f;
#pragma unroll
            for (int q = 0; q < 32; ++q) v[q] = rr[q];
#pragma unroll
            for (int q = 0; q < 32; ++q) tot += v[q];
            const int f = ft * 32 + li;
            if (f < FP) s12[lk][ct][f] = tot;
        }
        // the guarded stores go LAST, with no load in flight (hipcc waits for vmcnt(0) at the head of every guarded block --
        // with the next tile's W rows already requested, each of the 16 stores waited for them and for its predecessor:
        // 4 us per tile), and the next tile's W rows are requested behind them, under the next product
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int f = mma_row(r, lk, ft * 32);
            if (f < F) slab[(size_t)f * H + h] = acc[1][r];
        }
        if (ft + fstep < nft) {
            load_w(ft + fstep);
#pragma unroll
            for (int r = 0; r < 16; ++r) asm volatile("" : "+v"(wv[r]));
        }
    }
    BLK_CLK(3);
    __syncthreads();
    if (t < F) {
        double s1 = 0.0, s2 = 0.0;
        for (int k = 0; k < nct; ++k) { s1 += (double)s12[0][k][t]; s2 += (double)s12[1][k][t]; }
        parts[t] = s1; parts[F + t] = s2;
    }
    BLK_CLK(1);
}

}  // namespace cal
