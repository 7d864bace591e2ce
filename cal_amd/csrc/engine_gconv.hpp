// Per-graph fused GCN convolution of the step engine, forward:
//     out = relu(A_hat (BN(rs * x) @ W) + b)          (gcn_conv.py:75-104 behind model.py:93-95, 112-113)
// as ONE kernel instead of GEMM -> aggregation.  A mini-batch's adjacency is block diagonal (one block
// per graph, ~57 nodes for SPMotif), so a workgroup that owns a whole graph and a 64-column slice of the
// output keeps z = BN(x) W in LDS, builds the graph's dense normalised adjacency block next to it and
// aggregates with a second matrix product: z never goes to HBM, there is no neighbour gather at all, and
// the per-graph column sums of the output (add-pool, model.py:115-116) and the next BatchNorm's batch
// statistics fall out of the epilogue.
//
//   grid (B graphs, H / 64 column slices, branches), 256 threads; requires per graph <= GC_T nodes and
//   <= GC_E stored edges (the host passes the batch's bounds, cal_engine_set_graph_bounds; otherwise the
//   unfused kernels run), H % 64 == 0 and K = hidden <= GC_K.
//
// Timeline of a workgroup: graph extents (gptr/eptr) -> every global load of the kernel issued at once
// (x rows, W slice, CSR rows and edges, BN statistics) -> edge coefficients dis_j * w_e -> operands
// staged in LDS (x transposed to k-major with BN / row scale applied) -> z = x' W on 32x32x2 f32 MFMAs ->
// z tile to LDS (over the W stage), adjacency block At[j][i] = dis_i * coef_ij (+ the self loop) built
// over the x stage by one lane per row -> out tile = A z on MFMAs -> bias, ReLU, store, column sums.
// (Aggregating from the CSR rows with LDS reads instead was a chain of dependent LDS accesses per edge
// with one wave per SIMD to hide it: 4.5-9 us per graph; the dense product is ~1 us.)
#pragma once
#include "engine_readout.hpp"     // RO_CLK profiling aid
#include "engine_mma.hpp"         // 32 x 32 tile products, row mapping, tile stores
#include "engine_gunit.hpp"       // unit extents, slot batch, operand tiles, BatchNorm tables, z tile / adjacency block, column sums
// CAL_GCF_ATT_UNIT (gconv_fwd_att.hip alone defines it): the kernel below is compiled as k_gconv_fwd_att -- one more argument, the
// attention forward's operands, and that forward as its tail (engine_attfwd_fold.hpp).  The additions are preprocessor blocks and
// not `if constexpr`: without the macro the compiler sees the tokens it has always seen, and engine.hip's device code stays what
// it was ("What decided the form").
#ifdef CAL_GCF_ATT_UNIT
#include "engine_attfwd_fold.hpp"
#define GCF_KERNEL k_gconv_fwd_att
#define GCF_ATT_PARAM , const AttFwdFoldArgs fa
#else
#define GCF_KERNEL k_gconv_fwd
#define GCF_ATT_PARAM
#endif

namespace cal {

constexpr int GC_T = 128;                 // nodes per graph (T = 128 instantiation; T = 64 for small graphs)
constexpr int GC_N = 64;                  // output columns per workgroup
constexpr int GC_K = 128;                 // reduction width (= hidden)
constexpr int GC_E = 2048;                // stored edges per graph (T = 128; half of it for T = 64)
constexpr int GC_LDB = GC_N + 4, GC_LDZ = GC_N + 1;
// T = 64 keeps a workgroup under 80 KB of LDS, so two of them share a CU: the two-branch launch (512
// workgroups) then needs one pass over the chip instead of two, and one workgroup's loads overlap the
// other's MFMAs.
constexpr int gc_edge_cap(int T) { return T == 64 ? 1024 : 2048; }

struct GconvBranch {
    const float* x;          // [N,K] layer input (raw)
    const float* W;          // [K,H]
    const float* bias;       // [H]
    const float* ew;         // per-edge weight in edge-id order, or null (all ones)
    const float* dis;        // [N] deg^-1/2 (of the weighted degrees when ew is set)
    const float* rs;         // per-row scale of x (node attention), or null
    int rs_stride;
    BNRef bn;                // BatchNorm applied to rs * x
    float* out;              // [N,H]
    float* z;                // [N,H] BN(rs x) W, kept for the backward of the weighted convs, or null
    float* pooled;           // [B,H] per-graph column sums of out (global_add_pool), or null
    Acc st_sum, st_sq;       // column statistics of out (one partial row per graph), or off
    // edge coefficients dis_j * w_e in CSR-slot order: the first kernel of a step that needs them writes them
    // (coef_out), every later one (deeper layers, the backward) reads them in its first round of loads (coef_in)
    // instead of chasing nbr -> dis / eid -> w in a second one
    const float* coef_in;
    float* coef_out;
    float* w_out;            // with coef_out: the raw edge weights w_e in CSR-slot order (read by the per-graph attention backward), or null
    // packed batch (TILED instantiation, cal_engine_set_tiles): the workgroup's unit is a tile of the consecutive graphs
    // [tile_gptr[b], tile_gptr[b + 1]) and `pooled` is per GRAPH: batch [N] names the graph of every row
    const int64_t* batch;
    const int64_t* tile_gptr;
};
constexpr int GC_TILE_GRAPHS = 8;         // graphs per tile at most (the POOL backward keeps one pooled-gradient row per graph in LDS)

struct GconvBranch2 { GconvBranch b[2]; };

constexpr int GC_LDX = GC_K + 4;            // x' rows as loaded: Xr[row * GC_LDX + k], stride 132 = 4 mod 32 (conflict-free 16 B reads)

template <bool RS, int T, int NT = 256, bool TILED = false>
__global__ void __launch_bounds__(NT, (T == 64 ? 2 : 1)) GCF_KERNEL(const CSR g, const int* __restrict__ gptr, const int* __restrict__ eptr,
                                                   const GconvBranch2 bb, int relu, float loop_w, int H,
                                                   int K, int* __restrict__ status GCF_ATT_PARAM) {
    // NT = 256: one 32 x 32 tile pair per wave.  NT = 512 (T = 64): eight waves -- the first product's reduction range is
    // split over two waves per tile (partial z tiles combined through LDS), twice the lanes stage the operands, and waves
    // 4-7 are free for the adjacency block while waves 0-3 finish the z tile
    constexpr int LDA = T + 1, ECAP = gc_edge_cap(T);
    constexpr int WU = 2048 / NT, CU = (ECAP + NT - 1) / NT, RPP = NT / 8, NRS = T / RPP > 0 ? T / RPP : 1;
    static_assert(NT == 256 || (NT == 512 && T == 64), "512 threads: 64-node variant only");
    __shared__ __attribute__((aligned(16))) float As[(GC_K * LDA > T * GC_LDX) ? GC_K * LDA : T * GC_LDX];   // x' rows [row][k] (stride GC_LDX); later the adjacency block [j][i] (stride LDA)
    __shared__ __attribute__((aligned(16))) float Bs[GC_K * GC_LDB];       // W slice [k][col]; later the z tile [row][col]
    __shared__ float sc_s[GC_K], sh_s[GC_K];
    __shared__ int ptr_s[T + 4];
    __shared__ float dis_s[T];
    __shared__ short en[ECAP];                          // (local node index < T: 2 bytes keep the T = 64 instantiation at two workgroups per CU)
    __shared__ float ec[ECAP];
    __shared__ signed char er[ECAP];
    __shared__ double red[4][2][32];
    __shared__ float pool_s[4][32];
    __shared__ unsigned char bg_s[TILED ? T : 4];        // TILED: graph (inside the tile) of every row
#ifdef CAL_GCF_ATT_UNIT
    static_assert(!RS && T == AFF_T && NT == 512 && !TILED && ECAP == AFF_E && GC_N == AFF_N, "the attention tail: the backbone's 64-node form");
    __shared__ float Ot_att[AFF_T * AFF_LDO];           // the output tile, parked for the tail (an array of its own: with it the kernel's LDS is over half a CU's, ONE workgroup per CU)
    __shared__ float4 wsl[AFF_ND * 16];                  // the six 64-float weight slices of the attention dots
    AttFwdFoldLoads fr;
#endif
    BLK_CLK(0);
#ifdef CAL_GCF_ATT_UNIT
    warm_kernargs<sizeof(CSR) + 2 * sizeof(void*) + sizeof(GconvBranch2) + 32 + sizeof(AttFwdFoldArgs)>();
#else
    warm_kernargs<sizeof(CSR) + 2 * sizeof(void*) + sizeof(GconvBranch2) + 32>();
#endif
    const GconvBranch& br = bb.b[blockIdx.z];           // indexed in the kernel-argument segment: one set of scalar loads (b0 / b1 as two parameters were loaded both and selected field by field)
    const int b = blockIdx.x, n0 = blockIdx.y * GC_N, t = threadIdx.x;
    // the W slice does not depend on the graph: requested before the graph's extents (a scalar round trip) are known
    float4 vb[WU];                                       // W[k][n0 + 4 j4 ..]: 16 lanes per k row
#pragma unroll
    for (int u = 0; u < WU; ++u) {
        const int idx = t + u * NT, k = min(idx >> 4, K - 1), j4 = idx & 15;
        vb[u] = *reinterpret_cast<const float4*>(br.W + (size_t)k * H + n0 + 4 * j4);
    }
    const GUnit un = gunit_load(gptr, eptr, b);
    const int g0 = un.g0, rows = un.rows, e0 = un.e0;
    const int tg0 = TILED ? (int)br.tile_gptr[b] : b, ng = TILED ? (int)br.tile_gptr[b + 1] - tg0 : 1;
    const bool want = br.st_sum.on();
    if (un.empty()) {                                    // empty graph: its partial rows still have to exist
        gunit_empty_update_running(br.bn, t, K);
        if (t < GC_N) {
            if (want) { br.st_sum.add(n0 + t, 0.0); br.st_sq.add(n0 + t, 0.0); }
            if (br.pooled) for (int q = 0; q < ng; ++q) br.pooled[(size_t)(tg0 + q) * H + n0 + t] = 0.f;
        }
        return;
    }
    if (TILED && (ng < 1 || ng > GC_TILE_GRAPHS)) { if (t == 0) atomicOr(status, 8); return; }
    if (un.exceeds<T, ECAP>()) { gunit_flag(un, status, t); return; }      // the host's bounds were wrong: flag it, write nothing
    RO_CLK(32);
    BLK_CLK(2);
    const int rowsP = (rows + 31) & ~31, R = rowsP >> 5, nkc = K >> 5, RB = (rowsP + RPP - 1) / RPP;
    // ---- every global load of the kernel, issued before the first wait -------------------------------------
    constexpr int UA = T * 32 / NT;                    // x float4s per lane: T rows x GC_K / 4 over NT lanes
    float4 va[UA];
    xrow_issue<UA, RPP>(va, br.x, un, K, nkc, RB, t);
    const int pv = g.ptr[g0 + min(t, rows)];
    const float dv = br.dis[g0 + min(t, rows - 1)];
    long long bgv = 0;
    if (TILED) bgv = br.batch[g0 + min(t, rows - 1)];
    float rsv[4] = {1.f, 1.f, 1.f, 1.f};                 // row scale of this lane's x row in each RPP-row block
    if (RS) {
#pragma unroll
        for (int q = 0; q < NRS; ++q) rsv[q] = br.rs[(size_t)(g0 + min(q * RPP + (t >> 3), rows - 1)) * br.rs_stride];
    }
    // CSR slots, BatchNorm constants, bias, coefficients of an earlier kernel of this step, if any
    GSlots<CU, true, true> slots;
    slots.template load_ids<NT>(g, un, t);
    const int lane = t & 63, li = lane & 31, lk = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);
    const int kh = w >> 2, ct = w & 1, r0 = (w & 3) >> 1;     // kh: half of the first product's reduction range (NT = 512)
    const float* biasp = br.bias ? br.bias : br.W;       // W: any valid [>= H] float array; the value is masked below
    float bias = biasp[n0 + ct * 32 + li];
    BNRawS braws = bn_raws_load(br.bn, min(t, K - 1));       // (striped reader: the producer may be a per-graph kernel)
    slots.template load_coef<NT>(g, un, t, br.coef_in, br.dis);
#ifdef CAL_GCF_ATT_UNIT
    aff_issue(fr, fa, un, n0, H, t);                     // the tail's weight slices and (slice 0) by-source CSR rows, in the same round
#endif
    // all of the above stay in flight together (engine_gunit.hpp)
#pragma unroll
    for (int u = 0; u < UA; ++u) ro_pin(va[u]);
#pragma unroll
    for (int u = 0; u < WU; ++u) ro_pin(vb[u]);
    bn_raws_pin(braws);
    slots.pin();
#ifdef CAL_GCF_ATT_UNIT
    aff_pin(fr);
#endif
    asm volatile("" : "+v"(bias));
    if (!br.bias) bias = 0.f;
    slots.repair_empty(un);
    bn_table_scale_shift(br.bn, braws, t, K, sc_s, sh_s);
    {   // second round: edge coefficients dis_j * w_e (needs the neighbour / edge ids), into the slot batch
        const bool hasw = br.ew != nullptr;
        if (br.coef_in) {
#pragma unroll
            for (int u = 0; u < CU; ++u) { slots.cv[u] = slots.cin[u]; slots.wv[u] = 1.f; }
        } else {
            const float* ewp = hasw ? br.ew : br.dis;
#pragma unroll
            for (int u = 0; u < CU; ++u) {
                const float c = br.dis[slots.nv[u]];
                const float wl = ewp[hasw ? slots.ev[u] : 0];
                slots.wv[u] = hasw ? wl : 1.f;
                slots.cv[u] = c * slots.wv[u];
            }
        }
    }
    RO_CLK(33);
    // ---- stage everything in LDS ---------------------------------------------------------------------------
    if (t <= rows) ptr_s[t] = pv - e0;
    if (t < rows) dis_s[t] = dv;
    if (TILED && t < rows) bg_s[t] = (unsigned char)min(max((int)(bgv - tg0), 0), ng - 1);
    slots.template stage<NT>(un, t, status, [&](int s, int u, int loc, bool inb) {
        en[s] = (short)(inb ? loc : 0); ec[s] = inb ? slots.cv[u] : 0.f;
        if (br.coef_out && blockIdx.y == 0) { br.coef_out[e0 + s] = slots.cv[u]; if (br.w_out) br.w_out[e0 + s] = slots.wv[u]; }
    });
    wslice_commit<NT, GC_LDB>(vb, Bs, K, t);
    RO_CLK(34);
    __syncthreads();                                     // BN tables
    gslots_dest_rows(er, ptr_s, t, rows);
    xrow_commit<UA, RPP, GC_LDX>(va, As, nkc, RB, t, [&](float4 v, int rr, int k) {
        if (RS) {
            const float s = (NRS == 1 || rr == 0) ? rsv[0] : ((NRS == 2 || rr == 1) ? rsv[1] : (rr == 2 ? rsv[2] : rsv[3]));
            v.x *= s; v.y *= s; v.z *= s; v.w *= s;
        }
        return bn_affine4(v, sc_s, sh_s, k);
    });
    __syncthreads();
    RO_CLK(35);
    BLK_CLK(3);
    // ---- z tile = BN(x) W on the matrix cores: wave w owns column tile w & 1 and row tiles w >> 1 (, + 2) ---
    gc_f32x16 acc0, acc1;
#pragma unroll
    for (int i = 0; i < 16; ++i) { acc0[i] = 0.f; acc1[i] = 0.f; }
    if (r0 < R) {
        if (NT == 512) {                                 // this wave's half of the reduction range
            const int kofs = kh * (K >> 1);
            mma_arow<false, GC_LDX, GC_LDB>(As + kofs, Bs + kofs * GC_LDB, K >> 1, r0, ct, li, lk, acc0, acc1);
        } else if (r0 + 2 < R) mma_arow<true, GC_LDX, GC_LDB>(As, Bs, K, r0, ct, li, lk, acc0, acc1);
        else mma_arow<false, GC_LDX, GC_LDB>(As, Bs, K, r0, ct, li, lk, acc0, acc1);
    }
    RO_CLK(36);
    __syncthreads();                                     // every wave is done reading both stages
    // ---- z tile -> LDS (over the W stage); zero the adjacency block (over the x stage) ------------------------
    constexpr int LDT = T + 4;                           // row stride of the two j-major tiles below (4 mod 32)
    float* Zt = Bs;                                      // Zt[col * LDT + j] = z[j][col]   (over the W stage)
    float* At = As;                                      // At[i * LDT + j] = weight of edge j -> i, times dis_i   (over the x stage)
    // the z rows of row tile rt (for the POOL backward's SDDMM): 16-byte stores, four columns per lane, like the output tile
    auto store_z = [&](const gc_f32x16& acc, int rt) {
        const int c0 = n0 + ct * 32;
        gc_store_tile<gc_site(WT_Z)>(acc, br.z + (size_t)(g0 + rt * 32) * H + c0, H, rows - rt * 32, li, lk, MmaIdent(), ((rows - rt * 32) * H - c0) * 4);
    };
    const bool own = NT == 256 || kh == 0;               // the wave that finishes its tile (NT = 512: adds its partner's partial below)
    if (r0 < R && (NT == 256 || kh == 1)) {
        z_park<LDT>(Zt, acc0, r0, ct, li, lk);
        if (NT == 256 && br.z) store_z(acc0, r0);
        if (NT == 256 && r0 + 2 < R) {
            z_park<LDT>(Zt, acc1, r0 + 2, ct, li, lk);
            if (br.z) store_z(acc1, r0 + 2);
        }
    }
    adj_zero<NT>(At, (rowsP * LDT) >> 2, t);             // rows i < rowsP of the block (contiguous)
    __syncthreads();
    if (NT == 512 && kh == 0 && r0 < R) {                // z tile = this wave's half + the partner's (already in Zt)
        z_combine<LDT, true>(Zt, acc0, r0, ct, li, lk);
        if (br.z) store_z(acc0, r0);
    }
    adj_scatter<NT, LDT>(At, er, en, un, t, [&](int i, int s) { return dis_s[i] * ec[s]; }, [&](int i) { return dis_s[i] * dis_s[i] * loop_w; });
    __syncthreads();
    RO_CLK(37);
    // ---- out tile = A z on the matrix cores (reduction over the graph's rowsP nodes) ---------------------------
#pragma unroll
    for (int i = 0; i < 16; ++i) { acc0[i] = 0.f; acc1[i] = 0.f; }
    if (own && r0 < R) {
        if (r0 + 2 < R) mma_rowk_tile<true, LDT>(At, Zt, rowsP, r0, ct, li, lk, acc0, acc1);
        else mma_rowk_tile<false, LDT>(At, Zt, rowsP, r0, ct, li, lk, acc0, acc1);
    }
    RO_CLK(38);
#ifdef CAL_GCF_ATT_UNIT
    BLK_CLK_X(4, 0, acc0[0]);
#endif
    // ---- epilogue: bias, ReLU, store, column sums of this graph ---------------------------------------------------
    float f1[4] = {0.f, 0.f, 0.f, 0.f}, f2[4] = {0.f, 0.f, 0.f, 0.f};
    float psum = 0.f;
    const int col = n0 + ct * 32 + li;
    asm volatile("" :: "v"(bias));                       // consume the bias load before the guarded stores (see gemm.hip)
    // TILED: the add-pool is per graph, several graphs share the tile: the output tile is parked in LDS (over the adjacency
    // block, once every wave has finished reading it) and summed per graph below, rows in order
    constexpr int LDO = GC_N + 1;
    float* Ot = As;
    if (TILED) __syncthreads();
    if (own && r0 < R) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = mma_row(r, lk, r0 * 32);
            float v = acc0[r] + bias;
            if (relu) v = fmaxf(v, 0.f);
            acc0[r] = v;                                 // (stored below, four columns per lane)
            const float vm = row < rows ? v : 0.f;
            if (TILED) Ot[row * LDO + ct * 32 + li] = vm;
#ifdef CAL_GCF_ATT_UNIT
            Ot_att[row * AFF_LDO + ct * 32 + li] = vm;   // (T = 64: two row tiles at most, this loop holds every row)
#endif
            f1[r & 3] += vm; f2[r & 3] = fmaf(vm, vm, f2[r & 3]);
        }
        if (r0 + 2 < R) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = mma_row(r, lk, (r0 + 2) * 32);
                float v = acc1[r] + bias;
                if (relu) v = fmaxf(v, 0.f);
                acc1[r] = v;
                const float vm = row < rows ? v : 0.f;
                if (TILED) Ot[row * LDO + ct * 32 + li] = vm;
                f1[r & 3] += vm; f2[r & 3] = fmaf(vm, vm, f2[r & 3]);
            }
        }
        // (the extent: from the tile's first word to the end of this graph's rows)
        const int c0 = n0 + ct * 32;
        gc_store_tile<gc_site(WT_OUT)>(acc0, br.out + (size_t)(g0 + r0 * 32) * H + c0, H, rows - r0 * 32, li, lk, MmaIdent(), ((rows - r0 * 32) * H - c0) * 4);
        if (r0 + 2 < R) gc_store_tile<gc_site(WT_OUT)>(acc1, br.out + (size_t)(g0 + (r0 + 2) * 32) * H + c0, H, rows - (r0 + 2) * 32, li, lk, MmaIdent(), ((rows - (r0 + 2) * 32) * H - c0) * 4);
    }
    psum = (f1[0] + f1[1]) + (f1[2] + f1[3]);
    double s1, s2;
    colsum_fold(f1, f2, s1, s2);
    psum += __shfl_xor(psum, 32, 64);
    // (colsum_commit written out: the add-pool's fp32 sums share its store, barrier and lanes)
    if (own && lk == 0) { red[w & 3][0][li] = s1; red[w & 3][1][li] = s2; pool_s[w & 3][li] = psum; }
#ifdef CAL_GCF_ATT_UNIT
    if (t < AFF_ND * 16) wsl[t] = fr.wq;                 // (published, with the parked tile, by the barrier below)
#endif
    __syncthreads();
    if (w < 2 && lk == 0) {
        if (want) {
            br.st_sum.add(col, red[w][0][li] + red[w + 2][0][li]);
            br.st_sq.add(col, red[w][1][li] + red[w + 2][1][li]);
        }
        if (!TILED && br.pooled) br.pooled[(size_t)b * H + col] = pool_s[w][li] + pool_s[w + 2][li];
    }
    if (TILED && br.pooled && t < GC_N) {
        // one lane per column walks the tile's rows in order and closes a pooled row whenever the graph changes; graphs
        // without nodes keep the zero written first (same lane, same address: program order)
        float* pp = br.pooled + (size_t)tg0 * H + n0 + t;
        for (int q = 0; q < ng; ++q) pp[(size_t)q * H] = 0.f;
        float sum = 0.f;
        int cur = bg_s[0];
        for (int r = 0; r < rows; ++r) {
            const int gq = bg_s[r];
            if (gq != cur) { pp[(size_t)cur * H] = sum; sum = 0.f; cur = gq; }
            sum += Ot[r * LDO + t];
        }
        pp[(size_t)cur * H] = sum;
    }
#ifdef CAL_GCF_ATT_UNIT
    // every wave is past the second product and the barrier above: the z tile's stage is free for the tail's fp64 partials
    aff_tail(fa, fr, un, Ot_att, wsl, reinterpret_cast<double*>(Bs), n0, loop_w, status);
#endif
    RO_CLK(39);
    BLK_CLK(1);
}

}  // namespace cal
