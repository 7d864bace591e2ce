// The body of the per-graph GCNConv backward kernels (engine_gconv_bwd.hpp has the description), included as TEXT by its two
// entries: k_gconv_bwd<RS, MODE, TILED, LEAN> (engine_gconv_bwd.hpp; MODE 0-2; instantiated in engine.hip with the products in
// order 0 and in gconv_bwd_seq.hip in the build's order) and k_gconv_bwd_att (gconv_bwd_att.hip; MODE 3 = ATT,
// RS / TILED / LEAN false).  Text and not a __device__ function: as a function the instantiations of k_gconv_bwd came out a few
// scalar instructions different from what they were, and every kernel behind them in the code object moved.
// In scope at the point of inclusion: RS, MODE, TILED, LEAN (compile-time), the kernel arguments g, gptr, eptr, bb, loop_w, N, H, K,
// status, and ga (AttBwdGraphArgs in the ATT mode, an empty struct of a dependent type otherwise).  No include guard: it is included once per entry.
    constexpr int LDX = LEAN ? GC_K : GB_LDX;
    __shared__ __attribute__((aligned(16))) float Ab[GB_T * GB_LDJ];       // adjacency block Ab[j][i]: dz_i += Ab[j][i] dOut_j
    __shared__ __attribute__((aligned(16))) float Ds[GB_T * GB_LDD];       // dOut slice [j][n]; later dz [i][n]
    __shared__ __attribute__((aligned(16))) float Ws[LEAN ? 4 : GC_K * GB_LDD];   // POOL: W[:, ns] as loaded: Ws[k_in][n] (row-major in n, 16 B operand reads)
    __shared__ __attribute__((aligned(16))) float Xs[GB_T * LDX];          // x_hat rows [i][k_in] (normalised, no affine)
    __shared__ float mean_s[GC_K], rstd_s[GC_K], gam_s[GC_K], bet_s[GC_K];
    __shared__ int ptr_s[GB_T + 4];
    __shared__ float dis_s[GB_T], rs_s[GB_T];
    __shared__ unsigned char en[GB_E];                   // (local node index < 64)
    __shared__ float ec[GB_E];
    __shared__ float um_s[MODE == 1 ? GC_N : 1], ur_s[MODE == 1 ? GC_N : 1], ug_s[MODE == 1 ? GC_N : 1], u1_s[MODE == 1 ? GC_N : 1], u2_s[MODE == 1 ? GC_N : 1];     // UP: upper BatchNorm, this slice's columns
    __shared__ float bs_s[GB_NT / 64][16][4];
    __shared__ __attribute__((aligned(16))) float Zr_own[(MODE == 2 && !LEAN) ? GB_T * GB_LDD : 4];       // POOL: z slice rows [j][n]
    // LEAN POOL: the z rows live in the x_hat stage until P1 and the SDDMM are done with them; x_hat is committed only then
    // (its registers wait through P1) -- the two are never needed at the same time
    float* const Zr = (MODE == 2 && LEAN) ? Xs : Zr_own;
    __shared__ float gv_s[TILED ? GC_TILE_GRAPHS * GC_N : GC_N];   // POOL: gradient of this graph's pooled row (TILED: of every graph of the tile), slice columns
    __shared__ unsigned char bg_s[TILED ? GB_T : 4];     // TILED: graph (inside the tile) of every row
    __shared__ int ee[(MODE == 2 && !LEAN) ? GB_E : 1];  // POOL: edge id of CSR slot s (LEAN: gn goes out in slot order only, the caller vouches for gn_slot)
    __shared__ unsigned char er[GB_E];                   // destination row of CSR slot s (< 64)
    constexpr bool UP = MODE == 1, POOL = MODE == 2, ATT = MODE == 3;
    static_assert(!TILED || MODE == 2, "only the POOL variant looks at the graphs inside a tile");
    static_assert(!ATT || (!LEAN && !RS), "the ATT mode keeps the staged W slice (one workgroup per CU) and has no row scales");
    // ATT: the attention backward's LDS (engine_attphases.hpp) next to the stages; its dense blocks alias the W / x_hat stages
    __shared__ double red[ATT ? 8 : 1][4][ATT ? GC_N : 1];               // column sums of this slice: [wave][quantity][column]
    __shared__ double sc_lds[2][ATT ? 8 : 1];
    __shared__ float bnk_s[ATT ? 8 : 1][ATT ? GC_K : 1];
    __shared__ float dis_c_s[ATT ? GB_T : 1], dis_o_s[ATT ? GB_T : 1], dd_c_s[ATT ? GB_T : 1], dd_o_s[ATT ? GB_T : 1], spv_s[ATT ? GB_T : 1], sqv_s[ATT ? GB_T : 1],
                     gs_c_s[ATT ? GB_T : 1], gs_o_s[ATT ? GB_T : 1];
    static_assert(LEAN || (2 * GB_T * GB_LDJ <= GC_K * GB_LDD && GB_T * GB_LDJ <= GB_T * LDX), "Tc, To fit the W stage and Dm the x_hat stage");
    BLK_CLK(0);
    if constexpr (ATT) warm_kernargs<sizeof(CSR) + 2 * sizeof(void*) + sizeof(GconvBwdBranch2) + 32 + sizeof(ga)>();
    else warm_kernargs<sizeof(CSR) + 2 * sizeof(void*) + sizeof(GconvBwdBranch2) + 32>();
    const GconvBwdBranch& br = bb.b[blockIdx.z];         // indexed in the kernel-argument segment (see k_gconv_fwd)
    const int b = blockIdx.x, sl = blockIdx.y, ns0 = sl * GC_N, t = threadIdx.x;
    const GUnit un = gunit_load(gptr, eptr, b);
    const int g0 = un.g0, rows = un.rows, e0 = un.e0, ne = un.ne;
    const int pb = (MODE == 2 && !TILED && br.iperm) ? br.iperm[b] : b;         // row of the second pooled-gradient partial (scalar load, with the extents)
    const int tg0 = TILED ? (int)br.tile_gptr[b] : b, ng = TILED ? (int)br.tile_gptr[b + 1] - tg0 : 1;
    const int lane = t & 63, li = lane & 31, lk = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);
    double* parts = br.dot_parts + ((size_t)sl * gridDim.x + b) * (2 * K);
    float* slab = br.slab + (size_t)b * K * H;
    if (rows <= 0 || rows > GB_T || ne > GB_E || ne < 0 || (TILED && (ng < 1 || ng > GC_TILE_GRAPHS))) {
        // empty graph (or a violated bound, flagged): its partial row and its slab slice must still exist
        if (rows > 0 && t == 0) atomicOr(status, 8);
        if (!br.dacc_sum) for (int i = t; i < 2 * K; i += GB_NT) parts[i] = 0.0;
        if ((UP || POOL) && t < GC_N) br.bias_parts[(size_t)b * H + ns0 + t] = 0.0;
        if constexpr (ATT) {                             // and this slice's columns of the attention backward's partial rows
            const AttBwdArgs& a = ga.a;
            if (t < GC_N) {
                if (a.dbias.on()) a.dbias.add(ns0 + t, 0.0);
                a.dWn.add(ns0 + t, 0.0); a.dWe.add(ns0 + t, 0.0); a.dWe.add(H + ns0 + t, 0.0);
            }
            if (t == 0 && sl == 0) { a.dWn.add(H, 0.0); a.dWe.add(2 * H, 0.0); }
        }
        for (int i = t; i < K * GC_N; i += GB_NT) slab[(size_t)(i / GC_N) * H + ns0 + i % GC_N] = 0.f;
        return;
    }
    const int rowsP = (rows + 31) & ~31, R = rowsP >> 5, K4 = K >> 2;
    // ---- every global load of the kernel, issued before the first wait ------------------------------------------
    RoBatch<float4, 2> bd, bd1, by;                      // dOut[g0 + j][ns0 + 4 n4 ..]: rows x 16 float4 (UP: dy0, dy1, y)
    RoBatch<float4, 4> bx, bw;                           // x[g0 + i][4 k4 ..]: rows x K/4;  W[k_in][ns0 + 4 n4 ..]: K x 16
    RoBatch<float4, 2> bz;                               // POOL: z[g0 + j][ns0 + 4 n4 ..]
    float gv = 0.f, gv1 = 0.f;
    int pbq = 0;
    long long bgv = 0;
    if (POOL) {
        ro_issue<GB_NT>(by, rows, 16, [&](int j, int n4) { return *reinterpret_cast<const float4*>(br.y + (size_t)(g0 + j) * H + ns0 + 4 * n4); });
        ro_issue<GB_NT>(bz, rows, 16, [&](int j, int n4) { return *reinterpret_cast<const float4*>(br.z + (size_t)(g0 + j) * H + ns0 + 4 * n4); });
        if (!TILED) {   // gradient of this graph's pooled row, slice columns: both partials unconditionally (gp1 absent: gp0 twice, weight 0)
            const float* gp1 = br.gp1 ? br.gp1 : br.gp0;
            gv = br.gp0[(size_t)b * H + ns0 + (t & (GC_N - 1))];
            gv1 = gp1[(size_t)pb * H + ns0 + (t & (GC_N - 1))];
        } else {        // lane (q = t / 64, column t % 64): graph tg0 + q of the tile; the permuted row's index is a load of its own
            const int gq = tg0 + min(t >> 6, ng - 1);
            gv = br.gp0[(size_t)gq * H + ns0 + (t & (GC_N - 1))];
            pbq = br.iperm ? br.iperm[gq] : gq;
            bgv = br.batch[g0 + min(t, rows - 1)];
        }
    } else if (!ATT) {
        const float* d0 = UP ? br.dy0 : br.dout;
        ro_issue<GB_NT>(bd, rows, 16, [&](int j, int n4) { return *reinterpret_cast<const float4*>(d0 + (size_t)(g0 + j) * H + ns0 + 4 * n4); });
        if (UP) {
            const float* d1 = br.dy1 ? br.dy1 : br.dy0;
            ro_issue<GB_NT>(bd1, rows, 16, [&](int j, int n4) { return *reinterpret_cast<const float4*>(d1 + (size_t)(g0 + j) * H + ns0 + 4 * n4); });
            ro_issue<GB_NT>(by, rows, 16, [&](int j, int n4) { return *reinterpret_cast<const float4*>(br.y + (size_t)(g0 + j) * H + ns0 + 4 * n4); });
        }
    }
    ro_issue<GB_NT>(bx, rows, K4, [&](int i, int k4) { return *reinterpret_cast<const float4*>(br.x + (size_t)(g0 + i) * K + 4 * k4); });
    auto issue_w = [&]() { ro_issue<GB_NT>(bw, K, 16, [&](int k, int n4) { return *reinterpret_cast<const float4*>(br.W + (size_t)k * H + ns0 + 4 * n4); }); };
    if (!LEAN && !ATT) issue_w();                        // (ATT: behind the BatchNorm table, see below)
    const int pv = g.ptr[g0 + min(t, rows)];
    const int pn = g.ptr[g0 + min(t + 1, rows)];
    const float dv = br.dis[g0 + min(t, rows - 1)];
    const float rv = RS ? br.rs[(size_t)(g0 + min(t, rows - 1)) * br.rs_stride] : 1.f;
    // CSR slots, coefficients and the BatchNorm constants (engine_gunit.hpp)
    GSlots<2, true, true> slots;
    slots.template load<GB_NT>(g, un, t, br.coef_in, br.dis);
    // (striped readers, engine.hpp: the producers may be per-graph kernels.  Lanes 0 .. K-1 need this layer's BatchNorm, lanes
    //  256 .. 319 the upper one's constants of this slice's 64 columns: ONE register set, the pointers chosen per lane)
    const bool ulane = UP && t >= 256;
    BNRawS braws = UP ? bn_raws_load2(br.bn, min(t, K - 1), br.ubn, ns0 + (t & (GC_N - 1)), ulane) : bn_raws_load(br.bn, min(t, K - 1));
    StripeVal ud1s, ud2s;
    if (UP) {
        const int c = ns0 + (t & (GC_N - 1));
        ud1s = stripe_load(br.udot_sum, c, br.ubn.ss); ud2s = stripe_load(br.udot_prod, c, br.ubn.ss);
    }
    // ATT: everything k_att_bwd_graph loads, in the same round (nbr: the slot batch above).  Lane layout of its row phase: G = H / 4
    // lanes per row (column group c), RPB = 512 / G rows per pass, the unit's 64 rows = items u = 0 .. 64 / RPB - 1 of every lane.
    // Items 0, 1 go out here; items 2, 3 (H = 128) behind the BatchNorm table below.
    const int agl = ATT ? t & (H / 4 - 1) : 0, agrp = ATT ? t / (H / 4) : 0, arpb = ATT ? GB_NT / (H / 4) : 0, ac = 4 * agl;
    const bool aown = (ac >> 6) == sl;                   // this lane's four columns are in the slice
    StripeVal sv[ATT ? 4 : 1];
    float agc[4], ago[4], aw0[4], aw1[4], aw2[4], aw3[4], aw4[4], aw5[4];
    float dcv = 0.f, dov = 0.f, gsc = 0.f, gso = 0.f, gsc2 = 0.f, gso2 = 0.f, af2 = 0.f;
    float dgc[2], dgo[2], dwc[2], dwo[2], dgc2[2], dgo2[2];
    float ra0[4], ra1[4];
    Vec<4> rx[4], rhc[4], rho[4], rhc2[4], rho2[4];
    auto att_load_rows = [&](auto u0tag) {
        if constexpr (ATT) {
            constexpr int u0 = decltype(u0tag)::value;
            const AttBwdArgs& a = ga.a;
            const float* dxhc2 = a.dxhc2 ? a.dxhc2 : a.dxhc;
            const float* dxho2 = a.dxho2 ? a.dxho2 : a.dxho;
#pragma unroll
            for (int u = u0; u < u0 + 2; ++u) {
                const size_t v = (size_t)(g0 + min(agrp + u * arpb, rows - 1));
                ra0[u] = a.anode[2 * v]; ra1[u] = a.anode[2 * v + 1];
                rx[u] = Vec<4>::ld(a.x + v * H + ac); rhc[u] = Vec<4>::ld(a.dxhc + v * H + ac); rho[u] = Vec<4>::ld(a.dxho + v * H + ac);
                rhc2[u] = Vec<4>::ld(dxhc2 + v * H + ac); rho2[u] = Vec<4>::ld(dxho2 + v * H + ac);
            }
        }
    };
    if constexpr (ATT) {
        const AttBwdArgs& a = ga.a;
        // the eight striped BatchNorm sums per column: lanes 0 .. H-1 take the statistics of bnc / bno, lanes 256 .. 256+H-1 their
        // backward sums -- ONE register set of 4 x NSTRIPE doubles, the pointers chosen per lane (as bn_raws_load2 does)
        const bool hi = t >= 256;
        const int oc = min(t & 255, H - 1);
        sv[0] = stripe_load(hi ? a.dsc : a.bnc.sum, oc, hi ? a.dss : a.bnc.ss); sv[1] = stripe_load(hi ? a.dpc : a.bnc.sq, oc, hi ? a.dss : a.bnc.ss);
        sv[2] = stripe_load(hi ? a.dso : a.bno.sum, oc, hi ? a.dss : a.bno.ss); sv[3] = stripe_load(hi ? a.dpo : a.bno.sq, oc, hi ? a.dss : a.bno.ss);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            agc[j] = a.bnc.gamma[ac + j]; ago[j] = a.bno.gamma[ac + j];
            aw0[j] = a.Wn[ac + j]; aw1[j] = a.Wn[H + ac + j];
            aw2[j] = a.We[ac + j]; aw3[j] = a.We[2 * H + ac + j]; aw4[j] = a.We[H + ac + j]; aw5[j] = a.We[3 * H + ac + j];
        }
        const float* gself2 = ga.gself2 ? ga.gself2 : ga.gself;
        const float* gn2 = ga.gn2 ? ga.gn2 : ga.gn;
        af2 = ga.gn2 ? 1.f : 0.f;                        // weight of the slice-1 partials
        const int vn = g0 + min(t, rows - 1);
        const int64_t E = ga.E;
        dcv = ga.dis[vn]; dov = ga.dis[(size_t)ga.N + vn];
        gsc = ga.gself[vn]; gso = ga.gself[(size_t)ga.N + vn]; gsc2 = gself2[vn]; gso2 = gself2[(size_t)ga.N + vn];
        att_load_rows(std::integral_constant<int, 0>());
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int64_t s = min(slots.template slot<GB_NT>(un, t, u), max(g.nnz - 1, 0));
            dgc[u] = ga.gn[s]; dgo[u] = ga.gn[E + s]; dgc2[u] = gn2[s]; dgo2[u] = gn2[E + s];
            dwc[u] = ga.att[s]; dwo[u] = ga.att[E + s];
        }
    }
    bn_raws_pin(braws);
    if (UP) { stripe_pin(ud1s); stripe_pin(ud2s); }
    slots.pin();
    if constexpr (ATT) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            asm volatile("" : "+v"(agc[j]), "+v"(ago[j]), "+v"(aw0[j]), "+v"(aw1[j]), "+v"(aw2[j]), "+v"(aw3[j]), "+v"(aw4[j]), "+v"(aw5[j]));
#pragma unroll
        for (int q = 0; q < 4; ++q) stripe_pin(sv[q]);
        asm volatile("" : "+v"(dcv), "+v"(dov), "+v"(gsc), "+v"(gso), "+v"(gsc2), "+v"(gso2));
#pragma unroll
        for (int u = 0; u < 2; ++u)
            asm volatile("" : "+v"(dgc[u]), "+v"(dgo[u]), "+v"(dgc2[u]), "+v"(dgo2[u]), "+v"(dwc[u]), "+v"(dwo[u]));
#pragma unroll
        for (int u = 0; u < 2; ++u) { dgc[u] = fmaf(af2, dgc2[u], dgc[u]); dgo[u] = fmaf(af2, dgo2[u], dgo[u]); }
        gsc = fmaf(af2, gsc2, gsc); gso = fmaf(af2, gso2, gso);
        if (t < H) att_bn_stats(ga.a, sv[0], sv[1], sv[2], sv[3], bnk_s, t);
        else if (t >= 256 && t < 256 + H) att_bn_dsums(ga.a, sv[0], sv[1], sv[2], sv[3], bnk_s, t - 256);
        // (every lane's columns exist -- H = 4 G: the row phase's constants wn, wp, wq are differences, taken here: 12 registers fewer
        //  through the edge phase, and w - 0 below gives the same bits)
#pragma unroll
        for (int j = 0; j < 4; ++j) { aw0[j] -= aw1[j]; aw1[j] = 0.f; aw2[j] -= aw3[j]; aw3[j] = 0.f; aw4[j] -= aw5[j]; aw5[j] = 0.f; }
        // second batch, in the registers the striped doubles leave: the W slice and the row items 2, 3 (H = 128).  Both are
        // wanted only behind the edge phase, which they stay in flight through -- with them in the first batch the kernel spilled.
        issue_w();
        if (H > GC_N) att_load_rows(std::integral_constant<int, 2>());                 // stay in flight through the edge phase
    }
    if (POOL && !TILED) { asm volatile("" : "+v"(gv), "+v"(gv1)); gv += br.gp1 ? gv1 : 0.f; }
    if (TILED) {                                         // second round: the permuted graph's pooled-gradient row
        asm volatile("" : "+v"(gv), "+v"(pbq), "+v"(bgv));
        const float* gp1 = br.gp1 ? br.gp1 : br.gp0;
        gv1 = gp1[(size_t)pbq * H + ns0 + (t & (GC_N - 1))];
    }
    slots.repair_empty(un);
    if (UP && t >= 256 && t < 256 + GC_N) bn_table_upper(br.ubn, braws, ud1s, ud2s, t - 256, um_s, ur_s, ug_s, u1_s, u2_s);
    bn_table_hat(br.bn, braws, t, K, mean_s, rstd_s, gam_s, bet_s);
    adj_zero<GB_NT>(Ab, (rowsP * GB_LDJ + 3) / 4, t);
    // ATT: the edge phase's dense blocks [source][destination] -- Tc, To over the W stage, Dm over the x_hat stage -- are dead
    // before those are committed
    [[maybe_unused]] float* const Tc = Ws; [[maybe_unused]] float* const To = Ws + GB_T * GB_LDJ; [[maybe_unused]] float* const Dm = Xs;
    if constexpr (ATT) {
        adj_zero<GB_NT>(Ws, 2 * GB_T * GB_LDJ / 4, t);
        adj_zero<GB_NT>(Xs, GB_T * GB_LDJ / 4, t);
    }
    {   // second round, as in k_gconv_fwd (wv is not used here)
        const bool hasw = br.ew != nullptr;
        if (br.coef_in) {
#pragma unroll
            for (int u = 0; u < 2; ++u) { slots.cv[u] = slots.cin[u]; slots.wv[u] = 1.f; }
        } else {
            const float* ewp = hasw ? br.ew : br.dis;
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const float c = br.dis[slots.nv[u]];
                const float wl = ewp[hasw ? slots.ev[u] : 0];
                slots.wv[u] = hasw ? wl : 1.f;
                slots.cv[u] = c * slots.wv[u];
            }
        }
    }
    // ---- stage everything in LDS -----------------------------------------------------------------------------------
    if (t <= rows) ptr_s[t] = pv - e0;
    if (t < rows) {
        dis_s[t] = dv; rs_s[t] = rv;
        gslots_dest_rows(er, t, pv - e0, pn - e0);
    }
    if constexpr (ATT) {
        if (t < GB_T) {                                  // (rows past the graph: zero, the block sums run over all 64)
            dis_c_s[t] = t < rows ? dcv : 0.f; dis_o_s[t] = t < rows ? dov : 0.f;
        }
        if (t < rows) { gs_c_s[t] = gsc; gs_o_s[t] = gso; }
    }
    slots.template stage<GB_NT>(un, t, status, [&](int s, int u, int loc, bool inb) {
        en[s] = (unsigned char)(inb ? loc : 0); ec[s] = inb ? slots.cv[u] : 0.f;
        if (POOL && !LEAN) ee[s] = slots.ev[u];
    });
    if (POOL && !TILED && t < GC_N) gv_s[t] = gv;
    if (TILED) {
        if (t < ng * GC_N) gv_s[t] = gv + (br.gp1 ? gv1 : 0.f);
        if (t < rows) bg_s[t] = (unsigned char)min(max((int)(bgv - tg0), 0), ng - 1);
    }
    if (MODE == 0) ro_commit<GB_NT>(bd, rows, 16, [&](int j, int n4, const float4 v) { *reinterpret_cast<float4*>(Ds + j * GB_LDD + 4 * n4) = v; });
    if (!LEAN && !ATT) ro_commit<GB_NT>(bw, K, 16, [&](int k, int n4, const float4 v) { *reinterpret_cast<float4*>(Ws + k * GB_LDD + 4 * n4) = v; });
    __syncthreads();                                     // per-column BN constants, row scales, zeroed Ab, CSR
    auto commit_x = [&]() {
        ro_commit<GB_NT>(bx, rows, K4, [&](int i, int k4, float4 v) {
            const float s = RS ? rs_s[i] : 1.f;
            const int k = 4 * k4;
            v.x = (v.x * s - mean_s[k]) * rstd_s[k]; v.y = (v.y * s - mean_s[k + 1]) * rstd_s[k + 1];
            v.z = (v.z * s - mean_s[k + 2]) * rstd_s[k + 2]; v.w = (v.w * s - mean_s[k + 3]) * rstd_s[k + 3];
            *reinterpret_cast<float4*>(Xs + i * LDX + k) = v;
        });
    };
    if (!(POOL && LEAN) && !ATT) commit_x();
    double acs[ATT ? 4 : 1][4];                          // ATT: this lane's column sums behind d bias_L, d Wn, d We (source / destination half)
    double asdl = 0.0, assp = 0.0;
    if constexpr (ATT) {
        const AttBwdArgs& a = ga.a;
        adj_scatter<GB_NT, GB_LDJ>(Ab, er, en, un, t, [&](int j, int s) { return dis_s[j] * ec[s]; }, [&](int j) { return dis_s[j] * dis_s[j] * loop_w; });
        att_edge_phase<GB_LDJ>(Tc, To, Dm, en, er, dis_c_s, dis_o_s, gs_c_s, gs_o_s, dd_c_s, dd_o_s, spv_s, sqv_s, dgc, dgo, dwc, dwo,
                               t, rows, ne, a.fedge, ga.loop_w);
        BLK_CLK(2);
        // the blocks are done with (the edge phase ends on a barrier): the W slice and the x_hat rows take their stages
        ro_commit<GB_NT>(bw, K, 16, [&](int k, int n4, const float4 v) { *reinterpret_cast<float4*>(Ws + k * GB_LDD + 4 * n4) = v; });
        commit_x();
        // row phase over all rows and all H columns; dOut = dZ of this slice's columns goes to Ds
        float mc[4], rc[4], m1c[4], m2c[4], mo[4], ro[4], m1o[4], m2o[4], wn[4], wp[4], wq[4];
        att_row_consts<4>(bnk_s, ac, ac, true, H, mc, rc, agc, m1c, m2c, mo, ro, ago, m1o, m2o, aw0, aw1, aw2, aw3, aw4, aw5, wn, wp, wq);
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int j = 0; j < 4; ++j) acs[q][j] = 0.0;
        auto row_pass = [&](auto gtag, auto u0tag) {
            constexpr int G = decltype(gtag)::value, u0 = decltype(u0tag)::value;
#pragma unroll
            for (int u = u0; u < u0 + 2; ++u) {
                rx[u].pin(); rhc[u].pin(); rho[u].pin(); rhc2[u].pin(); rho2[u].pin();
                rhc[u].fma(af2, rhc2[u]); rho[u].fma(af2, rho2[u]);
                asm volatile("" : "+v"(ra0[u]), "+v"(ra1[u]));
            }
#pragma unroll
            for (int u = u0; u < u0 + 2; ++u) {
                att_row_item<4, G>(a, 1, agrp + u * (GB_NT / G), rows, agl, true, aown, rx[u], rhc[u], rho[u], ra0[u], ra1[u], mc, rc, agc, m1c, m2c,
                                   mo, ro, ago, m1o, m2o, wn, wp, wq, spv_s, sqv_s, acs, asdl, assp, [&](int i, const float (&o)[4]) {
                    *reinterpret_cast<float4*>(Ds + i * GB_LDD + ac - ns0) = make_float4(o[0], o[1], o[2], o[3]);
                });
            }
        };
        if (H > GC_N) {
            row_pass(std::integral_constant<int, 32>(), std::integral_constant<int, 0>()); row_pass(std::integral_constant<int, 32>(), std::integral_constant<int, 2>());
            att_colsum_waves<4, 32>(acs, asdl, assp, red, sc_lds, t, agl, ac - ns0, aown);
        } else {
            row_pass(std::integral_constant<int, 16>(), std::integral_constant<int, 0>());
            att_colsum_waves<4, 16>(acs, asdl, assp, red, sc_lds, t, agl, ac - ns0, aown);
        }
    }
    if (POOL) {
        float cs[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int u = 0; u < 2; ++u) { ro_pin(by.v[u]); ro_pin(bz.v[u]); }
        const int c = 4 * (t & 15);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int j = (t >> 4) + u * (GB_NT / 16);
            if (j < rows) {
                const float4 yv = by.v[u];
                const float* gvr = gv_s + (TILED ? bg_s[j] * GC_N : 0);
                const float4 o = make_float4(yv.x > 0.f ? gvr[c] : 0.f, yv.y > 0.f ? gvr[c + 1] : 0.f,
                                             yv.z > 0.f ? gvr[c + 2] : 0.f, yv.w > 0.f ? gvr[c + 3] : 0.f);
                cs[0] += o.x; cs[1] += o.y; cs[2] += o.z; cs[3] += o.w;
                *reinterpret_cast<float4*>(Ds + j * GB_LDD + c) = o;
                *reinterpret_cast<float4*>(Zr + j * GB_LDD + c) = bz.v[u];
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            cs[q] += __shfl_xor(cs[q], 16, 64);
            cs[q] += __shfl_xor(cs[q], 32, 64);
        }
        if (lane < 16) {
#pragma unroll
            for (int q = 0; q < 4; ++q) bs_s[t >> 6][lane][q] = cs[q];
        }
    }
    if (UP) {
        // dOut slice from the upper layer's partials: lane t always holds column group t % 16 (512 % 16 == 0), so
        // its column sums stay in registers until the cross-lane reduction below
        float cs[4] = {0.f, 0.f, 0.f, 0.f};
        const bool two = br.dy1 != nullptr;
#pragma unroll
        for (int u = 0; u < 2; ++u) { ro_pin(bd.v[u]); ro_pin(bd1.v[u]); ro_pin(by.v[u]); }
        const int c = 4 * (t & 15);
#pragma unroll
        for (int u = 0; u < 2; ++u) {                   // item (u, t) = row t / 16 + 32 u, column group t % 16
            const int j = (t >> 4) + u * (GB_NT / 16);
            if (j < rows) {
                const float4 v0 = bd.v[u], v1 = bd1.v[u], yv = by.v[u];
                const float d[4] = {v0.x + (two ? v1.x : 0.f), v0.y + (two ? v1.y : 0.f), v0.z + (two ? v1.z : 0.f), v0.w + (two ? v1.w : 0.f)};
                const float yy[4] = {yv.x, yv.y, yv.z, yv.w};
                float o[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float yn = (yy[q] - um_s[c + q]) * ur_s[c + q];
                    const float g1 = ug_s[c + q] * (d[q] - u1_s[c + q] - yn * u2_s[c + q]);
                    o[q] = yy[q] > 0.f ? g1 : 0.f;
                    cs[q] += o[q];
                }
                *reinterpret_cast<float4*>(Ds + j * GB_LDD + c) = make_float4(o[0], o[1], o[2], o[3]);
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            cs[q] += __shfl_xor(cs[q], 16, 64);
            cs[q] += __shfl_xor(cs[q], 32, 64);
        }
        if (lane < 16) {
#pragma unroll
            for (int q = 0; q < 4; ++q) bs_s[t >> 6][lane][q] = cs[q];
        }
    }
    // rows rows .. rowsP of dOut / x_hat: zero (they are reduced over in the products below)
    for (int i = t; i < (rowsP - rows) * GB_LDD; i += GB_NT) Ds[rows * GB_LDD + i] = 0.f;
    for (int i = t; i < (rowsP - rows) * LDX; i += GB_NT) Xs[rows * LDX + i] = 0.f;
    if (!ATT) adj_scatter<GB_NT, GB_LDJ>(Ab, er, en, un, t, [&](int j, int s) { return dis_s[j] * ec[s]; }, [&](int j) { return dis_s[j] * dis_s[j] * loop_w; });
    __syncthreads();
    if ((UP || POOL) && t < GC_N) {
        double tot = 0.0;
#pragma unroll
        for (int k = 0; k < GB_NT / 64; ++k) tot += (double)bs_s[k][t >> 2][t & 3];
        br.bias_parts[(size_t)b * H + ns0 + t] = tot;
    }
    // (ATT: 2 = the edge phase's end, 3 = the row phase's -- pinned on wave 0, which runs P1 next: as a plain mark hipcc moved its
    //  store behind the products -- and no clock behind P2)
    if (!ATT) BLK_CLK(2); else BLK_CLK_W(3, 0, t);
    auto ident = [](float v) { return v; };
    gc_f32x16 acc[2];
    // ---- P1: dz[:, ns] = Ab^T dOut[:, ns]   (rows i x 64 columns, reduction over the graph's rowsP nodes) ------------
    {
        const int rt = w >> 1, ct = w & 1;              // waves 0-3: one tile each; waves 4-7 wait at the barriers
#pragma unroll
        for (int i = 0; i < 16; ++i) { acc[0][i] = 0.f; acc[1][i] = 0.f; }
        if (rt < R) mma_kmajor<1, 1, GB_LDJ, GB_LDD>(Ab + rt * 32 + li, Ds + ct * 32 + li, rowsP, lk, ident, MmaIdent(), acc);
        // ATT, waves 4-7 (idle during P1): this slice's columns of the unit's partial rows
        if constexpr (ATT) { if (w >= 4) att_colsum_store(ga.a, red, sc_lds, t - 256, 256, ns0, GC_N, H, sl == 0); }
        if (POOL && w >= 4) {
            // waves 4-7 (idle during P1): gn / gself of this slice, 4 lanes per item (16 columns each) straight from LDS
            const int q4 = (t - 256) & 3, it0 = (t - 256) >> 2;
            float* gn = br.gn + (size_t)sl * br.gn_stride;
            float* gs = br.gself + (size_t)sl * br.gself_stride;
            for (int it = it0; it - it0 < ne + rows; it += 64) {
                const bool ok = it < ne + rows, isedge = it < ne;
                const int itc = ok ? it : 0;
                const int jd = isedge ? er[itc] : itc - ne, js = isedge ? en[itc] : itc - ne;      // destination / source row
                const float4* a = reinterpret_cast<const float4*>(Ds + (ok ? jd : 0) * GB_LDD + 16 * q4);
                const float4* bsrc = reinterpret_cast<const float4*>(Zr + (ok ? js : 0) * GB_LDD + 16 * q4);
                float p = 0.f;
#pragma unroll
                for (int k = 0; k < 4; ++k) p = dot4(a[k], bsrc[k], p);
                p += __shfl_xor(p, 1, 64);
                p += __shfl_xor(p, 2, 64);
                if (ok && q4 == 0) {
                    if (isedge) gn[(LEAN || br.gn_slot) ? e0 + itc : ee[itc]] = p; else gs[g0 + itc - ne] = p;
                }
            }
        }
        __syncthreads();                                 // every wave is done reading dOut (and the z rows)
        if (POOL && LEAN) commit_x();                    // x_hat over the z rows (visible after the barrier below)
        if (rt < R) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = mma_row(r, lk, rt * 32);
                Ds[row * GB_LDD + ct * 32 + li] = acc[0][r];           // dz row-major over the dOut stage
            }
        }
        __syncthreads();
    }
    // The two products behind P1, in the order CAL_GCB_ORDER chooses at build time (engine_gconv_bwd.hpp; LEAN keeps order 0
    // unless the build says 2).
    constexpr bool SEQ = GCB_SEQ && (!LEAN || GCB_SEQ_LEAN);
    if constexpr (SEQ) {
    // ---- order 1, stage A: partial dX' on all eight waves -- wave (rt = w >> 2, kq = w & 3) owns row tile rt x input columns
    // kq * 32 .. + 31 (H = 64: kq 0, 1).  Every element keeps the reduction order of P2 below (mma_rowk, the same k walk).
    {
        const int rt = w >> 2, kq = w & 3, k = kq * 32 + li;
        const bool on = kq * 32 < K;
        // the column sums keep P2's operation sequence: four fp32 chains per sum over the lane's 16 terms of row tile 0, then over
        // its 16 of row tile 1 -- the tile-0 wave parks its 4 + 4 floats per lane (in the adjacency block, dead behind P1), the
        // tile-1 wave picks them up behind ONE barrier and goes on (a graph of <= 32 rows: with zero terms, as P2 adds zero
        // accumulators), folds and adds.  The tile-0 waves enter stage B straight from the barrier: what the consumers wait for
        // -- the dX' tiles, the fold, the striped atomics -- drains under stage B's MFMAs.
        float4* const park = reinterpret_cast<float4*>(Ab);
        float xh[16];
        float f1[4] = {0.f, 0.f, 0.f, 0.f}, f2[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[0][i] = 0.f;
        if (on) {
            // (LEAN: the lane's W row straight from global memory / L2, as in P2 -- read by the waves of both row tiles)
            const float* wrow = LEAN ? br.W + (size_t)k * H + ns0 : Ws + k * GB_LDD;
            if (rt < R) mma_rowk(Ds + (rt * 32 + li) * GB_LDD, wrow, GC_N, lk, acc[0]);
            BLK_CLK_X(4, 4, acc[0][15]);                 // (clocks build: the dX' accumulator of wave 4 is done)
            // x_hat of the tile's rows as ONE batch of unconditional LDS reads, masked after the read (see P2)
#pragma unroll
            for (int r = 0; r < 16; ++r) xh[r] = Xs[(mma_row(r, lk, rt * 32)) * LDX + k];
#pragma unroll
            for (int r = 0; r < 16; ++r) { asm volatile("" : "+v"(xh[r])); if (rt >= R) xh[r] = 0.f; }
            float* dxp = sl ? br.dxp1 : br.dxp0;
            if (rt < R) gc_store_tile<gc_site(WT_DXP)>(acc[0], dxp + (size_t)(g0 + rt * 32) * K + kq * 32, K, rows - rt * 32, li, lk, MmaIdent(),
                                                       ((rows - rt * 32) * K - kq * 32) * 4);
            if (rt == 0) {
#pragma unroll
                for (int r = 0; r < 16; ++r) { const float v = acc[0][r]; f1[r & 3] += v; f2[r & 3] = fmaf(v, xh[r], f2[r & 3]); }
                park[(2 * kq) * 64 + lane] = make_float4(f1[0], f1[1], f1[2], f1[3]);
                park[(2 * kq + 1) * 64 + lane] = make_float4(f2[0], f2[1], f2[2], f2[3]);
            }
        }
        __syncthreads();
        if (!ATT) BLK_CLK(3);
        if (on && rt == 1) {
            const float4 p1 = park[(2 * kq) * 64 + lane], p2 = park[(2 * kq + 1) * 64 + lane];
            f1[0] = p1.x; f1[1] = p1.y; f1[2] = p1.z; f1[3] = p1.w;
            f2[0] = p2.x; f2[1] = p2.y; f2[2] = p2.z; f2[3] = p2.w;
#pragma unroll
            for (int r = 0; r < 16; ++r) { const float v = acc[0][r]; f1[r & 3] += v; f2[r & 3] = fmaf(v, xh[r], f2[r & 3]); }
            double s1, s2;
            colsum_fold(f1, f2, s1, s2);
            if (lk == 0) {
                if (br.dacc_sum) {
                    const size_t po = (size_t)stripe_of_block() * br.dacc_ss + k;
                    atomicAdd(br.dacc_sum + po, s1); atomicAdd(br.dacc_prod + po, s2);
                } else { parts[k] = s1; parts[K + k] = s2; }
            }
        }
        BLK_CLK_X(5, 4, f1[0]);                          // (clocks build: the tile and the atomics of wave 4 have left)
    }
    // ---- order 1, stage B: dW[:, ns] (this graph) on all eight waves -- the (K / 32) x 2 tiles of the slab slice one per wave
    // (wave w: input-column tile w % (K / 32), slice half w / (K / 32); H = 64: waves 0-3).  Per element the reduction order of P3.
    if (w < (K >> 4)) {
        const int ct = w >= (K >> 5) ? 1 : 0, kt = w - ct * (K >> 5), k = kt * 32 + li;
        const float gam = gam_s[k], bet = bet_s[k];
        auto affine = [&](float v) { return fmaf(v, gam, bet); };
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[0][i] = 0.f;
        mma_kmajor_ptrs<1, 1, LDX, GB_LDD>(Xs + kt * 32 + li, nullptr, Ds + ct * 32 + li, nullptr, rowsP, lk, affine, MmaIdent(), acc);
        const int off = kt * 32 * H + ns0 + ct * 32;         // (the extent: to the end of this graph's slab)
        gc_store_tile<gc_site(WT_DW)>(acc[0], slab + off, H, 32, li, lk, MmaIdent(), (K * H - off) * 4);
    }
    BLK_CLK_X(6, 4, acc[0][15]);                         // (clocks build: the slab tile of wave 4, the last to enter stage B, has left)
    } else {
    // ---- P2: partial dX'[:, :] = dz[:, ns] W[:, ns]^T   (rows i x K columns, reduction over the 64 columns of ns) ------
    if (w < 4 && w * 32 < K) {
#pragma unroll
        for (int i = 0; i < 16; ++i) { acc[0][i] = 0.f; acc[1][i] = 0.f; }
        // both operands row-major in the reduction index n (dz rows in Ds, W rows in Ws, stride 68 = 4 mod 32): 16 B reads,
        // four MFMA steps per read; W is staged as loaded (no transposing scatter) and dz needs no transposed copy
        // (LEAN: the lane's W row -- 64 consecutive floats of row w * 32 + li -- comes straight from global memory / L2)
        const float* wrow = LEAN ? br.W + (size_t)min(w * 32 + li, K - 1) * H + ns0 : Ws + (w * 32 + li) * GB_LDD;
        if (R == 2) mma_rowk<true>(Ds + li * GB_LDD, Ds + (32 + li) * GB_LDD, wrow, GC_N, lk, acc[0], acc[1]);
        else mma_rowk<false>(Ds + li * GB_LDD, nullptr, wrow, GC_N, lk, acc[0], acc[1]);
        BLK_CLK_X(4, 0, acc[0][15]);                     // (clocks build: the dX' accumulators of wave 0 are done)
        const int k = w * 32 + li;
        float* dxp = sl ? br.dxp1 : br.dxp0;
        // x_hat of all rows first, as ONE batch of unconditional LDS reads (rows rows .. rowsP are zero, as are their dz;
        // rows past rowsP hold stale LDS and are masked after the read): written as `q < R ? Xs[..] : 0` hipcc made 32
        // branches, each with its own ds_read + s_waitcnt lgkmcnt(0) -- 3.6 us of a 13 us kernel -- and before that, with the
        // read inside the guarded store block, one ~140 ns iteration at a time
        float xh[2][16];
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int r = 0; r < 16; ++r) xh[q][r] = Xs[(mma_row(r, lk, q * 32)) * LDX + k];
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int r = 0; r < 16; ++r) { asm volatile("" : "+v"(xh[q][r])); if (q >= R) xh[q][r] = 0.f; }
        // this lane's 32 terms of the two column sums in fp32 (four independent chains), everything across lanes,
        // workgroups and graphs in fp64 as before: 128 dependent fp64 conversions / adds per lane were 3.5 us here
        float f1[4] = {0.f, 0.f, 0.f, 0.f}, f2[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < 2; ++q) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = mma_row(r, lk, q * 32);
                const float v = acc[q][r];                   // (row tile 1 of a one-tile graph: zero accumulators)
                f1[r & 3] += v;
                f2[r & 3] = fmaf(v, xh[q][r], f2[r & 3]);
            }
        }
        // (16-byte stores, four columns per lane: gc_store_tile)
        // (the extent: from the tile's first word to the end of this graph's rows)
        gc_store_tile<gc_site(WT_DXP)>(acc[0], dxp + (size_t)g0 * K + w * 32, K, rows, li, lk, MmaIdent(), (rows * K - w * 32) * 4);
        if (R == 2) gc_store_tile<gc_site(WT_DXP)>(acc[1], dxp + (size_t)(g0 + 32) * K + w * 32, K, rows - 32, li, lk, MmaIdent(), ((rows - 32) * K - w * 32) * 4);
        double s1, s2;
        colsum_fold(f1, f2, s1, s2);
        if (lk == 0) {
            if (br.dacc_sum) {
                const size_t po = (size_t)stripe_of_block() * br.dacc_ss + k;
                atomicAdd(br.dacc_sum + po, s1); atomicAdd(br.dacc_prod + po, s2);
            } else { parts[k] = s1; parts[K + k] = s2; }
        }
        BLK_CLK_X(5, 0, f1[0]);                          // (clocks build: the tiles and the atomics of wave 0 have left)
    }
    if (!ATT) BLK_CLK(3);
    // ---- P3: dW[:, ns] (this graph) = x'^T dz[:, ns]   (K rows x 64 columns, reduction over the graph's nodes) ---------
    if (w >= 4 && (w - 4) * 32 < K) {
        const int wq = w - 4, k = wq * 32 + li;
        const float gam = gam_s[k], bet = bet_s[k];
        auto affine = [&](float v) { return fmaf(v, gam, bet); };
#pragma unroll
        for (int i = 0; i < 16; ++i) { acc[0][i] = 0.f; acc[1][i] = 0.f; }
        mma_kmajor<1, 2, LDX, GB_LDD>(Xs + wq * 32 + li, Ds + li, rowsP, lk, affine, MmaIdent(), acc);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int off = wq * 32 * H + ns0 + q * 32;      // (the extent: to the end of this graph's slab)
            gc_store_tile<gc_site(WT_DW)>(acc[q], slab + off, H, 32, li, lk, MmaIdent(), (K * H - off) * 4);
        }
        BLK_CLK_X(6, 4, acc[1][15]);                     // (clocks build: the slab tiles of wave 4 have left)
    }
    }
    BLK_CLK(1);
