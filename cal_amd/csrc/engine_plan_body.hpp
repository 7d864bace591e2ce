// The per-graph plan of k_plan_graph (engine_plan.hpp) behind its PlanFold prologue, as included text: k_plan_graph and the plan
// part of k_finish_plan (finish_plan.hip) include this file.  In scope at the include: GT, GE, NT and k_plan_graph's parameters
// (ei .. coef_src) under their names; workgroup blockIdx.x plans unit blockIdx.x of B.  CAL_PLAN_LDS_GIVEN: the includer has
// declared the LDS arrays itself (k_finish_plan carves them from the LDS it shares with its commit part).
    // coef_dst / coef_src != null: the unit-weight edge coefficient deg^-1/2 of the slot's neighbour, in slot order of either view (the
    // wide per-graph convolutions read them with their first loads instead of chasing nbr -> dis in a second round)
#ifndef CAL_PLAN_LDS_GIVEN
    __shared__ float dis_l[GT];
    // x0 != null: also the column sums / sums of squares of the raw features (bn_feat's batch statistics, model.py:90;
    // F <= 64), pre-reduced per graph in LDS and added to the zeroed accumulators with F fp64 atomics per workgroup
    __shared__ double fs[2][64];
#endif
    constexpr int EU = GE / NT;                          // edges per lane
    static_assert(GE % NT == 0 && GT <= NT && NT >= 256, "block shape");
    constexpr int SU = GT / 64;                          // scan elements per lane
#ifndef CAL_PLAN_LDS_GIVEN
    __shared__ int deg_in[GT], deg_out[GT], off_in[GT + 1], off_out[GT + 1], cur_in[GT], cur_out[GT];
    __shared__ short rl[GE], cl[GE];                     // local endpoints of the graph's edges (edge-id order)
    __shared__ short tn_d[GE], te_d[GE], tn_s[GE], te_s[GE];             // unordered row contents: neighbour, local edge id
    __shared__ int gid_s[GT];                            // packed batch: graph of every row of the tile
#endif
    BLK_CLK(0);
    const int b = blockIdx.x, t = threadIdx.x;
    // packed batch (cal_engine_set_tiles): this workgroup's unit is a TILE of the consecutive graphs [tg0, tg1); node_ptr /
    // edge_ptr are the tiles' offsets.  The batch vector must stay inside [tg0, tg1), sorted, and no edge may join two graphs
    const int64_t tg0 = tile_gptr ? tile_gptr[b] : (int64_t)b, tg1 = tile_gptr ? tile_gptr[b + 1] : (int64_t)b + 1;
    if (tile_gptr && t == 0 && ((b == 0 && tg0 != 0) || (b == B - 1 && tg1 != Bgraphs) || tg1 < tg0)) atomicOr(status, 2);
    const int g0 = (int)node_ptr[b], rows = (int)node_ptr[b + 1] - g0;
    const int64_t e0 = edge_ptr[b];
    const int m = (int)(edge_ptr[b + 1] - e0);
    if (t == 0) {
        gptr[b] = g0; eptr[b] = (int)e0;
        if (b == B - 1) { gptr[B] = g0 + rows; eptr[B] = (int)(e0 + m); ptr_dst[N] = (int)(e0 + m); ptr_src[N] = (int)(e0 + m); }
        if (b == B - 1 && (g0 + rows != N || e0 + m != E)) atomicOr(status, 2);
        if (b == 0 && (g0 != 0 || e0 != 0)) atomicOr(status, 2);
    }
    if (rows < 0 || rows > GT || m < 0 || m > GE) { if (t == 0) atomicOr(status, 8); return; }
    // edges: EU per lane, both endpoints requested before anything waits
    int64_t rv[EU], cv[EU];
#pragma unroll
    for (int u = 0; u < EU; ++u) {
        const int64_t e = e0 + max(min(t + u * NT, m - 1), 0);
        rv[u] = m > 0 ? ei[e] : 0;
        cv[u] = m > 0 ? ei[E + e] : 0;
    }
    const int64_t bv = rows > 0 ? batch[g0 + min(t, rows - 1)] : (int64_t)b;
    if (t < GT) { deg_in[t] = 0; deg_out[t] = 0; cur_in[t] = 0; cur_out[t] = 0; gid_s[t] = (int)(bv - tg0); }
    if (t < 128) fs[t >> 6][t & 63] = 0.0;
    __syncthreads();
    if (x0) {
        // lane t of the first (256 / F) F lanes walks the elements t, t + lanes, ..: its column (t % F) is fixed, so it sums
        // in registers (<= ~10 terms, fp32) and adds ONE pair of values to the LDS accumulators -- one fp64 LDS atomic per
        // element was 480 serialised updates per address at 240-node graphs (5 us of this kernel)
        const int lanes = (NT / F) * F, tot = rows * F;
        float s1 = 0.f, s2 = 0.f;
        if (t < lanes) {
            for (int i0 = t; i0 < tot; i0 += 4 * lanes) {
                float v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = x0[(size_t)g0 * F + min(i0 + u * lanes, tot - 1)];
#pragma unroll
                for (int u = 0; u < 4; ++u) asm volatile("" : "+v"(v[u]));
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float vv = i0 + u * lanes < tot ? v[u] : 0.f;
                    s1 += vv; s2 = fmaf(vv, vv, s2);
                }
            }
            atomicAdd(&fs[0][t % F], (double)s1);
            atomicAdd(&fs[1][t % F], (double)s2);
        }
    }
    if (t < rows && (bv < tg0 || bv >= tg1 || (t > 0 && gid_s[t - 1] > gid_s[t]))) atomicOr(status, 2);
#pragma unroll
    for (int u = 0; u < EU; ++u) {
        const int s = t + u * NT;
        if (s < m) {
            int r = (int)(rv[u] - g0), c = (int)(cv[u] - g0);
            const bool bad = r < 0 || r >= rows || c < 0 || c >= rows;
            if (bad) { atomicOr(status, 1); r = 0; c = 0; }
            if (r == c) atomicOr(status, bad ? 1 : 32);
            if (gid_s[r] != gid_s[c]) atomicOr(status, 16);              // an edge between two graphs of the tile: not a mini-batch
            rl[s] = (short)r; cl[s] = (short)c;
            row32[e0 + s] = g0 + r; col32[e0 + s] = g0 + c;
            atomicAdd(&deg_out[r], 1);
            atomicAdd(&deg_in[c], 1);
        }
    }
    __syncthreads();
    BLK_CLK(2);
    // exclusive scans of the two degree arrays: waves 0 / 1, SU consecutive elements per lane
    if (t < 128) {
        const int* deg = t < 64 ? deg_in : deg_out;
        int* off = t < 64 ? off_in : off_out;
        const int l = t & 63;
        int a[SU], x = 0;
#pragma unroll
        for (int u = 0; u < SU; ++u) { a[u] = SU * l + u < rows ? deg[SU * l + u] : 0; x += a[u]; }
        const int own = x;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(x, o, 64);
            if (l >= o) x += y;
        }
        int ex = x - own;
#pragma unroll
        for (int u = 0; u < SU; ++u) { if (SU * l + u <= rows) off[SU * l + u] = ex; ex += a[u]; }
        if (l == 63) off[rows] = x;                      // the total (rows == GT has no lane for it above)
    }
    __syncthreads();
    if (x0 && t < F) { atomicAdd(st_sum + t, fs[0][t]); atomicAdd(st_sq + t, fs[1][t]); }
    if (t < rows) {
        ptr_dst[g0 + t] = (int)e0 + off_in[t];
        ptr_src[g0 + t] = (int)e0 + off_out[t];
        const float d = (float)deg_out[t] + loop_w;
        const float dd = d == 0.f ? 0.f : 1.0f / sqrtf(d);
        dis_unit[g0 + t] = dd;
        dis_l[t] = dd;
    }
    // scatter into the rows (arbitrary order inside a row) ...
#pragma unroll
    for (int u = 0; u < EU; ++u) {
        const int s = t + u * NT;
        if (s < m) {
            const int r = rl[s], c = cl[s];
            const int p = off_in[c] + atomicAdd(&cur_in[c], 1);
            tn_d[p] = (short)r; te_d[p] = (short)s;
            const int q = off_out[r] + atomicAdd(&cur_out[r], 1);
            tn_s[q] = (short)c; te_s[q] = (short)s;
        }
    }
    __syncthreads();
    BLK_CLK(3);
    // ... then every slot moves to its rank by edge id inside its row
    for (int p = t; p < 2 * m; p += NT) {
        const bool d = p < m;
        const int q = d ? p : p - m;
        const short* te = d ? te_d : te_s;
        const short* tn = d ? tn_d : tn_s;
        const int s = te[q];
        const int v = d ? cl[s] : rl[s];
        const int* off = d ? off_in : off_out;
        const int s0 = off[v], s1 = off[v + 1];
        int rank = 0;
        for (int k = s0; k < s1; k += 8) {               // eight independent LDS reads per round (hub rows: 30+ slots)
            int x[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) x[u] = te[min(k + u, s1 - 1)];
#pragma unroll
            for (int u = 0; u < 8; ++u) rank += (k + u < s1 && x[u] < s) ? 1 : 0;
        }
        const int64_t slot = e0 + s0 + rank;
        if (d) { nbr_dst[slot] = g0 + tn[q]; eid_dst[slot] = (int)(e0 + s); if (coef_dst) coef_dst[slot] = dis_l[tn[q]]; }
        else { nbr_src[slot] = g0 + tn[q]; eid_src[slot] = (int)(e0 + s); if (coef_src) coef_src[slot] = dis_l[tn[q]]; }
    }
    BLK_CLK(1);
