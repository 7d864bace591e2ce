// The graph-unit staging vocabulary of the per-graph fused kernels (engine_gconv.hpp, engine_gconv_bwd.hpp, engine_ggat.hpp,
// engine_ggin.hpp, engine_gwide.hpp): everything a workgroup does AROUND its MFMA products (engine_mma.hpp) -- the unit's
// extents and their guard, the CSR slot batch, the operand tiles and BatchNorm tables staged in LDS, the z tile / adjacency
// block of the second product, the column-sum epilogue.  All of it is __forceinline__ text of the calling kernel: LDS arrays
// (and their element types, chosen per kernel for LDS reasons) stay declared in the kernels and come in as pointers.
//
//   unit        GUnit, gunit_load, exceeds<T, ECAP>, gunit_flag, gunit_empty_update_running
//   slots       GSlots<U, EID, COEF>: load / load_ids + load_coef, pin, repair_empty, stage; gslots_dest_rows
//   tiles       xrow_issue / xrow_commit (forward x rows), wslice_commit (W slice [k][col])
//   BatchNorm   bn_affine4, bn_table_scale_shift, bn_table_hat, bn_table_upper
//   2nd product z_park, z_combine, adj_zero, adj_scatter
//   epilogue    colsum_fold, colsum_commit
//
// The rule of every prologue here: a small operand is an UNCONDITIONAL load on a clamped index (or through a substituted
// pointer), requested with the tile loads and pinned with them; selects, not branches, turn it into a value afterwards.
// Guarded loads were four to ten serial round trips behind the tile loads (BNRaw in engine.hpp), and without the pins
// hipcc pairs every load with its LDS store ("load, s_waitcnt vmcnt(0), ds_write" per register: 5-30 us of serial round
// trips under 256-way contention).
//
// Kept in the kernels on purpose: what an empty or invalid unit must still write (partial rows, pooled zeros, slab slice,
// the TILED graph count), bn_raws_load2's one-register-set trick of the UP backward kernels, the pool_s leg next to
// k_gconv_fwd's column sums (its store, barrier and lanes are colsum_commit's), and the MFMA / softmax / sparse phases.
//
// Kernels that keep their own copy of a piece, because the shared form changed their register allocation.  The rule is
// IDENTICAL, not "no worse" -- no spill, no scratch, the same VGPR count wherever two or more workgroups share a CU (a
// count that goes down is a different schedule of a latency-bound kernel just as one that goes up), the same waves per
// SIMD elsewhere; profiles/r8/isa_gunit.txt has the comparison that holds for the tree as it is:
//   k_gw_fwd               all of it (its epilogue is not the MFMA tile form): with the unit, slot-batch, W-slice or
//                          BatchNorm-table pieces its four instantiations moved between -9 and +2 VGPRs
//   k_gw_bwd               everything but colsum_fold (k_gw_bwd<false, 1>: +1 VGPR)
//   k_ggin_fwd             extents and guard, W^T slice, x-row tile and slot batch (k_ggin_fwd<1>: 93 -> 92 VGPRs)
//   k_gconv_bwd, k_ggin_bwd   the guard (through exceeds / gunit_flag the LEAN k_gconv_bwd spilled 1-4 VGPRs and
//                          k_ggin_bwd<2> went from 128 to 129 VGPRs, 4 to 3 waves per SIMD)
//   every kernel           the issue of its W slice, ahead of the extents (shared, k_gconv_fwd<., 64, 512, .> went from 93 to
//                          96 / 98 VGPRs; the transposed Linear form of the GIN kernels had one user left)
//   k_gconv_fwd, k_gconv_bwd  the second coefficient round (see GSlots)
#pragma once
#include "engine_readout.hpp"     // ro_pin, CSR, Acc
#include "engine_mma.hpp"         // gc_f32x16

namespace cal {

// ---- the unit: one graph (or tile of graphs) = rows [g0, g0 + rows) and CSR slots [e0, e0 + ne) -------------------------------
struct GUnit {
    int g0, rows, e0, ne;
    __device__ __forceinline__ bool empty() const { return rows <= 0; }
    // the host's bounds (cal_engine_set_graph_bounds) do NOT hold for this unit.  (The predicate is the violation, not
    // "fits": through a negation hipcc lays the flagged block out ahead of the kernel body and every kernel's code shifts.)
    template <int T, int ECAP> __device__ __forceinline__ bool exceeds() const { return rows > T || ne > ECAP || ne < 0; }
};
__device__ __forceinline__ GUnit gunit_load(const int* gptr, const int* eptr, int b) {
    GUnit u;
    u.g0 = gptr[b]; u.rows = gptr[b + 1] - u.g0; u.e0 = eptr[b]; u.ne = eptr[b + 1] - u.e0;
    return u;
}
// the host's bounds were wrong: status bit 8, from lane 0 (an empty unit is not a violation)
__device__ __forceinline__ void gunit_flag(const GUnit& u, int* status, int t) {
    if (u.rows > 0 && t == 0) atomicOr(status, 8);
}
// forward kernels: the workgroup (0, 0) that owns a BatchNorm's running statistics updates them even when its unit is empty
__device__ __forceinline__ void gunit_empty_update_running(const BNRef& bn, int t, int K) {
    if (bn.update && blockIdx.x == 0 && blockIdx.y == 0 && t < K) { const BNRaw r0 = bn_raw_load_st(bn, t); bn_raw_update_running(bn, r0, t); }
}

// ---- CSR slot batch: lane t holds slots t, t + NT, .. of the unit (U per lane) ---------------------------------------------
// nv: neighbour (global node id), ev: edge id (EID), cin: coefficient dis_j * w_e written by an earlier kernel of the step (COEF).
template <int U, bool EID, bool COEF>
struct GSlots {
    int nv[U], ev[EID ? U : 1];
    float cin[COEF ? U : 1], cv[COEF ? U : 1], wv[COEF ? U : 1];      // cv, wv: the second round's results (filled by the kernel)
    // slot q of lane t, clamped into the unit and into the CSR arrays
    template <int NT>
    __device__ __forceinline__ static int slot(const GUnit& u, int t, int q) { return u.e0 + max(min(t + q * NT, u.ne - 1), 0); }

    // first round.  coef_in null: the coefficient load goes to dis[0] instead (the second round ignores it).
    template <int NT>
    __device__ __forceinline__ void load(const CSR& g, const GUnit& u, int t, const float* coef_in = nullptr, const float* dis = nullptr) {
        const int slot_hi = max(g.nnz - 1, 0);
        const float* coefp = coef_in ? coef_in : dis;
        const int coef_hi = coef_in ? slot_hi : 0;
#pragma unroll
        for (int q = 0; q < U; ++q) {
            const int s = min(slot<NT>(u, t, q), slot_hi);
            nv[q] = g.nbr[s];
            if (EID) ev[q] = g.eid[s];
            if (COEF) cin[q] = coefp[min(s, coef_hi)];
        }
    }
    // the same as two batches, for a kernel that requests other operands between them
    template <int NT>
    __device__ __forceinline__ void load_ids(const CSR& g, const GUnit& u, int t) {
        const int slot_hi = max(g.nnz - 1, 0);
#pragma unroll
        for (int q = 0; q < U; ++q) {
            const int s = min(slot<NT>(u, t, q), slot_hi);
            nv[q] = g.nbr[s];
            if (EID) ev[q] = g.eid[s];
        }
    }
    template <int NT>
    __device__ __forceinline__ void load_coef(const CSR& g, const GUnit& u, int t, const float* coef_in, const float* dis) {
        const float* coefp = coef_in ? coef_in : dis;
        const int coef_hi = coef_in ? max(g.nnz - 1, 0) : 0;
#pragma unroll
        for (int q = 0; q < U; ++q) cin[q] = coefp[min(slot<NT>(u, t, q), coef_hi)];
    }
    __device__ __forceinline__ void pin() {
#pragma unroll
        for (int q = 0; q < U; ++q) {
            if constexpr (EID && COEF) asm volatile("" : "+v"(nv[q]), "+v"(ev[q]), "+v"(cin[q]));
            else if constexpr (EID) asm volatile("" : "+v"(nv[q]), "+v"(ev[q]));
            else asm volatile("" : "+v"(nv[q]));
        }
    }
    // no slot of this unit exists: what the clamped loads fetched is not an index
    __device__ __forceinline__ void repair_empty(const GUnit& u) {
        if (u.ne <= 0) {
#pragma unroll
            for (int q = 0; q < U; ++q) { nv[q] = u.g0; if (EID) ev[q] = 0; }
        }
    }
    // The second round (cv = dis_j * w_e from dis[nv] and ew[ev], or cin; wv = the raw w_e) stays written out in the two kernels
    // that have one: as a function -- member or free -- hipcc left cv[1] in scratch memory (12 bytes, a store and a load per
    // workgroup) in every instantiation of k_gconv_fwd and k_gconv_bwd.  Its results live HERE, not in arrays of the kernels:
    // with kernel-local cv / wv (k_gconv_bwd on its old `hasw ? c * wl : c`) the headline step measured 0.45 % slower than the
    // parent against a spread of 0.07 %, the GIN step 0.26 % (profiles/r8/ab_gunit.txt, second table).
    template <int NT, int Q = 0, class St>
    __device__ __forceinline__ void stage(const GUnit& u, int t, int* status, St st) const {
        // (one instantiation per slot instead of a loop: the slot index reaches st() as a constant however late the loop
        //  would have been unrolled -- as a loop variable it left the kernels' per-slot arrays in scratch memory)
        if constexpr (Q < U) {
            const int s = t + Q * NT;
            if (s < u.ne) {
                const int loc = nv[Q] - u.g0;
                const bool inb = loc >= 0 && loc < u.rows;
                st(s, Q, loc, inb);
                if (!inb) atomicOr(status, 16);
            }
            stage<NT, Q + 1>(u, t, status, st);
        }
    }
};
// destination row of every CSR slot: lane t < rows walks its row's slots [s0, s1) (stores only: no LDS latency chain).
// The extents come from ptr_s after a barrier, or straight from the registers that hold ptr[t] - e0 / ptr[t + 1] - e0.
template <class ER>
__device__ __forceinline__ void gslots_dest_rows(ER* er, int t, int s0, int s1) {
    for (int s = s0; s < s1; ++s) er[s] = (ER)t;
}
template <class ER>
__device__ __forceinline__ void gslots_dest_rows(ER* er, const int* ptr_s, int t, int rows) {
    if (t < rows) {
        const int s1 = ptr_s[t + 1];
        gslots_dest_rows(er, t, ptr_s[t], s1);
    }
}

// ---- forward x-row tile: Xr[row * LD + k] ------------------------------------------------------------------------------------
// item (u, t) -> 32-wide k chunk kc, row block rr of RPP rows, row (t >> 3) of the block, float4 (t & 7) of the chunk:
// 8 lanes x 16 B per row (coalesced), and the LDS stores see only 2-way bank conflicts.  RB row blocks cover the unit,
// nkc = K / 32 chunks; items past the tile reload item 0 (clamped, dropped by the commit).  Not ro_issue: its item order differs.
template <int UA, int RPP>
__device__ __forceinline__ void xrow_issue(float4 (&va)[UA], const float* x, const GUnit& un, int K, int nkc, int RB, int t) {
    int kc = 0, rr = 0;
#pragma unroll
    for (int u = 0; u < UA; ++u) {
        const bool ok = kc < nkc;
        const int r = min((ok ? rr : 0) * RPP + (t >> 3), un.rows - 1), k = ((ok ? kc : 0) << 5) + ((t & 7) << 2);
        va[u] = *reinterpret_cast<const float4*>(x + (size_t)(un.g0 + r) * K + k);
        if (++rr == RB) { rr = 0; ++kc; }
    }
}
// f(v, rr, k): the transform of the four values of columns k .. k + 3 in row block rr (reads the BatchNorm tables)
template <int UA, int RPP, int LD, class F>
__device__ __forceinline__ void xrow_commit(const float4 (&va)[UA], float* Xr, int nkc, int RB, int t, F f) {
    int kc = 0, rr = 0;
#pragma unroll
    for (int u = 0; u < UA; ++u) {
        if (kc < nkc) {
            const int r = rr * RPP + (t >> 3), k = (kc << 5) + ((t & 7) << 2);
            *reinterpret_cast<float4*>(Xr + r * LD + k) = f(va[u], rr, k);
        }
        if (++rr == RB) { rr = 0; ++kc; }
    }
}
__device__ __forceinline__ float4 bn_affine4(const float4& v, const float* sc_s, const float* sh_s, int k) {
    return make_float4(fmaf(v.x, sc_s[k], sh_s[k]), fmaf(v.y, sc_s[k + 1], sh_s[k + 1]), fmaf(v.z, sc_s[k + 2], sh_s[k + 2]),
                       fmaf(v.w, sc_s[k + 3], sh_s[k + 3]));
}

// ---- W slice [k][n0 + 4 j4 ..] of 64 columns, 16 lanes per k row, as the kernels request it ahead of the unit's extents ---------
template <int NT, int LDB, int WU>
__device__ __forceinline__ void wslice_commit(const float4 (&vb)[WU], float* Bs, int K, int t) {
#pragma unroll
    for (int u = 0; u < WU; ++u) {
        const int idx = t + u * NT, k = idx >> 4, j4 = idx & 15;
        if (k < K) *reinterpret_cast<float4*>(Bs + k * LDB + 4 * j4) = vb[u];
    }
}
// ---- BatchNorm tables in LDS, from a loaded and pinned BNRawS (striped reader, engine.hpp) -----------------------------------------
// forward: x' = fmaf(x, sc, sh); workgroup (0, 0) also owns the running statistics
__device__ __forceinline__ void bn_table_scale_shift(const BNRef& bn, const BNRawS& raws, int t, int K, float* sc_s, float* sh_s) {
    if (t < K) {
        const BNRaw raw = bn_raws_sum(bn, raws);
        bn_raw_scale_shift(bn, raw, sc_s[t], sh_s[t]);
        if (bn.update && blockIdx.x == 0 && blockIdx.y == 0) bn_raw_update_running(bn, raw, t);
    }
}
// backward: x_hat = (x - mean) * rstd, x' = fmaf(x_hat, gamma, beta)
__device__ __forceinline__ void bn_table_hat(const BNRef& bn, const BNRawS& raws, int t, int K, float* mean_s, float* rstd_s, float* gam_s, float* bet_s) {
    if (t < K) {
        float m1, r1;
        const BNRaw raw = bn_raws_sum(bn, raws);
        bn_raw_mean_rstd(bn, raw, m1, r1);
        mean_s[t] = m1; rstd_s[t] = r1;
        gam_s[t] = raw.g;
        bet_s[t] = raw.b;
    }
}
// the BatchNorm ABOVE, column c of the table: dOut = relu'(y) ug (dY - u1 - y_hat u2), y_hat = (y - um) ur, from the finalised
// BatchNorm-backward sums ud1 / ud2 (inv_n stays a double, see BNRef).  The caller picks the lanes.
__device__ __forceinline__ void bn_table_upper(const BNRef& ubn, const BNRawS& raws, const StripeVal& ud1s, const StripeVal& ud2s, int c,
                                               float* um_s, float* ur_s, float* ug_s, float* u1_s, float* u2_s) {
    float m1, r1;
    const BNRaw uraw = bn_raws_sum(ubn, raws);
    const double ud1 = stripe_total(ud1s, ubn.ss), ud2 = stripe_total(ud2s, ubn.ss);
    bn_raw_mean_rstd(ubn, uraw, m1, r1);
    um_s[c] = m1; ur_s[c] = r1;
    ug_s[c] = uraw.g * r1;
    u1_s[c] = (float)(ud1 * (double)ubn.inv_n);
    u2_s[c] = (float)(ud2 * (double)ubn.inv_n);
}

// ---- z tile parked transposed for the second product: Zt[col * LDT + j] = z[j][col] ----------------------------------------------------
// an accumulator holds rows 8 g + 4 lk .. + 3 of its tile in elements 4 g .. 4 g + 3: four consecutive j of one column
template <int LDT>
__device__ __forceinline__ void z_park(float* Zt, const gc_f32x16& acc, int rt, int ct, int li, int lk) {
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
        const int row = rt * 32 + 8 * gq + 4 * lk;
        *reinterpret_cast<float4*>(Zt + (ct * 32 + li) * LDT + row) = make_float4(acc[4 * gq], acc[4 * gq + 1], acc[4 * gq + 2], acc[4 * gq + 3]);
    }
}
// 512-thread variants: acc = this wave's half of the reduction range + the partner's (parked in Zt); PARK: and back into Zt
template <int LDT, bool PARK>
__device__ __forceinline__ void z_combine(float* Zt, gc_f32x16& acc, int rt, int ct, int li, int lk) {
#pragma unroll
    for (int gq = 0; gq < 4; ++gq) {
        float4* zp = reinterpret_cast<float4*>(Zt + (ct * 32 + li) * LDT + rt * 32 + 8 * gq + 4 * lk);
        const float4 p = *zp;
        acc[4 * gq] += p.x; acc[4 * gq + 1] += p.y; acc[4 * gq + 2] += p.z; acc[4 * gq + 3] += p.w;
        if (PARK) *zp = make_float4(acc[4 * gq], acc[4 * gq + 1], acc[4 * gq + 2], acc[4 * gq + 3]);
    }
}

// ---- dense adjacency block A[i * LD + j] (i: row of the slot's destination as er names it) -------------------------------------------
template <int NT>
__device__ __forceinline__ void adj_zero(float* A, int n4, int t) {        // the first n4 float4s
    float4* z4 = reinterpret_cast<float4*>(A);
    for (int idx = t; idx < n4; idx += NT) z4[idx] = make_float4(0.f, 0.f, 0.f, 0.f);
}
// one lane per CSR slot (then one per self loop): duplicate edges accumulate through the LDS atomic.  One lane per
// destination ROW walked a hub's 30 slots as 30 dependent LDS round trips (read source, read coefficient,
// read-modify-write the block) while the other lanes idled -- the slowest row was the phase.
// edge(i, s): weight of slot s into row i; loop(i): weight of row i's self loop
template <int NT, int LD, class ER, class EN, class Edge, class Loop>
__device__ __forceinline__ void adj_scatter(float* A, const ER* er, const EN* en, const GUnit& u, int t, Edge edge, Loop loop) {
    for (int s = t; s < u.ne; s += NT) {
        const int i = er[s];
        atomicAdd(&A[i * LD + en[s]], edge(i, s));
    }
    if (t < u.rows) atomicAdd(&A[t * LD + t], loop(t));
}

// ---- column sums of an output tile ------------------------------------------------------------------------------------------------------
// A lane's <= 32 terms arrive in fp32 (four chains f[0..3] per sum, masked, no guards: inside the row guard every element was
// a branch with two fp64 conversions and two dependent fp64 adds); everything across lanes / waves / units is fp64.
// Lanes lk = 0 / 1 hold different rows of the same column.
__device__ __forceinline__ void colsum_fold(const float (&f1)[4], const float (&f2)[4], double& s1, double& s2) {
    s1 = ((double)f1[0] + (double)f1[1]) + ((double)f1[2] + (double)f1[3]);
    s2 = ((double)f2[0] + (double)f2[1]) + ((double)f2[2] + (double)f2[3]);
    s1 += __shfl_xor(s1, 32, 64);
    s2 += __shfl_xor(s2, 32, 64);
}
// waves w and w + 2 hold the two row tiles of column tile w & 1: through red, then one add per column into the statistics
__device__ __forceinline__ void colsum_commit(double (&red)[4][2][32], bool own, bool want, int w, int li, int lk, int col, double s1, double s2,
                                              const Acc& st_sum, const Acc& st_sq) {
    if (own && lk == 0) { red[w & 3][0][li] = s1; red[w & 3][1][li] = s2; }
    __syncthreads();
    if (w < 2 && lk == 0 && want) {
        st_sum.add(col, red[w][0][li] + red[w + 2][0][li]);
        st_sq.add(col, red[w][1][li] + red[w + 2][1][li]);
    }
}

}  // namespace cal
