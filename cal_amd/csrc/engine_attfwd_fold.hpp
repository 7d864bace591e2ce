// The attention forward of one graph (k_att_fwd_graph, engine_plan.hpp: model.py:97-111, gcn_conv.py:63-68) as the TAIL of the last
// backbone layer's per-graph forward, k_gconv_fwd_att (gconv_fwd_att.hip: the body of k_gconv_fwd<false, 64, 512> in engine_gconv.hpp
// compiled with CAL_GCF_ATT_UNIT).  H = 128: the graph's output rows are computed by TWO workgroups, one per 64-column slice, and the
// six attention dots of a row run over the full width -- so each workgroup computes the dots over its own 64 columns from the
// output tile it parked in LDS, the two exchange their [64 rows][6] partials through memory, and both add them in slice order:
// the same bits on both sides -- and the bits of k_att_fwd_graph<4, 32>, whose 32-lane sum of a row ends with (lanes 0-15: columns
// 0-63) + (lanes 16-31: columns 64-127); the partials here are formed as its 16-lane halves are.  anode, pq, att and dis_c / dis_o
// are therefore what the launch of its own writes, bit for bit; the fp64 column statistics are added in another order (as the
// striped accumulator planes already are from run to run).  Everything else is slice-local: the bnc / bno column statistics of the slice's own columns, and,
// in the slice-0 workgroup only, anode / pq and the edge phase (att, weighted degrees, dis_c / dis_o).
//
// The exchange (MI355X: the XCDs' L2s are not coherent with each other, a CU's L1 is never refreshed by another CU's stores).
// Producer: the partials as 8-byte agent-scope (write-through) stores, every storing wave drains them, a workgroup barrier, then
// ONE lane stores the workgroup's flag, agent scope.  Consumer: ONE lane polls the partner's flag with relaxed agent-scope loads
// (s_sleep between polls, bounded), a workgroup barrier, then every load of the partner's partials is an agent-scope load (past
// the L1).  One workgroup per CU (the kernel's LDS is over half a CU's), both workgroups of a graph co-resident (the route: one
// round, 2 T <= CUs).  The flags live in the step's fp64 arena (zeroed at the start of every step, like k_ro_step's counters).
// With CAL_AFF_ACQUIRE the consumer also runs an agent-scope acquire behind the poll (the form that does not rest on where the
// loads are served from; ~1.7 us).
#pragma once
#include "engine_kernels.hpp"
#include "engine_gunit.hpp"       // GUnit, ro_pin

namespace cal {

constexpr int AFF_T = 64;                  // rows of a graph (the 64-node forward)
constexpr int AFF_ND = 6;                  // dots per row: node logits 0 / 1, edge projections p0, p1, q0, q1
constexpr int AFF_XCH = AFF_T * AFF_ND;    // floats a workgroup publishes
constexpr int AFF_MAXT = 128;              // graphs per launch at most (two flags each in the arena)
constexpr int AFF_E = 1024;                // CSR slots per graph (= GP_E of k_att_fwd_graph, = the 64-node forward's edge cap)
constexpr int AFF_N = 64;                  // columns of a slice (the forward's GC_N)
constexpr int AFF_LDO = AFF_N + 1;         // row stride of the parked output tile

struct AttFwdFoldArgs {
    CSR gs;                                // CSR by SOURCE (the edge phase; the convolution's own is by destination)
    const float* Wn; const float* bn;      // node_att_mlp [2,H], [2]
    const float* We; const float* be;      // edge_att_mlp [2,2H], [2]
    float* anode; float* pq; float* att; float* dis_c; float* dis_o;
    Acc stc_sum, stc_sq, sto_sum, sto_sq;  // column statistics of a0 x / a1 x (bnc / bno): striped accumulator planes
    int64_t E;
    float fnode, fedge;                    // 1, or 0 for without_node_attention / without_edge_attention
    float* xch;                            // [T][2][AFF_XCH] partial dots, indexed (graph, slice)
    int* flags;                            // [T][2], zero at the start of the step
};

// the tail's operands, requested at the top of the kernel with its other loads
struct AttFwdFoldLoads {
    float4 wq;                             // lane t < 96: four columns of weight row t >> 4 of this slice
    int pv, pn, nd[2], ed[2];              // slice 0: by-source CSR row pointers t, t + 1; targets and edge ids of slots t, t + 512
    float b0, b1, eb0, eb1;
};

__device__ __forceinline__ void aff_issue(AttFwdFoldLoads& fr, const AttFwdFoldArgs& fa, const GUnit& un, int n0, int H, int t) {
    // weight rows in the operand roles of k_att_fwd_graph: Wn[0], Wn[1], then We rows 0, 2 (P, the source's half) and 1, 3 (Q)
    const int q = min(t, 95) >> 4, j4 = t & 15;
    const float* wrow = q < 2 ? fa.Wn + (size_t)q * H : fa.We + (size_t)(((q - 2) & 1) * 2 + ((q - 2) >> 1)) * H;
    fr.wq = *reinterpret_cast<const float4*>(wrow + n0 + 4 * j4);
    fr.b0 = fa.bn[0]; fr.b1 = fa.bn[1]; fr.eb0 = fa.be[0]; fr.eb1 = fa.be[1];
    fr.pv = fr.pn = 0; fr.nd[0] = fr.nd[1] = un.g0; fr.ed[0] = fr.ed[1] = 0;
    if (blockIdx.y == 0) {
        const int rcl = max(un.rows, 0), slot_hi = max(fa.gs.nnz - 1, 0);
        fr.pv = fa.gs.ptr[un.g0 + min(t, rcl)]; fr.pn = fa.gs.ptr[un.g0 + min(t + 1, rcl)];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int s = min(un.e0 + max(min(t + u * 512, un.ne - 1), 0), slot_hi);
            fr.nd[u] = fa.gs.nbr[s];
            fr.ed[u] = fa.gs.eid[s];
        }
    }
}
__device__ __forceinline__ void aff_pin(AttFwdFoldLoads& fr) {
    ro_pin(fr.wq);
    asm volatile("" : "+v"(fr.pv), "+v"(fr.pn), "+v"(fr.nd[0]), "+v"(fr.nd[1]), "+v"(fr.ed[0]), "+v"(fr.ed[1]));
}

// The tail.  Called by all 512 threads behind the barrier that published the parked tile Ot[row * AFF_LDO + column] (rows < rows of
// it are written) and the weight slices wsl[q * 16 + j4].  scr: >= 2048 doubles of LDS that nothing else uses any more.
__device__ __forceinline__ void aff_tail(const AttFwdFoldArgs& fa, AttFwdFoldLoads& fr, const GUnit& un, const float* Ot, const float4* wsl,
                                         double* scr, int n0, float loop_w, int* status) {
    __shared__ __attribute__((aligned(16))) float dot_s[AFF_T * AFF_ND];
    __shared__ float4 pq_s[AFF_T];
    __shared__ int fail_s;
    const int t = threadIdx.x, b = blockIdx.x, sl = blockIdx.y, rows = un.rows;
    // ---- (b) six partial dots per row over this slice's 64 columns, in the order k_att_fwd_graph<4, 32> adds its half of a row: 16
    //      lanes x 4 columns (Vec<4>::dot), then group_sum<16>.  That kernel's group_sum<32> ends with (lanes 0-15) + (lanes 16-31),
    //      which is slice 0 + slice 1: the totals below have its bits.  Rows t >> 4 and 32 + (t >> 4).
    const int l = t & 15;
    float own0[2], own1[2];
    size_t pair[2];
    {
        float4 w[AFF_ND];
#pragma unroll
        for (int q = 0; q < AFF_ND; ++q) w[q] = wsl[q * 16 + l];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int row = (t >> 4) + 32 * u;
            float x[4], d[AFF_ND];
#pragma unroll
            for (int j = 0; j < 4; ++j) x[j] = row < rows ? Ot[row * AFF_LDO + l * 4 + j] : 0.f;
#pragma unroll
            for (int q = 0; q < AFF_ND; ++q) d[q] = group_sum<16>(fmaf(x[3], w[q].w, fmaf(x[2], w[q].z, fmaf(x[1], w[q].y, x[0] * w[q].x))));
            // ---- (c) exchange: lanes 0 .. 2 of a row own the pairs (0, 1), (2, 3), (4, 5) --------------------------------------------
            own0[u] = l == 0 ? d[0] : l == 1 ? d[2] : d[4]; own1[u] = l == 0 ? d[1] : l == 1 ? d[3] : d[5];
            pair[u] = (size_t)row * AFF_ND + 2 * l;
            if (l < 3) {
                unsigned long long* dst = reinterpret_cast<unsigned long long*>(fa.xch + ((size_t)b * 2 + sl) * AFF_XCH + pair[u]);
                const unsigned long long bits = ((unsigned long long)__float_as_uint(own1[u]) << 32) | __float_as_uint(own0[u]);
                __hip_atomic_store(dst, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    // slice 0 stages the edge phase's CSR rows while those stores (and the output tile's) are on their way: nothing of it depends
    // on the exchange, and the barriers below publish it
    const int g0 = un.g0, e0 = un.e0, ne = un.ne;
    __shared__ int sp_s[AFF_T + 1];
    __shared__ short sd_s[AFF_E], sr_s[AFF_E];
    if (sl == 0) {
        if (ne <= 0) { fr.nd[0] = fr.nd[1] = g0; fr.ed[0] = fr.ed[1] = 0; }      // no slot of this graph exists: the clamped loads fetched no index
        if (t <= rows) sp_s[t] = min(max(fr.pv - e0, 0), ne);
        if (t < rows) for (int s = max(fr.pv - e0, 0); s < min(fr.pn - e0, ne); ++s) sr_s[s] = (short)t;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int s = t + u * 512;
            if (s < ne) sd_s[s] = (short)min(max(fr.nd[u] - g0, 0), rows - 1);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // every storing wave, before the barrier the flag store waits behind
    __syncthreads();
    BLK_CLK_X(5, 0, 0);
    if (t == 0) {
        __hip_atomic_store(fa.flags + b * 2 + sl, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // the partner runs the same graph in lock step on another CU (co-resident: the route); the poll gives up after ~2^21
        // rounds and flags status bit 1024 instead of hanging the stream -- the step then updates nothing
        const int* pf = fa.flags + b * 2 + (sl ^ 1);
        int spins = 0, bad = 0;
        while (__hip_atomic_load(pf, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) {
            if (++spins > (1 << 21)) { atomicOr(status, 1024); bad = 1; break; }
            __builtin_amdgcn_s_sleep(1);
        }
#ifdef CAL_AFF_ACQUIRE
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
        fail_s = bad;
    }
    __syncthreads();
    BLK_CLK_X(6, 0, 0);
    if (fail_s) return;                                    // none of the attention outputs is written
    // ---- (d) totals, slice 0 + slice 1 on both sides ----------------------------------------------------------------------------------
    if (l < 3) {
        unsigned long long bits[2];
#pragma unroll
        for (int u = 0; u < 2; ++u)
            bits[u] = __hip_atomic_load(reinterpret_cast<const unsigned long long*>(fa.xch + ((size_t)b * 2 + (sl ^ 1)) * AFF_XCH + pair[u]),
                                        __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const float oth0 = __uint_as_float((unsigned)bits[u]), oth1 = __uint_as_float((unsigned)(bits[u] >> 32));
            dot_s[pair[u]] = sl == 0 ? own0[u] + oth0 : oth0 + own0[u];
            dot_s[pair[u] + 1] = sl == 0 ? own1[u] + oth1 : oth1 + own1[u];
        }
    }
    __syncthreads();
    // wave rg owns rows rg * 8 .. + 7: lane k < 8 computes row rg * 8 + k's softmax (the lines of k_att_fwd_graph), the wave then
    // walks its rows in order with one column of the slice per lane
    const int rg = t >> 6, lane = t & 63;
    float a0v = 0.f, a1v = 0.f;
    if (lane < 8) {
        const int i = rg * 8 + lane;
        const float l0 = fa.fnode * (dot_s[i * AFF_ND] + fr.b0), l1 = fa.fnode * (dot_s[i * AFF_ND + 1] + fr.b1);
        const float p0 = dot_s[i * AFF_ND + 2], p1 = dot_s[i * AFF_ND + 3], q0 = dot_s[i * AFF_ND + 4], q1 = dot_s[i * AFF_ND + 5];
        const float m = fmaxf(l0, l1);
        const float x0 = expf(l0 - m), x1 = expf(l1 - m);
        const float inv = 1.f / (x0 + x1);
        a0v = x0 * inv; a1v = x1 * inv;
        if (i < rows && sl == 0) {
            const size_t v = (size_t)(un.g0 + i);
            fa.anode[2 * v] = a0v;
            fa.anode[2 * v + 1] = a1v;
            const float4 pv = make_float4(p0, p1, q0, q1);
            *reinterpret_cast<float4*>(fa.pq + 4 * v) = pv;
            pq_s[i] = pv;
        }
    }
    // ---- (e) column statistics of this slice's columns: (double)(a0 x), its square, likewise a1; fp64, rows in order --------------------
    double sc1 = 0.0, sc2 = 0.0, so1 = 0.0, so2 = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float a0 = __shfl(a0v, k, 64), a1 = __shfl(a1v, k, 64);
        const int i = rg * 8 + k;
        if (i < rows) {
            const float x = Ot[i * AFF_LDO + lane];
            const double xc = (double)(a0 * x), xo = (double)(a1 * x);
            sc1 += xc; sc2 += xc * xc; so1 += xo; so2 += xo * xo;
        }
    }
    scr[(rg * 4 + 0) * AFF_N + lane] = sc1; scr[(rg * 4 + 1) * AFF_N + lane] = sc2;
    scr[(rg * 4 + 2) * AFF_N + lane] = so1; scr[(rg * 4 + 3) * AFF_N + lane] = so2;
    __syncthreads();
    if (t < 4 * AFF_N) {
        const int q = t >> 6;
        double v[8], tot = 0.0;
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = scr[(k * 4 + q) * AFF_N + lane];
#pragma unroll
        for (int k = 0; k < 8; ++k) tot += v[k];
        const int col = n0 + lane;
        if (q == 0) fa.stc_sum.add(col, tot);
        else if (q == 1) fa.stc_sq.add(col, tot);
        else if (q == 2) fa.sto_sum.add(col, tot);
        else fa.sto_sq.add(col, tot);
    }
    BLK_CLK_X(7, 0, 0);
    if (sl != 0) return;
    // ---- (f) slice 0: edge softmax (model.py:102-104) + weighted degrees, the edge phase of k_att_fwd_graph ---------------------------
    // (the CSR rows were staged before the exchange; pq_s is behind the barrier in front of the statistics' sums)
    __shared__ float a0_s[AFF_E], a1_s[AFF_E];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int s = t + u * 512;
        if (s < ne) {
            const float4 pvv = pq_s[min(max((int)sr_s[s], 0), rows - 1)], qd = pq_s[sd_s[s]];
            const float l0 = fa.fedge * (pvv.x + qd.z + fr.eb0), l1 = fa.fedge * (pvv.y + qd.w + fr.eb1);
            const float m = fmaxf(l0, l1);
            const float x0 = expf(l0 - m), x1 = expf(l1 - m);
            const float inv = 1.f / (x0 + x1);
            const float a0 = x0 * inv, a1 = x1 * inv;
            const int64_t ed = min(max((int64_t)fr.ed[u], (int64_t)0), fa.E - 1);
            fa.att[ed] = a0;
            fa.att[fa.E + ed] = a1;
            a0_s[s] = a0; a1_s[s] = a1;
        }
    }
    __syncthreads();
    if (t < rows) {
        float dc = loop_w, dq = loop_w;
        const int s1 = sp_s[t + 1];
        for (int s = sp_s[t]; s < s1; s += 8) {
            float x[8], y[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) { const int sq = min(s + q, s1 - 1); x[q] = a0_s[sq]; y[q] = a1_s[sq]; }
#pragma unroll
            for (int q = 0; q < 8; ++q) { dc += s + q < s1 ? x[q] : 0.f; dq += s + q < s1 ? y[q] : 0.f; }
        }
        fa.dis_c[g0 + t] = dc == 0.f ? 0.f : 1.0f / sqrtf(dc);
        fa.dis_o[g0 + t] = dq == 0.f ? 0.f : 1.0f / sqrtf(dq);
    }
}

}  // namespace cal
