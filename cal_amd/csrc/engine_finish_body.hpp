// The task loops of the step's final commit, as included text: k_finish (engine.hip) and k_finish_plan (finish_plan.hip) include
// this file behind their prologues.  In scope at the include: fa (FinishArgs), grad, task, bx / nbx (this block's index inside its
// task and the task's blocks), A (AdamArgs, .on already cleared for a flagged step), adam_t, adam_lr.  CAL_FINISH_LDS_GIVEN: the
// includer has declared sred (256 floats) and red (256 doubles) itself (k_finish_plan carves them from the LDS it shares with
// its plan part).
    // Both task kinds are pure reductions over S slabs / P partial rows: the loops keep 8 loads in flight
    // per lane (unconditional on a clamped index, pinned, masked when added) -- as dependent loops with
    // two loads in flight the 58-slab weight-gradient sums made this kernel 11 us.
    if (task < fa.nst) {
        // 64 elements per block pass, the S slabs split over the block's 4 waves (S = #graphs = 128 with the
        // per-graph fused backward): 4x shorter load chains, combined through LDS in a fixed order
        const SlabTask t = fa.st[task];
#ifndef CAL_FINISH_LDS_GIVEN
        __shared__ float sred[256];
#endif
        const int el = threadIdx.x & 63, grp = threadIdx.x >> 6;
        const int per = (t.S + 3) / 4, z_lo = grp * per, z_hi = min(t.S, z_lo + per);
        for (int i0 = bx * 64; i0 < t.n; i0 += nbx * 64) {
            const int i = min(i0 + el, t.n - 1);
            float s0 = 0.f, s1 = 0.f;
            for (int z0 = z_lo; z0 < z_hi; z0 += 8) {
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = t.slabs[(size_t)max(min(z0 + u, z_hi - 1), 0) * t.n + i];
#pragma unroll
                for (int u = 0; u < 8; ++u) asm volatile("" : "+v"(v[u]));
#pragma unroll
                for (int u = 0; u < 8; u += 2) {
                    s0 += z0 + u < z_hi ? v[u] : 0.f;
                    s1 += z0 + u + 1 < z_hi ? v[u + 1] : 0.f;
                }
            }
            sred[threadIdx.x] = s0 + s1;
            __syncthreads();
            if (grp == 0 && i0 + el < t.n) {
                const float gsum = (sred[el] + sred[64 + el]) + (sred[128 + el] + sred[192 + el]);
                t.dst[i] = gsum;
                if (A.on) adam_update(A, (t.dst - grad) + i, gsum, adam_t, adam_lr);
            }
            __syncthreads();
        }
    } else if (task - fa.nst < fa.nct) {
        const CommitTask t = fa.ct[task - fa.nst];
        // 16 part-lanes x 16 columns per block pass
#ifndef CAL_FINISH_LDS_GIVEN
        __shared__ double red[256];
#endif
        const int pl = threadIdx.x >> 4, cl = threadIdx.x & 15;
        for (int c0 = bx * 16; c0 < t.n; c0 += nbx * 16) {
            const int c = c0 + cl, cc = min(c, t.n - 1);
            double sacc = 0.0;
            for (int q0 = pl; q0 < t.P; q0 += 16 * 8) {
                double v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = t.src[(size_t)max(min(q0 + 16 * u, t.P - 1), 0) * t.stride + cc];
#pragma unroll
                for (int u = 0; u < 8; ++u) asm volatile("" : "+v"(v[u]));
#pragma unroll
                for (int u = 0; u < 8; ++u) sacc += q0 + 16 * u < t.P ? v[u] : 0.0;
            }
            red[threadIdx.x] = sacc;
            __syncthreads();
            if (pl == 0 && c < t.n) {
                double tot = 0.0;
#pragma unroll
                for (int k = 0; k < 16; ++k) tot += red[k * 16 + cl];
                const float gv = t.scale * (float)tot;
                grad[t.dst + c] = gv;
                if (A.on) adam_update(A, t.dst + c, gv, adam_t, adam_lr);
            }
            __syncthreads();
        }
    } else if (A.on) {
        const AdamRange r = fa.ar[task - fa.nst - fa.nct];
        const int64_t i = r.begin + (int64_t)bx * 256 + threadIdx.x;
        if (i < r.end) adam_update(A, i, grad[i], adam_t, adam_lr);
    }
