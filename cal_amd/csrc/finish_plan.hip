// k_finish_plan: the final commit of step i (k_finish's work: slab tasks, commit tasks, Adam ranges) and the graph plan of batch
// i + 1 (k_plan_graph<GP_T, GP_E, 256> with its PlanFold duties) in ONE launch; launched by bwd_commit of engine.hip through
// cal_launch_finish_plan when the step's successor is known (cal_engine_set_next).  The two are the one pair of neighbouring
// launches of a training loop that do not depend on each other: nothing in the plan reads a parameter.  Blocks [0, nplan) are the
// plan -- dispatched first, 129 latency-bound workgroups at the headline -- and the commit's ~2700 short reduction blocks fill the
// machine around them.  With no plan part (nplan = 0) it is the finish-only launch that ends a chain.
//
// Both bodies are the included text their stand-alone kernels compile (engine_plan_body.hpp, engine_finish_body.hpp); the
// prologues differ, because run side by side the two would race on every word one of them writes and the other reads
// ("Chained steps"): the counters go through in / out words (ChainCtl), the plan raises its status bits in
// a pending word, and the host gives the next step the other fp64 arena.
//
// LDS: one buffer carved for whichever part a block runs (the maximum of the two, not the sum), so that the commit blocks keep
// the eight waves per SIMD k_finish has.  A code object of its own for the reason gconv_bwd_seq.hip is one; the entry follows
// engine_unit.hpp.
#include <stdint.h>
#include "engine_unit.hpp"

namespace {
#include "engine_kernels.hpp"
#include "engine_plan.hpp"
#include "engine_finish.hpp"

namespace cal {

constexpr int FP_PLAN_LDS = 4 * GP_T + 2 * 64 * 8 + 4 * (4 * GP_T + 2 * (GP_T + 2)) + 6 * 2 * GP_E + 4 * GP_T;
constexpr int FP_LDS = FP_PLAN_LDS > 8192 ? FP_PLAN_LDS : 8192;        // (the draw's 1024 keys: 8192)
static_assert(sizeof(FinishArgs) + sizeof(float*) + sizeof(ChainPlan) + sizeof(ChainCtl) <= 4096, "kernel arguments: 4 KB");
static_assert(FP_LDS >= 256 * 8 && FP_LDS * 9 <= 160 * 1024, "the commit blocks keep 8 waves per SIMD (9 workgroups of LDS per CU)");

__global__ void __launch_bounds__(256) k_finish_plan(const FinishArgs fa, float* __restrict__ grad, const ChainPlan pn, const ChainCtl ctl) {
    __shared__ __align__(16) unsigned char smem[FP_LDS];
    // every earlier kernel of the step has finished, and no block of this launch changes the union: uniform (the one writer, the
    // commit's block 0, only moves bits of the pending word into status[0])
    const int pend = ctl.pend_cur ? ctl.pend_cur[0] : 0;
    const bool flagged = (fa.status[0] | fa.status[1] | pend) != 0;
    if ((int)blockIdx.x < ctl.nplan) {
        // ---- the plan of the next batch ----
        constexpr int GT = GP_T, GE = GP_E, NT = 256;
        const int B = pn.B;
        if ((int)blockIdx.x >= B) {                      // permutation draw (blocks B ..): the commit part writes ctr_in + 1 to ctr_out
            randperm_slice<NT>(pn.perm, pn.permB, pn.seed, ctl.ctr_in, 1ull, (unsigned long long*)smem, (int)blockIdx.x - B);
            return;
        }
        const int64_t per = (pn.n + B - 1) / B, lo = (int64_t)blockIdx.x * per, hi = lo + per < pn.n ? lo + per : pn.n;
        for (int64_t i = lo + threadIdx.x; i < hi; i += NT)
            if (i < pn.skip_lo || i >= pn.skip_hi) pn.arena[i] = 0.0;
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            if (pn.gat_tick) *pn.gat_tick += 1;
            // the current step's tick is taken back when it is flagged (k_finish), the next step's is added (k_plan_graph)
            const float s = ctl.step_in[0];
            ctl.step_out[0] = (flagged ? s - 1.f : s) + 1.f;
            // (no dirty check: inside a chain the host vouches that a commit has run since the last training forward)
        }
        const int64_t* __restrict__ ei = pn.ei; const int64_t E = pn.E; const int N = pn.N;
        const int64_t* __restrict__ node_ptr = pn.node_ptr; const int64_t* __restrict__ edge_ptr = pn.edge_ptr;
        const int64_t* __restrict__ batch = pn.batch; const int64_t* __restrict__ tile_gptr = pn.tile_gptr;
        const int Bgraphs = pn.Bgraphs; const float loop_w = pn.loop_w;
        int* __restrict__ ptr_dst = pn.ptr_dst; int* __restrict__ nbr_dst = pn.nbr_dst; int* __restrict__ eid_dst = pn.eid_dst;
        int* __restrict__ ptr_src = pn.ptr_src; int* __restrict__ nbr_src = pn.nbr_src; int* __restrict__ eid_src = pn.eid_src;
        int* __restrict__ row32 = pn.row32; int* __restrict__ col32 = pn.col32; int* __restrict__ gptr = pn.gptr;
        int* __restrict__ eptr = pn.eptr; float* __restrict__ dis_unit = pn.dis_unit;
        int* __restrict__ status = pn.pending;           // the plan's status bits wait in the pending word of the step it plans for
        const float* __restrict__ x0 = pn.x0; const int F = pn.F;
        double* __restrict__ st_sum = pn.st_sum; double* __restrict__ st_sq = pn.st_sq;
        float* __restrict__ coef_dst = pn.coef_dst; float* __restrict__ coef_src = pn.coef_src;
        // the LDS arrays of engine_plan_body.hpp, carved
        unsigned char* sp = smem;
        double (*fs)[64] = (double (*)[64])sp; sp += 2 * 64 * 8;
        float* dis_l = (float*)sp; sp += 4 * GT;
        int* deg_in = (int*)sp; sp += 4 * GT;
        int* deg_out = (int*)sp; sp += 4 * GT;
        int* cur_in = (int*)sp; sp += 4 * GT;
        int* cur_out = (int*)sp; sp += 4 * GT;
        int* gid_s = (int*)sp; sp += 4 * GT;
        int* off_in = (int*)sp; sp += 4 * (GT + 2);
        int* off_out = (int*)sp; sp += 4 * (GT + 2);
        short* rl = (short*)sp; sp += 2 * GE;
        short* cl = (short*)sp; sp += 2 * GE;
        short* tn_d = (short*)sp; sp += 2 * GE;
        short* te_d = (short*)sp; sp += 2 * GE;
        short* tn_s = (short*)sp; sp += 2 * GE;
        short* te_s = (short*)sp; sp += 2 * GE;
#define CAL_PLAN_LDS_GIVEN
#include "engine_plan_body.hpp"
#undef CAL_PLAN_LDS_GIVEN
        return;
    }
    // ---- the commit of the current step: k_finish behind another prologue ----
    const int fb = (int)blockIdx.x - ctl.nplan;
    int task = 0;
    const int ntask = fa.nst + fa.nct + fa.nar;
    AdamArgs A = fa.adam;
    float adam_t = 0.f, adam_lr = 0.f;
    if (A.on && flagged) A.on = 0;
    if (A.on) { adam_t = ctl.step_in[0]; adam_lr = A.lr[0]; }      // the step's first kernel has already advanced the counter
    while (task + 1 < ntask && fb >= fa.blk0[task + 1]) ++task;
    const int bx = fb - fa.blk0[task], nbx = fa.blk0[task + 1] - fa.blk0[task];
    if (fb == 0 && threadIdx.x == 0) {
        if (fa.stats) fa.stats[0] = fa.wc * fa.stats[1] + fa.wo * fa.stats[2] + fa.wco * fa.stats[3];
        // finish-only: the counter goes back to where the optimizer keeps it, without the tick of a flagged step
        if (ctl.nplan == 0) { const float s = ctl.step_in[0]; ctl.step_out[0] = flagged ? s - 1.f : s; }
        if (ctl.ctr_out) ctl.ctr_out[0] = ctl.ctr_in[0] + 1;
        // what this step's plan found wrong with its batch is the step's from here on (sticky until check_status)
        if (pend) atomicOr(const_cast<int*>(fa.status), pend);
        if (fa.host_status)
            __hip_atomic_store(fa.host_status, fa.status[0] | fa.status[1] | pend, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (fa.bn0z && fb == 0) {
        for (int i = threadIdx.x; i < fa.bn0z_n; i += 256) fa.bn0z[i] = 0.0;
        if (threadIdx.x == 0) *fa.dirty = 0;
    }
    float* sred = (float*)smem;
    double* red = (double*)smem;
#define CAL_FINISH_LDS_GIVEN
#include "engine_finish_body.hpp"
#undef CAL_FINISH_LDS_GIVEN
}

}  // namespace cal
}  // namespace

// at.grid.x = ChainCtl::nplan + the commit's blocks.  Return codes: engine_unit.hpp
extern "C" int cal_launch_finish_plan(const calunit::LaunchSite& at, const void* finish, size_t finish_bytes, float* grad, const void* plan,
                                      size_t plan_bytes, const void* ctl, size_t ctl_bytes) {
    using namespace cal;
    FinishArgs fa; ChainPlan pn; ChainCtl cc;
    if (!calunit::take(fa, finish, finish_bytes) || !calunit::take(pn, plan, plan_bytes) || !calunit::take(cc, ctl, ctl_bytes)) return 2;
    calunit::launch(k_finish_plan, at, dim3(256), fa, grad, pn, cc);
    return 0;
}

CAL_UNIT_BLK_CLOCKS(cal_debug_blk_clocks_finish_plan)
