// The arguments of the step's final commit -- k_finish (engine.hip) and the chained form k_finish_plan (finish_plan.hip), which
// runs the same commit beside the graph plan of the NEXT batch in one launch.  The two kernels share their task loops as included
// text (engine_finish_body.hpp); what differs is the prologue: where the counters are read and written.
#pragma once
#include "engine_kernels.hpp"

namespace cal {

constexpr int MAX_LAYERS = 6;
constexpr int MAX_SLABS = 24;
constexpr int MAX_COMMITS = 64;

struct FinishArgs {
    SlabTask st[MAX_SLABS];
    CommitTask ct[MAX_COMMITS];
    int nst, nct;
    float* stats;            // fused readout: stats[0] = wc*stats[1] + wo*stats[2] + wco*stats[3]
    float wc, wo, wco;
    float* tick;             // Adam step counter to advance (the update follows in the same step) or null
    float* ticked;           // Adam step counter the step's FIRST kernel has already advanced (k_zero_f64), or null: taken back here when the
                             // step is flagged -- whether the update rides in this kernel (adam.on) or follows as k_adam (range overflow)
    unsigned long long* perm_ctr;   // counter of the in-step permutation draw to advance (k_zero_f64's rank-sort workgroups only read it), or null
    // Adam inside this kernel (single-process steps, mode bit 4 without bit 8): every gradient element is updated by the
    // thread that finishes it, the ranges no task writes (gradients other kernels stored directly) by `nar` extra tasks
    // of 256 elements per block; the step counter was advanced by the step's FIRST kernel (a ticket of 2700 blocks on one
    // address, each behind a device-scope fence, cost 47 us)
    AdamArgs adam;
    AdamRange ar[MAX_ADAM_RANGES];
    int nar;
    double* bn0z; int bn0z_n;   // bn_feat's statistics range of the fp64 arena: zeroed HERE for the next step (engine_plan.hpp: PlanFold)
    int* dirty;              // the device word of that invariant, cleared here
    int* host_status;        // host-mapped mirror of status[0] | status[1], written by this kernel (cal_engine_peek_status), or null
    const int* status;       // the engine's status words: while any bit is up (this step's or a sticky earlier one) the gradients are
                             // not trusted and NO parameter / moment is updated (check_status raises and clears them)
    int blk0[MAX_SLABS + MAX_COMMITS + MAX_ADAM_RANGES + 1];   // first block of every task in the flattened 1-D grid (filled at launch)
};

// ---- the chained form (finish_plan.hip) ----------------------------------------------------------------------------------
// Status words of the engine (Engine::status, one 256-byte granule of ints): [0] latest step, [1] sticky, [3] the dirty word of
// PlanFold; the chained steps add
constexpr int ST_PEND = 4;       // [4], [5]: what the plan of a chained step found wrong with ITS batch, one word per chain parity
constexpr int ST_STEP = 6;       // [6], [7]: the Adam step counter between two chained steps (floats), alternating
constexpr int ST_CTR = 8;        // [8 .. 11]: the permutation counter between two chained steps (two 64-bit words), alternating

// The plan of the NEXT batch: k_plan_graph<GP_T, GP_E, 256>'s arguments and its PlanFold duties.  B = 0: no plan part (the
// finish-only launch at the end of a chain).
struct ChainPlan {
    const int64_t* ei; int64_t E; int N, B;
    const int64_t *node_ptr, *edge_ptr, *batch, *tile_gptr;
    int Bgraphs; float loop_w;
    int *ptr_dst, *nbr_dst, *eid_dst, *ptr_src, *nbr_src, *eid_src, *row32, *col32, *gptr, *eptr;
    float* dis_unit;
    int* pending;            // where this plan raises its status bits (1, 2, 8, 16, 32): the pending word of the step it plans for
    const float* x0; int F;
    double *st_sum, *st_sq;  // bn_feat's sums in the NEXT step's arena
    float *coef_dst, *coef_src;
    double* arena; int64_t n; int skip_lo, skip_hi;      // the next step's arena, zeroed here but for bn_feat's statistics range
    unsigned long long* gat_tick;
    int64_t* perm; int permB; unsigned long long seed;   // the next step's permutation draw (null: none), keyed by ctr_in + 1
};
// Where the counters are read and written.  No launch writes an address another of its blocks reads: the commit blocks read
// step_in / ctr_in, block 0 of either part writes step_out / ctr_out, and the host never passes the same word as both.
struct ChainCtl {
    const float* step_in;    // the Adam step counter as the current step's first kernel left it (already advanced)
    float* step_out;         // <- step_in, less the tick of a flagged step, plus the next step's tick when there is a plan part
    const unsigned long long* ctr_in;   // permutation counter of the current step's draw (null: the steps do not draw)
    unsigned long long* ctr_out;        // <- ctr_in + 1
    const int* pend_cur;     // pending word of the CURRENT step (null: its plan was the stand-alone kernel and wrote status itself)
    int nplan;               // blocks of the plan part: ChainPlan::B planning ones + the draw's
};

}  // namespace cal
