// Native CausalGCN step engine: the whole training step of train_causal.py:173-192 on
// model.py:85-164 -- forward (3 heads), 3-term loss, backward, Adam -- as ONE C call that enqueues
// a few dozen hand-written kernels on a stream (hipGraph-capturable: no allocation, no sync, no memset
// nodes).  What is fused, relative to the op sequence of the reference:
//   * every BatchNorm is folded into its consumer: batch statistics are accumulated (fp64) by the
//     producer's epilogue, the normalised tensor is never written -- the consumer GEMM applies
//     scale/shift (and the node-attention row scale) while staging its operand;
//   * bias + ReLU (+ next-BN statistics) ride on the aggregation / GEMM epilogues;
//   * xc = a0*x, xo = a1*x and the [E,2H] edge representation are never materialised;
//   * the GCN normalisation is computed on the fly from deg^-1/2 (no per-layer norm(), no
//     message tensor);
//   * BatchNorm-backward column sums ride on the GEMM that produces the incoming gradient;
//   * all parameter gradients that are column sums go through one fp64 arena and one commit
//     kernel; split-K weight-gradient slabs are reduced deterministically in the same launch;
//   * the three readout heads (BN -> fc1 -> ReLU -> BN -> fc2 -> log_softmax -> loss) and their backward are ONE launch
//     of resident workgroups that meet at two in-kernel barriers per head (engine_ro_step.hpp);
//   * Adam runs inside that last commit kernel for single-process steps (every gradient element is updated by the
//     thread that finishes it), as one kernel over the flat parameter buffer after a gradient exchange.
#include <string.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <type_traits>
#include <vector>

#include "engine_kernels.hpp"
#include "engine_readout.hpp"
#include "engine_gconv.hpp"
#include "engine_gconv_bwd.hpp"
#include "engine_ggat.hpp"
#include "engine_plan.hpp"
#include "engine_attbwd.hpp"
#include "engine_ro_step.hpp"
#include "engine_gin.hpp"
#include "engine_ggin.hpp"
#include "engine_feat.hpp"
#include "engine_gwide.hpp"
#include "engine_attwide.hpp"
#include "engine_finish.hpp"        // FinishArgs; ChainPlan / ChainCtl (the kernel that takes them is in finish_plan.hip)
#include "engine_attfwd_fold.hpp"     // AttFwdFoldArgs (the kernel that takes them is in gconv_fwd_att.hip)
#include "engine_unit.hpp"            // the entries of the side units (gconv_fwd_att.hip, gconv_bwd_att.hip, gconv_bwd_seq.hip)

namespace cal {

// grid: 1-D, task t owns blocks [blk0[t], blk0[t+1]): n/64 per slab task, ceil(n/16) per commit task (a
// (64, tasks) grid spent most of its ~12k blocks on nothing once the slab tasks wanted 256 blocks each)
__global__ void __launch_bounds__(256) k_finish(const FinishArgs fa, float* __restrict__ grad) {
    int task = 0;
    const int ntask = fa.nst + fa.nct + fa.nar;
    AdamArgs A = fa.adam;
    float adam_t = 0.f, adam_lr = 0.f;
    const bool flagged = fa.status && (fa.status[0] | fa.status[1]) != 0;     // every earlier kernel of the step has finished: uniform
    // a gated step applies no update, so it must not count as one either: the step's first kernel has already advanced the
    // Adam step counter (bias correction) -- take that back (advisor, round 4: the counter drifted by the frozen steps)
    // (advisor, round 5: keyed on adam.on the fallback to a separate k_adam -- adam.on = 0, counter already advanced -- kept counting)
    if (fa.ticked && flagged && blockIdx.x == 0 && threadIdx.x == 0) fa.ticked[0] -= 1.f;
    if (A.on && flagged) A.on = 0;
    if (A.on) { adam_t = A.step[0]; adam_lr = A.lr[0]; }      // the step's first kernel has already advanced the counter
    while (task + 1 < ntask && (int)blockIdx.x >= fa.blk0[task + 1]) ++task;
    const int bx = blockIdx.x - fa.blk0[task], nbx = fa.blk0[task + 1] - fa.blk0[task];
    if (fa.stats && blockIdx.x == 0 && threadIdx.x == 0)
        fa.stats[0] = fa.wc * fa.stats[1] + fa.wo * fa.stats[2] + fa.wco * fa.stats[3];
    if (fa.tick && !flagged && blockIdx.x == 0 && threadIdx.x == 0) fa.tick[0] += 1.f;      // (the k_adam that follows skips a flagged step too)
    if (fa.perm_ctr && blockIdx.x == 0 && threadIdx.x == 0) fa.perm_ctr[0] += 1;
    if (fa.bn0z && blockIdx.x == 0) {
        for (int i = threadIdx.x; i < fa.bn0z_n; i += 256) fa.bn0z[i] = 0.0;
        if (threadIdx.x == 0) *fa.dirty = 0;
    }
    if (fa.host_status && fa.status && blockIdx.x == 0 && threadIdx.x == 0)
        __hip_atomic_store(fa.host_status, fa.status[0] | fa.status[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
#include "engine_finish_body.hpp"
}

struct BNSlot { int gamma, beta; int width; float* rm; float* rv; int64_t* nbt; int arena; };

struct Engine {
    int F, H, C, L;
    int cat;                    // cat_or_add == "cat": the co readout takes cat(xc[perm], xo) [B, 2H] (model.py:65-69,153-154)
    int no_node_att, no_edge_att;   // without_node_attention / without_edge_attention: constant 0.5 masks (model.py:99-107)
    int gin;                    // backbone of GINConv(Linear, BN, ReLU, Linear, ReLU) layers (CausalGIN, model.py:188-194)
    int o_gin_w2[MAX_LAYERS], o_gin_b2[MAX_LAYERS];      // second Linear of every GIN layer (o_conv_w / o_conv_b: the first)
    float *gagg, *gt1, *gy, *ones;   // GIN: per layer aggregation output, pre-BN activations, relu(BN(.)) [L][N,H]; ones [N]
    float loop_w;
    // bound buffers
    float *P, *G, *M1, *M2, *step, *lr;
    int64_t nparam;
    float beta1, beta2, eps, wd;
    unsigned long long perm_seed; unsigned long long* perm_ctr;   // device draw of the random-intervention permutation (mode bit 16)
    int64_t* perm_dev;          // [capB] the permutation drawn by the step itself
    P2PArgs p2p; int p2p_on;    // one-shot peer-memory gradient exchange (cal_engine_p2p_bind)
    int num_cus;                      // compute units of the device (launch-shape decisions)
    int* host_status;                 // host-mapped mirror of the status words, refreshed by every step's last kernel (cal_engine_peek_status)
    int* p2p_host_status;             // host-mapped word k_p2p_adam sets when an exchange timed out (cal_engine_p2p_status)
    int p2p_max_polls;                // bound of k_p2p_adam's flag wait (cal_engine_create: 2^22; cal_engine_p2p_set_timeout)
    float grad_scale;           // gradient factor inside Adam (1 / world_size after a sum all-reduce)
    // parameter offsets (floats into P / G)
    int o_feat_w;
    int o_conv_w[MAX_LAYERS], o_conv_b[MAX_LAYERS];
    int o_eatt_w, o_eatt_b, o_natt_w, o_natt_b;
    int o_cw, o_cb, o_ow, o_ob;
    int o_fc1_w[3], o_fc1_b[3], o_fc2_w[3], o_fc2_b[3];
    // BatchNorms: 0 bn_feat, 1..L bns_conv, L+1 bnc, L+2 bno, L+3+2h fc1_bn_h, L+4+2h fc2_bn_h
    BNSlot bn[MAX_LAYERS + 9];
    int nbn;
    // arena offsets (doubles)
    int a_convb[MAX_LAYERS], a_cb, a_ob, a_dwn, a_dwe, a_db1, a_db2, a_sync, a_aff, arena_n, bn_plane;
    // workspace
    char* ws; size_t ws_bytes;
    int64_t capN, capE, capB;
    // float regions
    float *h, *z, *zco, *hco, *anode, *pq, *att, *dis_unit, *dis_co, *pooled, *pcnt, *xco, *y1, *zl, *logp, *stats, *zpart;
    int adam_fused;          // 1: mode-4 steps apply Adam inside k_finish; CAL_AMD_ADAM_FUSED=0 keeps the k_adam launch
    int ro_rows;             // 1: ... also for 129 .. 512 graphs, in row blocks (k_ro_step<true>); CAL_AMD_RO_ROWS=0: the GEMM chain there
    int striped;             // 1: the per-graph kernels exchange their BatchNorm sums through NSTRIPE accumulator planes (engine.hpp: stripe_sum)
                             // instead of partial rows + k_stats_final; CAL_AMD_STRIPED=0 keeps the finishing launches
    int fold_zero;           // 1: forward + backward steps on the per-graph plan have no k_zero_f64 launch (PlanFold); CAL_AMD_FOLD_ZERO=0: always the launch
    int bn0_dirty_host;      // host twin of the device word status[3]: a training forward has been enqueued since the last k_finish
    int att_fold;            // 1: the per-graph attention backward runs inside the last backbone layer's k_gconv_bwd launch (its ATT mode);
                             // CAL_AMD_ATT_FOLD=0 keeps the two launches
    int att_fwd_fold;        // 1: the per-graph attention forward runs as the tail of the last backbone layer's forward launch (k_gconv_fwd_att);
                             // CAL_AMD_ATT_FWD_FOLD=0 / cal_engine_set_att_fwd_fold(h, 0) keep the two launches
    float* att_xch;          // [AFF_MAXT][2][AFF_XCH] partial attention dots the two slice workgroups of a graph exchange in that launch
    int gwide;              // 1: graphs of 129 .. 256 nodes run the wide per-graph convolutions (engine_gwide.hpp); CAL_AMD_GWIDE=0: the node-level chain
    int ro_step;             // 1: training steps run the readout as one launch (k_ro_step); CAL_AMD_RO_STEP=0 keeps the four kernels
    float *dzl, *dyh1, *dy1, *dxh, *dpool, *dZco, *gn, *gself, *ddeg, *dl, *dzco, *dXhco, *dZ, *dzi, *dXh, *slabs;
    size_t slab_floats;
    double* arena;
    double* parts; size_t parts_doubles;
    int *rowptr_dst, *nbr_dst, *eid_dst, *rowptr_src, *nbr_src, *eid_src, *row32, *col32, *work, *status, *gptr, *iperm, *eptr;
    float* wslot;               // [2][E] attention edge weights (context, objects) in CSR-by-destination slot order
    float* coef_src;            // [E] unit-weight coefficients deg^-1/2 of the destination in CSR-by-SOURCE slot order (k_plan_graph, for the wide per-graph backward)
    float* coef;                // [3][E] edge coefficients dis_j * w_e in CSR-by-destination slot order: unit, context, objects
    int max_nodes, max_edges;   // per-graph bounds of the coming batches (0 = unknown): cal_engine_set_graph_bounds
    const int64_t *node_ptr, *edge_ptr;   // [B+1] device arrays of the coming batch (null = unknown): cal_engine_set_graph_ptrs
    // small-graph packing (cal_engine_set_tiles): the per-graph kernels run one workgroup per TILE = a run of consecutive
    // graphs; node_ptr / edge_ptr and the bounds above then describe tiles, tile_gptr [ntiles + 1] = first graph of every tile
    const int64_t* tile_gptr; int ntiles;
    // GATConv backbone (CausalGAT, model.py:340,390): K heads (0 = GCNConv backbone), attention dropout p with
    // per-layer seeds and an optional device step counter, att [K, 2D] parameter offsets
    int K; float gat_p, gat_slope;
    uint64_t gat_seed[MAX_LAYERS];
    unsigned long long* gat_ctr;
    int o_conv_att[MAX_LAYERS];
    float *gz, *gsc, *gws;      // per layer: z = BN(h) W [L][N,H]; a_dst, a_src, max, denominator [L][4][N,K]; backward scratch
    // what the latest bwd_commit handed k_finish, kept for cal_engine_finish_layout (host bookkeeping only; tests read it):
    // the flat-buffer interval of every slab task (kind 0), commit task (1) and update-only range (2), in task order, and the
    // value of adam_in_finish the step ended with (0: no update in k_finish, 1: in k_finish, 2: fell back to k_adam)
    struct FinishIv { int64_t begin, end; int kind; } fin_iv[MAX_SLABS + MAX_COMMITS + MAX_ADAM_RANGES];
    int fin_n, fin_adam;
    // chained steps (finish_plan.hip; DESIGN.md section 7, "Chained steps"): a step whose successor is known (cal_engine_set_next) ends
    // with k_finish_plan, which also plans the successor; that step then skips fwd_plan and runs on the other fp64 arena
    int chain;               // 1: on; CAL_AMD_CHAIN=0 / cal_engine_set_chain(h, 0): every step ends with k_finish and starts with its own plan
    int chain_ok;            // 0 after cal_engine_chain_reset dropped a planned step: arena 1 is no longer known to be clean (until the next workspace)
    double* arena2[2];       // the two arenas; `arena` is the current step's: arena2[0] for a stand-alone step, alternating inside a chain
    // a batch as a step call describes it; `next`: announced by cal_engine_set_next for the coming call only; `planned`: what the
    // latest k_finish_plan planned for -- the next cal_engine_step must be for exactly this (valid: 1 while a planned step is owed)
    struct BatchDesc {
        const float* x0; const int64_t* ei; const int64_t* batch; int64_t N, E, B;
        const int64_t *node_ptr, *edge_ptr, *tile_gptr; int ntiles, max_nodes, max_edges;
        int mode, parity, valid; const char* ws;
    } next, planned;
};

static size_t al(size_t n) { return (n + 63) / 64 * 64; }   // 256 B granules (in floats/ints)
static int env_on(const char* name) { const char* v = getenv(name); return !(v && v[0] == '0'); }   // CAL_AMD_* switches: on unless "0..."

}  // namespace cal

using namespace cal;
#include "engine_order.hpp"           // pins the order of this file's kernels in its code object: nothing that names a kernel goes in front of it

namespace cal {
int gat_forward(const int32_t* rowptr_dst, const int32_t* nbr_dst, const int32_t* eid_dst, const float* z,
                const float* att, const float* bias, int relu, float slope, float p, uint64_t seed, const uint64_t* ctr,
                float* out, float* adst, float* asrc, float* mx, float* den, int64_t N, int64_t E,
                int64_t K, int64_t D, hipStream_t stream);
int gat_backward(const int32_t* rowptr_dst, const int32_t* nbr_dst, const int32_t* eid_dst,
                 const int32_t* rowptr_src, const int32_t* nbr_src, const int32_t* eid_src, const float* z,
                 const float* att, const float* adst, const float* asrc, const float* mx, const float* den,
                 const float* gout, float slope, float p, uint64_t seed, const uint64_t* ctr, float* dz, float* datt,
                 float* ws, int64_t N, int64_t E, int64_t K, int64_t D, hipStream_t stream, float* part_out, int* nparts);
int gat_datt_parts(int64_t N);
int plan_build(const int64_t* edge_index, int64_t E, int64_t N, int32_t* rowptr_dst, int32_t* nbr_dst, int32_t* eid_dst,
               int32_t* rowptr_src, int32_t* nbr_src, int32_t* eid_src, int32_t* row32, int32_t* col32, int32_t* work,
               int32_t* status, bool prezeroed, hipStream_t stream);
int plan_rank(int64_t E, int64_t N, const int32_t* rowptr_dst, int32_t* nbr_dst, int32_t* eid_dst, const int32_t* rowptr_src,
              int32_t* nbr_src, int32_t* eid_src, const int32_t* row32, const int32_t* col32, const int32_t* scratch,
              hipStream_t stream);
}

extern "C" int64_t cal_gat_bwd_ws(int64_t N, int64_t E, int64_t K, int64_t D);

// cfg: [F, H, C, L].  Returns an opaque handle (0 on failure).
CAL_EXPORT void* cal_engine_create(int64_t F, int64_t H, int64_t C, int64_t L) {
    if (H % 4 != 0 || H > 256 || H < 4 || L < 0 || L > MAX_LAYERS || F < 1 || C < 1 || C > 64) {
        set_error("cal_engine_create: unsupported shape (need hidden %% 4 == 0, hidden <= 256, layers <= %d, classes <= 64)", MAX_LAYERS);
        return nullptr;
    }
    Engine* e = new Engine();
    memset(e, 0, sizeof(Engine));
    if (hipHostMalloc((void**)&e->host_status, 64, hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess) *e->host_status = 0;
    else { (void)hipGetLastError(); e->host_status = nullptr; }       // (no mirror: cal_engine_peek_status reports 0, check_status still works)
    e->ro_step = env_on("CAL_AMD_RO_STEP"); e->ro_rows = env_on("CAL_AMD_RO_ROWS"); e->striped = env_on("CAL_AMD_STRIPED");
    e->gwide = env_on("CAL_AMD_GWIDE"); e->fold_zero = env_on("CAL_AMD_FOLD_ZERO"); e->att_fold = env_on("CAL_AMD_ATT_FOLD");
    e->att_fwd_fold = env_on("CAL_AMD_ATT_FWD_FOLD");
    e->adam_fused = env_on("CAL_AMD_ADAM_FUSED");
    e->chain = env_on("CAL_AMD_CHAIN");
    e->bn0_dirty_host = 1;
    {
        // k_ro_step's 3 * H / 16 workgroups (133 KB of LDS each: one per CU) meet at spin barriers: they must all be
        // resident.  A device (or CU mask / partition) with fewer compute units than that takes the four-kernel readout.
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) cus = 0;
        if (cus < 3 * ((int)H / RO_CW) + 8) e->ro_step = 0;
        e->num_cus = cus > 0 ? cus : 256;
        if (cus < 3 * ((int)H / RO_CW) * RBK_MAXRB + 8) e->ro_rows = 0;
    }
    e->F = (int)F; e->H = (int)H; e->C = (int)C; e->L = (int)L;
    e->loop_w = 1.f;
    e->grad_scale = 1.f;
    e->p2p_max_polls = 1 << 22;
    e->nbn = (int)L + 9;
    return e;
}

CAL_EXPORT void cal_engine_destroy(void* h) {
    Engine* e = (Engine*)h;
    if (!e) return;
    if (e->p2p_host_status) hipHostFree(e->p2p_host_status);
    if (e->host_status) hipHostFree(e->host_status);
    delete e;
}

CAL_EXPORT int64_t cal_engine_num_param_slots(void* h) { Engine* e = (Engine*)h; return 3 + (e->gin ? 6 : 4) * e->L + 12 + 24; }
CAL_EXPORT int64_t cal_engine_num_bn(void* h) { return ((Engine*)h)->nbn; }
// Where BatchNorm k's batch sums live in the fp64 arena (tests read them back): out = {offset of the column sums (plane 0), padded
// width -- the sums of squares follow that many doubles later --, distance of the NSTRIPE accumulator planes}, all in doubles
CAL_EXPORT int cal_engine_bn_arena(void* h, int64_t k, int64_t* out) {
    Engine* e = (Engine*)h;
    CAL_REQUIRE(e != nullptr && out != nullptr && k >= 0 && k < e->nbn, "bad arguments");
    out[0] = e->bn[k].arena; out[1] = (e->bn[k].width + 3) / 4 * 4; out[2] = e->bn_plane;
    return 0;
}

// Bind the flat parameter / gradient / Adam-state buffers.
//   offs[slot]: float offset of every parameter inside P (and G, M1, M2), slots in the order
//     bn_feat.{weight,bias}, conv_feat.weight,
//     {bns_conv.i.weight, bns_conv.i.bias, convs.i.weight, convs.i.bias} for i < L,
//     edge_att_mlp.{weight,bias}, node_att_mlp.{weight,bias}, bnc.{weight,bias}, bno.{weight,bias},
//     context_convs.{weight,bias}, objects_convs.{weight,bias},
//     {fc1_bn_h.weight, .bias, fc1_h.weight, .bias, fc2_bn_h.weight, .bias, fc2_h.weight, .bias} for h in (c, o, co)
//   bn_ptrs[3*k + {0,1,2}]: running_mean / running_var / num_batches_tracked device addresses of
//     BatchNorm k in the order bn_feat, bns_conv.*, bnc, bno, fc1_bn_c, fc2_bn_c, fc1_bn_o, fc2_bn_o,
//     fc1_bn_co, fc2_bn_co.
//   step, lr: device floats (Adam step counter, learning rate).
CAL_EXPORT int cal_engine_bind(void* h, float* P, float* G, float* M1, float* M2, float* step, float* lr,
                               int64_t nparam, const int64_t* offs, const int64_t* bn_ptrs, float beta1, float beta2,
                               float eps, float weight_decay) {
    Engine* e = (Engine*)h;
    e->P = P; e->G = G; e->M1 = M1; e->M2 = M2; e->step = step; e->lr = lr; e->nparam = nparam;
    e->beta1 = beta1; e->beta2 = beta2; e->eps = eps; e->wd = weight_decay;
    const int L = e->L, H = e->H, F = e->F, C = e->C;
    int s = 0;
    int bn_g[MAX_LAYERS + 9], bn_b[MAX_LAYERS + 9], bn_w[MAX_LAYERS + 9];
    int k = 0;
    bn_g[k] = (int)offs[s++]; bn_b[k] = (int)offs[s++]; bn_w[k] = F; ++k;
    e->o_feat_w = (int)offs[s++];
    for (int i = 0; i < L; ++i) {
        bn_g[k] = (int)offs[s++]; bn_b[k] = (int)offs[s++]; bn_w[k] = H; ++k;
        e->o_conv_w[i] = (int)offs[s++]; e->o_conv_b[i] = (int)offs[s++];
        if (e->gin) { e->o_gin_w2[i] = (int)offs[s++]; e->o_gin_b2[i] = (int)offs[s++]; }
    }
    e->o_eatt_w = (int)offs[s++]; e->o_eatt_b = (int)offs[s++];
    e->o_natt_w = (int)offs[s++]; e->o_natt_b = (int)offs[s++];
    bn_g[k] = (int)offs[s++]; bn_b[k] = (int)offs[s++]; bn_w[k] = H; ++k;   // bnc
    bn_g[k] = (int)offs[s++]; bn_b[k] = (int)offs[s++]; bn_w[k] = H; ++k;   // bno
    e->o_cw = (int)offs[s++]; e->o_cb = (int)offs[s++];
    e->o_ow = (int)offs[s++]; e->o_ob = (int)offs[s++];
    for (int hd = 0; hd < 3; ++hd) {
        bn_g[k] = (int)offs[s++]; bn_b[k] = (int)offs[s++]; bn_w[k] = (hd == 2 && e->cat) ? 2 * H : H; ++k;
        e->o_fc1_w[hd] = (int)offs[s++]; e->o_fc1_b[hd] = (int)offs[s++];
        bn_g[k] = (int)offs[s++]; bn_b[k] = (int)offs[s++]; bn_w[k] = H; ++k;
        e->o_fc2_w[hd] = (int)offs[s++]; e->o_fc2_b[hd] = (int)offs[s++];
    }
    int a = 0;
    for (int i = 0; i < L; ++i) { e->a_convb[i] = a; a += H; }
    e->a_cb = a; a += H;
    e->a_ob = a; a += H;
    e->a_dwn = a; a += H + 4;
    e->a_dwe = a; a += 2 * H + 4;
    e->a_db1 = a; a += 3 * H;
    e->a_db2 = a; a += (3 * C + 3) / 4 * 4;
    e->a_sync = a; a += (RBK_SYNC_INTS + 1) / 2 + 2;  // barrier counters of k_ro_step (ints: 6, or RBK_SYNC_INTS row-blocked), zeroed with the arena
    e->a_aff = a; a += AFF_MAXT;                      // k_gconv_fwd_att's flags (ints: two per graph), zeroed with the arena
    // the BatchNorm sums last: NSTRIPE planes of them, bn_plane doubles apart (engine.hpp: stripe_sum); BNSlot::arena is plane 0
    a = (a + 3) / 4 * 4;
    const int a_bn = a;
    for (int i = 0; i < e->nbn; ++i) {
        BNSlot& b = e->bn[i];
        b.gamma = bn_g[i]; b.beta = bn_b[i]; b.width = bn_w[i];
        b.rm = (float*)bn_ptrs[3 * i]; b.rv = (float*)bn_ptrs[3 * i + 1]; b.nbt = (int64_t*)bn_ptrs[3 * i + 2];
        b.arena = a;
        a += 4 * ((b.width + 3) / 4 * 4);
    }
    e->bn_plane = a - a_bn;
    a = a_bn + NSTRIPE * e->bn_plane;
    e->arena_n = a;
    return 0;
}

static size_t engine_layout(Engine* e, int64_t N, int64_t E, int64_t B, bool assign) {
    const size_t H = e->H, C = e->C, L = e->L, F = e->F;
    size_t off = 0;   // in 4-byte units
    auto F32 = [&](float*& p, size_t n) { if (assign) p = (float*)(e->ws) + off; off += al(n); };
    auto I32 = [&](int*& p, size_t n) { if (assign) p = (int*)(e->ws) + off; off += al(n); };
    F32(e->h, (L + 1) * N * H); F32(e->z, N * H); F32(e->zco, 2 * N * H); F32(e->hco, 2 * N * H);
    F32(e->anode, 2 * N); F32(e->pq, 4 * N); F32(e->att, 2 * E); F32(e->dis_unit, N); F32(e->dis_co, 2 * N);
    F32(e->pooled, 2 * B * H); F32(e->pcnt, 2 * B * H); F32(e->xco, 2 * B * H); F32(e->y1, 3 * B * H); F32(e->zl, 3 * B * C); F32(e->logp, 3 * B * C);
    F32(e->stats, 8); F32(e->zpart, 3 * ((H + 15) / 16) * B * C);
    F32(e->dzl, 3 * B * C); F32(e->dyh1, 3 * B * H); F32(e->dy1, 3 * B * H); F32(e->dxh, 4 * B * H); F32(e->dpool, 2 * B * H);
    F32(e->dZco, 2 * N * H); F32(e->gn, 4 * E); F32(e->gself, 4 * N); F32(e->ddeg, 2 * N); F32(e->dl, E);
    F32(e->dzco, 2 * N * H); F32(e->dXhco, 2 * N * H); F32(e->dZ, N * H); F32(e->dzi, (L > 0 ? L : 1) * N * H); F32(e->dXh, N * H);
    // split-K slabs: worst case per weight gradient (S <= 256, but S*tiles ~ 512 => S*M*N <= ~512*64*64 + M*N)
    size_t slab = 0;
    // (per-graph fused backward: one [M,N] slab per graph)
    // (big batches: one slab per 1024-node split-K slice of the 128x128 gradient kernel, gemm_big.hip)
    auto slab_of = [&](size_t M, size_t Nn) {
        const size_t big = gemm_wres_grad((int)M, (int)Nn, (int)N) ? (size_t)gemm_wres_grad_splits((int)N, 1) * M * Nn
                         : gemm_big_grad((int)M, (int)Nn, (int)N) ? (size_t)gemm_big_grad_splits((int)N) * M * Nn : 0;
        return std::max<size_t>(std::max<size_t>(512 * 64 * 64, (size_t)B * M * Nn), big) + 2 * M * Nn;
    };
    slab += slab_of(F, H) + (L + 2) * slab_of(H, H) + 2 * slab_of(H, H) + slab_of(H, 2 * H) + 3 * slab_of(C, H);
    if (e->gin) slab += L * slab_of(H, H);            // two weight gradients per GIN layer
    if (e->K > 0) slab += L * (size_t)1024 * H;      // GATConv: <= 512 partial rows of d att [2H] per layer
    if (assign) e->slab_floats = slab;
    F32(e->slabs, slab);
    {
        float* tmp = nullptr;
        F32(tmp, 2 * (size_t)e->arena_n);
        if (assign) e->arena = e->arena2[0] = (double*)tmp;
        // partial rows of the cross-row sums: <= 1024 producer blocks x (2..6)H columns per set,
        // ~(3L + 16) sets alive per step
        size_t pcap = std::max<size_t>((N + 15) / 16 + 1, (std::min<int64_t>(N, 16384) + 7) / 8 + 1);
        size_t pd = pcap * (size_t)H * 2 * (3 * L + 20);
        F32(tmp, 2 * pd);
        if (assign) { e->parts = (double*)tmp; e->parts_doubles = pd; }
    }
    I32(e->rowptr_dst, N + 1); I32(e->nbr_dst, E); I32(e->eid_dst, E);
    I32(e->rowptr_src, N + 1); I32(e->nbr_src, E); I32(e->eid_src, E);
    I32(e->row32, E); I32(e->col32, E); I32(e->work, 4 * (N + 1) + 4 * E); I32(e->status, 4); I32(e->gptr, B + 1);
    I32(e->iperm, B);
    { int* tmp = nullptr; I32(tmp, 2 * B + 2); if (assign) e->perm_dev = (int64_t*)tmp; }
    I32(e->eptr, B + 1);
    F32(e->coef, 3 * E);
    F32(e->coef_src, E);
    F32(e->wslot, 2 * E);
    if (e->gin) {
        const size_t Lg = L > 0 ? L : 1;
        F32(e->gagg, Lg * N * H); F32(e->gt1, Lg * N * H); F32(e->gy, Lg * N * H); F32(e->ones, N);
    }
    if (e->K > 0) {
        const size_t K = e->K;
        F32(e->gz, (L > 0 ? L : 1) * N * H); F32(e->gsc, (L > 0 ? L : 1) * 4 * al(N * K));
        F32(e->gws, (size_t)cal_gat_bwd_ws(N, E, K, H / K));
    }
    F32(e->att_xch, (size_t)std::min<size_t>(B, AFF_MAXT) * 2 * AFF_XCH);
    {
        // the second arena of chained steps ("arena1"), behind everything else so that every other buffer keeps its offset: whoever
        // sets the workspace zeroes it once (StepEngine.reserve) -- a chain's first k_finish_plan adds bn_feat's sums of the next batch
        // into it, and only a commit that ran on it cleans that range
        float* tmp = nullptr;
        F32(tmp, 2 * (size_t)e->arena_n);
        if (assign) e->arena2[1] = (double*)tmp;
    }
    return off * 4;
}

// Switch the backbone to GATConv(H, H/heads, heads, dropout=p) layers (model.py:340,390).  att_offs[i]: float offset of
// convs.i.att [heads, 2*H/heads] inside P / G; seeds[i]: attention-dropout seed of layer i; ctr: device counter the
// engine advances once per training step and folds into the seeds (null: the seeds are used as given -- tests).
// Call before cal_engine_workspace_bytes / cal_engine_set_workspace (the layout grows by the saved GAT activations).
CAL_EXPORT int cal_engine_set_gat(void* h, int64_t heads, float p, float slope, const int64_t* att_offs,
                                  const uint64_t* seeds, void* ctr) {
    Engine* e = (Engine*)h;
    CAL_REQUIRE(heads > 0 && e->H % heads == 0, "heads must divide hidden");
    const int64_t D = e->H / heads;
    CAL_REQUIRE(D % 4 == 0 && ((D / 4) & (D / 4 - 1)) == 0, "head dim must be 4 * a power of two");
    CAL_REQUIRE(p >= 0.f && p < 1.f, "dropout p must be in [0,1)");
    e->K = (int)heads; e->gat_p = p; e->gat_slope = slope; e->gat_ctr = (unsigned long long*)ctr;
    for (int i = 0; i < e->L; ++i) { e->o_conv_att[i] = (int)att_offs[i]; e->gat_seed[i] = seeds[i]; }
    return 0;
}

CAL_EXPORT int64_t cal_engine_workspace_bytes(void* h, int64_t N, int64_t E, int64_t B) {
    return (int64_t)engine_layout((Engine*)h, N, E, B, false) + 256;
}

CAL_EXPORT int cal_engine_set_workspace(void* h, void* ws, int64_t bytes, int64_t capN, int64_t capE, int64_t capB) {
    Engine* e = (Engine*)h;
    CAL_REQUIRE(((uintptr_t)ws & 255) == 0, "workspace must be 256-byte aligned");
    e->ws = (char*)ws;
    e->capN = capN; e->capE = capE; e->capB = capB;
    size_t need = engine_layout(e, capN, capE, capB, true);
    CAL_REQUIRE((int64_t)need <= bytes, "workspace too small");
    e->ws_bytes = bytes;
    e->bn0_dirty_host = 1;          // nothing is known about the new arena: the next step zeroes all of it (k_zero_f64)
    e->planned.valid = 0; e->next.valid = 0; e->chain_ok = 1;
    return 0;
}

// float offset (from the workspace base) of a named intermediate, for tests / debugging; -1 if unknown
CAL_EXPORT int64_t cal_engine_buffer_offset(void* h, const char* name) {
    Engine* e = (Engine*)h;
    struct { const char* n; void* p; } tab[] = {
        {"h", e->h}, {"z", e->z}, {"zco", e->zco}, {"hco", e->hco}, {"anode", e->anode}, {"pq", e->pq}, {"att", e->att},
        {"dis_unit", e->dis_unit}, {"dis_co", e->dis_co}, {"pooled", e->pooled}, {"xco", e->xco}, {"y1", e->y1},
        {"zl", e->zl}, {"logp", e->logp}, {"stats", e->stats}, {"dzl", e->dzl}, {"dyh1", e->dyh1}, {"dy1", e->dy1},
        {"dxh", e->dxh}, {"dpool", e->dpool}, {"dZco", e->dZco}, {"gn", e->gn}, {"gself", e->gself}, {"ddeg", e->ddeg},
        {"dl", e->dl}, {"dzco", e->dzco}, {"dXhco", e->dXhco}, {"dZ", e->dZ}, {"dzi", e->dzi}, {"dXh", e->dXh},
        {"arena", e->arena2[0]}, {"arena1", e->arena2[1]}, {"gptr", e->gptr}, {"status", e->status}, {"eptr", e->eptr},
        {"gt1", e->gin ? e->gt1 : nullptr}, {"gy", e->gin ? e->gy : nullptr},
        {"rowptr_dst", e->rowptr_dst}, {"nbr_dst", e->nbr_dst}, {"eid_dst", e->eid_dst},
        {"rowptr_src", e->rowptr_src}, {"nbr_src", e->nbr_src}, {"eid_src", e->eid_src}, {"perm", e->perm_dev}, {"ones", e->ones},
    };
    for (auto& t : tab)
        if (!strcmp(t.n, name)) return t.p ? ((char*)t.p - e->ws) / 4 : -1;
    return -1;
}

namespace {

// How a step runs, block by block: chosen once per step (make_route) from the engine, the batch's shape and the mode, and read
// by every phase of engine_forward / engine_backward.  Conv: node-level chain, per-graph kernels for graphs of <= 64 / <= 128 nodes
// (engine_gconv*.hpp; the GAT / GIN ones are the 64-node form), wide per-graph kernels for 129 .. 256 nodes (engine_gwide.hpp).
enum class Plan { Node, Graph256, Graph1024, Big };
enum class Conv { Node, Graph64, Graph128, Wide };
enum class Att { Node, Graph, Wide };
enum class FeatFwd { Gemm, Rows };
enum class FeatBwd { Gemm, Rows, Units };
enum class Readout { Gemm, FourKernel, OneLaunch, Rows };
struct Route {
    Plan plan;          // GraphPlan: k_plan_graph<256 | 1024 threads> per graph, k_plan_big + plan_rank, or the node-level plan_build
    bool plan_stats;    // bn_feat's statistics ride in the plan kernel
    bool plan_coef;     // k_plan_graph writes the unit coefficients for the wide convolutions (coef in slot order, coef_src by source)
    FeatFwd feat_fwd;   // feature layer: tiled GEMM, or row kernels (engine_feat.hpp)
    // Units: k_feat_bwd* fed by the first backbone layer's partial input gradients, per graph or (feat_chunks, behind the wide
    // convolutions) per FB_T-row chunk; Rows: k_bn_bwd_feat, only behind a node-level GCN / GAT layer 1 (the forward's row kernels
    // do not imply the backward's); Gemm: the GEMM chain
    FeatBwd feat_bwd;
    bool feat_chunks;
    // backbone: the forward may run per graph where the backward is node-level (128-node graphs, > 512 units, a GAT layer's
    // per-graph bounds GG_E against GGB_E); a GIN forward in training mode runs per graph only where its backward does (it
    // leaves gt1 alone, and the node-level backward reads gagg / gy)
    Conv bb_fwd, bb_bwd;
    int gw_cols_bb, gw_cols_co;   // wide forward slice width: 32 (two workgroups per CU) when 64-column slices would leave CUs idle
    int nsplit_bb, nsplit_co;     // wide backward: workgroups per (graph, slice) of k_gw_bwd
    bool lean_bb, lean_co;        // per-graph backward: the 80 KB k_gconv_bwd (two workgroups per CU) when there are more workgroups than CUs
    // attention block between the backbone and the causal convolutions: the wide forward needs 3 T >= CUs (fewer workgroups lose
    // to the node-parallel pair), its backward does not; the per-graph forward and backward have bounds of their own
    Att att_fwd, att_bwd;
    int ag_split;                 // workgroups per graph of k_att_bwd_graph / k_att_bwd_wide
    // the per-graph attention backward and the last backbone layer's backward are ONE launch (k_gconv_bwd's ATT mode builds dOut
    // from the attention backward instead of reading e->dZ): GCN layers on the one-workgroup-per-CU k_gconv_bwd only
    bool att_fold;
    // the per-graph attention forward is the tail of the last backbone layer's forward launch (k_gconv_fwd_att, gconv_fwd_att.hip):
    // GCN, H = 128 (the graph's two slice workgroups exchange their partial attention dots inside the launch), striped sums, and
    // a launch of ONE round -- both workgroups of a graph are resident together (2 T <= CUs, one workgroup per CU)
    bool att_fwd_fold;
    // causal convolutions: forward per graph up to 128 nodes, backward only for 64-node graphs of <= 512 units; where the
    // forward pooled per graph and the backward is node-level, the backward counts the positive rows itself (launch_pool_cnt)
    Conv co_fwd, co_bwd;
    // readout: the backward of OneLaunch is done by the forward's launch; Rows leaves slabs for k_finish; FourKernel runs
    // k_ro_bwd_a / _b.  Only training steps with a backward take OneLaunch / Rows.
    Readout ro;
    // BatchNorm sites whose sums go through the accumulator planes (engine.hpp: stripe_sum): those whose producers are per-graph
    // kernels and whose EVERY reader is a striped reader (k_gconv_fwd, k_gconv_bwd, k_att_bwd_graph, k_feat_bwd*, the final commit)
    bool st_feat;       // BatchNorm_1 from the feature layer's GEMM: read by the first backbone layer both ways and k_feat_bwd*
    bool st_bb;         // the backbone's: forward statistics, backward sums of layers L..2 (layers that run per graph both ways)
    bool st_bb1;        // backward sums of layer 1: read by k_feat_bwd*, or by a striped k_bn_bwd (wide), or inside the GIN layer
    bool st_co;         // bnc / bno: statistics from the attention forward, backward sums from the two-branch convolution backward
    // the node-level GCNConv chain of a SMALL batch (graphs beyond the per-graph kernels): the sums that leave a GEMM epilogue
    // go into the planes; their readers are the small-batch GEMMs' prologues, k_bn_bwd<.., ST> and k_att_bwd<.., ST>.  The
    // aggregation / attention kernels' statistics keep their partial rows (thousands of short workgroups).
    bool st_node;
};

struct Ctx {
    Engine* e;
    hipStream_t st;
    int N, B;
    const int64_t* batch;   // [N] graph id of every node (the step's input)
    int T;              // units of the per-graph kernels: tiles of consecutive graphs when the batch is packed, else graphs (= B)
    int64_t E;
    int training;
    int rpb_n, rpb_b;   // rows per block for node-level / graph-level row walkers
    const int64_t* y; const int64_t* perm; float wc, wo, wco; int want_grad;
    int draw_perm;      // the step draws its own intervention permutation (first kernel) into Engine::perm_dev
    int tick_in_finish; // the step ends with the Adam update: k_finish advances the step counter
    int adam_in_finish; // k_finish applies Adam to every gradient it completes (no k_adam launch)
    int chained_in;     // the previous step's k_finish_plan has planned this batch: no fwd_plan, arena and counter words of `parity`
    int chain_out;      // the step ends with k_finish_plan, which plans Engine::next (decided before the forward; bwd_commit may still
                        // fall back when Adam does not fit the commit launch)
    int parity;         // position in the chain, mod 2 (0: a stand-alone step or a chain's first)
    int mode;
    size_t parts_off;   // bump allocator over Engine::parts
    FinalArgs fin;      // pending k_stats_final tasks
    Route r;
};

// what the backward's phases share: the final commit's task list (k_finish), the bump allocator over Engine::slabs, and the
// column sums kept as partial rows until that commit (no finalise launch).  Bwd::slabs / slabs_at / defer (below) are the
// ledger of that workspace: the only code that writes fa.st[], fa.nst, slab_off or a Deferred's fields
struct Deferred {
    double* p; int P; int stride;
    Acc acc() const { return Acc(nullptr, p, stride); }
};
struct Bwd {
    FinishArgs fa;
    size_t slab_off;
    Deferred d_convb[MAX_LAYERS], d_gin_b1[MAX_LAYERS], d_cb, d_ob, d_dwn, d_dwe, d_bn0;
    float* slabs(Ctx& c, int S, int n, float* dst);
    float* slabs_at(Ctx& c, size_t at, int S, int n, float* dst);
    double* defer(Ctx& c, Deferred& d, int P, int cols);
};

void next_ctx(Ctx& cn, Engine* e, hipStream_t st, const Engine::BatchDesc& d, int mode);

BNRef bnref(const Ctx& c, int k, int rows, int update) {
    const Engine* e = c.e;
    const BNSlot& b = e->bn[k];
    BNRef r;
    const int wp = (b.width + 3) / 4 * 4;
    r.sum = e->arena + b.arena; r.sq = e->arena + b.arena + wp;
    r.gamma = e->P + b.gamma; r.beta = e->P + b.beta;
    r.inv_n = 1.0 / (double)rows; r.eps = 1e-5f;
    r.run_mean = b.rm; r.run_var = b.rv; r.nbt = b.nbt;
    r.unbias = rows > 1 ? (float)rows / (float)(rows - 1) : 1.f;
    r.update = (update && c.training) ? 1 : 0;
    r.use_running = c.training ? 0 : 1;
    r.ss = e->bn_plane;
    return r;
}
double* bn_stsum(const Ctx& c, int k) { return c.e->arena + c.e->bn[k].arena; }
double* bn_stsq(const Ctx& c, int k) { return c.e->arena + c.e->bn[k].arena + (c.e->bn[k].width + 3) / 4 * 4; }
double* bn_dsum(const Ctx& c, int k) { return c.e->arena + c.e->bn[k].arena + 2 * ((c.e->bn[k].width + 3) / 4 * 4); }
double* bn_dprod(const Ctx& c, int k) { return c.e->arena + c.e->bn[k].arena + 3 * ((c.e->bn[k].width + 3) / 4 * 4); }

// partial-row accumulator: `cols` columns x P producer blocks, finalised into `dst` by flush_finals
double* parts_alloc(Ctx& c, size_t n) {
    n = (n + 1) & ~(size_t)1;
    if (c.parts_off + n > c.e->parts_doubles) return nullptr;
    double* p = c.e->parts + c.parts_off;
    c.parts_off += n;
    return p;
}
void final_task(Ctx& c, const double* parts, int P, int stride, int n, double* dst) {
    c.fin.t[c.fin.nt++] = FinalTask{parts, P, stride, n, dst};
}
int flush_finals(Ctx& c) {
    if (c.fin.nt == 0) return 0;
    int nmax = 0;
    for (int i = 0; i < c.fin.nt; ++i) nmax = std::max(nmax, c.fin.t[i].n);
    hipLaunchKernelGGL(k_stats_final, dim3(cdiv(nmax, 8), c.fin.nt), dim3(256), 0, c.st, c.fin);
    c.fin.nt = 0;
    cal::g_last_launch = "k_stats_final";
    hipError_t e_ = hipGetLastError();
    if (e_ != hipSuccess) { set_error("k_stats_final: %s", hipGetErrorString(e_)); return 1; }
    return 0;
}
// aggregation launches: one feature row per lane group when nothing is reduced across rows
// (most waves in flight for the gather), two rows per group when the epilogue carries statistics
int spmm_rpb(int H, bool stats, int N = 1 << 30) {
    // (small batches are latency-bound: a second row per group is a second chain of three dependent gathers, 14 vs 8 us
    //  at 7.5 k nodes -- one row per group there, the partial-row buffer holds N / 8 rows up to 16 k nodes)
    // (big batches: every workgroup leaves one fp64 partial row per statistic -- at two rows per group a 160 k-node batch wrote
    //  2 x 20 000 rows of 2 KB and k_stats_final spent 65 us walking them; rows per workgroup grow with N while the launch keeps
    //  >= 4096 workgroups: 131 + 68 us -> 127 + 17 us per layer at config 5, 16 rows per group lose to the tail: 152 + 9)
    const int rows = 256 / group_for(H, 4);
    return stats && N > 16384 ? std::min(8, std::max(2, N / (rows * 4096))) * rows : rows;
}
Acc spmm_acc(Ctx& c, double* dst, int cols, int rpb) {
    const int P = cdiv(c.N, rpb);
    double* p = parts_alloc(c, (size_t)P * cols);
    if (!p) return Acc(dst);
    final_task(c, p, P, cols, cols, dst);
    return Acc(dst, p, cols);
}

// statistics destination for a node-level kernel with P = cdiv(N, rpb_n) blocks: partial rows
// (finalised right away into dst) when the launch is large, atomics otherwise
Acc node_acc(Ctx& c, double* dst, int cols) {
    const int P = cdiv(c.N, c.rpb_n);
    if ((size_t)P * cols <= 4096) return Acc(dst);
    double* p = parts_alloc(c, (size_t)P * cols);
    if (!p) return Acc(dst);
    final_task(c, p, P, cols, cols, dst);
    return Acc(dst, p, cols);
}
// activation x weight products: the K-split kernel wins on latency for few rows (readouts, 4.6 vs
// 6.9 us at 128 rows), the 64x64 tiled kernel on throughput for node-level row counts
bool use_ks(int M) { return M <= 2048; }
int fwd_gemm(Ctx& c, bool transB, const GemmArgs& a, int nbatch) {
    return use_ks(a.M) ? launch_gemm_ks(transB, a, nbatch, c.st) : launch_gemm(false, transB, a, nbatch, c.st);
}
// same for a GEMM epilogue (two sums per column, P = row tiles)
// st: the site's readers are striped readers (engine.hpp) -- k_gemm's row tiles add into the accumulator planes, no finishing launch
void gemm_stats(Ctx& c, GemmProb& pr, int M, int N, double* d0, double* d1, bool dot, int K = 0, bool st = false) {
    if (dot) { pr.dot_sum = d0; pr.dot_prod = d1; } else { pr.st_sum = d0; pr.st_sq = d1; }
    if (st && (use_ks(M) || (!gemm_wres_rows(M, N, K) && !gemm_big_rows(M, K)))) { pr.st_ss = c.e->bn_plane; return; }
    const int P = use_ks(M) ? gemm_ks_row_tiles(M) : gemm_row_tiles(M, N, K);
    if ((size_t)P * N * 2 <= 4096) return;
    double* p = parts_alloc(c, (size_t)P * 2 * N);
    if (!p) return;
    pr.parts = p;
    final_task(c, p, P, 2 * N, N, d0);
    final_task(c, p + N, P, 2 * N, N, d1);
}

GemmArgs gemm_args(int M, int N, int K, bool transA, bool transB, int relu) {
    GemmArgs a;
    memset(&a, 0, sizeof(a));
    a.M = M; a.N = N; a.K = K;
    a.lda = transA ? M : K; a.ldb = transB ? K : N; a.ldc = N;
    a.relu = relu;
    gemm_set_split(a, 1);
    return a;
}

// pick G for H (VEC = 4): lanes per row
template <typename F>
int with_g(int H, F f) {
    int g = group_for(H, 4);
    if (g <= 8) return f(std::integral_constant<int, 8>());
    if (g == 16) return f(std::integral_constant<int, 16>());
    if (g == 32) return f(std::integral_constant<int, 32>());
    return f(std::integral_constant<int, 64>());
}

int pow2ceil(int v) { int p = 1; while (p < v) p <<= 1; return p; }

// k_espmm launch: lanes per row from the width, per-edge weights / output statistics from the branch (both branches alike)
int launch_espmm(hipStream_t st, const CSR& csr, const SpmmBranch2& bb, int nbranch, int relu, float loop_w, int N, int H, int rpb);

#define RC(x) do { int rc_ = (x); if (rc_) return rc_; } while (0)
int no_parts() { set_error("engine: partial-row workspace exhausted"); return 2; }
int no_slabs() { set_error("engine: slab workspace exhausted"); return 2; }
// S slabs of n floats that a kernel has already written `at` floats into the slab workspace (the row-blocked readout's, at its
// front), summed into dst [n] by k_finish: recorded where they are, the allocator moves past them in 64-float granules; null
// (no_slabs()'s error set) when they do not fit
float* Bwd::slabs_at(Ctx& c, size_t at, int S, int n, float* dst) {
    const size_t end = at + (size_t)S * n;
    if (end > c.e->slab_floats || fa.nst >= MAX_SLABS) { no_slabs(); return nullptr; }
    fa.st[fa.nst++] = SlabTask{c.e->slabs + at, dst, n, S};
    slab_off = std::max(slab_off, al(end));
    return c.e->slabs + at;
}
// the same, taken from the allocator (packed: no granule between two takes)
float* Bwd::slabs(Ctx& c, int S, int n, float* dst) {
    const size_t at = slab_off;
    float* p = slabs_at(c, at, S, n, dst);
    if (p) slab_off = at + (size_t)S * n;
    return p;
}
// deferred column sums: P partial rows of `cols` in d, summed by the final commit; null (error set) when the partial-row workspace
// is exhausted or d has already been filled in this step
double* Bwd::defer(Ctx& c, Deferred& d, int P, int cols) {
    if (d.p) { set_error("engine: a deferred column sum was filled twice in one step"); return nullptr; }
    d.p = parts_alloc(c, (size_t)P * cols); d.P = P; d.stride = cols;
    if (!d.p) no_parts();
    return d.p;
}
// a null from the ledger: its error is set
#define RCP(x) do { if (!(x)) return 2; } while (0)

// Slabs of the row-blocked readout (k_ro_step<true>) at the front of the slab workspace, as float offsets from Engine::slabs: per
// (head, row block) one [H,H] fc1 weight-gradient slab, then one [C,H] fc2 slab, head-major
struct RoSlabs {
    size_t nrb, hh, ch;
    size_t w1(int hd) const { return hd * nrb * hh; }
    size_t w2(int hd) const { return 3 * nrb * hh + hd * nrb * ch; }
    size_t total() const { return 3 * nrb * (hh + ch); }
};
RoSlabs ro_slabs(int H, int C, int B) { return RoSlabs{(size_t)cdiv(B, RS_B), (size_t)H * H, (size_t)C * H}; }

// split-K slabs of a weight-gradient GEMM (TN) when the reduction axis is long
int grad_slabs(Ctx& c, Bwd& b, GemmArgs& a, int nbatch, float** dst) {
    gemm_set_split(a, splitk_for(a.M, a.N, a.K, nbatch));
    for (int q = 0; q < nbatch; ++q) RCP(a.p[q].C = a.nsplit > 1 ? b.slabs(c, a.nsplit, a.M * a.N, dst[q]) : dst[q]);
    return 0;
}
// weight-gradient GEMM (TN) with split-K slabs when the reduction axis is long, on the step's stream (a fork to a side stream
// was a measured loss: DESIGN section 7, "Round-4 negatives")
int grad_gemm(Ctx& c, Bwd& b, GemmArgs& a, int nbatch, float** dst) {
    RC(grad_slabs(c, b, a, nbatch, dst));
    return launch_gemm(true, false, a, nbatch, c.st);
}

// dX (NT, `ax`) and dW (TN, `aw`, split-K slabs like grad_gemm) of one layer in a single launch when both
// go to the tiled kernel; otherwise the two launches of before.
int dual_gemm(Ctx& c, Bwd& b, GemmArgs& ax, int nbx, GemmArgs& aw, int nbw, float** dst) {
    if (use_ks(ax.M)) {
        RC(grad_gemm(c, b, aw, nbw, dst));
        return fwd_gemm(c, true, ax, nbx);
    }
    RC(grad_slabs(c, b, aw, nbw, dst));
    return launch_gemm_dual(ax, nbx, aw, nbw, c.st);
}

// live kernel timing for bench.py's roofline block: when enabled, HIP events are attached to the backbone's kernels:
// unfused forward GEMM ([N,H]x[H,H], class 0), aggregation (k_espmm forward / transposed backward, class 1), per-graph
// fused convolution forward (class 2, flops), the backward's dX + dW dual GEMM (class 3, flops), the per-graph fused
// backward (class 4, flops), the GATConv classes 5-8.  Single-kernel scopes (`single`) launch their kernel with
// hipExtLaunchKernelGGL, which stamps the two events with the START and END of that dispatch -- the kernel's own
// duration, what rocprofv3 reports; event records on the stream around the launch also measured the two marker packets
// and the gap between them (20.1 against 16.1 us for k_gconv_bwd).  Multi-kernel scopes (the GEMM helpers of gemm*.hip,
// the GAT backward) keep the records around the launches.  Events are created here (never in a normal step).
struct ProfRec { hipEvent_t e0, e1; int cls; double work; };
static bool g_prof_on = false;
static std::vector<ProfRec> g_prof;
struct ProfScope;
static ProfScope* g_prof_cur = nullptr;
struct ProfScope {
    hipStream_t st; bool on, single, used; ProfRec r;
    ProfScope(hipStream_t s, int cls, double work, bool single_kernel = false) : st(s), on(g_prof_on), single(single_kernel), used(false) {
        if (!on) return;
        r.cls = cls; r.work = work;
        hipEventCreate(&r.e0); hipEventCreate(&r.e1);
        if (single) g_prof_cur = this; else hipEventRecord(r.e0, st);
    }
    ~ProfScope() {
        if (!on) return;
        if (single) { g_prof_cur = nullptr; if (used) g_prof.push_back(r); }
        else { hipEventRecord(r.e1, st); g_prof.push_back(r); }
    }
};
// launch inside a single-kernel ProfScope: the dispatch carries the scope's events when profiling is on
static calunit::LaunchSite prof_site(dim3 grid, hipStream_t st) {
    return {grid, st, g_prof_cur ? g_prof_cur->r.e0 : nullptr, g_prof_cur ? g_prof_cur->r.e1 : nullptr};
}
template <typename K, typename... A>
void prof_launch(K kern, dim3 grid, dim3 block, hipStream_t st, const A&... a) {
    calunit::launch(kern, prof_site(grid, st), block, a...);
    if (g_prof_cur) g_prof_cur->used = true;
}
// the same for a kernel of a side unit (engine_unit.hpp), through the unit's entry; its refusals become the step's error
template <typename... P, typename... A>
int side_launch(int (*entry)(const calunit::LaunchSite&, P...), const char* kernel, const char* file, dim3 grid, hipStream_t st, const A&... a) {
    const int rc = entry(prof_site(grid, st), static_cast<P>(a)...);
    if (rc) { set_error(rc == 2 ? "%s: argument structures differ between engine.hip and %s" : "%s: instantiation missing from %s", kernel, file); return 2; }
    if (g_prof_cur) g_prof_cur->used = true;
    return 0;
}

int launch_espmm(hipStream_t st, const CSR& csr, const SpmmBranch2& bb, int nbranch, int relu, float loop_w, int N, int H, int rpb) {
    const bool wt = bb.b[0].w != nullptr, stt = bb.b[0].st_sum.on(), sd = bb.b[0].sd_z != nullptr;
    if (wt != (bb.b[nbranch - 1].w != nullptr) || stt != bb.b[nbranch - 1].st_sum.on() || sd != (bb.b[nbranch - 1].sd_z != nullptr) || rpb % 4 != 0 || H > 256) {
        set_error("k_espmm: branches differ in kind"); return 2;
    }
    const dim3 grid(cdiv(N, rpb), nbranch);
    if (sd) {       // transposed weighted aggregation + SDDMM
        if (!wt || stt) { set_error("k_espmm: the fused SDDMM is built for the weighted branches without statistics"); return 2; }
        const bool pb = bb.b[0].pb_g != nullptr;
        if (pb != (bb.b[nbranch - 1].pb_g != nullptr)) { set_error("k_espmm: branches differ in kind"); return 2; }
        return with_g(H, [&](auto g) {
            constexpr int G = decltype(g)::value;
            if (pb) prof_launch(k_espmm<4, G, true, false, true, true>, grid, dim3(256), st, csr, bb, relu, loop_w, N, H, rpb);
            else prof_launch(k_espmm<4, G, true, false, true>, grid, dim3(256), st, csr, bb, relu, loop_w, N, H, rpb);
            return 0;
        });
    }
    return with_g(H, [&](auto g) {
        constexpr int G = decltype(g)::value;
        if (wt && stt) prof_launch(k_espmm<4, G, true, true>, grid, dim3(256), st, csr, bb, relu, loop_w, N, H, rpb);
        else if (wt) prof_launch(k_espmm<4, G, true, false>, grid, dim3(256), st, csr, bb, relu, loop_w, N, H, rpb);
        else if (stt) prof_launch(k_espmm<4, G, false, true>, grid, dim3(256), st, csr, bb, relu, loop_w, N, H, rpb);
        else prof_launch(k_espmm<4, G, false, false>, grid, dim3(256), st, csr, bb, relu, loop_w, N, H, rpb);
        return 0;
    });
}

// partial-row statistics of a per-graph kernel: one row per graph; st: into the workgroup's accumulator plane, no finishing launch
Acc graph_acc(Ctx& c, double* dst, int cols, bool st = false) {
    if (st) return Acc(dst, nullptr, c.e->bn_plane);
    double* p = parts_alloc(c, (size_t)c.T * cols);
    if (!p) return Acc(dst);
    final_task(c, p, c.T, cols, cols, dst);
    return Acc(dst, p, cols);
}
CSR csr_dst(const Ctx& c) { return CSR{c.e->rowptr_dst, c.e->nbr_dst, c.e->eid_dst, (int)c.E}; }
CSR csr_src(const Ctx& c) { return CSR{c.e->rowptr_src, c.e->nbr_src, c.e->eid_src, (int)c.E}; }

// the BatchNorm-backward sums of a per-graph backward kernel: into the accumulator planes of the site (st: every reader adds
// them), or P partial rows [sum | prod] finalised by k_stats_final
template <typename Args>
int bn_bwd_sums(Ctx& c, Args& a, int P, double* dsum, double* dprod, bool st) {
    if (st) { a.dacc_sum = dsum; a.dacc_prod = dprod; a.dacc_ss = c.e->bn_plane; return 0; }
    const int H = c.e->H;
    double* p = parts_alloc(c, (size_t)P * 2 * H);
    if (!p) return no_parts();
    a.dot_parts = p;
    final_task(c, p, P, 2 * H, H, dsum);
    final_task(c, p + H, P, 2 * H, H, dprod);
    return 0;
}

// Launch the per-graph fused backward for nb branches (2: the causal convolutions, 1: a backbone layer): slabs (one per graph)
// and the BatchNorm-backward partial rows are registered like those of the GEMM path.  gb[k].dot_parts / .slab are filled in here.
int gconv_bwd(Ctx& c, Bwd& b, GconvBwdBranch* gb, int nb, float** dst, double** dsum, double** dprod, bool st, const AttBwdGraphArgs* att = nullptr) {
    Engine* e = c.e;
    const bool co = nb == 2;
    const bool wide = (co ? c.r.co_bwd : c.r.bb_bwd) == Conv::Wide;
    const int nsplit = co ? c.r.nsplit_co : c.r.nsplit_bb;
    const bool lean = co ? c.r.lean_co : c.r.lean_bb;
    const int H = e->H, B = c.T, nsl = H / GC_N;         // (B: units of this launch -- tiles or graphs)
    const int np2 = nsplit == 4 ? 2 : 1;                 // workgroups per (graph, slice) that leave BatchNorm-backward partial rows
    for (int k = 0; k < nb; ++k) {
        gb[k].batch = c.batch; gb[k].tile_gptr = e->ntiles > 0 ? e->tile_gptr : nullptr;
        RCP(gb[k].slab = b.slabs(c, B, H * H, dst[k]));
        RC(bn_bwd_sums(c, gb[k], B * nsl * np2, dsum[k], dprod[k], st));
    }
    const GconvBwdBranch2 b2{{gb[0], gb[nb - 1]}};
    if (wide) {
        // graphs of up to 256 nodes (engine_gwide.hpp): CSR by SOURCE; the dX' and dW products of a (graph, slice) go to two or
        // four workgroups when one each would leave CUs without one
        const CSR gs = csr_src(c);
        const dim3 gridw(B, nsl * nsplit, nb);
        if (co) prof_launch(k_gw_bwd<true, 2>, gridw, dim3(GW_NT), c.st, gs, e->gptr, e->eptr, b2, e->loop_w, c.N, H, H, nsplit, e->status);
        else if (gb[0].dout) prof_launch(k_gw_bwd<false, 0>, gridw, dim3(GW_NT), c.st, gs, e->gptr, e->eptr, b2, e->loop_w, c.N, H, H, nsplit, e->status);
        else prof_launch(k_gw_bwd<false, 1>, gridw, dim3(GW_NT), c.st, gs, e->gptr, e->eptr, b2, e->loop_w, c.N, H, H, nsplit, e->status);
        CAL_CHECK_LAUNCH("k_gw_bwd");
        return 0;
    }
    const CSR gd = csr_dst(c);
    const dim3 grid(B, nsl, nb);
    if (att) {      // ATT: dOut comes from the attention backward inside the launch (bwd_att)
        if (co || lean || gb[0].dout) { set_error("k_gconv_bwd: the ATT mode is a one-branch, one-workgroup-per-CU launch"); return 2; }
        RC(side_launch(cal_launch_gconv_bwd_att, "k_gconv_bwd_att", "gconv_bwd_att.hip", grid, c.st, &gd, sizeof(gd), e->gptr, e->eptr,
                       &b2, sizeof(b2), e->loop_w, c.N, H, H, e->status, att, sizeof(*att)));
        CAL_CHECK_LAUNCH("k_att_bwd_graph");
        return 0;
    }
    // lean: the 80 KB instantiation, two workgroups per CU -- the two-branch launch at 128 graphs is twice the CUs, packed batches
    // and batches of > 128 graphs more (its two-branch gn goes out in slot order: only when k_att_bwd_graph consumes it)
    const bool tiles = e->ntiles > 0;
    auto kern = co ? (lean ? (tiles ? k_gconv_bwd<true, 2, true, true> : k_gconv_bwd<true, 2, false, true>) : tiles ? k_gconv_bwd<true, 2, true> : k_gconv_bwd<true, 2>)
              : gb[0].dout ? (lean ? k_gconv_bwd<false, 0, false, true> : k_gconv_bwd<false, 0>) : lean ? k_gconv_bwd<false, 1, false, true> : k_gconv_bwd<false, 1>;
    // order 1 of the two products (engine_gconv_bwd.hpp: the non-LEAN instantiations; 2: all): those kernels are in
    // gconv_bwd_seq.hip, a code object of their own; this file's instantiations serve the LEAN launches and the order-0 builds
    if (CAL_GCB_ORDER != 0 && (!lean || CAL_GCB_ORDER == 2)) {
        const int sel = (co ? 1 : 0) | (co && tiles ? 2 : 0) | (!co && gb[0].dout ? 4 : 0) | (lean ? 8 : 0);
        RC(side_launch(cal_launch_gconv_bwd_seq, "k_gconv_bwd", "gconv_bwd_seq.hip", grid, c.st, sel, &gd, sizeof(gd), e->gptr, e->eptr,
                       &b2, sizeof(b2), e->loop_w, c.N, H, H, e->status));
        CAL_CHECK_LAUNCH("k_gconv_bwd");
        return 0;
    }
    prof_launch(kern, grid, dim3(GB_NT), c.st, gd, e->gptr, e->eptr, b2, e->loop_w, c.N, H, H, e->status);
    CAL_CHECK_LAUNCH("k_gconv_bwd");
    return 0;
}

RoArgs make_ro(const Ctx& c) {
    Engine* e = c.e;
    const int L = e->L, H = e->H, C = e->C, B = c.B;
    RoArgs a;
    memset(&a, 0, sizeof(a));
    for (int hd = 0; hd < 3; ++hd) {
        RoHead& h = a.h[hd];
        const int k1 = L + 3 + 2 * hd, k2 = L + 4 + 2 * hd;
        h.W1 = e->P + e->o_fc1_w[hd]; h.b1 = e->P + e->o_fc1_b[hd];
        h.W2 = e->P + e->o_fc2_w[hd]; h.b2 = e->P + e->o_fc2_b[hd];
        h.bn1 = bnref(c, k1, B, 1); h.bn2 = bnref(c, k2, B, 1);
        h.st2_sum = bn_stsum(c, k2); h.st2_sq = bn_stsq(c, k2);
        h.d1_sum = bn_dsum(c, k1); h.d1_prod = bn_dprod(c, k1);
        h.d2_sum = bn_dsum(c, k2); h.d2_prod = bn_dprod(c, k2);
        h.db1 = e->arena + e->a_db1 + hd * H; h.db2 = e->arena + e->a_db2 + hd * C;
        h.gW1 = e->G + e->o_fc1_w[hd]; h.gW2 = e->G + e->o_fc2_w[hd];
    }
    a.pooled = e->pooled; a.perm = c.perm; a.iperm = e->iperm; a.xco = e->xco; a.y1 = e->y1;
    a.zl = e->zl; a.logp = e->logp; a.dzl = e->dzl; a.dy1 = e->dy1; a.dxin = e->dxh;
    a.rowloss = e->dyh1;                  // [6,B] scratch: the unfused path's dyh1 is idle here
    a.y = c.y; a.stats = e->stats; a.B = B; a.H = H; a.C = C;
    a.wc = c.wc; a.wo = c.wo; a.wco = c.wco; a.training = c.training; a.want_grad = c.want_grad;
    return a;
}

// profiling aid: cal_engine_debug_stop(k) makes the step return after its k-th launch site (0 = run all)
static int g_stop_after = 0;
static int g_stage = 0;
static std::vector<const char*> g_stage_names;      // launch-site names of the latest full step
#define STAGE() do { if (g_stop_after == 0) g_stage_names.push_back(cal::g_last_launch); \
                     if (g_stop_after > 0 && ++g_stage >= g_stop_after) return -12345; } while (0)

// launch helper of the row-wise GIN passes (engine_gin.hpp): mode 0 forward BN + ReLU, 1 masked BatchNorm-backward sums,
// 2 BatchNorm backward behind the ReLU, 3 ReLU mask + column sums
int gin_rows(Ctx& c, int mode, const GinRowArgs& ga) {
    const int N = c.N, H = c.e->H;
    hipStream_t st = c.st;
    return with_g(H, [&](auto g) {
        constexpr int G = decltype(g)::value;
        const dim3 grid(cdiv(N, c.rpb_n));
        if (mode == 0) hipLaunchKernelGGL((k_gin_rows<4, G, 0>), grid, dim3(256), 0, st, ga, N, H, c.rpb_n);
        else if (mode == 1) hipLaunchKernelGGL((k_gin_rows<4, G, 1>), grid, dim3(256), 0, st, ga, N, H, c.rpb_n);
        else if (mode == 2) hipLaunchKernelGGL((k_gin_rows<4, G, 2>), grid, dim3(256), 0, st, ga, N, H, c.rpb_n);
        else hipLaunchKernelGGL((k_gin_rows<4, G, 3>), grid, dim3(256), 0, st, ga, N, H, c.rpb_n);
        return 0;
    });
}

template <typename Fn>
int with_g_fp(int H, int F, Fn f) {
    return with_g(H, [&](auto g) {
        constexpr int G = decltype(g)::value;
        if constexpr (G >= FEAT_FMAX) {
            if (F <= 4) return f(g, std::integral_constant<int, 4>());
            if (F <= 8) return f(g, std::integral_constant<int, 8>());
            if (F <= 12) return f(g, std::integral_constant<int, 12>());
            return f(g, std::integral_constant<int, 16>());
        } else {
            set_error("feature row kernels: hidden width too small"); return 2;
        }
    });
}

// few large graphs: split every graph's rows over S workgroups (slices parked in dZco, a backward-only buffer that the
// backward itself no longer writes; slices of >= 128 rows: at S = 4 the 256 workgroups of config 5 read its 328 MB at 3.3 TB/s)
int pool2_slices(int N, int B) { return std::max(1, std::min(32, N / std::max(1, B * 128))); }
// add-pool of the two causal branches (model.py:115-116) + the per-graph positive counts the node-level backward uses.
// hc / ho [N, H], pooled [2, B, H], cnt [2, B, H] or null, slices: S x [4, B, H] floats when S = pool2_slices > 1
int launch_pool2(hipStream_t st, const float* hc, const float* ho, const int* gptr, float* pooled, float* cnt, float* slices,
                 int N, int B, int H) {
    const int tc = std::min(256, pow2ceil(H / 4));
    const int S = pool2_slices(N, B);
    hipLaunchKernelGGL((k_pool2<4>), dim3(B, 2, S), dim3(256), 0, st, hc, ho, gptr, pooled, pooled + (size_t)B * H, H, tc, slices, cnt);
    CAL_CHECK_LAUNCH("k_pool2");
    if (S > 1) {
        hipLaunchKernelGGL(k_pool2_sum, dim3(cdiv(4 * (int64_t)B * H, 256)), dim3(256), 0, st, slices, S, 2 * (int64_t)B * H, pooled, cnt);
        CAL_CHECK_LAUNCH("k_pool2_sum");
    }
    return 0;
}
int launch_pool2(Ctx& c) {
    Engine* e = c.e;
    const size_t NH = (size_t)c.N * e->H;
    return launch_pool2(c.st, e->hco, e->hco + NH, e->gptr, e->pooled, e->pcnt, e->dZco, (int)c.N, (int)c.B, e->H);
}
// the counts alone (forward pooled per graph inside k_gconv_fwd, backward node-level); cnt [2, B, H]
int launch_pool_cnt(hipStream_t st, const float* hc, const float* ho, const int64_t* batch, float* cnt, int N, int B, int H, int rpb_n) {
    hipLaunchKernelGGL(k_zero_f32, dim3(cdiv(2 * (int64_t)B * H, 256)), dim3(256), 0, st, cnt, 2 * (int64_t)B * H);
    CAL_CHECK_LAUNCH("k_zero_f32");
    return with_g(H, [&](auto g) {
        constexpr int G = decltype(g)::value;
        hipLaunchKernelGGL((k_pool_cnt<4, G>), dim3(cdiv(N, rpb_n), 2), dim3(256), 0, st, hc, ho, batch, cnt, N, B, H, rpb_n);
        CAL_CHECK_LAUNCH("k_pool_cnt");
        return 0;
    });
}
int launch_pool_cnt(Ctx& c) {
    Engine* e = c.e;
    const size_t NH = (size_t)c.N * e->H;
    return launch_pool_cnt(c.st, e->hco, e->hco + NH, c.batch, e->pcnt, (int)c.N, (int)c.B, e->H, c.rpb_n);
}

// The route of a step of this shape and mode (want_grad: a backward follows the forward in the same step)
Route make_route(const Ctx& c, bool want_grad) {
    const Engine* e = c.e;
    const int N = c.N, B = c.B, T = c.T, H = e->H, F = e->F, C = e->C, L = e->L, mn = e->max_nodes, me = e->max_edges;
    const bool gin = e->gin, gat = e->K > 0, gcn = !gin && !gat;
    Route r;
    memset(&r, 0, sizeof(r));
    // per-graph plan (engine_plan.hpp) when the host vouches for the batch layout; for graphs of up to 8192 nodes (config 5) one
    // 1024-thread workgroup per graph, rows ranked from a global scratch
    const bool layout = e->node_ptr && e->edge_ptr && B > 0 && mn > 0;
    if (layout && mn <= GP_T2 && me <= GP_E2) r.plan = mn > GP_T || me > GP_E ? Plan::Graph1024 : Plan::Graph256;
    else if (layout && e->ntiles == 0 && mn <= GPB_T) r.plan = Plan::Big;
    else r.plan = Plan::Node;
    const bool graph_plan = r.plan == Plan::Graph256 || r.plan == Plan::Graph1024;
    r.plan_stats = r.plan != Plan::Node && c.training && F <= 64;
    // per-graph fused convolutions (engine_gconv.hpp): need the batch's per-graph bounds from the host; backward: 64-node graphs
    const bool gc = mn > 0 && mn <= GC_T && me <= GC_E && H % GC_N == 0 && H <= GC_K && B > 0;
    const bool small = mn <= 64 && me <= gc_edge_cap(64);
    const bool gcb = gc && small && T <= 128 * 4;
    // wide per-graph convolutions, both ways (engine_gwide.hpp): graphs of 129 .. 256 nodes (the reference's default SPMotif shape)
    const bool gw = e->gwide && mn > GC_T && mn <= GW_T && me <= GW_E && H % GC_N == 0 && H <= GW_K && B > 0 && e->ntiles == 0 && gcn;
    r.plan_coef = graph_plan && gw;
    if (gin) {
        r.bb_fwd = gc && small && (!c.training || (gcb && me <= GB_E)) ? Conv::Graph64 : Conv::Node;
        r.bb_bwd = gcb && me <= GB_E ? Conv::Graph64 : Conv::Node;
    } else if (gat) {
        const int D = H / e->K;
        r.bb_fwd = gc && small && (D == 32 || D == 64) && me <= GG_E ? Conv::Graph64 : Conv::Node;
        r.bb_bwd = gcb && (D == 32 || D == 64) && me <= GGB_E ? Conv::Graph64 : Conv::Node;
    } else {
        r.bb_fwd = gw ? Conv::Wide : !gc ? Conv::Node : small ? Conv::Graph64 : Conv::Graph128;
        r.bb_bwd = gw ? Conv::Wide : gcb ? Conv::Graph64 : Conv::Node;
    }
    r.co_fwd = gw ? Conv::Wide : !gc ? Conv::Node : small ? Conv::Graph64 : Conv::Graph128;
    r.co_bwd = gw ? Conv::Wide : gcb ? Conv::Graph64 : Conv::Node;
    const int64_t w1 = (int64_t)T * (H / GC_N), w2 = 2 * w1;     // workgroups of a one- / two-branch per-graph launch
    r.gw_cols_bb = w1 * 2 <= e->num_cus ? 32 : 64;
    r.gw_cols_co = w2 * 2 <= e->num_cus ? 32 : 64;
    auto nsplit = [&](int64_t w) { return !gw ? 1 : w * 4 <= e->num_cus ? 4 : w * 2 <= e->num_cus ? 2 : 1; };
    r.nsplit_bb = nsplit(w1); r.nsplit_co = nsplit(w2);
    // attention: per graph needs the per-graph plan's facts (a graph's edges are one run of edge_index columns, no self loops)
    const bool aw = gw && e->node_ptr && e->edge_ptr && mn <= AW_T && me <= AW_E && H <= 256 && T <= 512;
    const bool ag = gc && mn <= 4 * (512 / group_for(H, 4)) && me <= GP_E;
    r.att_fwd = aw && 3 * T >= e->num_cus ? Att::Wide : ag ? Att::Graph : Att::Node;
    r.att_bwd = aw ? Att::Wide : gcb && T <= 256 ? Att::Graph : Att::Node;
    r.ag_split = aw ? std::max(1, std::min(8, e->num_cus / std::max(T, 1))) : 2;
    r.lean_bb = w1 > e->num_cus;
    r.lean_co = w2 > e->num_cus && r.att_bwd == Att::Graph;
    r.att_fold = e->att_fold && gcn && r.att_bwd == Att::Graph && r.bb_bwd == Conv::Graph64 && L >= 1 && !r.lean_bb;
    // narrow feature matrices of big batches: the feature layer as row kernels (engine_feat.hpp) instead of tiled GEMMs
    const bool feat_rows = F <= FEAT_FMAX && N > 16384 && H % 4 == 0 && H <= 256 && group_for(H, 4) >= FEAT_FMAX;
    r.feat_fwd = feat_rows ? FeatFwd::Rows : FeatFwd::Gemm;
    r.feat_chunks = r.bb_bwd == Conv::Wide;
    const bool rides = H <= FB_H && (r.feat_chunks ? F <= FB_F : F <= FM_F);
    if (L == 0) r.feat_bwd = FeatBwd::Gemm;
    else if (r.bb_bwd != Conv::Node) r.feat_bwd = rides ? FeatBwd::Units : FeatBwd::Gemm;
    else r.feat_bwd = feat_rows && !gin ? FeatBwd::Rows : FeatBwd::Gemm;
    const bool st = e->striped && c.training;
    r.st_bb = st && r.bb_fwd == r.bb_bwd && r.bb_bwd != Conv::Node;
    r.st_bb1 = r.st_bb && (gin || gw || r.feat_bwd == FeatBwd::Units);
    r.st_node = st && gcn && !gc && N > 0 && N < 16384;
    r.st_feat = (r.st_bb && !gin && !gw && r.feat_bwd == FeatBwd::Units) || r.st_node;
    r.st_co = gw ? st : st && ag && gcb && T <= 256;
    r.att_fwd_fold = e->att_fwd_fold && gcn && r.bb_fwd == Conv::Graph64 && r.att_fwd == Att::Graph && H == 2 * GC_N && L >= 1 &&
                     e->ntiles == 0 && r.st_co && 2 * T <= e->num_cus && T <= AFF_MAXT;
    // readout (the 2H-wide co head of cat takes the GEMM chain); row blocks: training steps of 129 .. 512 graphs
    const int B4 = (B + 15) & ~15;
    const bool ro = !e->cat && (size_t)B4 * (H + 4) <= (size_t)RO_LDS && B * H <= 16384 && H % RO_CW == 0 && B4 <= 256 && H <= 256 &&
                    B * C <= 2048 && C <= 64;
    const bool ro_rows = e->ro_rows && e->ro_step && !e->cat && B > RS_B && B <= RBK_MAXRB * RS_B && H <= RS_K && H % RO_CW == 0 &&
                         RS_B * C <= 2048 && C <= 64 && ro_slabs(H, C, B).total() <= e->slab_floats;
    const bool step = want_grad && c.training;
    r.ro = ro && step && B <= RS_B && H <= RS_K && e->ro_step ? Readout::OneLaunch : ro_rows && step ? Readout::Rows
         : ro ? Readout::FourKernel : Readout::Gemm;
    return r;
}

// 0. zero the fp64 arena and the GraphPlan counters (one kernel, not memset nodes) -- or, for a forward + backward step on the
//    per-graph plan, nothing: those duties ride in k_plan_graph (engine_plan.hpp: PlanFold) and bn_feat's statistics range was
//    zeroed by the previous step's k_finish.  1. GraphPlan
int fwd_plan(Ctx& c, const float* x0, const int64_t* edge_index) {
    Engine* e = c.e;
    const Route& r = c.r;
    const int N = c.N, B = c.B, T = c.T, F = e->F;
    const int64_t E = c.E;
    hipStream_t st = c.st;
    if (c.chained_in) {                             // planned by the previous step's last launch (k_finish_plan), PlanFold duties included
        if (c.training) e->bn0_dirty_host = 1;
        return 0;
    }
    const bool graph_plan = r.plan == Plan::Graph256 || r.plan == Plan::Graph1024;
    const bool fold = e->fold_zero && graph_plan && c.training && c.want_grad && !e->bn0_dirty_host && g_stop_after == 0;
    if (c.training) e->bn0_dirty_host = 1;          // (cleared where k_finish is enqueued)
    if (!fold) {
        const int64_t ni = r.plan != Plan::Node ? 0 : 4 * ((int64_t)N + 1);
        hipLaunchKernelGGL(k_zero_f64, dim3(cdiv(std::max<int64_t>(e->arena_n, ni), 256) + (c.draw_perm ? cdiv(B, ZP_EPB) : 0)), dim3(256), 0, st,
                           e->arena, (int64_t)e->arena_n, e->work, ni, e->status, (e->K > 0 && c.training) ? e->gat_ctr : nullptr,
                           c.draw_perm ? e->perm_dev : nullptr, B, e->perm_seed, e->perm_ctr, c.adam_in_finish ? e->step : nullptr,
                           c.training ? e->status + 3 : nullptr);
        CAL_CHECK_LAUNCH("k_zero_f64"); STAGE();
    }
    if (graph_plan) {
        const bool wide = r.plan == Plan::Graph1024;
        auto kern = wide ? k_plan_graph<GP_T2, GP_E2, 1024> : k_plan_graph<GP_T, GP_E, 256>;
        const int nt = wide ? 1024 : 256;
        PlanFold pf;
        memset(&pf, 0, sizeof(pf));
        if (fold) {
            const int wp0 = (e->bn[0].width + 3) / 4 * 4;
            pf.on = 1; pf.arena = e->arena; pf.n = e->arena_n; pf.skip_lo = e->bn[0].arena; pf.skip_hi = e->bn[0].arena + 2 * wp0;
            pf.gat_tick = e->K > 0 ? e->gat_ctr : nullptr; pf.adam_step = c.adam_in_finish ? e->step : nullptr;
            pf.perm = c.draw_perm ? e->perm_dev : nullptr; pf.permB = B; pf.seed = e->perm_seed; pf.perm_ctr = e->perm_ctr;
            pf.dirty = e->status + 3;
        }
        hipLaunchKernelGGL(kern, dim3(T + ((fold && c.draw_perm) ? cdiv(B, nt / 4) : 0)), dim3(nt), 0, st, edge_index, E, N, T, e->node_ptr, e->edge_ptr,
                           c.batch, e->ntiles > 0 ? e->tile_gptr : nullptr, B, e->loop_w,
                           e->rowptr_dst, e->nbr_dst, e->eid_dst, e->rowptr_src, e->nbr_src, e->eid_src, e->row32, e->col32,
                           e->gptr, e->eptr, e->dis_unit, e->status, r.plan_stats ? x0 : nullptr, F, bn_stsum(c, 0), bn_stsq(c, 0),
                           r.plan_coef ? e->coef : nullptr, r.plan_coef ? e->coef_src : nullptr, pf);
        CAL_CHECK_LAUNCH("k_plan_graph"); STAGE();
    } else if (r.plan == Plan::Big) {
        int* scratch = e->work + 4 * ((size_t)e->capN + 1);
        hipLaunchKernelGGL(k_plan_big, dim3(B, 2), dim3(1024), 0, st, edge_index, E, N, B, e->node_ptr, e->edge_ptr, c.batch, e->loop_w,
                           e->rowptr_dst, e->rowptr_src, e->row32, e->col32, e->gptr, e->eptr, e->dis_unit, e->status, scratch,
                           r.plan_stats ? x0 : nullptr, F, bn_stsum(c, 0), bn_stsq(c, 0));
        CAL_CHECK_LAUNCH("k_plan_big"); STAGE();
        RC(plan_rank(E, N, e->rowptr_dst, e->nbr_dst, e->eid_dst, e->rowptr_src, e->nbr_src, e->eid_src, e->row32, e->col32, scratch, st)); STAGE();
    } else {
        RC(plan_build(edge_index, E, N, e->rowptr_dst, e->nbr_dst, e->eid_dst, e->rowptr_src, e->nbr_src, e->eid_src,
                      e->row32, e->col32, e->work, e->status, true, st)); STAGE();
        hipLaunchKernelGGL(k_gptr_dis, dim3(cdiv(N + 1, 256)), dim3(256), 0, st, c.batch, N, B, e->gptr, e->rowptr_src, e->loop_w,
                           e->dis_unit, e->status, e->rowptr_dst, e->eptr);
        CAL_CHECK_LAUNCH("k_gptr_dis"); STAGE();
    }
    return 0;
}

// 2. bn_feat statistics (model.py:90), unless they rode in the plan kernel; 3. h0 = relu(BN(x0) @ W_feat) (model.py:90-91, gcn_conv.py:75-77)
int fwd_feat(Ctx& c, const float* x0) {
    Engine* e = c.e;
    const int N = c.N, H = e->H, F = e->F, L = e->L;
    hipStream_t st = c.st;
    if (c.training && !c.r.plan_stats) {
        // wide feature matrices (one-hot degrees: F = 139 at the NCI1-like shape): many short blocks whose column sums go to
        // partial rows (k_stats_final) -- F fp64 atomics per block on the same 2 F addresses cost more than the reads
        int tc = std::min(256, pow2ceil(F));
        const bool wide = (size_t)cdiv(N, 32) * F > 16384;
        int rpb = wide ? std::max(32, cdiv(N, 1024)) : std::max(128, cdiv(N, 256));
        const Acc a0 = wide ? spmm_acc(c, bn_stsum(c, 0), F, rpb) : Acc(bn_stsum(c, 0));
        const Acc a1 = wide ? spmm_acc(c, bn_stsq(c, 0), F, rpb) : Acc(bn_stsq(c, 0));
        hipLaunchKernelGGL(k_colstats, dim3(cdiv(N, rpb)), dim3(256), 0, st, x0, N, F, tc, rpb, a0, a1);
        CAL_CHECK_LAUNCH("k_colstats"); STAGE();
        if (wide) { RC(flush_finals(c)); STAGE(); }
    }
    if (c.r.feat_fwd == FeatFwd::Rows) {
        FeatFwdArgs fw;
        fw.x0 = x0; fw.W = e->P + e->o_feat_w; fw.out = e->h; fw.bn0 = bnref(c, 0, N, 1);
        if (c.training && L > 0 && !e->gin) { fw.st_sum = node_acc(c, bn_stsum(c, 1), H); fw.st_sq = node_acc(c, bn_stsq(c, 1), H); }
        RC(with_g_fp(H, F, [&](auto g, auto fp) {
            hipLaunchKernelGGL((k_feat_fwd_rows<decltype(g)::value, decltype(fp)::value>), dim3(cdiv(N, c.rpb_n)), dim3(256), 0, st, fw, N, H, F, c.rpb_n);
            return 0;
        }));
        CAL_CHECK_LAUNCH("k_feat_fwd_rows"); STAGE();
    } else {
        GemmArgs a = gemm_args(N, H, F, false, false, 1);
        a.p[0].A = x0; a.p[0].B = e->P + e->o_feat_w; a.p[0].C = e->h;
        a.p[0].xa.has_bn = 1; a.p[0].xa.bn = bnref(c, 0, N, 1);
        // (a GIN layer starts with the aggregation, not a BatchNorm)
        if (c.training && L > 0 && !e->gin) gemm_stats(c, a.p[0], N, H, bn_stsum(c, 1), bn_stsq(c, 1), false, F, c.r.st_feat);
        RC(fwd_gemm(c, false, a, 1)); STAGE();
    }
    RC(flush_finals(c)); STAGE();
    return 0;
}

// GCNConv forward per graph, k_gconv_fwd / k_gw_fwd: one backbone layer (nb = 1) or the two causal convolutions with the add-pool
// (nb = 2; tiles: packed batch) -- kind: Graph64 / Graph128 / Wide, cols: the wide kernels' slice width
void launch_gconv_fwd(Ctx& c, int nb, Conv kind, int cols, bool tiles, const GconvBranch2& b2) {
    Engine* e = c.e;
    const int H = e->H;
    const bool wide = kind == Conv::Wide, g64 = kind == Conv::Graph64;
    auto kern = nb == 1 ? (wide ? (cols == 32 ? k_gw_fwd<false, 32> : k_gw_fwd<false, 64>) : g64 ? k_gconv_fwd<false, 64, 512> : k_gconv_fwd<false, GC_T>)
              : tiles ? k_gconv_fwd<true, 64, 512, true> : g64 ? k_gconv_fwd<true, 64, 512> : !wide ? k_gconv_fwd<true, GC_T>
              : cols == 32 ? k_gw_fwd<true, 32> : k_gw_fwd<true, 64>;
    const int ncol = wide ? cols : GC_N, nt = wide ? GW_NT : tiles || g64 ? 512 : 256;      // (a packed batch runs the 64-node form)
    prof_launch(kern, dim3(c.T, H / ncol, nb), dim3(nt), c.st, csr_dst(c), e->gptr, e->eptr, b2, 1, e->loop_w, H, H, e->status);
}

// 4. backbone: h_i = relu(A_hat (BN_i(h_{i-1}) @ W_i) + b_i)   (model.py:93-95)
int fwd_backbone(Ctx& c) {
    Engine* e = c.e;
    const Route& r = c.r;
    const int N = c.N, T = c.T, H = e->H, L = e->L;
    const int64_t E = c.E;
    hipStream_t st = c.st;
    const size_t NH = (size_t)N * H;
    const CSR gd = csr_dst(c);
    for (int i = 1; i <= L; ++i) {
        const float* hin = e->h + (size_t)(i - 1) * NH;
        float* hout = e->h + (size_t)i * NH;
        if (e->gin && r.bb_fwd == Conv::Graph64) {
            // GINConv per graph (engine_ggin.hpp): (A + I)(h W1^T) + b1 with the BatchNorm statistics | BN, ReLU, Linear, ReLU
            float* t1 = e->gt1 + (size_t)(i - 1) * NH;
            GginFwdArgs ga;
            memset(&ga, 0, sizeof(ga));
            ga.x = hin; ga.W = e->P + e->o_conv_w[i - 1]; ga.bias = e->P + e->o_conv_b[i - 1]; ga.out = t1;
            if (c.training) { ga.st_sum = graph_acc(c, bn_stsum(c, i), H, r.st_bb); ga.st_sq = graph_acc(c, bn_stsq(c, i), H, r.st_bb); }
            {
                ProfScope ps(st, 9, 2.0 * N * H * H + 2.0 * (double)(E + N) * H, true);
                prof_launch(k_ggin_fwd<1>, dim3(T, H / GC_N), dim3(512), st, gd, e->gptr, e->eptr, ga, H, H, e->status);
            }
            CAL_CHECK_LAUNCH("k_ggin_fwd<1>"); STAGE();
            RC(flush_finals(c)); STAGE();
            memset(&ga, 0, sizeof(ga));
            ga.x = t1; ga.W = e->P + e->o_gin_w2[i - 1]; ga.bias = e->P + e->o_gin_b2[i - 1]; ga.out = hout;
            ga.bn = bnref(c, i, N, 1);
            hipLaunchKernelGGL((k_ggin_fwd<2>), dim3(T, H / GC_N), dim3(512), 0, st, gd, e->gptr, e->eptr, ga, H, H, e->status);
            CAL_CHECK_LAUNCH("k_ggin_fwd<2>"); STAGE();
        } else if (e->gin) {    // GINConv: unit-coefficient aggregation -> Linear -> BN -> ReLU -> Linear -> ReLU (model.py:188-194)
            float* agg = e->gagg + (size_t)(i - 1) * NH;
            float* t1 = e->gt1 + (size_t)(i - 1) * NH;
            float* yy = e->gy + (size_t)(i - 1) * NH;
            {
                SpmmBranch br{hin, agg, nullptr, nullptr, e->ones, Acc(), Acc(), nullptr, nullptr, nullptr};
                RC(launch_espmm(st, gd, SpmmBranch2{{br, br}}, 1, 0, 1.0f, N, H, spmm_rpb(H, false)));
                CAL_CHECK_LAUNCH("k_espmm(gin)"); STAGE();
            }
            {
                GemmArgs a = gemm_args(N, H, H, false, true, 0);
                a.p[0].A = agg; a.p[0].B = e->P + e->o_conv_w[i - 1]; a.p[0].bias = e->P + e->o_conv_b[i - 1]; a.p[0].C = t1;
                if (c.training) gemm_stats(c, a.p[0], N, H, bn_stsum(c, i), bn_stsq(c, i), false, H);
                RC(fwd_gemm(c, true, a, 1)); STAGE();
                RC(flush_finals(c)); STAGE();
            }
            {
                GinRowArgs ga;
                memset(&ga, 0, sizeof(ga));
                ga.a = t1; ga.out = yy; ga.bn = bnref(c, i, N, 1);
                RC(gin_rows(c, 0, ga));
                CAL_CHECK_LAUNCH("k_gin_bn_relu"); STAGE();
            }
            {
                GemmArgs a = gemm_args(N, H, H, false, true, 1);
                a.p[0].A = yy; a.p[0].B = e->P + e->o_gin_w2[i - 1]; a.p[0].bias = e->P + e->o_gin_b2[i - 1]; a.p[0].C = hout;
                RC(fwd_gemm(c, true, a, 1)); STAGE();
            }
        } else if (e->K > 0) {  // z = BN_i(h) W_i; attention scores, edge softmax (+dropout), aggregation, bias, ReLU (GATConv)
            const int K = e->K, D = H / K;
            float* zi = e->gz + (size_t)(i - 1) * NH;
            const size_t nk = al((size_t)e->capN * K);
            float* sc = e->gsc + (size_t)(i - 1) * 4 * nk;
            if (r.bb_fwd == Conv::Graph64) {      // the whole layer per graph (engine_ggat.hpp)
                GgatArgs ga;
                memset(&ga, 0, sizeof(ga));
                ga.x = hin; ga.W = e->P + e->o_conv_w[i - 1]; ga.bias = e->P + e->o_conv_b[i - 1];
                ga.att = e->P + e->o_conv_att[i - 1]; ga.bn = bnref(c, i, N, 1); ga.out = hout; ga.z = zi;
                ga.adst = sc; ga.asrc = sc + nk; ga.mx = sc + 2 * nk; ga.den = sc + 3 * nk;
                if (c.training && i < L) { ga.st_sum = graph_acc(c, bn_stsum(c, i + 1), H, r.st_bb); ga.st_sq = graph_acc(c, bn_stsq(c, i + 1), H, r.st_bb); }
                ga.heads = K; ga.D = D; ga.slope = e->gat_slope; ga.p = c.training ? e->gat_p : 0.f;
                ga.seed = e->gat_seed[i - 1]; ga.ctr = (const uint64_t*)e->gat_ctr; ga.E = E;
                {
                    ProfScope ps(st, 7, 2.0 * N * H * H + 2.0 * (double)(E + N) * H, true);
                    prof_launch(k_ggat_fwd, dim3(T, H / GC_N), dim3(256), st, gd, e->gptr, e->eptr, ga, H, H, e->status);
                }
                CAL_CHECK_LAUNCH("k_ggat_fwd"); STAGE();
                RC(flush_finals(c)); STAGE();
                continue;
            }
            GemmArgs a = gemm_args(N, H, H, false, false, 0);
            a.p[0].A = hin; a.p[0].B = e->P + e->o_conv_w[i - 1]; a.p[0].C = zi;
            a.p[0].xa.has_bn = 1; a.p[0].xa.bn = bnref(c, i, N, 1);
            { ProfScope ps(st, 0, 2.0 * N * H * H); RC(fwd_gemm(c, false, a, 1)); } STAGE();
            {
                ProfScope ps(st, 5, 2.0 * N * H * 4 + (double)(E + N) * (8 + 12.0 * K) + (N + 1) * 4.0);
                RC(gat_forward(e->rowptr_dst, e->nbr_dst, e->eid_dst, zi, e->P + e->o_conv_att[i - 1], e->P + e->o_conv_b[i - 1], 1,
                               e->gat_slope, c.training ? e->gat_p : 0.f, e->gat_seed[i - 1], (const uint64_t*)e->gat_ctr, hout,
                               sc, sc + nk, sc + 2 * nk, sc + 3 * nk, N, E, K, D, st));
            }
            STAGE();
            if (c.training && i < L) {
                int tc = std::min(256, pow2ceil(H));
                int rpb = std::max(32, cdiv(N, 1024));
                if (H == 256 && aligned16(hout))
                    hipLaunchKernelGGL(k_colstats4, dim3(cdiv(N, rpb)), dim3(256), 0, st, hout, N, rpb, Acc(bn_stsum(c, i + 1)), Acc(bn_stsq(c, i + 1)));
                else
                    hipLaunchKernelGGL(k_colstats, dim3(cdiv(N, rpb)), dim3(256), 0, st, hout, N, H, tc, rpb, Acc(bn_stsum(c, i + 1)), Acc(bn_stsq(c, i + 1)));
                CAL_CHECK_LAUNCH("k_colstats"); STAGE();
            }
        } else if (r.bb_fwd != Conv::Node) {
            // GCNConv per graph: MFMA product + aggregation + statistics in one kernel (engine_gconv.hpp); graphs of up to 256 nodes:
            // the sparse aggregation from LDS (engine_gwide.hpp).  The first layer writes the unit coefficients in slot order
            // unless k_plan_graph has.
            GconvBranch gb;
            memset(&gb, 0, sizeof(gb));
            gb.x = hin; gb.W = e->P + e->o_conv_w[i - 1]; gb.bias = e->P + e->o_conv_b[i - 1];
            gb.dis = e->dis_unit; gb.bn = bnref(c, i, N, 1); gb.out = hout;
            if (i == 1 && !r.plan_coef) gb.coef_out = e->coef; else gb.coef_in = e->coef;
            if (c.training && i < L) { gb.st_sum = graph_acc(c, bn_stsum(c, i + 1), H, r.st_bb); gb.st_sq = graph_acc(c, bn_stsq(c, i + 1), H, r.st_bb); }
            const GconvBranch2 b2{{gb, gb}};
            if (i == L && r.att_fwd_fold) {
                // the attention forward (fwd_att's per-graph kernel) as this launch's tail: k_gconv_fwd_att in gconv_fwd_att.hip, a code
                // object of its own
                AttFwdFoldArgs fa;
                memset(&fa, 0, sizeof(fa));
                fa.gs = csr_src(c);
                fa.Wn = e->P + e->o_natt_w; fa.bn = e->P + e->o_natt_b; fa.We = e->P + e->o_eatt_w; fa.be = e->P + e->o_eatt_b;
                fa.anode = e->anode; fa.pq = e->pq; fa.att = e->att; fa.dis_c = e->dis_co; fa.dis_o = e->dis_co + N;
                fa.stc_sum = graph_acc(c, bn_stsum(c, L + 1), H, true); fa.stc_sq = graph_acc(c, bn_stsq(c, L + 1), H, true);
                fa.sto_sum = graph_acc(c, bn_stsum(c, L + 2), H, true); fa.sto_sq = graph_acc(c, bn_stsq(c, L + 2), H, true);
                fa.E = E; fa.fnode = e->no_node_att ? 0.f : 1.f; fa.fedge = e->no_edge_att ? 0.f : 1.f;
                fa.xch = e->att_xch; fa.flags = (int*)(e->arena + e->a_aff);
                {
                    ProfScope ps(st, 2, 2.0 * N * H * H + 2.0 * (double)(E + N) * H, true);
                    RC(side_launch(cal_launch_gconv_fwd_att, "k_gconv_fwd_att", "gconv_fwd_att.hip", dim3(T, 2), st, &gd, sizeof(gd), e->gptr, e->eptr,
                                   &b2, sizeof(b2), 1, e->loop_w, H, H, e->status, &fa, sizeof(fa)));
                }
                CAL_CHECK_LAUNCH("k_gconv_fwd_att"); STAGE();
                RC(flush_finals(c)); STAGE();
                continue;
            }
            {
                ProfScope ps(st, 2, 2.0 * N * H * H + 2.0 * (double)(E + N) * H, true);
                launch_gconv_fwd(c, 1, r.bb_fwd, r.gw_cols_bb, false, b2);
            }
            CAL_CHECK_LAUNCH(r.bb_fwd == Conv::Wide ? "k_gw_fwd" : "k_gconv_fwd"); STAGE();
            RC(flush_finals(c)); STAGE();
        } else {
            GemmArgs a = gemm_args(N, H, H, false, false, 0);
            a.p[0].A = hin; a.p[0].B = e->P + e->o_conv_w[i - 1]; a.p[0].C = e->z;
            a.p[0].xa.has_bn = 1; a.p[0].xa.bn = bnref(c, i, N, 1);
            { ProfScope ps(st, 0, 2.0 * N * H * H); RC(fwd_gemm(c, false, a, 1)); } STAGE();
            SpmmBranch br{e->z, hout, e->P + e->o_conv_b[i - 1], nullptr, e->dis_unit, Acc(), Acc(), nullptr, nullptr, nullptr};
            const bool wst = c.training && i < L;
            const int rpb = spmm_rpb(H, wst, N);
            if (wst) { br.st_sum = spmm_acc(c, bn_stsum(c, i + 1), H, rpb); br.st_sq = spmm_acc(c, bn_stsq(c, i + 1), H, rpb); }
            {
                ProfScope ps(st, 1, 2.0 * N * H * 4 + (double)(E + N) * 8 + (N + 1) * 4.0, true);
                RC(launch_espmm(st, gd, SpmmBranch2{{br, br}}, 1, 1, e->loop_w, N, H, rpb));
            }
            CAL_CHECK_LAUNCH("k_espmm"); STAGE();
            RC(flush_finals(c)); STAGE();
        }
    }
    return 0;
}

// 5+6. node attention, edge projections, bnc / bno statistics, edge softmax + weighted degrees (model.py:97-111, gcn_conv.py:63-68)
int fwd_att(Ctx& c) {
    Engine* e = c.e;
    const Route& r = c.r;
    const int N = c.N, H = e->H, L = e->L;
    const int64_t E = c.E;
    hipStream_t st = c.st;
    const float* x = e->h + (size_t)L * N * H;
    const CSR gs = csr_src(c);
    if (r.att_fwd_fold) return 0;         // done by the last backbone layer's launch (fwd_backbone: k_gconv_fwd_att)
    if (r.att_fwd != Att::Node) {
        // per graph: all of it in one kernel (4 rows per lane group); graphs of 129-256 nodes: the same kernel in four row passes,
        // four slots per lane (engine_attwide.hpp)
        // (only when the launch has enough workgroups -- 32 graphs on 256 CUs lose to the node-parallel pair, 19.3 vs 12.6 us;
        //  128 graphs win, 20.5 vs 24.0 us with their finishing launch.  The backward per graph wins at both: 22.8 vs 28.1, 30.8 vs 47.7 us)
        const bool wide = r.att_fwd == Att::Wide;
        const Acc a0 = graph_acc(c, bn_stsum(c, L + 1), H, r.st_co), a1 = graph_acc(c, bn_stsq(c, L + 1), H, r.st_co);
        const Acc a2 = graph_acc(c, bn_stsum(c, L + 2), H, r.st_co), a3 = graph_acc(c, bn_stsq(c, L + 2), H, r.st_co);
        auto launch = [&](auto kernel_of) {
            return with_g(H, [&](auto g) {
                hipLaunchKernelGGL(kernel_of(g), dim3(c.T), dim3(512), 0, st, e->gptr, gs, x, e->P + e->o_natt_w, e->P + e->o_natt_b,
                                   e->P + e->o_eatt_w, e->P + e->o_eatt_b, e->anode, e->pq, e->att, e->dis_co, e->dis_co + N, a0, a1, a2, a3,
                                   e->loop_w, H, E, e->status, e->no_node_att ? 0.f : 1.f, e->no_edge_att ? 0.f : 1.f, e->eptr);
                return 0;
            });
        };
        if (wide) RC(launch([](auto g) { return k_att_fwd_wide<4, decltype(g)::value>; }));
        else RC(launch([](auto g) { return k_att_fwd_graph<4, decltype(g)::value>; }));
        CAL_CHECK_LAUNCH(wide ? "k_att_fwd_wide" : "k_att_fwd_graph"); STAGE();
        RC(flush_finals(c)); STAGE();
        return 0;
    }
    const Acc a0 = node_acc(c, bn_stsum(c, L + 1), H), a1 = node_acc(c, bn_stsq(c, L + 1), H);
    const Acc a2 = node_acc(c, bn_stsum(c, L + 2), H), a3 = node_acc(c, bn_stsq(c, L + 2), H);
    RC(with_g(H, [&](auto g) {
        constexpr int G = decltype(g)::value;
        hipLaunchKernelGGL((k_node_att_fwd<4, G>), dim3(cdiv(N, c.rpb_n)), dim3(256), 0, st, x, e->P + e->o_natt_w,
                           e->P + e->o_natt_b, e->P + e->o_eatt_w, e->anode, e->pq, a0, a1, a2, a3, N, H, c.rpb_n, e->no_node_att ? 0.f : 1.f);
        return 0;
    }));
    CAL_CHECK_LAUNCH("k_node_att_fwd"); STAGE();
    RC(flush_finals(c)); STAGE();
    hipLaunchKernelGGL(k_edge_att_deg, dim3(cdiv(N, 32)), dim3(256), 0, st, gs, e->pq, e->P + e->o_eatt_b, e->att, e->dis_co,
                       e->dis_co + N, e->loop_w, N, E, e->no_edge_att ? 0.f : 1.f);
    CAL_CHECK_LAUNCH("k_edge_att_deg"); STAGE();
    return 0;
}

// 7-9. z_k = BN_k(a_k * x) @ W_k, h_k = relu(A_hat_k z_k + b_k) for k in (context, objects), add-pool (model.py:112-116)
int fwd_co(Ctx& c) {
    Engine* e = c.e;
    const Route& r = c.r;
    const int N = c.N, B = c.B, H = e->H, L = e->L;
    const int64_t E = c.E;
    hipStream_t st = c.st;
    const size_t NH = (size_t)N * H;
    const float* x = e->h + (size_t)L * NH;
    const CSR gd = csr_dst(c);
    if (r.co_fwd != Conv::Node) {      // both weighted convolutions and the add-pool in one per-graph launch
        const bool wide = r.co_fwd == Conv::Wide;
        const int64_t* tgp = e->ntiles > 0 ? e->tile_gptr : nullptr;
        GconvBranch gb[2];
        memset(gb, 0, sizeof(gb));
        for (int k = 0; k < 2; ++k) {
            gb[k].x = x; gb[k].W = e->P + (k ? e->o_ow : e->o_cw); gb[k].bias = e->P + (k ? e->o_ob : e->o_cb);
            gb[k].ew = e->att + (size_t)k * E; gb[k].dis = e->dis_co + (size_t)k * N;
            gb[k].rs = e->anode + k; gb[k].rs_stride = 2; gb[k].bn = bnref(c, L + 1 + k, N, 1);
            gb[k].out = e->hco + (size_t)k * NH; gb[k].z = e->zco + (size_t)k * NH; gb[k].pooled = e->pooled + (size_t)k * B * H;
            if (wide) continue;
            gb[k].coef_out = e->coef + (size_t)(1 + k) * E;
            gb[k].w_out = e->wslot + (size_t)k * E;
            gb[k].batch = c.batch; gb[k].tile_gptr = tgp;          // packed batch: the add-pool is per GRAPH inside the tile
        }
        const GconvBranch2 b2{{gb[0], gb[1]}};
        launch_gconv_fwd(c, 2, r.co_fwd, r.gw_cols_co, tgp != nullptr, b2);
        CAL_CHECK_LAUNCH(wide ? "k_gw_fwd(co)" : "k_gconv_fwd(co)"); STAGE();
        return 0;
    }
    GemmArgs a = gemm_args(N, H, H, false, false, 0);
    for (int k = 0; k < 2; ++k) {
        a.p[k].A = x; a.p[k].B = e->P + (k ? e->o_ow : e->o_cw); a.p[k].C = e->zco + (size_t)k * NH;
        a.p[k].xa.rs = e->anode + k; a.p[k].xa.rs_stride = 2;
        a.p[k].xa.has_bn = 1; a.p[k].xa.bn = bnref(c, L + 1 + k, N, 1);
    }
    RC(fwd_gemm(c, false, a, 2)); STAGE();
    SpmmBranch b0{e->zco, e->hco, e->P + e->o_cb, e->att, e->dis_co, Acc(), Acc(), nullptr, nullptr, nullptr};
    SpmmBranch b1{e->zco + NH, e->hco + NH, e->P + e->o_ob, e->att + E, e->dis_co + N, Acc(), Acc(), nullptr, nullptr, nullptr};
    RC(launch_espmm(st, gd, SpmmBranch2{{b0, b1}}, 2, 1, e->loop_w, N, H, spmm_rpb(H, false)));
    CAL_CHECK_LAUNCH("k_espmm(co)"); STAGE();
    RC(launch_pool2(c)); STAGE();
    return 0;
}

// 10. readouts (model.py:125-164)
int fwd_readout(Ctx& c) {
    Engine* e = c.e;
    const int B = c.B, H = e->H, C = e->C, L = e->L;
    hipStream_t st = c.st;
    if (c.r.ro == Readout::OneLaunch || c.r.ro == Readout::Rows) {
        // the whole readout, forward and backward, in one launch (engine_ro_step.hpp); 128 < B <= 512: in row blocks of 128 graphs
        // (k_ro_step<true>): the sums over all rows are exchanged between the row blocks inside the kernel, the weight gradients
        // leave as one slab per row block (front of the slab workspace; engine_backward registers them with k_finish)
        RoStepArgs sa;
        memset(&sa, 0, sizeof(sa));
        sa.a = make_ro(c); sa.zpart = e->zpart; sa.sync = reinterpret_cast<int*>(e->arena + e->a_sync); sa.status = e->status;
        if (c.r.ro == Readout::OneLaunch) {
            hipLaunchKernelGGL(k_ro_step<false>, dim3(3, H / RO_CW), dim3(256), 0, st, sa);
        } else {
            const int nrb = cdiv(B, RS_B), nch = H / RO_CW;
            sa.nrb = nrb;
            sa.xch = parts_alloc(c, (size_t)3 * nch * RBK_XCH);
            if (!sa.xch) return no_parts();
            const RoSlabs rs = ro_slabs(H, C, B);
            sa.gw1_slab = e->slabs + rs.w1(0); sa.gw2_slab = e->slabs + rs.w2(0);
            hipLaunchKernelGGL(k_ro_step<true>, dim3(3, nch, nrb), dim3(256), 0, st, sa);
        }
        CAL_CHECK_LAUNCH("k_ro_step"); STAGE();
        return 0;
    }
    if (c.r.ro == Readout::FourKernel) {
        const RoArgs ra = make_ro(c);
        hipLaunchKernelGGL(k_ro_fwd_a, dim3(3, H / RO_CW), dim3(256), 0, st, ra);
        CAL_CHECK_LAUNCH("k_ro_fwd_a"); STAGE();
        hipLaunchKernelGGL(k_ro_fwd_b, dim3(3, cdiv(B, RO_RB)), dim3(256), 0, st, ra);
        CAL_CHECK_LAUNCH("k_ro_fwd_b"); STAGE();
        if (!c.want_grad) {                  // no backward to finish the loss sums
            hipLaunchKernelGGL(k_ro_loss, dim3(3), dim3(256), 0, st, ra);
            CAL_CHECK_LAUNCH("k_ro_loss");
        }
        return 0;
    }
    const int bn_fc1 = L + 3, bn_fc2 = L + 4;   // + 2*head
    {
        int tc = std::min(256, pow2ceil(H));
        hipLaunchKernelGGL(k_readout_prep, dim3(cdiv(B, c.rpb_b)), dim3(256), 0, st, e->pooled, c.perm, e->iperm, e->xco, B, H, tc,
                           c.rpb_b, bn_stsum(c, bn_fc1), bn_stsq(c, bn_fc1), bn_stsum(c, bn_fc1 + 2), bn_stsq(c, bn_fc1 + 2),
                           bn_stsum(c, bn_fc1 + 4), bn_stsq(c, bn_fc1 + 4), e->cat);
        CAL_CHECK_LAUNCH("k_readout_prep"); STAGE();
    }
    const float* xin[3] = {e->pooled, e->pooled + (size_t)B * H, e->xco};
    const int Wco = e->cat ? 2 * H : H;                 // input width of the co head
    {
        // fc1 of the three heads: one batched launch, or (cat: the co head reduces over 2H) heads c / o batched + co alone
        auto fc1 = [&](int hd0, int nh, int Kin) -> int {
            GemmArgs a = gemm_args(B, H, Kin, false, true, 1);
            for (int q = 0; q < nh; ++q) {
                const int hd = hd0 + q;
                a.p[q].A = xin[hd]; a.p[q].B = e->P + e->o_fc1_w[hd]; a.p[q].bias = e->P + e->o_fc1_b[hd];
                a.p[q].C = e->y1 + (size_t)hd * B * H;
                a.p[q].xa.has_bn = 1; a.p[q].xa.bn = bnref(c, bn_fc1 + 2 * hd, B, 1);
                if (c.training) gemm_stats(c, a.p[q], B, H, bn_stsum(c, bn_fc2 + 2 * hd), bn_stsq(c, bn_fc2 + 2 * hd), false);
            }
            return fwd_gemm(c, true, a, nh);
        };
        if (e->cat) { RC(fc1(0, 2, H)); STAGE(); RC(fc1(2, 1, Wco)); STAGE(); }
        else { RC(fc1(0, 3, H)); STAGE(); }
        RC(flush_finals(c)); STAGE();
    }
    {
        GemmArgs a = gemm_args(B, C, H, false, true, 0);
        for (int hd = 0; hd < 3; ++hd) {
            a.p[hd].A = e->y1 + (size_t)hd * B * H; a.p[hd].B = e->P + e->o_fc2_w[hd]; a.p[hd].bias = e->P + e->o_fc2_b[hd];
            a.p[hd].C = e->zl + (size_t)hd * B * C;
            a.p[hd].xa.has_bn = 1; a.p[hd].xa.bn = bnref(c, bn_fc2 + 2 * hd, B, 1);
        }
        RC(fwd_gemm(c, true, a, 3)); STAGE();
    }
    if (B > 256) hipLaunchKernelGGL(k_loss<1024>, dim3(1), dim3(1024), 0, st, e->zl, c.y, e->logp, e->dzl, e->stats, e->arena + e->a_db2, B, C, c.wc, c.wo,
                                    c.wco, c.want_grad);
    else hipLaunchKernelGGL(k_loss<256>, dim3(1), dim3(256), 0, st, e->zl, c.y, e->logp, e->dzl, e->stats, e->arena + e->a_db2, B, C, c.wc, c.wo,
                            c.wco, c.want_grad);
    CAL_CHECK_LAUNCH("k_loss"); STAGE();
    return 0;
}

int engine_forward(Ctx& c, const float* x0, const int64_t* edge_index) {
    RC(fwd_plan(c, x0, edge_index));
    RC(fwd_feat(c, x0));
    RC(fwd_backbone(c));
    RC(fwd_att(c));
    RC(fwd_co(c));
    return fwd_readout(c);
}

// R. readout backward: nothing after the one-launch readout, the slabs of the row-blocked one, k_ro_bwd_a / _b, or the GEMM chain
int bwd_readout(Ctx& c, Bwd& b) {
    Engine* e = c.e;
    const int B = c.B, H = e->H, C = e->C, L = e->L;
    const size_t BH = (size_t)B * H;
    hipStream_t st = c.st;
    FinishArgs& fa = b.fa;
    if (c.r.ro == Readout::Rows) {                     // the row-blocked readout left one weight-gradient slab per row block
        const RoSlabs rs = ro_slabs(H, C, B);
        for (int hd = 0; hd < 3; ++hd) {
            RCP(b.slabs_at(c, rs.w1(hd), (int)rs.nrb, H * H, e->G + e->o_fc1_w[hd]));
            RCP(b.slabs_at(c, rs.w2(hd), (int)rs.nrb, C * H, e->G + e->o_fc2_w[hd]));
        }
    }
    if (c.r.ro != Readout::Gemm) {
        if (c.r.ro == Readout::FourKernel) {
            const RoArgs ra = make_ro(c);
            hipLaunchKernelGGL(k_ro_bwd_a, dim3(3, H / RO_CW), dim3(256), 0, st, ra);
            CAL_CHECK_LAUNCH("k_ro_bwd_a"); STAGE();
            hipLaunchKernelGGL(k_ro_bwd_b, dim3(3, H / RO_CW), dim3(256), 0, st, ra);
            CAL_CHECK_LAUNCH("k_ro_bwd_b"); STAGE();
        }
        fa.stats = e->stats; fa.wc = c.wc; fa.wo = c.wo; fa.wco = c.wco;
        return 0;
    }
    const int bn_fc1 = L + 3, bn_fc2 = L + 4;
    const float* xin[3] = {e->pooled, e->pooled + BH, e->xco};
    // R1. dW2_h = dz_h^T @ BN2(y1_h)
    {
        GemmArgs a = gemm_args(C, H, B, true, false, 0);
        float* dst[3];
        for (int hd = 0; hd < 3; ++hd) {
            a.p[hd].A = e->dzl + (size_t)hd * B * C; a.p[hd].B = e->y1 + hd * BH;
            a.p[hd].xb.has_bn = 1; a.p[hd].xb.bn = bnref(c, bn_fc2 + 2 * hd, B, 0);
            dst[hd] = e->G + e->o_fc2_w[hd];
        }
        RC(grad_gemm(c, b, a, 3, dst)); STAGE();
    }
    // R2. d(BN2 out)_h = dz_h @ W2_h, with the BN2-backward sums
    {
        GemmArgs a = gemm_args(B, H, C, false, false, 0);
        for (int hd = 0; hd < 3; ++hd) {
            a.p[hd].A = e->dzl + (size_t)hd * B * C; a.p[hd].B = e->P + e->o_fc2_w[hd]; a.p[hd].C = e->dyh1 + hd * BH;
            a.p[hd].aux = e->y1 + hd * BH; a.p[hd].has_aux = 1; a.p[hd].aux_bn = bnref(c, bn_fc2 + 2 * hd, B, 0);
            gemm_stats(c, a.p[hd], B, H, bn_dsum(c, bn_fc2 + 2 * hd), bn_dprod(c, bn_fc2 + 2 * hd), true);
        }
        RC(fwd_gemm(c, false, a, 3)); STAGE();
        RC(flush_finals(c)); STAGE();
    }
    // R3. BN2 backward + ReLU mask + fc1 bias gradients
    {
        BnBwdProb p[3];
        for (int hd = 0; hd < 3; ++hd)
            p[hd] = BnBwdProb{e->dyh1 + hd * BH, e->y1 + hd * BH, e->dy1 + hd * BH, bnref(c, bn_fc2 + 2 * hd, B, 0),
                              bn_dsum(c, bn_fc2 + 2 * hd), bn_dprod(c, bn_fc2 + 2 * hd), e->arena + e->a_db1 + hd * H};
        RC(with_g(H, [&](auto g) {
            constexpr int G = decltype(g)::value;
            hipLaunchKernelGGL((k_bn_bwd<4, G>), dim3(cdiv(B, c.rpb_b), 3), dim3(256), 0, st, BnBwdProb3{{p[0], p[1], p[2]}}, 1, B, H, c.rpb_b);
            return 0;
        }));
        CAL_CHECK_LAUNCH("k_bn_bwd(readout)"); STAGE();
    }
    const int Wco = e->cat ? 2 * H : H;                 // input width of the co head (cat: [xc[perm] | xo])
    float* const dxh_hd[3] = {e->dxh, e->dxh + BH, e->dxh + 2 * BH};
    // R4. dW1_h = dy1_h^T @ BN1(xin_h)
    {
        auto r4 = [&](int hd0, int nh, int Kin) -> int {
            GemmArgs a = gemm_args(H, Kin, B, true, false, 0);
            float* dst[3];
            for (int q = 0; q < nh; ++q) {
                const int hd = hd0 + q;
                a.p[q].A = e->dy1 + hd * BH; a.p[q].B = xin[hd];
                a.p[q].xb.has_bn = 1; a.p[q].xb.bn = bnref(c, bn_fc1 + 2 * hd, B, 0);
                dst[q] = e->G + e->o_fc1_w[hd];
            }
            return grad_gemm(c, b, a, nh, dst);
        };
        if (e->cat) { RC(r4(0, 2, H)); STAGE(); RC(r4(2, 1, Wco)); STAGE(); }
        else { RC(r4(0, 3, H)); STAGE(); }
    }
    // R5. d(BN1 out)_h = dy1_h @ W1_h with the BN1-backward sums
    {
        auto r5 = [&](int hd0, int nh, int Kin) -> int {
            GemmArgs a = gemm_args(B, Kin, H, false, false, 0);
            for (int q = 0; q < nh; ++q) {
                const int hd = hd0 + q;
                a.p[q].A = e->dy1 + hd * BH; a.p[q].B = e->P + e->o_fc1_w[hd]; a.p[q].C = dxh_hd[hd];
                a.p[q].aux = xin[hd]; a.p[q].has_aux = 1; a.p[q].aux_bn = bnref(c, bn_fc1 + 2 * hd, B, 0);
                gemm_stats(c, a.p[q], B, Kin, bn_dsum(c, bn_fc1 + 2 * hd), bn_dprod(c, bn_fc1 + 2 * hd), true);
            }
            return fwd_gemm(c, false, a, nh);
        };
        if (e->cat) { RC(r5(0, 2, H)); STAGE(); RC(r5(2, 1, Wco)); STAGE(); }
        else { RC(r5(0, 3, H)); STAGE(); }
        RC(flush_finals(c)); STAGE();
    }
    // R6. BN1 backward + un-permute the random intervention -> d pooled
    BnIn in[3];
    for (int hd = 0; hd < 3; ++hd)
        in[hd] = BnIn{dxh_hd[hd], xin[hd], bnref(c, bn_fc1 + 2 * hd, B, 0), bn_dsum(c, bn_fc1 + 2 * hd), bn_dprod(c, bn_fc1 + 2 * hd)};
    hipLaunchKernelGGL(k_readout_bwd_tail, dim3(cdiv((int64_t)BH, 256)), dim3(256), 0, st, in[0], in[1], in[2], e->iperm, e->dpool, B, H, e->cat);
    CAL_CHECK_LAUNCH("k_readout_bwd_tail"); STAGE();
    return 0;
}

// P2-P4. gradient w.r.t. the edge weights through propagate and through the normalisation
int norm_bwd(Ctx& c, const float* gn2, const float* gself2) {
    Engine* e = c.e;
    const int N = c.N;
    const int64_t E = c.E;
    hipLaunchKernelGGL(k_normbwd_node2, dim3(cdiv(N, 32), 2), dim3(256), 0, c.st, csr_src(c), csr_dst(c), e->att, e->dis_co, e->gn, e->gself,
                       e->ddeg, e->loop_w, N, E, gn2, gself2);
    CAL_CHECK_LAUNCH("k_normbwd_node2"); STAGE();
    if (E > 0) {
        hipLaunchKernelGGL(k_normbwd_edge, dim3(cdiv(E, 256)), dim3(256), 0, c.st, e->row32, e->col32, e->att, e->dis_co, e->gn, e->ddeg,
                           e->dl, N, E, gn2, e->no_edge_att ? 0.f : 1.f);
        CAL_CHECK_LAUNCH("k_normbwd_edge"); STAGE();
    }
    return 0;
}

// P. the causal / trivial convolutions and the add-pool
int bwd_co(Ctx& c, Bwd& b) {
    Engine* e = c.e;
    const Route& r = c.r;
    const int N = c.N, B = c.B, T = c.T, H = e->H, L = e->L;
    const int64_t E = c.E;
    hipStream_t st = c.st;
    const size_t NH = (size_t)N * H;
    const bool ro = r.ro != Readout::Gemm;
    const float* x = e->h + (size_t)L * NH;
    if (r.co_bwd != Conv::Node) {
        // P5-P7 fused per graph: dz_k stays in LDS; dX'_k arrives as one partial per output-column slice
        GconvBwdBranch gb[2];
        memset(gb, 0, sizeof(gb));
        float* dst[2]; double* dsum[2]; double* dprod[2];
        for (int k = 0; k < 2; ++k) {
            gb[k].x = x; gb[k].W = e->P + (k ? e->o_ow : e->o_cw);
            // dOut = relu'(h_k) * (gradient of the graph's pooled row); gn / gself partials per 64-column slice
            gb[k].y = e->hco + (size_t)k * NH; gb[k].z = e->zco + (size_t)k * NH;
            if (ro) { gb[k].gp0 = e->dxh + (size_t)k * B * H; gb[k].gp1 = e->dxh + (size_t)2 * B * H; gb[k].iperm = k == 0 ? e->iperm : nullptr; }
            else gb[k].gp0 = e->dpool + (size_t)k * B * H;
            gb[k].gn = e->gn + (size_t)k * E; gb[k].gself = e->gself + (size_t)k * N;
            gb[k].gn_stride = 2 * (size_t)E; gb[k].gself_stride = 2 * (size_t)N;
            RCP(gb[k].bias_parts = b.defer(c, k ? b.d_ob : b.d_cb, T, H));
            gb[k].ew = e->att + (size_t)k * E; gb[k].dis = e->dis_co + (size_t)k * N;
            gb[k].rs = e->anode + k; gb[k].rs_stride = 2; gb[k].bn = bnref(c, L + 1 + k, N, 0);
            gb[k].dxp0 = e->dXhco + (size_t)k * NH; gb[k].dxp1 = e->dzco + (size_t)k * NH;
            gb[k].coef_in = r.co_bwd == Conv::Wide ? nullptr : e->coef + (size_t)(1 + k) * E;      // (the wide kernels walk the CSR by source: other slot order)
            gb[k].gn_slot = r.att_bwd == Att::Graph ? 1 : 0;        // consumed by k_att_bwd_graph in slot order (else by k_normbwd_* in edge-id order)
            dst[k] = e->G + (k ? e->o_ow : e->o_cw); dsum[k] = bn_dsum(c, L + 1 + k); dprod[k] = bn_dprod(c, L + 1 + k);
        }
        RC(gconv_bwd(c, b, gb, 2, dst, dsum, dprod, r.st_co)); STAGE();
        RC(flush_finals(c)); STAGE();
        // the edge-weight gradients through the normalisation are part of the per-graph attention backward; big batches (a per-graph
        // launch would be several waves of one-per-CU workgroups) keep the node- / edge-parallel kernels
        if (r.att_bwd == Att::Node) {
            const bool two = H > GC_N;
            RC(norm_bwd(c, two ? e->gn + 2 * (size_t)E : nullptr, two ? e->gself + 2 * (size_t)N : nullptr));
        }
        return 0;
    }
    // P1. add-pool backward + ReLU of the causal/trivial convs: d(conv output)[v] = relu'(h_k[v]) * (gradient of the pooled row of v's
    // graph) is never stored -- the transposed aggregation below (P5) builds it per gathered row from the activation, and the bias
    // gradients are count x pooled-row gradient per graph (k_pool2 counted the positive rows).  Rounds 1-3 wrote and re-read the
    // two [N, H] matrices (656 MB and 155 us per step at config 5).
    if (r.co_fwd != Conv::Node) { RC(launch_pool_cnt(c)); STAGE(); }          // the forward pooled inside k_gconv_fwd: no counts yet
    RCP(b.defer(c, b.d_cb, B, H)); RCP(b.defer(c, b.d_ob, B, H));
    // (fused readout: d pooled is still two addends per row -- combined here into dpool, which that path leaves unused)
    hipLaunchKernelGGL(k_pool_bias_grad, dim3(B, 2), dim3(256), 0, st, e->pcnt, ro ? e->dxh : e->dpool, ro ? e->dxh + 2 * (size_t)B * H : nullptr,
                       e->iperm, e->dpool, b.d_cb.p, b.d_ob.p, B, H);
    CAL_CHECK_LAUNCH("k_pool_bias_grad"); STAGE();
    // P5. dz_k = A_hat_k^T dZ_k with the SDDMM riding on it, then P2-P4 on its output.  The transposed aggregation gathers
    // dZ_k[dst] for every out-edge of a source row anyway, so gn_e = <dZ_k[dst_e], z_k[src_e]> costs it one more row (z_k[src]) and a
    // lane-group reduction per slot instead of a second pass over both matrices (the separate SDDMM kernel of rounds 1-3: 265 us per
    // step at config 5).  Input self-loop edges have no slot: their gn entry is never read (k_normbwd_* skip them like the plan does).
    {
        SpmmBranch b0{e->hco, e->dzco, nullptr, e->att, e->dis_co, Acc(), Acc(), nullptr, nullptr, nullptr};
        SpmmBranch b1{e->hco + NH, e->dzco + NH, nullptr, e->att + E, e->dis_co + N, Acc(), Acc(), nullptr, nullptr, nullptr};
        b0.sd_z = e->zco; b0.sd_gn = e->gn; b0.sd_gself = e->gself;
        b1.sd_z = e->zco + NH; b1.sd_gn = e->gn + E; b1.sd_gself = e->gself + N;
        b0.pb_g = e->dpool; b0.pb_batch = c.batch;
        b1.pb_g = e->dpool + (size_t)B * H; b1.pb_batch = c.batch;
        RC(launch_espmm(st, csr_src(c), SpmmBranch2{{b0, b1}}, 2, 0, e->loop_w, N, H, spmm_rpb(H, false)));
        CAL_CHECK_LAUNCH("k_espmm(co,T)"); STAGE();
        RC(norm_bwd(c, nullptr, nullptr));
    }
    // P6. dW_k = BN_k(a_k x)^T @ dz_k and P7. d(BN_k out) = dz_k @ W_k^T with the BN_k-backward sums, one launch
    GemmArgs aw = gemm_args(H, H, N, true, false, 0);
    float* dst[2];
    for (int k = 0; k < 2; ++k) {
        aw.p[k].A = x; aw.p[k].B = e->dzco + (size_t)k * NH;
        aw.p[k].xa.rs = e->anode + k; aw.p[k].xa.rs_stride = 2;
        aw.p[k].xa.has_bn = 1; aw.p[k].xa.bn = bnref(c, L + 1 + k, N, 0);
        dst[k] = e->G + (k ? e->o_ow : e->o_cw);
    }
    GemmArgs a = gemm_args(N, H, H, false, true, 0);
    for (int k = 0; k < 2; ++k) {
        a.p[k].A = e->dzco + (size_t)k * NH; a.p[k].B = e->P + (k ? e->o_ow : e->o_cw); a.p[k].C = e->dXhco + (size_t)k * NH;
        a.p[k].aux = x; a.p[k].aux_rs = e->anode + k; a.p[k].aux_rs_stride = 2; a.p[k].has_aux = 1;
        a.p[k].aux_bn = bnref(c, L + 1 + k, N, 0);
        gemm_stats(c, a.p[k], N, H, bn_dsum(c, L + 1 + k), bn_dprod(c, L + 1 + k), true, H, r.st_node);
    }
    RC(dual_gemm(c, b, a, 2, aw, 2, dst)); STAGE();
    RC(flush_finals(c)); STAGE();
    return 0;
}

// GCNConv layer i's backward per graph (engine_gconv_bwd.hpp), unit coefficients as the forward's first layer wrote them -- or per
// graph of up to 256 nodes (engine_gwide.hpp): CSR by source, the unit coefficients k_plan_graph left in that slot order, if it ran.
// Layer i reads dOut = e->dZ (i == L, written by the attention backward), or builds it while staging: from layer i+1's partial dX'
// (BatchNorm_{i+1}-backward + ReLU mask fused in: no k_bn_bwd launch, no dZ round trip), or (att, i == L) from the attention
// backward itself.  Slice-0 partials ping-pong between dXh and z (idle in the fused forward), slice-1 partials are per layer.
// (one definition of the two per-layer choices for bwd_backbone and bb_gconv_bwd)
float* bb_dxp0(const Engine* e, int i) { return ((e->L - i) & 1) ? e->z : e->dXh; }     // slice-0 partial dX' of layer i
bool bb_striped(const Route& r, int i) { return i > 1 ? r.st_bb : r.st_bb1; }            // layer i's BatchNorm-backward sums go to the accumulator planes
int bb_gconv_bwd(Ctx& c, Bwd& b, int i, const AttBwdGraphArgs* att) {
    Engine* e = c.e;
    const Route& r = c.r;
    const int N = c.N, H = e->H, L = e->L;
    const int64_t E = c.E;
    const size_t NH = (size_t)N * H;
    const bool two = H > GC_N;
    GconvBwdBranch gb;
    memset(&gb, 0, sizeof(gb));
    gb.x = e->h + (size_t)(i - 1) * NH; gb.W = e->P + e->o_conv_w[i - 1]; gb.dis = e->dis_unit; gb.bn = bnref(c, i, N, 0);
    gb.dxp0 = bb_dxp0(e, i); gb.dxp1 = e->dzi + (size_t)(i - 1) * NH;
    gb.coef_in = r.bb_bwd != Conv::Wide ? e->coef : r.plan_coef ? e->coef_src : nullptr;
    if (i == L) gb.dout = att ? nullptr : e->dZ;
    else {
        gb.dy0 = bb_dxp0(e, i + 1);
        gb.dy1 = two ? e->dzi + (size_t)i * NH : nullptr;
        gb.y = e->h + (size_t)i * NH;
        gb.ubn = bnref(c, i + 1, N, 0); gb.udot_sum = bn_dsum(c, i + 1); gb.udot_prod = bn_dprod(c, i + 1);
        gb.bias_parts = b.d_convb[i - 1].p;
    }
    float* dst[1] = {e->G + e->o_conv_w[i - 1]};
    double* dsum[1] = {bn_dsum(c, i)}; double* dprod[1] = {bn_dprod(c, i)};
    ProfScope ps(c.st, 4, 4.0 * N * H * H + 2.0 * (double)(E + N) * H, true);
    return gconv_bwd(c, b, &gb, 1, dst, dsum, dprod, bb_striped(r, i), att);
}

// P8. everything between the last backbone conv and the two causal convs
int bwd_att(Ctx& c, Bwd& b) {
    Engine* e = c.e;
    const Route& r = c.r;
    const int N = c.N, T = c.T, H = e->H, L = e->L;
    const int64_t E = c.E;
    hipStream_t st = c.st;
    const size_t NH = (size_t)N * H;
    AttBwdArgs aa;
    aa.x = e->h + (size_t)L * NH; aa.anode = e->anode; aa.dxhc = e->dXhco; aa.dxho = e->dXhco + NH;
    const bool two = r.co_bwd != Conv::Node && H > GC_N;      // second output-column slice of the fused backward
    aa.dxhc2 = two ? e->dzco : nullptr; aa.dxho2 = two ? e->dzco + NH : nullptr;
    aa.bnc = bnref(c, L + 1, N, 0); aa.bno = bnref(c, L + 2, N, 0);
    aa.dsc = bn_dsum(c, L + 1); aa.dpc = bn_dprod(c, L + 1); aa.dso = bn_dsum(c, L + 2); aa.dpo = bn_dprod(c, L + 2); aa.dss = e->bn_plane;
    aa.Wn = e->P + e->o_natt_w; aa.We = e->P + e->o_eatt_w; aa.dl = e->dl;
    aa.fnode = e->no_node_att ? 0.f : 1.f; aa.fedge = e->no_edge_att ? 0.f : 1.f;
    aa.gs = csr_src(c); aa.gd = csr_dst(c); aa.dZ = e->dZ;
    // one partial row per workgroup: r.ag_split per graph (k_att_bwd_graph / k_att_bwd_wide), or one per row block (k_att_bwd)
    // (folded into the last backbone layer's launch: one per unit, the column slices write disjoint columns)
    const int P = r.att_bwd == Att::Node ? cdiv(N, c.rpb_n) : r.att_fold ? T : r.ag_split * T;
    if (L > 0) { RCP(b.defer(c, b.d_convb[L - 1], P, H)); aa.dbias = b.d_convb[L - 1].acc(); }
    RCP(b.defer(c, b.d_dwn, P, H + 4)); RCP(b.defer(c, b.d_dwe, P, 2 * H + 4));
    aa.dWn = b.d_dwn.acc(); aa.dWe = b.d_dwe.acc();
    if (r.att_bwd == Att::Wide) {       // per graph of up to 256 nodes: with a sparse edge phase (engine_attwide.hpp); inputs in edge-id order
        AttBwdWideArgs ag;
        ag.a = aa; ag.gptr = e->gptr; ag.eptr = e->eptr; ag.row32 = e->row32; ag.col32 = e->col32; ag.att = e->att; ag.dis = e->dis_co;
        ag.gn = e->gn; ag.gn2 = two ? e->gn + 2 * (size_t)E : nullptr;
        ag.gself = e->gself; ag.gself2 = two ? e->gself + 2 * (size_t)N : nullptr;
        ag.loop_w = e->loop_w; ag.E = E; ag.N = N; ag.status = e->status;
        RC(with_g(H, [&](auto g) {
            constexpr int G = decltype(g)::value;
            hipLaunchKernelGGL((k_att_bwd_wide<4, G>), dim3(r.ag_split * T), dim3(512), 0, st, ag, 1, H, r.ag_split);
            return 0;
        }));
        CAL_CHECK_LAUNCH("k_att_bwd_wide"); STAGE();
    } else if (r.att_bwd == Att::Graph) {       // per graph: d deg, d edge logits and the row pass in one kernel (engine_attbwd.hpp)
        AttBwdGraphArgs ag;
        ag.a = aa; ag.gptr = e->gptr; ag.eptr = e->eptr; ag.att = e->wslot; ag.dis = e->dis_co;
        ag.gn = e->gn; ag.gn2 = two ? e->gn + 2 * (size_t)E : nullptr;
        ag.gself = e->gself; ag.gself2 = two ? e->gself + 2 * (size_t)N : nullptr;
        ag.loop_w = e->loop_w; ag.E = E; ag.N = N; ag.status = e->status;
        if (r.att_fold) {
            // one launch with layer L's backward (k_gconv_bwd's ATT mode): this site keeps its name, bwd_backbone launches nothing for L
            RC(bb_gconv_bwd(c, b, L, &ag)); STAGE();
            RC(flush_finals(c)); STAGE();
            return 0;
        }
        RC(with_g(H, [&](auto g) {
            constexpr int G = decltype(g)::value;
            hipLaunchKernelGGL((k_att_bwd_graph<4, G>), dim3(r.ag_split * T), dim3(512), 0, st, ag, 1, H, r.ag_split);
            return 0;
        }));
        CAL_CHECK_LAUNCH("k_att_bwd_graph"); STAGE();
    } else {
        // striped reader where the bnc / bno backward sums went to the planes
        const bool sr = r.st_node || r.st_co;
        RC(with_g(H, [&](auto g) {
            constexpr int G = decltype(g)::value;
            if (sr) hipLaunchKernelGGL((k_att_bwd<4, G, true>), dim3(cdiv(N, c.rpb_n)), dim3(256), 0, st, aa, 1, N, H, c.rpb_n);
            else hipLaunchKernelGGL((k_att_bwd<4, G>), dim3(cdiv(N, c.rpb_n)), dim3(256), 0, st, aa, 1, N, H, c.rpb_n);
            return 0;
        }));
        CAL_CHECK_LAUNCH("k_att_bwd"); STAGE();
    }
    return 0;
}

// feature layer h0 = relu(BN0(x0) W_feat) per unit, fed from the first backbone layer's partial input gradients
// (engine_gconv_bwd.hpp: one MFMA product per unit, any F <= 160); nobn: no BatchNorm between h0 and that layer (GIN)
int bwd_feat_units(Ctx& c, Bwd& b, const float* x0, const float* p0, const float* p1, bool nobn) {
    Engine* e = c.e;
    const int N = c.N, H = e->H, F = e->F;
    hipStream_t st = c.st;
    FeatBwdArgs fb;
    memset(&fb, 0, sizeof(fb));
    fb.dy0 = p0; fb.dy1 = p1; fb.y = e->h;
    if (!nobn) { fb.ubn = bnref(c, 1, N, 0); fb.udot_sum = bn_dsum(c, 1); fb.udot_prod = bn_dprod(c, 1); }
    fb.x0 = x0; fb.W = e->P + e->o_feat_w; fb.bn0 = bnref(c, 0, N, 0);
    // units: the graphs (tiles) of the per-graph kernels -- or, behind the wide convolutions (129-256-node graphs), uniform chunks
    // of FB_T rows: the layer is row-wise, the chunks need not be graphs (k_feat_bwd with a null unit table)
    const bool chunks = c.r.feat_chunks;
    const int U = chunks ? cdiv(N, FB_T) : c.T;
    RCP(fb.slab = b.slabs(c, U, F * H, e->G + e->o_feat_w));
    RCP(fb.parts = b.defer(c, b.d_bn0, U, 2 * F));
    const dim3 grid(U), blk(GB_NT);
    if (F <= FB_F && !nobn) {
        // few features (SPMotif: F = 10): the FMA-loop kernel is 1.7 us shorter than one MFMA tile behind three barriers
        if (F <= 16) hipLaunchKernelGGL(k_feat_bwd<16>, grid, blk, 0, st, chunks ? (const int*)nullptr : (const int*)e->gptr, fb, H, F, e->status, N);
        else hipLaunchKernelGGL(k_feat_bwd<FB_F>, grid, blk, 0, st, chunks ? (const int*)nullptr : (const int*)e->gptr, fb, H, F, e->status, N);
    } else if (F <= 64) {
        hipLaunchKernelGGL((k_feat_bwd_mma<8, true>), grid, blk, 0, st, e->gptr, fb, H, F, e->status);
    } else {
        if (nobn) hipLaunchKernelGGL((k_feat_bwd_mma<20, true>), grid, blk, 0, st, e->gptr, fb, H, F, e->status);
        else hipLaunchKernelGGL((k_feat_bwd_mma<20, false>), grid, blk, 0, st, e->gptr, fb, H, F, e->status);
    }
    CAL_CHECK_LAUNCH("k_feat_bwd");
    return 0;
}

// Q. backbone layers, last to first (and the feature layer's backward where it rides with layer 1)
int bwd_backbone(Ctx& c, Bwd& b, const float* x0) {
    Engine* e = c.e;
    const Route& r = c.r;
    const int N = c.N, T = c.T, H = e->H, F = e->F, L = e->L;
    const int64_t E = c.E;
    hipStream_t st = c.st;
    const size_t NH = (size_t)N * H;
    const CSR gd = csr_dst(c), gs = csr_src(c);
    const int PN = cdiv(N, c.rpb_n);
    const bool units = r.feat_bwd == FeatBwd::Units, two = H > GC_N;
    for (int i = L; i >= 1; --i) {
        float* dzi = e->dzi + (size_t)(i - 1) * NH;     // per layer: dz_i of the node-level chain, slice-1 partial dX' of the per-graph kernels
        const float* hin = e->h + (size_t)(i - 1) * NH;
        const bool st_i = bb_striped(r, i);
        if (e->gin && r.bb_bwd == Conv::Graph64) {
            // GINConv backward per graph (engine_ggin.hpp): second Linear (+ the BatchNorm-backward sums behind the ReLU) |
            // BatchNorm backward, first Linear, transposed aggregation.  Partial input gradients (one per output-column
            // slice): PART 2 -> (dXh, gy[i-1]), PART 1 -> (z, gagg[i-1]); the layer below (or the mask pass in front of the
            // feature layer) adds the two and masks by h_{i-1} > 0.
            const int nsl = H / GC_N;
            float* c0 = e->dXh; float* c1 = e->gy + (size_t)(i - 1) * NH;
            float* d0 = e->z; float* d1 = e->gagg + (size_t)(i - 1) * NH;
            const float* t1 = e->gt1 + (size_t)(i - 1) * NH;
            GginBwdArgs ga;
            memset(&ga, 0, sizeof(ga));
            if (i == L) ga.dout = e->dZ;
            else {
                ga.dy0 = e->z; ga.dy1 = two ? e->gagg + (size_t)i * NH : nullptr; ga.hmask = e->h + (size_t)i * NH;
                // d b2 of this layer: column sums of the masked d h_i, one partial row per unit
                RCP(ga.bias_parts = b.defer(c, b.d_convb[i - 1], T, H));
            }
            ga.x = t1; ga.W = e->P + e->o_gin_w2[i - 1]; ga.bn = bnref(c, i, N, 0);
            ga.dxp0 = c0; ga.dxp1 = c1;
            RCP(ga.slab = b.slabs(c, T, H * H, e->G + e->o_gin_w2[i - 1]));
            RC(bn_bwd_sums(c, ga, T * nsl, bn_dsum(c, i), bn_dprod(c, i), st_i));
            hipLaunchKernelGGL((k_ggin_bwd<2>), dim3(T, nsl), dim3(GB_NT), 0, st, gd, e->gptr, e->eptr, ga, N, H, H, e->status);
            CAL_CHECK_LAUNCH("k_ggin_bwd<2>"); STAGE();
            RC(flush_finals(c)); STAGE();
            memset(&ga, 0, sizeof(ga));
            ga.dy0 = c0; ga.dy1 = two ? c1 : nullptr; ga.t1 = t1;
            ga.dot_sum = bn_dsum(c, i); ga.dot_prod = bn_dprod(c, i);
            RCP(ga.bias_parts = b.defer(c, b.d_gin_b1[i - 1], T, H));             // d b1: column sums of dt1
            ga.x = hin; ga.W = e->P + e->o_conv_w[i - 1]; ga.bn = bnref(c, i, N, 0);
            ga.dxp0 = d0; ga.dxp1 = d1;
            RCP(ga.slab = b.slabs(c, T, H * H, e->G + e->o_conv_w[i - 1]));
            {
                ProfScope ps(st, 10, 4.0 * N * H * H + 2.0 * (double)(E + N) * H, true);
                prof_launch(k_ggin_bwd<1>, dim3(T, nsl), dim3(GB_NT), st, gd, e->gptr, e->eptr, ga, N, H, H, e->status);
            }
            CAL_CHECK_LAUNCH("k_ggin_bwd<1>"); STAGE();
            if (i == 1 && units) {
                RC(bwd_feat_units(c, b, x0, d0, two ? d1 : nullptr, true)); STAGE();
            } else if (i == 1) {                         // the feature layer below takes d h0 masked by h0 > 0 in e->dZ
                GinRowArgs gr;
                memset(&gr, 0, sizeof(gr));
                gr.a = d0; gr.a2 = two ? d1 : nullptr; gr.y = e->h; gr.out = e->dZ;
                RC(gin_rows(c, 3, gr));
                CAL_CHECK_LAUNCH("k_gin_mask"); STAGE();
            }
            continue;
        }
        if (e->gin) {
            // GINConv backward (model.py:188-194 differentiated).  e->dZ holds dz2 = d h_i masked by h_i > 0 (its column sums,
            // d b2, are already deferred): dW2 = dz2^T y, dy = dz2 W2, BatchNorm backward behind the ReLU -> dt1 (+ d b1),
            // dW1 = dt1^T agg, dagg = dt1 W1, d h_{i-1} = dagg + A^T dagg, masked by h_{i-1} > 0 for the layer below
            const float* agg = e->gagg + (size_t)(i - 1) * NH;
            const float* t1 = e->gt1 + (size_t)(i - 1) * NH;
            const float* yy = e->gy + (size_t)(i - 1) * NH;
            {
                GemmArgs a = gemm_args(H, H, N, true, false, 0);
                a.p[0].A = e->dZ; a.p[0].B = yy;
                float* dst[1] = {e->G + e->o_gin_w2[i - 1]};
                RC(grad_gemm(c, b, a, 1, dst)); STAGE();
            }
            {
                GemmArgs a = gemm_args(N, H, H, false, false, 0);
                a.p[0].A = e->dZ; a.p[0].B = e->P + e->o_gin_w2[i - 1]; a.p[0].C = e->dXh;      // dy
                RC(fwd_gemm(c, false, a, 1)); STAGE();
            }
            {
                GinRowArgs ga;
                memset(&ga, 0, sizeof(ga));
                ga.a = e->dXh; ga.y = yy; ga.t1 = t1; ga.bn = bnref(c, i, N, 0);
                ga.acc0 = node_acc(c, bn_dsum(c, i), H); ga.acc1 = node_acc(c, bn_dprod(c, i), H);
                RC(gin_rows(c, 1, ga));
                CAL_CHECK_LAUNCH("k_gin_dots"); STAGE();
                RC(flush_finals(c)); STAGE();
            }
            {
                GinRowArgs ga;
                memset(&ga, 0, sizeof(ga));
                ga.a = e->dXh; ga.y = yy; ga.t1 = t1; ga.out = dzi; ga.bn = bnref(c, i, N, 0);       // dt1
                ga.dot_sum = bn_dsum(c, i); ga.dot_prod = bn_dprod(c, i);
                RCP(b.defer(c, b.d_gin_b1[i - 1], PN, H));
                ga.acc0 = b.d_gin_b1[i - 1].acc();
                RC(gin_rows(c, 2, ga));
                CAL_CHECK_LAUNCH("k_gin_bn_bwd"); STAGE();
            }
            {
                GemmArgs a = gemm_args(H, H, N, true, false, 0);
                a.p[0].A = dzi; a.p[0].B = agg;
                float* dst[1] = {e->G + e->o_conv_w[i - 1]};
                RC(grad_gemm(c, b, a, 1, dst)); STAGE();
            }
            {
                GemmArgs a = gemm_args(N, H, H, false, false, 0);
                a.p[0].A = dzi; a.p[0].B = e->P + e->o_conv_w[i - 1]; a.p[0].C = e->dXh;            // dagg
                RC(fwd_gemm(c, false, a, 1)); STAGE();
            }
            {
                SpmmBranch br{e->dXh, e->z, nullptr, nullptr, e->ones, Acc(), Acc(), nullptr, nullptr, nullptr};                // d h_{i-1}
                RC(launch_espmm(st, gs, SpmmBranch2{{br, br}}, 1, 0, 1.0f, N, H, spmm_rpb(H, false)));
                CAL_CHECK_LAUNCH("k_espmm(gin,T)"); STAGE();
            }
            {
                GinRowArgs ga;
                memset(&ga, 0, sizeof(ga));
                ga.a = e->z; ga.y = hin; ga.out = e->dZ;                                                // masked by h_{i-1} > 0
                if (i >= 2) { RCP(b.defer(c, b.d_convb[i - 2], PN, H)); ga.acc0 = b.d_convb[i - 2].acc(); }   // d b2 of the layer below
                RC(gin_rows(c, 3, ga));
                CAL_CHECK_LAUNCH("k_gin_mask"); STAGE();
            }
            continue;
        }
        // Per graph: slice-0 partials of dX' ping-pong between dXh and z (idle in the fused forward), slice-1 partials are per layer
        // (bb_gconv_bwd for the GCN layers).
        float* p0 = bb_dxp0(e, i);
        if (r.bb_bwd != Conv::Node && i < L) RCP(b.defer(c, b.d_convb[i - 1], T, H));   // bias of conv i: one partial row per graph
        if (e->K > 0 && r.bb_bwd == Conv::Graph64) {
            // GATConv layer backward per graph (engine_ggat.hpp): attention backward + dX' (two slice partials) + dW / d att slabs
            const int K = e->K, D = H / K, nsl = H / GC_N;
            const size_t nk = al((size_t)e->capN * K);
            const float* sc = e->gsc + (size_t)(i - 1) * 4 * nk;
            GgatBwdArgs ga;
            memset(&ga, 0, sizeof(ga));
            ga.x = hin; ga.W = e->P + e->o_conv_w[i - 1]; ga.att = e->P + e->o_conv_att[i - 1];
            ga.z = e->gz + (size_t)(i - 1) * NH; ga.adst = sc; ga.asrc = sc + nk; ga.mx = sc + 2 * nk; ga.den = sc + 3 * nk;
            ga.bn = bnref(c, i, N, 0); ga.dxp0 = p0; ga.dxp1 = dzi;
            ga.heads = K; ga.D = D; ga.slope = e->gat_slope; ga.p = c.training ? e->gat_p : 0.f;
            ga.seed = e->gat_seed[i - 1]; ga.ctr = (const uint64_t*)e->gat_ctr; ga.E = E;
            if (i == L) ga.dout = e->dZ;
            else {
                ga.dy0 = ((L - i - 1) & 1) ? e->z : e->dXh;
                ga.dy1 = two ? e->dzi + (size_t)i * NH : nullptr;
                ga.y = e->h + (size_t)i * NH;
                ga.ubn = bnref(c, i + 1, N, 0); ga.udot_sum = bn_dsum(c, i + 1); ga.udot_prod = bn_dprod(c, i + 1);
                ga.bias_parts = b.d_convb[i - 1].p;
            }
            RCP(ga.slab = b.slabs(c, T, H * H, e->G + e->o_conv_w[i - 1]));
            RCP(ga.att_slab = b.slabs(c, T, 2 * H, e->G + e->o_conv_att[i - 1]));
            RC(bn_bwd_sums(c, ga, T * nsl, bn_dsum(c, i), bn_dprod(c, i), st_i));
            {
                ProfScope ps(st, 8, 4.0 * N * H * H + 4.0 * (double)(E + N) * H, true);
                if (i == L) prof_launch(k_ggat_bwd<false>, dim3(T, nsl), dim3(GB_NT), st, gd, e->gptr, e->eptr, ga, N, H, H, e->status);
                else prof_launch(k_ggat_bwd<true>, dim3(T, nsl), dim3(GB_NT), st, gd, e->gptr, e->eptr, ga, N, H, H, e->status);
            }
            CAL_CHECK_LAUNCH("k_ggat_bwd"); STAGE();
            RC(flush_finals(c)); STAGE();
        } else if (r.bb_bwd != Conv::Node) {
            // GCNConv per graph (bb_gconv_bwd); layer L rode in the attention backward's launch when the route folds the two
            if (!(i == L && r.att_fold)) {
                RC(bb_gconv_bwd(c, b, i, nullptr)); STAGE();
                RC(flush_finals(c)); STAGE();
            }
        }
        // BatchNorm_i backward of layer i's input gradient (two slice partials q0 + q1, or one) into e->dZ, the bias sums of the layer
        // below into `acc`; st: the striped instantiation (the site's sums are in the accumulator planes)
        auto bn_bwd_dz = [&](const float* q0, const float* q1, Acc acc, bool st_rd) -> int {
            BnBwdProb p{q0, hin, e->dZ, bnref(c, i, N, 0), bn_dsum(c, i), bn_dprod(c, i), acc, q1};
            RC(with_g(H, [&](auto g) {
                constexpr int G = decltype(g)::value;
                if (st_rd) hipLaunchKernelGGL((k_bn_bwd<4, G, true>), dim3(PN, 1), dim3(256), 0, st, BnBwdProb3{{p, p, p}}, 1, N, H, c.rpb_n);
                else hipLaunchKernelGGL((k_bn_bwd<4, G>), dim3(PN, 1), dim3(256), 0, st, BnBwdProb3{{p, p, p}}, 1, N, H, c.rpb_n);
                return 0;
            }));
            CAL_CHECK_LAUNCH("k_bn_bwd"); STAGE();
            return 0;
        };
        if (r.bb_bwd != Conv::Node) {
            if (i > 1) continue;
            // the feature layer's backward per graph (wide graphs: per 64-row chunk), fed from this layer's partial dX' -- or, when
            // it is a plain GEMM, dZ materialised for it
            if (units) { RC(bwd_feat_units(c, b, x0, p0, two ? dzi : nullptr, false)); STAGE(); }
            else RC(bn_bwd_dz(p0, two ? dzi : nullptr, Acc(), r.st_bb1));
            continue;
        }
        if (e->K > 0) {       // dz_i and d att_i from dOut_i (GATConv backward; alpha recomputed from the saved max / denominator)
            const int K = e->K, D = H / K;
            const size_t nk = al((size_t)e->capN * K);
            const float* sc = e->gsc + (size_t)(i - 1) * 4 * nk;
            ProfScope ps(st, 6, 4.0 * N * H * 4 + (double)(E + N) * (16 + 24.0 * K));
            // d att: per-block partial rows parked in the slab area, summed by the final k_finish (no finishing launch)
            float* part = b.slabs(c, gat_datt_parts(N), 2 * H, e->G + e->o_conv_att[i - 1]);
            RCP(part);
            RC(gat_backward(e->rowptr_dst, e->nbr_dst, e->eid_dst, e->rowptr_src, e->nbr_src, e->eid_src,
                            e->gz + (size_t)(i - 1) * NH, e->P + e->o_conv_att[i - 1], sc, sc + nk, sc + 2 * nk, sc + 3 * nk, e->dZ,
                            e->gat_slope, c.training ? e->gat_p : 0.f, e->gat_seed[i - 1], (const uint64_t*)e->gat_ctr, dzi,
                            e->G + e->o_conv_att[i - 1], e->gws, N, E, K, D, st, part, nullptr));
        } else {
            SpmmBranch br{e->dZ, dzi, nullptr, nullptr, e->dis_unit, Acc(), Acc(), nullptr, nullptr, nullptr};
            ProfScope ps(st, 1, 2.0 * N * H * 4 + (double)(E + N) * 8 + (N + 1) * 4.0, true);
            RC(launch_espmm(st, gs, SpmmBranch2{{br, br}}, 1, 0, e->loop_w, N, H, spmm_rpb(H, false)));
            CAL_CHECK_LAUNCH("k_espmm(T)");
        }
        STAGE();
        {
            GemmArgs aw = gemm_args(H, H, N, true, false, 0);
            aw.p[0].A = hin; aw.p[0].B = dzi;
            aw.p[0].xa.has_bn = 1; aw.p[0].xa.bn = bnref(c, i, N, 0);
            float* dst[1] = {e->G + e->o_conv_w[i - 1]};
            GemmArgs a = gemm_args(N, H, H, false, true, 0);
            a.p[0].A = dzi; a.p[0].B = e->P + e->o_conv_w[i - 1]; a.p[0].C = e->dXh;
            a.p[0].aux = hin; a.p[0].has_aux = 1; a.p[0].aux_bn = bnref(c, i, N, 0);
            gemm_stats(c, a.p[0], N, H, bn_dsum(c, i), bn_dprod(c, i), true, H, r.st_node);
            { ProfScope ps(st, 3, 4.0 * N * H * H); RC(dual_gemm(c, b, a, 1, aw, 1, dst)); } STAGE();
            RC(flush_finals(c)); STAGE();
        }
        if (i == 1 && r.feat_bwd == FeatBwd::Rows) {
            // the last BatchNorm backward feeds only the feature layer: dZ stays in registers (engine_feat.hpp)
            const int cols = (F + 1) * H;
            FeatBwdRowsArgs fb{e->dXh, hin, bnref(c, 1, N, 0), bn_dsum(c, 1), bn_dprod(c, 1), x0, bnref(c, 0, N, 0), parts_alloc(c, (size_t)PN * cols)};
            double* sums = parts_alloc(c, cols);
            if (!fb.parts || !sums) return no_parts();
            RCP(b.defer(c, b.d_bn0, 1, 2 * F));
            float* dw = b.slabs(c, 1, F * H, e->G + e->o_feat_w);
            RCP(dw);
            RC(with_g_fp(H, F, [&](auto g, auto fp) {
                hipLaunchKernelGGL((k_bn_bwd_feat<decltype(g)::value, decltype(fp)::value>), dim3(PN), dim3(256), 0, st, fb, N, H, F, c.rpb_n);
                return 0;
            }));
            CAL_CHECK_LAUNCH("k_bn_bwd_feat"); STAGE();
            final_task(c, fb.parts, PN, cols, cols, sums);
            RC(flush_finals(c)); STAGE();
            hipLaunchKernelGGL(k_feat_bwd_final, dim3(F), dim3(256), 0, st, sums, e->P + e->o_feat_w, bnref(c, 0, N, 0), dw, b.d_bn0.p, H, F);
            CAL_CHECK_LAUNCH("k_feat_bwd_final"); STAGE();
        } else {
            if (i >= 2) RCP(b.defer(c, b.d_convb[i - 2], PN, H));       // the bias sums of the layer below
            RC(bn_bwd_dz(e->dXh, nullptr, i >= 2 ? b.d_convb[i - 2].acc() : Acc(), r.st_node));
        }
    }
    return 0;
}

// S. conv_feat weight and bn_feat affine gradients through the GEMM chain (unless they rode with layer 1 / the row kernels)
int bwd_feat(Ctx& c, Bwd& b, const float* x0) {
    Engine* e = c.e;
    const int N = c.N, H = e->H, F = e->F;
    if (c.r.feat_bwd != FeatBwd::Gemm) return 0;
    GemmArgs aw = gemm_args(F, H, N, true, false, 0);
    aw.p[0].A = x0; aw.p[0].B = e->dZ;
    aw.p[0].xa.has_bn = 1; aw.p[0].xa.bn = bnref(c, 0, N, 0);
    float* dst[1] = {e->G + e->o_feat_w};
    GemmArgs a = gemm_args(N, F, H, false, true, 0);
    a.p[0].A = e->dZ; a.p[0].B = e->P + e->o_feat_w; a.p[0].C = nullptr;
    a.p[0].aux = x0; a.p[0].has_aux = 1; a.p[0].aux_bn = bnref(c, 0, N, 0);
    a.p[0].dot_sum = bn_dsum(c, 0); a.p[0].dot_prod = bn_dprod(c, 0);
    {   // bn_feat's sums are only needed by the commit: keep the partial rows, no finalise launch
        const int P0 = use_ks(N) ? gemm_ks_row_tiles(N) : gemm_row_tiles(N, F, H, false);
        if ((size_t)P0 * F * 2 > 4096) {
            // (no rows left is no error here: the epilogue then adds into the arena, which bwd_commit reads while d_bn0 is empty)
            a.p[0].parts = b.defer(c, b.d_bn0, P0, 2 * F);
        }
    }
    RC(dual_gemm(c, b, a, 1, aw, 1, dst)); STAGE();
    return 0;
}

// The commit as k_finish_plan (finish_plan.hip): beside it the plan of Engine::next (plan_next), or alone as the finish-only launch
// that ends a chain.  The words a stand-alone pair of launches shares go through in / out addresses here (engine_finish.hpp,
// ChainCtl): position j of a chain reads the words of parity j & 1 and writes those of the other parity; the chain's first step
// reads, and its last step writes, the tensors the optimizer and the permutation stream are bound to.
int commit_chained(Ctx& c, FinishArgs& fa, int nblk, bool plan_next) {
    Engine* e = c.e;
    const int p = c.parity, q = p ^ 1;
    float* step_w = (float*)(e->status + ST_STEP);
    unsigned long long* ctr_w = (unsigned long long*)(e->status + ST_CTR);
    ChainPlan pn; ChainCtl ctl;
    memset(&pn, 0, sizeof(pn)); memset(&ctl, 0, sizeof(ctl));
    ctl.step_in = c.chained_in ? step_w + p : e->step;
    ctl.step_out = plan_next ? step_w + q : e->step;
    if (c.draw_perm) {
        ctl.ctr_in = c.chained_in ? ctr_w + p : e->perm_ctr;
        ctl.ctr_out = plan_next ? ctr_w + q : e->perm_ctr;
    }
    ctl.pend_cur = c.chained_in ? e->status + ST_PEND + p : nullptr;
    if (ctl.step_in == ctl.step_out || (c.draw_perm && ctl.ctr_in == ctl.ctr_out)) { set_error("engine: a chained commit would read the word it writes"); return 2; }
    fa.tick = nullptr; fa.ticked = nullptr; fa.perm_ctr = nullptr;      // (ChainCtl's words instead)
    fa.adam.step = const_cast<float*>(ctl.step_in);
    if (plan_next) {
        const Engine::BatchDesc& d = e->next;
        Ctx cn;
        next_ctx(cn, e, c.st, d, c.mode);
        const int wp0 = (e->bn[0].width + 3) / 4 * 4;
        double* an = e->arena2[q];
        pn.ei = d.ei; pn.E = d.E; pn.N = (int)d.N; pn.B = cn.T;
        pn.node_ptr = d.node_ptr; pn.edge_ptr = d.edge_ptr; pn.batch = d.batch; pn.tile_gptr = d.ntiles > 0 ? d.tile_gptr : nullptr;
        pn.Bgraphs = (int)d.B; pn.loop_w = e->loop_w;
        pn.ptr_dst = e->rowptr_dst; pn.nbr_dst = e->nbr_dst; pn.eid_dst = e->eid_dst;
        pn.ptr_src = e->rowptr_src; pn.nbr_src = e->nbr_src; pn.eid_src = e->eid_src;
        pn.row32 = e->row32; pn.col32 = e->col32; pn.gptr = e->gptr; pn.eptr = e->eptr; pn.dis_unit = e->dis_unit;
        pn.pending = e->status + ST_PEND + q;
        pn.x0 = cn.r.plan_stats ? d.x0 : nullptr; pn.F = e->F;
        pn.st_sum = an + e->bn[0].arena; pn.st_sq = an + e->bn[0].arena + wp0;
        pn.coef_dst = cn.r.plan_coef ? e->coef : nullptr; pn.coef_src = cn.r.plan_coef ? e->coef_src : nullptr;
        pn.arena = an; pn.n = e->arena_n; pn.skip_lo = e->bn[0].arena; pn.skip_hi = e->bn[0].arena + 2 * wp0;
        pn.gat_tick = e->K > 0 ? e->gat_ctr : nullptr;
        pn.perm = c.draw_perm ? e->perm_dev : nullptr; pn.permB = (int)d.B; pn.seed = e->perm_seed;
        ctl.nplan = cn.T + (c.draw_perm ? cdiv((int)d.B, 256 / 4) : 0);
    }
    const calunit::LaunchSite at{dim3(ctl.nplan + nblk), c.st, nullptr, nullptr};
    const int rc = cal_launch_finish_plan(at, &fa, sizeof(fa), e->G, &pn, sizeof(pn), &ctl, sizeof(ctl));
    if (rc) { set_error("engine: finish_plan.hip was built with other structures than engine.hip (code %d)", rc); return 2; }
    CAL_CHECK_LAUNCH(plan_next ? "k_finish_plan" : "k_finish_plan(finish)"); STAGE();
    e->bn0_dirty_host = 0;          // bn_feat's statistics range of this step's arena is clean again behind this launch (PlanFold)
    if (plan_next) {
        e->planned = e->next; e->planned.valid = 1; e->planned.parity = q; e->planned.mode = c.mode; e->planned.ws = e->ws;
    }
    return 0;
}

// commits: fp64 arena / partial rows -> fp32 gradients, the slab sums and (single-process steps) Adam in one k_finish
int bwd_commit(Ctx& c, Bwd& b) {
    Engine* e = c.e;
    const int H = e->H, F = e->F, C = e->C, L = e->L;
    FinishArgs& fa = b.fa;
    auto commit_p = [&](const double* src, int P, int stride, int dst, int n, float scale) {
        if (fa.nct < MAX_COMMITS) fa.ct[fa.nct] = CommitTask{src, P, stride, dst, n, scale};
        fa.nct++;
    };
    // (a Deferred its route never filled is refused below, with the conv biases')
    bool missing = false;
    auto commit_d = [&](const Deferred& d, int col, int dst, int n, float scale) {
        if (d.p) commit_p(d.p + col, d.P, d.stride, dst, n, scale); else missing = true;
    };
    for (int k = 0; k < e->nbn; ++k) {
        const BNSlot& s = e->bn[k];
        const int wp = (s.width + 3) / 4 * 4;
        if (k == 0 && b.d_bn0.p) {
            commit_d(b.d_bn0, F, s.gamma, F, 1.f);
            commit_d(b.d_bn0, 0, s.beta, F, 1.f);
            continue;
        }
        // (the NSTRIPE accumulator planes of the site: engine.hpp, stripe_sum)
        commit_p(e->arena + s.arena + 3 * wp, NSTRIPE, e->bn_plane, s.gamma, s.width, 1.f);   // d gamma = sum dyh * x_n
        commit_p(e->arena + s.arena + 2 * wp, NSTRIPE, e->bn_plane, s.beta, s.width, 1.f);    // d beta  = sum dyh
    }
    for (int i = 0; i < L; ++i) {
        // GCNConv / GATConv: the layer's bias; GINConv: the bias of its second Linear (the first one's has its own sums)
        commit_d(b.d_convb[i], 0, e->gin ? e->o_gin_b2[i] : e->o_conv_b[i], H, 1.f);
        if (e->gin) commit_d(b.d_gin_b1[i], 0, e->o_conv_b[i], H, 1.f);
    }
    commit_d(b.d_cb, 0, e->o_cb, H, 1.f);
    commit_d(b.d_ob, 0, e->o_ob, H, 1.f);
    commit_d(b.d_dwn, 0, e->o_natt_w, H, 1.f);
    commit_d(b.d_dwn, 0, e->o_natt_w + H, H, -1.f);
    commit_d(b.d_dwn, H, e->o_natt_b, 1, 1.f);
    commit_d(b.d_dwn, H, e->o_natt_b + 1, 1, -1.f);
    commit_d(b.d_dwe, 0, e->o_eatt_w, 2 * H, 1.f);
    commit_d(b.d_dwe, 0, e->o_eatt_w + 2 * H, 2 * H, -1.f);
    commit_d(b.d_dwe, 2 * H, e->o_eatt_b, 1, 1.f);
    commit_d(b.d_dwe, 2 * H, e->o_eatt_b + 1, 1, -1.f);
    for (int hd = 0; hd < 3; ++hd) {
        commit_p(e->arena + e->a_db1 + hd * H, 1, 0, e->o_fc1_b[hd], H, 1.f);
        commit_p(e->arena + e->a_db2 + hd * C, 1, 0, e->o_fc2_b[hd], C, 1.f);
    }
    if (missing) { set_error("engine: missing bias-gradient partials"); return 2; }
    if (fa.nct > MAX_COMMITS) { set_error("engine: too many commit tasks"); return 2; }
    if (c.adam_in_finish) {
        // Adam rides in this kernel: parameter ranges no task writes (gradients stored directly by the readout /
        // single-slab GEMMs) become update-only tasks
        fa.adam = AdamArgs{e->P, e->M1, e->M2, e->step, e->lr, e->beta1, e->beta2, e->eps, e->wd, e->grad_scale, 1};
        std::vector<std::pair<int64_t, int64_t>> iv;
        for (int i = 0; i < fa.nst; ++i) iv.push_back({fa.st[i].dst - e->G, (fa.st[i].dst - e->G) + fa.st[i].n});
        for (int i = 0; i < fa.nct; ++i) iv.push_back({fa.ct[i].dst, (int64_t)fa.ct[i].dst + fa.ct[i].n});
        std::sort(iv.begin(), iv.end());
        int64_t pos = 0;
        bool ok = true;
        auto gap = [&](int64_t a, int64_t b) {
            if (b <= a) return;
            if (fa.nar >= MAX_ADAM_RANGES) { ok = false; return; }
            fa.ar[fa.nar++] = AdamRange{a, b};
        };
        for (auto& r : iv) {
            if (r.first < pos) { ok = false; break; }          // two tasks finish the same element: not expected
            gap(pos, r.first);
            pos = r.second;
        }
        gap(pos, e->nparam);
        if (!ok || pos > e->nparam) {                          // keep the separate k_adam launch
            fa.adam.on = 0; fa.nar = 0; c.adam_in_finish = 2;     // 2: k_adam follows, counter already advanced
        }
    }
    e->fin_n = 0; e->fin_adam = c.adam_in_finish;
    for (int i = 0; i < fa.nst; ++i) e->fin_iv[e->fin_n++] = {fa.st[i].dst - e->G, (fa.st[i].dst - e->G) + fa.st[i].n, 0};
    for (int i = 0; i < fa.nct; ++i) e->fin_iv[e->fin_n++] = {fa.ct[i].dst, (int64_t)fa.ct[i].dst + fa.ct[i].n, 1};
    for (int i = 0; i < fa.nar; ++i) e->fin_iv[e->fin_n++] = {fa.ar[i].begin, fa.ar[i].end, 2};
    int nblk = 0;
    for (int i = 0; i < fa.nst; ++i) { fa.blk0[i] = nblk; nblk += std::max(1, cdiv(fa.st[i].n, 64)); }
    for (int i = 0; i < fa.nct; ++i) { fa.blk0[fa.nst + i] = nblk; nblk += std::max(1, cdiv(fa.ct[i].n, 16)); }
    for (int i = 0; i < fa.nar; ++i) { fa.blk0[fa.nst + fa.nct + i] = nblk; nblk += (int)cdiv(fa.ar[i].end - fa.ar[i].begin, 256); }
    fa.blk0[fa.nst + fa.nct + fa.nar] = nblk;
    const bool plan_next = c.chain_out && c.adam_in_finish == 1;
    if (plan_next || c.chained_in) return commit_chained(c, fa, nblk, plan_next);
    hipLaunchKernelGGL(k_finish, dim3(nblk), dim3(256), 0, c.st, fa, e->G);
    CAL_CHECK_LAUNCH("k_finish"); STAGE();
    e->bn0_dirty_host = 0;          // bn_feat's statistics range is clean again behind this launch (PlanFold)
    return 0;
}

int engine_backward(Ctx& c, const float* x0) {
    Engine* e = c.e;
    Bwd b;
    memset(&b, 0, sizeof(b));
    FinishArgs& fa = b.fa;
    fa.tick = (c.tick_in_finish && !c.adam_in_finish) ? e->step : nullptr;      // (adam_in_finish: k_zero_f64 did it)
    fa.ticked = c.adam_in_finish ? e->step : nullptr;
    fa.perm_ctr = c.draw_perm ? e->perm_ctr : nullptr;
    fa.status = e->status;
    fa.host_status = e->host_status;
    { const int wp0 = (e->bn[0].width + 3) / 4 * 4; fa.bn0z = e->arena + e->bn[0].arena; fa.bn0z_n = 2 * wp0; fa.dirty = e->status + 3; }
    RC(bwd_readout(c, b));
    RC(bwd_co(c, b));
    RC(bwd_att(c, b));
    RC(bwd_backbone(c, b, x0));
    RC(bwd_feat(c, b, x0));
    return bwd_commit(c, b);
}

// The Ctx both entry points set up, with the route of a `mode` step
void ctx_init(Ctx& c, Engine* e, void* stream, int64_t N, int64_t E, int64_t B, const int64_t* batch, int mode) {
    memset(&c, 0, sizeof(c));
    c.e = e; c.st = (hipStream_t)stream; c.N = (int)N; c.B = (int)B; c.E = E;
    c.T = e->ntiles > 0 ? e->ntiles : (int)B;
    c.batch = batch;
    c.training = (mode & 1) ? 1 : 0;
    c.want_grad = (mode & 2) ? 1 : 0;
    // (16 k - 64 k rows: 512 workgroups -- a workgroup's prologue / column-sum epilogue over 32 rows was a third of k_att_bwd at 30 k rows)
    c.rpb_n = std::max(32, cdiv(N, N >= 16384 && N <= 65536 ? 512 : 1024));
    c.rpb_b = std::max(32, cdiv(B, 64));
    c.r = make_route(c, c.want_grad);
}

// The Ctx (and so the route) of the batch `d` in a `mode` step: the engine's description of the coming batch is swapped for d's
// while the route is made
void next_ctx(Ctx& cn, Engine* e, hipStream_t st, const Engine::BatchDesc& d, int mode) {
    const Engine::BatchDesc cur{nullptr, nullptr, nullptr, 0, 0, 0, e->node_ptr, e->edge_ptr, e->tile_gptr, e->ntiles, e->max_nodes, e->max_edges, 0, 0, 0, nullptr};
    e->node_ptr = d.node_ptr; e->edge_ptr = d.edge_ptr; e->tile_gptr = d.tile_gptr; e->ntiles = d.ntiles;
    e->max_nodes = d.max_nodes; e->max_edges = d.max_edges;
    ctx_init(cn, e, st, d.N, d.E, d.B, d.batch, mode);
    e->node_ptr = cur.node_ptr; e->edge_ptr = cur.edge_ptr; e->tile_gptr = cur.tile_gptr; e->ntiles = cur.ntiles;
    e->max_nodes = cur.max_nodes; e->max_edges = cur.max_edges;
}
// May a `mode` step of context c end with k_finish_plan for Engine::next?  (Adam inside the commit, the successor on the 256-thread
// per-graph plan with the PlanFold, both batches inside the workspace; otherwise the step ends and the next one starts as ever)
bool can_chain(const Ctx& c, Engine* e, int mode) {
    const Engine::BatchDesc& d = e->next;
    if (!e->chain || !e->chain_ok || !d.valid || g_stop_after != 0 || g_prof_on) return false;
    if (c.adam_in_finish != 1 || (mode & 8) || !c.training || !c.want_grad || !e->fold_zero) return false;
    if (d.N <= 0 || d.B <= 0 || d.N > e->capN || d.E > e->capE || d.B > e->capB || d.ntiles > d.B) return false;
    if (c.draw_perm && d.B > ZP_CAP) return false;
    if (!d.node_ptr || !d.edge_ptr) return false;
    Ctx cn;
    next_ctx(cn, e, c.st, d, mode);
    return cn.r.plan == Plan::Graph256;
}

// Adam as one kernel over the flat parameter buffer; ticked: the step counter has already been advanced (by the step's k_finish)
int launch_adam(Engine* e, hipStream_t st, int ticked) {
    hipLaunchKernelGGL(k_adam, dim3(cdiv(e->nparam, 256)), dim3(256), 0, st, e->P, e->G, e->M1, e->M2, e->step, e->lr, e->beta1,
                       e->beta2, e->eps, e->wd, e->nparam, ticked, e->grad_scale, e->status);
    CAL_CHECK_LAUNCH("k_adam");
    return 0;
}

}  // namespace

// One training step (or, with mode bits cleared, parts of it) for a device-resident batch.
//   x0 [N,F] fp32, edge_index [2,E] int64, batch [N] int64 (sorted), y [B] int64, perm [B] int64
//   (the random-intervention index, model.py:147-152; identity = arange).
//   mode: bit0 = forward in training mode (batch statistics, running-stat updates);
//         bit1 = loss gradient + backward (fills the flat gradient buffer);
//         bit2 = Adam update.  mode = 0 is an eval-mode forward.
//   Outputs live in the workspace: "logp" [3,B,C] log-probabilities (c, o, co), "stats" [5].
CAL_EXPORT int cal_engine_step(void* h, const float* x0, const int64_t* edge_index, const int64_t* batch, const int64_t* y,
                               const int64_t* perm, int64_t N, int64_t E, int64_t B, float wc, float wo, float wco, int mode,
                               void* stream_) {
    Engine* e = (Engine*)h;
    CAL_REQUIRE(e && e->ws, "engine has no workspace");
    CAL_REQUIRE(N <= e->capN && E <= e->capE && B <= e->capB, "batch exceeds the workspace capacity");
    CAL_REQUIRE(N > 0 && B > 0, "empty batch");
    CAL_REQUIRE(e->ntiles <= B, "more tiles than graphs (cal_engine_set_tiles belongs to another batch)");
    CAL_REQUIRE(e->ntiles == 0 || (e->H % GC_N == 0 && e->H <= GC_K && e->node_ptr && e->edge_ptr && e->max_nodes > 0 && e->max_nodes <= 64 &&
                                   e->max_edges <= gc_edge_cap(64)),
                "cal_engine_set_tiles needs the per-graph kernels: hidden in {64, 128}, the tiles' offsets (cal_engine_set_graph_ptrs) and bounds <= 64 nodes / 1024 edges");
    const int want_grad = (mode & 2) ? 1 : 0;
    CAL_REQUIRE(!(mode & 16) || (e->perm_ctr && B <= ZP_CAP && want_grad), "mode bit 16 needs cal_engine_set_perm_rng, at most 1024 graphs per batch and the backward pass (its last kernel advances the permutation counter)");
    CAL_REQUIRE((mode & 16) || perm, "perm is null and the step does not draw its own (mode bit 16)");
    CAL_REQUIRE(!(mode & 8) || want_grad, "mode bit 8 (Adam follows a gradient exchange) needs the backward pass");
    CAL_REQUIRE(!want_grad || (mode & 1), "backward needs a training-mode forward");
    CAL_REQUIRE(!(mode & 4) || want_grad, "the Adam update needs the backward pass in the same step");
    if (e->planned.valid) {
        // the previous step's last launch has planned a batch: this call must be for it (nothing is enqueued otherwise, and nothing re-planned)
        const Engine::BatchDesc& d = e->planned;
        const bool same = d.x0 == x0 && d.ei == edge_index && d.batch == batch && d.N == N && d.E == E && d.B == B && d.mode == mode &&
                          d.node_ptr == e->node_ptr && d.edge_ptr == e->edge_ptr && d.ntiles == e->ntiles &&
                          (d.ntiles == 0 || d.tile_gptr == e->tile_gptr) && d.max_nodes == e->max_nodes && d.max_edges == e->max_edges && d.ws == e->ws;
        if (!same) {
            e->next.valid = 0;
            set_error("cal_engine_step: the previous step planned another batch (cal_engine_set_next): this call is not the step it announced "
                      "(run that step, or cal_engine_chain_reset)");
            return 2;
        }
    }
    Ctx c;
    ctx_init(c, e, stream_, N, E, B, batch, mode);
    c.mode = mode;
    c.chained_in = e->planned.valid; c.parity = c.chained_in ? e->planned.parity : 0;
    e->planned.valid = 0;
    e->arena = e->arena2[c.parity];
    c.adam_in_finish = ((mode & 4) && e->adam_fused) ? 1 : 0;
    c.draw_perm = (mode & 16) ? 1 : 0;
    c.y = y; c.perm = c.draw_perm ? e->perm_dev : perm; c.wc = wc; c.wo = wo; c.wco = wco;
    c.tick_in_finish = (mode & (4 | 8)) ? 1 : 0;
    c.chain_out = can_chain(c, e, mode) ? 1 : 0;
    struct NextOnce { Engine* e; ~NextOnce() { e->next.valid = 0; } } next_once{e};      // an announcement holds for one call
    g_stage = 0;
    g_stage_names.clear();
    {
        int rc = engine_forward(c, x0, edge_index);
        if (rc == -12345) return 0;
        if (rc) return rc;
        if (want_grad) {
            rc = engine_backward(c, x0);
            if (rc == -12345) return 0;
            if (rc) return rc;
        }
    }
    if ((mode & 4) && c.adam_in_finish != 1) {          // k_finish has already advanced the step counter (c.tick_in_finish)
        RC(launch_adam(e, c.st, 1));
        if (g_stop_after == 0) g_stage_names.push_back(cal::g_last_launch);      // (named like a stage; never a stop point)
    }
    return 0;
}

// Backward from an external gradient (autograd surface): `dlogp` [3,B,C] = d loss / d log-probs of
// the LAST training-mode forward of the same batch (cal_engine_step with mode = 1); fills the flat
// gradient buffer exactly like mode bit 2.  The forward's activations, plan and statistics are
// taken from the workspace, so no other step may run in between.
CAL_EXPORT int cal_engine_backward_from(void* h, const float* x0, const int64_t* batch, const float* dlogp, int64_t N,
                                        int64_t E, int64_t B, void* stream_) {
    Engine* e = (Engine*)h;
    CAL_REQUIRE(e && e->ws, "engine has no workspace");
    CAL_REQUIRE(N <= e->capN && E <= e->capE && B <= e->capB && N > 0 && B > 0, "bad batch sizes");
    CAL_REQUIRE(e->ntiles <= B, "more tiles than graphs (cal_engine_set_tiles belongs to another batch)");
    CAL_REQUIRE(!e->planned.valid, "a planned step is owed (cal_engine_set_next): run it first");
    Ctx c;
    ctx_init(c, e, stream_, N, E, B, batch, 1);      // the route of the mode-1 forward it follows
    c.want_grad = 1;
    hipLaunchKernelGGL(k_logsoftmax_bwd, dim3(1), dim3(256), 0, c.st, e->logp, dlogp, e->dzl, e->arena + e->a_db2, (int)B, e->C);
    CAL_CHECK_LAUNCH("k_logsoftmax_bwd");
    g_stage = 0;
    int rc = engine_backward(c, x0);
    return rc == -12345 ? 0 : rc;
}

// The 3-term loss of train_causal.py:176-183 on log-probabilities logp [3, B, C] (heads c, o, co) with labels y [B]: out [4] =
// {loss, c_loss, o_loss, co_loss}, and (dlogp non-null) d loss / d logp [3, B, C] -- what cal_engine_backward_from takes.
// flag (may be null): bit 1 is set when a label lies outside [0, C).
CAL_EXPORT int cal_causal_loss(const float* logp, const int64_t* y, int64_t B, int64_t C, float wc, float wo, float wco, float* out,
                               float* dlogp, int32_t* flag, void* stream_) {
    CAL_REQUIRE(logp && y && out && B > 0 && C > 0 && B * C < (1ll << 30), "bad arguments");
    hipLaunchKernelGGL(k_causal_loss, dim3(1), dim3(256), 0, (hipStream_t)stream_, logp, y, (int)B, (int)C, wc, wo, wco, out, dlogp, (int*)flag);
    CAL_CHECK_LAUNCH("k_causal_loss");
    return 0;
}

// Per-graph bounds of the batches that follow (largest node count / stored-edge count of any single graph;
// 0 = unknown).  With bounds that fit (engine_gconv.hpp) the step runs the per-graph fused convolutions; a
// bound that turns out too small sets bit 3 of the status word and leaves that graph's outputs unwritten.
CAL_EXPORT int cal_engine_set_graph_bounds(void* h, int64_t max_nodes, int64_t max_edges) {
    Engine* e = (Engine*)h;
    CAL_REQUIRE(e != nullptr && max_nodes >= 0 && max_edges >= 0, "bad arguments");
    e->max_nodes = (int)std::min<int64_t>(max_nodes, 1 << 30);
    e->max_edges = (int)std::min<int64_t>(max_edges, 1 << 30);
    return 0;
}
// Layout of the coming batch, as every collate knows it: graph b owns nodes [node_ptr[b], node_ptr[b+1]) and the
// contiguous edge_index columns [edge_ptr[b], edge_ptr[b+1]), and no edge is a self loop (both [B+1] int64 DEVICE
// arrays, alive until the step has run; null = unknown).  Together with the per-graph bounds this selects the
// one-kernel per-graph GraphPlan; what the kernel finds violated is flagged in the status word.
CAL_EXPORT int cal_engine_set_graph_ptrs(void* h, const int64_t* node_ptr, const int64_t* edge_ptr) {
    Engine* e = (Engine*)h;
    CAL_REQUIRE(e != nullptr, "bad arguments");
    e->node_ptr = node_ptr; e->edge_ptr = edge_ptr;
    return 0;
}
// Small-graph packing.  The per-graph kernels give every workgroup a 64-row MFMA tile; a batch of ~30-node graphs (NCI1,
// MUTAG: BASELINE.json configs[2..3]) leaves half of it empty and launches twice the workgroups.  A batch is a disjoint union,
// so any run of CONSECUTIVE graphs is itself a block-diagonal graph: the caller groups consecutive graphs into tiles
// (<= 64 nodes, <= 1024 edges, <= 8 graphs each), passes the TILES' node / edge offsets and bounds through
// cal_engine_set_graph_ptrs / cal_engine_set_graph_bounds, and here the first graph of every tile: tile_gptr [ntiles + 1]
// (device int64, tile_gptr[ntiles] = B; alive until the step has run).  Only the add-pool and its backward look at graphs
// inside a tile (model.py:115-116).  ntiles = 0 / null: one graph per workgroup.
CAL_EXPORT int cal_engine_set_tiles(void* h, const int64_t* tile_gptr, int64_t ntiles) {
    Engine* e = (Engine*)h;
    CAL_REQUIRE(e != nullptr && ntiles >= 0 && (ntiles == 0 || tile_gptr != nullptr), "bad arguments");
    e->tile_gptr = ntiles > 0 ? tile_gptr : nullptr; e->ntiles = (int)ntiles;
    return 0;
}
// Deterministic mode (atomic-free, bit-reproducible reductions): on = 1 turns the striped fp64 accumulators
// (engine.hpp: stripe_sum -- order-dependent in the last bits) off for this engine: every BatchNorm sum is then a partial row per
// workgroup, added in a fixed order by k_stats_final (what CAL_AMD_STRIPED=0 selects process-wide).  Same results to ~1e-16
// relative, bit-identical from run to run; a few finishing launches per step slower.  Call before the first step is captured.
CAL_EXPORT int cal_engine_set_deterministic(void* h, int on) {
    Engine* e = (Engine*)h;
    CAL_REQUIRE(e != nullptr, "bad arguments");
    e->striped = on ? 0 : 1;
    return 0;
}
// on = 0: the per-graph attention forward stays a launch of its own (k_att_fwd_graph) instead of the tail of the last backbone layer's
// forward (Route::att_fwd_fold; what CAL_AMD_ATT_FWD_FOLD=0 selects process-wide).  Call before the first step is captured.
CAL_EXPORT int cal_engine_set_att_fwd_fold(void* h, int on) {
    Engine* e = (Engine*)h;
    CAL_REQUIRE(e != nullptr, "bad arguments");
    e->att_fwd_fold = on ? 1 : 0;
    return 0;
}
// on = 0: no step ends with k_finish_plan (what CAL_AMD_CHAIN=0 selects process-wide).  Call before a sequence is captured.
CAL_EXPORT int cal_engine_set_chain(void* h, int on) {
    Engine* e = (Engine*)h;
    CAL_REQUIRE(e != nullptr, "bad arguments");
    e->chain = on ? 1 : 0;
    return 0;
}
// Announce the batch of the step AFTER the coming cal_engine_step (same mode): that step may then end with ONE launch that commits it
// and plans this batch (k_finish_plan), and the step after it must be called for exactly this batch -- same pointers, sizes, layout
// (node_ptr / edge_ptr or the tiles' offsets + tile_gptr, the per-graph bounds) and workspace -- or it is refused.  Holds for one
// call; N = 0 withdraws it.  Whether the engine chains is its own decision (cal_engine_stage_name shows it).
CAL_EXPORT int cal_engine_set_next(void* h, const float* x0, const int64_t* edge_index, const int64_t* batch, int64_t N, int64_t E, int64_t B,
                                   const int64_t* node_ptr, const int64_t* edge_ptr, const int64_t* tile_gptr, int64_t ntiles,
                                   int64_t max_nodes, int64_t max_edges) {
    Engine* e = (Engine*)h;
    CAL_REQUIRE(e != nullptr && N >= 0 && E >= 0 && B >= 0 && ntiles >= 0 && max_nodes >= 0 && max_edges >= 0, "bad arguments");
    memset(&e->next, 0, sizeof(e->next));
    if (N == 0 || !x0 || !edge_index || !batch) return 0;
    e->next.x0 = x0; e->next.ei = edge_index; e->next.batch = batch; e->next.N = N; e->next.E = E; e->next.B = B;
    e->next.node_ptr = node_ptr; e->next.edge_ptr = edge_ptr; e->next.tile_gptr = ntiles > 0 ? tile_gptr : nullptr; e->next.ntiles = (int)ntiles;
    e->next.max_nodes = (int)std::min<int64_t>(max_nodes, 1 << 30); e->next.max_edges = (int)std::min<int64_t>(max_edges, 1 << 30);
    e->next.valid = 1;
    return 0;
}
// 1 while the latest step has planned its successor and that step is owed
CAL_EXPORT int64_t cal_engine_chain_pending(void* h) { Engine* e = (Engine*)h; return e && e->planned.valid ? 1 : 0; }
// Drop a planned step that will not be run (an error path).  The chain's counters never reached the bound tensors and the second
// arena is no longer clean: the next step zeroes its arena itself and nothing is chained until the workspace is set again.
CAL_EXPORT int cal_engine_chain_reset(void* h) {
    Engine* e = (Engine*)h;
    CAL_REQUIRE(e != nullptr, "bad arguments");
    if (e->planned.valid) { e->planned.valid = 0; e->chain_ok = 0; e->bn0_dirty_host = 1; }
    e->next.valid = 0;
    return 0;
}
// doubles of one fp64 arena (buffers "arena", "arena1")
CAL_EXPORT int64_t cal_engine_arena_doubles(void* h) { Engine* e = (Engine*)h; return e ? e->arena_n : 0; }
CAL_EXPORT int cal_engine_debug_stop(int k) { g_stop_after = k; return 0; }
// name of launch site k (1-based, as counted by cal_engine_debug_stop) in the latest untruncated step; "" past the end
CAL_EXPORT const char* cal_engine_stage_name(int k) {
    return k >= 1 && k <= (int)g_stage_names.size() ? g_stage_names[k - 1] : "";
}

// Test hooks of the node-level sparse kernels (tests/test_gpu_sparse_contract.py): a flat description is copied field by field
// into the kernels' own argument structs and handed to the launch code above.  No logic of their own, no twin in the host library.
//
// cal_sparse_probe_espmm -> launch_espmm.  All arrays in HOST memory; pointers inside pv are DEVICE pointers, 0 = null:
//   iv[0..5]          nnz, nbranch (1 or 2), relu, N, H, rpb
//   iv[6 + 2 b + ..]  branch b: 0 st_sum.stride, 1 st_sq.stride
//   pv[0..2]          CSR ptr, nbr, eid
//   pv[3 + 14 b + ..] branch b: 0 h, 1 out, 2 bias, 3 w, 4 dis, 5 st_sum.dst, 6 st_sum.parts, 7 st_sq.dst, 8 st_sq.parts,
//                     9 sd_z, 10 sd_gn, 11 sd_gself, 12 pb_g, 13 pb_batch
//   dv[0]             loop_w
// The width rule is cal_engine_create's; every other refusal is launch_espmm's own (return code 2, cal_last_error).
CAL_EXPORT int cal_sparse_probe_espmm(const int64_t* iv, void* const* pv, const double* dv, void* stream_) {
    CAL_REQUIRE(iv && pv && dv, "description missing");
    const int64_t nnz = iv[0], nbranch = iv[1], N = iv[3], H = iv[4], rpb = iv[5];
    CAL_REQUIRE(nbranch == 1 || nbranch == 2, "one or two branches");
    CAL_REQUIRE(H % 4 == 0 && H >= 4 && H <= 256, "hidden must be a multiple of 4 in [4, 256]");
    CAL_REQUIRE(N >= 1 && N < (1ll << 31) && nnz >= 0 && nnz < (1ll << 31) && rpb >= 1 && rpb < (1ll << 31), "sizes out of range");
    CSR csr;
    csr.ptr = (const int*)pv[0]; csr.nbr = (const int*)pv[1]; csr.eid = (const int*)pv[2]; csr.nnz = (int)nnz;
    SpmmBranch2 bb;
    for (int b = 0; b < 2; ++b) {
        const int64_t* ib = iv + 6 + 2 * std::min<int64_t>(b, nbranch - 1);
        void* const* pb = pv + 3 + 14 * std::min<int64_t>(b, nbranch - 1);        // one branch: both slots alike, as the engine fills them
        SpmmBranch& br = bb.b[b];
        br.h = (const float*)pb[0]; br.out = (float*)pb[1]; br.bias = (const float*)pb[2]; br.w = (const float*)pb[3];
        br.dis = (const float*)pb[4];
        br.st_sum = Acc((double*)pb[5], (double*)pb[6], (int)ib[0]);
        br.st_sq = Acc((double*)pb[7], (double*)pb[8], (int)ib[1]);
        br.sd_z = (const float*)pb[9]; br.sd_gn = (float*)pb[10]; br.sd_gself = (float*)pb[11];
        br.pb_g = (const float*)pb[12]; br.pb_batch = (const int64_t*)pb[13];
    }
    RC(launch_espmm((hipStream_t)stream_, csr, bb, (int)nbranch, (int)iv[2], (float)dv[0], (int)N, (int)H, (int)rpb));
    CAL_CHECK_LAUNCH("k_espmm(probe)");
    return 0;
}
// k_edge_att_deg exactly as fwd_att launches it, on a by-source CSR: att [2, E], dis_c / dis_o [N]
CAL_EXPORT int cal_sparse_probe_edge_att(const int* ptr, const int* nbr, const int* eid, int64_t nnz, const float* pq, const float* be,
                                         float* att, float* dis_c, float* dis_o, double loop_w, int64_t N, int64_t E, double fedge,
                                         void* stream_) {
    CAL_REQUIRE(ptr && nbr && eid && pq && be && att && dis_c && dis_o, "null argument");
    CAL_REQUIRE(N >= 1 && N < (1ll << 31) && E >= 0 && nnz >= 0 && nnz < (1ll << 31), "sizes out of range");
    CSR gs;
    gs.ptr = ptr; gs.nbr = nbr; gs.eid = eid; gs.nnz = (int)nnz;
    hipLaunchKernelGGL(k_edge_att_deg, dim3(cdiv(N, 32)), dim3(256), 0, (hipStream_t)stream_, gs, pq, be, att, dis_c, dis_o,
                       (float)loop_w, (int)N, E, (float)fedge);
    CAL_CHECK_LAUNCH("k_edge_att_deg(probe)");
    return 0;
}
// sel 0: launch_pool2 with cnt, 1: launch_pool2 without cnt, 2: launch_pool_cnt (batch, rpb_n), 3: nothing is launched.  *S_out =
// the row slices launch_pool2 cuts this batch into (slices: S x [4, B, H] floats when S > 1); sel 3 is how a caller sizes `slices`.
CAL_EXPORT int cal_sparse_probe_pool(int sel, const float* hc, const float* ho, const int* gptr, const int64_t* batch, float* pooled,
                                     float* cnt, float* slices, int64_t N, int64_t B, int64_t H, int64_t rpb_n, int64_t* S_out,
                                     void* stream_) {
    CAL_REQUIRE(sel >= 0 && sel <= 3 && S_out != nullptr, "bad selector");
    CAL_REQUIRE(H % 4 == 0 && H >= 4 && H <= 256, "hidden must be a multiple of 4 in [4, 256]");
    CAL_REQUIRE(N >= 1 && N < (1ll << 31) && B >= 1 && B < (1ll << 31), "sizes out of range");
    const int S = pool2_slices((int)N, (int)B);
    *S_out = S;
    if (sel == 3) return 0;
    CAL_REQUIRE(hc && ho && (sel == 2 ? batch != nullptr && cnt != nullptr && rpb_n >= 1 && rpb_n < (1ll << 31) : gptr != nullptr && pooled != nullptr),
                "null argument");
    if (sel == 2) return launch_pool_cnt((hipStream_t)stream_, hc, ho, batch, cnt, (int)N, (int)B, (int)H, (int)rpb_n);
    CAL_REQUIRE(S == 1 || slices != nullptr, "row slices without a slice buffer");
    return launch_pool2((hipStream_t)stream_, hc, ho, gptr, pooled, sel == 0 ? cnt : nullptr, slices, (int)N, (int)B, (int)H);
}
#ifdef CAL_BLK_CLOCKS
CAL_EXPORT int cal_debug_blk_clocks(long long* out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(cal::g_blk_clk), sizeof(long long) * 8192);
}
// marks 4 .. 7 (BLK_CLK_X); the ATT entry's copies of both buffers: cal_debug_blk_clocks_att (gconv_bwd_att.hip)
CAL_EXPORT int cal_debug_blk_clocks_x(long long* out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(cal::g_blk_clk_x), sizeof(long long) * 8192);
}
#endif
#ifdef CAL_RO_CLOCKS
CAL_EXPORT int cal_debug_ro_clocks(long long* out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(cal::g_ro_clk), sizeof(long long) * 64);
}
#endif

// Live timing (bench.py roofline): enable, run steps eagerly, synchronise, read.
CAL_EXPORT int cal_engine_profile(int on) {
    g_prof_on = on != 0;
    if (on) {
        for (auto& r : g_prof) { hipEventDestroy(r.e0); hipEventDestroy(r.e1); }
        g_prof.clear();
    }
    return 0;
}
// Fills out[3*i + {0,1,2}] = (class, milliseconds, algorithmic work: flops for class 0, bytes for
// class 1) for up to cap records; returns the number of records.  Call after a stream sync.
CAL_EXPORT int64_t cal_engine_profile_read(double* out, int64_t cap) {
    int64_t n = 0;
    for (auto& r : g_prof) {
        if (n >= cap) break;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.e0, r.e1) != hipSuccess) ms = -1.f;
        out[3 * n] = r.cls; out[3 * n + 1] = ms; out[3 * n + 2] = r.work;
        ++n;
    }
    return n;
}

// The layout of the latest step's k_finish launch (read-only; see Engine::fin_iv): writes up to cap / 3 triples
// (begin, end, kind) into out -- kind 0 = slab task, 1 = commit task, 2 = update-only Adam range -- and the step's final
// adam_in_finish (0 / 1 / 2 = k_adam followed behind an already advanced counter) into *adam_in_finish; returns the number
// of intervals the step had (-1: bad arguments).
CAL_EXPORT int64_t cal_engine_finish_layout(void* h, int64_t* out, int64_t cap, int64_t* adam_in_finish) {
    Engine* e = (Engine*)h;
    if (!e || (cap > 0 && !out)) return -1;
    for (int i = 0; i < e->fin_n && 3 * (int64_t)(i + 1) <= cap; ++i) {
        out[3 * i] = e->fin_iv[i].begin; out[3 * i + 1] = e->fin_iv[i].end; out[3 * i + 2] = e->fin_iv[i].kind;
    }
    if (adam_in_finish) *adam_in_finish = e->fin_adam;
    return e->fin_n;
}

// Adam alone (after an external gradient all-reduce)
CAL_EXPORT int cal_engine_adam(void* h, void* stream_) {
    Engine* e = (Engine*)h;
    hipStream_t st = (hipStream_t)stream_;
    RC(launch_adam(e, st, 0));
    hipLaunchKernelGGL(k_adam_tick, dim3(1), dim3(1), 0, st, e->step, (const int*)e->status);
    CAL_CHECK_LAUNCH("k_adam_tick");
    return 0;
}
// Adam after a gradient exchange when the step ran with mode bit 8 (its k_finish already advanced the step counter):
// ONE launch -- [graph: forward + backward] -> all-reduce(sum) -> this, with the 1/world mean folded into grad_scale
CAL_EXPORT int cal_engine_adam_ticked(void* h, void* stream_) {
    return launch_adam((Engine*)h, (hipStream_t)stream_, 1);
}
// ---- one-shot gradient exchange over peer-mapped memory (k_p2p_adam, engine_kernels.hpp) ------------------------------
// The regions must be FINE-GRAINED device memory: a kernel that polls a flag a peer GPU writes and then reads the peer's bucket
// while both kernels run needs stores that become visible across devices without a kernel boundary; coarse-grained hipMalloc
// memory (what torch allocates) promises that only at kernel boundaries (RCCL allocates its buffers the same way).
CAL_EXPORT int cal_p2p_alloc(int64_t bytes, void** out) {
    CAL_REQUIRE(bytes > 0 && out, "bad arguments");
    void* p = nullptr;
    hipError_t rc = hipExtMallocWithFlags(&p, (size_t)bytes, hipDeviceMallocFinegrained);
    if (rc != hipSuccess || !p) { (void)hipGetLastError(); set_error("cal_p2p_alloc: hipExtMallocWithFlags(fine-grained, %lld bytes): %s", (long long)bytes, hipGetErrorString(rc)); return 3; }
    rc = hipMemset(p, 0, (size_t)bytes);
    if (rc == hipSuccess) rc = hipDeviceSynchronize();
    if (rc != hipSuccess) { (void)hipGetLastError(); (void)hipFree(p); set_error("cal_p2p_alloc: zeroing failed: %s", hipGetErrorString(rc)); return 3; }
    *out = p;
    return 0;
}
CAL_EXPORT int cal_p2p_free(void* p) {
    if (p && hipFree(p) != hipSuccess) { (void)hipGetLastError(); set_error("cal_p2p_free failed"); return 3; }
    return 0;
}
// 64-byte IPC handle of a cal_p2p_alloc region (hipIpcGetMemHandle) / its mapping in another process (hipIpcOpenMemHandle)
CAL_EXPORT int cal_p2p_export(void* p, void* handle64) {
    CAL_REQUIRE(p && handle64, "bad arguments");
    static_assert(sizeof(hipIpcMemHandle_t) == 64, "IPC handle size");
    hipIpcMemHandle_t hd;
    hipError_t rc = hipIpcGetMemHandle(&hd, p);
    if (rc != hipSuccess) { (void)hipGetLastError(); set_error("cal_p2p_export: hipIpcGetMemHandle: %s", hipGetErrorString(rc)); return 3; }
    memcpy(handle64, &hd, 64);
    return 0;
}
CAL_EXPORT int cal_p2p_open(const void* handle64, void** out) {
    CAL_REQUIRE(handle64 && out, "bad arguments");
    hipIpcMemHandle_t hd;
    memcpy(&hd, handle64, 64);
    void* p = nullptr;
    hipError_t rc = hipIpcOpenMemHandle(&p, hd, hipIpcMemLazyEnablePeerAccess);
    if (rc != hipSuccess || !p) { (void)hipGetLastError(); set_error("cal_p2p_open: hipIpcOpenMemHandle: %s", hipGetErrorString(rc)); return 3; }
    *out = p;
    return 0;
}
CAL_EXPORT int cal_p2p_close(void* p) {
    if (p && hipIpcCloseMemHandle(p) != hipSuccess) { (void)hipGetLastError(); set_error("cal_p2p_close failed"); return 3; }
    return 0;
}
// Bytes of the region every rank allocates (cal_p2p_alloc: zero-initialised, its own allocation) and shares with the others.
CAL_EXPORT int64_t cal_engine_p2p_region_bytes(void* h) {
    Engine* e = (Engine*)h;
    const int64_t np = (e->nparam + 63) / 64 * 64;
    return (2 * np + 64) * 4;
}
// peer_bases[r]: device address, in THIS process, of rank r's region (its own at index `rank`); peer_devices[r]: the HIP device
// that owns it (peer access is enabled here when it is another device), or null when all regions live on the current device
CAL_EXPORT int cal_engine_p2p_bind(void* h, void* const* peer_bases, const int64_t* peer_devices, int64_t world, int64_t rank) {
    Engine* e = (Engine*)h;
    CAL_REQUIRE(e && e->P && world >= 1 && world <= P2P_MAX_WORLD && rank >= 0 && rank < world && peer_bases, "bad arguments (bind the parameters first; at most 8 ranks)");
    int dev = 0;
    hipGetDevice(&dev);
    memset(&e->p2p, 0, sizeof(e->p2p));
    for (int r = 0; r < world; ++r) {
        CAL_REQUIRE(peer_bases[r] != nullptr, "null peer region");
        e->p2p.region[r] = (float*)peer_bases[r];
        if (peer_devices && (int)peer_devices[r] != dev) {
            hipError_t rc = hipDeviceEnablePeerAccess((int)peer_devices[r], 0);
            if (rc != hipSuccess && rc != hipErrorPeerAccessAlreadyEnabled) { set_error("cal_engine_p2p_bind: no peer access to device %d", (int)peer_devices[r]); return 3; }
            (void)hipGetLastError();
        }
    }
    if (!e->p2p_host_status) {
        hipError_t rc = hipHostMalloc((void**)&e->p2p_host_status, 64, hipHostMallocMapped | hipHostMallocCoherent);
        if (rc != hipSuccess) { (void)hipGetLastError(); e->p2p_host_status = nullptr; set_error("cal_engine_p2p_bind: hipHostMalloc failed"); return 3; }
    }
    *e->p2p_host_status = 0;
    e->p2p.host_status = e->p2p_host_status; e->p2p.max_polls = e->p2p_max_polls;
    e->p2p.rank = (int)rank; e->p2p.world = (int)world; e->p2p.np = (e->nparam + 63) / 64 * 64;
    e->p2p_on = 1;
    return 0;
}
// Bound of the peer-flag wait in polls (~0.5-2 us each; default 2^22).  A launch ENQUEUED (or captured) after this call uses it.
CAL_EXPORT int cal_engine_p2p_set_timeout(void* h, int64_t max_polls) {
    Engine* e = (Engine*)h;
    CAL_REQUIRE(e && max_polls >= 1 && max_polls <= (1ll << 30), "bad arguments");
    e->p2p_max_polls = (int)max_polls; e->p2p.max_polls = (int)max_polls;
    return 0;
}
// The status words (this step's | the sticky earlier ones) as the latest COMPLETED training step left them: a host-mapped word the
// step's last kernel refreshes, so the loops can look at it before every step without a synchronisation -- a flagged batch
// (whose step updated nothing, and neither does any later one) surfaces a step or two later instead of at the end of the epoch.
CAL_EXPORT int64_t cal_engine_peek_status(void* h) {
    Engine* e = (Engine*)h;
    if (!e || !e->host_status) return 0;
    return (int64_t)__atomic_load_n(e->host_status, __ATOMIC_ACQUIRE);
}
// 0, or 64 once an exchange has timed out (the word is host-mapped: no device synchronisation, cheap enough for every step).
// After a timeout k_p2p_adam updates nothing any more; allocate fresh regions and bind again to resume.
CAL_EXPORT int64_t cal_engine_p2p_status(void* h) {
    Engine* e = (Engine*)h;
    if (!e || !e->p2p_host_status) return 0;
    return (int64_t)__atomic_load_n(e->p2p_host_status, __ATOMIC_ACQUIRE);
}
// The exchange + update of a step that ran with mode bit 8 (its last kernel advanced the Adam step counter): ONE launch.
// The gradient factor is cal_engine_set_grad_scale's (1 / world for the replicas' mean).
CAL_EXPORT int cal_engine_p2p_adam(void* h, void* stream_) {
    Engine* e = (Engine*)h;
    CAL_REQUIRE(e && e->p2p_on && e->ws, "cal_engine_p2p_bind first");
    const AdamArgs A{e->P, e->M1, e->M2, e->step, e->lr, e->beta1, e->beta2, e->eps, e->wd, e->grad_scale, 1};
    const int nb = (int)std::min<int64_t>(P2P_BLOCKS, cdiv(e->nparam, 256));
    hipLaunchKernelGGL(k_p2p_adam, dim3(nb), dim3(256), 0, (hipStream_t)stream_, e->p2p, e->G, A, e->nparam, e->status);
    CAL_CHECK_LAUNCH("k_p2p_adam");
    return 0;
}
// Model variants (opts.py:96-103 / model.py:24-31): cat = the random-intervention readout concatenates xc[perm] and xo
// (fc1_bn_co and fc1_co are 2H wide) instead of adding them; no_node_att / no_edge_att = the ablation flags (constant 0.5
// node / edge masks, no gradient into the corresponding attention MLP).  Call before cal_engine_bind.
CAL_EXPORT int cal_engine_set_options(void* h, int cat, int no_node_att, int no_edge_att) {
    Engine* e = (Engine*)h;
    CAL_REQUIRE(e != nullptr, "bad arguments");
    e->cat = cat ? 1 : 0; e->no_node_att = no_node_att ? 1 : 0; e->no_edge_att = no_edge_att ? 1 : 0;
    return 0;
}
// CausalGIN (model.py:166-264): the backbone layers are GINConv(Sequential(Linear, BatchNorm1d, ReLU, Linear, ReLU)) (model.py:188-194,
// eps = 0): per layer the slots {nn.1.weight, nn.1.bias, nn.0.weight, nn.0.bias, nn.3.weight, nn.3.bias} replace the four of a
// GCNConv layer in `offs`, and BatchNorm i of `bn_ptrs` is convs.(i-1).nn.1.  Call before cal_engine_bind.  The workspace buffer
// "ones" ([N] floats) must hold 1.0 (unit aggregation coefficients).
CAL_EXPORT int cal_engine_set_gin(void* h, int on) {
    Engine* e = (Engine*)h;
    CAL_REQUIRE(e != nullptr && (!on || e->K == 0), "bad arguments");
    e->gin = on ? 1 : 0;
    return 0;
}
// Random-intervention permutation drawn by the step itself (mode bit 16; model.py:147-152): keyed by (seed, *counter), the
// device counter advancing once per drawing step.  The drawn permutation is the workspace buffer "perm" (int64 [B]).
CAL_EXPORT int cal_engine_set_perm_rng(void* h, uint64_t seed, uint64_t* counter) {
    Engine* e = (Engine*)h;
    CAL_REQUIRE(e != nullptr, "bad arguments");
    e->perm_seed = seed; e->perm_ctr = (unsigned long long*)counter;
    return 0;
}
// Adam hyper-parameters after cal_engine_bind (an optimizer object's param group may change them between steps:
// torch.optim.Adam(params, lr, betas, eps, weight_decay), train_causal.py:21,76); the learning rate is the bound device float
CAL_EXPORT int cal_engine_set_adam(void* h, float beta1, float beta2, float eps, float weight_decay) {
    Engine* e = (Engine*)h;
    CAL_REQUIRE(e != nullptr && beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f && eps >= 0.f && weight_decay >= 0.f, "bad arguments");
    e->beta1 = beta1; e->beta2 = beta2; e->eps = eps; e->wd = weight_decay;
    return 0;
}
// Factor applied to the bound gradient buffer inside the Adam update (1/world_size turns the all-reduced SUM of the
// replicas' gradients into the mean, train_causal.py:187-192 semantics per replica); default 1
CAL_EXPORT int cal_engine_set_grad_scale(void* h, float scale) {
    Engine* e = (Engine*)h;
    CAL_REQUIRE(e != nullptr && scale > 0.f, "bad arguments");
    e->grad_scale = scale;
    return 0;
}
