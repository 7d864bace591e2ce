/* libcalhip -- C ABI of the MI355X (gfx950) kernels behind cal_amd.
 *
 * The reference (yongduosui/CAL) has no FFI: its hot path is Python calling
 * PyTorch-Geometric / torch_scatter operators.  Each entry point below replaces
 * one such operator call site (cited file:line, paths relative to the reference
 * root) and is what a binding of that path would bind (INTEGRATION.md shows the
 * ctypes stub).
 *
 * Conventions
 *  - every function returns 0 on success, non-zero on error; cal_last_error()
 *    returns the (thread-local) message of the last failure;
 *  - all pointers are DEVICE pointers owned by the caller (torch allocations),
 *    contiguous row-major; float buffers 16-byte aligned for the vector paths
 *    (unaligned / H % 4 != 0 inputs take a scalar path);
 *  - features fp32, reference indices int64 (edge_index, batch), plan indices
 *    int32;
 *  - `stream` is the hipStream_t to launch on (torch's current stream);
 *    functions only enqueue work: no allocation, no synchronisation, safe to
 *    capture in a hipGraph;
 *  - E = number of edges of the input edge_index (self loops included),
 *    N = nodes, H = feature width, B = graphs, K = heads, D = head width.
 */
#ifndef CAL_HIP_H
#define CAL_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CAL_API __attribute__((visibility("default")))

CAL_API const char* cal_last_error(void);
CAL_API int cal_version(void);
/* kernel launches this library has enqueued so far in this process (every launch site counts itself; memsets do not):
 * the difference around a call is the call's launch count */
CAL_API int64_t cal_launch_count(void);

/* ---- GraphPlan ---------------------------------------------------------------
 * COO -> CSR-by-destination and CSR-by-source with edge ids, explicit self loops
 * dropped (remove_self_loops, gcn_conv.py:56); the N loops add_self_loops
 * appends (gcn_conv.py:57-63) stay implicit.  work: 4*(N+1) + 4*E int32.  status: 1
 * int32, bit0 = edge index out of range, bit1 = batch not sorted/out of range. */
CAL_API int cal_plan_build(const int64_t* edge_index, int64_t E, int64_t N,
                           int32_t* rowptr_dst, int32_t* nbr_dst, int32_t* eid_dst,
                           int32_t* rowptr_src, int32_t* nbr_src, int32_t* eid_src,
                           int32_t* row32, int32_t* col32, int32_t* work, int32_t* status,
                           void* stream);
/* node offsets of each graph from the sorted `batch` vector (train_causal.py:174 batch object) */
CAL_API int cal_graph_ptr(const int64_t* batch, int64_t N, int64_t B, int32_t* gptr,
                          int32_t* status, void* stream);

/* ---- GCNConv (gcn_conv.py:44-104) ------------------------------------------ */
/* GCNConv.norm, gcn_conv.py:44-70 */
CAL_API int cal_gcn_norm_fwd(const int32_t* rowptr_src, const int32_t* eid_src,
                             const int32_t* row32, const int32_t* col32, const float* w,
                             float loop_w, int64_t N, int64_t E, float* dis, float* norm_e,
                             void* stream);
/* propagate + message + update (+ fused ReLU of model.py:95), gcn_conv.py:92-104 */
CAL_API int cal_spmm_fwd(const int32_t* rowptr, const int32_t* nbr, const int32_t* eid,
                         const float* norm_e, const float* dis, float loop_w, const float* h,
                         const float* bias, int relu, float* out, int64_t N, int64_t H,
                         void* stream);
CAL_API int64_t cal_colsum_parts(int64_t N);
/* ReLU backward + bias gradient (gcn_conv.py:103, model.py:95) */
CAL_API int cal_relu_bwd_colsum(const float* dout, const float* y, float* dz, float* dbias,
                                float* part, int64_t N, int64_t H, void* stream);
/* autograd of gcn_conv.py:63-70,97 w.r.t. edge_weight */
CAL_API int cal_gcn_norm_bwd(const int32_t* rowptr_dst, const int32_t* nbr_dst, const int32_t* eid_dst,
                             const int32_t* rowptr_src, const int32_t* nbr_src, const int32_t* eid_src,
                             const int32_t* row32, const int32_t* col32, const float* w,
                             const float* dis, float loop_w, const float* h, const float* dz,
                             float* gn_e, float* gself, float* ddeg, float* dw, int64_t N,
                             int64_t E, int64_t H, void* stream);

/* ---- dense linear layers on the matrix cores (fp32 MFMA) ----------------------
 * x @ W (gcn_conv.py:75), torch.nn.Linear (model.py:46-75) and their gradients.
 * C[M,N] = op(A) op(B) (+bias[N]) (ReLU); transA: A stored [K,M]; transB: B stored [N,K]. */
CAL_API int64_t cal_gemm_ws(int64_t M, int64_t N, int64_t K);
CAL_API int cal_gemm(int transA, int transB, const float* A, const float* B, float* C,
                     const float* bias, int relu, float* ws, int64_t M, int64_t N, int64_t K,
                     void* stream);

/* K-split (latency-oriented) variant, A not transposed, K <= 512 recommended */
CAL_API int cal_gemm_ks(int transB, const float* A, const float* B, float* C, const float* bias,
                        int relu, int64_t M, int64_t N, int64_t K, void* stream);

/* ---- causal / trivial soft masks (model.py:97-111) ------------------------- */
CAL_API int cal_edge_att_fwd(const float* x, const float* W, const float* b, const int32_t* row32,
                             const int32_t* col32, float* pq, float* att, int64_t N, int64_t E,
                             int64_t H, void* stream);
CAL_API int64_t cal_edge_att_bwd_ws(int64_t N, int64_t E, int64_t H);
CAL_API int cal_edge_att_bwd(const float* x, const float* W, const float* att, const float* datt,
                             const int32_t* rowptr_src, const int32_t* eid_src,
                             const int32_t* rowptr_dst, const int32_t* eid_dst, float* dx,
                             int accumulate, float* dW, float* db, float* ws, int64_t N, int64_t E,
                             int64_t H, void* stream);
CAL_API int cal_node_att_split_fwd(const float* x, const float* Wn, const float* bn, float* att_n,
                                   float* xc, float* xo, int64_t N, int64_t H, void* stream);
CAL_API int64_t cal_node_att_bwd_ws(int64_t N, int64_t H);
CAL_API int cal_node_att_split_bwd(const float* x, const float* Wn, const float* att_n,
                                   const float* dxc, const float* dxo, float* dx, float* dWn,
                                   float* dbn, float* ws, int64_t N, int64_t H, void* stream);

/* ---- global_add_pool (model.py:115-116, 403-404) --------------------------- */
CAL_API int cal_add_pool_fwd(const float* x, const int32_t* gptr, float* out, float* part,
                             int64_t B, int64_t H, int64_t S, void* stream);
CAL_API int cal_add_pool_bwd(const float* dout, const int64_t* batch, float* dx, int64_t N,
                             int64_t H, void* stream);

/* ---- GATConv (PyG, call sites model.py:340,390) ----------------------------- */
CAL_API int cal_gat_fwd(const int32_t* rowptr_dst, const int32_t* nbr_dst, const int32_t* eid_dst,
                        const float* z, const float* att, const float* bias, int relu, float slope,
                        float p, uint64_t seed, float* out, float* adst, float* asrc, float* mx,
                        float* den, int64_t N, int64_t E, int64_t K, int64_t D, void* stream);
CAL_API int64_t cal_gat_bwd_ws(int64_t N, int64_t E, int64_t K, int64_t D);
CAL_API int cal_gat_bwd(const int32_t* rowptr_dst, const int32_t* nbr_dst, const int32_t* eid_dst,
                        const int32_t* rowptr_src, const int32_t* nbr_src, const int32_t* eid_src,
                        const float* z, const float* att, const float* adst, const float* asrc,
                        const float* mx, const float* den, const float* gout, float slope, float p,
                        uint64_t seed, float* dz, float* datt, float* ws, int64_t N, int64_t E,
                        int64_t K, int64_t D, void* stream);
CAL_API int cal_gat_dropout_mask(uint64_t seed, int64_t E, int64_t N, int64_t K, float p,
                                 float* mask, void* stream);

/* ---- soft edge masks (cal_amd/gradient.py; csrc/softmask.hip, host twins in csrc_host/calhost.cpp) ------------------------
 * cal_edge_dot: out[e] = <a[col32[e], :], b[row32[e], :]> over H floats, exactly 0 for a self-loop column; a, b [N, H].  With
 * a = the upstream gradient and b = the input it is d/dw_e of GINConv's weighted sum (1 + eps) x_i + sum_{j -> i} w_ji x_j, whose
 * forward and dx are cal_spmm_fwd with norm_e = w, dis = 1, loop_w = 1 + eps (call site cal_amd/ops.py _GINWeightedAggregate).
 * E = 0 launches nothing.
 * cal_gat_mask_fwd / _bwd: cal_gat_fwd / cal_gat_bwd without dropout and with a mask m [E] >= 0 by column inside the edge softmax,
 * alpha_ij = m_ij exp(s_ij - max_i) / (sum_k m_ik exp(s_ik - max_i) + 1e-16), the added loop at weight 1, max_i over the loop and
 * the columns with m > 0 and a constant in the backward (call site cal_amd/ops.py _GATMaskAggregate).  The backward returns dz and
 * dm [E] (0 for a column outside the plan's CSR, i.e. an input self loop) and no d att: parameters are frozen on this path.
 * One general path: 1 <= K <= 64, any D >= 1, no alignment demand.  ws: cal_gat_mask_bwd_ws floats. */
CAL_API int cal_edge_dot(const int32_t* row32, const int32_t* col32, const float* a, const float* b, float* out,
                         int64_t N, int64_t E, int64_t H, void* stream);
CAL_API int cal_gat_mask_fwd(const int32_t* rowptr_dst, const int32_t* nbr_dst, const int32_t* eid_dst,
                             const float* z, const float* att, const float* bias, int relu, float slope,
                             const float* m, float* out, float* adst, float* asrc, float* mx, float* den,
                             int64_t N, int64_t E, int64_t K, int64_t D, void* stream);
CAL_API int64_t cal_gat_mask_bwd_ws(int64_t N, int64_t E, int64_t K, int64_t D);
CAL_API int cal_gat_mask_bwd(const int32_t* rowptr_dst, const int32_t* nbr_dst, const int32_t* eid_dst,
                             const int32_t* rowptr_src, const int32_t* nbr_src, const int32_t* eid_src,
                             const float* z, const float* att, const float* adst, const float* asrc,
                             const float* mx, const float* den, const float* gout, float slope,
                             const float* m, float* dz, float* dm, float* ws, int64_t N, int64_t E,
                             int64_t K, int64_t D, void* stream);

/* ---- learned masks (cal_amd/maskopt.py; csrc/maskopt.hip, host twin in csrc_host/calhost.cpp) ---------------------------------
 * cal_mask_step: one optimiser step over the mask logits of a batch in one launch.  The P players
 * are grouped by graph, pptr [B + 1]; player p owns mask element rep[p] and, for a twin pair, mate[p] (else -1), both indices
 * into the M elements in the caller's order.  With m = sigma(theta), P_g the graph's player count and step >= 1:
 *   g      = (grad[rep] + (mate >= 0 ? grad[mate] : 0) + l_size - (l_ent / P_g) theta) m (1 - m)       [= dL / dtheta]
 *   exp_avg    = beta1 exp_avg + (1 - beta1) g,   exp_avg_sq = beta2 exp_avg_sq + (1 - beta2) g^2
 *   theta -= lr / (1 - beta1^step) * exp_avg / (sqrt(exp_avg_sq) / sqrt(1 - beta2^step) + eps)
 * and sigma(theta_new) is written to mask[rep] and mask[mate]; every other mask entry is left alone.  terms [B, 2] (or null)
 * receives per graph sum_p m_p and sum_p H(m_p), H(m) = softplus(theta) - theta m, of the mask BEFORE the update, summed in
 * double in a fixed order; a graph without players gets 0, 0.  step == 0 updates nothing and does not read grad (may be null) or
 * the moments: mask and terms are written from the current theta (the initial scatter, the closing evaluation).
 * One workgroup per graph; no atomics, one writer per output element: equal inputs give equal bits.  Finite for any finite
 * theta.  pptr is clamped into [0, P], a rep / mate outside [0, M) is neither read nor written, B = 0 or P = 0 launches nothing.
 * No alignment demand beyond the elements' own. */
CAL_API int cal_mask_step(const int64_t* pptr, const int32_t* rep, const int32_t* mate, const float* grad,
                          float* theta, float* exp_avg, float* exp_avg_sq, float* mask, double* terms,
                          int64_t B, int64_t P, int64_t M, int32_t step, float lr, float beta1, float beta2,
                          float eps, float l_size, float l_ent, void* stream);

/* ---- parametric edge explainer (cal_amd/pgexplain.py; csrc/edgemlp.hip, host twins in csrc_host/calhost.cpp) ------------------
 * A two-layer MLP on the embeddings of an edge's end nodes, hidden width Hd (a multiple of 4, 4 to
 * 256).  pq [N, 2 Hd] holds the node projections P = x W1a^T + b1 (columns [0, Hd)) and Q = x W1b^T (columns [Hd, 2 Hd)), one
 * cal_gemm; w2 [Hd], b2 [1].  For a column e = (u -> v), u = row32[e], v = col32[e]:
 *   h_e[k] = pq[u, k] + pq[v, Hd + k],   omega(e) = b2 + sum_k w2[k] relu(h_e[k])
 * The P players are grouped by graph, pptr [B + 1]; player p owns column rep[p] and, for a twin pair, mate[p] (else -1):
 *   omega_p = (omega(rep) + omega(mate)) / 2 for a pair, omega(rep) otherwise.
 * cal_edge_mlp_fwd samples the concrete relaxation: seed == 0 gives z_p = omega_p / tau; otherwise, with splitmix64 as in
 * csrc/common.hpp and H(s, i) = splitmix64(splitmix64(s) + i),
 *   u_p = ((H(seed, step 2^32 + p) >> 41) + 0.5) 2^-23   (23 bits: exact in fp32, as 1 - u_p is, and never 0 or 1)
 *   z_p = (log u_p - log(1 - u_p) + omega_p) / tau
 * and writes omega [P], z [P] and m_p = sigma(z_p) to mask[rep] and mask[mate]; every other entry of mask [E] keeps its bits.
 * terms [B, 2] (or null) receives per graph sum_p m_p and sum_p H(m_p), H(m) = softplus(z) - z sigma(z), summed in double in a
 * fixed order; a graph without players gets 0, 0.  One launch, one workgroup per graph, a group of lanes per player (Hd / 4
 * lanes with 16-byte loads); no atomics.
 * cal_edge_mlp_bwd: with gmask [E] the gradient of the prediction loss with respect to mask, P_g the graph's player count,
 *   domega_p = (gmask[rep] + gmask[mate] + l_size - (l_ent / P_g) z_p) m_p (1 - m_p) / tau
 * a column's coefficient c_e is domega_p, halved on both columns of a pair, 0 for a column of no player, and
 *   dpq[u, k]      = sum_{e: row = u} c_e w2[k] [h_e[k] > 0]        dw2[k] = sum_e c_e relu(h_e[k])
 *   dpq[v, Hd + k] = sum_{e: col = v} c_e w2[k] [h_e[k] > 0]        db2    = sum_e c_e
 * The node sums run over two CSRs by source and by destination with the columns' ids (the plan's, or any that list every
 * player column once per view: the plan's leave out input self loops), one wave per row in slot order; h_e is recomputed; dw2
 * and db2 go through per-block partials and a fixed-order finish.  One memset and three launches; every row of dpq is written
 * (0 for a node without a player column); equal inputs give equal bits.  ws: cal_edge_mlp_bwd_ws floats.
 * Both: pptr is clamped into [0, P]; a player whose rep is outside [0, E) (or has an end node outside [0, N)) is skipped --
 * omega = z = 0 are written for it, it reaches neither mask nor terms nor any gradient, it still counts in P_g -- and such a mate
 * counts as no mate.  B = 0 or P = 0 launches nothing.  pq / w2 / dpq that are not 16-byte aligned take a scalar path. */
CAL_API int cal_edge_mlp_fwd(const float* pq, const float* w2, const float* b2, const int32_t* row32, const int32_t* col32,
                             const int64_t* pptr, const int32_t* rep, const int32_t* mate, float* omega, float* z,
                             float* mask, double* terms, int64_t N, int64_t E, int64_t Hd, int64_t B, int64_t P,
                             float tau, uint64_t seed, int64_t step, void* stream);
CAL_API int64_t cal_edge_mlp_bwd_ws(int64_t N, int64_t E, int64_t Hd);
CAL_API int cal_edge_mlp_bwd(const float* pq, const float* w2, const int32_t* row32, const int32_t* col32,
                             const int32_t* rowptr_src, const int32_t* eid_src, const int32_t* rowptr_dst,
                             const int32_t* eid_dst, const int64_t* pptr, const int32_t* rep, const int32_t* mate,
                             const float* z, const float* gmask, float* dpq, float* dw2, float* db2, float* ws,
                             int64_t N, int64_t E, int64_t Hd, int64_t B, int64_t P, float tau, float l_size,
                             float l_ent, void* stream);

/* ---- on-device mini-batch assembly (PyG DataLoader / Batch collate, train_causal.py:13-15,171-174)
 * over a device-resident concatenated dataset; offsets of the selected graphs computed by the host */
CAL_API int cal_collate(const float* X, const int64_t* EI, int64_t sumE, int64_t F,
                        const int64_t* node_ptr, const int64_t* edge_ptr, const int64_t* Y,
                        const int64_t* sel, const int64_t* out_node_off, const int64_t* out_edge_off,
                        float* xo, int64_t* eio, int64_t Eout, int64_t* batcho, int64_t* yo, int64_t B,
                        void* stream);

/* host-side batch assembly of a HOST-resident dataset (DataLoader / Batch collate, train_causal.py:13-15,171-174): X [Ntot, F],
 * EI [2, Etot] (edge ids local to their graph), node_ptr / edge_ptr [G + 1], Y [G]; graphs idx [B] -> xo [N, F], eio [2, Eout]
 * (rebased by the batch's node offsets), batcho [N], yo [B] in caller-owned staging memory.  Host pointers, no device work. */
CAL_API int cal_collate_host(const float* X, const int64_t* EI, int64_t Etot, int64_t F, const int64_t* node_ptr,
                             const int64_t* edge_ptr, const int64_t* Y, const int64_t* idx, int64_t B, float* xo,
                             int64_t* eio, int64_t Eout, int64_t* batcho, int64_t* yo);
/* host-side helper of the small-graph packing (cal_engine_set_tiles): first-fit-decreasing order of the B graphs of a
 * mini-batch under the tile bounds; order_out [B] positions, first_out [T + 1] first emitted graph of every tile; returns T
 * (-1: a graph exceeds a bound).  Host pointers, no device work. */
CAL_API int64_t cal_pack_order(const int64_t* node_sizes, const int64_t* edge_sizes, int64_t B, int64_t max_nodes,
                               int64_t max_edges, int64_t max_graphs, int64_t* order_out, int64_t* first_out);

/* ---- random-intervention permutation (model.py:147-152, `random.shuffle(range(num))`) drawn on the
 * device: perm[0..B) <- uniformly random permutation keyed by (seed, *counter); the kernel advances
 * *counter (a device uint64), so a replayed hipGraph draws a fresh permutation every step.  B <= 4096 */
CAL_API int cal_randperm(int64_t* perm, int64_t B, uint64_t seed, uint64_t* counter, void* stream);

/* CausalGAT (model.py:315-409): switch the engine's backbone layers to GATConv(H, H/heads, heads, dropout=p)
 * (PyG GATConv at model.py:340,390).  att_offs[i] = float offset of convs.i.att [heads, 2H/heads] in the bound
 * parameter buffer; seeds[i] = attention-dropout seed of layer i; ctr = device uint64 the engine advances once
 * per training step and folds into the seeds so a replayed hipGraph still draws fresh masks (NULL: seeds as given).
 * Call before cal_engine_workspace_bytes / cal_engine_set_workspace. */
CAL_API int cal_engine_set_gat(void* engine, int64_t heads, float p, float slope, const int64_t* att_offs,
                               const uint64_t* seeds, void* ctr);

/* ---- native CausalGCN step engine ------------------------------------------------
 * The whole train step of train_causal.py:173-192 on model.py:85-164 (forward, 3-term loss,
 * backward, Adam) as one call enqueuing a few dozen fused kernels (24 at BASELINE config 2); see cal_amd/csrc/engine.hip for the
 * slot order of `offs` / `bn_ptrs`.  mode bits: 1 = training-mode forward, 2 = loss gradient +
 * backward into the flat gradient buffer, 4 = Adam (applied inside the step's last kernel; the step counter is advanced by
 * its first one), 8 = Adam follows separately (cal_engine_adam_ticked),
 * 16 = draw the random-intervention permutation on the device inside the step's first kernel (`perm` ignored; cal_engine_set_perm_rng).  Outputs ("logp" [3,B,C], "stats" [7] =
 * loss, c_loss, o_loss, co_loss, correct_o, correct_c, correct_co: the hit counts eval_acc_causal needs, train_causal.py:214-218)
 * live in the caller-owned workspace at
 * cal_engine_buffer_offset(name) floats from its base. */
CAL_API void* cal_engine_create(int64_t F, int64_t H, int64_t C, int64_t L);
CAL_API void cal_engine_destroy(void* engine);
/* model variants (model.py:24-31,65-69,99-107): cat = cat_or_add "cat" (fc1_bn_co / fc1_co are 2H wide), no_node_att / no_edge_att =
 * without_node_attention / without_edge_attention (constant 0.5 masks).  Call before cal_engine_bind. */
CAL_API int cal_engine_set_options(void* engine, int cat, int no_node_att, int no_edge_att);
/* CausalGIN (model.py:166-264): GINConv(Sequential(Linear, BatchNorm1d, ReLU, Linear, ReLU)) backbone layers (model.py:188-194); per
 * layer the `offs` slots are {nn.1.weight, nn.1.bias, nn.0.weight, nn.0.bias, nn.3.weight, nn.3.bias}, BatchNorm i of `bn_ptrs` is
 * convs.(i-1).nn.1; the workspace buffer "ones" ([N] floats) must hold 1.0.  Call before cal_engine_bind. */
CAL_API int cal_engine_set_gin(void* engine, int on);
CAL_API int64_t cal_engine_num_param_slots(void* engine);
CAL_API int64_t cal_engine_num_bn(void* engine);
/* P / G / M1 / M2: flat parameter, gradient and Adam-moment buffers of `nparam` floats; offs[slot] = offset of a parameter in
 * them.  Keep every offset a multiple of 4 floats (16 bytes; cal_amd.trainer.flat_offsets pads with zeros, which Adam leaves
 * alone): batches of >= 16 384 nodes read the weight matrices with 16-byte loads and cal_engine_step fails with "operands of a
 * statistics GEMM must be 16-byte aligned" otherwise. */
CAL_API int cal_engine_bind(void* engine, float* P, float* G, float* M1, float* M2, float* step,
                            float* lr, int64_t nparam, const int64_t* offs, const int64_t* bn_ptrs,
                            float beta1, float beta2, float eps, float weight_decay);
CAL_API int64_t cal_engine_workspace_bytes(void* engine, int64_t N, int64_t E, int64_t B);
CAL_API int cal_engine_set_workspace(void* engine, void* ws, int64_t bytes, int64_t capN,
                                     int64_t capE, int64_t capB);
CAL_API int64_t cal_engine_buffer_offset(void* engine, const char* name);
CAL_API int cal_engine_step(void* engine, const float* x0, const int64_t* edge_index,
                            const int64_t* batch, const int64_t* y, const int64_t* perm, int64_t N,
                            int64_t E, int64_t B, float wc, float wo, float wco, int mode,
                            void* stream);
CAL_API int cal_engine_adam(void* engine, void* stream);
/* small-graph packing: the per-graph kernels run one workgroup per TILE of consecutive graphs (<= 64 nodes, <= 1024 edges,
 * <= 8 graphs); the tiles' node / edge offsets and bounds go through cal_engine_set_graph_ptrs / _set_graph_bounds, and
 * tile_gptr [ntiles + 1] (device int64) names the first graph of every tile.  Only global_add_pool (model.py:115-116) and its
 * backward distinguish the graphs of a tile.  ntiles = 0: one graph per workgroup. */
CAL_API int cal_engine_set_tiles(void* engine, const int64_t* tile_gptr, int64_t ntiles);
/* torch.optim.Adam's betas / eps / weight_decay (train_causal.py:21,76) after the bind, e.g. when an optimizer object that
 * owns them is attached to an engine-backed model (cal_amd/optim.py); the learning rate is the bound device float `lr` */
CAL_API int cal_engine_set_adam(void* engine, float beta1, float beta2, float eps, float weight_decay);
/* model.py:147-152 on the device, inside the step (mode bit 16): permutation keyed by (seed, *counter), as cal_randperm draws it;
 * the device counter advances once per drawing step, so a replayed hipGraph draws a fresh permutation.  B <= 1024. */
CAL_API int cal_engine_set_perm_rng(void* engine, uint64_t seed, uint64_t* counter);
/* data parallel (train_causal.py:187-192 per replica): cal_engine_step(mode = 1|2|8) runs forward + backward
 * and advances the Adam step counter, the caller all-reduces (sum) the bound gradient buffer, cal_engine_adam_ticked applies
 * the update in ONE launch with the gradient multiplied by cal_engine_set_grad_scale's factor (1 / world_size = mean) */
CAL_API int cal_engine_adam_ticked(void* engine, void* stream);
CAL_API int cal_engine_set_grad_scale(void* engine, float scale);
/* the same exchange WITHOUT a collective library (the ~0.5 MB bucket is latency-bound): every rank shares one
 * region (cal_engine_p2p_region_bytes, from cal_p2p_alloc: FINE-GRAINED device memory, zero-initialised -- coarse-grained
 * hipMalloc memory is not visible across devices inside a running kernel) with the others through IPC / xGMI peer mappings
 * (cal_p2p_export -> 64-byte handle -> cal_p2p_open in the peer process); cal_engine_p2p_adam is ONE launch that publishes the
 * bucket, waits for every rank's flag, sums in rank order and applies Adam.  peer_bases[r] / peer_devices[r]: rank r's region as
 * mapped in this process and the device that owns it.  If a peer's flag does not arrive within the timeout
 * (cal_engine_p2p_set_timeout, polls) NO parameter is updated in that or any later launch, status bit 64 is set and
 * cal_engine_p2p_status (a host-mapped word, no synchronisation) returns 64. */
CAL_API int cal_p2p_alloc(int64_t bytes, void** out);
CAL_API int cal_p2p_free(void* region);
CAL_API int cal_p2p_export(void* region, void* handle64);
CAL_API int cal_p2p_open(const void* handle64, void** out);
CAL_API int cal_p2p_close(void* mapped);
CAL_API int64_t cal_engine_p2p_region_bytes(void* engine);
CAL_API int cal_engine_p2p_bind(void* engine, void* const* peer_bases, const int64_t* peer_devices, int64_t world, int64_t rank);
CAL_API int cal_engine_p2p_set_timeout(void* engine, int64_t max_polls);
CAL_API int64_t cal_engine_p2p_status(void* engine);
/* status words (latest step | sticky) as of the latest completed training step: host-mapped mirror, no synchronisation
 * (train_causal.py:171-192 has no counterpart: the reference validates nothing; here a stale batch attribute must not train on
 * garbage silently) */
CAL_API int64_t cal_engine_peek_status(void* engine);
/* read-only view of the latest backward step's last launch (k_finish): up to cap / 3 triples (begin, end, kind) of the flat
 * parameter buffer -- kind 0: finished by a slab task, 1: by a commit task, 2: an update-only Adam range -- and
 * *adam_in_finish = 0 (the update is a launch of its own or absent), 1 (every element updated inside k_finish) or 2 (the
 * ranges did not fit: k_adam followed behind the already advanced step counter).  Returns the number of intervals. */
CAL_API int64_t cal_engine_finish_layout(void* engine, int64_t* out, int64_t cap, int64_t* adam_in_finish);
CAL_API int cal_engine_p2p_adam(void* engine, void* stream);
/* the 3-term loss of train_causal.py:176-183 on log-probabilities logp [3,B,C] (heads c, o, co) and labels y [B]:
 * out [4] = {loss, c_loss, o_loss, co_loss}; dlogp [3,B,C] (or null) = d loss / d logp, the input of cal_engine_backward_from.
 * flag (or null): bit 1 set when a label is outside [0, C).  One launch. */
CAL_API int cal_causal_loss(const float* logp, const int64_t* y, int64_t B, int64_t C, float wc, float wo, float wco, float* out,
                            float* dlogp, int32_t* flag, void* stream);
/* backward from an external d loss / d log-probs [3,B,C] of the last training-mode forward (autograd surface) */
CAL_API int cal_engine_backward_from(void* engine, const float* x0, const int64_t* batch,
                                     const float* dlogp, int64_t N, int64_t E, int64_t B, void* stream);
/* per-graph bounds of the coming batches (largest node count / edge count of a single graph; 0 = unknown):
 * when they fit, the step runs its per-graph fused convolution kernels (GEMM + aggregation + add-pool in
 * LDS); a violated bound sets bit 3 of the engine's status word */
CAL_API int cal_engine_set_graph_bounds(void* engine, int64_t max_nodes, int64_t max_edges);
/* layout of the coming batch as the collate knows it: node / edge ranges per graph ([B+1] int64 device arrays, graph
 * b owns the contiguous edge_index columns [edge_ptr[b], edge_ptr[b+1])) and no self loops; null = unknown.  With the
 * per-graph bounds this selects the one-kernel per-graph CSR build; violations are flagged in the status word */
CAL_API int cal_engine_set_graph_ptrs(void* engine, const int64_t* node_ptr, const int64_t* edge_ptr);
/* profiling aid: make cal_engine_step return after its k-th launch site (0 = run everything) */
/* Deterministic mode of one engine: every BatchNorm sum as fixed-order partial rows (no fp64 atomics): bit-reproducible steps.
 * No reference counterpart (torch.use_deterministic_algorithms is the closest notion); SURVEY.md section 7 "determinism". */
CAL_API int cal_engine_set_deterministic(void* engine, int on);
/* on = 0: the per-graph attention forward stays a launch of its own instead of the tail of the last GCN layer's forward launch
 * (k_gconv_fwd_att; the environment variable CAL_AMD_ATT_FWD_FOLD=0 selects the same process-wide).  No reference counterpart. */
CAL_API int cal_engine_set_att_fwd_fold(void* engine, int on);
/* Chained steps (k_finish_plan; no reference counterpart).  cal_engine_set_next announces the batch of the step AFTER the coming
 * cal_engine_step (same mode): that step may then end with ONE launch that commits it and builds the graph plan of this batch, and
 * the step after it must be called for exactly this batch (same pointers, sizes, layout and workspace) or it is refused with an
 * error and nothing is enqueued.  node_ptr / edge_ptr, tile_gptr / ntiles and the bounds are what cal_engine_set_graph_ptrs,
 * cal_engine_set_tiles and cal_engine_set_graph_bounds will be given for it.  The announcement holds for one call; N = 0 withdraws
 * it.  The engine chains only single-process Adam steps (mode bit 4) whose successor takes the 256-thread per-graph plan; otherwise
 * the steps run as ever.  cal_engine_set_chain(on = 0) / the environment variable CAL_AMD_CHAIN=0: never.  cal_engine_chain_pending:
 * 1 while a planned step is owed; cal_engine_chain_reset drops it (error paths: the chain's counters are lost with it).
 * cal_engine_arena_doubles: size of the fp64 arenas (buffers "arena", "arena1"; whoever sets the workspace zeroes "arena1"). */
CAL_API int cal_engine_set_chain(void* engine, int on);
CAL_API int cal_engine_set_next(void* engine, const float* x0, const int64_t* edge_index, const int64_t* batch, int64_t N, int64_t E,
                                int64_t B, const int64_t* node_ptr, const int64_t* edge_ptr, const int64_t* tile_gptr, int64_t ntiles,
                                int64_t max_nodes, int64_t max_edges);
CAL_API int64_t cal_engine_chain_pending(void* engine);
CAL_API int cal_engine_chain_reset(void* engine);
CAL_API int64_t cal_engine_arena_doubles(void* engine);
/* test aid: where BatchNorm k's batch sums live in the engine's fp64 arena (buffer "arena"), in doubles: out[0] offset of the column
 * sums (plane 0 of the four accumulator planes), out[1] padded width (the sums of squares follow that far behind), out[2] distance
 * of the planes.  BatchNorms in the order 0 bn_feat, 1..L bns_conv, L+1 bnc, L+2 bno, then the readout's. */
CAL_API int cal_engine_bn_arena(void* engine, int64_t k, int64_t* out);
CAL_API int cal_engine_debug_stop(int k);
/* test hook (csrc/gemm_probe.hip, GPU only): a flat description of a batched GEMM -- sizes and flags iv, device pointers pv,
 * doubles dv, all three HOST arrays laid out as the file's header comment says -- becomes a GemmArgs and goes to launcher
 * sel: 0 launch_gemm, 1 launch_gemm_ks, 2 launch_gemm_big alone, 3 launch_gemm_wres alone, 4 launch_gemm_dual (iv2 / pv2:
 * the TN set).  0 launched, 2 refused with a message, 3 an "alone" kernel declined.  Split-K slices stay slabs.
 * cal_gemm_probe_plan: out[6] (host) = split-K factor, slices, slice length, partial rows of launch_gemm and of
 * launch_gemm_ks, NSTRIPE -- what a caller needs to size its buffers */
CAL_API int cal_gemm_probe_plan(int64_t M, int64_t N, int64_t K, int nbatch, int hasC, int64_t* out);
CAL_API int cal_gemm_probe(int sel, const int64_t* iv, void* const* pv, const int64_t* iv2, void* const* pv2,
                           const double* dv, void* stream);
/* test hook (csrc/store_probe.hip, GPU only): one 32 x 32 accumulator tile whose element (row, col) holds the bits
 * 0x40000000 | row << 8 | col goes through gc_store_tile to buf[tile_off + row * ld + col], rows < nrow, with store policy
 * 0 (plain) or 1 (write-through; `bytes` = the extent from the tile's first word past which its stores are dropped).
 * 0 launched, 2 refused with a message (a tile or extent that leaves the buffer is refused, not launched). */
CAL_API int cal_probe_store_tile(int policy, float* buf, int64_t buf_words, int64_t tile_off, int nrow, int ld, int64_t bytes,
                                 void* stream);
/* test hooks (csrc/engine.hip, GPU only) of the node-level sparse kernels; the descriptions go field by field into the
 * kernels' own argument structs and to the engine's own launch code.  0 launched, 2 refused with a message.
 * cal_sparse_probe_espmm: launch_espmm.  HOST arrays iv (sizes, flags, strides), pv (DEVICE pointers, 0 = null) and
 * dv (loop_w), laid out as the comment above its definition says.
 * cal_sparse_probe_edge_att: k_edge_att_deg on a by-source CSR; att [2, E], dis_c / dis_o [N].
 * cal_sparse_probe_pool: sel 0 add-pool of both branches with positive counts, 1 without counts, 2 the counts alone from the
 * node -> graph map, 3 nothing is launched; *S_out = the row slices of the add-pool (slices: S x [4, B, H] floats when S > 1) */
CAL_API int cal_sparse_probe_espmm(const int64_t* iv, void* const* pv, const double* dv, void* stream);
CAL_API int cal_sparse_probe_edge_att(const int* ptr, const int* nbr, const int* eid, int64_t nnz, const float* pq, const float* be,
                                      float* att, float* dis_c, float* dis_o, double loop_w, int64_t N, int64_t E, double fedge,
                                      void* stream);
CAL_API int cal_sparse_probe_pool(int sel, const float* hc, const float* ho, const int* gptr, const int64_t* batch, float* pooled,
                                  float* cnt, float* slices, int64_t N, int64_t B, int64_t H, int64_t rpb_n, int64_t* S_out,
                                  void* stream);
/* test hooks (end of csrc/gat.hip, GPU only) of the GATConv kernels.  0 launched, 2 refused with a message.
 * cal_gat_probe_fwd / _bwd: cal_gat_fwd / cal_gat_bwd with the arguments those pin to null -- ctr (DEVICE; the step engine's
 * per-step counter: the mask seed becomes seed + *ctr * 0x9E3779B97F4A7C15 mod 2^64), and part_out (DEVICE,
 * [cal_gat_datt_parts(N)][2 K D] floats: the d att partial rows go there and datt is not written) + nparts (HOST, receives that
 * row count).
 * cal_gat_probe_ws_layout: out[4] (host) = float offsets of draw [(E + N) K], dadst [N K], dasrc [N K] and the d att partial
 * rows inside a cal_gat_bwd workspace.
 * cal_gat_probe_last_launch: name of the latest launch site this library passed ("k_gat_fwd_w", "k_gat_fwd_fused", ...).
 * cal_gat_probe_exp2: out[t] = exp2f(in[t]) (raw = 0), the bare v_exp_f32 (raw = 1) or expf(in[t]) (raw = 2, the two-pass
 * forward), the forms the kernels use. */
CAL_API int cal_gat_probe_fwd(const int32_t* rowptr_dst, const int32_t* nbr_dst, const int32_t* eid_dst,
                              const float* z, const float* att, const float* bias, int relu, float slope,
                              float p, uint64_t seed, const uint64_t* ctr, float* out, float* adst, float* asrc,
                              float* mx, float* den, int64_t N, int64_t E, int64_t K, int64_t D, void* stream);
CAL_API int cal_gat_probe_bwd(const int32_t* rowptr_dst, const int32_t* nbr_dst, const int32_t* eid_dst,
                              const int32_t* rowptr_src, const int32_t* nbr_src, const int32_t* eid_src,
                              const float* z, const float* att, const float* adst, const float* asrc,
                              const float* mx, const float* den, const float* gout, float slope, float p,
                              uint64_t seed, const uint64_t* ctr, float* dz, float* datt, float* ws, int64_t N,
                              int64_t E, int64_t K, int64_t D, float* part_out, int* nparts, void* stream);
CAL_API int cal_gat_probe_ws_layout(int64_t N, int64_t E, int64_t K, int64_t D, int64_t* out);
CAL_API int cal_gat_datt_parts(int64_t N);
CAL_API const char* cal_gat_probe_last_launch(void);
CAL_API int cal_gat_probe_exp2(const float* in, float* out, int64_t n, int raw, void* stream);
/* name of launch site k (1-based) of the latest untruncated cal_engine_step; "" past the end */
CAL_API const char* cal_engine_stage_name(int k);
/* live HIP-event timing of the node-level GEMMs (class 0, work = flops) and aggregations (class 1,
 * work = algorithmic bytes) inside the step, for bench.py's roofline block; `out` is a HOST array */
CAL_API int cal_engine_profile(int on);
CAL_API int64_t cal_engine_profile_read(double* out, int64_t cap);

/* ---- explanations of the causal split (model.py:97-111): per-segment ranking, top-k selection, motif metrics ------ */
/* Segment g = elements [seg_ptr[g], seg_ptr[g+1]) of score[i * stride] (stride 2 reads node_att[:, 1] in place), seg_ptr
 * [B+1] int64.  Order: score descending, then element index ascending, NaN below every number; rank[i] = 0-based position
 * in its segment; mask[i] = rank[i] < k_g with k_g = min(k, m_g) (k >= 0), min(m_g, ceil(ratio m_g)) (k = -1) or the
 * segment's count of gt elements (k = -2, needs gt).  metrics (or null): [B, 4] fp64 rows k_g, hits (gt selected), P (gt in
 * the segment), ROC-AUC from the ascending average ranks (NaN when P = 0 or P = m_g).  max_seg: host-known bound on every
 * m_g, it picks the paths (a longer segment is not ranked: rank -1, mask 0, NaN metrics); above cal_explain_lds_cap()
 * the call needs ws (16-byte aligned, cal_explain_ws bytes).  Every segment within the cap: one launch; else three. */
CAL_API int64_t cal_explain_ws(int64_t M, int64_t B);
CAL_API int64_t cal_explain_lds_cap(void);
CAL_API int cal_explain_rank(const float* score, int64_t stride, const int64_t* seg_ptr, int64_t B, int64_t M,
                             int64_t max_seg, double ratio, int64_t k, const uint8_t* gt, uint8_t* mask, int32_t* rank,
                             double* metrics, void* ws, int64_t ws_bytes, void* stream);

/* ---- subgraph extraction: a keep mask over a batch's edges / nodes -> the compacted batch, order preserved ---------- */
/* Graph g owns the nodes [ptr[g], ptr[g+1]) and the edge_index ([2, E] int64) columns [edge_ptr[g], edge_ptr[g+1]) (ptr,
 * edge_ptr: [B+1] int64).  edge_keep [E] / node_keep [N] uint8 or null; with `complement` each given mask is read inverted.
 * An edge is kept iff edge_keep (when given), both endpoints kept (when node_keep is given) and both endpoints inside its
 * graph's node range (an edge that leaves it is dropped).  relabel = 0: every node stays with its id (N' = N), x is not
 * copied.  relabel = 1: the kept nodes are node_keep when given, else the nodes incident to a kept edge; they are renumbered
 * densely in their original order, the endpoints rewritten, and row i of x_out [N, F] is row node_map[i] of x (x, x_out may be
 * null).  Kept elements keep their relative order and B is unchanged (a graph may keep no edge and, with relabel, no node).
 * Outputs, allocated at the bounds N / E: edge_index_out [2 E] (row 0 at [0, E'), row 1 at [E', 2 E'): a contiguous [2, E']),
 * ptr_out / edge_ptr_out [B+1], batch_out [N] (graph of every new node; may be null with relabel = 0), node_map [N] / edge_map
 * [E] (new element -> old element; node_map is the identity with relabel = 0 and may then be null) and totals [4] int64 on the
 * device: N', E', max_nodes', max_edges'.  Every integer output is uniquely determined.  ws: 8-byte aligned,
 * cal_subgraph_ws bytes.  Two launches on `stream`, no synchronisation; the caller reads totals back to slice the outputs. */
CAL_API int64_t cal_subgraph_ws(int64_t N, int64_t E, int64_t B);
CAL_API int cal_subgraph_extract(const int64_t* edge_index, int64_t E, int64_t N, const int64_t* ptr, const int64_t* edge_ptr,
                                 int64_t B, const uint8_t* edge_keep, const uint8_t* node_keep, int complement, int relabel,
                                 const float* x, int64_t F, int64_t* edge_index_out, int64_t* ptr_out, int64_t* edge_ptr_out,
                                 int64_t* batch_out, float* x_out, int64_t* node_map, int64_t* edge_map, int64_t* totals,
                                 void* ws, int64_t ws_bytes, void* stream);

/* ---- undirected explanations: the reverse-edge ("twin") map and the ranking of edge pairs -------------------------- */
/* Graph g owns the nodes [ptr[g], ptr[g+1]) and the edge_index ([2, E] int64) columns [edge_ptr[g], edge_ptr[g+1]), as in
 * cal_subgraph_extract.  Among the columns of g equal to (u, v), u != v, the j-th in ascending column order pairs with the
 * j-th column of g equal to (v, u): twin[e] (int32 [E]) is the partner's global column index, -1 when there is no j-th
 * partner.  A self loop is its own twin (twin[e] = e); a column with an endpoint outside its graph's node range gets -1 and
 * pairs with nothing.  So twin[twin[e]] == e wherever twin[e] >= 0, and the output is uniquely determined (duplicates
 * allowed).  totals [2] int64 on the device: columns with twin < 0, self loops.  max_edges: host-known bound on every
 * segment, it picks the paths (a longer segment gets -1 throughout).  ws: 8-byte aligned, cal_edge_twin_ws bytes.  Every
 * segment within cal_explain_lds_cap(): one launch; else three.  No read-back, no synchronisation, on `stream`; no value is
 * accumulated atomically (the one-launch path finds the workgroup that finishes last with a completion ticket, and that
 * workgroup sums the per-workgroup counts in order). */
CAL_API int64_t cal_edge_twin_ws(int64_t E, int64_t B);
CAL_API int cal_edge_twin(const int64_t* edge_index, int64_t E, const int64_t* ptr, const int64_t* edge_ptr, int64_t B,
                          int64_t max_edges, int32_t* twin, int64_t* totals, void* ws, int64_t ws_bytes, void* stream);
/* cal_explain_rank over undirected edges: the arguments of cal_explain_rank (segments = each graph's columns) plus `twin`
 * (as cal_edge_twin writes it; a column pairs with twin[e] iff that lies in its segment, differs from e and points back),
 * `reduce` (0 mean, 1 max, 2 min) and score_out [M].  The lower column of a pair represents it; unpaired columns and self
 * loops represent themselves; m'_g = representatives of g.  score_out[e], fp32: (s[e] + s[t]) * 0.5f, or the maximum /
 * minimum of the two (NaN if either is, as torch.maximum / torch.minimum); s[e] for an unpaired column.  The representatives
 * of a segment are ranked by that score descending, then column index ascending, NaN lowest; k_g = min(k, m'_g),
 * min(m'_g, ceil(ratio m'_g)) or the ground-truth representatives (one is ground truth iff either of its columns is); both
 * columns of a pair receive the representative's rank and mask.  metrics [B, 4]: k_g, hits, P, ROC-AUC over the
 * representatives.  A segment above max_seg is not ranked (rank -1, mask 0, NaN metrics; score_out is still written).  ws:
 * 16-byte aligned, cal_explain_pairs_ws bytes.  Two launches (symmetrise + compact, scatter) around cal_explain_rank's. */
CAL_API int64_t cal_explain_pairs_ws(int64_t M, int64_t B);
CAL_API int cal_explain_rank_pairs(const float* score, int64_t stride, const int64_t* seg_ptr, int64_t B, int64_t M,
                                   int64_t max_seg, double ratio, int64_t k, const uint8_t* gt, const int32_t* twin, int reduce,
                                   float* score_out, uint8_t* mask, int32_t* rank, double* metrics, void* ws, int64_t ws_bytes,
                                   void* stream);

/* ---- all-pairs intervention readout: the eval-mode `co` head (model.py:145-164) on every (objects row, trivial row) pair -----
 * xo [B, H], xc [M, H] (the bank of trivial rows: the batch's own or any other set); cat = cat_or_add "cat".  The head's
 * eval-mode parameters: fc1_bn_co (weight, bias, running mean, running var [Kin], eps), fc1_co ([H, Kin], [H]), fc2_bn_co ([H]),
 * fc2_co ([C, H], [C]); Kin = 2H with cat, else H.  logp(g, j) = log_softmax(fc2(bn2(relu(fc1(bn1(x)))))), x = xc_j + xo_g or
 * cat(xc_j, xo_g).  Outputs: p_do [B, C] = (1 / M) sum_j exp(logp(g, j)) (fp32 inside a chunk of 64 partners, fp64 across the
 * chunks); with ref [B] int64 (the class each graph is judged against): hits [B] int32 = #{j : argmax_c logp(g, j) == ref[g]} (the
 * lowest class on equal values), p_min [B] = min_j exp(logp(g, j)[ref[g]]), j_min [B] int32 = the lowest j attaining it; ref null
 * or ref[g] outside [0, C): hits 0, p_min NaN, j_min -1 (nothing to read back).  logp_pairs [B, M, C] or null (inspection, tests).
 * GPU: 1 <= H <= 256, 2 <= C <= 64 (the engine's limits), M >= 1, B, M bounded by memory; ws 16-byte aligned,
 * cal_intervene_ws bytes.  THREE launches (fold the parameters and form the two halves of fc1's pre-activation on the matrix
 * cores; the pair kernel; the chunk reduction in fixed order), no atomics, no synchronisation, no read-back: bit-reproducible and
 * safe to capture.  B = 0: nothing is launched.  The host library takes any sizes and needs no ws. */
CAL_API int64_t cal_intervene_ws(int64_t B, int64_t M, int64_t H, int64_t C);
CAL_API int cal_intervene_pairs(const float* xo, int64_t B, const float* xc, int64_t M, int64_t H, int64_t C, int cat,
                                const float* bn1_w, const float* bn1_b, const float* bn1_mean, const float* bn1_var, float bn1_eps,
                                const float* fc1_w, const float* fc1_b, const float* bn2_w, const float* bn2_b,
                                const float* bn2_mean, const float* bn2_var, float bn2_eps, const float* fc2_w,
                                const float* fc2_b, const int64_t* ref, float* p_do, int32_t* hits, float* p_min,
                                int32_t* j_min, float* logp_pairs, void* ws, int64_t ws_bytes, void* stream);

/* ---- batch splice: per pair the disjoint union of one graph of batch A and one graph of batch B ----------------------------
 * A batch is x [N, F] fp32 (or null, F = 0), edge_index [2, E] int64, ptr / edge_ptr [B+1] int64 as in cal_subgraph_extract; A and
 * B share F.  Result graph p (of P) is graph ga[p] of A followed by graph gb[p] of B; an entry outside [0, Ba) / [0, Bb) counts
 * as -1: that part is absent.  A source graph may appear in any number of pairs; Ba, Bb and P are independent.  Nodes of p: A's
 * nodes of ga[p] in their order, then B's nodes of gb[p].  Columns of p: A's columns of ga[p] in their order, then B's, then --
 * when bridge_a / bridge_b [P] (node ids of A / B, -1 for none; both null: no bridges) are both >= 0 and lie inside the node
 * ranges of ga[p] / gb[p] -- the two columns (a', b') and (b', a').  A source column with an endpoint outside its graph's node
 * range is dropped; endpoints are rewritten to the new numbering.  A pair with a bridge id >= 0 whose bridge is not written (an
 * id outside its part, a part absent, the other id -1) is counted in totals[5].  Every integer output is uniquely determined.
 *   cal_graph_splice_count: ONE launch.  ptr_out / edge_ptr_out [P+1] and totals [6] int64 on the device: N', E', max_nodes',
 *     max_edges', result graphs with no node, bridges asked for and not written.  The per-pair counts stay in ws.
 *   The caller reads totals back once and allocates the outputs exactly.
 *   cal_graph_splice_write: ONE launch, with the same inputs, the same ws (untouched since the count) and Nout = totals[0],
 *     Eout = totals[1].  batch_out [N'], x_out [N', F] (row copies; null with F = 0), edge_index_out (a contiguous [2, E']),
 *     node_src [N'] (the source node id, B's encoded as -1 - id) and edge_src [E'] (the source column in the same encoding,
 *     CAL_SPLICE_BRIDGE for a bridge column).  The rows are copied 16 bytes per lane when F % 4 == 0 and xa, xb, x_out are
 *     16-byte aligned, else element by element (0 <= F < 2^22).
 * ws: 8-byte aligned, cal_graph_splice_ws bytes.  Everything on `stream`, no synchronisation inside; no value that reaches an
 * output is accumulated atomically (the count finds the workgroup that finishes last with a completion ticket, as cal_edge_twin
 * does, and that workgroup scans the per-pair counts in order).  P = 0: nothing is launched (the count zeroes totals and the
 * two offsets with memsets). */
#define CAL_SPLICE_BRIDGE INT64_MIN
CAL_API int64_t cal_graph_splice_ws(int64_t Ea, int64_t Eb, int64_t P);
CAL_API int cal_graph_splice_count(const int64_t* eia, int64_t Ea, int64_t Na, const int64_t* ptr_a, const int64_t* eptr_a,
                                   int64_t Ba, const int64_t* eib, int64_t Eb, int64_t Nb, const int64_t* ptr_b,
                                   const int64_t* eptr_b, int64_t Bb, const int64_t* ga, const int64_t* gb, int64_t P,
                                   const int64_t* bridge_a, const int64_t* bridge_b, int64_t* ptr_out, int64_t* edge_ptr_out,
                                   int64_t* totals, void* ws, int64_t ws_bytes, void* stream);
CAL_API int cal_graph_splice_write(const int64_t* eia, int64_t Ea, int64_t Na, const int64_t* ptr_a, const int64_t* eptr_a,
                                   int64_t Ba, const int64_t* eib, int64_t Eb, int64_t Nb, const int64_t* ptr_b,
                                   const int64_t* eptr_b, int64_t Bb, const int64_t* ga, const int64_t* gb, int64_t P,
                                   const int64_t* bridge_a, const int64_t* bridge_b, const float* xa, const float* xb, int64_t F,
                                   const int64_t* ptr_out, const int64_t* edge_ptr_out, int64_t Nout, int64_t Eout,
                                   int64_t* batch_out, float* x_out, int64_t* edge_index_out, int64_t* node_src,
                                   int64_t* edge_src, void* ws, int64_t ws_bytes, void* stream);

/* ---- occlusion replicas: R copies of graphs of one batch, each with one element removed (cal_amd/occlude.py occlude_batch) ----
 * The batch is x [N, F] fp32 (or null, F = 0), edge_index [2, E] int64, ptr / edge_ptr [B+1] int64 as in cal_subgraph_extract.
 * Replica r (of R) is graph g = rep_graph[r]; an id outside [0, B) gives a replica with no node and no column.  rep_elem[r] is a
 * GLOBAL id of the batch.  mode 0 (edges): a column of g; all nodes of g stay in order, all columns of g stay in order except
 * rep_elem[r] and -- when twin (int32 [E], as cal_edge_twin writes it; or null) is given and twin[rep_elem[r]] >= 0 -- that twin
 * column (a self loop is its own twin: one column goes).  mode 1 (nodes): a node of g; its row is left out, later nodes move
 * down by one, every column incident to it is dropped and the remaining endpoints are rewritten.  In both modes a rep_elem[r]
 * that is no column / node of g (-1, say) removes nothing: the control replica.  A source column with an endpoint outside its
 * graph's node range is dropped, as in the splice.  Every integer output is uniquely determined.
 *   cal_occlude_count: ONE launch.  ptr_out / edge_ptr_out [R+1] and totals [5] int64 on the device: N', E', max_nodes',
 *     max_edges', replicas with no node.  The per-replica counts stay in ws.  The caller reads totals back once.
 *   cal_occlude_write: ONE launch with the same inputs, the same ws and Nout = totals[0], Eout = totals[1].  batch_out [N'],
 *     x_out [N', F] (row copies; null with F = 0), edge_index_out (a contiguous [2, E']), node_src [N'] / edge_src [E'] (the
 *     source node / column of every new one).  The rows are copied 16 bytes per lane when F % 4 == 0 and x, x_out are 16-byte
 *     aligned, else element by element (0 <= F < 2^22).
 * ws: 8-byte aligned, cal_occlude_ws bytes.  Everything on `stream`, no synchronisation inside; no value that reaches an output
 * is accumulated atomically (the completion ticket and the ordered scan of cal_graph_splice_count).  R = 0: nothing is launched
 * (the count zeroes totals and the two offsets with memsets). */
CAL_API int64_t cal_occlude_ws(int64_t E, int64_t R);
CAL_API int cal_occlude_count(const int64_t* edge_index, int64_t E, int64_t N, const int64_t* ptr, const int64_t* edge_ptr,
                              int64_t B, const int64_t* rep_graph, const int64_t* rep_elem, int64_t R, int mode,
                              const int32_t* twin, int64_t* ptr_out, int64_t* edge_ptr_out, int64_t* totals, void* ws,
                              int64_t ws_bytes, void* stream);
CAL_API int cal_occlude_write(const int64_t* edge_index, int64_t E, int64_t N, const int64_t* ptr, const int64_t* edge_ptr,
                              int64_t B, const int64_t* rep_graph, const int64_t* rep_elem, int64_t R, int mode,
                              const int32_t* twin, const float* x, int64_t F, const int64_t* ptr_out,
                              const int64_t* edge_ptr_out, int64_t Nout, int64_t Eout, int64_t* batch_out, float* x_out,
                              int64_t* edge_index_out, int64_t* node_src, int64_t* edge_src, void* ws, int64_t ws_bytes,
                              void* stream);

/* ---- rank agreement of two score vectors, per segment, in integers (cal_amd/occlude.py rank_agreement) ----------------------
 * a, b fp32 [M]; segment g is [seg_ptr[g], seg_ptr[g+1]).  An element takes part iff sel (uint8 [M] or null) marks it and
 * neither a nor b is NaN there; values compare as floats (-0 == +0).  k_code / k_val are cal_explain_rank's k / ratio
 * (k_code >= 0: top k; -1: ceil(k_val n)); there is no ground truth here.  counts [B, 10] int64 per segment:
 *   n (elements taking part), C (concordant pairs), D (discordant pairs), Ta (pairs with equal a, whatever b), Tb (pairs with
 *   equal b, whatever a: a pair tied in both counts in Ta and in Tb), Saa = sum (2ra)^2, Sbb = sum (2rb)^2, Sab = sum (2ra)(2rb)
 *   with 2r_i = 2 #{j: v_j < v_i} + #{j: v_j = v_i} + 1 the doubled mid-rank, k_g = min(k, n) or min(n, ceil(k_val n)), and
 *   inter = |top-k_g(a) & top-k_g(b)|, each top-k in cal_explain_rank's order (value descending, then element index).
 * A segment longer than max_seg gets n = -1 and zeros.  max_seg < 2^20, so every sum fits int64.  All sums are integers: the
 * result has the same bits on the GPU, in the host library and in any order of summation.  Segments within
 * cal_explain_lds_cap(): one launch, no ws.  Above it the j loop runs in LDS-sized tiles over a grid of row chunks whose
 * partial sums go through ws (8-byte aligned, cal_rank_agreement_ws bytes) and are added in order by a second small launch.
 * No atomics, no synchronisation, no read-back.  B = 0: nothing is launched. */
CAL_API int64_t cal_rank_agreement_ws(int64_t M, int64_t B, int64_t max_seg);
CAL_API int cal_rank_agreement(const float* a, const float* b, int64_t M, const int64_t* seg_ptr, int64_t B, int64_t max_seg,
                               const uint8_t* sel, int64_t k_code, double k_val, int64_t* counts, void* ws, int64_t ws_bytes,
                               void* stream);

/* ---- coalition replicas: R copies of graphs of one batch, each restricted to a subset of its elements (cal_amd/coalition.py
 * coalition_batch; sampled Shapley values, deletion / insertion curves) ----
 * The batch is x [N, F] fp32 (or null, F = 0), edge_index [2, E] int64, ptr / edge_ptr [B+1] int64 as in cal_occlude_*.  key is
 * int32 [K, M], row-major, one entry per edge column (mode 0, M = E) or per node (mode 1, M = N).  Replica r (of R) is graph
 * g = rep_graph[r]; an id outside [0, B) gives a replica with no node and no column.  Element e of g STAYS iff rep_row[r] is
 * outside [0, K) (the control replica: everything stays), or key[rep_row[r], e] < rep_thresh[r] with invert = 0, or
 * key[rep_row[r], e] >= rep_thresh[r] with invert = 1.  A plain integer compare: ties, negative keys and keys that are no
 * permutation all have a defined result.  mode 0 (edges): all nodes of g stay in order, the columns that stay keep their order.
 * mode 1 (nodes): the nodes that stay are renumbered densely in their order and their rows copied; a column stays iff both
 * endpoints stay, and its endpoints are rewritten.  In both modes a source column with an endpoint outside its graph's node
 * range is dropped, as in the splice and the occlusion.  max_nodes (< 2^31) must bound every graph's node count: in mode 1 it is
 * the row length of the per-replica node map in ws, and a graph with more nodes gives a replica with nothing in it.  Every
 * integer output is uniquely determined.
 *   cal_coalition_count: ONE launch.  ptr_out / edge_ptr_out [R+1] and totals [5] int64 on the device: N', E', max_nodes',
 *     max_edges', replicas with no node.  The per-replica counts and (mode 1) the node maps stay in ws.  The caller reads totals
 *     back once.
 *   cal_coalition_write: ONE launch with the same inputs, the same ws and Nout = totals[0], Eout = totals[1].  batch_out [N'],
 *     x_out [N', F] (row copies; null with F = 0), edge_index_out (a contiguous [2, E']), node_src [N'] / edge_src [E'] (the
 *     source node / column of every new one).  The rows are copied 16 bytes per lane when F % 4 == 0 and x, x_out are 16-byte
 *     aligned, else element by element (0 <= F < 2^22).
 * ws: 8-byte aligned, cal_coalition_ws bytes (16 R + 256, and 4 R max_nodes more in mode 1).  Everything on `stream`, no
 * synchronisation inside; no value that reaches an output is accumulated atomically (the completion ticket and the ordered scan
 * of cal_occlude_count).  R = 0: nothing is launched (the count zeroes totals and the two offsets with memsets). */
CAL_API int64_t cal_coalition_ws(int64_t E, int64_t R, int64_t max_nodes, int mode);
CAL_API int cal_coalition_count(const int64_t* edge_index, int64_t E, int64_t N, const int64_t* ptr, const int64_t* edge_ptr,
                                int64_t B, const int32_t* key, int64_t K, const int64_t* rep_graph, const int64_t* rep_row,
                                const int64_t* rep_thresh, int64_t R, int mode, int invert, int64_t max_nodes,
                                int64_t* ptr_out, int64_t* edge_ptr_out, int64_t* totals, void* ws, int64_t ws_bytes,
                                void* stream);
CAL_API int cal_coalition_write(const int64_t* edge_index, int64_t E, int64_t N, const int64_t* ptr, const int64_t* edge_ptr,
                                int64_t B, const int32_t* key, int64_t K, const int64_t* rep_graph, const int64_t* rep_row,
                                const int64_t* rep_thresh, int64_t R, int mode, int invert, int64_t max_nodes, const float* x,
                                int64_t F, const int64_t* ptr_out, const int64_t* edge_ptr_out, int64_t Nout, int64_t Eout,
                                int64_t* batch_out, float* x_out, int64_t* edge_index_out, int64_t* node_src,
                                int64_t* edge_src, void* ws, int64_t ws_bytes, void* stream);

/* ---- subset replicas: R copies of graphs of one batch, each restricted to an arbitrary subset of its elements given as a bitset
 * over the replica's OWN graph (cal_amd/counterfactual.py subset_batch; the counterfactual search) ----
 * The batch is x [N, F] fp32 (or null, F = 0), edge_index [2, E] int64, ptr / edge_ptr [B+1] int64 as in cal_coalition_*.  bits is
 * uint32 [K, W], row-major: bit j of a row (word j >> 5, bit j & 31) is LOCAL element j of the replica's graph g -- column
 * edge_ptr[g] + j in mode 0, node ptr[g] + j in mode 1.  Replica r (of R) is graph g = rep_graph[r]; an id outside [0, B) gives
 * a replica with no node and no column.  Its base set is row rep_row[r]; a row id outside [0, K) means EVERY element is present
 * (the control replica, and the only base with K = 0; bits may be null when K = 0 or W = 0).  A local index >= 32 W is absent.
 * Then rep_flip[r], a local index, is toggled (XOR): a cleared bit is set, a set bit cleared, an absent index >= 32 W becomes
 * present.  In mode 0, when twin (int32 [E], as cal_edge_twin writes it; or null) is given and twin[edge_ptr[g] + rep_flip[r]]
 * lies inside g's segment, that twin column is toggled too; a self loop is its own twin (toggled once).  A flip outside
 * [0, m), m the graph's element count, toggles nothing.  mode 0 (edges): all nodes of g stay in order, the columns whose bit is set after the toggle stay in
 * order.  mode 1 (nodes): the nodes that stay are renumbered densely in their order and their rows copied; a column stays iff
 * both endpoints stay, and its endpoints are rewritten.  In both modes a source column with an endpoint outside its graph's node
 * range is dropped, as everywhere.  max_nodes (< 2^31) must bound every graph's node count: in mode 1 it is the row length of the
 * per-replica node map in ws, and a graph with more nodes gives a replica with nothing in it.  Every integer output is uniquely
 * determined.
 *   cal_subset_count: ONE launch.  ptr_out / edge_ptr_out [R+1] and totals [5] int64 on the device: N', E', max_nodes',
 *     max_edges', replicas with no node.  The per-replica counts and (mode 1) the node maps stay in ws.  The caller reads totals
 *     back once.
 *   cal_subset_write: ONE launch with the same inputs, the same ws and Nout = totals[0], Eout = totals[1]: node workgroups, then
 *     one column workgroup per replica.  batch_out [N'], x_out [N', F] (row copies; null with F = 0), edge_index_out (a
 *     contiguous [2, E']), node_src [N'] / edge_src [E'] (the source node / column of every new one).  The rows are copied 16
 *     bytes per lane when F % 4 == 0 and x, x_out are 16-byte aligned, else element by element (0 <= F < 2^22).
 * ws: 8-byte aligned, cal_subset_ws bytes (16 R + 256, and 4 R max_nodes more in mode 1).  Everything on `stream`, no
 * synchronisation inside; no value that reaches an output is accumulated atomically (the completion ticket and the ordered scan
 * of cal_occlude_count).  R = 0: nothing is launched (the count zeroes totals and the two offsets with memsets). */
CAL_API int64_t cal_subset_ws(int64_t E, int64_t R, int64_t max_nodes, int mode);
CAL_API int cal_subset_count(const int64_t* edge_index, int64_t E, int64_t N, const int64_t* ptr, const int64_t* edge_ptr,
                             int64_t B, const uint32_t* bits, int64_t K, int64_t W, const int64_t* rep_graph,
                             const int64_t* rep_row, const int64_t* rep_flip, int64_t R, const int32_t* twin, int mode,
                             int64_t max_nodes, int64_t* ptr_out, int64_t* edge_ptr_out, int64_t* totals, void* ws,
                             int64_t ws_bytes, void* stream);
CAL_API int cal_subset_write(const int64_t* edge_index, int64_t E, int64_t N, const int64_t* ptr, const int64_t* edge_ptr,
                             int64_t B, const uint32_t* bits, int64_t K, int64_t W, const int64_t* rep_graph,
                             const int64_t* rep_row, const int64_t* rep_flip, int64_t R, const int32_t* twin, int mode,
                             int64_t max_nodes, const float* x, int64_t F, const int64_t* ptr_out,
                             const int64_t* edge_ptr_out, int64_t Nout, int64_t Eout, int64_t* batch_out, float* x_out,
                             int64_t* edge_index_out, int64_t* node_src, int64_t* edge_src, void* ws, int64_t ws_bytes,
                             void* stream);

/* ---- the beam step of the counterfactual search (cal_amd/counterfactual.py counterfactual) ----
 * Graph g's current states are the rows [g beam, g beam + n_state[g]) of bits (uint32 [B beam, W], bitsets as in cal_subset_*
 * over the segments seg_ptr [B+1] of M elements: edge_ptr / E in mode 0, ptr / N in mode 1), 1 <= beam <= 16, W <= 64.  Its
 * candidates are [cand_ptr[g], cand_ptr[g+1]) of R: candidate c is the state row rep_row[c] with the local index rep_flip[c]
 * toggled -- and, in mode 0 with twin (int32 [M] or null), the twin column, exactly as in cal_subset_* -- whose replica gave
 * p[c] = p(y^) and flipped[c] (uint8: its argmax is no longer y^).  A rep_row[c] that is none of g's live rows stands for the
 * FULL set: the bits [0, min(m, 32 W)) of g's m elements.  A flip outside [0, min(m, 32 W)) toggles nothing.  All integer:
 *   - done[g] != 0 or no candidate: n_state_out[g] = 0 and nothing else of g is written.
 *   - more than max_cand candidates (max_cand <= cal_explain_lds_cap()): status[g] = 2, n_state_out[g] = 0, nothing else.
 *   - else status[g] = 0.  The candidates are totally ordered by (flipped first, score_key(p) ascending -- the 32-bit key that
 *     orders like the floats with NaN below every number and -0 as +0 --, rep_row ascending, rep_flip ascending, then index).
 *     A candidate's child is its parent row with the flip applied.  Candidates with equal children (all W words) are ONE child,
 *     the earliest in the order stands.  If the first candidate is flipped: done[g] = 1, cf_bits[g] (uint32 [B, W]) its child,
 *     cf_p[g] its p, cf_cand[g] its index in [0, R), n_state_out[g] = 0.  Otherwise the first `beam` distinct children become the
 *     rows g beam, g beam + 1, .. of bits_out in that order, p_state_out [B beam] their p and n_state_out[g] their count.
 * No floating-point arithmetic: p is compared through its key and copied.  ONE launch, one workgroup per graph, the candidates'
 * keys and the parent rows in LDS; no atomics, no synchronisation, no read-back.  bits_out must not alias bits.  B = 0: nothing is
 * launched. */
CAL_API int cal_beam_step(const uint32_t* bits, int64_t B, int beam, int64_t W, const int64_t* n_state,
                          const int64_t* cand_ptr, const int64_t* rep_row, const int64_t* rep_flip, const float* p,
                          const uint8_t* flipped, int64_t R, const int64_t* seg_ptr, int64_t M, const int32_t* twin, int mode,
                          int64_t max_cand, uint8_t* done, uint32_t* bits_out, float* p_state_out, int64_t* n_state_out,
                          uint32_t* cf_bits, float* cf_p, int64_t* cf_cand, int32_t* status, void* stream);

/* ---- structural-noise replicas: R copies of graphs of one batch, each with random edges deleted and random edges inserted
 * (cal_amd/noise.py noise_batch; noise curves, explanation stability) ----
 * The batch is x [N, F] fp32 (or null, F = 0), edge_index [2, E] int64, ptr / edge_ptr [B+1] int64 as in cal_coalition_*.  Replica
 * r (of R) is graph g = rep_graph[r]; an id outside [0, B) gives a replica with no node and no column.  Let n be g's node count
 * and H(s, i) = splitmix64(splitmix64(s) + i), splitmix64(x): x += 0x9E3779B97F4A7C15; x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9;
 * x = (x ^ x >> 27) * 0x94D049BB133111EB; x ^ x >> 31 (all mod 2^64).  twin is int32 [E] as cal_edge_twin writes it, or null:
 *   null (directed): every column that is no self loop is its own player, an inserted edge is the one column (u, v);
 *   given (undirected): the player of column e is the lower column of its pair -- twin[e] when it lies inside g's segment and
 *   below e, else e itself -- as cal_explain_rank_pairs has it; an inserted edge is the two columns (u, v), (v, u), adjacent.
 * Deletion: with e_loc the index of a column's player inside g's segment, the column GOES iff it is no self loop and
 *   (H(rep_seed[r] ^ CAL_NOISE_C_DEL, e_loc) >> 1) < rep_del[r] (signed): both columns of a pair go together, rep_del <= 0 deletes
 *   nothing, rep_del = 2^63 - 1 all but surely everything, and the deletions at a smaller threshold are a subset of those at a
 *   larger one.  Self loops always stay; a column with an endpoint outside its graph's node range is dropped, as everywhere.
 * Insertion: a = max(rep_add[r], 0); candidate c = 0 .. tries a - 1 is the pair of local ids u = (h >> 32) mod n,
 *   v = (h & 0xffffffff) mod n with h = H(rep_seed[r] ^ CAL_NOISE_C_ADD, c).  It is ACCEPTABLE iff u != v and the source graph g
 *   has no column (u, v) -- undirected: nor (v, u) -- whether or not this replica deleted it; FRESH iff acceptable and no earlier
 *   candidate is the same pair (undirected: unordered).  The replica receives the first a fresh candidates in candidate order,
 *   after its surviving source columns (which keep their order); n <= 1 or a = 0 inserts nothing.  Freshness does not depend on
 *   a: for one seed the insertions at a smaller a are a prefix of those at a larger one, as long as neither falls short.
 * Every output is an integer or a row copy and is uniquely determined (the host library and a plain restatement agree bit for bit).
 *   cal_noise_count: ONE launch.  added [R] (the insertions made), ptr_out / edge_ptr_out [R+1] and totals [7] int64 on the
 *     device: N', E', max_nodes', max_edges', replicas with no node, the sum of added, replicas that fell short (added < a).  The
 *     per-replica counts and the accepted pairs stay in ws.  The caller reads totals back once.
 *   cal_noise_write: ONE launch with the same inputs, the same added and ws (untouched since the count) and Nout = totals[0],
 *     Eout = totals[1].  batch_out [N'], x_out [N', F] (row copies; null with F = 0), edge_index_out (a contiguous [2, E']),
 *     node_src [N'] / edge_src [E'] (the source node / column of every new one; edge_src = -1 for an inserted column).  The rows
 *     are copied 16 bytes per lane when F % 4 == 0 and x, x_out are 16-byte aligned, else element by element (0 <= F < 2^22).
 * ws: 8-byte aligned, cal_noise_ws(E, R, cand, tries) bytes (24 R + 256 + 8 ceil(cand / tries)) with cand a host-known bound on
 *   the sum over the replicas of tries a, both entry points given the same ws_bytes.  Every replica takes its run of a pairs
 *   from a counter in ws (an integer atomic; where a run lies depends on the order of the workgroups, no output does); under a
 *   bound that does not hold, a replica whose pairs would not fit is treated as asking for fewer, so that nothing is overrun.  1 <= tries <= 2^20, N < 2^31.  One workgroup per replica: source segments
 *   within cal_explain_lds_cap() columns keep the adjacency test and the de-duplication in an LDS hash set; larger ones (or more
 *   than 3072 source columns and insertions together) test every candidate against the segment's columns and the accepted pairs
 *   one by one.  Everything on `stream`, no synchronisation inside; no value that reaches an output is accumulated in an
 *   order-dependent way (the completion ticket and the ordered scan of cal_occlude_count).  R = 0: nothing is launched (the count
 *   zeroes totals and the two offsets with memsets). */
#define CAL_NOISE_C_DEL 0xA0761D6478BD642FULL
#define CAL_NOISE_C_ADD 0xE7037ED1A0B428DBULL
CAL_API int64_t cal_noise_ws(int64_t E, int64_t R, int64_t cand, int64_t tries);
CAL_API int cal_noise_count(const int64_t* edge_index, int64_t E, int64_t N, const int64_t* ptr, const int64_t* edge_ptr,
                            int64_t B, const int32_t* twin, const int64_t* rep_graph, const int64_t* rep_seed,
                            const int64_t* rep_del, const int64_t* rep_add, int64_t R, int64_t tries, int64_t* added,
                            int64_t* ptr_out, int64_t* edge_ptr_out, int64_t* totals, void* ws, int64_t ws_bytes, void* stream);
CAL_API int cal_noise_write(const int64_t* edge_index, int64_t E, int64_t N, const int64_t* ptr, const int64_t* edge_ptr,
                            int64_t B, const int32_t* twin, const int64_t* rep_graph, const int64_t* rep_seed,
                            const int64_t* rep_del, const int64_t* rep_add, int64_t R, int64_t tries, int64_t* added,
                            const float* x, int64_t F, const int64_t* ptr_out, const int64_t* edge_ptr_out, int64_t Nout,
                            int64_t Eout, int64_t* batch_out, float* x_out, int64_t* edge_index_out, int64_t* node_src,
                            int64_t* edge_src, void* ws, int64_t ws_bytes, void* stream);

/* ---- capped one-hot degree features (SPMotif's node feature, cal_amd/spmotif.py make_graph) ----
 * Row i of x_out [N, F] fp32 becomes zero except a 1 at min(d_i, F - 1), d_i the number of columns of edge_index [2, E] with row-0
 * endpoint i and row-1 endpoint != i (a column whose row-0 endpoint lies outside [0, N) counts for nobody).  The counts are
 * integers, so the order of accumulation cannot show.  F >= 1; E = 0 gives column 0; N = 0 launches nothing.  A memset and two
 * launches on `stream`, no ws, no synchronisation. */
CAL_API int cal_degree_onehot(const int64_t* edge_index, int64_t E, int64_t N, int64_t F, float* x_out, void* stream);

/* ---- Weisfeiler-Lehman colour refinement of a batch, and the WL subtree kernel of two batches (cal_amd/wl.py wl_refine /
 * wl_match; shape census of explanations) ----
 * The batch is edge_index [2, E] int64, ptr / edge_ptr [B+1] int64 as in cal_noise_*: graph g owns the nodes [ptr[g], ptr[g+1])
 * and the columns [edge_ptr[g], edge_ptr[g+1]).  A column COUNTS iff both endpoints lie inside g's node range; the others are
 * ignored and counted in totals[0] (summed over the graphs, whatever max_nodes).  Self loops and duplicates count, with
 * multiplicity.  All arithmetic is mod 2^64 and sm is the splitmix64 of the noise block above.  With init int64 [N] (null: 0
 * everywhere) and depth T >= 0:
 *   c_0[v] = sm(init[v] ^ CAL_WL_C_INIT)
 *   for t = 1 .. T:  out[v] = sum over the counted columns (v, w) of sm(c_{t-1}[w] ^ CAL_WL_C_OUT)
 *                    in[v]  = sum over the counted columns (w, v) of sm(c_{t-1}[w] ^ CAL_WL_C_IN)
 *                    c_t[v] = sm(sm(sm(c_{t-1}[v] + CAL_WL_C_SELF) + out[v]) + in[v])
 *   graph hash, cumulative over the depths: h = sm(n_g ^ CAL_WL_C_GRAPH); for t = 0 .. T:
 *                    h = sm(h + sum over v in g of sm(c_t[v] ^ CAL_WL_C_NODE)), hash[g, t] = h.
 * colors int64 [T+1, N] (row t = c_t), hash int64 [B, T+1], totals [1] int64 on the device; the int64s carry the uint64 bit
 * patterns: compare them for equality only.  Equal hashes mean "1-WL-equivalent up to a 64-bit collision", not "isomorphic".
 * A graph with more than max_nodes nodes gets hash 0 and colours 0.  Every output is uniquely determined: the sums are integer
 * sums, so the order of the integer atomics that form them (into LDS, or into ws) cannot show; the host library and a plain
 * restatement agree bit for bit.
 *   cal_wl_refine: a memset of totals and ONE launch on `stream`, one workgroup per graph for all T rounds, no read-back, no
 *   synchronisation.  Graphs within cal_explain_lds_cap() nodes keep both colour buffers and the two sum arrays in LDS and
 *   stream their columns from global memory every round; larger graphs (max_nodes above the cap) run the same rounds through
 *   the rows of colors and the two sum arrays in ws (8-byte aligned, cal_wl_ws(N, E, B) bytes; not read when max_nodes is
 *   within the cap).  B = 0: nothing is launched.  N = 0 with B > 0: every graph gets the hash of the empty graph.  E = 0 is
 *   legal.  0 <= T <= 4096.
 *   cal_wl_match: the WL subtree kernel of every graph of a batch A against every graph of a prototype batch P, from the two
 *   colors arrays (row strides stride_a / stride_p in elements, Na / Np nodes, ptr_a [A+1] / ptr_p [P+1]) of ONE refinement
 *   depth T:   K[a, p, t] = sum over w in p of #{v in a : c_t[v] == c_t[w]}   int64 [A, P, T+1]
 *              self_a[a, t] = sum over the colours of a at depth t of count^2  int64 [A, T+1].
 *   ONE launch, one workgroup per graph of A, integers only, no atomics, no ws.  Per depth a graph within the cap has its
 *   colours sorted in LDS (by counting); one wave per prototype looks its nodes up by binary search -- a colour's count is the
 *   length of its run -- and sums.  Above the cap every pair is compared.  A graph of A with more than max_nodes_a nodes gets
 *   zeros.  Np <= 4096, else an error.  A = 0 launches nothing; P = 0 writes self_a only. */
#define CAL_WL_C_INIT 0xD6E8FEB86659FD93ULL
#define CAL_WL_C_SELF 0xC2B2AE3D27D4EB4FULL
#define CAL_WL_C_OUT 0x165667B19E3779F9ULL
#define CAL_WL_C_IN 0x27D4EB2F165667C5ULL
#define CAL_WL_C_NODE 0x85EBCA77C2B2AE63ULL
#define CAL_WL_C_GRAPH 0xFF51AFD7ED558CCDULL
CAL_API int64_t cal_wl_ws(int64_t N, int64_t E, int64_t B);
CAL_API int cal_wl_refine(const int64_t* edge_index, int64_t E, int64_t N, const int64_t* ptr, const int64_t* edge_ptr,
                          int64_t B, const int64_t* init, int64_t T, int64_t max_nodes, int64_t* colors, int64_t* hash,
                          int64_t* totals, void* ws, int64_t ws_bytes, void* stream);
CAL_API int cal_wl_match(const int64_t* colors_a, int64_t stride_a, int64_t Na, const int64_t* ptr_a, int64_t A,
                         const int64_t* colors_p, int64_t stride_p, int64_t Np, const int64_t* ptr_p, int64_t P, int64_t T,
                         int64_t max_nodes_a, int64_t* K, int64_t* self_a, void* stream);

/* ---- exact motif matching: the embeddings of small connected patterns in every graph of a batch (cal_amd/motif.py
 * motif_match; what 1-WL cannot tell: does an explanation CONTAIN the motif, IS it the motif, WHERE does the motif sit) ----
 * The target batch is edge_index [2, E] int64, ptr / edge_ptr [B+1] int64 as in cal_wl_refine, on the device (the host library:
 * host memory), with optional labels int64 [N].  The pattern batch of P graphs has the same layout -- pat_edge_index [2, PE],
 * pat_ptr / pat_edge_ptr [P+1] -- but lives in HOST memory in both libraries: the launcher reads it, works out every pattern's
 * match order and passes the plans to the kernel by value, so the call neither copies nor synchronises.  pat_labels int64 [PN]
 * lies where labels lies.  labels and pat_labels are both null (no labels) or both given.
 *   Both sides are read as SIMPLE UNDIRECTED graphs: nodes u != w of a graph are adjacent iff a column (u, w) or (w, u) exists
 *   with both endpoints inside the graph's node range.  Self loops and duplicate columns add nothing.  A target column with an
 *   endpoint outside its graph is ignored and counted in totals[0] (summed over the graphs, larger ones included); such a
 *   pattern column is ignored.
 *   A pattern has 1 .. CAL_MOTIF_MAX_PATTERN nodes and is connected, and P <= CAL_MOTIF_MAX_PATTERNS (the plans travel as
 *   kernel arguments): otherwise the call returns an error and launches nothing.  A target graph of more than
 *   CAL_MOTIF_MAX_NODES nodes is skipped: count = -1, truncated = 0, first = -1, tgt_edges = -1.
 *   count[g, p] = the number of injective maps f: V(p) -> V(g) such that labels[f(i)] == pat_labels[i] (with labels), adjacent
 *   pattern nodes have adjacent images and, with induced = 1, non-adjacent pattern nodes have non-adjacent images.  So the count
 *   of a pattern in itself with induced = 1 is |Aut(p)|, and count / |Aut(p)| the number of distinct occurrences.
 *   Match order (positions 0 .. k-1): pi[0] is the pattern node of the largest degree, the lowest id on ties; every next node
 *   is the unplaced node with the most placed neighbours, the lowest id on ties; the PARENT of position d >= 1 is the earliest
 *   position whose node is adjacent to pi[d].
 *   Roots: a root is an ordered pair (u, w) of adjacent target nodes, the images of pi[0] and pi[1]; both labels are checked at
 *   the root.  A one-node pattern has no roots: its count is the number of label-compatible nodes.
 *   Steps: below a root, position d = 2 .. k-1 tries the neighbours v of the parent's image in ascending id, depth first.
 *   Every v tried costs one step, counted BEFORE any filter (v already used, its label, adjacency / non-adjacency to the images
 *   of the positions before d).  A root that would take step budget + 1 stops; the embeddings it found before still count.
 *   truncated[g, p] = the number of roots that stopped.  budget >= 0.
 *   first[g, p, i] = the image of pattern node i in the lexicographically smallest embedding found (compared as
 *   (f(0), f(1), ..)), a local id of graph g; -1 where there is none and for i >= k.  int32 [B, P, CAL_MOTIF_MAX_PATTERN].
 *   tgt_edges int64 [B] / pat_edges int64 [P]: the numbers of adjacent unordered pairs.  count, truncated int64 [B, P];
 *   totals int64 [1].  Every output is uniquely determined; the host library and a plain restatement agree bit for bit.
 *   A memset of totals and ONE launch on `stream`, one workgroup per target graph: the adjacency as a 256 x 256 bit matrix in
 *   LDS (built with integer OR-atomics, used for all P patterns), the roots dealt to the lanes, every lane's depth-first search
 *   in registers, integer sums and an unsigned 64-bit minimum (the embedding as eight bytes, pattern node 0 on top) over the
 *   workgroup.  No floating point, no read-back, no ws.  B = 0 or P = 0 launches nothing (pat_edges is then not written either:
 *   workgroup 0 writes it).  N = 0 and E = 0 are legal. */
#define CAL_MOTIF_MAX_PATTERN 8
#define CAL_MOTIF_MAX_NODES 256
#define CAL_MOTIF_MAX_PATTERNS 64
CAL_API int cal_motif_match(const int64_t* edge_index, int64_t E, int64_t N, const int64_t* ptr, const int64_t* edge_ptr,
                            int64_t B, const int64_t* labels, const int64_t* pat_edge_index, int64_t PE, int64_t PN,
                            const int64_t* pat_ptr, const int64_t* pat_edge_ptr, int64_t P, const int64_t* pat_labels,
                            int induced, int64_t budget, int64_t* count, int64_t* truncated, int32_t* first,
                            int64_t* tgt_edges, int64_t* pat_edges, int64_t* totals, void* stream);

/* ---- graph centralities: hop distances, Brandes' node and edge betweenness and PageRank of every graph of a batch
 * (cal_amd/centrality.py; the structure-only baselines of the explanations, the reference's `cent` features) ----
 * The batch is edge_index [2, E] int64, ptr / edge_ptr [B+1] int64 as in cal_motif_match, and the graph semantics are
 * cal_motif_match's: SIMPLE UNDIRECTED graphs -- nodes u != w of a graph are adjacent iff a column (u, w) or (w, u) exists with
 * both endpoints inside the graph's node range [ptr[g], ptr[g+1]); self loops and duplicate columns add nothing; a column with
 * an endpoint outside its graph is ignored and counted in totals[0] (over all graphs, skipped ones included); segments are
 * clamped as everywhere (seg_clamp).  n = the graph's nodes, d(u, v) the hop distance, R(v) the nodes v reaches (v included).
 *   far[v]   int64 [N]  sum of d(v, u) over u in R(v)
 *   reach[v] int64 [N]  |R(v)|
 *   ecc[v]   int64 [N]  max of d(v, u) over u in R(v)
 *   deg[v]   int64 [N]  the neighbours of v (distinct, v itself never)
 *   bc[v]    fp64  [N]  sum over the sources s != v of Brandes' dependency delta_s(v): RAW, twice networkx's unnormalised value
 *   ebc[e]   fp64  [E]  per COLUMN, in the caller's order: for the column (a, b) the sum over s of sigma_s(a) q_s(b) where b is
 *                       one level below a (d(s, b) = d(s, a) + 1), of sigma_s(b) q_s(a) where a is below b, with
 *                       q_s(u) = (1 + delta_s(u)) / sigma_s(u): RAW, twice networkx's unnormalised value.  A column, its reverse
 *                       and its duplicates carry the same value (the same sums of the same terms); a self loop and an ignored
 *                       column 0.
 *   pr[v]    fp64  [N]  PageRank: x_0 = 1/n; x_{t+1}[v] = alpha (sum over the neighbours u of x_t[u] / deg(u) + D_t / n) +
 *                       (1 - alpha) / n with D_t the sum of x_t over the nodes without a neighbour (dangling mass spread
 *                       uniformly, uniform teleport, uniform start: nx.pagerank of an undirected graph); iterate until
 *                       err_t = sum_v |x_{t+1}[v] - x_t[v]| < tol (NOT n tol) or max_iter steps are done.
 *   pr_iters int32 [B]  the steps taken, the one that met the test included; 0 for a graph without nodes or max_iter = 0
 *   hop[v]   int32 [N]  optional (null: not wanted): the distance to the nearest node u of the same graph with sources[u] != 0
 *                       (sources: bytes [N]); 0 on such a node, -1 where there is none within reach
 *   skipped  int64 [B]  1 for a graph of more than CAL_MOTIF_MAX_NODES nodes, else 0.  The device library skips such a graph:
 *                       its far, reach, ecc, deg, hop and pr_iters are -1, its bc, ebc (every column of its segment) and pr NaN.
 *                       The HOST library has no such limit (plain Brandes over a CSR, OpenMP over the graphs): skipped is 0.
 *   totals   int64 [1]  the ignored columns
 * pr_iters null: only hop is wanted, far .. pr are not touched; else all of them are given.  Nodes and columns outside every graph's segment are not
 * written.  alpha in [0, 1), tol >= 0, max_iter >= 0.
 *   Integers are exact, the same bits in both libraries.  Floating point is DETERMINISTIC: no floating-point atomic; every sum
 *   has one order, the same in both libraries (rules.hpp):
 *   - sigma_s(v) = the sum of sigma_s(u) over the neighbours u of v one level above, in ascending u; sigma_s(s) = 1;
 *   - delta_s(v) = the sum of sigma_s(v) * q_s(u) over the neighbours u one level below, in ascending u (one product per term);
 *   - source s belongs to wave s mod 4; a wave adds its sources' delta_s(v) (its columns' terms) in ascending s into one partial
 *     per node (per column); the value is ((p0 + p1) + p2) + p3;
 *   - pr: the neighbours' sum in ascending u; D_t and err_t are the tree sum cent_tree_sum of rules.hpp (slot i mod 256, halved).
 *   The two libraries are NOT promised to agree bit for bit in fp64 (the device build contracts a * b + c within a statement);
 *   both are within gamma_k of the exact value, k = 2 n (n + 3): every output is a sum of non-negative terms.
 *   One memset of totals and ONE launch on `stream`, one workgroup of 4 waves per graph: the bit matrix in LDS, the sources dealt
 *   to the waves, sigma / q / distances per wave in LDS, the nodes lane + 64 j of a lane in registers, frontiers and level masks
 *   by ballot.  The per-wave partials of ebc sit in LDS for a graph of at most CAL_CENTRALITY_LDS_COLS columns; a graph with
 *   more uses ws, [4, E] fp64: cal_centrality_ws(E) bytes, 0 for E <= CAL_CENTRALITY_LDS_COLS (no graph can have more).  No
 *   read-back.  B = 0 launches nothing.  N = 0 and E = 0 are legal. */
#define CAL_CENTRALITY_LDS_COLS 768
CAL_API int64_t cal_centrality_ws(int64_t E);
CAL_API int cal_centrality(const int64_t* edge_index, int64_t E, int64_t N, const int64_t* ptr, const int64_t* edge_ptr,
                           int64_t B, const uint8_t* sources, double alpha, double tol, int64_t max_iter, int64_t* far,
                           int64_t* reach, int64_t* ecc, int64_t* deg, double* bc, double* ebc, double* pr, int32_t* pr_iters,
                           int32_t* hop, int64_t* skipped, int64_t* totals, void* ws, int64_t ws_bytes, void* stream);

/* ---- nearest neighbours in embedding space: the pooled rows of pooled_representations (cal_amd/intervene.py) as queries and as
 * a bank; what torch.cdist + torch.topk spell, without the [nq, M] matrix and with a total order (cal_amd/neighbors.py: knn) ----
 *   Q        fp32  [nq, H]  the query rows
 *   X        fp32  [M, H]   the bank
 *   metric   0: squared Euclidean, max(0, |q|^2 + |x|^2 - 2 q.x); 1: cosine distance, 1 - q.x / (|q| |x|), 1 where either row
 *            has norm zero.  A non-finite distance counts as +inf, anything else not above zero as +0 (knn_clamp of rules.hpp).
 *   k        neighbours per query
 *   skip     int64 [nq] or null: the bank row that is not returned for query q (the query's own row when the bank holds it); a
 *            value outside [0, M) skips nothing
 *   labels   int64 [M] or null, C: the classes of votes; a label outside [0, C) is not counted
 *   idx      int32 [nq, k], dist fp32 [nq, k]: the k' = min(k, eligible rows) nearest rows of q in ascending order of the key
 *            (bits of dist as uint32) << 32 | idx -- the lower row first on equal distances; positions k' .. k - 1: -1 and +inf
 *   votes    int32 [nq, C] or null (needs labels): how many of the k' neighbours carry label c
 *   chunk_rows  0: the bank is cut by the plan knn_chunk_rows of rules.hpp (enough chunks that 32-query blocks x chunks cover
 *            the compute units); a positive multiple of 32: rows of a chunk.  The result does not depend on it.
 *   ws       16-byte aligned, cal_knn_ws bytes: nq x chunks x k keys of 8 bytes (+ 256), never of the order of nq x M
 * GPU: 1 <= H <= 256, 1 <= k <= 64, 1 <= M < 2^31, C <= 64, nq <= 65535 x 32.  TWO launches (distances on the matrix cores with the
 * selection of a chunk's k nearest behind them; the merge of a query's chunk lists with idx, dist and votes), no floating-point
 * atomic, no synchronisation, no read-back: the same bits on every call and under every chunking; safe to capture.  nq = 0:
 * nothing is launched.  The host library takes any sizes, forms the distances in fp64 and needs no ws (cal_knn_ws is 0). */
CAL_API int64_t cal_knn_ws(int64_t nq, int64_t M, int64_t k, int64_t chunk_rows);
CAL_API int cal_knn(const float* Q, int64_t nq, const float* X, int64_t M, int64_t H, int metric, int64_t k, const int64_t* skip,
                    const int64_t* labels, int64_t C, int32_t* idx, float* dist, int32_t* votes, int64_t chunk_rows, void* ws,
                    int64_t ws_bytes, void* stream);

/* ---- k-means on embedding rows: Lloyd's iterations over the [N, H] node rows of a dataset (cal_amd/concepts.py: kmeans, assign);
 * what torch.cdist(X, C).argmin(1) + index_add_ + bincount spell, with one read of the rows per iteration, no [N, K] matrix, a
 * total order and fixed summation orders (the kmeans block of rules.hpp) ----
 *   X        fp32  [N, H]   the rows
 *   C_in     fp32  [K, H]   the initial centroids (Cn of cal_kmeans_assign: the centroids of a concept table)
 *   iters    Lloyd iterations, >= 1
 *   span_rows  0: superblocks of kmeans_span(N, 0) rows (at most 512 of them); a positive multiple of 128: rows of a superblock
 *   C_out    fp32  [K, H]   the centroids after iters_run iterations; a cluster without rows keeps its centroid's bits
 *   assign   int32 [N]      the centroid of every row under the centroids the LAST iteration run started from: the smallest key
 *            (bits of the squared distance) << 32 | centroid -- the lower centroid on equal distances; -1 for a row whose
 *            distance to every centroid is non-finite (it enters no sum, no count, no inertia)
 *   dist     fp32  [N]      (cal_kmeans_assign) the squared distance to that centroid, +inf with -1
 *   counts   int64 [K]      rows of every cluster under assign
 *   inertia  fp64  [iters], moved int64 [iters]: per iteration the sum of the assigned rows' distances and the number of rows
 *            whose assignment changed (iteration 0: against -1 everywhere, i.e. the assigned rows).  Entries at and behind
 *            iters_run are not written.
 *   iters_run int32 [1]     iterations run: the first with moved == 0 is the last
 *   ws       16-byte aligned, cal_kmeans_ws bytes: per superblock K x H partial sums, K counts, an inertia, a moved count (+ 256)
 * Order of sums: a superblock's partial for (c, h) is one chain of fp32 additions in ascending row order, a cluster's sum the
 * partials in ascending superblock order, the mean one correctly rounded division.  Two calls give the same bits.  The bits of
 * C_out DO depend on span_rows (the order is part of the rule); the assignment of a single step does not.
 * GPU: 1 <= H <= 256, 1 <= K <= 64, 1 <= N < 2^31.  cal_kmeans launches exactly 2 x iters kernels (per iteration the step kernel,
 * one workgroup per superblock, and the update kernel, one thread per (c, h)); after the iteration with moved == 0 the remaining
 * launches read a flag in ws and return at once.  cal_kmeans_assign is ONE launch.  No floating-point atomic, no ticket, no
 * synchronisation, no read-back: safe to capture.  N = 0: nothing is launched.  The host library takes any sizes, forms the
 * distances in fp64, follows the same order of sums in fp32 and needs no ws (cal_kmeans_ws is 0). */
CAL_API int64_t cal_kmeans_ws(int64_t N, int64_t K, int64_t H, int64_t span_rows);
CAL_API int cal_kmeans_assign(const float* X, int64_t N, int64_t H, const float* Cn, int64_t K, int32_t* assign, float* dist,
                              void* stream);
CAL_API int cal_kmeans(const float* X, int64_t N, int64_t H, const float* C_in, int64_t K, int64_t iters, int64_t span_rows,
                       float* C_out, int32_t* assign, int64_t* counts, double* inertia, int64_t* moved, int32_t* iters_run,
                       void* ws, int64_t ws_bytes, void* stream);

/* ---- surrogate attributions: per graph ONE weighted least-squares fit of the replicas' values on the players' membership bits
 * (cal_amd/surrogate.py: surrogate_fit, kernel_shap, local_surrogate); what a padded [R, n_max] design matrix, a batched Gram
 * product and cholesky_solve spell, in fp64 with one order for every sum (the surrogate block of rules.hpp) ----
 *   key        int32 [K, M]  the key rows coalition_batch took
 *   rep_ptr    int64 [B + 1] the samples (replicas) of graph g: rep_ptr[g] .. rep_ptr[g + 1], clamped into [0, R]
 *   rep_row, rep_thresh int64 [R], rep_invert int64 [R] or null (zeros): sample s holds player p iff
 *              (key[rep_row[s], pl_elem[p]] < rep_thresh[s]) != (rep_invert[s] != 0); a row outside [0, K): every player
 *   value      fp64 [R]      v_s, the model's answer on the replica;  weight fp64 [R] or null (ones)
 *   pl_ptr     int64 [B + 1], pl_elem int64 [P]: the element of every player's representative, grouped by graph
 *   v_empty, v_full fp64 [B] (mode 0 only; mode 1 does not read them and takes null)
 *   mode       0 "shap": d = n unknowns, y = v - v_empty, the solution corrected onto sum(phi) = v_full - v_empty, phi0 = v_empty;
 *              n = 1 is defined as phi = v_full - v_empty.  1 "lime": d = n + 1, a free intercept as the last unknown (phi0),
 *              y = v, ridge on the n player entries of the diagonal only
 *   phi        fp64 [P], phi0 fp64 [B], r2 fp64 [B] (1 - SSR / SST, weighted; NaN when SST = 0)
 *   status     int32 [B]     0 fitted; 1 rank-deficient (a Cholesky pivot d_j <= 2^-30 A_jj); 2 more than 127 players (device
 *              library only); 3 a non-finite value, a negative or non-finite weight, a player outside [0, M) or (mode 0) a
 *              non-finite v_empty / v_full.  Precedence 2, 3, 1.  Non-zero: the graph's phi, phi0 and r2 are NaN.  A graph without
 *              a player is never 1: phi0 is v_empty (mode 0) or the weighted mean (mode 1, NaN without weight).
 * ONE launch, one workgroup of 256 threads per graph, the packed lower triangle (66 KB at d = 128) and a tile of 512 samples'
 * membership bits in LDS; no workspace, no read-back, no floating-point atomic: the same bits on every call, in any batch, and the
 * same bits as the host library (which has no player limit).  B = 0 launches nothing. */
CAL_API int cal_surrogate_fit(const int32_t* key, int64_t K, int64_t M, const int64_t* rep_ptr, const int64_t* rep_row,
                              const int64_t* rep_thresh, const int64_t* rep_invert, const double* value, const double* weight,
                              int64_t R, const int64_t* pl_ptr, const int64_t* pl_elem, int64_t P, int64_t B,
                              const double* v_empty, const double* v_full, int mode, double ridge, double* phi, double* phi0,
                              double* r2, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CAL_HIP_H */
