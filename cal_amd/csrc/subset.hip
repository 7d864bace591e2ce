// Subset replicas: the device operator behind cal_amd/counterfactual.py subset_batch (counterfactual search; the primitive of
// any sampler over arbitrary subsets of a graph's elements).
//
// cal_subset_count / cal_subset_write: replica r is graph g = rep_graph[r] of the batch restricted to the elements whose bit is
// set in row rep_row[r] of bits (uint32 [K, W]; bit j of a row is LOCAL element j of the replica's own graph: column
// edge_ptr[g] + j in mode 0, node ptr[g] + j in mode 1), after the local index rep_flip[r] -- and, in mode 0 with a twin map,
// its twin column -- has been toggled.  A row id outside [0, K) means every element is present; a local index >= 32 W is absent.
// A key row per replica over the whole batch (cal_coalition_*) costs R x E int32; here a replica costs three int64 and shares
// its row with every other replica of the same state.
//
// The rule is SubSrc of rules.hpp (sub_src, replica, node_stays, col_stays), which the host twin compiles too; the kernels and
// the launches are the restriction pair of restrict.hpp with the node map in ws.  This file is the two entry points' checks.
#include "restrict.hpp"

using namespace cal;

// the checks both entry points share (CAL_REQUIRE names the entry point)
#define SUBSET_REQUIRE_INPUTS()                                                                                                  \
    CAL_RESTRICT_REQUIRE_HEAD(E >= 0 && N >= 0 && B >= 0 && R >= 0 && K >= 0 && W >= 0);                                         \
    CAL_REQUIRE(W <= (1 << 26), "W must be <= 2^26");                                                                            \
    CAL_REQUIRE(max_nodes >= 0 && max_nodes <= 0x7FFFFFFF, "max_nodes must be in [0, 2^31)");                                    \
    CAL_REQUIRE(R == 0 || (rep_graph && rep_row && rep_flip), "rep_graph / rep_row / rep_flip are null");                        \
    CAL_REQUIRE(K == 0 || W == 0 || bits, "bits is null");                                                                       \
    CAL_RESTRICT_REQUIRE_TAIL(max_nodes, "ws must be 8-byte aligned and hold cal_subset_ws(E, R, max_nodes, mode) bytes");       \
    const SubSrc src = sub_src({edge_index, E, N, ptr, edge_ptr, B, rep_graph, mode}, bits, K, W, rep_row, rep_flip, twin, max_nodes)

CAL_EXPORT int64_t cal_subset_ws(int64_t, int64_t R, int64_t max_nodes, int mode) { return restrict_ws_need(R, max_nodes, mode); }

CAL_EXPORT int cal_subset_count(const int64_t* edge_index, int64_t E, int64_t N, const int64_t* ptr, const int64_t* edge_ptr,
                                int64_t B, const uint32_t* bits, int64_t K, int64_t W, const int64_t* rep_graph,
                                const int64_t* rep_row, const int64_t* rep_flip, int64_t R, const int32_t* twin, int mode,
                                int64_t max_nodes, int64_t* ptr_out, int64_t* edge_ptr_out, int64_t* totals, void* ws,
                                int64_t ws_bytes, void* stream) {
    SUBSET_REQUIRE_INPUTS();
    CAL_REQUIRE(totals && ptr_out && edge_ptr_out, "totals / ptr_out / edge_ptr_out are null");
    return restrict_count(__func__, src, R, ptr_out, edge_ptr_out, totals, ws, (hipStream_t)stream);
}

CAL_EXPORT int cal_subset_write(const int64_t* edge_index, int64_t E, int64_t N, const int64_t* ptr, const int64_t* edge_ptr,
                                int64_t B, const uint32_t* bits, int64_t K, int64_t W, const int64_t* rep_graph,
                                const int64_t* rep_row, const int64_t* rep_flip, int64_t R, const int32_t* twin, int mode,
                                int64_t max_nodes, const float* x, int64_t F, const int64_t* ptr_out,
                                const int64_t* edge_ptr_out, int64_t Nout, int64_t Eout, int64_t* batch_out, float* x_out,
                                int64_t* edge_index_out, int64_t* node_src, int64_t* edge_src, void* ws, int64_t ws_bytes,
                                void* stream) {
    SUBSET_REQUIRE_INPUTS();
    CAL_REBATCH_REQUIRE_WRITE(R, !x_out || (F > 0 && (N == 0 || x)), "x_out needs F > 0 and x", Eout > 0 ? R : 0);
    return restrict_write(src, R, x, ptr_out, edge_ptr_out,
                          write_out(Nout, Eout, batch_out, x_out, edge_index_out, node_src, edge_src, F, x), nb, eb, ws,
                          (hipStream_t)stream);
}
