// Coalition replicas: the device operator behind cal_amd/coalition.py (sampled Shapley values, deletion / insertion curves).
//
// cal_coalition_count / cal_coalition_write: replica r is graph g = rep_graph[r] of the batch restricted to a subset of its
// elements.  Graph g owns the nodes [ptr[g], ptr[g+1]) and the edge_index columns [edge_ptr[g], edge_ptr[g+1]).  key is int32
// [K, M] with one entry per edge column (mode 0, M = E) or per node (mode 1, M = N); element e of g stays iff rep_row[r] is outside
// [0, K) (the control replica: everything stays), or key[rep_row[r], e] < rep_thresh[r] (invert = 0), or key[rep_row[r], e] >=
// rep_thresh[r] (invert = 1): a plain integer compare, so ties, negative keys and keys that are no permutation all have a defined
// result, and the replicas of one key row at growing thresholds are nested.  Mode 0: all nodes of g stay, the columns that stay
// keep their order.  Mode 1: the nodes that stay are renumbered densely in their order, a column stays iff both endpoints stay
// and its endpoints are rewritten.  A graph id outside the batch gives a replica with nothing in it; a source column with an
// endpoint outside its graph's node range is dropped.  Every integer output is uniquely determined (the host twin and a
// plain-torch restatement agree bit for bit); the feature rows are copies.
//
// The rule is CoSrc of rules.hpp (co_src, replica, node_stays, col_stays), which the host twin compiles too; the kernels and the
// launches are the restriction pair of restrict.hpp with the node map in ws.  This file is the two entry points' checks.
#include "restrict.hpp"

using namespace cal;

// the checks both entry points share (CAL_REQUIRE names the entry point)
#define COALITION_REQUIRE_INPUTS()                                                                                               \
    CAL_RESTRICT_REQUIRE_HEAD(E >= 0 && N >= 0 && B >= 0 && R >= 0 && K >= 0);                                                   \
    CAL_REQUIRE(invert == 0 || invert == 1, "invert must be 0 or 1");                                                            \
    CAL_REQUIRE(max_nodes >= 0 && max_nodes <= 0x7FFFFFFF, "max_nodes must be in [0, 2^31)");                                    \
    CAL_REQUIRE(R == 0 || (rep_graph && rep_row && rep_thresh), "rep_graph / rep_row / rep_thresh are null");                    \
    CAL_REQUIRE(K == 0 || (mode == 0 ? E : N) == 0 || key, "key is null");                                                       \
    CAL_RESTRICT_REQUIRE_TAIL(max_nodes, "ws must be 8-byte aligned and hold cal_coalition_ws(E, R, max_nodes, mode) bytes");    \
    const CoSrc src = co_src({edge_index, E, N, ptr, edge_ptr, B, rep_graph, mode}, key, K, rep_row, rep_thresh, invert, max_nodes)

CAL_EXPORT int64_t cal_coalition_ws(int64_t, int64_t R, int64_t max_nodes, int mode) { return restrict_ws_need(R, max_nodes, mode); }

CAL_EXPORT int cal_coalition_count(const int64_t* edge_index, int64_t E, int64_t N, const int64_t* ptr, const int64_t* edge_ptr,
                                   int64_t B, const int32_t* key, int64_t K, const int64_t* rep_graph, const int64_t* rep_row,
                                   const int64_t* rep_thresh, int64_t R, int mode, int invert, int64_t max_nodes,
                                   int64_t* ptr_out, int64_t* edge_ptr_out, int64_t* totals, void* ws, int64_t ws_bytes,
                                   void* stream) {
    COALITION_REQUIRE_INPUTS();
    CAL_REQUIRE(totals && ptr_out && edge_ptr_out, "totals / ptr_out / edge_ptr_out are null");
    return restrict_count(__func__, src, R, ptr_out, edge_ptr_out, totals, ws, (hipStream_t)stream);
}

CAL_EXPORT int cal_coalition_write(const int64_t* edge_index, int64_t E, int64_t N, const int64_t* ptr, const int64_t* edge_ptr,
                                   int64_t B, const int32_t* key, int64_t K, const int64_t* rep_graph, const int64_t* rep_row,
                                   const int64_t* rep_thresh, int64_t R, int mode, int invert, int64_t max_nodes, const float* x,
                                   int64_t F, const int64_t* ptr_out, const int64_t* edge_ptr_out, int64_t Nout, int64_t Eout,
                                   int64_t* batch_out, float* x_out, int64_t* edge_index_out, int64_t* node_src,
                                   int64_t* edge_src, void* ws, int64_t ws_bytes, void* stream) {
    COALITION_REQUIRE_INPUTS();
    CAL_REBATCH_REQUIRE_WRITE(R, !x_out || (F > 0 && (N == 0 || x)), "x_out needs F > 0 and x", Eout > 0 ? R : 0);
    return restrict_write(src, R, x, ptr_out, edge_ptr_out,
                          write_out(Nout, Eout, batch_out, x_out, edge_index_out, node_src, edge_src, F, x), nb, eb, ws,
                          (hipStream_t)stream);
}
