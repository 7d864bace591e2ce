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
// The two launches follow the protocol of rebatch.hpp.  What is particular here:
//  * k_coalition_count: in mode 1 the graph's nodes are walked in chunks of one workgroup's threads and every node's new local
//    id -- the number of staying nodes in front of it, whether it stays or not -- goes to the replica's row of the node map in ws
//    (int32, max_nodes per replica: any graph size, nothing is staged in LDS); then the columns that stay are counted the same
//    way.
//  * k_coalition_write: in mode 1 a node workgroup finds the source node by binary search in the replica's map row, which is
//    non-decreasing, and a column workgroup rewrites the endpoints through the map row.  The map is read one launch after it was
//    written.
#include "rebatch.hpp"

namespace cal {
namespace {

struct CoArgs {
    const int64_t* ei;         // [2, E]
    int64_t E, N;
    const int64_t* ptr;        // [B + 1]
    const int64_t* eptr;       // [B + 1]
    int64_t B;
    const int32_t* key;        // [K, M], M = E (mode 0) or N (mode 1)
    int64_t K, M;
    const int64_t* rg;         // [R] graph of every replica (outside [0, B): none)
    const int64_t* rrow;       // [R] key row of every replica (outside [0, K): everything stays)
    const int64_t* rth;        // [R] threshold
    int64_t R;
    int mode, invert;          // 0 edges, 1 nodes; 0: key < threshold stays, 1: key >= threshold stays
    int64_t mx;                // (mode 1) the map's row length: bounds every graph's node count
    int64_t* ptr_out;          // [R + 1]
    int64_t* eptr_out;         // [R + 1]
    int64_t* totals;           // [5]
    int64_t* cnt;              // ws [2 R]: nodes, columns of every replica
    int32_t* map;              // ws [R, mx] (mode 1): staying nodes in front of every node of the replica's graph
    const float* x;            // (write) [N, F] or null
    WriteOut out;              // (write)
    int ticket, nblk;
};

// (CoRep, co_replica, elem_stays, col_stays: rules.hpp)

// grid R, NT threads
template <int NT>
__global__ void __launch_bounds__(NT) k_coalition_count(CoArgs a) {
    __shared__ long long red[NT / 64];
    __shared__ int wcnt[NT / 64];
    __shared__ int last;
    const int64_t r = blockIdx.x, R = a.R;
    const CoRep q = co_replica(a, r);
    int64_t nodes = q.nn;
    if (a.mode == 1) {                                            // the map row: q.nn <= a.mx (co_replica()), uniform over the workgroup
        int32_t* row = a.map + r * a.mx;
        nodes = 0;
        for (int64_t base = 0; base < q.nn; base += NT) {
            const int64_t l = base + threadIdx.x;
            const bool f = l < q.nn && elem_stays(a, q, q.nlo + l);
            int t;
            const int pos = wg_excl<NT>(f, wcnt, t);
            if (l < q.nn) row[l] = (int32_t)(nodes + pos);
            nodes += t;
        }
    }
    long long c = 0;
    for (int64_t t = threadIdx.x; t < q.em; t += NT) c += col_stays(a, q, q.elo + t);
    const int64_t kept = wg_sum<NT>(c, red);
    if (threadIdx.x == 0) {
        a.cnt[r] = nodes;
        a.cnt[R + r] = kept;
    }
    if (last_workgroup(a.ticket, a.nblk, &last)) scan_counts<NT>(a.cnt, a.cnt + R, R, a.ptr_out, a.eptr_out, a.totals, red);
}

// grid ceil(Nout / kNodeChunk) node workgroups, then R column workgroups; 256 threads
__global__ void __launch_bounds__(256) k_coalition_write(CoArgs a, int node_blocks) {
    __shared__ int64_t src[kNodeChunk];
    __shared__ int wcnt[4];
    if ((int)blockIdx.x < node_blocks) {
        write_nodes(
            a.out, a.ptr_out, a.R, -1, src,
            [&](int64_t r, int64_t l) -> int64_t {
                const CoRep q = co_replica(a, r);
                if (a.mode == 1 && q.nn > 0) l = owner(a.map + r * a.mx, q.nn, l);
                return l < q.nn ? q.nlo + l : -1;
            },
            [&](int64_t s) { return a.x + s * a.out.F; });
        return;
    }
    const int64_t r = (int64_t)((int)blockIdx.x - node_blocks);
    const CoRep q = co_replica(a, r);
    const int32_t* row = a.mode == 1 ? a.map + r * a.mx : nullptr;
    write_cols(
        a.out, a.ptr_out, a.eptr_out, r, a.ei, a.E, q.elo, q.em, wcnt,
        [&](int64_t e) { return col_stays(a, q, e); },
        [&](int64_t u) { return row ? (int64_t)row[u - q.nlo] : u - q.nlo; });   // (u inside [nlo, nlo + nn): col_stays)
}

int64_t co_ws_need(int64_t R, int64_t max_nodes, int mode) {
    R = R > 0 ? R : 0;
    return 16 * R + (mode == 1 ? 4 * R * (max_nodes > 0 ? max_nodes : 0) : 0) + 256;
}

// the checks both entry points share (CAL_REQUIRE names the entry point)
#define COALITION_REQUIRE_INPUTS()                                                                                               \
    CAL_REQUIRE(E >= 0 && N >= 0 && B >= 0 && R >= 0 && K >= 0, "sizes must be >= 0");                                           \
    CAL_REQUIRE(R <= 0x7FFFFFFF, "too many replicas");                                                                           \
    CAL_REQUIRE(mode == 0 || mode == 1, "mode must be 0 (edges) or 1 (nodes)");                                                  \
    CAL_REQUIRE(invert == 0 || invert == 1, "invert must be 0 or 1");                                                            \
    CAL_REQUIRE(max_nodes >= 0 && max_nodes <= 0x7FFFFFFF, "max_nodes must be in [0, 2^31)");                                    \
    CAL_REQUIRE(R == 0 || (rep_graph && rep_row && rep_thresh), "rep_graph / rep_row / rep_thresh are null");                    \
    CAL_REQUIRE(K == 0 || (mode == 0 ? E : N) == 0 || key, "key is null");                                                       \
    CAL_REQUIRE(B == 0 || (ptr && edge_ptr), "ptr / edge_ptr are null");                                                         \
    CAL_REQUIRE(E == 0 || edge_index, "edge_index is null");                                                                     \
    CAL_REQUIRE(R == 0 || (ws && ws_bytes >= co_ws_need(R, max_nodes, mode) && (reinterpret_cast<uintptr_t>(ws) & 7) == 0),      \
                "ws must be 8-byte aligned and hold cal_coalition_ws(E, R, max_nodes, mode) bytes")

CoArgs co_args(const int64_t* edge_index, int64_t E, int64_t N, const int64_t* ptr, const int64_t* edge_ptr, int64_t B,
               const int32_t* key, int64_t K, const int64_t* rep_graph, const int64_t* rep_row, const int64_t* rep_thresh,
               int64_t R, int mode, int invert, int64_t max_nodes, void* ws) {
    CoArgs a{};
    a.ei = edge_index;
    a.E = E;
    a.N = N;
    a.ptr = ptr;
    a.eptr = edge_ptr;
    a.B = B;
    a.key = key;
    a.M = mode == 0 ? E : N;
    a.K = key && a.M > 0 ? K : 0;                                 // (no key entry: every replica keeps everything there is)
    a.rg = rep_graph;
    a.rrow = rep_row;
    a.rth = rep_thresh;
    a.R = R;
    a.mode = mode;
    a.invert = invert;
    a.mx = max_nodes;
    a.cnt = (int64_t*)ws;
    a.map = reinterpret_cast<int32_t*>((int64_t*)ws + 2 * R);
    return a;
}

}  // namespace
}  // namespace cal

using namespace cal;

CAL_EXPORT int64_t cal_coalition_ws(int64_t, int64_t R, int64_t max_nodes, int mode) { return co_ws_need(R, max_nodes, mode); }

CAL_EXPORT int cal_coalition_count(const int64_t* edge_index, int64_t E, int64_t N, const int64_t* ptr, const int64_t* edge_ptr,
                                   int64_t B, const int32_t* key, int64_t K, const int64_t* rep_graph, const int64_t* rep_row,
                                   const int64_t* rep_thresh, int64_t R, int mode, int invert, int64_t max_nodes,
                                   int64_t* ptr_out, int64_t* edge_ptr_out, int64_t* totals, void* ws, int64_t ws_bytes,
                                   void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    COALITION_REQUIRE_INPUTS();
    CAL_REQUIRE(totals && ptr_out && edge_ptr_out, "totals / ptr_out / edge_ptr_out are null");
    if (R == 0) return zero_counts(__func__, totals, 5, ptr_out, edge_ptr_out, stream);
    CoArgs a = co_args(edge_index, E, N, ptr, edge_ptr, B, key, K, rep_graph, rep_row, rep_thresh, R, mode, invert, max_nodes, ws);
    a.ptr_out = ptr_out;
    a.eptr_out = edge_ptr_out;
    a.totals = totals;
    a.ticket = next_ticket();
    a.nblk = (int)R;
    CAL_REBATCH_COUNT(k_coalition_count, E / (B > 0 ? B : 1), R, stream, a);
    CAL_CHECK_LAUNCH("k_coalition_count");
    return 0;
}

CAL_EXPORT int cal_coalition_write(const int64_t* edge_index, int64_t E, int64_t N, const int64_t* ptr, const int64_t* edge_ptr,
                                   int64_t B, const int32_t* key, int64_t K, const int64_t* rep_graph, const int64_t* rep_row,
                                   const int64_t* rep_thresh, int64_t R, int mode, int invert, int64_t max_nodes, const float* x,
                                   int64_t F, const int64_t* ptr_out, const int64_t* edge_ptr_out, int64_t Nout, int64_t Eout,
                                   int64_t* batch_out, float* x_out, int64_t* edge_index_out, int64_t* node_src,
                                   int64_t* edge_src, void* ws, int64_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    COALITION_REQUIRE_INPUTS();
    CAL_REBATCH_REQUIRE_WRITE(R, !x_out || (F > 0 && (N == 0 || x)), "x_out needs F > 0 and x", Eout > 0 ? R : 0);
    if (R == 0 || nb + eb == 0) return 0;
    CoArgs a = co_args(edge_index, E, N, ptr, edge_ptr, B, key, K, rep_graph, rep_row, rep_thresh, R, mode, invert, max_nodes, ws);
    a.x = x;
    a.ptr_out = const_cast<int64_t*>(ptr_out);
    a.eptr_out = const_cast<int64_t*>(edge_ptr_out);
    a.out = write_out(Nout, Eout, batch_out, x_out, edge_index_out, node_src, edge_src, F, x);
    hipLaunchKernelGGL(k_coalition_write, dim3((unsigned)(nb + eb)), dim3(256), 0, stream, a, (int)nb);
    CAL_CHECK_LAUNCH("k_coalition_write");
    return 0;
}
