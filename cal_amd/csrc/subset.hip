// Subset replicas: the device operator behind cal_amd/counterfactual.py subset_batch (counterfactual search; the primitive of
// any sampler over arbitrary subsets of a graph's elements).
//
// cal_subset_count / cal_subset_write: replica r is graph g = rep_graph[r] of the batch restricted to the elements whose bit is
// set in row rep_row[r] of bits (uint32 [K, W]; bit j of a row is LOCAL element j of the replica's own graph: column
// edge_ptr[g] + j in mode 0, node ptr[g] + j in mode 1), after the local index rep_flip[r] -- and, in mode 0 with a twin map,
// its twin column -- has been toggled.  A row id outside [0, K) means every element is present; a local index >= 32 W is absent.
// The rule is sub_replica / elem_stays / col_stays of rules.hpp, which the host twin compiles too.  A key row per replica over
// the whole batch (cal_coalition_*) costs R x E int32; here a replica costs three int64 and shares its row with every other
// replica of the same state.
//
// The two launches follow the protocol of rebatch.hpp, the fifth builder on it.  What is particular here is what is particular
// in coalition.hip: in mode 1 the count leaves every node's new local id in the replica's row of the node map in ws, the write
// finds a source node by binary search in that row and rewrites the endpoints through it.
#include "rebatch.hpp"

namespace cal {
namespace {

struct SubArgs {
    const int64_t* ei;         // [2, E]
    int64_t E, N;
    const int64_t* ptr;        // [B + 1]
    const int64_t* eptr;       // [B + 1]
    int64_t B;
    const uint32_t* bits;      // [K, W]
    int64_t K, W;
    const int64_t* rg;         // [R] graph of every replica (outside [0, B): none)
    const int64_t* rrow;       // [R] bitset row of every replica (outside [0, K): everything present)
    const int64_t* rflip;      // [R] local index toggled (outside the graph's elements: none)
    const int32_t* twin;       // [E] or null (mode 0)
    int64_t R;
    int mode;                  // 0 edges, 1 nodes
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

// (SubRep, sub_replica, elem_stays, col_stays: rules.hpp)

// grid R, NT threads
template <int NT>
__global__ void __launch_bounds__(NT) k_subset_count(SubArgs a) {
    __shared__ long long red[NT / 64];
    __shared__ int wcnt[NT / 64];
    __shared__ int last;
    const int64_t r = blockIdx.x, R = a.R;
    const SubRep q = sub_replica(a, r);
    int64_t nodes = q.nn;
    if (a.mode == 1) {                                            // the map row: q.nn <= a.mx (sub_replica()), uniform over the workgroup
        int32_t* row = a.map + r * a.mx;
        nodes = 0;
        for (int64_t base = 0; base < q.nn; base += NT) {
            const int64_t l = base + threadIdx.x;
            const bool f = l < q.nn && elem_stays(a, q, l);
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
__global__ void __launch_bounds__(256) k_subset_write(SubArgs a, int node_blocks) {
    __shared__ int64_t src[kNodeChunk];
    __shared__ int wcnt[4];
    if ((int)blockIdx.x < node_blocks) {
        write_nodes(
            a.out, a.ptr_out, a.R, -1, src,
            [&](int64_t r, int64_t l) -> int64_t {
                const SubRep q = sub_replica(a, r);
                if (a.mode == 1 && q.nn > 0) l = owner(a.map + r * a.mx, q.nn, l);
                return l < q.nn ? q.nlo + l : -1;
            },
            [&](int64_t s) { return a.x + s * a.out.F; });
        return;
    }
    const int64_t r = (int64_t)((int)blockIdx.x - node_blocks);
    const SubRep q = sub_replica(a, r);
    const int32_t* row = a.mode == 1 ? a.map + r * a.mx : nullptr;
    write_cols(
        a.out, a.ptr_out, a.eptr_out, r, a.ei, a.E, q.elo, q.em, wcnt,
        [&](int64_t e) { return col_stays(a, q, e); },
        [&](int64_t u) { return row ? (int64_t)row[u - q.nlo] : u - q.nlo; });   // (u inside [nlo, nlo + nn): col_stays)
}

int64_t sub_ws_need(int64_t R, int64_t max_nodes, int mode) {
    R = R > 0 ? R : 0;
    return 16 * R + (mode == 1 ? 4 * R * (max_nodes > 0 ? max_nodes : 0) : 0) + 256;
}

// the checks both entry points share (CAL_REQUIRE names the entry point)
#define SUBSET_REQUIRE_INPUTS()                                                                                                  \
    CAL_REQUIRE(E >= 0 && N >= 0 && B >= 0 && R >= 0 && K >= 0 && W >= 0, "sizes must be >= 0");                                 \
    CAL_REQUIRE(R <= 0x7FFFFFFF, "too many replicas");                                                                           \
    CAL_REQUIRE(W <= (1 << 26), "W must be <= 2^26");                                                                            \
    CAL_REQUIRE(mode == 0 || mode == 1, "mode must be 0 (edges) or 1 (nodes)");                                                  \
    CAL_REQUIRE(max_nodes >= 0 && max_nodes <= 0x7FFFFFFF, "max_nodes must be in [0, 2^31)");                                    \
    CAL_REQUIRE(R == 0 || (rep_graph && rep_row && rep_flip), "rep_graph / rep_row / rep_flip are null");                        \
    CAL_REQUIRE(K == 0 || W == 0 || bits, "bits is null");                                                                       \
    CAL_REQUIRE(B == 0 || (ptr && edge_ptr), "ptr / edge_ptr are null");                                                         \
    CAL_REQUIRE(E == 0 || edge_index, "edge_index is null");                                                                     \
    CAL_REQUIRE(R == 0 || (ws && ws_bytes >= sub_ws_need(R, max_nodes, mode) && (reinterpret_cast<uintptr_t>(ws) & 7) == 0),     \
                "ws must be 8-byte aligned and hold cal_subset_ws(E, R, max_nodes, mode) bytes")

SubArgs sub_args(const int64_t* edge_index, int64_t E, int64_t N, const int64_t* ptr, const int64_t* edge_ptr, int64_t B,
                 const uint32_t* bits, int64_t K, int64_t W, const int64_t* rep_graph, const int64_t* rep_row,
                 const int64_t* rep_flip, int64_t R, const int32_t* twin, int mode, int64_t max_nodes, void* ws) {
    SubArgs a{};
    a.ei = edge_index;
    a.E = E;
    a.N = N;
    a.ptr = ptr;
    a.eptr = edge_ptr;
    a.B = B;
    a.bits = bits;
    a.K = K;
    a.W = W;
    a.rg = rep_graph;
    a.rrow = rep_row;
    a.rflip = rep_flip;
    a.twin = mode == 0 ? twin : nullptr;
    a.R = R;
    a.mode = mode;
    a.mx = max_nodes;
    a.cnt = (int64_t*)ws;
    a.map = reinterpret_cast<int32_t*>((int64_t*)ws + 2 * R);
    return a;
}

}  // namespace
}  // namespace cal

using namespace cal;

CAL_EXPORT int64_t cal_subset_ws(int64_t, int64_t R, int64_t max_nodes, int mode) { return sub_ws_need(R, max_nodes, mode); }

CAL_EXPORT int cal_subset_count(const int64_t* edge_index, int64_t E, int64_t N, const int64_t* ptr, const int64_t* edge_ptr,
                                int64_t B, const uint32_t* bits, int64_t K, int64_t W, const int64_t* rep_graph,
                                const int64_t* rep_row, const int64_t* rep_flip, int64_t R, const int32_t* twin, int mode,
                                int64_t max_nodes, int64_t* ptr_out, int64_t* edge_ptr_out, int64_t* totals, void* ws,
                                int64_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    SUBSET_REQUIRE_INPUTS();
    CAL_REQUIRE(totals && ptr_out && edge_ptr_out, "totals / ptr_out / edge_ptr_out are null");
    if (R == 0) return zero_counts(__func__, totals, 5, ptr_out, edge_ptr_out, stream);
    SubArgs a = sub_args(edge_index, E, N, ptr, edge_ptr, B, bits, K, W, rep_graph, rep_row, rep_flip, R, twin, mode, max_nodes, ws);
    a.ptr_out = ptr_out;
    a.eptr_out = edge_ptr_out;
    a.totals = totals;
    a.ticket = next_ticket();
    a.nblk = (int)R;
    CAL_REBATCH_COUNT(k_subset_count, E / (B > 0 ? B : 1), R, stream, a);
    CAL_CHECK_LAUNCH("k_subset_count");
    return 0;
}

CAL_EXPORT int cal_subset_write(const int64_t* edge_index, int64_t E, int64_t N, const int64_t* ptr, const int64_t* edge_ptr,
                                int64_t B, const uint32_t* bits, int64_t K, int64_t W, const int64_t* rep_graph,
                                const int64_t* rep_row, const int64_t* rep_flip, int64_t R, const int32_t* twin, int mode,
                                int64_t max_nodes, const float* x, int64_t F, const int64_t* ptr_out,
                                const int64_t* edge_ptr_out, int64_t Nout, int64_t Eout, int64_t* batch_out, float* x_out,
                                int64_t* edge_index_out, int64_t* node_src, int64_t* edge_src, void* ws, int64_t ws_bytes,
                                void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    SUBSET_REQUIRE_INPUTS();
    CAL_REBATCH_REQUIRE_WRITE(R, !x_out || (F > 0 && (N == 0 || x)), "x_out needs F > 0 and x", Eout > 0 ? R : 0);
    if (R == 0 || nb + eb == 0) return 0;
    SubArgs a = sub_args(edge_index, E, N, ptr, edge_ptr, B, bits, K, W, rep_graph, rep_row, rep_flip, R, twin, mode, max_nodes, ws);
    a.x = x;
    a.ptr_out = const_cast<int64_t*>(ptr_out);
    a.eptr_out = const_cast<int64_t*>(edge_ptr_out);
    a.out = write_out(Nout, Eout, batch_out, x_out, edge_index_out, node_src, edge_src, F, x);
    hipLaunchKernelGGL(k_subset_write, dim3((unsigned)(nb + eb)), dim3(256), 0, stream, a, (int)nb);
    CAL_CHECK_LAUNCH("k_subset_write");
    return 0;
}
