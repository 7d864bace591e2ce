// Subgraph extraction: a per-edge / per-node keep mask -> the compacted (and optionally relabelled) batch, on the device.
//
// Graph g owns the nodes [ptr[g], ptr[g+1]) and the edge_index columns [edge_ptr[g], edge_ptr[g+1]).  An edge is kept iff
// edge_keep says so (when given), both endpoints are kept nodes (when node_keep is given) and both endpoints lie inside its
// graph's node range; with `complement` each given mask is read inverted.  relabel = 0: every node stays, ids unchanged.
// relabel = 1: the kept nodes are node_keep when given, else the nodes incident to a kept edge; they are renumbered densely in
// their original order, the endpoints rewritten, the rows of x gathered.  Kept elements keep their relative order, graphs keep
// theirs, so every integer output is uniquely determined (the host twin and a plain-torch restatement agree bit for bit).
//
// Two launches, one workgroup per graph, any graph size (the graph is walked in chunks of one workgroup's threads):
//  * k_subgraph_count: effective node flags and edge flags into ws, the graph's kept-node / kept-edge counts into ws.
//  * k_subgraph_write: every workgroup sums the counts of the graphs before it (B is at most a few thousand) and the whole
//    row (totals, the offset E' of the second edge_index row), then compacts its nodes and edges in order: per chunk the
//    ballot scan of segment.hpp, a running carry across the chunks.
// No grid depends on a value the device computed; the caller reads the four totals back once and slices the outputs.
// The clamped ranges, the fixed-order workgroup sums and the scan are segment.hpp's, shared with explain.hip and twin.hip.
#include "segment.hpp"

namespace cal {
namespace {

struct SubArgs {
    const int64_t* ei;         // [2, E]
    int64_t E, N;
    const int64_t* ptr;        // [B + 1]
    const int64_t* eptr;       // [B + 1]
    int64_t B;
    const uint8_t* ekeep;      // [E] or null
    const uint8_t* nkeep;      // [N] or null
    int complement, relabel;
    const float* x;            // [N, F] or null
    int64_t F;
    int64_t* ei_out;           // [2 E]: row 0 at [0, E'), row 1 at [E', 2 E')
    int64_t* ptr_out;          // [B + 1]
    int64_t* eptr_out;         // [B + 1]
    int64_t* batch_out;        // [N] or null
    float* x_out;              // [N, F] or null
    int64_t* node_map;         // [N] or null
    int64_t* edge_map;         // [E]
    int64_t* totals;           // [4]: N', E', max_nodes', max_edges'
    int64_t* cnt;              // ws: [2 B] kept nodes, kept edges per graph
    int64_t* newid;            // ws: [N] new id of a kept node (relabel)
    uint8_t* nflag;            // ws: [N] effective node flags
    uint8_t* eflag;            // ws: [E] effective edge flags
};

// grid B, NT threads
template <int NT>
__global__ void __launch_bounds__(NT) k_subgraph_count(SubArgs a) {
    __shared__ long long red[NT / 64];
    const int64_t g = blockIdx.x;
    int64_t nlo, nn, elo, em;
    seg_clamp(a.ptr, g, a.N, nlo, nn);
    seg_clamp(a.eptr, g, a.E, elo, em);
    const bool from_edges = a.relabel && !a.nkeep;            // kept nodes = the endpoints of the kept edges
    if (a.nkeep) {
        for (int64_t q = threadIdx.x; q < nn; q += NT) a.nflag[nlo + q] = (a.nkeep[nlo + q] != 0) != (a.complement != 0);
    } else if (from_edges) {
        for (int64_t q = threadIdx.x; q < nn; q += NT) a.nflag[nlo + q] = 0;
    }
    __syncthreads();
    long long ec = 0;
    for (int64_t q = threadIdx.x; q < em; q += NT) {
        const int64_t e = elo + q, s = a.ei[e], d = a.ei[a.E + e];
        bool k = s >= nlo && s < nlo + nn && d >= nlo && d < nlo + nn;
        if (k && a.ekeep) k = (a.ekeep[e] != 0) != (a.complement != 0);
        if (k && a.nkeep) k = a.nflag[s] && a.nflag[d];
        a.eflag[e] = k;
        ec += k;
        if (k && from_edges) {
            a.nflag[s] = 1;
            a.nflag[d] = 1;
        }
    }
    __syncthreads();
    long long nc = 0;
    if (a.relabel)
        for (int64_t q = threadIdx.x; q < nn; q += NT) nc += a.nflag[nlo + q];
    nc = wg_sum<NT>(nc, red);
    ec = wg_sum<NT>(ec, red);
    if (threadIdx.x == 0) {
        a.cnt[g] = a.relabel ? nc : nn;
        a.cnt[a.B + g] = ec;
    }
}

// grid B, NT threads
template <int NT>
__global__ void __launch_bounds__(NT) k_subgraph_write(SubArgs a) {
    __shared__ long long red[NT / 64];
    __shared__ int wcnt[NT / 64];
    const int64_t g = blockIdx.x;
    int64_t nlo, nn, elo, em;
    seg_clamp(a.ptr, g, a.N, nlo, nn);
    seg_clamp(a.eptr, g, a.E, elo, em);

    long long on = 0, oe = 0, tn = 0, te = 0, mn = 0, me = 0;
    for (int64_t h = threadIdx.x; h < a.B; h += NT) {
        const long long n = a.cnt[h], e = a.cnt[a.B + h];
        tn += n;
        te += e;
        if (h < g) {
            on += n;
            oe += e;
        }
        mn = n > mn ? n : mn;
        me = e > me ? e : me;
    }
    on = wg_sum<NT>(on, red);
    oe = wg_sum<NT>(oe, red);
    tn = wg_sum<NT>(tn, red);
    te = wg_sum<NT>(te, red);
    // (segments that overlap could count an element twice: nothing is written past the outputs' N / E entries)
    const int64_t Nt = tn < a.N ? tn : a.N, Et = te < a.E ? te : a.E;
    if (g == 0) {                                             // (uniform over the workgroup)
        mn = wg_max<NT>(mn, red);
        me = wg_max<NT>(me, red);
        if (threadIdx.x == 0) {
            a.totals[0] = Nt;
            a.totals[1] = Et;
            a.totals[2] = mn;
            a.totals[3] = me;
            a.ptr_out[a.B] = Nt;
            a.eptr_out[a.B] = Et;
        }
    }
    if (threadIdx.x == 0) {
        a.ptr_out[g] = on < Nt ? on : Nt;
        a.eptr_out[g] = oe < Et ? oe : Et;
    }

    if (a.relabel) {
        int64_t carry = 0;
        for (int64_t base = 0; base < nn; base += NT) {
            const int64_t q = base + threadIdx.x;
            const bool f = q < nn && a.nflag[nlo + q];
            int tot;
            const int pos = wg_excl<NT>(f, wcnt, tot);
            if (f) {
                const int64_t p = on + carry + pos;
                a.newid[nlo + q] = p;
                if (p < Nt) {
                    if (a.node_map) a.node_map[p] = nlo + q;
                    if (a.batch_out) a.batch_out[p] = g;
                }
            }
            carry += tot;
        }
        __syncthreads();                                      // newid / node_map of this graph are read below
        if (a.x && a.x_out && a.node_map) {
            const int64_t rows = a.cnt[g], F = a.F;
            for (int64_t t = threadIdx.x; t < rows * F; t += NT) {
                const int64_t r = t / F, c = t - r * F, p = on + r;
                if (p < Nt) a.x_out[p * F + c] = a.x[a.node_map[p] * F + c];
            }
        }
    } else {
        for (int64_t q = threadIdx.x; q < nn; q += NT) {
            if (a.node_map) a.node_map[nlo + q] = nlo + q;
            if (a.batch_out) a.batch_out[nlo + q] = g;
        }
    }

    int64_t carry = 0;
    for (int64_t base = 0; base < em; base += NT) {
        const int64_t q = base + threadIdx.x;
        const bool f = q < em && a.eflag[elo + q];
        int tot;
        const int pos = wg_excl<NT>(f, wcnt, tot);
        if (f) {
            const int64_t e = elo + q, p = oe + carry + pos;
            if (p < Et) {
                const int64_t s = a.ei[e], d = a.ei[a.E + e];
                a.ei_out[p] = a.relabel ? a.newid[s] : s;
                a.ei_out[Et + p] = a.relabel ? a.newid[d] : d;
                a.edge_map[p] = e;
            }
        }
        carry += tot;
    }
}

}  // namespace
}  // namespace cal

using namespace cal;

CAL_EXPORT int64_t cal_subgraph_ws(int64_t N, int64_t E, int64_t B) {
    N = N > 0 ? N : 0;
    E = E > 0 ? E : 0;
    B = B > 0 ? B : 0;
    return 16 * B + 8 * N + N + E + 256;
}

CAL_EXPORT int cal_subgraph_extract(const int64_t* edge_index, int64_t E, int64_t N, const int64_t* ptr, const int64_t* edge_ptr,
                                    int64_t B, const uint8_t* edge_keep, const uint8_t* node_keep, int complement, int relabel,
                                    const float* x, int64_t F, int64_t* edge_index_out, int64_t* ptr_out, int64_t* edge_ptr_out,
                                    int64_t* batch_out, float* x_out, int64_t* node_map, int64_t* edge_map, int64_t* totals,
                                    void* ws, int64_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CAL_REQUIRE(E >= 0 && N >= 0 && B >= 0 && F >= 0, "E, N, B, F must be >= 0");
    CAL_REQUIRE(B <= 0x7FFFFFFF, "too many graphs");
    CAL_REQUIRE(totals && ptr_out && edge_ptr_out, "totals / ptr_out / edge_ptr_out are null");
    CAL_REQUIRE(B == 0 || (ptr && edge_ptr), "ptr / edge_ptr are null");
    CAL_REQUIRE(E == 0 || (edge_index && edge_index_out && edge_map), "edge_index / edge_index_out / edge_map are null");
    CAL_REQUIRE(!relabel || N == 0 || (node_map && batch_out), "relabel needs node_map and batch_out");
    CAL_REQUIRE(!x_out || (x && relabel && F > 0), "x_out needs x, F > 0 and relabel");
    CAL_REQUIRE(ws && ws_bytes >= cal_subgraph_ws(N, E, B) && (reinterpret_cast<uintptr_t>(ws) & 7) == 0,
                "ws must be 8-byte aligned and hold cal_subgraph_ws(N, E, B) bytes");
    if (B == 0) {
        if (hipMemsetAsync(totals, 0, 4 * sizeof(int64_t), stream) != hipSuccess ||
            hipMemsetAsync(ptr_out, 0, sizeof(int64_t), stream) != hipSuccess ||
            hipMemsetAsync(edge_ptr_out, 0, sizeof(int64_t), stream) != hipSuccess) {
            cal::set_error("cal_subgraph_extract: hipMemsetAsync failed");
            return 1;
        }
        return 0;
    }
    SubArgs a{edge_index, E, N, ptr, edge_ptr, B, edge_keep, node_keep, complement, relabel, x, F, edge_index_out, ptr_out,
              edge_ptr_out, batch_out, x_out, node_map, edge_map, totals, nullptr, nullptr, nullptr, nullptr};
    char* w = (char*)ws;
    a.cnt = (int64_t*)w;
    a.newid = (int64_t*)(w + 16 * B);
    a.nflag = (uint8_t*)(w + 16 * B + 8 * N);
    a.eflag = a.nflag + N;
    // wide workgroups once the average graph has more elements than a 256-thread workgroup walks in a few chunks
    const bool wide = (N + E) / B > 2048;
    if (wide) {
        hipLaunchKernelGGL(k_subgraph_count<1024>, dim3((unsigned)B), dim3(1024), 0, stream, a);
        CAL_CHECK_LAUNCH("k_subgraph_count");
        hipLaunchKernelGGL(k_subgraph_write<1024>, dim3((unsigned)B), dim3(1024), 0, stream, a);
        CAL_CHECK_LAUNCH("k_subgraph_write");
    } else {
        hipLaunchKernelGGL(k_subgraph_count<256>, dim3((unsigned)B), dim3(256), 0, stream, a);
        CAL_CHECK_LAUNCH("k_subgraph_count");
        hipLaunchKernelGGL(k_subgraph_write<256>, dim3((unsigned)B), dim3(256), 0, stream, a);
        CAL_CHECK_LAUNCH("k_subgraph_write");
    }
    return 0;
}
