// Batch splice: result graph p is the disjoint union of graph ga[p] of batch A and graph gb[p] of batch B, on the device.
//
// Graph g of a batch owns the nodes [ptr[g], ptr[g+1]) and the edge_index columns [edge_ptr[g], edge_ptr[g+1]).  The nodes of
// result graph p are A's nodes of ga[p] in their order, then B's nodes of gb[p]; its columns are A's columns of ga[p] in their
// order, then B's, then (for a bridge whose two ids are >= 0 and lie inside the two parts) the columns (a', b') and (b', a').  A
// pairing entry outside its batch counts as -1: that part is absent.  A source column with an endpoint outside its graph's node
// range is dropped, as in subgraph.hip.  Every integer output is uniquely determined (the host twin and a plain-torch
// restatement agree bit for bit); the feature rows are copies.
//
// The two launches follow the protocol of rebatch.hpp.  What is particular here:
//  * k_splice_count: a part that drops a column also gets sel[] in ws, the position of its k-th valid column (a property of the
//    source graph: pairs that share it write the same values); totals[5] counts the bridges asked for and not written.
//  * k_splice_write works on fixed chunks of the OUTPUT, so that a 5000-node part and a 3-node part cost what their elements
//    cost: after the node workgroups (two sources: node_src holds A's row id as it is, B's as -1 - id) the column workgroups
//    take kColChunk result columns each (the pair by binary search in edge_ptr_out, the source column directly or through
//    sel[], the endpoints rewritten).
#include "rebatch.hpp"

namespace cal {
namespace {

constexpr int kColPerLane = 4;             // result columns per thread of a column workgroup
constexpr int kColChunk = 256 * kColPerLane;
constexpr int64_t kBridge = INT64_MIN;     // edge_src of a bridge column (CAL_SPLICE_BRIDGE); as a row code: no row

struct Side {
    const int64_t* ei;         // [2, E]
    int64_t E, N;
    const int64_t* ptr;        // [B + 1]
    const int64_t* eptr;       // [B + 1]
    int64_t B;
    const int64_t* pick;       // [P] graph of this batch in every pair (-1 or out of range: none)
    const int64_t* bridge;     // [P] node id of this batch or null
    const float* x;            // [N, F] or null
    int64_t* sel;              // ws [E]: local index of the k-th valid column of a graph that drops one
};

struct SpliceArgs {
    Side a, b;
    int64_t P;
    int64_t* ptr_out;          // [P + 1]
    int64_t* eptr_out;         // [P + 1]
    int64_t* totals;           // [6]
    int64_t* cnt;              // ws [5 P]: valid columns of A, of B, nodes, columns, bridges asked for and not written
    WriteOut out;              // (write)
    int ticket, nblk;
};

// (side_ranges, col_valid: rules.hpp)

// valid columns of the part; when one is dropped, sel[elo + k] = local index of the k-th valid one.  All threads call it.
template <int NT>
__device__ __forceinline__ int64_t count_side(const Side& s, int64_t nlo, int64_t nn, int64_t elo, int64_t em, long long* red,
                                              int* wcnt) {
    long long c = 0;
    for (int64_t q = threadIdx.x; q < em; q += NT) c += col_valid(s, elo + q, nlo, nn);
    const int64_t tot = wg_sum<NT>(c, red);
    if (tot != em) {                                              // (uniform over the workgroup)
        int64_t carry = 0;
        for (int64_t base = 0; base < em; base += NT) {
            const int64_t q = base + threadIdx.x;
            const bool f = q < em && col_valid(s, elo + q, nlo, nn);
            int t;
            const int pos = wg_excl<NT>(f, wcnt, t);
            if (f) s.sel[elo + carry + pos] = q;
            carry += t;
        }
    }
    return tot;
}

// grid P, NT threads
template <int NT>
__global__ void __launch_bounds__(NT) k_splice_count(SpliceArgs a) {
    __shared__ long long red[NT / 64];
    __shared__ int wcnt[NT / 64];
    __shared__ int last;
    const int64_t p = blockIdx.x, P = a.P;
    int64_t alo, an, aelo, aem, blo, bn, belo, bem;
    side_ranges(a.a, p, alo, an, aelo, aem);
    side_ranges(a.b, p, blo, bn, belo, bem);
    const int64_t ea = count_side<NT>(a.a, alo, an, aelo, aem, red, wcnt);
    const int64_t eb = count_side<NT>(a.b, blo, bn, belo, bem, red, wcnt);
    if (threadIdx.x == 0) {
        const int64_t ba = a.a.bridge ? a.a.bridge[p] : -1, bb = a.b.bridge ? a.b.bridge[p] : -1;
        const bool asked = ba >= 0 || bb >= 0;
        const bool put = ba >= alo && ba < alo + an && bb >= blo && bb < blo + bn && ba >= 0 && bb >= 0;
        a.cnt[p] = ea;
        a.cnt[P + p] = eb;
        a.cnt[2 * P + p] = an + bn;
        a.cnt[3 * P + p] = ea + eb + (put ? 2 : 0);
        a.cnt[4 * P + p] = asked && !put;
    }
    if (!last_workgroup(a.ticket, a.nblk, &last)) return;
    long long unput = 0;                                          // (read before the scan: its loads' latency hides under it)
    for (int64_t q = threadIdx.x; q < P; q += NT)
        unput += __hip_atomic_load(a.cnt + 4 * P + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    scan_counts<NT>(a.cnt + 2 * P, a.cnt + 3 * P, P, a.ptr_out, a.eptr_out, a.totals, red);
    unput = wg_sum<NT>(unput, red);
    if (threadIdx.x == 0) a.totals[5] = unput;
}

// grid ceil(Nout / kNodeChunk) node workgroups, then ceil(Eout / kColChunk) column workgroups; 256 threads
__global__ void __launch_bounds__(256) k_splice_write(SpliceArgs a, int node_blocks) {
    __shared__ int64_t src[kNodeChunk];
    const int64_t P = a.P;
    if ((int)blockIdx.x < node_blocks) {
        write_nodes(
            a.out, a.ptr_out, P, kBridge, src,
            [&](int64_t p, int64_t l) -> int64_t {
                int64_t alo, an, blo, bn, e0, e1;
                side_ranges(a.a, p, alo, an, e0, e1);
                if (l < an) return alo + l;
                side_ranges(a.b, p, blo, bn, e0, e1);
                return l - an < bn ? -1 - (blo + l - an) : kBridge;
            },
            [&](int64_t s) { return s >= 0 ? a.a.x + s * a.out.F : a.b.x + (-1 - s) * a.out.F; });
        return;
    }
    const int64_t j0 = (int64_t)((int)blockIdx.x - node_blocks) * kColChunk;
#pragma unroll
    for (int k = 0; k < kColPerLane; ++k) {
        const int64_t j = j0 + k * 256 + threadIdx.x;
        if (j >= a.out.Eout) continue;
        const int64_t p = owner(a.eptr_out, P + 1, j);
        if (p >= P) continue;
        const int64_t l = j - a.eptr_out[p], ea = a.cnt[p], eb = a.cnt[P + p], n0 = a.ptr_out[p];
        int64_t alo, an, aelo, aem, blo, bn, belo, bem;
        side_ranges(a.a, p, alo, an, aelo, aem);
        int64_t u, v, code;
        if (l < ea) {
            const int64_t e = aelo + (ea != aem ? a.a.sel[aelo + l] : l);
            u = n0 + (a.a.ei[e] - alo);
            v = n0 + (a.a.ei[a.a.E + e] - alo);
            code = e;
        } else {
            side_ranges(a.b, p, blo, bn, belo, bem);
            const int64_t m = l - ea;
            if (m < eb) {
                const int64_t e = belo + (eb != bem ? a.b.sel[belo + m] : m);
                u = n0 + an + (a.b.ei[e] - blo);
                v = n0 + an + (a.b.ei[a.b.E + e] - blo);
                code = -1 - e;
            } else {
                if (m - eb > 1 || !a.a.bridge || !a.b.bridge) continue;
                const int64_t ba = a.a.bridge[p], bb = a.b.bridge[p];
                if (ba < alo || ba >= alo + an || bb < blo || bb >= blo + bn) continue;
                const int64_t x = n0 + (ba - alo), y = n0 + an + (bb - blo);
                u = m == eb ? x : y;
                v = m == eb ? y : x;
                code = kBridge;
            }
        }
        a.out.ei_out[j] = u;
        a.out.ei_out[a.out.Eout + j] = v;
        a.out.edge_src[j] = code;
    }
}

int64_t ws_need(int64_t Ea, int64_t Eb, int64_t P) {            // cnt [5 P], sel of A [Ea], sel of B [Eb]
    return 40 * (P > 0 ? P : 0) + 8 * (Ea > 0 ? Ea : 0) + 8 * (Eb > 0 ? Eb : 0) + 256;
}

// the checks both entry points share (CAL_REQUIRE names the entry point)
#define SPLICE_REQUIRE_INPUTS()                                                                                                  \
    CAL_REQUIRE(Ea >= 0 && Na >= 0 && Ba >= 0 && Eb >= 0 && Nb >= 0 && Bb >= 0 && P >= 0, "sizes must be >= 0");                 \
    CAL_REQUIRE(P <= 0x7FFFFFFF, "too many pairs");                                                                              \
    CAL_REQUIRE(P == 0 || (ga && gb), "ga / gb are null");                                                                       \
    CAL_REQUIRE((Ba == 0 || (ptr_a && eptr_a)) && (Bb == 0 || (ptr_b && eptr_b)), "ptr / edge_ptr are null");                    \
    CAL_REQUIRE((Ea == 0 || eia) && (Eb == 0 || eib), "edge_index is null");                                                     \
    CAL_REQUIRE((bridge_a == nullptr) == (bridge_b == nullptr), "bridge_a and bridge_b come together");                         \
    CAL_REQUIRE(P == 0 || (ws && ws_bytes >= ws_need(Ea, Eb, P) && (reinterpret_cast<uintptr_t>(ws) & 7) == 0),                  \
                "ws must be 8-byte aligned and hold cal_graph_splice_ws(Ea, Eb, P) bytes")

SpliceArgs make_args(const int64_t* eia, int64_t Ea, int64_t Na, const int64_t* ptr_a, const int64_t* eptr_a, int64_t Ba,
                     const int64_t* eib, int64_t Eb, int64_t Nb, const int64_t* ptr_b, const int64_t* eptr_b, int64_t Bb,
                     const int64_t* ga, const int64_t* gb, int64_t P, const int64_t* bridge_a, const int64_t* bridge_b, void* ws) {
    SpliceArgs a{};
    int64_t* w = (int64_t*)ws;
    a.a = Side{eia, Ea, Na, ptr_a, eptr_a, Ba, ga, bridge_a, nullptr, w + 5 * P};
    a.b = Side{eib, Eb, Nb, ptr_b, eptr_b, Bb, gb, bridge_b, nullptr, w + 5 * P + Ea};
    a.P = P;
    a.cnt = w;
    return a;
}

}  // namespace
}  // namespace cal

using namespace cal;

CAL_EXPORT int64_t cal_graph_splice_ws(int64_t Ea, int64_t Eb, int64_t P) {
    return ws_need(Ea, Eb, P);
}

CAL_EXPORT int cal_graph_splice_count(const int64_t* eia, int64_t Ea, int64_t Na, const int64_t* ptr_a, const int64_t* eptr_a,
                                      int64_t Ba, const int64_t* eib, int64_t Eb, int64_t Nb, const int64_t* ptr_b,
                                      const int64_t* eptr_b, int64_t Bb, const int64_t* ga, const int64_t* gb, int64_t P,
                                      const int64_t* bridge_a, const int64_t* bridge_b, int64_t* ptr_out, int64_t* edge_ptr_out,
                                      int64_t* totals, void* ws, int64_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    SPLICE_REQUIRE_INPUTS();
    CAL_REQUIRE(totals && ptr_out && edge_ptr_out, "totals / ptr_out / edge_ptr_out are null");
    if (P == 0) return zero_counts(__func__, totals, 6, ptr_out, edge_ptr_out, stream);
    SpliceArgs a = make_args(eia, Ea, Na, ptr_a, eptr_a, Ba, eib, Eb, Nb, ptr_b, eptr_b, Bb, ga, gb, P, bridge_a, bridge_b, ws);
    a.ptr_out = ptr_out;
    a.eptr_out = edge_ptr_out;
    a.totals = totals;
    a.ticket = next_ticket();
    a.nblk = (int)P;
    CAL_REBATCH_COUNT(k_splice_count, (Ea + Eb) / (Ba + Bb > 0 ? Ba + Bb : 1), P, stream, a);
    CAL_CHECK_LAUNCH("k_splice_count");
    return 0;
}

CAL_EXPORT int cal_graph_splice_write(const int64_t* eia, int64_t Ea, int64_t Na, const int64_t* ptr_a, const int64_t* eptr_a,
                                      int64_t Ba, const int64_t* eib, int64_t Eb, int64_t Nb, const int64_t* ptr_b,
                                      const int64_t* eptr_b, int64_t Bb, const int64_t* ga, const int64_t* gb, int64_t P,
                                      const int64_t* bridge_a, const int64_t* bridge_b, const float* xa, const float* xb, int64_t F,
                                      const int64_t* ptr_out, const int64_t* edge_ptr_out, int64_t Nout, int64_t Eout,
                                      int64_t* batch_out, float* x_out, int64_t* edge_index_out, int64_t* node_src,
                                      int64_t* edge_src, void* ws, int64_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    SPLICE_REQUIRE_INPUTS();
    CAL_REBATCH_REQUIRE_WRITE(P, !x_out || (F > 0 && (Na == 0 || xa) && (Nb == 0 || xb)), "x_out needs F > 0, xa and xb",
                              (Eout + kColChunk - 1) / kColChunk);
    if (P == 0 || nb + eb == 0) return 0;
    SpliceArgs a = make_args(eia, Ea, Na, ptr_a, eptr_a, Ba, eib, Eb, Nb, ptr_b, eptr_b, Bb, ga, gb, P, bridge_a, bridge_b, ws);
    a.a.x = xa;
    a.b.x = xb;
    a.ptr_out = const_cast<int64_t*>(ptr_out);
    a.eptr_out = const_cast<int64_t*>(edge_ptr_out);
    a.out = write_out(Nout, Eout, batch_out, x_out, edge_index_out, node_src, edge_src, F, xa, xb);
    hipLaunchKernelGGL(k_splice_write, dim3((unsigned)(nb + eb)), dim3(256), 0, stream, a, (int)nb);
    CAL_CHECK_LAUNCH("k_splice_write");
    return 0;
}
