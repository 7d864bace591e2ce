// The restriction builders (occlude.hip, coalition.hip, subset.hip): one count kernel, one write kernel and their launches,
// templated on the source S of rules.hpp, whose replica / node_stays / col_stays overloads are the only thing a builder says
// about itself.  The two launches follow the protocol of rebatch.hpp.  No translation unit of its own: each builder instantiates
// the pair for its source.
//
// Renumbering the nodes that stay (mode 1) has two forms.  A source with a map (S::mx) keeps, per replica, a row of ws with every
// node's new local id -- the number of staying nodes in front of it, whether it stays or not (int32, mx per replica: any graph
// size, nothing is staged in LDS): the count walks the graph's nodes in chunks of one workgroup's threads and writes it, the
// write finds a source node by binary search in the row, which is non-decreasing, and rewrites the endpoints through it.  The map
// is read one launch after it was written.  Occlusion removes at most one node, q.rn: the closed form, no map and no ws for one.
#pragma once
#include <type_traits>

#include "rebatch.hpp"

namespace cal {
namespace {

template <class S>
constexpr bool kClosedForm = std::is_same<S, OccSrc>::value;

template <class S>
struct RestrictArgs {
    S s;                       // the batch, the replicas and their rule
    int64_t R;
    int64_t* ptr_out;          // [R + 1]
    int64_t* eptr_out;         // [R + 1]
    int64_t* totals;           // (count) [5]
    int64_t* cnt;              // ws [2 R]: nodes, columns of every replica
    int32_t* map;              // ws [R, s.mx] (mode 1, not the closed form): staying nodes in front of every node of the graph
    const float* x;            // (write) [N, F] or null
    WriteOut out;              // (write)
    int ticket, nblk;          // (count)
};

// grid R, NT threads
template <int NT, class S>
__global__ void __launch_bounds__(NT) k_restrict_count(RestrictArgs<S> a) {
    __shared__ long long red[NT / 64];
    __shared__ int last;
    const int64_t r = blockIdx.x, R = a.R;
    const auto q = replica(a.s, r);
    int64_t nodes = q.nn;
    if constexpr (kClosedForm<S>) {
        nodes -= q.rn >= 0 ? 1 : 0;
    } else if (a.s.mode == 1) {                                   // the map row: q.nn <= s.mx (replica()), uniform over the workgroup
        __shared__ int wcnt[NT / 64];
        int32_t* row = a.map + r * a.s.mx;
        nodes = 0;
        for (int64_t base = 0; base < q.nn; base += NT) {
            const int64_t l = base + threadIdx.x;
            const bool f = l < q.nn && node_stays(a.s, q, l);
            int t;
            const int pos = wg_excl<NT>(f, wcnt, t);
            if (l < q.nn) row[l] = (int32_t)(nodes + pos);
            nodes += t;
        }
    }
    long long c = 0;
    for (int64_t t = threadIdx.x; t < q.em; t += NT) c += col_stays(a.s, q, q.elo + t);
    const int64_t kept = wg_sum<NT>(c, red);
    if (threadIdx.x == 0) {
        a.cnt[r] = nodes;
        a.cnt[R + r] = kept;
    }
    if (last_workgroup(a.ticket, a.nblk, &last)) scan_counts<NT>(a.cnt, a.cnt + R, R, a.ptr_out, a.eptr_out, a.totals, red);
}

// grid ceil(Nout / kNodeChunk) node workgroups, then R column workgroups; 256 threads
template <class S>
__global__ void __launch_bounds__(256) k_restrict_write(RestrictArgs<S> a, int node_blocks) {
    __shared__ int64_t src[kNodeChunk];
    __shared__ int wcnt[4];
    if ((int)blockIdx.x < node_blocks) {
        write_nodes(
            a.out, a.ptr_out, a.R, -1, src,
            [&](int64_t r, int64_t l) -> int64_t {
                const auto q = replica(a.s, r);
                if constexpr (kClosedForm<S>) l += q.rn >= 0 && q.nlo + l >= q.rn;
                else if (a.s.mode == 1 && q.nn > 0) l = owner(a.map + r * a.s.mx, q.nn, l);
                return l < q.nn ? q.nlo + l : -1;
            },
            [&](int64_t s) { return a.x + s * a.out.F; });
        return;
    }
    const int64_t r = (int64_t)((int)blockIdx.x - node_blocks);
    const auto q = replica(a.s, r);
    const int32_t* row = nullptr;
    if constexpr (!kClosedForm<S>) row = a.s.mode == 1 ? a.map + r * a.s.mx : nullptr;
    write_cols(
        a.out, a.ptr_out, a.eptr_out, r, a.s.ei, a.s.E, q.elo, q.em, wcnt,
        [&](int64_t e) { return col_stays(a.s, q, e); },
        [&](int64_t u) -> int64_t {                                // (u inside [nlo, nlo + nn): col_stays)
            if constexpr (kClosedForm<S>) return (u - q.nlo) - (q.rn >= 0 && u > q.rn);
            else return row ? (int64_t)row[u - q.nlo] : u - q.nlo;
        });
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
template <class S>
RestrictArgs<S> restrict_args(const S& s, int64_t R, const int64_t* ptr_out, const int64_t* eptr_out, void* ws) {
    RestrictArgs<S> a{};
    a.s = s;
    a.R = R;
    a.ptr_out = const_cast<int64_t*>(ptr_out);
    a.eptr_out = const_cast<int64_t*>(eptr_out);
    a.cnt = (int64_t*)ws;
    a.map = reinterpret_cast<int32_t*>((int64_t*)ws + 2 * R);
    return a;
}

// what a count entry point does after its checks (entry: its name)
template <class S>
int restrict_count(const char* entry, const S& s, int64_t R, int64_t* ptr_out, int64_t* eptr_out, int64_t* totals, void* ws,
                   hipStream_t stream) {
    if (R == 0) return zero_counts(entry, totals, 5, ptr_out, eptr_out, stream);
    RestrictArgs<S> a = restrict_args(s, R, ptr_out, eptr_out, ws);
    a.totals = totals;
    a.ticket = next_ticket();
    a.nblk = (int)R;
    CAL_REBATCH_COUNT(k_restrict_count, s.E / (s.B > 0 ? s.B : 1), R, stream, a);
    CAL_CHECK_LAUNCH("k_restrict_count");
    return 0;
}

// what a write entry point does after its checks; nb, eb: CAL_REBATCH_REQUIRE_WRITE
template <class S>
int restrict_write(const S& s, int64_t R, const float* x, const int64_t* ptr_out, const int64_t* eptr_out, const WriteOut& out,
                   int64_t nb, int64_t eb, void* ws, hipStream_t stream) {
    if (R == 0 || nb + eb == 0) return 0;
    RestrictArgs<S> a = restrict_args(s, R, ptr_out, eptr_out, ws);
    a.x = x;
    a.out = out;
    hipLaunchKernelGGL(k_restrict_write<S>, dim3((unsigned)(nb + eb)), dim3(256), 0, stream, a, (int)nb);
    CAL_CHECK_LAUNCH("k_restrict_write");
    return 0;
}

// The checks the entry points of the three share (CAL_REQUIRE names the entry point): HEAD, then the builder's own, then TAIL.
#define CAL_RESTRICT_REQUIRE_HEAD(sizes_ok)                                                                                      \
    CAL_REQUIRE(sizes_ok, "sizes must be >= 0");                                                                                 \
    CAL_REQUIRE(R <= 0x7FFFFFFF, "too many replicas");                                                                           \
    CAL_REQUIRE(mode == 0 || mode == 1, "mode must be 0 (edges) or 1 (nodes)")
#define CAL_RESTRICT_REQUIRE_TAIL(max_nodes, ws_msg)                                                                             \
    CAL_REQUIRE(B == 0 || (ptr && edge_ptr), "ptr / edge_ptr are null");                                                         \
    CAL_REQUIRE(E == 0 || edge_index, "edge_index is null");                                                                     \
    CAL_REQUIRE(R == 0 || (ws && ws_bytes >= restrict_ws_need(R, max_nodes, mode) && (reinterpret_cast<uintptr_t>(ws) & 7) == 0), \
                ws_msg)

}  // namespace
}  // namespace cal
