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
// endpoint outside its graph's node range is dropped, as in splice.hip / occlude.hip.  Every integer output is uniquely
// determined (the host twin and a plain-torch restatement agree bit for bit); the feature rows are copies.
//
// Two launches with the caller's one read-back of totals between them, the shape of occlude.hip:
//  * k_coalition_count, one workgroup per replica: in mode 1 the graph's nodes are walked in chunks of one workgroup's threads
//    and every node's new local id -- the number of staying nodes in front of it, whether it stays or not -- goes to the
//    replica's row of the node map in ws (int32, max_nodes per replica: any graph size, nothing is staged in LDS); then the
//    columns that stay are counted the same way.  The workgroup that finishes last scans the R counts into ptr_out /
//    edge_ptr_out and writes totals; it is found with the completion ticket of occlude.hip (one atomicInc per workgroup on a
//    wrapping counter, nothing else): no output value is accumulated atomically.
//  * k_coalition_write: node workgroups take kNodeChunk result nodes (the replica by binary search in ptr_out; in mode 1 the
//    source node by binary search in the replica's map row, which is non-decreasing; batch_out / node_src, then the feature
//    rows: 16 bytes per lane when F % 4 == 0 and both bases are 16-byte aligned, else element by element); after them one
//    column workgroup per replica walks the source graph's columns in chunks and writes the ones that stay, in order, at
//    edge_ptr_out[r] on, the endpoints of mode 1 through the map row.  The map is read one launch after it was written.
#include <atomic>

#include "segment.hpp"

namespace cal {
namespace {

constexpr int kNodeChunk = 256;            // result nodes of one node workgroup (one per thread in the index phase)
constexpr int kTickets = 64;               // concurrent count launches (on different streams) that may be in flight

__device__ unsigned int g_coalition_ticket[kTickets];   // zero at load; atomicInc wraps each back to zero

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
    int64_t F, Nout, Eout;     // (write) totals[0], totals[1] as the caller read them
    int64_t* batch_out;        // [Nout]
    float* x_out;              // [Nout, F] or null
    int64_t* ei_out;           // [2, Eout]
    int64_t* node_src;         // [Nout]
    int64_t* edge_src;         // [Eout]
    int ticket, nblk;
    int vec;                   // (write) the 16-byte row copy applies
};

// replica r: its graph's node range [nlo, nlo + nn) and column range [elo, elo + em) (all zero without a graph), its key row
// (null: everything stays) and threshold.  In mode 1 a graph with more nodes than the map's row length has no replica either.
struct Rep {
    int64_t nlo, nn, elo, em, th;
    const int32_t* row;
};

__device__ __forceinline__ Rep replica(const CoArgs& a, int64_t r) {
    Rep q{0, 0, 0, 0, 0, nullptr};
    const int64_t g = a.rg[r];
    if (g < 0 || g >= a.B) return q;
    seg_clamp(a.ptr, g, a.N, q.nlo, q.nn);
    seg_clamp(a.eptr, g, a.E, q.elo, q.em);
    if (a.mode == 1 && q.nn > a.mx) {
        q.nlo = q.nn = q.elo = q.em = 0;
        return q;
    }
    const int64_t k = a.rrow[r];
    if (k >= 0 && k < a.K) q.row = a.key + k * a.M;
    q.th = a.rth[r];
    return q;
}

// element e (a column in mode 0, a node in mode 1; inside [0, M)) stays in the replica
__device__ __forceinline__ bool elem_stays(const CoArgs& a, const Rep& q, int64_t e) {
    if (!q.row) return true;
    const int64_t k = q.row[e];
    return a.invert ? k >= q.th : k < q.th;
}

// column e of the replica's graph stays
__device__ __forceinline__ bool col_stays(const CoArgs& a, const Rep& q, int64_t e) {
    const int64_t u = a.ei[e], v = a.ei[a.E + e];
    if (!(u >= q.nlo && u < q.nlo + q.nn && v >= q.nlo && v < q.nlo + q.nn)) return false;
    return a.mode == 0 ? elem_stays(a, q, e) : elem_stays(a, q, u) && elem_stays(a, q, v);
}

// exclusive prefix of v over the workgroup's NT threads in thread order, the workgroup's sum in tot (two barriers); as in
// occlude.hip
template <int NT>
__device__ __forceinline__ long long wg_excl_sum(long long v, long long* red, long long& tot) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    long long inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const long long u = __shfl_up(inc, o, 64);
        if (lane >= o) inc += u;
    }
    __syncthreads();
    if (lane == 63) red[w] = inc;
    __syncthreads();
    long long base = 0, t = 0;
#pragma unroll
    for (int i = 0; i < NT / 64; ++i) {
        const long long r = red[i];
        base += i < w ? r : 0;
        t += r;
    }
    tot = t;
    return base + inc - v;
}

// grid R, NT threads
template <int NT>
__global__ void __launch_bounds__(NT) k_coalition_count(CoArgs a) {
    __shared__ long long red[NT / 64];
    __shared__ int wcnt[NT / 64];
    __shared__ int last;
    const int64_t r = blockIdx.x, R = a.R;
    const Rep q = replica(a, r);
    int64_t nodes = q.nn;
    if (a.mode == 1) {                                            // the map row: q.nn <= a.mx (replica()), uniform over the workgroup
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
        __threadfence();
        last = atomicInc(&g_coalition_ticket[a.ticket], (unsigned)(a.nblk - 1)) == (unsigned)(a.nblk - 1);
    }
    __syncthreads();
    if (!last) return;
    __threadfence();
    // the scan over the R replicas: thread t owns the run [t L, (t + 1) L) of replicas
    const int64_t L = (R + NT - 1) / NT, lo = (int64_t)threadIdx.x * L, hi = lo + L < R ? lo + L : R;
    long long sn = 0, se = 0, mn = 0, me = 0, empty = 0;
    for (int64_t p = lo; p < hi; ++p) {
        const long long n = __hip_atomic_load(a.cnt + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const long long e = __hip_atomic_load(a.cnt + R + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        sn += n;
        se += e;
        mn = n > mn ? n : mn;
        me = e > me ? e : me;
        empty += n == 0;
    }
    long long tn, te;
    long long on = wg_excl_sum<NT>(sn, red, tn), oe = wg_excl_sum<NT>(se, red, te);
    for (int64_t p = lo; p < hi; ++p) {
        a.ptr_out[p] = on;
        a.eptr_out[p] = oe;
        on += __hip_atomic_load(a.cnt + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        oe += __hip_atomic_load(a.cnt + R + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    mn = wg_max<NT>(mn, red);
    me = wg_max<NT>(me, red);
    empty = wg_sum<NT>(empty, red);
    if (threadIdx.x == 0) {
        a.ptr_out[R] = tn;
        a.eptr_out[R] = te;
        a.totals[0] = tn;
        a.totals[1] = te;
        a.totals[2] = mn;
        a.totals[3] = me;
        a.totals[4] = empty;
    }
}

// last index q in [0, n) with p[q] <= i; p non-decreasing with p[0] = 0 <= i (the replica that owns result node i, empty ones
// skipped; the node of a map row with i staying nodes in front of it that stays itself)
template <class T>
__device__ __forceinline__ int64_t owner(const T* p, int64_t n, int64_t i) {
    int64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (p[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// grid ceil(Nout / kNodeChunk) node workgroups, then R column workgroups; 256 threads
__global__ void __launch_bounds__(256) k_coalition_write(CoArgs a, int node_blocks) {
    __shared__ int64_t src[kNodeChunk];
    __shared__ int wcnt[4];
    const int64_t R = a.R;
    if ((int)blockIdx.x < node_blocks) {
        const int64_t i0 = (int64_t)blockIdx.x * kNodeChunk, i = i0 + threadIdx.x;
        int64_t s = -1;                                           // (no row)
        if (i < a.Nout) {
            const int64_t r = owner(a.ptr_out, R + 1, i);
            if (r < R) {
                const Rep q = replica(a, r);
                int64_t l = i - a.ptr_out[r];
                if (a.mode == 1 && q.nn > 0) l = owner(a.map + r * a.mx, q.nn, l);
                if (l < q.nn) {
                    s = q.nlo + l;
                    a.batch_out[i] = r;
                    a.node_src[i] = s;
                }
            }
        }
        if (!a.x_out) return;
        src[threadIdx.x] = s;
        __syncthreads();
        const int64_t left = a.Nout - i0;
        const unsigned rows = (unsigned)(left < kNodeChunk ? left : kNodeChunk);
        if (a.vec) {
            const unsigned F4 = (unsigned)(a.F >> 2), n = rows * F4;
            float4* out = reinterpret_cast<float4*>(a.x_out) + i0 * F4;
            for (unsigned t = threadIdx.x; t < n; t += 256) {
                const unsigned rr = t / F4, c = t - rr * F4;
                const int64_t sr = src[rr];
                if (sr < 0) continue;
                out[t] = reinterpret_cast<const float4*>(a.x + sr * a.F)[c];
            }
        } else {
            const unsigned F = (unsigned)a.F, n = rows * F;
            float* out = a.x_out + i0 * a.F;
            for (unsigned t = threadIdx.x; t < n; t += 256) {
                const unsigned rr = t / F, c = t - rr * F;
                const int64_t sr = src[rr];
                if (sr < 0) continue;
                out[t] = a.x[sr * a.F + c];
            }
        }
        return;
    }
    const int64_t r = (int64_t)((int)blockIdx.x - node_blocks);
    const Rep q = replica(a, r);
    const int32_t* row = a.mode == 1 ? a.map + r * a.mx : nullptr;
    const int64_t n0 = a.ptr_out[r], j0 = a.eptr_out[r], j1 = a.eptr_out[r + 1] < a.Eout ? a.eptr_out[r + 1] : a.Eout;
    int64_t carry = 0;
    for (int64_t base = 0; base < q.em; base += 256) {            // (q.em is uniform over the workgroup)
        const int64_t e = q.elo + base + threadIdx.x;
        const bool f = base + threadIdx.x < q.em && col_stays(a, q, e);
        int t;
        const int pos = wg_excl<256>(f, wcnt, t);
        const int64_t j = j0 + carry + pos;
        if (f && j < j1) {
            const int64_t u = a.ei[e] - q.nlo, v = a.ei[a.E + e] - q.nlo;      // (both inside [0, q.nn): col_stays)
            a.ei_out[j] = n0 + (row ? (int64_t)row[u] : u);
            a.ei_out[a.Eout + j] = n0 + (row ? (int64_t)row[v] : v);
            a.edge_src[j] = e;
        }
        carry += t;
    }
}

std::atomic<unsigned> g_coalition_calls{0};

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
    if (R == 0) {
        if (hipMemsetAsync(totals, 0, 5 * sizeof(int64_t), stream) != hipSuccess ||
            hipMemsetAsync(ptr_out, 0, sizeof(int64_t), stream) != hipSuccess ||
            hipMemsetAsync(edge_ptr_out, 0, sizeof(int64_t), stream) != hipSuccess) {
            cal::set_error("cal_coalition_count: hipMemsetAsync failed");
            return 1;
        }
        return 0;
    }
    CoArgs a = co_args(edge_index, E, N, ptr, edge_ptr, B, key, K, rep_graph, rep_row, rep_thresh, R, mode, invert, max_nodes, ws);
    a.ptr_out = ptr_out;
    a.eptr_out = edge_ptr_out;
    a.totals = totals;
    a.ticket = (int)(g_coalition_calls.fetch_add(1) % kTickets);
    a.nblk = (int)R;
    // wide workgroups once the average source graph has more columns than a 256-thread workgroup walks in a few chunks
    if (E / (B > 0 ? B : 1) > 2048)
        hipLaunchKernelGGL(k_coalition_count<1024>, dim3((unsigned)R), dim3(1024), 0, stream, a);
    else
        hipLaunchKernelGGL(k_coalition_count<256>, dim3((unsigned)R), dim3(256), 0, stream, a);
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
    CAL_REQUIRE(Nout >= 0 && Eout >= 0 && F >= 0 && F < (1 << 22), "Nout, Eout must be >= 0 and 0 <= F < 2^22");
    CAL_REQUIRE(R == 0 || (ptr_out && edge_ptr_out), "ptr_out / edge_ptr_out are null");
    CAL_REQUIRE(Nout == 0 || (batch_out && node_src), "batch_out / node_src are null");
    CAL_REQUIRE(Eout == 0 || (edge_index_out && edge_src), "edge_index_out / edge_src are null");
    CAL_REQUIRE(!x_out || (F > 0 && (N == 0 || x)), "x_out needs F > 0 and x");
    const int64_t nb = (Nout + kNodeChunk - 1) / kNodeChunk, eb = Eout > 0 ? R : 0;
    CAL_REQUIRE(nb + eb <= 0x7FFFFFFF, "too many elements");
    if (R == 0 || nb + eb == 0) return 0;
    CoArgs a = co_args(edge_index, E, N, ptr, edge_ptr, B, key, K, rep_graph, rep_row, rep_thresh, R, mode, invert, max_nodes, ws);
    a.x = x;
    a.F = F;
    a.ptr_out = const_cast<int64_t*>(ptr_out);
    a.eptr_out = const_cast<int64_t*>(edge_ptr_out);
    a.Nout = Nout;
    a.Eout = Eout;
    a.batch_out = batch_out;
    a.x_out = x_out;
    a.ei_out = edge_index_out;
    a.node_src = node_src;
    a.edge_src = edge_src;
    a.vec = x_out && F % 4 == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(x_out)) & 15) == 0;
    hipLaunchKernelGGL(k_coalition_write, dim3((unsigned)(nb + eb)), dim3(256), 0, stream, a, (int)nb);
    CAL_CHECK_LAUNCH("k_coalition_write");
    return 0;
}
