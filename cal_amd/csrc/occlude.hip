// Occlusion replicas and rank agreement: the two device operators behind cal_amd/occlude.py.
//
// (1) cal_occlude_count / cal_occlude_write: replica r is graph g = rep_graph[r] of the batch with one element removed.  Graph g
// owns the nodes [ptr[g], ptr[g+1]) and the edge_index columns [edge_ptr[g], edge_ptr[g+1]); rep_elem[r] is a global column id
// (mode 0: that column goes, and its twin column when a twin map is given) or a global node id (mode 1: the node's row goes, later
// nodes move down by one, every column incident to it goes, the remaining endpoints are rewritten).  An element that is not one
// of g's removes nothing (the control replica); a graph id outside the batch gives a replica with nothing in it.  A source
// column with an endpoint outside its graph's node range is dropped.  Every integer output is uniquely determined (the host
// twin and a plain-torch restatement agree bit for bit); the feature rows are copies.  The rule is OccSrc of rules.hpp (occ_src,
// replica, node_stays, col_stays), which the host twin compiles too; the kernels and the launches are the restriction pair of
// restrict.hpp in its closed form (no node map: ws holds the counts alone).  A replica drops a different set of columns each,
// so one column workgroup per replica walks the source graph's columns (the replicas of an occlusion run are small graphs, one
// chunk each).  Here: the two entry points' checks.
//
// (2) cal_rank_agreement: per segment the ten integer counts two score vectors' rank correlations are made of (Spearman's rho
// from the doubled mid-ranks, Kendall's tau-b from the concordant / discordant / tied pairs, the top-k overlap).  Each lane owns
// an element i and loops over the segment's (a, b) pairs staged in LDS as broadcast reads, the counting of twin.hip.  Segments
// within kSegCap: one launch (the geometry of segment.hpp: G = 64 .. 1024 threads per segment).  Longer ones: workgroup
// (g, c) owns the rows [c S, (c + 1) S) of segment g and stages the segment tile by tile; its partial sums go to ws and
// k_agree_finish adds them per segment in chunk order.  Integers only: the same bits in any order.
#include "restrict.hpp"

namespace cal {
namespace {

constexpr int kAgIt = kSegCap / kSegWide;  // elements per lane at the widest group
constexpr int kAgPart = 9;                 // a row chunk's partial: the eight sums (pair counts doubled) and n

// ---- rank agreement ------------------------------------------------------------------------------------------------------------
struct AgArgs {
    const float* a;            // [M]
    const float* b;            // [M]
    int64_t M;
    const int64_t* seg;        // [B + 1]
    int64_t B, max_seg;
    const uint8_t* sel;        // [M] or null
    int64_t k;                 // >= 0 top k, -1 ceil(ratio n)
    double ratio;
    int64_t* counts;           // [B, 10]
    int64_t* part;             // ws [slots, kAgPart] (large launches)
    int large;
};

// the (a, b) of element i of the batch, NaN twice when it does not take part
__device__ __forceinline__ float2 ag_load(const AgArgs& a, int64_t i, bool& part) {
    float2 v = make_float2(a.a[i], a.b[i]);
    part = (!a.sel || a.sel[i] != 0) && v.x == v.x && v.y == v.y;
    if (!part) v.x = v.y = __builtin_nanf("");
    return v;
}

// slot of row chunk c of segment g (at lo) in part[]: chunks of earlier segments number at most floor(lo / S) + g
__device__ __forceinline__ int64_t ag_slot(int64_t lo, int64_t g, int64_t c) { return lo / kSegCap + g + c; }

__device__ __forceinline__ void ag_write(int64_t* row, int64_t n, const long long* s, int64_t kg) {
    row[0] = n;
    row[1] = s[0] / 2;
    row[2] = s[1] / 2;
    row[3] = s[2] / 2;
    row[4] = s[3] / 2;
    row[5] = s[4];
    row[6] = s[5];
    row[7] = s[6];
    row[8] = kg;
    row[9] = s[7];
}

// grid (ceil(B / (NT / G)), row chunks), NT threads; dynamic LDS: (a, b) [NT/G][cap] float2, then [NT/64] i64.
// cap = G x (elements per lane) >= min(max_seg, S).  A launch whose max_seg is within S finishes every segment here (one tile);
// otherwise G = NT = 1024, cap = S, one segment per workgroup, and the workgroup owns the rows [c S, (c + 1) S) of it.
template <int NT>
__global__ void __launch_bounds__(NT) k_agree(AgArgs a, int G, int cap) {
    extern __shared__ __align__(16) float2 alds[];
    const int spb = NT / G, grp = threadIdx.x / G, lt = threadIdx.x % G;
    float2* sv = alds + (size_t)grp * cap;
    long long* red = reinterpret_cast<long long*>(alds + (size_t)spb * cap);
    const int64_t g = (int64_t)blockIdx.x * spb + grp, c = blockIdx.y;
    int64_t lo = 0, m = 0;
    if (g < a.B) seg_clamp(a.seg, g, a.M, lo, m);
    const bool work = g < a.B && m <= a.max_seg, bad = g < a.B && m > a.max_seg;
    const int64_t rlo = c * kSegCap;
    const int rn = work && rlo < m ? (int)(m - rlo < cap ? m - rlo : cap) : 0;       // rows of this group
    // tiles of j: one in a launch without large segments; else (one segment per workgroup: uniform) the segment's, none when
    // this workgroup has no row
    const int nt = a.large ? (rn > 0 ? (int)((m + kSegCap - 1) / kSegCap) : 0) : 1;
    const int nit = cap / G;

    float ai[kAgIt], bi[kAgIt];
    bool pi[kAgIt];
    int64_t gi[kAgIt];
    int la[kAgIt], ea[kAgIt], ga[kAgIt], fa[kAgIt], lb[kAgIt], eb[kAgIt], gb[kAgIt], fb[kAgIt], cc[kAgIt], dd[kAgIt];
#pragma unroll
    for (int it = 0; it < kAgIt; ++it) {
        const int q = lt + it * G;
        pi[it] = false;
        gi[it] = rlo + q;
        ai[it] = bi[it] = __builtin_nanf("");
        if (it < nit && q < rn) {
            const float2 v = ag_load(a, lo + gi[it], pi[it]);
            ai[it] = v.x;
            bi[it] = v.y;
        }
        la[it] = ea[it] = ga[it] = fa[it] = lb[it] = eb[it] = gb[it] = fb[it] = cc[it] = dd[it] = 0;
    }
    long long pc = 0;
    for (int t = 0; t < nt; ++t) {
        const int64_t tlo = (int64_t)t * kSegCap;
        const int tn = work && tlo < m ? (int)(m - tlo < cap ? m - tlo : cap) : 0;
        for (int s = lt; s < tn; s += G) {
            bool p;
            sv[s] = ag_load(a, lo + tlo + s, p);
            pc += p;
        }
        __syncthreads();
        for (int j = 0; j < tn; ++j) {
            const float2 v = sv[j];                                // (every lane of the group the same address: a broadcast)
#pragma unroll
            for (int it = 0; it < kAgIt; ++it) {
                if (it < nit) {
                    const int before = tlo + j < gi[it];
                    const int lta = v.x < ai[it], gta = v.x > ai[it], eqa = v.x == ai[it];
                    const int ltb = v.y < bi[it], gtb = v.y > bi[it], eqb = v.y == bi[it];
                    la[it] += lta;
                    ga[it] += gta;
                    ea[it] += eqa;
                    fa[it] += eqa & before;
                    lb[it] += ltb;
                    gb[it] += gtb;
                    eb[it] += eqb;
                    fb[it] += eqb & before;
                    cc[it] += (lta & ltb) | (gta & gtb);
                    dd[it] += (lta & gtb) | (gta & ltb);
                }
            }
        }
        __syncthreads();
    }
    const int64_t n = group_total(pc, G, red);
    const int64_t kg = ag_sel_count(n, a.ratio, a.k);
    long long s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int it = 0; it < kAgIt; ++it) {
        if (pi[it]) {
            const long long ra = 2ll * la[it] + ea[it] + 1, rb = 2ll * lb[it] + eb[it] + 1;
            s[0] += cc[it];
            s[1] += dd[it];
            s[2] += ea[it] - 1;
            s[3] += eb[it] - 1;
            s[4] += ra * ra;
            s[5] += rb * rb;
            s[6] += ra * rb;
            s[7] += (ga[it] + fa[it] < kg) && (gb[it] + fb[it] < kg);
        }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) s[i] = group_total(s[i], G, red);
    if (lt != 0 || g >= a.B) return;
    if (!a.large) {
        if (bad) {
            for (int i = 0; i < 8; ++i) s[i] = 0;
        }
        ag_write(a.counts + 10 * g, bad ? -1 : n, s, bad ? 0 : kg);
    } else if (rn > 0) {
        int64_t* p = a.part + ag_slot(lo, g, c) * kAgPart;
        for (int i = 0; i < 8; ++i) p[i] = s[i];
        p[8] = n;
    }
}

// one thread per segment: the row chunks' partials added in chunk order (a launch with large segments)
__global__ void __launch_bounds__(256) k_agree_finish(AgArgs a) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= a.B) return;
    int64_t lo, m;
    seg_clamp(a.seg, g, a.M, lo, m);
    long long s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int64_t n = 0;
    if (m > a.max_seg) {
        ag_write(a.counts + 10 * g, -1, s, 0);
        return;
    }
    const int64_t nch = (m + kSegCap - 1) / kSegCap;
    for (int64_t c = 0; c < nch; ++c) {
        const int64_t* p = a.part + ag_slot(lo, g, c) * kAgPart;
        for (int i = 0; i < 8; ++i) s[i] += p[i];
        n = p[8];
    }
    ag_write(a.counts + 10 * g, n, s, ag_sel_count(n, a.ratio, a.k));
}

int64_t ag_ws_need(int64_t M, int64_t B, int64_t max_seg) {
    if (max_seg <= kSegCap) return 0;
    return 8 * kAgPart * ((M > 0 ? M : 0) / kSegCap + (B > 0 ? B : 0) + 1) + 256;
}

}  // namespace
}  // namespace cal

using namespace cal;

// the checks both occlusion entry points share (CAL_REQUIRE names the entry point)
#define OCCLUDE_REQUIRE_INPUTS()                                                                                                 \
    CAL_RESTRICT_REQUIRE_HEAD(E >= 0 && N >= 0 && B >= 0 && R >= 0);                                                             \
    CAL_REQUIRE(R == 0 || (rep_graph && rep_elem), "rep_graph / rep_elem are null");                                             \
    CAL_RESTRICT_REQUIRE_TAIL(0, "ws must be 8-byte aligned and hold cal_occlude_ws(E, R) bytes");                               \
    const OccSrc src = occ_src({edge_index, E, N, ptr, edge_ptr, B, rep_graph, mode}, rep_elem, twin)

CAL_EXPORT int64_t cal_occlude_ws(int64_t, int64_t R) { return restrict_ws_need(R, 0, 0); }

CAL_EXPORT int cal_occlude_count(const int64_t* edge_index, int64_t E, int64_t N, const int64_t* ptr, const int64_t* edge_ptr,
                                 int64_t B, const int64_t* rep_graph, const int64_t* rep_elem, int64_t R, int mode,
                                 const int32_t* twin, int64_t* ptr_out, int64_t* edge_ptr_out, int64_t* totals, void* ws,
                                 int64_t ws_bytes, void* stream) {
    OCCLUDE_REQUIRE_INPUTS();
    CAL_REQUIRE(totals && ptr_out && edge_ptr_out, "totals / ptr_out / edge_ptr_out are null");
    return restrict_count(__func__, src, R, ptr_out, edge_ptr_out, totals, ws, (hipStream_t)stream);
}

CAL_EXPORT int cal_occlude_write(const int64_t* edge_index, int64_t E, int64_t N, const int64_t* ptr, const int64_t* edge_ptr,
                                 int64_t B, const int64_t* rep_graph, const int64_t* rep_elem, int64_t R, int mode,
                                 const int32_t* twin, const float* x, int64_t F, const int64_t* ptr_out,
                                 const int64_t* edge_ptr_out, int64_t Nout, int64_t Eout, int64_t* batch_out, float* x_out,
                                 int64_t* edge_index_out, int64_t* node_src, int64_t* edge_src, void* ws, int64_t ws_bytes,
                                 void* stream) {
    OCCLUDE_REQUIRE_INPUTS();
    CAL_REBATCH_REQUIRE_WRITE(R, !x_out || (F > 0 && (N == 0 || x)), "x_out needs F > 0 and x", Eout > 0 ? R : 0);
    return restrict_write(src, R, x, ptr_out, edge_ptr_out,
                          write_out(Nout, Eout, batch_out, x_out, edge_index_out, node_src, edge_src, F, x), nb, eb, ws,
                          (hipStream_t)stream);
}

CAL_EXPORT int64_t cal_rank_agreement_ws(int64_t M, int64_t B, int64_t max_seg) { return ag_ws_need(M, B, max_seg); }

CAL_EXPORT int cal_rank_agreement(const float* a_, const float* b_, int64_t M, const int64_t* seg_ptr, int64_t B, int64_t max_seg,
                                  const uint8_t* sel, int64_t k_code, double k_val, int64_t* counts, void* ws, int64_t ws_bytes,
                                  void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CAL_REQUIRE(M >= 0 && B >= 0 && max_seg >= 0, "M, B, max_seg must be >= 0");
    CAL_REQUIRE(max_seg < ((int64_t)1 << 20), "segments of 2^20 elements or more are not supported (the sums would leave int64)");
    CAL_REQUIRE(k_code >= -1, "k_code must be >= 0 or -1 (ratio)");
    CAL_REQUIRE(k_code != -1 || k_val >= 0.0, "k_code = -1 needs a ratio >= 0");
    if (B == 0) return 0;
    CAL_REQUIRE(seg_ptr && counts, "seg_ptr / counts are null");
    CAL_REQUIRE(M == 0 || (a_ && b_), "a / b are null");
    const SegGeom q = seg_geom(max_seg, B);
    CAL_REQUIRE(q.chunks_ok(), "max_seg too large");
    CAL_REQUIRE(q.grid_ok(), "too many segments");
    CAL_REQUIRE(!q.large || (ws && ws_bytes >= ag_ws_need(M, B, max_seg) && (reinterpret_cast<uintptr_t>(ws) & 7) == 0),
                "ws must be 8-byte aligned and hold cal_rank_agreement_ws(M, B, max_seg) bytes");
    AgArgs a{a_, b_, M, seg_ptr, B, max_seg, sel, k_code, k_val, counts, (int64_t*)ws, q.large ? 1 : 0};
    const size_t lds = (size_t)8 * q.spb * q.cap + (size_t)(q.NT / 64) * 8;
    CAL_SEG_LAUNCH(k_agree, q, lds, stream, a);
    CAL_CHECK_LAUNCH("k_agree");
    if (q.large) {
        hipLaunchKernelGGL(k_agree_finish, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, stream, a);
        CAL_CHECK_LAUNCH("k_agree_finish");
    }
    return 0;
}
