// Explanations of the causal attention (model.py:97-111): per-segment ranking, top-k selection and motif metrics.
//
// One segment = one graph's edge (or node) scores [seg_ptr[g], seg_ptr[g+1]) of score[i * stride].  Order: score
// descending, then element index ascending, NaN below every number; rank[i] = 0-based position inside the segment;
// mask[i] = rank[i] < k_g.  Metrics per segment: k_g, hits (gt among the selected), P (gt in the segment) and the ROC-AUC
// (R_pos - P(P+1)/2) / (P (m - P)) from the 1-based ascending average ranks of the positives (ties count one half).
//
// Scores become 32-bit keys that order like the floats (NaN -> 1, -0 -> +0; key 0 pads LDS rows and never counts), so the
// rank of element i is a count: #{key_j > key_i} + #{key_j == key_i, j < i}.
//
//  * segments of at most S = XS elements: k_explain_rank_lds, one group of G threads per segment (G = 64 .. 1024, the
//    smallest power of two covering the batch's largest segment; 256-thread workgroups hold 256 / G segments), keys in
//    LDS, every lane counts its element against the whole row read as uint4 broadcasts.  Ranking, mask and metrics in
//    this one launch; the metrics are integer sums reduced in a fixed order (no atomics).
//  * larger segments (m > S): the same kernel ranks every S-element chunk in LDS and writes the chunk's keys in sorted
//    order to ws; k_explain_rank_merge adds each element's count against every other chunk of its segment (binary
//    searches on the sorted chunks, staged through LDS); k_explain_rank_large reduces the mask and the metrics.  A batch
//    that mixes both kinds runs the three launches, the small segments finishing in the first.
//
// Undirected edges (cal_explain_rank_pairs): a column and its reverse (twin.hip) are one element.  k_pairs_compact writes the
// symmetrised score of every column and compacts each segment's representatives (the lower column of a pair, every unpaired
// column) in order to the front of the segment's rows in ws (a fixed-order ballot scan, as subgraph.hip compacts); the
// kernels above rank those rows (their lengths come from seg_len instead of seg_ptr[g+1]); k_pairs_scatter gives both
// columns of a pair the representative's rank and mask.  Two launches around the ranking's.
#include <math.h>

#include "common.hpp"

namespace cal {
namespace {

constexpr int XS = 2048;       // LDS capacity S (elements of one segment / chunk)
constexpr int XNT = 1024;      // threads of the large-segment workgroups
constexpr int XIT = XS / XNT;  // elements per lane at the widest group

struct RankArgs {
    const float* score;
    int64_t stride;
    const int64_t* seg_ptr;
    int64_t B, M, max_seg;
    double ratio;
    int64_t k;
    const uint8_t* gt;
    uint8_t* mask;
    int32_t* rank;
    double* metrics;
    uint32_t* skey;    // ws: chunk keys in sorted order [M]      (large segments only)
    int32_t* r2;       // ws: 2 x ascending average rank [M]     (large segments only)
    const int64_t* seg_len;   // or null: segment g is [seg_ptr[g], seg_ptr[g] + seg_len[g]) (compacted rows of the pair ranking)
};

__device__ __forceinline__ uint32_t score_key(float s) {
    if (s != s) return 1u;                                     // NaN: below every number
    const uint32_t u = s == 0.f ? 0u : __float_as_uint(s);     // -0 ranks as +0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ void seg_range(const RankArgs& a, int64_t g, int64_t& lo, int64_t& m) {
    int64_t l = a.seg_ptr[g], h = a.seg_ptr[g + 1];
    l = l < 0 ? 0 : (l > a.M ? a.M : l);
    if (a.seg_len) h = l + a.seg_len[g];
    h = h < l ? l : (h > a.M ? a.M : h);
    lo = l;
    m = h - l;
}

// k_g of a segment of m elements with P positives (k >= 0: top k; -1: ceil(ratio m); -2: P)
__device__ __forceinline__ int64_t sel_count(int64_t m, int64_t P, double ratio, int64_t k) {
    if (k >= 0) return k < m ? k : m;
    if (k == -1) {
        const double c = ceil(ratio * (double)m);
        return c < (double)m ? (int64_t)c : m;
    }
    return P;
}

__device__ __forceinline__ double seg_auc(int64_t m, int64_t P, int64_t r2) {
    if (P <= 0 || P >= m) return __builtin_nan("");
    return ((double)r2 * 0.5 - (double)P * (double)(P + 1) * 0.5) / ((double)P * (double)(m - P));
}

__device__ __forceinline__ void put_metrics(double* row, int64_t kg, int64_t hits, int64_t P, double auc) {
    row[0] = (double)kg; row[1] = (double)hits; row[2] = (double)P; row[3] = auc;
}

// sum over the G consecutive threads (whole waves) of this thread's group, every thread of the group gets it; all threads
// of the workgroup call it (two barriers).  Fixed order: wave butterflies, then the group's wave partials in wave order.
__device__ __forceinline__ int64_t group_total(int64_t v, int G, long long* red) {
    long long s = v;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    const int nw = G >> 6, w0 = (int)(threadIdx.x / G) * nw;
    long long t = 0;
    for (int i = 0; i < nw; ++i) t += red[w0 + i];
    return t;
}

// count of keys > key (gt) and >= key (ge) in a descending row of n keys
__device__ __forceinline__ int count_gt(const uint32_t* s, int n, uint32_t key) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s[mid] > key) lo = mid + 1; else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ int count_ge(const uint32_t* s, int n, uint32_t key) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s[mid] >= key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// grid (ceil(B / (NT / G)), chunks), NT threads; dynamic LDS: keys [NT/G][cap] u32, gt flags [NT/G][cap] u8, then (8-byte
// aligned) [NT/64] i64.
// cap = G x (elements per lane) >= min(max_seg, S).  Segments of at most cap elements are finished here (chunk 0 only); a
// segment above S (then G = NT = 1024, cap = S) gets its chunk blockIdx.y ranked locally; one above max_seg is not ranked
// (rank -1, mask 0, NaN metrics).
template <int NT>
__global__ void __launch_bounds__(NT) k_explain_rank_lds(RankArgs a, int G, int cap) {
    extern __shared__ __align__(16) uint32_t xlds[];
    const int spb = NT / G, grp = threadIdx.x / G, lt = threadIdx.x % G;
    uint32_t* sk = xlds + grp * cap;
    uint8_t* sg = reinterpret_cast<uint8_t*>(xlds + spb * cap) + grp * cap;
    long long* red = reinterpret_cast<long long*>(reinterpret_cast<char*>(xlds) + ((5 * spb * cap + 7) & ~7));
    const int64_t g = (int64_t)blockIdx.x * spb + grp;
    const int64_t c = blockIdx.y;
    int64_t lo = 0, m = 0;
    if (g < a.B) seg_range(a, g, lo, m);
    const bool bad = g < a.B && m > a.max_seg;
    const bool full = g < a.B && !bad && m <= cap && c == 0;
    const bool chunk = g < a.B && !bad && m > cap;             // (m > S here: cap = S whenever max_seg > S)
    const int64_t ulo = chunk ? c * XS : 0;
    const int un = full ? (int)m : (chunk && ulo < m ? (int)(m - ulo < XS ? m - ulo : XS) : 0);
    const int nq = (un + 3) & ~3;
    const int64_t base = lo + ulo;

    int64_t pc = 0;
    for (int q = lt; q < nq; q += G) {
        uint32_t key = 0u;
        uint8_t f = 0;
        if (q < un) {
            key = score_key(a.score[(base + q) * a.stride]);
            if (a.gt) f = a.gt[base + q] != 0;
        }
        sk[q] = key;
        sg[q] = f;
        pc += f;
    }
    if (bad && c == 0) {
        for (int64_t q = lt; q < m; q += G) {
            a.rank[lo + q] = -1;
            a.mask[lo + q] = 0;
        }
        if (a.metrics && lt == 0)
            for (int t = 0; t < 4; ++t) a.metrics[4 * g + t] = __builtin_nan("");
    }
    __syncthreads();

    const int nit = cap / G;
    uint32_t ki[XIT];
    int gtc[XIT], eqc[XIT], eqb[XIT];
#pragma unroll
    for (int it = 0; it < XIT; ++it) {
        const int q = lt + it * G;
        ki[it] = (it < nit && q < un) ? sk[q] : 0u;
        gtc[it] = eqc[it] = eqb[it] = 0;
    }
    for (int j = 0; j < nq; j += 4) {
        const uint4 kv = *reinterpret_cast<const uint4*>(sk + j);
        const uint32_t kj[4] = {kv.x, kv.y, kv.z, kv.w};
#pragma unroll
        for (int it = 0; it < XIT; ++it) {
            if (it < nit) {
                const int q = lt + it * G;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    gtc[it] += kj[t] > ki[it];
                    const int e = kj[t] == ki[it];
                    eqc[it] += e;
                    eqb[it] += e & (j + t < q);
                }
            }
        }
    }

    if (chunk) {                                                  // local rank + the chunk's keys in sorted order
#pragma unroll
        for (int it = 0; it < XIT; ++it) {
            const int q = lt + it * G;
            if (it < nit && q < un) {
                const int r = gtc[it] + eqb[it];
                a.rank[base + q] = r;
                a.skey[base + r] = ki[it];
            }
        }
    }
    const bool need_p = a.k == -2 || a.metrics;
    const int64_t P = need_p ? group_total(pc, G, red) : 0;     // (uniform condition: every thread takes the barriers)
    const int64_t kg = sel_count(m, P, a.ratio, a.k);
    int64_t hits = 0, r2 = 0;
    if (full) {
#pragma unroll
        for (int it = 0; it < XIT; ++it) {
            const int q = lt + it * G;
            if (it < nit && q < un) {
                const int r = gtc[it] + eqb[it];
                const bool sel = r < kg;
                a.rank[base + q] = r;
                a.mask[base + q] = sel;
                if (sg[q]) {
                    hits += sel;
                    r2 += 2 * (un - gtc[it] - eqc[it]) + eqc[it] + 1;
                }
            }
        }
    }
    if (a.metrics) {
        hits = group_total(hits, G, red);
        r2 = group_total(r2, G, red);
        if (full && lt == 0) put_metrics(a.metrics + 4 * g, kg, hits, P, seg_auc(m, P, r2));
    }
}

// grid (B, chunks), XNT threads: element counts against every chunk of its (large) segment -> final rank, 2 x average rank
__global__ void __launch_bounds__(XNT) k_explain_rank_merge(RankArgs a) {
    __shared__ uint32_t sk[XS];
    const int64_t g = blockIdx.x, c = blockIdx.y;
    int64_t lo, m;
    seg_range(a, g, lo, m);
    if (m <= XS || m > a.max_seg || c * XS >= m) return;          // (uniform over the workgroup)
    const int64_t ulo = c * XS;
    const int un = (int)(m - ulo < XS ? m - ulo : XS);
    uint32_t ki[XIT];
    int64_t before[XIT], gtt[XIT], eqt[XIT];
#pragma unroll
    for (int it = 0; it < XIT; ++it) {
        const int q = threadIdx.x + it * XNT;
        const bool v = q < un;
        ki[it] = v ? score_key(a.score[(lo + ulo + q) * a.stride]) : 0u;
        before[it] = v ? a.rank[lo + ulo + q] : 0;
        gtt[it] = eqt[it] = 0;
    }
    const int64_t nch = (m + XS - 1) / XS;
    for (int64_t cc = 0; cc < nch; ++cc) {
        const int n2 = (int)(m - cc * XS < XS ? m - cc * XS : XS);
        for (int t = threadIdx.x; t < n2; t += XNT) sk[t] = a.skey[lo + cc * XS + t];
        __syncthreads();
#pragma unroll
        for (int it = 0; it < XIT; ++it) {
            if ((int)threadIdx.x + it * XNT < un) {
                const int ng = count_gt(sk, n2, ki[it]), ne = count_ge(sk, n2, ki[it]);
                gtt[it] += ng;
                eqt[it] += ne - ng;
                if (cc < c) before[it] += ne;                          // equal keys of an earlier chunk: lower index
                else if (cc > c) before[it] += ng;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int it = 0; it < XIT; ++it) {
        const int q = threadIdx.x + it * XNT;
        if (q < un) {
            a.rank[lo + ulo + q] = (int32_t)before[it];
            a.r2[lo + ulo + q] = (int32_t)(2 * (m - gtt[it] - eqt[it]) + eqt[it] + 1);
        }
    }
}

// grid B, XNT threads: mask and metrics of the large segments
__global__ void __launch_bounds__(XNT) k_explain_rank_large(RankArgs a) {
    __shared__ long long red[XNT / 64];
    const int64_t g = blockIdx.x;
    int64_t lo, m;
    seg_range(a, g, lo, m);
    if (m <= XS || m > a.max_seg) return;
    int64_t pc = 0;
    if (a.gt)
        for (int64_t q = threadIdx.x; q < m; q += XNT) pc += a.gt[lo + q] != 0;
    const int64_t P = group_total(pc, XNT, red);
    const int64_t kg = sel_count(m, P, a.ratio, a.k);
    int64_t hits = 0, r2 = 0;
    for (int64_t q = threadIdx.x; q < m; q += XNT) {
        const bool sel = a.rank[lo + q] < kg;
        a.mask[lo + q] = sel;
        if (a.gt && a.gt[lo + q]) {
            hits += sel;
            r2 += a.r2[lo + q];
        }
    }
    if (a.metrics) {
        hits = group_total(hits, XNT, red);
        r2 = group_total(r2, XNT, red);
        if (threadIdx.x == 0) put_metrics(a.metrics + 4 * g, kg, hits, P, seg_auc(m, P, r2));
    }
}

struct PairArgs {
    const float* score;
    int64_t stride;
    const int64_t* seg_ptr;
    int64_t B, M, max_seg;
    const uint8_t* gt;
    const int32_t* twin;
    int reduce;                // 0 mean, 1 max, 2 min
    float* score_out;
    uint8_t* mask;
    int32_t* rank;
    float* cs;                 // ws: representatives' scores, compacted to the front of each segment's rows [M]
    int32_t* crank;            // ws: their ranks [M]
    int32_t* cpos;             // ws: row of a representative column [M]
    uint8_t* cgt;              // ws: their ground truth [M]
    uint8_t* cmask;            // ws: their masks [M]
    int64_t* seg_len;          // ws: representatives per segment [B] (the segment's length where it is not ranked)
};

__device__ __forceinline__ void pair_range(const PairArgs& a, int64_t g, int64_t& lo, int64_t& m) {
    int64_t l = a.seg_ptr[g], h = a.seg_ptr[g + 1];
    l = l < 0 ? 0 : (l > a.M ? a.M : l);
    h = h < l ? l : (h > a.M ? a.M : h);
    lo = l;
    m = h - l;
}

// the partner of column e of the segment [lo, lo + m), or -1: twin[e] inside the segment, not e itself, pointing back
__device__ __forceinline__ int64_t pair_of(const PairArgs& a, int64_t e, int64_t lo, int64_t m) {
    const int64_t t = a.twin[e];
    return (t >= lo && t < lo + m && t != e && a.twin[t] == e) ? t : -1;
}

// position of this thread's flag among the set flags of the workgroup's NT threads (exclusive), their count in tot;
// every thread of the workgroup calls it (two barriers)
template <int NT>
__device__ __forceinline__ int pair_excl(bool f, int* wcnt, int& tot) {
    const unsigned long long b = __ballot(f);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int pre = __popcll(b & ((1ull << lane) - 1ull));
    __syncthreads();
    if (lane == 0) wcnt[w] = __popcll(b);
    __syncthreads();
    int base = 0, t = 0;
#pragma unroll
    for (int i = 0; i < NT / 64; ++i) {
        const int v = wcnt[i];
        base += i < w ? v : 0;
        t += v;
    }
    tot = t;
    return base + pre;
}

// grid B, NT threads: score_out of every column; the representatives' scores and ground truth compacted in order
template <int NT>
__global__ void __launch_bounds__(NT) k_pairs_compact(PairArgs a) {
    __shared__ int wcnt[NT / 64];
    const int64_t g = blockIdx.x;
    int64_t lo, m;
    pair_range(a, g, lo, m);
    const bool bad = m > a.max_seg;
    int64_t carry = 0;
    for (int64_t base = 0; base < m; base += NT) {
        const int64_t q = base + threadIdx.x, e = lo + q;
        bool f = false;
        float sym = 0.f;
        uint8_t pos_gt = 0;
        if (q < m) {
            const int64_t t = pair_of(a, e, lo, m);
            sym = a.score[e * a.stride];
            if (a.gt) pos_gt = a.gt[e] != 0;
            if (t >= 0) {                                          // x: the lower column's score, so both columns get the same bits
                const float o = a.score[t * a.stride];
                const float x = e < t ? sym : o, y = e < t ? o : sym;
                if (a.reduce == 0) sym = (x + y) * 0.5f;
                else if (x != x || y != y) sym = __builtin_nanf("");
                else if (a.reduce == 1) sym = x >= y ? x : y;
                else sym = x <= y ? x : y;
                if (a.gt) pos_gt |= a.gt[t] != 0;
            }
            a.score_out[e] = sym;
            f = !bad && (t < 0 || e < t);
        }
        int tot;
        const int pos = pair_excl<NT>(f, wcnt, tot);
        if (f) {
            const int64_t p = lo + carry + pos;
            a.cs[p] = sym;
            a.cgt[p] = pos_gt;
            a.cpos[e] = (int32_t)p;
        }
        carry += tot;
    }
    if (threadIdx.x == 0) a.seg_len[g] = bad ? m : carry;
}

// grid B, NT threads: rank and mask of every column from its representative's row
template <int NT>
__global__ void __launch_bounds__(NT) k_pairs_scatter(PairArgs a) {
    const int64_t g = blockIdx.x;
    int64_t lo, m;
    pair_range(a, g, lo, m);
    const bool bad = m > a.max_seg;
    for (int64_t q = threadIdx.x; q < m; q += NT) {
        const int64_t e = lo + q;
        int32_t r = -1;
        uint8_t s = 0;
        if (!bad) {
            const int64_t t = pair_of(a, e, lo, m);
            int64_t p = a.cpos[t >= 0 && t < e ? t : e];
            p = p < 0 ? 0 : (p >= a.M ? a.M - 1 : p);
            r = a.crank[p];
            s = a.cmask[p];
        }
        a.rank[e] = r;
        a.mask[e] = s;
    }
}

int rank_launch(const RankArgs& a, hipStream_t stream) {
    const bool large = a.max_seg > XS;
    const int64_t nch = large ? (a.max_seg + XS - 1) / XS : 1;
    const int eff = (int)(a.max_seg < XS ? a.max_seg : XS);
    int G = 64;
    while (G < eff && G < XNT) G <<= 1;
    const int cap = (eff > 0 ? (eff + G - 1) / G : 1) * G;
    const int NT = G <= 256 ? 256 : G;
    const int spb = NT / G;
    const size_t lds = (((size_t)5 * spb * cap + 7) & ~(size_t)7) + (size_t)(NT / 64) * 8;
    const dim3 grid((unsigned)((a.B + spb - 1) / spb), (unsigned)nch);
    CAL_REQUIRE(grid.x <= 0x7FFFFFFFu, "too many segments");
    if (NT == 256) hipLaunchKernelGGL(k_explain_rank_lds<256>, grid, dim3(256), lds, stream, a, G, cap);
    else if (NT == 512) hipLaunchKernelGGL(k_explain_rank_lds<512>, grid, dim3(512), lds, stream, a, G, cap);
    else hipLaunchKernelGGL(k_explain_rank_lds<1024>, grid, dim3(1024), lds, stream, a, G, cap);
    CAL_CHECK_LAUNCH("k_explain_rank_lds");
    if (large) {
        hipLaunchKernelGGL(k_explain_rank_merge, dim3((unsigned)a.B, (unsigned)nch), dim3(XNT), 0, stream, a);
        CAL_CHECK_LAUNCH("k_explain_rank_merge");
        hipLaunchKernelGGL(k_explain_rank_large, dim3((unsigned)a.B), dim3(XNT), 0, stream, a);
        CAL_CHECK_LAUNCH("k_explain_rank_large");
    }
    return 0;
}

}  // namespace
}  // namespace cal

using namespace cal;

CAL_EXPORT int64_t cal_explain_ws(int64_t M, int64_t B) {
    (void)B;
    return 8 * (M > 0 ? M : 0) + 256;
}

CAL_EXPORT int64_t cal_explain_lds_cap(void) { return XS; }

CAL_EXPORT int cal_explain_rank(const float* score, int64_t stride, const int64_t* seg_ptr, int64_t B, int64_t M,
                                int64_t max_seg, double ratio, int64_t k, const uint8_t* gt, uint8_t* mask, int32_t* rank,
                                double* metrics, void* ws, int64_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CAL_REQUIRE(B >= 0 && M >= 0 && max_seg >= 0 && stride >= 1, "B, M, max_seg must be >= 0 and stride >= 1");
    CAL_REQUIRE(k >= -2, "k must be >= 0, -1 (ratio) or -2 (ground-truth count)");
    CAL_REQUIRE(k != -2 || gt, "k = -2 needs gt");
    CAL_REQUIRE(k != -1 || ratio >= 0.0, "k = -1 needs a ratio >= 0");
    CAL_REQUIRE(B == 0 || seg_ptr, "seg_ptr is null");
    CAL_REQUIRE(M == 0 || (score && mask && rank), "score / mask / rank are null");
    CAL_REQUIRE(max_seg < ((int64_t)1 << 30), "segments of 2^30 elements or more are not supported");
    if (B == 0) return 0;
    const bool large = max_seg > XS;
    const int64_t nch = large ? (max_seg + XS - 1) / XS : 1;
    CAL_REQUIRE(nch <= 65535, "max_seg too large");
    CAL_REQUIRE(!large || (ws && ws_bytes >= cal_explain_ws(M, B) && aligned16(ws)),
                "segments above cal_explain_lds_cap() need a 16-byte aligned ws of cal_explain_ws(M, B) bytes");
    RankArgs a{score, stride, seg_ptr, B, M, max_seg, ratio, k, gt, mask, rank, metrics,
               large ? (uint32_t*)ws : nullptr,
               large ? (int32_t*)((char*)ws + ((4 * M + 15) / 16) * 16) : nullptr};
    return rank_launch(a, stream);
}

CAL_EXPORT int64_t cal_explain_pairs_ws(int64_t M, int64_t B) {
    M = M > 0 ? M : 0;
    B = B > 0 ? B : 0;
    return 14 * M + 8 * B + 512 + cal_explain_ws(M, B);
}

CAL_EXPORT int cal_explain_rank_pairs(const float* score, int64_t stride, const int64_t* seg_ptr, int64_t B, int64_t M,
                                      int64_t max_seg, double ratio, int64_t k, const uint8_t* gt, const int32_t* twin,
                                      int reduce, float* score_out, uint8_t* mask, int32_t* rank, double* metrics, void* ws,
                                      int64_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CAL_REQUIRE(B >= 0 && M >= 0 && max_seg >= 0 && stride >= 1, "B, M, max_seg must be >= 0 and stride >= 1");
    CAL_REQUIRE(k >= -2, "k must be >= 0, -1 (ratio) or -2 (ground-truth count)");
    CAL_REQUIRE(k != -2 || gt, "k = -2 needs gt");
    CAL_REQUIRE(k != -1 || ratio >= 0.0, "k = -1 needs a ratio >= 0");
    CAL_REQUIRE(reduce >= 0 && reduce <= 2, "reduce must be 0 (mean), 1 (max) or 2 (min)");
    CAL_REQUIRE(B == 0 || seg_ptr, "seg_ptr is null");
    CAL_REQUIRE(M == 0 || (score && twin && score_out && mask && rank), "score / twin / score_out / mask / rank are null");
    CAL_REQUIRE(M < ((int64_t)1 << 31), "2^31 columns or more are not supported (twin is int32)");
    CAL_REQUIRE(max_seg < ((int64_t)1 << 30), "segments of 2^30 elements or more are not supported");
    if (B == 0) return 0;
    CAL_REQUIRE((max_seg + XS - 1) / XS <= 65535, "max_seg too large");
    CAL_REQUIRE(B <= 0x7FFFFFFF, "too many segments");
    CAL_REQUIRE(ws && ws_bytes >= cal_explain_pairs_ws(M, B) && aligned16(ws),
                "ws must be 16-byte aligned and hold cal_explain_pairs_ws(M, B) bytes");
    char* w = (char*)ws;
    const int64_t m16 = ((M + 15) / 16) * 16;                    // (every array starts 16-byte aligned)
    PairArgs p{score, stride, seg_ptr, B, M, max_seg, gt, twin, reduce, score_out, mask, rank,
               (float*)w, (int32_t*)(w + 4 * m16), (int32_t*)(w + 8 * m16), (uint8_t*)(w + 12 * m16),
               (uint8_t*)(w + 13 * m16), (int64_t*)(w + 14 * m16)};
    char* rw = w + 14 * m16 + ((8 * B + 15) / 16) * 16;
    hipLaunchKernelGGL(k_pairs_compact<256>, dim3((unsigned)B), dim3(256), 0, stream, p);
    CAL_CHECK_LAUNCH("k_pairs_compact");
    RankArgs a{p.cs, 1, seg_ptr, B, M, max_seg, ratio, k, gt ? p.cgt : nullptr, p.cmask, p.crank, metrics,
               (uint32_t*)rw, (int32_t*)(rw + ((4 * M + 15) / 16) * 16), p.seg_len};
    if (rank_launch(a, stream) != 0) return 1;
    hipLaunchKernelGGL(k_pairs_scatter<256>, dim3((unsigned)B), dim3(256), 0, stream, p);
    CAL_CHECK_LAUNCH("k_pairs_scatter");
    return 0;
}
