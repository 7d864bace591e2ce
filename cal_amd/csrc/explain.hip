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
//  * segments of at most S = kSegCap elements: k_explain_rank_lds, one group of G threads per segment (the geometry of
//    segment.hpp: G = 64 .. 1024 covers the batch's largest segment, 256-thread workgroups hold 256 / G segments), keys in
//    LDS, every lane counts its element against the whole row read as uint4 broadcasts.  Ranking, mask and metrics in
//    this one launch; the metrics are integer sums reduced in a fixed order (no atomics).
//  * larger segments (m > S): the same kernel ranks every S-element chunk in LDS and writes the chunk's keys in sorted
//    order to ws; k_explain_rank_merge adds each element's count against every other chunk of its segment (binary
//    searches on the sorted chunks, staged through LDS); k_explain_rank_large reduces the mask and the metrics.  A batch
//    that mixes both kinds runs the three launches, the small segments finishing in the first.
//
// Undirected edges (cal_explain_rank_pairs): a column and its reverse (twin.hip) are one element.  k_pairs_compact writes the
// symmetrised score of every column and compacts each segment's representatives (the lower column of a pair, every unpaired
// column) in order to the front of the segment's rows in ws (the fixed-order ballot scan of segment.hpp); the kernels above
// rank those rows (their lengths come from seg_len instead of seg_ptr[g+1]); k_pairs_scatter gives both columns of a pair the
// representative's rank and mask.  Two launches around the ranking's.
#include <math.h>

#include "segment.hpp"

namespace cal {
namespace {

constexpr int kIt = kSegCap / kSegWide;   // elements per lane at the widest group

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

__device__ __forceinline__ void seg_range(const RankArgs& a, int64_t g, int64_t& lo, int64_t& m) {
    seg_clamp(a.seg_ptr, g, a.M, lo, m);
    if (a.seg_len) {                                           // compacted rows: [lo, lo + seg_len[g]), clamped alike
        const int64_t n = a.seg_len[g], room = a.M - lo;
        m = n < 0 ? 0 : (n > room ? room : n);
    }
}

// (score_key, sel_count -- the k_g of a segment -- and seg_auc: rules.hpp)

__device__ __forceinline__ void put_metrics(double* row, int64_t kg, int64_t hits, int64_t P, double auc) {
    row[0] = (double)kg; row[1] = (double)hits; row[2] = (double)P; row[3] = auc;
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
    const SegUnit u = seg_unit(g < a.B, m, a.max_seg, cap, c);
    const bool bad = u.bad, full = u.full, chunk = u.chunk;
    const int un = u.un, nq = (un + 3) & ~3;
    const int64_t base = lo + u.ulo;

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
    uint32_t ki[kIt];
    int gtc[kIt], eqc[kIt], eqb[kIt];
#pragma unroll
    for (int it = 0; it < kIt; ++it) {
        const int q = lt + it * G;
        ki[it] = (it < nit && q < un) ? sk[q] : 0u;
        gtc[it] = eqc[it] = eqb[it] = 0;
    }
    for (int j = 0; j < nq; j += 4) {
        const uint4 kv = *reinterpret_cast<const uint4*>(sk + j);
        const uint32_t kj[4] = {kv.x, kv.y, kv.z, kv.w};
#pragma unroll
        for (int it = 0; it < kIt; ++it) {
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
        for (int it = 0; it < kIt; ++it) {
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
        for (int it = 0; it < kIt; ++it) {
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

// grid (B, chunks), kSegWide threads: element counts against every chunk of its (large) segment -> final rank, 2 x average
// rank
__global__ void __launch_bounds__(kSegWide) k_explain_rank_merge(RankArgs a) {
    __shared__ uint32_t sk[kSegCap];
    const int64_t g = blockIdx.x, c = blockIdx.y;
    int64_t lo, m;
    seg_range(a, g, lo, m);
    if (m <= kSegCap || m > a.max_seg || c * kSegCap >= m) return;   // (uniform over the workgroup)
    const int64_t ulo = c * kSegCap;
    const int un = (int)(m - ulo < kSegCap ? m - ulo : kSegCap);
    uint32_t ki[kIt];
    int64_t before[kIt], gtt[kIt], eqt[kIt];
#pragma unroll
    for (int it = 0; it < kIt; ++it) {
        const int q = threadIdx.x + it * kSegWide;
        const bool v = q < un;
        ki[it] = v ? score_key(a.score[(lo + ulo + q) * a.stride]) : 0u;
        before[it] = v ? a.rank[lo + ulo + q] : 0;
        gtt[it] = eqt[it] = 0;
    }
    const int64_t nch = (m + kSegCap - 1) / kSegCap;
    for (int64_t cc = 0; cc < nch; ++cc) {
        const int n2 = (int)(m - cc * kSegCap < kSegCap ? m - cc * kSegCap : kSegCap);
        for (int t = threadIdx.x; t < n2; t += kSegWide) sk[t] = a.skey[lo + cc * kSegCap + t];
        __syncthreads();
#pragma unroll
        for (int it = 0; it < kIt; ++it) {
            if ((int)threadIdx.x + it * kSegWide < un) {
                const uint32_t key = ki[it];                      // (a descending row: the keys > key, then those == key)
                const int ng = first_false(sk, n2, [key](uint32_t x) { return x > key; });
                const int ne = first_false(sk, n2, [key](uint32_t x) { return x >= key; });
                gtt[it] += ng;
                eqt[it] += ne - ng;
                if (cc < c) before[it] += ne;                          // equal keys of an earlier chunk: lower index
                else if (cc > c) before[it] += ng;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int it = 0; it < kIt; ++it) {
        const int q = threadIdx.x + it * kSegWide;
        if (q < un) {
            a.rank[lo + ulo + q] = (int32_t)before[it];
            a.r2[lo + ulo + q] = (int32_t)(2 * (m - gtt[it] - eqt[it]) + eqt[it] + 1);
        }
    }
}

// grid B, kSegWide threads: mask and metrics of the large segments
__global__ void __launch_bounds__(kSegWide) k_explain_rank_large(RankArgs a) {
    __shared__ long long red[kSegWide / 64];
    const int64_t g = blockIdx.x;
    int64_t lo, m;
    seg_range(a, g, lo, m);
    if (m <= kSegCap || m > a.max_seg) return;
    int64_t pc = 0;
    if (a.gt)
        for (int64_t q = threadIdx.x; q < m; q += kSegWide) pc += a.gt[lo + q] != 0;
    const int64_t P = wg_sum<kSegWide>(pc, red);
    const int64_t kg = sel_count(m, P, a.ratio, a.k);
    int64_t hits = 0, r2 = 0;
    for (int64_t q = threadIdx.x; q < m; q += kSegWide) {
        const bool sel = a.rank[lo + q] < kg;
        a.mask[lo + q] = sel;
        if (a.gt && a.gt[lo + q]) {
            hits += sel;
            r2 += a.r2[lo + q];
        }
    }
    if (a.metrics) {
        hits = wg_sum<kSegWide>(hits, red);
        r2 = wg_sum<kSegWide>(r2, red);
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

// the partner of column e of the segment [lo, lo + m), or -1: twin[e] inside the segment, not e itself, pointing back
__device__ __forceinline__ int64_t pair_of(const PairArgs& a, int64_t e, int64_t lo, int64_t m) {
    const int64_t t = a.twin[e];
    return (t >= lo && t < lo + m && t != e && a.twin[t] == e) ? t : -1;
}

// grid B, NT threads: score_out of every column; the representatives' scores and ground truth compacted in order
template <int NT>
__global__ void __launch_bounds__(NT) k_pairs_compact(PairArgs a) {
    __shared__ int wcnt[NT / 64];
    const int64_t g = blockIdx.x;
    int64_t lo, m;
    seg_clamp(a.seg_ptr, g, a.M, lo, m);
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
        const int pos = wg_excl<NT>(f, wcnt, tot);
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
    seg_clamp(a.seg_ptr, g, a.M, lo, m);
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

int rank_launch(const RankArgs& a, const SegGeom& q, hipStream_t stream) {
    const size_t lds = (((size_t)5 * q.spb * q.cap + 7) & ~(size_t)7) + (size_t)(q.NT / 64) * 8;
    CAL_REQUIRE(q.grid_ok(), "too many segments");
    CAL_SEG_LAUNCH(k_explain_rank_lds, q, lds, stream, a);
    CAL_CHECK_LAUNCH("k_explain_rank_lds");
    if (q.large) {
        hipLaunchKernelGGL(k_explain_rank_merge, dim3((unsigned)a.B, (unsigned)q.nch), dim3(kSegWide), 0, stream, a);
        CAL_CHECK_LAUNCH("k_explain_rank_merge");
        hipLaunchKernelGGL(k_explain_rank_large, dim3((unsigned)a.B), dim3(kSegWide), 0, stream, a);
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

CAL_EXPORT int64_t cal_explain_lds_cap(void) { return kSegCap; }

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
    const SegGeom q = seg_geom(max_seg, B);
    const bool large = q.large;
    CAL_REQUIRE(q.chunks_ok(), "max_seg too large");
    CAL_REQUIRE(!large || (ws && ws_bytes >= cal_explain_ws(M, B) && aligned16(ws)),
                "segments above cal_explain_lds_cap() need a 16-byte aligned ws of cal_explain_ws(M, B) bytes");
    RankArgs a{score, stride, seg_ptr, B, M, max_seg, ratio, k, gt, mask, rank, metrics,
               large ? (uint32_t*)ws : nullptr,
               large ? (int32_t*)((char*)ws + ((4 * M + 15) / 16) * 16) : nullptr};
    return rank_launch(a, q, stream);
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
    const SegGeom q = seg_geom(max_seg, B);
    CAL_REQUIRE(q.chunks_ok(), "max_seg too large");
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
    if (rank_launch(a, q, stream) != 0) return 1;
    hipLaunchKernelGGL(k_pairs_scatter<256>, dim3((unsigned)B), dim3(256), 0, stream, p);
    CAL_CHECK_LAUNCH("k_pairs_scatter");
    return 0;
}
