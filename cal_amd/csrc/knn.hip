// k nearest neighbours of nq query rows in a bank of M rows (cal_knn): squared Euclidean or cosine distance, the k' nearest eligible
// rows of every query in ascending order of the 64-bit key (bits of the distance) << 32 | row, and the votes of their labels.  The
// [nq, M] distance matrix never exists; the workspace is one sorted k-list of keys per (query, chunk).  TWO launches:
//
//  1. k_knn_select  one workgroup = 4 waves = 32 queries x one chunk of the bank, walked in tiles of 128 bank rows.  The reduction
//                   runs in slices of 32: the 32 query rows and the 128 bank rows of a slice are staged row-major in LDS (row stride
//                   36 floats: conflict-free 16-byte reads) and each wave forms its 32 x 32 tile of q . x with mma_rowk of
//                   engine_mma.hpp; rows and widths are zero-padded to the slice, and a slice's rows are fetched into registers while
//                   the slice before is multiplied.  The squared norm of a row -- query or bank -- is
//                   ONE fmaf chain in ascending k, so a pair's distance (knn_dist of rules.hpp) has the same bits wherever the pair
//                   lands in a tile, a chunk or a call.  A lane then holds, for one bank row, the distances to 16 queries: it packs
//                   the keys (knn_key), drops those not below the query's threshold (LDS, all-ones at first) and appends the rest
//                   to the query's candidate buffer through an LDS counter.  A buffer that the next tile could overflow, and every
//                   buffer at the end of the chunk, is compacted by one wave to its k smallest keys in ascending order by counting
//                   ranks (keys are distinct: the rank of a key is the number of keys below it), and the threshold drops to the
//                   k-th.  The selected set is a function of the key set alone, whatever order the appends arrived in.
//  2. k_knn_merge   one wave per query: the chunks' lists are joined in chunk order, 64 keys against the k kept so far, by the same
//                   rank count; then idx, dist and the votes (an integer LDS count per class).
//
// No floating-point atomic, no ticket, no read-back: two calls give the same bits, and so does any chunking.
// LDS of k_knn_select: 4.5 KB queries + 18 KB bank slice + 48 KB candidates (32 x 192 keys) + 1.5 KB: two workgroups per CU.
// A buffer takes at most 128 appends per tile (one per bank row) on top of at most k <= 64 kept keys: 192 slots, compacted
// whenever more than 64 are in use, cannot overflow.
#include "engine_mma.hpp"

namespace cal {
namespace {

constexpr int KN_TR = 128;                       // bank rows of a tile (32 per wave)
constexpr int KN_KS = 32;                        // reduction slice staged in LDS
constexpr int KN_LD = 36;                        // row stride of the LDS tiles (= 4 mod 32)
constexpr int KN_CAP = kKnnMaxK + KN_TR;         // slots of a candidate buffer
static_assert(KN_CAP <= 3 * 64, "knn_compact ranks three keys per lane");

struct KnnArgs {
    const float *Q, *X;
    int64_t nq, M, rows, nch;
    int H, metric, k, C;
    const int64_t *skip, *labels;
    int32_t* idx;
    float* dist;
    int32_t* votes;
    uint64_t* lists;                             // ws: [nq, nch, k] keys, ascending, kKnnNone behind the last
};

// One wave: the n <= KN_CAP distinct keys c[0 .. n) (c 16-byte aligned) -> their min(n, k) smallest in ascending order in
// c[0 ..); returns that count.  *thr becomes the k-th smallest when there are k.  Lane l ranks the keys l, l + 64, .. (U of
// them: n <= 64 U); the keys are read two per 16-byte broadcast.  Every read of c precedes every write.
template <int U>
__device__ __forceinline__ void knn_rank(uint64_t* c, int n, int k, int lane, uint64_t* thr) {
    uint64_t mine[U];
    int rk[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        mine[u] = lane + 64 * u < n ? c[lane + 64 * u] : kKnnNone;
        rk[u] = 0;
    }
    int j = 0;
    for (; j + 2 <= n; j += 2) {
        const ulonglong2 kj = *reinterpret_cast<const ulonglong2*>(c + j);
#pragma unroll
        for (int u = 0; u < U; ++u) rk[u] += (kj.x < mine[u] ? 1 : 0) + (kj.y < mine[u] ? 1 : 0);
    }
    if (j < n) {
        const uint64_t kj = c[j];
#pragma unroll
        for (int u = 0; u < U; ++u) rk[u] += kj < mine[u] ? 1 : 0;
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int u = 0; u < U; ++u) {
        if (lane + 64 * u < n && rk[u] < k) {
            c[rk[u]] = mine[u];
            if (thr && rk[u] == k - 1) *thr = mine[u];
        }
    }
}
__device__ __forceinline__ int knn_compact(uint64_t* c, int n, int k, int lane, uint64_t* thr) {
    if (n <= 64) knn_rank<1>(c, n, k, lane, thr);                 // (n is uniform over the wave)
    else if (n <= 128) knn_rank<2>(c, n, k, lane, thr);
    else knn_rank<3>(c, n, k, lane, thr);
    return n < k ? n : k;
}

// grid (nch, ceil(nq / 32)), 256 threads
__global__ void __launch_bounds__(256, 2) k_knn_select(KnnArgs a) {
    __shared__ __align__(16) float qs[kKnnQB * KN_LD];
    __shared__ __align__(16) float xs[KN_TR * KN_LD];
    __shared__ __align__(16) uint64_t cand[kKnnQB * KN_CAP];
    __shared__ uint64_t thr[kKnnQB];
    __shared__ int64_t skip_s[kKnnQB];
    __shared__ int cnt[kKnnQB];
    __shared__ float qn_s[kKnnQB], xn_s[KN_TR];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, li = lane & 31, lk = lane >> 5;
    const int H = a.H, k = a.k;
    const int64_t chunk = blockIdx.x, q0 = (int64_t)blockIdx.y * kKnnQB;
    const int64_t j0 = chunk * a.rows, jend = min(a.M, j0 + a.rows);

    if (t < kKnnQB) {
        skip_s[t] = (a.skip && q0 + t < a.nq) ? a.skip[q0 + t] : -1;
        thr[t] = kKnnNone;
        cnt[t] = 0;
    }
    // (the first barrier of the tile loop publishes these; a chunk has at least one row)

    // a slice's rows come from memory one slice ahead, into registers: the loads fly under the products of the slice before
    float qr[4], xr[16];
    auto fetch = [&](int64_t t0, int k0) {                        // thread t: column k0 + (t & 31) of the rows (t >> 5) + 8 i
        const int kk = k0 + (t & 31);
        const int64_t qrow = q0 + (t >> 5), xrow = t0 + (t >> 5);
        const float* qp = a.Q + (size_t)qrow * H + kk;
        const float* xp = a.X + (size_t)xrow * H + kk;
#pragma unroll
        for (int i = 0; i < 4; ++i) qr[i] = (qrow + 8 * i < a.nq && kk < H) ? qp[(size_t)(8 * i) * H] : 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) xr[i] = (xrow + 8 * i < jend && kk < H) ? xp[(size_t)(8 * i) * H] : 0.f;
    };
    fetch(j0, 0);

    for (int64_t t0 = j0; t0 < jend; t0 += KN_TR) {
        gc_f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        float nrm = 0.f;                                          // t < 128: bank row t; 128 <= t < 160: query t - 128
        for (int k0 = 0; k0 < H; k0 += KN_KS) {
#pragma unroll
            for (int i = 0; i < 4; ++i) qs[((t + i * 256) >> 5) * KN_LD + (t & 31)] = qr[i];
#pragma unroll
            for (int i = 0; i < 16; ++i) xs[((t + i * 256) >> 5) * KN_LD + (t & 31)] = xr[i];
            __syncthreads();
            const bool endk = k0 + KN_KS >= H;
            if (!endk) fetch(t0, k0 + KN_KS);
            else if (t0 + KN_TR < jend) fetch(t0 + KN_TR, 0);
            if (t < KN_TR + kKnnQB) {                             // the row's norm: one chain in ascending k (the padding adds +0)
                const float* row = t < KN_TR ? xs + t * KN_LD : qs + (t - KN_TR) * KN_LD;
#pragma unroll
                for (int i = 0; i < KN_KS / 4; ++i) {
                    const float4 v = *reinterpret_cast<const float4*>(row + 4 * i);
                    nrm = fmaf(v.w, v.w, fmaf(v.z, v.z, fmaf(v.y, v.y, fmaf(v.x, v.x, nrm))));
                }
                if (endk) {
                    if (t < KN_TR) xn_s[t] = nrm;
                    else qn_s[t - KN_TR] = nrm;
                }
            }
            mma_rowk(qs + li * KN_LD, xs + (wave * 32 + li) * KN_LD, KN_KS, lk, acc);
            __syncthreads();
        }

        const int64_t j = t0 + wave * 32 + li;
        if (j < jend) {
            const float xnj = xn_s[wave * 32 + li];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ql = mma_row(r, lk);
                if (q0 + ql >= a.nq || !knn_eligible(j, skip_s[ql])) continue;
                const uint64_t key = knn_key(knn_dist<float>(a.metric, qn_s[ql], xnj, acc[r]), (uint32_t)j);
                if (key < thr[ql]) {
                    const int pos = atomicAdd(&cnt[ql], 1);
                    if (pos < KN_CAP) cand[ql * KN_CAP + pos] = key;
                }
            }
        }
        __syncthreads();
        const bool last = t0 + KN_TR >= jend;
        for (int ql = wave; ql < kKnnQB; ql += 4) {               // (uniform over the wave)
            const int n = min(cnt[ql], KN_CAP);
            if (!last && n <= KN_CAP - KN_TR) continue;
            const int m = knn_compact(cand + ql * KN_CAP, n, k, lane, thr + ql);
            if (lane == 0) cnt[ql] = m;
        }
    }
    __syncthreads();
    for (int i = t; i < kKnnQB * k; i += 256) {
        const int ql = i / k, p = i % k;
        if (q0 + ql < a.nq) a.lists[((size_t)(q0 + ql) * a.nch + chunk) * k + p] = p < cnt[ql] ? cand[ql * KN_CAP + p] : kKnnNone;
    }
}

// grid ceil(nq / 4), 256 threads: wave w merges query 4 blockIdx.x + w (a wave past the last query repeats the last one and
// stores nothing: the barriers stay uniform)
__global__ void __launch_bounds__(256) k_knn_merge(KnnArgs a) {
    __shared__ __align__(16) uint64_t buf_s[4][2 * 64];
    __shared__ int vt_s[4][kKnnMaxC];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, k = a.k;
    const int64_t qx = (int64_t)blockIdx.x * 4 + wave, q = min(qx, a.nq - 1);
    const bool live = qx < a.nq;
    uint64_t* buf = buf_s[wave];
    int n = 0;
    for (int64_t ch = 0; ch < a.nch; ++ch) {
        const uint64_t key = lane < k ? a.lists[((size_t)q * a.nch + ch) * k + lane] : kKnnNone;
        const unsigned long long has = __ballot(key != kKnnNone);
        if (key != kKnnNone) buf[n + __popcll(has & ((1ull << lane) - 1ull))] = key;
        const int n2 = n + __popcll(has);
        __syncthreads();
        n = a.nch == 1 ? n2 : knn_compact(buf, n2, k, lane, nullptr);
        __syncthreads();
    }
    const uint64_t key = lane < n ? buf[lane] : kKnnNone;
    const int32_t id = key != kKnnNone ? knn_key_idx(key) : -1;
    if (live && lane < k) {
        a.idx[(size_t)q * k + lane] = id;
        a.dist[(size_t)q * k + lane] = key != kKnnNone ? knn_key_dist(key) : INFINITY;
    }
    if (!a.votes) return;                                         // (uniform)
    int* vt = vt_s[wave];
    if (lane < a.C) vt[lane] = 0;
    __syncthreads();
    if (id >= 0 && a.labels) {
        const int64_t lab = a.labels[id];
        if (knn_votes_for(lab, a.C)) atomicAdd(&vt[lab], 1);
    }
    __syncthreads();
    if (live && lane < a.C) a.votes[(size_t)q * a.C + lane] = vt[lane];
}

}  // namespace
}  // namespace cal

using namespace cal;

CAL_EXPORT int64_t cal_knn_ws(int64_t nq, int64_t M, int64_t k, int64_t chunk_rows) {
    if (nq < 0 || M < 1 || k < 1 || k > kKnnMaxK) return 0;
    return nq * knn_chunks(M, knn_chunk_rows(nq, M, chunk_rows)) * k * 8 + 256;
}

CAL_EXPORT int cal_knn(const float* Q, int64_t nq, const float* X, int64_t M, int64_t H, int metric, int64_t k, const int64_t* skip,
                       const int64_t* labels, int64_t C, int32_t* idx, float* dist, int32_t* votes, int64_t chunk_rows, void* ws,
                       int64_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CAL_REQUIRE(nq >= 0, "nq must be >= 0");
    CAL_REQUIRE(M >= 1 && M < (1ll << 31), "M must be in [1, 2^31)");
    CAL_REQUIRE(H >= 1 && H <= kKnnMaxH, "H must be in [1, 256]");
    CAL_REQUIRE(k >= 1 && k <= kKnnMaxK, "k must be in [1, 64]");
    CAL_REQUIRE(metric == 0 || metric == 1, "metric must be 0 (squared Euclidean) or 1 (cosine)");
    CAL_REQUIRE(C >= 0 && C <= kKnnMaxC, "C must be in [0, 64]");
    CAL_REQUIRE(chunk_rows >= 0 && chunk_rows % 32 == 0, "chunk_rows must be 0 or a positive multiple of 32");
    if (nq == 0) return 0;
    CAL_REQUIRE(Q && X && idx && dist, "Q / X / idx / dist is null");
    CAL_REQUIRE(!votes || (labels && C >= 1), "votes needs labels and C >= 1");
    const int64_t rows = knn_chunk_rows(nq, M, chunk_rows), nch = knn_chunks(M, rows), nqb = (nq + kKnnQB - 1) / kKnnQB;
    CAL_REQUIRE(nqb <= 65535, "nq too large (at most 65535 query blocks of 32 per call)");
    CAL_REQUIRE(ws && ws_bytes >= cal_knn_ws(nq, M, k, chunk_rows) && (reinterpret_cast<uintptr_t>(ws) & 15) == 0,
                "ws must be 16-byte aligned and hold cal_knn_ws(nq, M, k, chunk_rows) bytes");
    KnnArgs a;
    a.Q = Q; a.X = X; a.nq = nq; a.M = M; a.rows = rows; a.nch = nch; a.H = (int)H; a.metric = metric; a.k = (int)k; a.C = (int)C;
    a.skip = skip; a.labels = labels; a.idx = idx; a.dist = dist; a.votes = votes; a.lists = (uint64_t*)ws;
    hipLaunchKernelGGL(k_knn_select, dim3((unsigned)nch, (unsigned)nqb), dim3(256), 0, stream, a);
    CAL_CHECK_LAUNCH("k_knn_select");
    hipLaunchKernelGGL(k_knn_merge, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, stream, a);
    CAL_CHECK_LAUNCH("k_knn_merge");
    return 0;
}
