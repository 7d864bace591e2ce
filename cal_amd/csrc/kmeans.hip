// Lloyd's k-means over N rows of width H with K centroids (cal_kmeans, cal_kmeans_assign): every row goes to the centroid with the
// smallest 64-bit key (bits of the squared distance) << 32 | centroid, a cluster's new centroid is the mean of its rows summed in
// the fixed order of rules.hpp.  The rows are read from memory ONCE per iteration, the [N, K] distances never exist, and no
// floating-point sum depends on an arrival order.  TWO launches per iteration:
//
//  1. k_km_step    one workgroup = 4 waves = one superblock of kmeans_span rows, walked in tiles of TR rows.  The K centroids,
//                  zero-padded to KP = 32 or 64 rows of Hp = ceil32(H) columns (row stride Hp + 4 = 4 mod 32: conflict-free
//                  16-byte reads), and their squared norms stay in LDS for the whole launch.  A tile is staged WHOLE, row-major
//                  with the same stride; wave w forms the 32 x 32 tile (centroid tile w / nrt) x (row tile w % nrt) of c . x
//                  with mma_rowk of engine_mma.hpp while the last wave forms the rows' norms -- ONE fmaf chain in ascending
//                  k, as in knn.hip, so a pair's distance has the same bits wherever the row lands.  A lane then holds one
//                  row's distances to 16 centroids: it takes the minimum of their keys, joins the other half of the row's lanes
//                  by one exchange, and an integer LDS minimum joins the centroid tiles.  Then, the tile still in LDS, the
//                  cluster sums: thread (g, h) owns column h of the clusters c = g mod G and walks the tile's rows in ascending
//                  order, adding into a [K, H] LDS accumulator that lives across the tiles of the superblock -- the chain of
//                  the rule, literally (eight rows per LDS round trip, a row taking an earlier row's new value where the two
//                  share a cluster).  One thread chains the fp64 inertia the same way; counts and moved rows are integer LDS
//                  atomics.  At the end the workgroup stores its partial sums, counts, inertia and moved count to ws.
//  2. k_km_update  one thread per (c, h): the superblocks' partials in ascending order, kmeans_mean, counts; thread 0 also
//                  inertia[it], moved[it], iters_run and the stop flag.
//
// Early exit without a read-back: ws holds `stop`, the first iteration whose work is skipped (INT_MAX while not converged).
// The update of iteration it writes it + 1 there when nothing moved; both kernels of a later iteration return at once.  The
// kernels of iteration `it` only ever see values above `it` while they run (the old INT_MAX or the new it + 1), so a late
// workgroup of the update kernel cannot mistake its own launch's flag.  Iteration 0 does not read it: ws needs no zeroing.
//
// LDS of k_km_step, all dynamic: centroids KP (Hp + 4) + tile TR (Hp + 4) + accumulator K H floats + KP norms + TR x 20 B + KP
// counts.  TR is the largest of 64, 32, 16 that fits 160 KB (MI355X: 160 KB per CU).  H = 128, K = 16: 16.9 + 33.8 + 8 KB = 60 KB,
// two workgroups per CU; H = 128, K = 64: 33.8 + 33.8 + 32 = 101 KB, one; at the limits H = 256, K = 64: 66.6 + 64 + 16.6 (TR = 16:
// the MFMA tile is half empty there) = 149 KB, one.  The accumulator stays in LDS at every shape: no second pass over a tile.
// Registers (hipcc, gfx950): k_km_step<true> 102 VGPRs + 16 AGPRs, k_km_step<false> 94 + 16 (4 waves per SIMD by registers),
// k_km_update 49; no scratch.  LDS, not registers, bounds the occupancy of the step kernel: one or two workgroups per CU.
#include <limits.h>

#include "engine_mma.hpp"

namespace cal {
namespace {

constexpr int KM_LDS_MAX = 160 * 1024;
constexpr int KM_U = 8;                          // rows of the sum phase per LDS round trip (divides every TR)

struct KmShape {
    int H, K, KP, Hp, LDH, TR, G, vec;           // G: cluster groups of the sum phase (a power of two, G H <= 256); vec: 16-byte loads
    int lds;                                     // bytes of dynamic LDS
};

struct KmArgs {
    const float *X, *C;
    int64_t N, span;
    KmShape s;
    int it;
    int32_t* assign;
    float* dist;                                 // (assign mode)
    float* psum;                                 // ws: [spans, K, H]
    double* pin;                                 //     [spans]
    int32_t *pcnt, *pmv;                         //     [spans, K], [spans]
    const int32_t* stop;
};

struct KmUpdArgs {
    const float* Cold;
    float* Cout;
    const float* psum;
    const double* pin;
    const int32_t *pcnt, *pmv;
    int64_t spans;
    int K, H, it;
    int64_t* counts;
    double* inertia;
    int64_t* moved;
    int32_t *iters_run, *stop;
};

__host__ __device__ constexpr int km_al16(int b) { return (b + 15) & ~15; }
// byte offsets of the LDS regions, in this order: centroids, tile, accumulator, keys, centroid norms, row norms, row distances,
// row clusters, counts, moved
struct KmLds { int cs, xt, acc, key, cn, xn, dst, asg, cnt, mv, end; };
__host__ __device__ inline KmLds km_lds(int KP, int LDH, int TR, int K, int H, bool sums) {
    KmLds l;
    l.cs = 0;
    l.xt = l.cs + km_al16(KP * LDH * 4);
    l.acc = l.xt + km_al16(TR * LDH * 4);
    l.key = l.acc + (sums ? km_al16(K * H * 4) : 0);
    l.cn = l.key + km_al16(TR * 8);
    l.xn = l.cn + km_al16(KP * 4);
    l.dst = l.xn + km_al16(TR * 4);
    l.asg = l.dst + km_al16(TR * 4);
    l.cnt = l.asg + km_al16(TR * 4);
    l.mv = l.cnt + km_al16(KP * 4);
    l.end = l.mv + 16;
    return l;
}

// one ascending fmaf chain over the n (a multiple of 4) floats of an LDS row
__device__ __forceinline__ float km_norm(const float* row, int n) {
    float nrm = 0.f;
    for (int i = 0; i < n; i += 4) {
        const float4 v = *reinterpret_cast<const float4*>(row + i);
        nrm = fmaf(v.w, v.w, fmaf(v.z, v.z, fmaf(v.y, v.y, fmaf(v.x, v.x, nrm))));
    }
    return nrm;
}

// grid spans, 256 threads.  SUMS: a Lloyd step (partials to ws); otherwise assign and dist only.
template <bool SUMS>
__global__ void __launch_bounds__(256) k_km_step(KmArgs a) {
    extern __shared__ __align__(16) char km_smem[];
    if (SUMS && a.it > 0 && __atomic_load_n(a.stop, __ATOMIC_RELAXED) <= a.it) return;      // (uniform) converged earlier
    const KmShape s = a.s;
    const int H = s.H, K = s.K, KP = s.KP, Hp = s.Hp, LDH = s.LDH, TR = s.TR;
    const KmLds l = km_lds(KP, LDH, TR, K, H, SUMS);
    float* cs = reinterpret_cast<float*>(km_smem + l.cs);
    float* xt = reinterpret_cast<float*>(km_smem + l.xt);
    float* acc_s = reinterpret_cast<float*>(km_smem + l.acc);
    unsigned long long* key_s = reinterpret_cast<unsigned long long*>(km_smem + l.key);
    float* cn_s = reinterpret_cast<float*>(km_smem + l.cn);
    float* xn_s = reinterpret_cast<float*>(km_smem + l.xn);
    float* dst_s = reinterpret_cast<float*>(km_smem + l.dst);
    int* asg_s = reinterpret_cast<int*>(km_smem + l.asg);
    int* cnt_s = reinterpret_cast<int*>(km_smem + l.cnt);
    int* mv_s = reinterpret_cast<int*>(km_smem + l.mv);
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, li = lane & 31, lk = lane >> 5;
    const int64_t j0 = (int64_t)blockIdx.x * a.span, jend = min(a.N, j0 + a.span);

    for (int i = t; i < KP * LDH; i += 256) {
        const int c = i / LDH, k = i - c * LDH;
        cs[i] = (c < K && k < H) ? a.C[(size_t)c * H + k] : 0.f;
    }
    if (SUMS)
        for (int i = t; i < K * H; i += 256) acc_s[i] = 0.f;
    if (t < KP) cnt_s[t] = 0;
    if (t == 0) *mv_s = 0;
    __syncthreads();
    if (t < KP) cn_s[t] = km_norm(cs + t * LDH, Hp);
    // (the first barrier of the tile loop publishes the norms)

    const int nrt = TR >= 32 ? TR / 32 : 1, ntile = nrt * (KP / 32);     // 32 x 32 products of a tile: at most 4, one per wave
    const int rt = wave % nrt, ct = wave / nrt;
    const int rl = rt * 32 + li;                                          // this lane's row of the tile in the product
    const int gsum = t / H, hsum = t - gsum * H;                          // sum phase: cluster group and column
    double inert = 0.0;                                                   // (t == 255)

    for (int64_t t0 = j0; t0 < jend; t0 += TR) {
        if (s.vec) {
            const int qpr = Hp >> 2;                                      // 16-byte pieces of a padded row
#pragma unroll 4
            for (int e = t; e < TR * qpr; e += 256) {
                const int r = e / qpr, k = (e - r * qpr) << 2;
                const int64_t row = t0 + r;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (row < jend && k < H) v = *reinterpret_cast<const float4*>(a.X + (size_t)row * H + k);
                *reinterpret_cast<float4*>(xt + r * LDH + k) = v;
            }
        } else {
#pragma unroll 4
            for (int e = t; e < TR * Hp; e += 256) {
                const int r = e / Hp, k = e - r * Hp;
                const int64_t row = t0 + r;
                xt[r * LDH + k] = (row < jend && k < H) ? a.X[(size_t)row * H + k] : 0.f;
            }
        }
        if (t < TR) key_s[t] = kKnnNone;
        __syncthreads();

        gc_f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        if (255 - t < TR) xn_s[255 - t] = km_norm(xt + (255 - t) * LDH, Hp);          // the last wave: the rows' norms
        if (wave < ntile)                                                             // (uniform over the wave)
            mma_rowk(cs + (ct * 32 + li) * LDH, xt + (rl < TR ? rl : 0) * LDH, Hp, lk, acc);
        __syncthreads();

        if (wave < ntile) {
            unsigned long long best = kKnnNone;
            if (rl < TR && t0 + rl < jend) {
                const float xnj = xn_s[rl];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int c = ct * 32 + mma_row(r, lk);
                    if (c >= K) continue;
                    const unsigned long long key = kmeans_key(knn_dist<float>(0, xnj, cn_s[c], acc[r]), (uint32_t)c);
                    best = key < best ? key : best;
                }
            }
            const unsigned long long other = __shfl_xor(best, 32);                    // the other 16 centroids of the row
            best = other < best ? other : best;
            if (lk == 0 && rl < TR) atomicMin(&key_s[rl], best);                      // integer: any order, one result
        }
        __syncthreads();

        if (t < TR) {
            const int64_t row = t0 + t;
            int c = -1;
            float dsum = 0.f;                                             // what the row adds to the inertia
            if (row < jend) {
                const uint64_t key = key_s[t];
                c = kmeans_cluster(key);
                const float d = knn_key_dist(key);
                if (SUMS) {
                    const int old = a.it > 0 ? a.assign[row] : -1;
                    if (c != old) atomicAdd(mv_s, 1);
                    if (c >= 0) atomicAdd(&cnt_s[c], 1);
                } else {
                    a.dist[row] = d;
                }
                a.assign[row] = c;
                dsum = c >= 0 ? d : 0.f;
            }
            asg_s[t] = c;
            dst_s[t] = dsum;
        }
        __syncthreads();

        if (SUMS) {
            if (gsum < s.G) {
                // ascending rows: the chain of the rule, KM_U rows per LDS round trip.  The accumulators of KM_U rows are read
                // together; a row whose cluster an earlier row of the group also has takes that row's new value instead of
                // the one read (the latest such row: w ascends), so every (c, h) chain is the sequential one, add for add.
                for (int r0 = 0; r0 < TR; r0 += KM_U) {
                    int c[KM_U];
                    float x[KM_U], av[KM_U], nv[KM_U];
#pragma unroll
                    for (int u = 0; u < KM_U; ++u) c[u] = asg_s[r0 + u];
#pragma unroll
                    for (int u = 0; u < KM_U; ++u) {
                        const bool mine = c[u] >= 0 && (c[u] & (s.G - 1)) == gsum;
                        c[u] = mine ? c[u] : -1 - u;                      // (distinct, equal to no cluster)
                        x[u] = xt[(r0 + u) * LDH + hsum];
                        av[u] = mine ? acc_s[c[u] * H + hsum] : 0.f;
                    }
#pragma unroll
                    for (int u = 0; u < KM_U; ++u) {
                        float v = av[u];
#pragma unroll
                        for (int w = 0; w < u; ++w) v = c[u] == c[w] ? nv[w] : v;
                        nv[u] = kmeans_add(v, x[u]);
                    }
#pragma unroll
                    for (int u = 0; u < KM_U; ++u)
                        if (c[u] >= 0) acc_s[c[u] * H + hsum] = nv[u];
                }
            }
            if (t == 255) {
#pragma unroll 8
                for (int r = 0; r < TR; ++r) inert += (double)dst_s[r];   // (+0 for a row without a cluster: the chain's bits stay)
            }
        }
        __syncthreads();
    }

    if (SUMS) {
        const size_t sb = blockIdx.x;
        for (int i = t; i < K * H; i += 256) a.psum[sb * K * H + i] = acc_s[i];
        if (t < K) a.pcnt[sb * K + t] = cnt_s[t];
        if (t == 255) a.pin[sb] = inert;
        if (t == 0) a.pmv[sb] = *mv_s;
    }
}

// grid ceil(K H / 256), 256 threads
__global__ void __launch_bounds__(256) k_km_update(KmUpdArgs a) {
    if (a.it > 0 && __atomic_load_n(a.stop, __ATOMIC_RELAXED) <= a.it) return;
    const int i = blockIdx.x * 256 + threadIdx.x, KH = a.K * a.H;
    if (i < KH) {
        const int c = i / a.H;
        float sum = a.psum[i];
        int64_t n = a.pcnt[c];
#pragma unroll 16
        for (int64_t s = 1; s < a.spans; ++s) {
            sum = kmeans_add(sum, a.psum[(size_t)s * KH + i]);
            n += a.pcnt[(size_t)s * a.K + c];
        }
        a.Cout[i] = kmeans_mean(sum, n, a.Cold[i]);
        if (i == c * a.H) a.counts[c] = n;
    }
    if (i == 0) {
        double in = a.pin[0];
        int64_t mv = a.pmv[0];
        for (int64_t s = 1; s < a.spans; ++s) {
            in += a.pin[s];
            mv += a.pmv[s];
        }
        a.inertia[a.it] = in;
        a.moved[a.it] = mv;
        *a.iters_run = a.it + 1;
        __atomic_store_n(a.stop, mv == 0 ? a.it + 1 : INT_MAX, __ATOMIC_RELAXED);
    }
}

KmShape km_shape(const float* X, int64_t H, int64_t K, bool sums) {
    KmShape s;
    s.H = (int)H;
    s.K = (int)K;
    s.KP = K <= 32 ? 32 : 64;
    s.Hp = (int)((H + 31) / 32 * 32);
    s.LDH = s.Hp + 4;
    s.vec = (H % 4 == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0) ? 1 : 0;
    s.G = 1;
    while (2 * s.G * s.H <= 256) s.G *= 2;
    s.TR = 64;
    while (s.TR > 16 && km_lds(s.KP, s.LDH, s.TR, s.K, s.H, sums).end > KM_LDS_MAX) s.TR /= 2;
    s.lds = km_lds(s.KP, s.LDH, s.TR, s.K, s.H, sums).end;
    return s;
}

struct KmWs { int64_t psum, pin, pcnt, pmv, stop, end; };
KmWs km_ws(int64_t spans, int64_t K, int64_t H) {
    KmWs w;
    w.psum = 0;
    w.pin = (spans * K * H * 4 + 15) & ~15ll;
    w.pcnt = w.pin + spans * 8;
    w.pmv = w.pcnt + spans * K * 4;
    w.stop = w.pmv + spans * 4;
    w.end = w.stop + 4;
    return w;
}

template <bool SUMS>
int km_allow_lds(int lds) {                      // a workgroup above 64 KB of dynamic LDS is asked for once per kernel
    static bool done = false;
    if (lds <= 64 * 1024 || done) return 0;
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&k_km_step<SUMS>), hipFuncAttributeMaxDynamicSharedMemorySize, KM_LDS_MAX) != hipSuccess) {
        (void)hipGetLastError();
        return 1;
    }
    done = true;
    return 0;
}

}  // namespace
}  // namespace cal

using namespace cal;

CAL_EXPORT int64_t cal_kmeans_ws(int64_t N, int64_t K, int64_t H, int64_t span_rows) {
    if (N < 1 || K < 1 || K > kKmMaxK || H < 1 || H > kKmMaxH) return 0;
    return km_ws(kmeans_spans(N, kmeans_span(N, span_rows)), K, H).end + 256;
}

#define KM_LIMITS()                                                                 \
    CAL_REQUIRE(N >= 0 && N < (1ll << 31), "N must be in [0, 2^31)");                \
    CAL_REQUIRE(H >= 1 && H <= kKmMaxH, "H must be in [1, 256]");                    \
    CAL_REQUIRE(K >= 1 && K <= kKmMaxK, "K must be in [1, 64]")

CAL_EXPORT int cal_kmeans_assign(const float* X, int64_t N, int64_t H, const float* Cn, int64_t K, int32_t* assign, float* dist,
                                 void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    KM_LIMITS();
    if (N == 0) return 0;
    CAL_REQUIRE(X && Cn && assign && dist, "X / Cn / assign / dist is null");
    KmArgs a = {};
    a.X = X; a.C = Cn; a.N = N; a.span = kmeans_span(N, 0); a.s = km_shape(X, H, K, false); a.it = 0;
    a.assign = assign; a.dist = dist;
    CAL_REQUIRE(a.s.lds <= KM_LDS_MAX && km_allow_lds<false>(a.s.lds) == 0, "the step kernel's LDS does not fit");
    hipLaunchKernelGGL(k_km_step<false>, dim3((unsigned)kmeans_spans(N, a.span)), dim3(256), a.s.lds, stream, a);
    CAL_CHECK_LAUNCH("k_km_step<assign>");
    return 0;
}

CAL_EXPORT int cal_kmeans(const float* X, int64_t N, int64_t H, const float* C_in, int64_t K, int64_t iters, int64_t span_rows,
                          float* C_out, int32_t* assign, int64_t* counts, double* inertia, int64_t* moved, int32_t* iters_run,
                          void* ws, int64_t ws_bytes, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    KM_LIMITS();
    CAL_REQUIRE(iters >= 1 && iters < INT_MAX, "iters must be >= 1");
    CAL_REQUIRE(span_rows >= 0 && span_rows % kKmTile == 0, "span_rows must be 0 or a positive multiple of 128");
    if (N == 0) return 0;
    CAL_REQUIRE(X && C_in && C_out && assign && counts && inertia && moved && iters_run, "a tensor is null");
    CAL_REQUIRE(ws && ws_bytes >= cal_kmeans_ws(N, K, H, span_rows) && (reinterpret_cast<uintptr_t>(ws) & 15) == 0,
                "ws must be 16-byte aligned and hold cal_kmeans_ws(N, K, H, span_rows) bytes");
    const int64_t span = kmeans_span(N, span_rows), spans = kmeans_spans(N, span);
    const KmWs w = km_ws(spans, K, H);
    char* base = static_cast<char*>(ws);
    KmArgs a = {};
    a.X = X; a.N = N; a.span = span; a.s = km_shape(X, H, K, true); a.assign = assign;
    a.psum = reinterpret_cast<float*>(base + w.psum); a.pin = reinterpret_cast<double*>(base + w.pin);
    a.pcnt = reinterpret_cast<int32_t*>(base + w.pcnt); a.pmv = reinterpret_cast<int32_t*>(base + w.pmv);
    a.stop = reinterpret_cast<int32_t*>(base + w.stop);
    CAL_REQUIRE(a.s.lds <= KM_LDS_MAX && km_allow_lds<true>(a.s.lds) == 0, "the step kernel's LDS does not fit");
    KmUpdArgs u = {};
    u.Cout = C_out; u.psum = a.psum; u.pin = a.pin; u.pcnt = a.pcnt; u.pmv = a.pmv; u.spans = spans; u.K = (int)K; u.H = (int)H;
    u.counts = counts; u.inertia = inertia; u.moved = moved; u.iters_run = iters_run; u.stop = reinterpret_cast<int32_t*>(base + w.stop);
    for (int64_t it = 0; it < iters; ++it) {
        a.it = u.it = (int)it;
        a.C = u.Cold = it == 0 ? C_in : C_out;
        hipLaunchKernelGGL(k_km_step<true>, dim3((unsigned)spans), dim3(256), a.s.lds, stream, a);
        CAL_CHECK_LAUNCH("k_km_step");
        hipLaunchKernelGGL(k_km_update, dim3((unsigned)((K * H + 255) / 256)), dim3(256), 0, stream, u);
        CAL_CHECK_LAUNCH("k_km_update");
    }
    return 0;
}
