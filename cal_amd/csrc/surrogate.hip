// The fit of the surrogate attributions (cal_amd/surrogate.py): per graph one weighted least-squares problem of the replicas'
// values on the players' membership bits -- KernelSHAP's constrained system (mode 0) or LIME's local linear model with a free
// intercept (mode 1) -- solved in fp64 by a Cholesky factorisation.
//
// cal_surrogate_fit: ONE launch, one workgroup of 256 threads per graph, no workspace, no read-back, no floating-point atomic.
// Every floating-point operation is a function of the surrogate block of rules.hpp, applied in the order stated there, so the
// host twin (csrc_host/calhost.cpp) gives the same bits; nothing here writes an a * b + c expression.
//
// Device shape.  The membership bits of a tile of kSurTile samples are staged once: a wave takes a sample, its lanes the players
// p and p + 64, the two ballots are the sample's 128-bit row (the intercept's bit set with them), so `key` is read once per
// sample and player -- for a graph of at most kSurTile = 512 samples; a larger graph's bits do not fit beside the matrix, and its
// tiles are staged a second time for the R^2.  The Gram matrix is accumulated in
// REGISTERS over all tiles: wave 0, 1, 2 own the 64 x 64 blocks (0,0), (1,0), (1,1) of the lower triangle, a lane one column of
// its block with 64 accumulators; the row bits of a sample are wave-uniform (scalar tests), the column bit selects w_s or +0
// (an accumulator is never -0, so adding +0 is skipping).  Every entry is owned by one lane that walks the samples in ascending
// order.  Wave 3 meanwhile forms the right-hand side (a lane the rows lane and lane + 64) and the two weighted sums of the R^2.
// The matrix then lives in LDS as a packed lower triangle stored BY COLUMNS (column j: rows j .. d - 1, contiguous): 66 048
// bytes at d = 128.  In the factorisation thread i owns row i: at column j it walks k < j with L_ik from column k -- consecutive
// threads read consecutive doubles, conflict-free under the (a / 4) % 64 banking of ds_read_b64 -- and L_jk, one address for the
// whole wave (a broadcast); every thread also carries the pivot chain (it reads L_jk anyway), so the pivot test is uniform and a
// column costs ONE barrier.  The diagonal of L is kept aside so that A_jj stays readable.  The two right-hand sides (b and the
// ones of the constraint) are solved side by side by the two halves of the workgroup, one barrier per unknown: as soon as y_k
// exists every row below takes its term, which gives each row its chain in ascending k (descending in the back substitution).
#include <atomic>

#include "segment.hpp"

namespace cal {
namespace {

constexpr int kSurNT = 256;
constexpr int kSurTile = 512;                                   // samples whose bits are staged at a time
constexpr int kSurD = kSurrogateMaxDim;
static_assert(kSurD == 128 && kSurrogateMaxPlayers == kSurD - 1, "two 64-bit words per sample, the intercept inside them");

// the dynamic LDS of the workgroup, in bytes from its start
constexpr int kSurTri = kSurD * (kSurD + 1) / 2;                // 8256 entries
constexpr int kSurOffMask = kSurTri * 8;                        // uint64 [kSurTile][2]
constexpr int kSurOffW = kSurOffMask + kSurTile * 16;           // double [kSurTile] weights
constexpr int kSurOffV = kSurOffW + kSurTile * 8;               // double [kSurTile] values
constexpr int kSurOffR = kSurOffV + kSurTile * 8;               // double [kSurTile] residuals
constexpr int kSurOffB = kSurOffR + kSurTile * 8;               // double [kSurD] the right-hand side b
constexpr int kSurOffDiag = kSurOffB + kSurD * 8;               // double [kSurD] the diagonal of L
constexpr int kSurOffY = kSurOffDiag + kSurD * 8;               // double [2][kSurD] forward solutions
constexpr int kSurOffX = kSurOffY + 2 * kSurD * 8;              // double [2][kSurD] x and u
constexpr int kSurOffPhi = kSurOffX + 2 * kSurD * 8;            // double [kSurD]
constexpr int kSurOffRed = kSurOffPhi + kSurD * 8;              // double [8]
constexpr int kSurOffBad = kSurOffRed + 64;                     // int [4]
constexpr int kSurLds = kSurOffBad + 16;
static_assert(kSurLds <= 160 * 1024, "the workgroup's LDS");

struct SurArgs {
    const int32_t* key;
    int64_t K, M;
    const int64_t *rptr, *rrow, *rth, *rinv;
    const double *val, *wt;
    int64_t R;
    const int64_t *pptr, *pel;
    int64_t P;
    const double *ve, *vf;
    int mode;
    double ridge;
    double *phi, *phi0, *r2;
    int32_t* status;
};

// entry (i, j), i >= j, of the packed lower triangle of dimension d stored by columns
__device__ __forceinline__ int sur_at(int d, int i, int j) { return j * d - (j * (j - 1)) / 2 + (i - j); }

// grid B, 256 threads
__global__ void __launch_bounds__(kSurNT) k_surrogate_fit(SurArgs a) {
    extern __shared__ __align__(16) char sur_smem[];
    double* A = reinterpret_cast<double*>(sur_smem);
    uint64_t* mask = reinterpret_cast<uint64_t*>(sur_smem + kSurOffMask);
    double* wl = reinterpret_cast<double*>(sur_smem + kSurOffW);
    double* vl = reinterpret_cast<double*>(sur_smem + kSurOffV);
    double* rl = reinterpret_cast<double*>(sur_smem + kSurOffR);
    double* bx = reinterpret_cast<double*>(sur_smem + kSurOffB);
    double* ldiag = reinterpret_cast<double*>(sur_smem + kSurOffDiag);
    double* ys = reinterpret_cast<double*>(sur_smem + kSurOffY);
    double* xs = reinterpret_cast<double*>(sur_smem + kSurOffX);
    double* phil = reinterpret_cast<double*>(sur_smem + kSurOffPhi);
    double* red = reinterpret_cast<double*>(sur_smem + kSurOffRed);
    int* sbad = reinterpret_cast<int*>(sur_smem + kSurOffBad);

    const int64_t g = blockIdx.x;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, mode = a.mode;
    const double nan = __builtin_nan("");
    int64_t plo, n64, rlo, S;
    seg_clamp(a.pptr, g, a.P, plo, n64);
    seg_clamp(a.rptr, g, a.R, rlo, S);
    if (n64 > kSurrogateMaxPlayers) {                             // (uniform over the workgroup, like every return below)
        for (int64_t p = tid; p < n64; p += kSurNT) a.phi[plo + p] = nan;
        if (tid == 0) {
            a.phi0[g] = a.r2[g] = nan;
            a.status[g] = sur_status(true, false, false);
        }
        return;
    }
    const int n = (int)n64, d = (int)sur_dim(n, mode);            // d <= 128
    const double ve = mode == 0 ? a.ve[g] : 0.0, vf = mode == 0 ? a.vf[g] : 0.0, delta = vf - ve;
    // this lane's two players
    const int64_t e0 = lane < n ? a.pel[plo + lane] : 0, e1 = 64 + lane < n ? a.pel[plo + 64 + lane] : 0;
    const bool ok0 = sur_player_ok(e0, a.M), ok1 = sur_player_ok(e1, a.M);
    if (tid == 0) sbad[0] = (mode == 0 && !(sur_finite(ve) && sur_finite(vf))) ? 1 : 0;
    __syncthreads();
    if ((lane < n && !ok0) || (64 + lane < n && !ok1)) sbad[0] = 1;

    // the bits, weights and values of the samples [t0, t0 + ts) of the graph
    auto stage = [&](int64_t t0, int ts) {
        for (int s = wave; s < ts; s += kSurNT / 64) {
            const int64_t i = rlo + t0 + s;
            const int64_t row = a.rrow[i], th = a.rth[i];
            const bool inv = a.rinv && a.rinv[i] != 0;
            const bool z0 = lane < n ? (ok0 && sur_member(a.key, a.K, a.M, row, e0, th, inv)) : (mode == 1 && lane == n);
            const bool z1 = 64 + lane < n ? (ok1 && sur_member(a.key, a.K, a.M, row, e1, th, inv)) : (mode == 1 && 64 + lane == n);
            const uint64_t m0 = __ballot(z0), m1 = __ballot(z1);
            if (lane == 0) {
                const double v = a.val[i], w = a.wt ? a.wt[i] : 1.0;
                mask[2 * s] = m0;
                mask[2 * s + 1] = m1;
                vl[s] = v;
                wl[s] = w;
                if (!sur_sample_ok(v, w)) sbad[0] = 1;
            }
        }
    };

    // ---- pass 1: the Gram matrix in registers, the right-hand side, the weighted sums
    const int rb = wave >= 1 ? 1 : 0, cb = wave == 2 ? 1 : 0;    // the block of waves 0, 1, 2
    const bool gram = wave < 3 && d > 0 && (wave == 0 || d > 64);
    double acc[64];
#pragma unroll
    for (int ii = 0; ii < 64; ++ii) acc[ii] = 0.0;
    double b0 = 0.0, b1 = 0.0, sw = 0.0, swv = 0.0;
    for (int64_t t0 = 0; t0 < S; t0 += kSurTile) {
        const int ts = (int)(S - t0 < kSurTile ? S - t0 : kSurTile);
        if (t0 > 0) __syncthreads();                              // the tile before has been read
        stage(t0, ts);
        __syncthreads();
        if (gram) {
            for (int s = 0; s < ts; ++s) {
                const uint64_t mr = mask[2 * s + rb], mc = mask[2 * s + cb];
                const double wj = ((mc >> lane) & 1) ? wl[s] : 0.0;
                const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)mr);
                const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(mr >> 32));
#pragma unroll
                for (int ii = 0; ii < 32; ++ii)
                    if ((lo >> ii) & 1) acc[ii] = sur_gram_add(acc[ii], wj);
#pragma unroll
                for (int ii = 0; ii < 32; ++ii)
                    if ((hi >> ii) & 1) acc[32 + ii] = sur_gram_add(acc[32 + ii], wj);
            }
        } else if (wave == 3) {
            for (int s = 0; s < ts; ++s) {
                const uint64_t m0 = mask[2 * s], m1 = mask[2 * s + 1];
                const double w = wl[s], v = vl[s], y = sur_y(v, ve, mode);
                if ((m0 >> lane) & 1) b0 = sur_rhs_add(b0, w, y);
                if ((m1 >> lane) & 1) b1 = sur_rhs_add(b1, w, y);
                sw = sur_gram_add(sw, w);
                swv = sur_rhs_add(swv, w, v);
            }
        }
    }
    if (gram) {
        const int j = cb * 64 + lane;
#pragma unroll
        for (int ii = 0; ii < 64; ++ii) {
            const int i = rb * 64 + ii;
            if (i < d && j <= i) A[sur_at(d, i, j)] = i == j ? sur_ridge(acc[ii], a.ridge, i, n) : acc[ii];
        }
    }
    if (wave == 3) {
        if (lane < d) bx[lane] = b0;
        if (64 + lane < d) bx[64 + lane] = b1;
        if (lane == 0) {
            red[0] = sw;
            red[1] = swv;
        }
    }
    __syncthreads();
    if (sbad[0]) {
        if (tid < n) a.phi[plo + tid] = nan;
        if (tid == 0) {
            a.phi0[g] = a.r2[g] = nan;
            a.status[g] = sur_status(false, true, false);
        }
        return;
    }

    // ---- the solve
    double phi0 = ve;
    bool deficient = false;
    if (sur_one_player(n, mode)) {
        if (tid == 0) phil[0] = delta;
    } else if (d > 0) {
        {                                                         // Cholesky, left-looking: thread i owns row i
            const int i = tid;
            for (int j = 0; j < d; ++j) {
                const bool mine = i > j && i < d;
                const double ajj = A[sur_at(d, j, j)];
                double dj = ajj, lij = mine ? A[sur_at(d, i, j)] : 0.0;
                int off = 0;                                      // column k starts here
                for (int k = 0; k < j; ++k) {
                    const double ljk = A[off + j - k];
                    dj = sur_sub(dj, ljk, ljk);
                    if (mine) lij = sur_sub(lij, A[off + i - k], ljk);
                    off += d - k;
                }
                if (!sur_pivot_ok(dj, ajj)) {                     // (every thread holds the same dj)
                    deficient = true;
                    break;
                }
                const double ljj = sur_sqrt(dj);
                if (mine) A[sur_at(d, i, j)] = sur_div(lij, ljj);
                if (tid == 0) ldiag[j] = ljj;
                __syncthreads();
            }
        }
        if (!deficient) {                                         // b and the ones side by side
            const int r = tid >> 7, i = tid & 127;
            const bool in = i < d && (r == 0 || mode == 0);        // (mode 1 has no constraint: nobody reads u)
            double t = in ? (r == 0 ? bx[i] : 1.0) : 0.0;
            for (int k = 0; k < d; ++k) {
                if (in && i == k) ys[r * kSurD + k] = sur_div(t, ldiag[k]);
                __syncthreads();
                if (in && i > k) t = sur_sub(t, A[sur_at(d, i, k)], ys[r * kSurD + k]);
            }
            t = in ? ys[r * kSurD + i] : 0.0;
            for (int k = d - 1; k >= 0; --k) {
                if (in && i == k) xs[r * kSurD + k] = sur_div(t, ldiag[k]);
                __syncthreads();
                if (in && i < k) t = sur_sub(t, A[sur_at(d, k, i)], xs[r * kSurD + k]);
            }
            if (i == 0 && (r == 0 || mode == 0)) {                // sum(x) and sum(u), ascending
                double sum = 0.0;
                for (int q = 0; q < d; ++q) sum = sum + xs[r * kSurD + q];
                red[2 + r] = sum;
            }
            __syncthreads();
            if (mode == 0) {
                if (tid < n) phil[tid] = sur_correct(xs[tid], xs[kSurD + tid], red[2], red[3], delta);
            } else {
                if (tid < n) phil[tid] = xs[tid];
                phi0 = xs[n];
            }
        }
    }
    if (deficient && n > 0) {
        if (tid < n) a.phi[plo + tid] = nan;
        if (tid == 0) {
            a.phi0[g] = a.r2[g] = nan;
            a.status[g] = sur_status(false, false, true);
        }
        return;
    }
    if (deficient) phi0 = nan;                                    // (mode 1 without a player and without weight)
    __syncthreads();

    // ---- pass 2: the weighted R^2
    const double mean = sur_div(red[1], red[0]);
    double ssq = 0.0;                                             // SSR in thread 0, SST in thread 64
    for (int64_t t0 = 0; t0 < S; t0 += kSurTile) {
        const int ts = (int)(S - t0 < kSurTile ? S - t0 : kSurTile);
        if (S > kSurTile) {                                       // more than one tile: its bits again
            __syncthreads();
            stage(t0, ts);
            __syncthreads();
        }
        for (int s = tid; s < ts; s += kSurNT) {
            const uint64_t m0 = mask[2 * s], m1 = mask[2 * s + 1];
            double fit = phi0;
            for (int p = 0; p < n; ++p)
                if (((p < 64 ? m0 : m1) >> (p & 63)) & 1) fit = fit + phil[p];
            rl[s] = vl[s] - fit;
        }
        __syncthreads();
        if (tid == 0)
            for (int s = 0; s < ts; ++s) ssq = sur_sq_add(ssq, wl[s], rl[s]);
        if (tid == 64)
            for (int s = 0; s < ts; ++s) ssq = sur_sq_add(ssq, wl[s], vl[s] - mean);
    }
    if (tid == 64) red[4] = ssq;
    __syncthreads();
    if (tid < n) a.phi[plo + tid] = phil[tid];
    if (tid == 0) {
        a.phi0[g] = phi0;
        a.r2[g] = sur_r2(ssq, red[4]);
        a.status[g] = 0;
    }
}

// above 64 KB of dynamic LDS: asked for once per DEVICE (the attribute belongs to the device's copy of the kernel).  Two threads
// may both ask, which is harmless; the flag is only ever set.
int sur_allow_lds() {
    constexpr int kMaxDev = 64;
    static std::atomic<bool> done[kMaxDev];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) {
        (void)hipGetLastError();
        return 1;
    }
    const bool tracked = dev >= 0 && dev < kMaxDev;
    if (tracked && done[dev].load(std::memory_order_acquire)) return 0;
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&k_surrogate_fit), hipFuncAttributeMaxDynamicSharedMemorySize, kSurLds) != hipSuccess) {
        (void)hipGetLastError();
        return 1;
    }
    if (tracked) done[dev].store(true, std::memory_order_release);
    return 0;
}

}  // namespace
}  // namespace cal

using namespace cal;

CAL_EXPORT int cal_surrogate_fit(const int32_t* key, int64_t K, int64_t M, const int64_t* rep_ptr, const int64_t* rep_row,
                                 const int64_t* rep_thresh, const int64_t* rep_invert, const double* value, const double* weight,
                                 int64_t R, const int64_t* pl_ptr, const int64_t* pl_elem, int64_t P, int64_t B,
                                 const double* v_empty, const double* v_full, int mode, double ridge, double* phi, double* phi0,
                                 double* r2, int32_t* status, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CAL_REQUIRE(K >= 0 && M >= 0 && R >= 0 && P >= 0 && B >= 0 && B <= 0x7FFFFFFF, "sizes must be >= 0, B < 2^31");
    CAL_REQUIRE(mode == 0 || mode == 1, "mode must be 0 (shap) or 1 (lime)");
    CAL_REQUIRE(ridge >= 0.0 && sur_finite(ridge), "ridge must be finite and >= 0");
    if (B == 0) return 0;
    CAL_REQUIRE(rep_ptr && pl_ptr && phi0 && r2 && status, "rep_ptr / pl_ptr / phi0 / r2 / status is null");
    CAL_REQUIRE(R == 0 || (rep_row && rep_thresh && value), "rep_row / rep_thresh / value is null");
    CAL_REQUIRE(P == 0 || (pl_elem && phi), "pl_elem / phi is null");
    CAL_REQUIRE(mode == 1 || (v_empty && v_full), "mode 0 needs v_empty and v_full");
    CAL_REQUIRE(sur_allow_lds() == 0, "the kernel's LDS does not fit");
    const SurArgs a{key, key && M > 0 ? K : 0, M, rep_ptr, rep_row, rep_thresh, rep_invert, value, weight, R, pl_ptr, pl_elem, P,
                    v_empty, v_full, mode, ridge, phi, phi0, r2, status};
    hipLaunchKernelGGL(k_surrogate_fit, dim3((unsigned)B), dim3(kSurNT), kSurLds, stream, a);
    CAL_CHECK_LAUNCH("k_surrogate_fit");
    return 0;
}
