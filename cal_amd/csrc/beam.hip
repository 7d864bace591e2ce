// The beam step of the counterfactual search (cal_amd/counterfactual.py): out of a graph's candidates -- a live state with one
// more element toggled, each with its replica's p(y^) and whether its argmax left y^ -- pick the counterfactual, or else the
// `beam` best distinct children as the next states.
//
// cal_beam_step: ONE launch, one workgroup of 256 threads per graph, no read-back.  The rule is all integer and lives in
// rules.hpp (beam_parent, full_word, flip_word, flip_pair, beam_head, beam_before): p is read through score_key only, nothing
// here does floating-point arithmetic, so the host twin and a plain-int restatement agree bit for bit.
//
// Device shape: the heads of the order, the parent slot and the two toggled indices of up to kSegCap = 2048 candidates sit in
// LDS next to the graph's parent rows ((beam + 1) x W words: the live states and the full set).  A pick is four wg_max rounds
// (head, rep_row, rep_flip, index: the order's components, every thread offering the best of its own candidates), the picked
// child is formed in LDS and every thread drops those of its candidates whose child equals it, word by word.  At most `beam`
// picks, so at most 16 x (8 barriers + W words x 8 candidates per thread).
#include <limits.h>

#include "segment.hpp"

namespace cal {
namespace {

constexpr int kBeamNT = 256;
constexpr uint8_t kBeamDead = 0xFF;

struct BeamArgs {
    const uint32_t* bits;      // [B beam, W]
    int64_t B;
    int beam;
    int64_t W;
    const int64_t* nst;        // [B] live states
    const int64_t* cptr;       // [B + 1] candidates of every graph
    const int64_t* rrow;       // [R]
    const int64_t* rflip;      // [R]
    const float* p;            // [R]
    const uint8_t* flipped;    // [R]
    int64_t R;
    const int64_t* seg;        // [B + 1] the element segments (edge_ptr in mode 0, ptr in mode 1)
    int64_t M;
    const int32_t* twin;       // [M] or null (mode 0 only)
    int64_t max_cand;
    uint8_t* done;             // [B]
    uint32_t* bits_out;        // [B beam, W]
    float* p_out;              // [B beam]
    int64_t* nst_out;          // [B]
    uint32_t* cf_bits;         // [B, W]
    float* cf_p;               // [B]
    int64_t* cf_cand;          // [B]
    int32_t* status;           // [B]
};

// grid B, 256 threads
__global__ void __launch_bounds__(kBeamNT) k_beam_step(BeamArgs a) {
    __shared__ unsigned long long head[kSegCap];
    __shared__ short f0s[kSegCap], f1s[kSegCap];
    __shared__ uint8_t slot[kSegCap];
    __shared__ uint32_t par[(kBeamMax + 1) * kBeamWords];
    __shared__ uint32_t sel[kBeamWords];
    __shared__ long long red[kBeamNT / 64];
    const int64_t g = blockIdx.x;
    const int tid = threadIdx.x, W = (int)a.W, beam = a.beam;
    if (tid == 0) a.nst_out[g] = 0;
    int64_t clo, cn64;
    seg_clamp(a.cptr, g, a.R, clo, cn64);
    if (a.done[g] || cn64 == 0) return;                            // (uniform over the workgroup, like every return below)
    if (cn64 > a.max_cand) {
        if (tid == 0) a.status[g] = 2;
        return;
    }
    const int cn = (int)cn64;                                     // <= max_cand <= kSegCap
    int64_t lo, m;
    seg_clamp(a.seg, g, a.M, lo, m);
    int64_t nlive = a.nst[g];
    nlive = nlive < 0 ? 0 : (nlive > beam ? beam : nlive);
    for (int t = tid; t < (beam + 1) * W; t += kBeamNT) {
        const int s = t / W, w = t - s * W;
        par[t] = s < nlive ? a.bits[(g * beam + s) * W + w] : (s == beam ? full_word(m, W, w) : 0u);
    }
    for (int c = tid; c < cn; c += kBeamNT) {
        const int64_t i = clo + c;
        head[c] = beam_head(a.flipped[i], a.p[i]);
        slot[c] = (uint8_t)beam_parent(a, g, i);
        int64_t f0, f1;
        flip_pair(a.rflip[i], lo, m, a.twin, f0, f1);
        f0s[c] = (short)(f0 < 32 * W ? f0 : -1);                   // (an index >= 32 W toggles nothing)
        f1s[c] = (short)(f1 < 32 * W ? f1 : -1);
    }
    __syncthreads();
    if (tid == 0) a.status[g] = 0;
    int picked = 0;
    for (int it = 0; it < beam; ++it) {
        // the best of this thread's own candidates that are still there (ascending c: of equals the earliest stands)
        int best = -1;
        unsigned long long bh = 0;
        int64_t br = 0, bf = 0;
        for (int c = tid; c < cn; c += kBeamNT) {
            if (slot[c] == kBeamDead) continue;
            const unsigned long long h = head[c];
            const int64_t rr = a.rrow[clo + c], ff = a.rflip[clo + c];
            if (best < 0 || beam_before(h, rr, ff, c, bh, br, bf, best)) {
                best = c;
                bh = h;
                br = rr;
                bf = ff;
            }
        }
        // the order's components one by one over the workgroup; ~x turns the smallest signed x into the largest
        bool in = best >= 0;
        const long long m1 = wg_max<kBeamNT>(in ? (long long)(0x3FFFFFFFFull - bh) : -1ll, red);
        if (m1 < 0) break;                                        // nothing left
        in = in && (long long)(0x3FFFFFFFFull - bh) == m1;
        const long long m2 = wg_max<kBeamNT>(in ? ~(long long)br : LLONG_MIN, red);
        in = in && ~(long long)br == m2;
        const long long m3 = wg_max<kBeamNT>(in ? ~(long long)bf : LLONG_MIN, red);
        in = in && ~(long long)bf == m3;
        const long long m4 = wg_max<kBeamNT>(in ? ~(long long)best : LLONG_MIN, red);
        const int wi = (int)~m4;
        if (tid < W) sel[tid] = par[slot[wi] * W + tid] ^ flip_word(f0s[wi], f1s[wi], tid);
        __syncthreads();
        const int64_t ci = clo + wi;
        if (it == 0 && (head[wi] >> 32) == 0) {                    // its argmax left y^: the counterfactual
            if (tid < W) a.cf_bits[g * W + tid] = sel[tid];
            if (tid == 0) {
                a.done[g] = 1;
                a.cf_p[g] = a.p[ci];
                a.cf_cand[g] = ci;
            }
            return;
        }
        if (tid < W) a.bits_out[(g * beam + it) * W + tid] = sel[tid];
        if (tid == 0) a.p_out[g * beam + it] = a.p[ci];
        ++picked;
        for (int c = tid; c < cn; c += kBeamNT) {                 // equal children are one child
            const int s = slot[c];
            if (s == kBeamDead) continue;
            const int f0 = f0s[c], f1 = f1s[c];
            bool eq = true;
            for (int w = 0; w < W && eq; ++w) eq = (par[s * W + w] ^ flip_word(f0, f1, w)) == sel[w];
            if (eq) slot[c] = kBeamDead;
        }
        __syncthreads();
    }
    if (tid == 0) a.nst_out[g] = picked;
}

}  // namespace
}  // namespace cal

using namespace cal;

CAL_EXPORT int cal_beam_step(const uint32_t* bits, int64_t B, int beam, int64_t W, const int64_t* n_state,
                             const int64_t* cand_ptr, const int64_t* rep_row, const int64_t* rep_flip, const float* p,
                             const uint8_t* flipped, int64_t R, const int64_t* seg_ptr, int64_t M, const int32_t* twin,
                             int mode, int64_t max_cand, uint8_t* done, uint32_t* bits_out, float* p_state_out, int64_t* n_state_out,
                             uint32_t* cf_bits, float* cf_p, int64_t* cf_cand, int32_t* status, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    CAL_REQUIRE(B >= 0 && R >= 0 && M >= 0 && B <= 0x7FFFFFFF, "sizes must be >= 0, B < 2^31");
    CAL_REQUIRE(beam >= 1 && beam <= kBeamMax, "beam must be in [1, 16]");
    CAL_REQUIRE(W >= 0 && W <= kBeamWords, "W must be in [0, 64]");
    CAL_REQUIRE(mode == 0 || mode == 1, "mode must be 0 (edges) or 1 (nodes)");
    CAL_REQUIRE(max_cand >= 0 && max_cand <= kSegCap, "max_cand must be <= cal_explain_lds_cap()");
    if (B == 0) return 0;
    CAL_REQUIRE(n_state && cand_ptr && seg_ptr && done && n_state_out && status, "n_state / cand_ptr / seg_ptr / done / n_state_out / status are null");
    CAL_REQUIRE(W == 0 || (bits && bits_out && cf_bits), "bits / bits_out / cf_bits are null");
    CAL_REQUIRE(p_state_out && cf_p && cf_cand, "p_state_out / cf_p / cf_cand are null");
    CAL_REQUIRE(R == 0 || (rep_row && rep_flip && p && flipped), "rep_row / rep_flip / p / flipped are null");
    const BeamArgs a{bits, B, beam, W, n_state, cand_ptr, rep_row, rep_flip, p, flipped, R, seg_ptr, M, mode == 0 ? twin : nullptr, max_cand,
                     done,
                     bits_out, p_state_out, n_state_out, cf_bits, cf_p, cf_cand, status};
    hipLaunchKernelGGL(k_beam_step, dim3((unsigned)B), dim3(kBeamNT), 0, stream, a);
    CAL_CHECK_LAUNCH("k_beam_step");
    return 0;
}
