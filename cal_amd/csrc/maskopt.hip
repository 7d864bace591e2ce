// Learned mask explanations (cal_amd/maskopt.py): one optimiser step over the mask logits of a batch in ONE launch -- the
// sigmoid, the twin gather of the prediction gradient, the size and entropy regularisers with their gradients in closed form,
// Adam with bias correction, the scatter of sigma(theta_new) back to one or two mask entries and the per-graph sums of the
// loss history.
//
// One workgroup per graph strides over the graph's players.  Every output element has one writer, the two per-graph sums are
// taken in double in a fixed order (lane partials, a butterfly per wave, the wave partials in wave order) and nothing is
// atomic, so two calls on equal inputs give equal bits.  Scalar loads and stores only: no operand needs an alignment beyond
// its element's.
#include <math.h>

#include "cal_hip.h"
#include "common.hpp"
#include "segment.hpp"

namespace cal {
namespace {

constexpr int kMaskNT = 256;

// (Logit, logit_terms -- what one player's logit gives: rules.hpp)

// step_size = lr / (1 - beta1^step), rsq2 = 1 / sqrt(1 - beta2^step): taken once on the host, in double
__global__ void __launch_bounds__(kMaskNT) k_mask_step(const int64_t* __restrict__ pptr, const int32_t* __restrict__ rep,
                                                       const int32_t* __restrict__ mate, const float* __restrict__ grad,
                                                       float* __restrict__ theta, float* __restrict__ exp_avg,
                                                       float* __restrict__ exp_avg_sq, float* __restrict__ mask,
                                                       double* __restrict__ terms, int64_t P, int64_t M, int update,
                                                       float step_size, float rsq2, float beta1, float beta2, float eps,
                                                       float l_size, float l_ent) {
    __shared__ double red[2 * (kMaskNT / 64)];
    const int64_t g = blockIdx.x;
    int64_t lo, n;
    seg_clamp(pptr, g, P, lo, n);
    const float ent_w = n > 0 ? l_ent / (float)n : 0.f;
    double s_size = 0.0, s_ent = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += kMaskNT) {
        const int64_t p = lo + i;
        const int64_t r = rep[p], t = mate[p];
        const bool r_ok = r >= 0 && r < M, t_ok = t >= 0 && t < M;
        float th = theta[p];
        Logit q = logit_terms(th);
        s_size += (double)q.m;
        s_ent += (double)q.ent;
        if (update) {
            // dL/dtheta = (dL_pred/dm of the player's elements + d size/dm + d entropy/dm) dm/dtheta
            const float gr = ((r_ok ? grad[r] : 0.f) + (t_ok ? grad[t] : 0.f) + (l_size - ent_w * th)) * q.dm;
            const float m1 = beta1 * exp_avg[p] + (1.f - beta1) * gr;
            const float m2 = beta2 * exp_avg_sq[p] + (1.f - beta2) * gr * gr;
            th -= step_size * (m1 / (sqrtf(m2) * rsq2 + eps));
            exp_avg[p] = m1;
            exp_avg_sq[p] = m2;
            theta[p] = th;
            q = logit_terms(th);
        }
        if (r_ok) mask[r] = q.m;
        if (t_ok) mask[t] = q.m;
    }
    if (terms == nullptr) return;                             // (uniform over the grid)
    s_size = group_sum_d<64>(s_size);
    s_ent = group_sum_d<64>(s_ent);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[2 * w] = s_size; red[2 * w + 1] = s_ent; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0, b = 0.0;
        for (int k = 0; k < kMaskNT / 64; ++k) { a += red[2 * k]; b += red[2 * k + 1]; }
        terms[2 * g] = a;
        terms[2 * g + 1] = b;
    }
}

}  // namespace
}  // namespace cal

using namespace cal;

// call site: cal_amd/maskopt.py MaskOptimizer.step (step >= 1) and its initial scatter / closing evaluation (step == 0)
CAL_EXPORT int cal_mask_step(const int64_t* pptr, const int32_t* rep, const int32_t* mate, const float* grad, float* theta,
                             float* exp_avg, float* exp_avg_sq, float* mask, double* terms, int64_t B, int64_t P, int64_t M,
                             int32_t step, float lr, float beta1, float beta2, float eps, float l_size, float l_ent,
                             void* stream) {
    CAL_REQUIRE(B >= 0 && P >= 0 && M >= 0 && step >= 0 && B < (1ll << 31) && M < (1ll << 31), "bad sizes");
    if (B == 0 || P == 0) return 0;
    CAL_REQUIRE(pptr && rep && mate && theta && (M == 0 || mask), "null operand");
    CAL_REQUIRE(step == 0 || (grad && exp_avg && exp_avg_sq), "a step >= 1 needs grad and both moments");
    CAL_REQUIRE(step == 0 || (beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f), "betas must be in [0, 1)");
    float step_size = 0.f, rsq2 = 1.f;
    if (step > 0) {
        step_size = (float)((double)lr / (1.0 - pow((double)beta1, (double)step)));
        rsq2 = (float)(1.0 / sqrt(1.0 - pow((double)beta2, (double)step)));
    }
    k_mask_step<<<dim3((unsigned)B), dim3(kMaskNT), 0, (hipStream_t)stream>>>(pptr, rep, mate, grad, theta, exp_avg, exp_avg_sq, mask,
                                                                             terms, P, M, step > 0, step_size, rsq2, beta1, beta2,
                                                                             eps, l_size, l_ent);
    CAL_CHECK_LAUNCH("k_mask_step");
    return 0;
}
