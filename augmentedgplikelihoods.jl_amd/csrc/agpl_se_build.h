// agpl_se_build.h -- the feature generator of a plan made from raw inputs (agpl_plan_create_se, agpl_plan_create_stationary), shared
// by the libraries that build a marginal image from raw inputs: libagpl_se.so (agpl_features.hip: the plan's own images,
// agpl_plan_predict), libagpl_kernels.so (agpl_kernels.hip: the plan's own images) and libagpl_chain.so (agpl_chain.hip: the chunk
// images of agpl_plan_predict_chain).  The covariance function (agpl_kernel_rules.h) is a template parameter of the kernel: one
// instantiation per kind, chosen once on the host.  Internal: every including source gets its own copy of the kernels (anonymous
// namespace).
#pragma once
#include "agpl_kernel_rules.h"
#include "agpl_plan_impl.h"

namespace {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int BS = 128;          // feature rows per block; points per tile (= the marginal image's tile)
constexpr int KT = 16;           // k-slice per stage
constexpr int KPITCH = KT + 1;
constexpr int kStageFloats = KT * BS + BS * KPITCH; // Lt [16][128] + Kt [128][17]
constexpr int EPITCH = 65;                          // epilogue tile [128 rows][64 points + 1]
static_assert(BS * EPITCH <= 2 * kStageFloats, "the epilogue tile reuses the two stage buffers");
constexpr uint32_t kImageMagic = 0x41474951u; // "AGIQ" (agpl_syrk.hip)

__device__ __forceinline__ f32x16 mfma(float a, float b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

// One workgroup (4 waves) per 128-point tile.  LDS: two stage buffers (reused by the epilogue) | xs [128][D] float64 | 2 x 128 floats.
// Ph / Pl: the marginal image (NULL: not written); acc: the accumulate image's blocks (NULL: not written), nps point slices of 16.
// words[2]: first point whose x is not finite; words[3]: first point whose residual is negative beyond round-off;
// maxbits: max |phi| as float bits (atomicMax per wave).  KIND: the covariance function (agpl_kernel_kind), kparam its parameter.
// DERIV (libagpl_grad.so, include/agpl_grad.h): the generated column is that of the normalised derivative feature of input
// dimension dd, K[b][n] = s2 (kappa'(r) / r) u_dd u'_dd / sqrt(c) with u the rule's term of r^2 (agpl::kernel_warp; (x_n - z_b) / ell
// for the unwarped kinds), u' = d u / d ((x_n - z_b) / ell) (agpl::kernel_dwarp; 1 for them) and inv_sqrt_c = 1 / sqrt(c),
// c = -lim kappa'(r) / r at r = 0 times u'(0)^2 (a modulated dimension, agpl::kernel_dim_modulated: u u' becomes u m - m' and c gains the
// factor's curvature, agpl::kernel_modulation_curvature, formed here; the other dimensions of such a kind carry the factor m; an additive
// kind, agpl::kernel_kind_additive: K[b][n] = (s2 / D) (d e_dd / d u_dd) / sqrt(c) with c = 1 / D, dimension dd's term alone; the second-order additive kind,
// agpl::kernel_kind_additive2: K[b][n] = s2 (d e_dd / d u_dd) c_dd / sqrt(c) with c_dd = w1 + w2 sum_{d != dd} e_d and c = (2 - w) / D; a product kind,
// agpl::kernel_kind_product: K[b][n] = s2 u_dd t(a_dd) (prod_{d != dd} p(a_d)) exp(-sum a) / sqrt(c) with c = -t(0); a squared exponential x Matern kind,
// agpl::kernel_kind_se_matern: K[b][n] = -u_dd k / sqrt(c), c = 1, in a leading dimension and s2 u t(a) exp(-(r_lead^2 / 2 + a)) / sqrt(c), c = -t(0), in the last; the all-orders additive kind,
// agpl::kernel_kind_anova: K[b][n] = s2 eta (-u_dd e_dd) (prod_{d != dd} g_d) / sqrt(c) with c = eta; the squared exponential x categorical kind,
// agpl::kernel_kind_categorical: K[b][n] = -u_dd k / sqrt(c), c = 1, in a leading dimension, and no column at all for a categorical one); everything after the generator is the same code (|psi| <= sigma as |phi|: the same scale, clamp and words).  Without DERIV
// dd and inv_sqrt_c are not read.
//
// The body, inlined into the two kernels below (which carry the __restrict__ qualifiers: restated here they would
// reach the compiler as scoped-alias metadata and reorder the existing kinds' instruction streams).  A kind whose distance is warped (agpl::kernel_warp: the periodic kinds) takes its
// parameter in float64 (`period`: a float32 period would lose the phase after a few thousand periods) and keeps the rule's
// per-dimension constants w_d = ell_d / period and 1 / ell_d in 32 more doubles of LDS; the other kinds read neither.
template <int KIND, bool DERIV>
__device__ __forceinline__ void se_build_body(int64_t N, int Mp, int Mc, int D, const double *x,
                                              const double *zs, const double *ell, float s2,
                                              float kparam, double period, int dd, float inv_sqrt_c, const float *Lt, float scale, h8 *Ph,
                                              h8 *Pl, h8 *acc_blocks, int64_t nps,
                                              float *resid, unsigned *maxbits,
                                              unsigned long long *words) {
    constexpr bool WARPED = agpl::kernel_kind_warps(KIND);
    constexpr bool LAST = KIND == AGPL_KERNEL_SE_PERIODIC; // only the last dimension is warped: peeled out of the pair loop (gen4)
    constexpr bool MOD = agpl::kernel_kind_modulated(KIND); // kappa times a factor of the last dimension's difference: peeled likewise
    constexpr bool ADD = agpl::kernel_kind_additive(KIND);  // a sum of per-dimension terms, no r^2: a form of gen4 of its own
    constexpr bool ADD2 = agpl::kernel_kind_additive2(KIND); // those terms and their pairwise products: a fourth form (period = the share w)
    constexpr bool PROD = agpl::kernel_kind_product(KIND);   // a product of per-dimension Matern factors: a fifth form (no parameter)
    constexpr bool SEM = agpl::kernel_kind_se_matern(KIND);  // squared exponential in the leading dimensions, Matern in the last: a sixth form
    constexpr bool ANOVA = agpl::kernel_kind_anova(KIND);    // a product of (constant + squared exponential) factors: a seventh form (kparam = eta)
    constexpr bool CAT = agpl::kernel_kind_categorical(KIND); // squared exponential in the leading dimensions, code comparisons in the last kparam = C: an eighth form
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *stage0 = smem;                                          // [2][kStageFloats]
    double *xs = reinterpret_cast<double *>(smem + 2 * kStageFloats); // [128][D]
    float *qred = reinterpret_cast<float *>(xs + BS * D);          // [2][128]
    double *wt = reinterpret_cast<double *>(qred + 2 * BS);        // WARPED: [2][16] = ell_d / period | 1 / ell_d (the warped d only); MOD: ell_d / period of the modulated d; CAT: h_d of the categorical d
    if constexpr (CAT) { // h_d = 1 / (2 ell_d^2), formed once per workgroup and never per pair (visible after the barrier below the xs fill)
        if ((int)threadIdx.x < D && agpl::kernel_dim_categorical(KIND, (int)threadIdx.x, D, kparam))
            wt[threadIdx.x] = agpl::kernel_categorical_half(ell[threadIdx.x]);
    }
    if constexpr (WARPED) {
        if ((int)threadIdx.x < D && agpl::kernel_dim_warped(KIND, (int)threadIdx.x, D)) {
            wt[threadIdx.x] = ell[threadIdx.x] / period;
            wt[16 + threadIdx.x] = 1.0 / ell[threadIdx.x];
        }
    }
    if constexpr (MOD) { // the factor's constant, in the slot the periodic kinds fill
        if ((int)threadIdx.x < D && agpl::kernel_dim_modulated(KIND, (int)threadIdx.x, D)) wt[threadIdx.x] = ell[threadIdx.x] / period;
    }

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int li = lane & 31, lk = lane >> 5;
    const int nb = Mp / BS;
    const int64_t tile = blockIdx.x;
    const int64_t n0 = tile * BS;

    for (int t = tid; t < BS * D; t += 256) {
        const int n = t / D, d = t - n * D;
        double v = 0.0;
        if (n0 + n < N) {
            const double xv = x[(n0 + n) * D + d];
            if (!(fabs(xv) <= 1.79e308)) atomicMin(&words[2], (unsigned long long)(n0 + n));
            v = xv / ell[d];
        }
        xs[t] = v;
    }
    __syncthreads();

    // staging coordinates: Lt q = tid + 256 j -> (k = q >> 5, a4 = q & 31);  K q -> (point q >> 2, b4 = q & 3)
    int poff[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int q = tid + 256 * j;
        poff[j] = (q >> 5) * Mp + ((q & 31) << 2);
    }
    const int kn0 = tid >> 2, kn1 = kn0 + 64, kb = (tid & 3) << 2;
    const int Mc16 = (Mc + KT - 1) / KT * KT;

    float ssq[2] = {0.f, 0.f}; // |phi_n|^2 shares of this lane's two columns
    unsigned mx = 0u;
    float4 pr0, pr1, kr0, kr1;

    // 1 / sqrt(c) of the derivative feature: the caller's, and in a modulated dimension that of c + curvature ell_dd^2 (agpl_kernel_rules.h)
    float isc = inv_sqrt_c;
    if constexpr (MOD && DERIV) {
        if (agpl::kernel_dim_modulated(KIND, dd, D))
            isc = (float)(1.0 / sqrt(1.0 / ((double)inv_sqrt_c * (double)inv_sqrt_c) +
                                     agpl::kernel_modulation_curvature(KIND, dd, D, period) * (ell[dd] * ell[dd])));
    }
    // an additive kind's variance / D, folded once (at D = 1 s2 itself: the squared exponential's expression to the bit)
    [[maybe_unused]] const float s2d = ADD ? (float)((double)s2 * agpl::kernel_term_weight(KIND, D)) : 0.f;
    // the second-order additive kind's variance w / D and variance (1 - w) / P, folded once per thread in float64 (at D = 1 s2 itself and
    // 0: the squared exponential's expression to the bit; at w = 1 the additive kind's s2d and 0)
    [[maybe_unused]] const float s2w1 = ADD2 ? (float)((double)s2 * agpl::kernel_sum_weight1(KIND, D, period)) : 0.f;
    [[maybe_unused]] const float s2w2 = ADD2 ? (float)((double)s2 * agpl::kernel_sum_weight2(KIND, D, period)) : 0.f;
    auto gen4 = [&](int n, int b) -> float4 { // K[b .. b + 3][n]
        float v[4];
        if constexpr (ANOVA) {
            // The seventh peeled form: k = s2 prod_d g_d, g_d = 1 - eta (1 - e_d) (agpl_kernel_rules.h: kernel_kind_anova; kparam = eta, rounded
            // to float32 once on the host).  The additive form's loop (d outermost, the quad's four inducing inputs inside: one LDS read of
            // x_d feeds four float64 differences, four float32 exponentials and four INDEPENDENT float32 running products
            // P_j <- P_j fmaf(-eta, 1 - e, 1)) in the fixed order d = 0 .. D - 1: the additive kind's D exponentials per pair plus one
            // subtraction, one FMA and one multiply each, no float64 arithmetic after the difference and no square root.  Every factor
            // lies in [1 - eta, 1]: the product cannot overflow and there is no cut.  A point's rows depend on its x alone.  Rows at or
            // past Mc as the additive form.
            // DERIV: d k / d u_dd = s2 eta (-u_dd e_dd) prod_{d != dd} g_d: the same single pass with d g / d u in place of g_dd (a uniform
            // select), the exclusive product for free: no prefix or suffix array, no division by g_dd (0 at eta = 1 far away).
            v[0] = v[1] = v[2] = v[3] = 0.f;
            if (b < Mc) {
                const double *xn = xs + n * D;
                const double *zb[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) zb[e] = zs + (int64_t)min(b + e, Mc - 1) * D;
                float P[4] = {1.f, 1.f, 1.f, 1.f};
                for (int d = 0; d < D; ++d) {
                    const double xd = xn[d];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const double us = xd - zb[e][d];
                        if (DERIV && d == dd) P[e] *= agpl::kernel_anova_dfactor<float>(kparam, us);
                        else P[e] *= agpl::kernel_anova_factor<float>(kparam, us);
                    }
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    v[e] = s2 * P[e];
                    if constexpr (DERIV) v[e] *= isc;
                    if (b + e >= Mc) v[e] = 0.f;
                }
            }
            return make_float4(v[0], v[1], v[2], v[3]);
        }
        if constexpr (CAT) {
            // The eighth peeled form: k = s2 exp(-(r_lead^2 / 2 + sum_{d >= D - C} [x_d != z_d] h_d)), h_d = 1 / (2 ell_d^2)
            // (agpl_kernel_rules.h: kernel_kind_categorical; kparam = C, uniform over the launch).  The sixth form's loop order (d outermost,
            // the quad's four inducing inputs inside): over the D - C leading dimensions one LDS read of x_d feeds four INDEPENDENT float64
            // chains r2 += us us; then each categorical dimension costs one LDS read of x_d, one of h_d (wt, formed once per workgroup) and
            // four compares, each selecting h_d or 0 into the element's float64 argument s = r2 / 2 + ...: no multiply, no subtraction
            // (x_d != z_d is us != 0 for the finite scaled values held here), no sinpi, no square root.  s is rounded ONCE to float32 and
            // there is ONE float32 exponential per element.  With every code equal, s = r2 / 2 and the value is the squared exponential's.
            // DERIV (leading dd only: a code has no derivative and agpl_plan_predict_grad builds no feature for it): -u_dd times the value,
            // as the unwarped kinds; a categorical dd would leave ud = 0 and give a zero column.  Rows at or past Mc as the sixth form.
            v[0] = v[1] = v[2] = v[3] = 0.f;
            if (b < Mc) {
                const int dl = D - (int)kparam; // the leading (continuous) dimensions
                const double *xn = xs + n * D;
                const double *zb[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) zb[e] = zs + (int64_t)min(b + e, Mc - 1) * D;
                double s[4] = {0.0, 0.0, 0.0, 0.0};
                [[maybe_unused]] double ud[4] = {0.0, 0.0, 0.0, 0.0};
                for (int d = 0; d < dl; ++d) {
                    const double xd = xn[d];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const double us = xd - zb[e][d];
                        s[e] += us * us;
                        if (DERIV && d == dd) ud[e] = us;
                    }
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) s[e] *= 0.5;
                for (int d = dl; d < D; ++d) {
                    const double xd = xn[d], hd = wt[d];
#pragma unroll
                    for (int e = 0; e < 4; ++e) s[e] += xd != zb[e][d] ? hd : 0.0;
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    v[e] = s2 * agpl::kernel_exp(-(float)s[e]);
                    if constexpr (DERIV) v[e] *= -(float)ud[e] * isc;
                    if (b + e >= Mc) v[e] = 0.f;
                }
            }
            return make_float4(v[0], v[1], v[2], v[3]);
        }
        if constexpr (SEM) {
            // The sixth peeled form: k = s2 p(a) exp(-(r_lead^2 / 2 + a)), a = c |u_{D-1}| (agpl_kernel_rules.h: kernel_kind_se_matern).  The
            // squared exponential's float64 chain r2 += us us over d < D - 1 with no flag and no branch per dimension, as the LAST and MOD
            // forms, then the last dimension peeled: a64 = c |us| in float64, s = r2 / 2 + a64 rounded ONCE to float32, a rounded once from
            // a64, and ONE float32 exponential per element.  No float64 square root (the isotropic Matern kinds take one per element) and no
            // float32 work per dimension (the product kinds take D Horner steps and a running product).
            // DERIV: leading dd: -u_dd times the value (ud, as the unwarped kinds); last dd: u t(a) in place of p(a), a uniform select; no
            // division.  Past the cut of agpl::kernel_product_value the value is 0, never inf 0: |u_dd| p(a) and |u t(a)| are at most e^s.
            // Loop order: the additive and product forms' (d outermost, the quad's four inducing inputs inside: one LDS read of x_d feeds
            // four INDEPENDENT float64 chains), not the r^2 forms' (element outermost).  In the gfx950 listing the r^2 order is four loops
            // one after the other, each 8 dependent v_fmac_f64 on ONE accumulator per trip with 4 LDS reads; this order is one loop of 16
            // v_fmac_f64 on four accumulators (dependent depth 4) with 2 LDS reads per trip, for 14 more VGPRs.  A row
            // at or past Mc reads row Mc - 1 (in bounds) and is zeroed; a quad wholly past Mc costs nothing.
            v[0] = v[1] = v[2] = v[3] = 0.f;
            if (b < Mc) {
                constexpr double cs = agpl::kernel_se_matern_scale(KIND);
                const int dl = D - 1;
                const double *xn = xs + n * D;
                const double *zb[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) zb[e] = zs + (int64_t)min(b + e, Mc - 1) * D;
                double r2[4] = {0.0, 0.0, 0.0, 0.0};
                [[maybe_unused]] double ud[4] = {0.0, 0.0, 0.0, 0.0};
                for (int d = 0; d < dl; ++d) {
                    const double xd = xn[d];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const double us = xd - zb[e][d];
                        r2[e] += us * us;
                        if (DERIV && d == dd) ud[e] = us;
                    }
                }
                const double xl = xn[dl];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const double us = xl - zb[e][dl];
                    const double a64 = cs * fabs(us);
                    const float s = (float)(0.5 * r2[e] + a64), a = (float)a64;
                    float P = agpl::kernel_se_matern_pterm<KIND, float>(a);
                    if constexpr (DERIV) P = dd == dl ? (float)us * agpl::kernel_se_matern_dpterm<KIND, float>(a) : -(float)ud[e] * P;
                    v[e] = s2 * agpl::kernel_product_value(s, P);
                    if constexpr (DERIV) v[e] *= isc;
                    if (b + e >= Mc) v[e] = 0.f;
                }
            }
            return make_float4(v[0], v[1], v[2], v[3]);
        }
        if constexpr (PROD) {
            // The fifth peeled form: k = s2 (prod_d p(a_d)) exp(-sum_d a_d), a_d = c |u_d| (agpl_kernel_rules.h: kernel_kind_product).  The
            // additive form's loop (d outermost, the quad's four inducing inputs inside: one LDS read of x_d feeds four independent float64
            // differences) with two float32 accumulators per element, s <- s + a_d and P <- P p(a_d) (Horner, fmaf), in the fixed order
            // d = 0 .. D - 1.  a_d is rounded once from the float64 product c |u_d|.  Then ONE float32 exponential per element: no float64
            // square root (the isotropic Matern kinds take one per element), no exponential per dimension (the additive kinds take D).  A
            // point's rows depend on its x alone.  Rows at or past Mc as the additive form.
            // DERIV: d k / d u_dd = s2 u_dd t(a_dd) (prod_{d != dd} p(a_d)) exp(-sum a): the same single pass with u_dd t(a_dd) in place
            // of p(a_dd) (a uniform select), the exclusive product for free: no prefix or suffix array, no division.
            v[0] = v[1] = v[2] = v[3] = 0.f;
            if (b < Mc) {
                constexpr double cs = agpl::kernel_product_scale(KIND);
                const double *xn = xs + n * D;
                const double *zb[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) zb[e] = zs + (int64_t)min(b + e, Mc - 1) * D;
                float s[4] = {0.f, 0.f, 0.f, 0.f}, P[4] = {1.f, 1.f, 1.f, 1.f};
                for (int d = 0; d < D; ++d) {
                    const double xd = xn[d];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const double us = xd - zb[e][d];
                        const float a = (float)(cs * fabs(us));
                        s[e] += a;
                        if (DERIV && d == dd) P[e] *= (float)us * agpl::kernel_dpterm<KIND, float>(a);
                        else P[e] *= agpl::kernel_pterm<KIND, float>(a);
                    }
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    v[e] = s2 * agpl::kernel_product_value(s[e], P[e]);
                    if constexpr (DERIV) v[e] *= isc;
                    if (b + e >= Mc) v[e] = 0.f;
                }
            }
            return make_float4(v[0], v[1], v[2], v[3]);
        }
        if constexpr (ADD2) {
            // The fourth peeled form: k = s2 (w1 S1 + w2 E2), S1 = sum_d e_d, E2 = sum_{d < d'} e_d e_d'.  The additive form's loop (d outermost,
            // the quad's four inducing inputs inside: one LDS read of x_d feeds four independent float64 differences and four float32
            // exponentials) with TWO float32 accumulators per element, E2 by the elementary-symmetric recurrence E2 <- fma(e_d, S1, E2),
            // S1 <- S1 + e_d (agpl::kernel_sum_step) in the fixed order d = 0 .. D - 1: the D exponentials the first order forms are all the
            // second order needs, one more FMA per term, and 8 accumulators where the additive form has 4.  Every term is >= 0 (no
            // cancellation, unlike (S1^2 - sum e_d^2) / 2) and a point's rows depend on its x alone.  Rows at or past Mc as the additive form.
            // DERIV: d k / d u_dd = s2 (-u_dd e_dd) (w1 + w2 sum_{d != dd} e_d): the other dimensions' terms weight dd's, summed without dd
            // (no S1 - e_dd to cancel), so a derivative column costs D exponentials per element where the additive kind's costs one.
            v[0] = v[1] = v[2] = v[3] = 0.f;
            if (b < Mc) {
                const double *xn = xs + n * D;
                const double *zb[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) zb[e] = zs + (int64_t)min(b + e, Mc - 1) * D;
                float S1[4] = {0.f, 0.f, 0.f, 0.f};
                if constexpr (DERIV) {
                    for (int d = 0; d < D; ++d) {
                        if (d == dd) continue; // (uniform)
                        const double xd = xn[d];
#pragma unroll
                        for (int e = 0; e < 4; ++e) S1[e] += agpl::kernel_term<float>(xd - zb[e][d]);
                    }
                    const double xd = xn[dd];
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = agpl::kernel_dterm<float>(xd - zb[e][dd]) * fmaf(s2w2, S1[e], s2w1) * isc;
                } else {
                    float E2[4] = {0.f, 0.f, 0.f, 0.f};
                    for (int d = 0; d < D; ++d) {
                        const double xd = xn[d];
#pragma unroll
                        for (int e = 0; e < 4; ++e) agpl::kernel_sum_step(agpl::kernel_term<float>(xd - zb[e][d]), S1[e], E2[e]);
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = fmaf(s2w2, E2[e], s2w1 * S1[e]); // (w2 = 0: s2w1 S1 exactly, the additive kind's value)
                }
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (b + e >= Mc) v[e] = 0.f;
            }
            return make_float4(v[0], v[1], v[2], v[3]);
        }
        if constexpr (ADD) {
            // The third peeled form: k = (s2 / D) sum_d e_d has no r^2 to accumulate, so the loop is turned inside out.  d runs outermost
            // and the four inducing inputs inside: one LDS read of x_d feeds four float64 differences and four float32 exponentials that
            // do not depend on each other (the r^2 forms run one dependent float64 chain per element), and each element's sum is taken in
            // float32 in the fixed order d = 0 .. D - 1, so a point's rows depend on its x alone.  A row at or past Mc reads row Mc - 1
            // (in bounds) and is zeroed; a quad wholly past Mc costs nothing.  DERIV: only dimension dd's term is left in the column.
            v[0] = v[1] = v[2] = v[3] = 0.f;
            if (b < Mc) {
                const double *xn = xs + n * D;
                const double *zb[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) zb[e] = zs + (int64_t)min(b + e, Mc - 1) * D;
                if constexpr (DERIV) {
                    const double xd = xn[dd];
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = s2d * agpl::kernel_dterm<float>(xd - zb[e][dd]) * isc;
                } else {
                    float sum[4] = {0.f, 0.f, 0.f, 0.f};
                    for (int d = 0; d < D; ++d) {
                        const double xd = xn[d];
#pragma unroll
                        for (int e = 0; e < 4; ++e) sum[e] += agpl::kernel_term<float>(xd - zb[e][d]);
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = s2d * sum[e];
                }
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (b + e >= Mc) v[e] = 0.f;
            }
            return make_float4(v[0], v[1], v[2], v[3]);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float k = 0.f;
            if (b + e < Mc) {
                double r2 = 0.0, ud = 0.0;
                [[maybe_unused]] double mod = 1.0;
                if constexpr (LAST) { // the squared exponential's sum over d < D - 1 (no flag, no branch per dimension), then one warped term
                    const int dl = D - 1;
                    for (int d = 0; d < dl; ++d) {
                        const double us = xs[n * D + d] - zs[(int64_t)(b + e) * D + d];
                        r2 += us * us;
                        if (DERIV && d == dd) ud = us;
                    }
                    const double us = xs[n * D + dl] - zs[(int64_t)(b + e) * D + dl];
                    const double u = agpl::kernel_warp<KIND>(us, wt[dl], wt[16 + dl]);
                    r2 += u * u;
                    if (DERIV && dd == dl) ud = u * agpl::kernel_dwarp<KIND>(us, wt[dl], wt[16 + dl]);
                } else if constexpr (MOD) { // the squared exponential's sum over every d, the last peeled: its difference also feeds the factor
                    const int dl = D - 1;
                    for (int d = 0; d < dl; ++d) {
                        const double us = xs[n * D + d] - zs[(int64_t)(b + e) * D + d];
                        r2 += us * us;
                        if (DERIV && d == dd) ud = us;
                    }
                    const double us = xs[n * D + dl] - zs[(int64_t)(b + e) * D + dl];
                    r2 += us * us;
                    mod = agpl::kernel_modulation(us, wt[dl]);
                    // d (kappa m) / d us_dd over kappa'(r) / r = -kappa: u_dd m in a leading dimension, u m - m' in the last (product rule)
                    if constexpr (DERIV) ud = dd == dl ? us * mod - agpl::kernel_dmodulation(us, wt[dl]) : ud * mod;
                } else {
                    for (int d = 0; d < D; ++d) {
                        const double us = xs[n * D + d] - zs[(int64_t)(b + e) * D + d];
                        const double u = agpl::kernel_warp<KIND>(us, WARPED ? wt[d] : 0.0, WARPED ? wt[16 + d] : 0.0);
                        r2 += u * u;
                        if (DERIV && d == dd) ud = u * agpl::kernel_dwarp<KIND>(us, WARPED ? wt[d] : 0.0, WARPED ? wt[16 + d] : 0.0);
                    }
                }
                if constexpr (DERIV) {
                    k = s2 * agpl::kernel_drule<KIND, float>(r2, kparam) * (float)ud * isc;
                } else {
                    k = s2 * agpl::kernel_rule<KIND, float>(r2, kparam);
                    if constexpr (MOD) k *= (float)mod;
                }
            }
            v[e] = k;
        }
        return make_float4(v[0], v[1], v[2], v[3]);
    };
#define AGPL_SE_LOAD(rb_, b0_)                                                          \
    do {                                                                                \
        const float *psrc_ = Lt + (int64_t)(b0_) * Mp + (rb_) * BS;                     \
        pr0 = *reinterpret_cast<const float4 *>(psrc_ + poff[0]);                       \
        pr1 = *reinterpret_cast<const float4 *>(psrc_ + poff[1]);                       \
        kr0 = gen4(kn0, (b0_) + kb);                                                    \
        kr1 = gen4(kn1, (b0_) + kb);                                                    \
    } while (0)
#define AGPL_SE_STORE(buf_)                                                             \
    do {                                                                                \
        float *Pt_ = stage0 + (buf_) * kStageFloats;                                    \
        float *Kt_ = Pt_ + KT * BS;                                                     \
        *reinterpret_cast<float4 *>(Pt_ + (tid >> 5) * BS + ((tid & 31) << 2)) = pr0;   \
        *reinterpret_cast<float4 *>(Pt_ + ((tid >> 5) + 8) * BS + ((tid & 31) << 2)) = pr1; \
        float *kd_ = Kt_ + kn0 * KPITCH + kb;                                           \
        kd_[0] = kr0.x; kd_[1] = kr0.y; kd_[2] = kr0.z; kd_[3] = kr0.w;                 \
        kd_ += 64 * KPITCH;                                                             \
        kd_[0] = kr1.x; kd_[1] = kr1.y; kd_[2] = kr1.z; kd_[3] = kr1.w;                 \
    } while (0)

    for (int rb = 0; rb < nb; ++rb) {
        f32x16 acc[2][2];
#pragma unroll
        for (int ii = 0; ii < 2; ++ii)
#pragma unroll
            for (int jj = 0; jj < 2; ++jj)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[ii][jj][r] = 0.f;

        // L^-1 is lower triangular: rows of block rb need b < 128 (rb + 1); K is zero for b >= Mc; rows >= Mc are zero
        const int bend = rb * BS >= Mc ? 0 : min((rb + 1) * BS, Mc16);
        const int nstage = bend / KT;
        if (nstage > 0) {
            AGPL_SE_LOAD(rb, 0);
            AGPL_SE_STORE(0);
            __syncthreads();
            for (int s = 0; s < nstage; ++s) {
                const int buf = s & 1;
                if (s + 1 < nstage) AGPL_SE_LOAD(rb, (s + 1) * KT);
                const float *Pt = stage0 + buf * kStageFloats;
                const float *Kt = Pt + KT * BS;
                const float *pa = Pt + lk * BS + wr * 64 + li;
                const float *pb = Kt + (wc * 64 + li) * KPITCH + lk;
#pragma unroll
                for (int k0 = 0; k0 < KT; k0 += 2) {
                    const float a0 = pa[k0 * BS], a1 = pa[k0 * BS + 32];
                    const float b0 = pb[k0], b1 = pb[k0 + 32 * KPITCH];
                    acc[0][0] = mfma(a0, b0, acc[0][0]);
                    acc[0][1] = mfma(a0, b1, acc[0][1]);
                    acc[1][0] = mfma(a1, b0, acc[1][0]);
                    acc[1][1] = mfma(a1, b1, acc[1][1]);
                }
                if (s + 1 < nstage) AGPL_SE_STORE(buf ^ 1);
                __syncthreads();
            }
        }
        // this lane holds Phi[a][n] for a = rb 128 + wr 64 + ii 32 + 8 g4 + 4 lk + (r & 3), n = n0 + wc 64 + jj 32 + li
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            const bool live = n0 + wc * 64 + jj * 32 + li < N;
#pragma unroll
            for (int ii = 0; ii < 2; ++ii)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float v = acc[ii][jj][r];
                    ssq[jj] += v * v;
                    if (live) mx = max(mx, __float_as_uint(v) & 0x7FFFFFFFu);
                }
        }
        // images, 64 points at a time through LDS (E [row][point], pitch 65)
        float *E = stage0;
        const int64_t nbk = Mp / KT; // k-slices of the marginal image per tile
        for (int p = 0; p < 2; ++p) {
            if (wc == p) {
#pragma unroll
                for (int ii = 0; ii < 2; ++ii)
#pragma unroll
                    for (int jj = 0; jj < 2; ++jj)
#pragma unroll
                        for (int r = 0; r < 16; ++r)
                            E[(wr * 64 + ii * 32 + 8 * (r >> 2) + 4 * lk + (r & 3)) * EPITCH + jj * 32 + li] = acc[ii][jj][r];
            }
            __syncthreads();
            if (Ph) { // marginal image: block (tile, k-slice) = [plane][row = point][8 features]
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int g = tid + 256 * k, fg = g >> 6, pl = g & 63;
                    const bool live = n0 + p * 64 + pl < N;
                    h8 hi, lo;
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const float v = live ? E[(fg * 8 + j) * EPITCH + pl] * scale : 0.f;
                        const _Float16 h = (_Float16)v;
                        hi[j] = h;
                        lo[j] = (_Float16)(v - (float)h);
                    }
                    const int64_t o = (tile * nbk + rb * 8 + (fg >> 1)) * 256 + (fg & 1) * 128 + p * 64 + pl;
                    Ph[o] = hi;
                    Pl[o] = lo;
                }
            }
            if (acc_blocks) { // accumulate image: block (slice of 16 points, feature block, hi | lo) = [plane][row = feature][8 points]
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int g = tid + 256 * k, row = g & 127, pp = g >> 7; // pp = (slice in the half) * 2 + plane
                    const int pl0 = pp * 8;
                    const int64_t ps = (n0 + p * 64) / 16 + (pp >> 1);
                    if (ps < nps) {
                        h8 hi, lo;
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            const float v = n0 + p * 64 + pl0 + j < N ? E[row * EPITCH + pl0 + j] * scale : 0.f;
                            const _Float16 h = (_Float16)v;
                            hi[j] = h;
                            lo[j] = (_Float16)(v - (float)h);
                        }
                        const int64_t o = ((ps * nb + rb) * 2) * 256 + (pp & 1) * 128 + row;
                        acc_blocks[o] = hi;
                        acc_blocks[o + 256] = lo;
                    }
                }
            }
            __syncthreads();
        }
    }
#undef AGPL_SE_LOAD
#undef AGPL_SE_STORE

    // |phi_n|^2: lane halves (lk), then the two row waves (wr) in a fixed order
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) ssq[jj] += __shfl_xor(ssq[jj], 32);
    if (lk == 0) {
        qred[wr * BS + wc * 64 + li] = ssq[0];
        qred[wr * BS + wc * 64 + 32 + li] = ssq[1];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = max(mx, (unsigned)__shfl_xor((int)mx, o));
    if (lane == 0 && mx) atomicMax(maxbits, mx);
    __syncthreads();
    if (tid < BS && n0 + tid < N) {
        const float s = qred[tid] + qred[BS + tid];
        const float d = s2 - s;
        if (d < -1e-5f * (fabsf(d) + s)) atomicMin(&words[3], (unsigned long long)(n0 + tid));
        resid[n0 + tid] = d > 0.f ? d : (d == d ? 0.f : d);
    }
}

template <int KIND, bool DERIV = false>
__global__ __launch_bounds__(256, 2) void se_build_kernel(int64_t N, int Mp, int Mc, int D, const double *__restrict__ x,
                                                          const double *__restrict__ zs, const double *__restrict__ ell, float s2,
                                                          float kparam, int dd, float inv_sqrt_c, const float *__restrict__ Lt, float scale, h8 *__restrict__ Ph,
                                                          h8 *__restrict__ Pl, h8 *__restrict__ acc_blocks, int64_t nps,
                                                          float *__restrict__ resid, unsigned *__restrict__ maxbits,
                                                          unsigned long long *__restrict__ words) {
    se_build_body<KIND, DERIV>(N, Mp, Mc, D, x, zs, ell, s2, kparam, 0.0, dd, inv_sqrt_c, Lt, scale, Ph, Pl, acc_blocks, nps, resid, maxbits,
                               words);
}

// the periodic kind's generator: the same body, the period in float64 where the others carry a float32 parameter
template <bool DERIV = false>
__global__ __launch_bounds__(256, 2) void se_build_periodic_kernel(int64_t N, int Mp, int Mc, int D, const double *__restrict__ x,
                                                                   const double *__restrict__ zs, const double *__restrict__ ell,
                                                                   float s2, double period, int dd, float inv_sqrt_c,
                                                                   const float *__restrict__ Lt, float scale,
                                                                   h8 *__restrict__ Ph, h8 *__restrict__ Pl, h8 *__restrict__ acc_blocks,
                                                                   int64_t nps, float *__restrict__ resid, unsigned *__restrict__ maxbits,
                                                                   unsigned long long *__restrict__ words) {
    se_build_body<AGPL_KERNEL_PERIODIC, DERIV>(N, Mp, Mc, D, x, zs, ell, s2, 0.f, period, dd, inv_sqrt_c, Lt, scale, Ph, Pl, acc_blocks, nps,
                                               resid, maxbits, words);
}

// the squared exponential x periodic kind's generator (AGPL_KERNEL_SE_PERIODIC): the same body with the last dimension's term peeled
// out of the pair loop, the period in float64
template <bool DERIV = false>
__global__ __launch_bounds__(256, 2) void se_build_se_periodic_kernel(int64_t N, int Mp, int Mc, int D, const double *__restrict__ x,
                                                                      const double *__restrict__ zs, const double *__restrict__ ell,
                                                                      float s2, double period, int dd, float inv_sqrt_c,
                                                                      const float *__restrict__ Lt, float scale,
                                                                      h8 *__restrict__ Ph, h8 *__restrict__ Pl, h8 *__restrict__ acc_blocks,
                                                                      int64_t nps, float *__restrict__ resid, unsigned *__restrict__ maxbits,
                                                                      unsigned long long *__restrict__ words) {
    se_build_body<AGPL_KERNEL_SE_PERIODIC, DERIV>(N, Mp, Mc, D, x, zs, ell, s2, 0.f, period, dd, inv_sqrt_c, Lt, scale, Ph, Pl, acc_blocks,
                                                  nps, resid, maxbits, words);
}

// the squared exponential x cosine kind's generator (AGPL_KERNEL_SE_COSINE): the squared exponential's body over all D dimensions, the
// last peeled, times the factor agpl::kernel_modulation of the last dimension's difference: one float64 cospi per pair, the period in
// float64
template <bool DERIV = false>
__global__ __launch_bounds__(256, 2) void se_build_se_cosine_kernel(int64_t N, int Mp, int Mc, int D, const double *__restrict__ x,
                                                                    const double *__restrict__ zs, const double *__restrict__ ell,
                                                                    float s2, double period, int dd, float inv_sqrt_c,
                                                                    const float *__restrict__ Lt, float scale,
                                                                    h8 *__restrict__ Ph, h8 *__restrict__ Pl, h8 *__restrict__ acc_blocks,
                                                                    int64_t nps, float *__restrict__ resid, unsigned *__restrict__ maxbits,
                                                                    unsigned long long *__restrict__ words) {
    se_build_body<AGPL_KERNEL_SE_COSINE, DERIV>(N, Mp, Mc, D, x, zs, ell, s2, 0.f, period, dd, inv_sqrt_c, Lt, scale, Ph, Pl, acc_blocks,
                                                nps, resid, maxbits, words);
}

// the additive squared exponential kind's generator (AGPL_KERNEL_ADDITIVE_SE): the same body with gen4's additive form, D float32
// exponentials per pair summed in float32; no parameter
template <bool DERIV = false>
__global__ __launch_bounds__(256, 2) void se_build_additive_se_kernel(int64_t N, int Mp, int Mc, int D, const double *__restrict__ x,
                                                                      const double *__restrict__ zs, const double *__restrict__ ell,
                                                                      float s2, int dd, float inv_sqrt_c, const float *__restrict__ Lt,
                                                                      float scale, h8 *__restrict__ Ph, h8 *__restrict__ Pl,
                                                                      h8 *__restrict__ acc_blocks, int64_t nps, float *__restrict__ resid,
                                                                      unsigned *__restrict__ maxbits, unsigned long long *__restrict__ words) {
    se_build_body<AGPL_KERNEL_ADDITIVE_SE, DERIV>(N, Mp, Mc, D, x, zs, ell, s2, 0.f, 0.0, dd, inv_sqrt_c, Lt, scale, Ph, Pl, acc_blocks, nps,
                                                  resid, maxbits, words);
}

// the second-order additive squared exponential kind's generator (AGPL_KERNEL_ADDITIVE2_SE): the same body with gen4's fourth form, D
// float32 exponentials and D FMAs per pair into two float32 accumulators; the share w in float64 (the weights are folded from it once
// per thread).  Dynamic LDS is the squared exponential's: no period, no table.  gfx950 listing: 201 VGPRs (DERIV: 208; the
// additive kind's are 204 and 176), no scratch, no spill: two 256-thread workgroups per CU.
template <bool DERIV = false>
__global__ __launch_bounds__(256, 2) void se_build_additive2_se_kernel(int64_t N, int Mp, int Mc, int D, const double *__restrict__ x,
                                                                       const double *__restrict__ zs, const double *__restrict__ ell,
                                                                       float s2, double share, int dd, float inv_sqrt_c,
                                                                       const float *__restrict__ Lt, float scale, h8 *__restrict__ Ph,
                                                                       h8 *__restrict__ Pl, h8 *__restrict__ acc_blocks, int64_t nps,
                                                                       float *__restrict__ resid, unsigned *__restrict__ maxbits,
                                                                       unsigned long long *__restrict__ words) {
    se_build_body<AGPL_KERNEL_ADDITIVE2_SE, DERIV>(N, Mp, Mc, D, x, zs, ell, s2, 0.f, share, dd, inv_sqrt_c, Lt, scale, Ph, Pl, acc_blocks, nps,
                                                   resid, maxbits, words);
}

// the product Matern kinds' generator (AGPL_KERNEL_MATERN32_PRODUCT, AGPL_KERNEL_MATERN52_PRODUCT): the same body with gen4's fifth form, two
// float32 accumulators and one float32 exponential per pair; no parameter.  A kernel of its own name: tests/test_kernels_cpu.py holds that
// se_build_kernel is instantiated for kinds 0 .. 4 and no other.  Dynamic LDS is the squared exponential's.
template <int KIND, bool DERIV = false>
__global__ __launch_bounds__(256, 2) void se_build_product_kernel(int64_t N, int Mp, int Mc, int D, const double *__restrict__ x,
                                                                  const double *__restrict__ zs, const double *__restrict__ ell, float s2,
                                                                  int dd, float inv_sqrt_c, const float *__restrict__ Lt, float scale,
                                                                  h8 *__restrict__ Ph, h8 *__restrict__ Pl, h8 *__restrict__ acc_blocks,
                                                                  int64_t nps, float *__restrict__ resid, unsigned *__restrict__ maxbits,
                                                                  unsigned long long *__restrict__ words) {
    static_assert(agpl::kernel_kind_product(KIND), "a product kind");
    se_build_body<KIND, DERIV>(N, Mp, Mc, D, x, zs, ell, s2, 0.f, 0.0, dd, inv_sqrt_c, Lt, scale, Ph, Pl, acc_blocks, nps, resid, maxbits, words);
}

// the squared exponential x Matern kinds' generator (AGPL_KERNEL_SE_MATERN32, AGPL_KERNEL_SE_MATERN52): the same body with gen4's sixth
// form, four float64 chains over the leading dimensions and one float32 exponential per pair; no parameter.  A kernel of its own name, as
// se_build_product_kernel.  Dynamic LDS is the squared exponential's.
template <int KIND, bool DERIV = false>
__global__ __launch_bounds__(256, 2) void se_build_se_matern_kernel(int64_t N, int Mp, int Mc, int D, const double *__restrict__ x,
                                                                    const double *__restrict__ zs, const double *__restrict__ ell, float s2,
                                                                    int dd, float inv_sqrt_c, const float *__restrict__ Lt, float scale,
                                                                    h8 *__restrict__ Ph, h8 *__restrict__ Pl, h8 *__restrict__ acc_blocks,
                                                                    int64_t nps, float *__restrict__ resid, unsigned *__restrict__ maxbits,
                                                                    unsigned long long *__restrict__ words) {
    static_assert(agpl::kernel_kind_se_matern(KIND), "a squared exponential x Matern kind");
    se_build_body<KIND, DERIV>(N, Mp, Mc, D, x, zs, ell, s2, 0.f, 0.0, dd, inv_sqrt_c, Lt, scale, Ph, Pl, acc_blocks, nps, resid, maxbits, words);
}

// the all-orders additive (ANOVA) squared exponential kind's generator (AGPL_KERNEL_ANOVA_SE): the same body with gen4's seventh form, D
// float32 exponentials per pair into one float32 running product; eta in the float32 parameter slot of se_build_kernel.  A kernel of
// its own name, as se_build_product_kernel.  Dynamic LDS is the squared exponential's: no period, no table.
template <bool DERIV = false>
__global__ __launch_bounds__(256, 2) void se_build_anova_se_kernel(int64_t N, int Mp, int Mc, int D, const double *__restrict__ x,
                                                                   const double *__restrict__ zs, const double *__restrict__ ell, float s2,
                                                                   float eta, int dd, float inv_sqrt_c, const float *__restrict__ Lt,
                                                                   float scale, h8 *__restrict__ Ph, h8 *__restrict__ Pl,
                                                                   h8 *__restrict__ acc_blocks, int64_t nps, float *__restrict__ resid,
                                                                   unsigned *__restrict__ maxbits, unsigned long long *__restrict__ words) {
    se_build_body<AGPL_KERNEL_ANOVA_SE, DERIV>(N, Mp, Mc, D, x, zs, ell, s2, eta, 0.0, dd, inv_sqrt_c, Lt, scale, Ph, Pl, acc_blocks, nps,
                                               resid, maxbits, words);
}

// the squared exponential x categorical kind's generator (AGPL_KERNEL_SE_CATEGORICAL): the same body with gen4's eighth form, four float64
// chains over the leading dimensions, four compares per categorical dimension and one float32 exponential per pair; C in the float32
// parameter slot of se_build_kernel (an integer up to 16: exact).  A kernel of its own name, as se_build_product_kernel.  Dynamic LDS
// is the periodic kinds': 32 more doubles, of which the categorical dimensions' h_d = 1 / (2 ell_d^2) fill the first 16.
template <bool DERIV = false>
__global__ __launch_bounds__(256, 2) void se_build_se_categorical_kernel(int64_t N, int Mp, int Mc, int D, const double *__restrict__ x,
                                                                         const double *__restrict__ zs, const double *__restrict__ ell,
                                                                         float s2, float ncat, int dd, float inv_sqrt_c,
                                                                         const float *__restrict__ Lt, float scale, h8 *__restrict__ Ph,
                                                                         h8 *__restrict__ Pl, h8 *__restrict__ acc_blocks, int64_t nps,
                                                                         float *__restrict__ resid, unsigned *__restrict__ maxbits,
                                                                         unsigned long long *__restrict__ words) {
    se_build_body<AGPL_KERNEL_SE_CATEGORICAL, DERIV>(N, Mp, Mc, D, x, zs, ell, s2, ncat, 0.0, dd, inv_sqrt_c, Lt, scale, Ph, Pl, acc_blocks,
                                                     nps, resid, maxbits, words);
}

// the accumulate image's header (written once the realised max |phi| is known)
__global__ void se_header_kernel(int64_t N, int Mp, int scale_exp, const unsigned *__restrict__ maxbits, unsigned char *__restrict__ image) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    uint32_t *w = reinterpret_cast<uint32_t *>(image);
    w[0] = kImageMagic;
    w[1] = (uint32_t)scale_exp;
    w[2] = *maxbits; // max_abs (float bits)
    w[3] = 0u;
    *reinterpret_cast<int64_t *>(image + 16) = N;
    *reinterpret_cast<int32_t *>(image + 24) = Mp;
}

} // namespace

static size_t agpl_se_build_lds(int D) { return sizeof(float) * 2 * kStageFloats + sizeof(double) * BS * D + sizeof(float) * 2 * BS; }

// the images of 2^scale_exp Phi (either may be NULL) and the residual of N points; words[2], words[3], maxbits as se_build_kernel.
// DERIV: of the normalised derivative feature of dimension dd instead (se_build_kernel); a template, so that only a source that
// asks for it carries those instantiations.  Matern-1/2 has no derivative feature (kappa'(r) / r has no limit at 0).
template <bool DERIV>
static int32_t agpl_se_build_mode(agpl_ctx *ctx, int32_t kind, double kparam, int dd, double inv_sqrt_c, int64_t N, int32_t Mp, int32_t Mc,
                                  int32_t D, const double *x, const double *zs, const double *ell, double s2, const float *Lt, int scale_exp,
                                  void *Phi_hi, void *Phi_lo, void *acc_image, float *resid, unsigned *maxbits, unsigned long long *words) {
    if (Mp % 256 || D < 1 || D > 16 || N <= 0) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "se build: bad sizes");
    const int64_t ntiles = agpl_cdiv(N, BS);
    if (ntiles > 0x7fffffffLL) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "problem too large for one launch");
    const int64_t nps = ((N + 31) / 32) * 2; // the accumulate image's point slices (agpl_accumulate_image_bytes)
    h8 *blocks = acc_image ? reinterpret_cast<h8 *>((unsigned char *)acc_image + 256) : nullptr;
    switch (kind) { // the one dispatch on the kind: each instantiation holds its own rule's registers only
#define AGPL_SE_KIND_(K)                                                                                                      \
    case K:                                                                                                                   \
        se_build_kernel<K, DERIV><<<(unsigned)ntiles, 256, agpl_se_build_lds(D), ctx->stream>>>(                               \
            N, Mp, Mc, D, x, zs, ell, (float)s2, (float)kparam, dd, (float)inv_sqrt_c, Lt, ldexpf(1.f, scale_exp), (h8 *)Phi_hi,  \
            (h8 *)Phi_lo, blocks, nps, resid, maxbits, words);                                                                \
        break;
        AGPL_SE_KIND_(AGPL_KERNEL_SE)
    case AGPL_KERNEL_MATERN12:
        if constexpr (DERIV) {
            AGPL_FAIL(ctx, AGPL_ERR_UNSUPPORTED, "the Matern-1/2 kernel is not mean-square differentiable: it has no derivative feature");
        } else {
            se_build_kernel<AGPL_KERNEL_MATERN12><<<(unsigned)ntiles, 256, agpl_se_build_lds(D), ctx->stream>>>(
                N, Mp, Mc, D, x, zs, ell, (float)s2, (float)kparam, dd, (float)inv_sqrt_c, Lt, ldexpf(1.f, scale_exp), (h8 *)Phi_hi,
                (h8 *)Phi_lo, blocks, nps, resid, maxbits, words);
        }
        break;
        AGPL_SE_KIND_(AGPL_KERNEL_MATERN32)
        AGPL_SE_KIND_(AGPL_KERNEL_MATERN52)
        AGPL_SE_KIND_(AGPL_KERNEL_RQ)
#undef AGPL_SE_KIND_
#define AGPL_SE_KIND_(K) /* the product kinds: the same dispatch onto their own kernel name, no parameter */                   \
    case K:                                                                                                                   \
        se_build_product_kernel<K, DERIV><<<(unsigned)ntiles, 256, agpl_se_build_lds(D), ctx->stream>>>(                       \
            N, Mp, Mc, D, x, zs, ell, (float)s2, dd, (float)inv_sqrt_c, Lt, ldexpf(1.f, scale_exp), (h8 *)Phi_hi, (h8 *)Phi_lo,   \
            blocks, nps, resid, maxbits, words);                                                                              \
        break;
        AGPL_SE_KIND_(AGPL_KERNEL_MATERN32_PRODUCT)
        AGPL_SE_KIND_(AGPL_KERNEL_MATERN52_PRODUCT)
#undef AGPL_SE_KIND_
#define AGPL_SE_KIND_(K) /* the squared exponential x Matern kinds: likewise */                                                \
    case K:                                                                                                                   \
        se_build_se_matern_kernel<K, DERIV><<<(unsigned)ntiles, 256, agpl_se_build_lds(D), ctx->stream>>>(                     \
            N, Mp, Mc, D, x, zs, ell, (float)s2, dd, (float)inv_sqrt_c, Lt, ldexpf(1.f, scale_exp), (h8 *)Phi_hi, (h8 *)Phi_lo,   \
            blocks, nps, resid, maxbits, words);                                                                              \
        break;
        AGPL_SE_KIND_(AGPL_KERNEL_SE_MATERN32)
        AGPL_SE_KIND_(AGPL_KERNEL_SE_MATERN52)
#undef AGPL_SE_KIND_
    case AGPL_KERNEL_PERIODIC:
        se_build_periodic_kernel<DERIV><<<(unsigned)ntiles, 256, agpl_se_build_lds(D) + 32 * sizeof(double), ctx->stream>>>(
            N, Mp, Mc, D, x, zs, ell, (float)s2, kparam, dd, (float)inv_sqrt_c, Lt, ldexpf(1.f, scale_exp), (h8 *)Phi_hi, (h8 *)Phi_lo, blocks,
            nps, resid, maxbits, words);
        break;
    case AGPL_KERNEL_SE_PERIODIC:
        se_build_se_periodic_kernel<DERIV><<<(unsigned)ntiles, 256, agpl_se_build_lds(D) + 32 * sizeof(double), ctx->stream>>>(
            N, Mp, Mc, D, x, zs, ell, (float)s2, kparam, dd, (float)inv_sqrt_c, Lt, ldexpf(1.f, scale_exp), (h8 *)Phi_hi, (h8 *)Phi_lo, blocks,
            nps, resid, maxbits, words);
        break;
    case AGPL_KERNEL_SE_COSINE:
        se_build_se_cosine_kernel<DERIV><<<(unsigned)ntiles, 256, agpl_se_build_lds(D) + 32 * sizeof(double), ctx->stream>>>(
            N, Mp, Mc, D, x, zs, ell, (float)s2, kparam, dd, (float)inv_sqrt_c, Lt, ldexpf(1.f, scale_exp), (h8 *)Phi_hi, (h8 *)Phi_lo, blocks,
            nps, resid, maxbits, words);
        break;
    case AGPL_KERNEL_ADDITIVE_SE:
        se_build_additive_se_kernel<DERIV><<<(unsigned)ntiles, 256, agpl_se_build_lds(D), ctx->stream>>>(
            N, Mp, Mc, D, x, zs, ell, (float)s2, dd, (float)inv_sqrt_c, Lt, ldexpf(1.f, scale_exp), (h8 *)Phi_hi, (h8 *)Phi_lo, blocks, nps,
            resid, maxbits, words);
        break;
    case AGPL_KERNEL_ADDITIVE2_SE:
        se_build_additive2_se_kernel<DERIV><<<(unsigned)ntiles, 256, agpl_se_build_lds(D), ctx->stream>>>(
            N, Mp, Mc, D, x, zs, ell, (float)s2, kparam, dd, (float)inv_sqrt_c, Lt, ldexpf(1.f, scale_exp), (h8 *)Phi_hi, (h8 *)Phi_lo, blocks,
            nps, resid, maxbits, words);
        break;
    case AGPL_KERNEL_ANOVA_SE: // (eta rounded to float32 here, once)
        se_build_anova_se_kernel<DERIV><<<(unsigned)ntiles, 256, agpl_se_build_lds(D), ctx->stream>>>(
            N, Mp, Mc, D, x, zs, ell, (float)s2, (float)kparam, dd, (float)inv_sqrt_c, Lt, ldexpf(1.f, scale_exp), (h8 *)Phi_hi, (h8 *)Phi_lo,
            blocks, nps, resid, maxbits, words);
        break;
    case AGPL_KERNEL_SE_CATEGORICAL: // (C checked against D where the plan was made; checked again here: it bounds the loops over LDS)
        if (!(kparam >= 1.0 && kparam <= (double)D)) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "se build: C = %g categorical inputs of D = %d", kparam, D);
        se_build_se_categorical_kernel<DERIV><<<(unsigned)ntiles, 256, agpl_se_build_lds(D) + 32 * sizeof(double), ctx->stream>>>(
            N, Mp, Mc, D, x, zs, ell, (float)s2, (float)kparam, dd, (float)inv_sqrt_c, Lt, ldexpf(1.f, scale_exp), (h8 *)Phi_hi, (h8 *)Phi_lo,
            blocks, nps, resid, maxbits, words);
        break;
    default: AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "se build: unknown kernel kind %d", kind);
    }
    AGPL_LAUNCH_CHECK(ctx);
    if (acc_image) {
        se_header_kernel<<<1, 64, 0, ctx->stream>>>(N, Mp, scale_exp, maxbits, (unsigned char *)acc_image);
        AGPL_LAUNCH_CHECK(ctx);
        if (ctx->checked_image == acc_image) ctx->checked_image = nullptr;
    }
    return AGPL_OK;
}

// the plans' own mode (a template only so that a source that never calls it carries none of its instantiations)
template <int = 0>
static int32_t agpl_se_build(agpl_ctx *ctx, int32_t kind, double kparam, int64_t N, int32_t Mp, int32_t Mc, int32_t D, const double *x,
                      const double *zs, const double *ell, double s2, const float *Lt, int scale_exp, void *Phi_hi, void *Phi_lo, void *acc_image,
                      float *resid, unsigned *maxbits, unsigned long long *words) {
    return agpl_se_build_mode<false>(ctx, kind, kparam, 0, 0.0, N, Mp, Mc, D, x, zs, ell, s2, Lt, scale_exp, Phi_hi, Phi_lo, acc_image, resid,
                                     maxbits, words);
}
