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
// factor's curvature, agpl::kernel_modulation_curvature, formed here; the other dimensions of such a kind carry the factor m); everything after the generator is the same code (|psi| <= sigma as |phi|: the same scale, clamp and words).  Without DERIV
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
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *stage0 = smem;                                          // [2][kStageFloats]
    double *xs = reinterpret_cast<double *>(smem + 2 * kStageFloats); // [128][D]
    float *qred = reinterpret_cast<float *>(xs + BS * D);          // [2][128]
    double *wt = reinterpret_cast<double *>(qred + 2 * BS);        // WARPED: [2][16] = ell_d / period | 1 / ell_d (the warped d only); MOD: ell_d / period of the modulated d
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
    auto gen4 = [&](int n, int b) -> float4 { // K[b .. b + 3][n]
        float v[4];
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
