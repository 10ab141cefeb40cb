// agpl_pathwise.hip -- pathwise draws of the posterior function at new inputs (agpl_plan_sample_paths, include/agpl_pathwise.h):
//     F_out[t][l][i] = mu0 + phi(x_i)' c_tl + s psi(x_i)' W_tl,   c_tl = V_tl - L^-1 (s Psi(Z)' W_tl + sqrt(jitter) Xi_tl),   s = sigma sqrt(2 / F)
// is ONE product [Ns x (M + F)] . [(M + F) x T L] whose left operand is the chunk's marginal image that se_build_kernel
// (agpl_se_build.h) writes followed by the image of Psi written here, and whose right operand [c ; s W] is packed here in the same
// blocked split-float16 layout (agpl_split.hip): blocks (row block of 128, k-slice of 16) = [plane 2][row 128][8 halves].
//
//   set-up, float64, once per call (L^-1: hy_linv of agpl_hyper_impl.h, the route of agpl_plan_hyper_grad; hy_gemm, hy_max_kernel):
//   pw_check_kernel    the first draw with a non-finite V / W / Xi, the first feature with a non-finite omega / phase
//   pw_psiz_kernel     Psi(Z) [F][Mc] from the plan's z / ell
//   pw_axpy_kernel     up += sqrt(jitter) Xi
//   pw_pack_kernel     rows t L + l of [c ; s W]: the Mc features of c in ceil(Mc / 16) slices at 2^ec, then the F of s W in Fp / 16
//                      slices at 2^ew (pw_scales: e_phi + ec = epsi + ew); rows past T L and features past Mc / F zero; the one
//                      factor 2^-(e_phi + ec) that undoes the scales
//   per chunk of 65536 points, per sub-chunk of the Psi image:
//   pw_feature_kernel  Psi of the sub-chunk at 2^epsi: one workgroup per 128-point tile and group of slices, thread = (plane, point),
//                      8 features per slice: float64 phase (d ascending, FMA), one period in float64, cospif in float32
//   pw_project_kernel  one 128-point tile per workgroup (4 waves, 64 rows x 64 points each); for each 128-row block of [c ; s W],
//                      the row-masked tile product of agpl_tile_product.h (where the pipeline is stated: two 16-feature slices per
//                      stage through LDS, register-staged double buffer, hi hi + hi lo + lo hi on v_mfma_f32_32x32x16_f16, float32
//                      accumulation) with a loader of its own: the slices of Phi, then those of Psi, then zeros to the end of the last
//                      stage, into one accumulator set.  The 128 x 128 result goes through LDS once ([row][point]) and is
//                      read back with one thread per point and half block: F_out = mu0 + result, coalesced along the points.
// No float atomics, no sum depends on the launch: a point's outputs depend on its x, the call's arrays and the plan alone.
#include "../../include/agpl_pathwise.h"
#include "agpl_hyper_impl.h"
#include "agpl_tile_product.h"

namespace {

constexpr int64_t kPathChunk = 1 << 16;            // points per step (agpl_plan_predict's chunk)
constexpr size_t kPsiBudget = (size_t)256 << 20;   // bytes of the Psi image (both planes)
constexpr int kPsiExpMax = 14, kPsiExpMin = 0;     // |psi| <= 1: 2^14 psi is well inside float16; below 2^0 the lo plane is all subnormal
constexpr int kFree = 1000;                        // "no bound" exponent of an all-zero operand
constexpr double kInv2Pi = 0.15915494309189535;    // 1 / (2 pi)
constexpr int kMaxF = 8192;

// words[0] <- first draw with a non-finite V / W / Xi entry, words[1] <- first feature with a non-finite omega / phase (min)
__global__ __launch_bounds__(256) void pw_check_kernel(int64_t nV, int64_t LM, int64_t nW, int64_t LF, int64_t nO, int D, int F,
                                                       const double *__restrict__ V, const double *__restrict__ W,
                                                       const double *__restrict__ Xi, const double *__restrict__ omega,
                                                       const double *__restrict__ phase, unsigned long long *__restrict__ words) {
    const int64_t total = 2 * nV + nW + nO + F;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        double v;
        int64_t id;
        int w = 0;
        if (e < nV) {
            v = V[e], id = e / LM;
        } else if (e < 2 * nV) {
            v = Xi ? Xi[e - nV] : 0.0, id = (e - nV) / LM;
        } else if (e < 2 * nV + nW) {
            v = W[e - 2 * nV], id = (e - 2 * nV) / LF;
        } else if (e < 2 * nV + nW + nO) {
            v = omega[e - 2 * nV - nW], id = (e - 2 * nV - nW) / D, w = 1;
        } else {
            v = phase[e - 2 * nV - nW - nO], id = e - 2 * nV - nW - nO, w = 1;
        }
        if (!(fabs(v) <= 1.79e308)) atomicMin(&words[w], (unsigned long long)id);
    }
}

// one period of the phase b + sum_d omega_d u_d (d ascending, FMA): t in [-1/2, 1/2] with cos(phase) = cos(2 pi t)
__device__ __forceinline__ double pw_period(const double *__restrict__ om, double b, const double *u, int D) {
    double p = b;
    for (int d = 0; d < D; ++d) p = fma(om[d], u[d], p);
    const double q = p * kInv2Pi;
    return q - rint(q);
}

// PZ[j][a] = cos(omega_j . zs_a + b_j) in float64
__global__ __launch_bounds__(256) void pw_psiz_kernel(int F, int Mc, int D, const double *__restrict__ omega,
                                                      const double *__restrict__ phase, const double *__restrict__ zs,
                                                      double *__restrict__ PZ) {
    const int64_t total = (int64_t)F * Mc;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int j = (int)(e / Mc), a = (int)(e - (int64_t)j * Mc);
        double u[16];
        for (int d = 0; d < D; ++d) u[d] = zs[(int64_t)a * D + d];
        PZ[e] = cos(6.283185307179586 * pw_period(omega + (int64_t)j * D, phase[j], u, D));
    }
}

// y += alpha x
__global__ __launch_bounds__(256) void pw_axpy_kernel(int64_t total, double alpha, const double *__restrict__ x, double *__restrict__ y) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) y[e] += alpha * x[e];
}

// The three exponents from words[2] = max |c| and words[3] = max |W| (bit patterns), s and the plan's e_phi:  with ecm / ewm the
// largest exponents float16 allows (2^e max in [2^13, 2^14); no bound for an all-zero operand),
//   E = min(e_phi + ecm, 14 + ewm);  ec = E - e_phi;  epsi = max(E - ewm, 0);  ew = E - epsi:
// e_phi + ec = epsi + ew = E always, ec <= ecm, ew <= ewm, 0 <= epsi <= 14 -- the operand that gives way is the one whose product is
// the smaller.  E stays within float32's exponent range (|e_phi| <= 30, |ecm|, |ewm| <= 90).
struct PwScales {
    int E, ec, ew, epsi;
};
__device__ __forceinline__ PwScales pw_scales(const unsigned long long *__restrict__ words, double s, int e_phi) {
    const double mc = __longlong_as_double((long long)words[2]), mw = s * __longlong_as_double((long long)words[3]);
    const int ecm = mc > 0.0 ? tile_scale_exp(mc) : kFree, ewm = mw > 0.0 ? tile_scale_exp(mw) : kFree;
    PwScales o;
    o.E = e_phi + ecm < kPsiExpMax + ewm ? e_phi + ecm : kPsiExpMax + ewm;
    if (ecm == kFree && ewm == kFree) o.E = e_phi;
    o.ec = o.E - e_phi;
    o.epsi = ewm == kFree ? kPsiExpMin : (o.E - ewm > kPsiExpMin ? o.E - ewm : kPsiExpMin);
    o.ew = o.E - o.epsi;
    return o;
}

// grid (nks = nksM + Fp / 16 k-slices, row blocks): rows of Cc [T L][Mc] and W [T L][F]; *unscale = 2^-E
__global__ __launch_bounds__(256) void pw_pack_kernel(int64_t TL, int Mc, int nksM, int F, double s, const double *__restrict__ Cc,
                                                      const double *__restrict__ W, const unsigned long long *__restrict__ words,
                                                      int e_phi, h8 *__restrict__ Rh, h8 *__restrict__ Rl, float *__restrict__ unscale) {
    const int nks = gridDim.x;
    const int ks = blockIdx.x, rb = blockIdx.y;
    const int plane = threadIdx.x >> 7, row = threadIdx.x & 127;
    const PwScales sc = pw_scales(words, s, e_phi);
    if (ks == 0 && rb == 0 && threadIdx.x == 0) *unscale = ldexpf(1.f, -sc.E);
    const int64_t g = (int64_t)rb * BS + row;
    const bool phi_part = ks < nksM;
    const double f = phi_part ? ldexp(1.0, sc.ec) : ldexp(s, sc.ew);
    h8 hi, lo;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int a = (phi_part ? ks : ks - nksM) * KT + plane * 8 + j;
        double x = 0.0;
        if (g < TL) {
            if (phi_part) {
                if (a < Mc) x = Cc[g * Mc + a] * f;
            } else if (a < F) {
                x = W[g * F + a] * f;
            }
        }
        tile_split(hi, lo, j, (float)x);
    }
    const int64_t o = ((int64_t)rb * nks + ks) * 256 + threadIdx.x;
    Rh[o] = hi;
    Rl[o] = lo;
}

// grid (tiles of the sub-chunk, groups of slices): block (tile, slice) of the Psi image = [plane 2][point 128][8 features] at 2^epsi;
// points past n and features past F are zero.  x: the sub-chunk's inputs.
__global__ __launch_bounds__(256) void pw_feature_kernel(int64_t n, int D, int F, int nksF, const double *__restrict__ x,
                                                         const double *__restrict__ ell, const double *__restrict__ omega,
                                                         const double *__restrict__ phase, const unsigned long long *__restrict__ words,
                                                         double s, int e_phi, h8 *__restrict__ Sh, h8 *__restrict__ Sl) {
    const int64_t tile = blockIdx.x;
    const int plane = threadIdx.x >> 7, pt = threadIdx.x & 127;
    const int64_t np = tile * BS + pt;
    const bool live = np < n;
    const float scale = ldexpf(1.f, pw_scales(words, s, e_phi).epsi);
    double u[16];
#pragma unroll
    for (int d = 0; d < 16; ++d) u[d] = (live && d < D) ? x[np * D + d] / ell[d] : 0.0;
    for (int ks = blockIdx.y; ks < nksF; ks += gridDim.y) {
        h8 hi, lo;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int f = ks * KT + plane * 8 + j;
            float v = 0.f;
            if (live && f < F) {
                double p = phase[f];
                const double *om = omega + (int64_t)f * D;
#pragma unroll
                for (int d = 0; d < 16; ++d)
                    if (d < D) p = fma(om[d], u[d], p);
                const double q = p * kInv2Pi;
                const double t = q - rint(q);
                v = cospif((float)(2.0 * t)) * scale;
            }
            tile_split(hi, lo, j, v);
        }
        const int64_t o = (tile * nksF + ks) * 256 + threadIdx.x;
        Sh[o] = hi;
        Sl[o] = lo;
    }
}

// n: the sub-chunk's points; pitch: Ns (the row pitch of mu0 and F_out, which point at the sub-chunk's first point).
// Ph / Pl: the sub-chunk's first tile of the marginal image (nksP = Mp / 16 slices per tile, the first nksM carry features);
// Sh / Sl: the Psi image (nksF slices per tile); Rh / Rl: [c ; s W] (nksM + nksF slices per row block).
// LDS: two stage buffers, reused by the epilogue tile.
__global__ __launch_bounds__(256, 2) void pw_project_kernel(int64_t n, int64_t pitch, int nksP, int nksM, int nksF, int64_t TL, int L,
                                                            int nblk, const h8 *__restrict__ Ph, const h8 *__restrict__ Pl,
                                                            const h8 *__restrict__ Sh, const h8 *__restrict__ Sl,
                                                            const h8 *__restrict__ Rh, const h8 *__restrict__ Rl,
                                                            const float *__restrict__ unscale, const float *__restrict__ mu0,
                                                            float *__restrict__ F_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    h8 *st = reinterpret_cast<h8 *>(smem_raw);     // [2][kStageH8]
    float *E = reinterpret_cast<float *>(smem_raw); // [128 rows][128 points]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int li = lane & 31, lk = lane >> 5;
    const int nks = nksM + nksF, nst = (nks + KU - 1) / KU;
    const int64_t tile = blockIdx.x;
    const int p = tid & 127, hh = tid >> 7; // epilogue: this thread's point and half block
    const int64_t np = tile * BS + p;
    const bool livep = np < n;
    const float un = *unscale;
    const h8 *psrc_h = Ph + tile * nksP * 256 + tid, *psrc_l = Pl + tile * nksP * 256 + tid;
    const h8 *ssrc_h = Sh + tile * nksF * 256 + tid, *ssrc_l = Sl + tile * nksF * 256 + tid;
    const int fa = lk * 128 + wr * 64 + li;       // row fragment of rows wr 64 + li (+ 32), plane lk
    const int fb = 512 + lk * 128 + wc * 64 + li; // point fragment of points wc 64 + li (+ 32)

    for (int rb = 0; rb < nblk; ++rb) {
        const int rows_live = (int)(TL - (int64_t)rb * BS < BS ? TL - (int64_t)rb * BS : BS);
        const bool act0 = wr * 64 < rows_live, act1 = wr * 64 + 32 < rows_live;
        const h8 *rsrc_h = Rh + (int64_t)rb * nks * 256 + tid, *rsrc_l = Rl + (int64_t)rb * nks * 256 + tid;
        f32x16 acc[2][2];
        // slice k of the product: Phi's slice k for k < nksM, Psi's slice k - nksM after it; a stage past the last slice is zero
        tile_product<true, false>(
            [&](int k, h8(&rg)[4]) __attribute__((always_inline)) {
                if (k < nks) {
                    rg[0] = rsrc_h[k * 256];
                    rg[1] = rsrc_l[k * 256];
                    if (k < nksM) {
                        rg[2] = psrc_h[k * 256];
                        rg[3] = psrc_l[k * 256];
                    } else {
                        rg[2] = ssrc_h[(k - nksM) * 256];
                        rg[3] = ssrc_l[(k - nksM) * 256];
                    }
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q)
#pragma unroll
                        for (int e = 0; e < 8; ++e) rg[q][e] = (_Float16)0.f;
                }
            },
            nst, st, tid, fa, fb, acc, act0, act1);
        AGPL_TILE_SCATTER(E, BS, un, acc); // as [row][point]
        __syncthreads();
        const int64_t g0 = (int64_t)rb * BS + hh * 64;
        const int cnt = (int)(TL - g0 < 64 ? (TL - g0 < 0 ? 0 : TL - g0) : 64);
        int l = (int)(g0 % L);
        if (livep) {
            for (int i = 0; i < cnt; ++i) {
                float v = E[(hh * 64 + i) * BS + p];
                if (mu0) v += mu0[(int64_t)l * pitch + np];
                F_out[(g0 + i) * pitch + np] = v;
                if (++l == L) l = 0;
            }
        }
        __syncthreads();
    }
}

} // namespace

extern "C" int32_t agpl_plan_sample_paths(agpl_plan *p, int32_t T, const double *V, int32_t F, const double *omega, const double *phase,
                                          const double *W, const double *Xi, int64_t Ns, const double *x_s, const float *mu0_s,
                                          float *F_out) {
    if (!p || !p->ctx) return AGPL_ERR_INVALID_ARGUMENT;
    agpl_ctx *ctx = p->ctx;
    if (!p->se)
        AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT,
                  "agpl_plan_sample_paths needs a plan made from raw inputs (agpl_plan_create_se / agpl_plan_create_stationary)");
    if (T < 1) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "T = %d: at least one draw is needed", T);
    if (F < 1 || F > kMaxF) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "F = %d features: 1 ... %d are supported", F, kMaxF);
    if (Ns < 0) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "Ns = %lld < 0", (long long)Ns);
    if (Ns == 0) return AGPL_OK;
    if (!V || !omega || !phase || !W || !x_s || !F_out) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "null argument");
    const int L = p->L, Mp = p->M, Mc = p->Mc, D = p->D;
    const int64_t TL = (int64_t)T * L, nV = TL * Mc, nW = TL * F;
    const int64_t nblk = agpl_cdiv(TL, BS);
    if (nblk > 8191) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "T L = %lld rows are too many for one call", (long long)TL);
    const int Fp = (F + KT - 1) / KT * KT;
    const int nksP = Mp / KT, nksM = (Mc + KT - 1) / KT, nksF = Fp / KT, nks = nksM + nksF;
    const int64_t C = Ns < kPathChunk ? Ns : kPathChunk;
    const int64_t Cpad = agpl_cdiv(C, BS) * BS;
    int64_t sub = (int64_t)(kPsiBudget / (4 * (size_t)Fp)) / BS * BS; // points of a sub-chunk
    if (sub < BS) sub = BS;
    if (sub > Cpad) sub = Cpad;
    const double s = sqrt(p->s2) * sqrt(2.0 / (double)F);
    const auto al = agpl_align256;
    const size_t img = al((size_t)agpl_split_features_bytes(C, Mp));      // one plane of the chunk's marginal image
    const size_t simg = al(sizeof(_Float16) * (size_t)sub * Fp);          // one plane of the Psi image
    const size_t rimg = al(sizeof(_Float16) * (size_t)nblk * BS * nks * KT); // one plane of [c ; s W]
    const size_t rsb = al(sizeof(float) * (size_t)C);
    const size_t matp = al(sizeof(double) * (size_t)Mp * Mp), matc = al(sizeof(double) * (size_t)Mc * Mc);
    const size_t zsb = al(sizeof(double) * (size_t)Mp * D), gzb = al(sizeof(double) * (size_t)Mp);
    const size_t pzb = al(sizeof(double) * (size_t)F * Mc), rowb = al(sizeof(double) * (size_t)nV);
    const size_t need = 2 * img + 2 * simg + 2 * rimg + rsb + 2 * matp + matc + zsb + gzb + pzb + 2 * rowb + 4096;
    if (int32_t rc_ = agpl_pred_reserve(p, need, "prediction")) return rc_; // (every call carves the scratch anew)
    char *w = (char *)p->pred;
    auto take = [&](size_t b) { char *r = w; w += b; return r; };
    void *Ph = take(img), *Pl = take(img);
    h8 *Sh = (h8 *)take(simg), *Sl = (h8 *)take(simg);
    h8 *Rh = (h8 *)take(rimg), *Rl = (h8 *)take(rimg);
    float *rs = (float *)take(rsb);
    double *Gk = (double *)take(matp), *Fw = (double *)take(matp), *Li = (double *)take(matc);
    double *zsc = (double *)take(zsb), *gz = (double *)take(gzb);
    double *PZ = (double *)take(pzb), *Up = (double *)take(rowb), *Cc = (double *)take(rowb);
    char *tail = take(4096);
    unsigned long long *words = (unsigned long long *)tail;      // the generator's eight status words (not reported: NaN outputs)
    unsigned *maxbits = (unsigned *)(words + 8);
    unsigned long long *kw = (unsigned long long *)(tail + 128);  // se_kzz_kernel's words (not reported: the plan was made from this z)
    unsigned long long *cw = (unsigned long long *)(tail + 256);  // [0] first bad draw, [1] first bad feature, [2] max |c|, [3] max |W|
    float *unscale = (float *)(tail + 512);
    double *ones = (double *)(tail + 1024);                      // [16] unit lengthscales: the plan holds z / ell

    // the set-up: the domain check, L^-1, c, the scales, the image of [c ; s W]; the one wait of the call is behind it
    AGPL_HIP(ctx, hipMemsetAsync(words, 0xff, 8 * sizeof(unsigned long long), ctx->stream));
    AGPL_HIP(ctx, hipMemsetAsync(maxbits, 0, sizeof(unsigned), ctx->stream));
    AGPL_HIP(ctx, hipMemsetAsync(kw, 0xff, 8 * sizeof(unsigned long long), ctx->stream));
    AGPL_HIP(ctx, hipMemsetAsync(cw, 0xff, 2 * sizeof(unsigned long long), ctx->stream));
    AGPL_HIP(ctx, hipMemsetAsync(cw + 2, 0, 2 * sizeof(unsigned long long), ctx->stream));
    AGPL_HIP(ctx, hipMemsetAsync(gz, 0, sizeof(double) * Mp, ctx->stream));
    static const double host_ones[16] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1};
    AGPL_HIP(ctx, hipMemcpyAsync(ones, host_ones, sizeof(host_ones), hipMemcpyHostToDevice, ctx->stream));
    pw_check_kernel<<<hy_blocks(2 * nV + nW + (int64_t)F * (D + 1)), 256, 0, ctx->stream>>>(nV, (int64_t)L * Mc, nW, (int64_t)L * F,
                                                                                         (int64_t)F * D, D, F, V, W, Xi, omega, phase, cw);
    AGPL_LAUNCH_CHECK(ctx);
    int32_t rc = hy_linv(ctx, p, ones, Gk, gz, Fw, Li, zsc, kw);
    if (rc) return rc;
    pw_psiz_kernel<<<hy_blocks((int64_t)F * Mc), 256, 0, ctx->stream>>>(F, Mc, D, omega, phase, zsc, PZ);
    AGPL_LAUNCH_CHECK(ctx);
    if ((rc = hy_gemm(ctx, (int)TL, Mc, F, W, F, 0, PZ, Mc, 0, Up, Mc, s, 0.0))) return rc; // up = s W Psi(Z)
    if (Xi && p->jitter > 0.0) {
        pw_axpy_kernel<<<hy_blocks(nV), 256, 0, ctx->stream>>>(nV, sqrt(p->jitter), Xi, Up);
        AGPL_LAUNCH_CHECK(ctx);
    }
    AGPL_HIP(ctx, hipMemcpyAsync(Cc, V, sizeof(double) * (size_t)nV, hipMemcpyDeviceToDevice, ctx->stream));
    if ((rc = hy_gemm(ctx, (int)TL, Mc, Mc, Up, Mc, 0, Li, Mc, 1, Cc, Mc, -1.0, 1.0))) return rc; // c = V - up L^-T
    hy_max_kernel<<<hy_blocks(nV), 256, 0, ctx->stream>>>(nV, Cc, cw + 2);
    AGPL_LAUNCH_CHECK(ctx);
    hy_max_kernel<<<hy_blocks(nW), 256, 0, ctx->stream>>>(nW, W, cw + 3);
    AGPL_LAUNCH_CHECK(ctx);
    pw_pack_kernel<<<dim3((unsigned)nks, (unsigned)nblk), 256, 0, ctx->stream>>>(TL, Mc, nksM, F, s, Cc, W, cw, p->scale_exp, Rh, Rl, unscale);
    AGPL_LAUNCH_CHECK(ctx);
    unsigned long long bad[2] = {~0ull, ~0ull};
    AGPL_HIP(ctx, hipMemcpyAsync(bad, cw, sizeof(bad), hipMemcpyDeviceToHost, ctx->stream));
    rc = agpl_ctx_synchronize(ctx); // waits, and collects the outcome of the factorisation
    if (rc) return rc;
    if (bad[0] != ~0ull) AGPL_FAIL(ctx, AGPL_ERR_DOMAIN, "draw %llu has a non-finite entry (V, W or Xi)", bad[0]);
    if (bad[1] != ~0ull) AGPL_FAIL(ctx, AGPL_ERR_DOMAIN, "feature %llu has a non-finite frequency or phase", bad[1]);

    AGPL_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&pw_project_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      kStageBytes));
    const unsigned fgroups = nksF < 4 ? (unsigned)nksF : 4u;
    for (int64_t c0 = 0; c0 < Ns; c0 += C) {
        const int64_t n = Ns - c0 < C ? Ns - c0 : C;
        rc = agpl_se_build(ctx, p->kind, p->kparam, n, Mp, Mc, D, x_s + c0 * D, p->zs, p->ell, p->s2, p->Lt, p->scale_exp, Ph, Pl, nullptr,
                           rs, maxbits, words);
        if (rc) return rc;
        for (int64_t q0 = 0; q0 < n; q0 += sub) { // (sub is a multiple of 128: a sub-chunk starts at a tile of the chunk's image)
            const int64_t nq = n - q0 < sub ? n - q0 : sub;
            const unsigned tiles = (unsigned)agpl_cdiv(nq, BS);
            pw_feature_kernel<<<dim3(tiles, fgroups), 256, 0, ctx->stream>>>(nq, D, F, nksF, x_s + (c0 + q0) * D, p->ell, omega, phase, cw, s,
                                                                            p->scale_exp, Sh, Sl);
            AGPL_LAUNCH_CHECK(ctx);
            const int64_t t0 = q0 / BS;
            pw_project_kernel<<<tiles, 256, kStageBytes, ctx->stream>>>(
                nq, Ns, nksP, nksM, nksF, TL, L, (int)nblk, (const h8 *)Ph + t0 * nksP * 256, (const h8 *)Pl + t0 * nksP * 256, Sh, Sl, Rh, Rl,
                unscale, mu0_s ? mu0_s + c0 + q0 : nullptr, F_out + c0 + q0);
            AGPL_LAUNCH_CHECK(ctx);
        }
    }
    return AGPL_OK;
}
