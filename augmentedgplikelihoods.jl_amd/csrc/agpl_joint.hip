// agpl_joint.hip -- the joint posterior of f at new inputs under a plan's q(v) (agpl_plan_predict_cov, include/agpl_joint.h):
//     Cov_l[i][j] = k(x_a_i, x_b_j) + phi(x_a_i)' W_l phi(x_b_j),   W_l = U_l' U_l - I,
// as two products on the f16 matrix cores over images in the blocked split-float16 layout of agpl_split.hip / agpl_chain.hip:
// blocks (tile of 128 rows, k-slice of 16) = [plane 2][row 128][8 halves].
//
//   joint_w_kernel    per call and latent: W_l in float64 from the column-major lower triangle U_l of the plan's A_work
//                     (W[a][b] = sum_{c >= max(a, b)} U[c][a] U[c][b] - [a == b], c ascending, fused multiply-adds; zero beyond Mc,
//                     where U is the identity), packed at 2^15 (kUExp: |W| <= 1 because 0 <= S <= I).
//   joint_t_kernel    per chunk of x_b and latent: T = W_l Phi_b, one 128-point tile of the chunk's image (se_build_kernel,
//                     agpl_se_build.h) per workgroup, the row blocks of W in turn -- the tile product of agpl_tile_product.h (where
//                     the pipeline is stated: hi hi + hi lo + lo hi on v_mfma_f32_32x32x16_f16, float32 accumulation, two k-slices
//                     per stage through LDS, register-staged double buffer), all rows live -- kept as a second split image at the
//                     plan's scale (|W phi| <= |phi| <= sigma: no overflow).
//   joint_cov_kernel  per (128 a points, 128 b points): Phi_a' T over Mp with the same product; the tile goes through LDS once and is
//                     read back one column j per thread: r^2 in float64 from x / ell staged in LDS, k = s2 kappa(r) by the generator's
//                     float32 rule (one instantiation per kind, chosen on the host), the sum stored coalesced along j under ld and
//                     the ragged edges.  Symmetric form: tiles wholly above the diagonal leave at once, entries above it are not
//                     stored, and every entry below it is stored a second time at its mirror position (through the LDS tile, so that
//                     those stores are coalesced too): one writer per entry, no atomics.
// Every sum runs in a fixed order: an entry depends on (x_a_i, x_b_j, the plan) only.
#include "../../include/agpl_joint.h"
#include "agpl_se_build.h"
#include "agpl_tile_product.h"

namespace {

constexpr int EP = BS + 1;                     // pitch of joint_cov_kernel's tile: read by rows and by columns
constexpr int kCovTileBytes = (BS * EP * 4 + 15) / 16 * 16;
static_assert(kCovTileBytes >= kStageBytes, "the covariance tile covers the two stage buffers");
constexpr int64_t kJointChunk = 1 << 16; // points of either set per step (agpl_plan_predict's chunk)

// grid (Mp / 16 k-slices, Mp / 128 row blocks, L).  A: the plan's A_work, [L][Mp][Mp], U[c][a] = A[a Mp + c] for c >= a.
__global__ __launch_bounds__(256) void joint_w_kernel(int Mc, int Mp, const double *__restrict__ A, h8 *__restrict__ Wh,
                                                      h8 *__restrict__ Wl) {
    __shared__ double Ua[KT][BS + 1];
    __shared__ double Ub[KT][KT + 1];
    const int nks = Mp / KT, nrb = Mp / BS;
    const int ks = blockIdx.x, rb = blockIdx.y, l = blockIdx.z;
    const int tid = threadIdx.x;
    const int plane = tid >> 7, row = tid & 127;
    const double *U = A + (int64_t)l * Mp * Mp;
    const int a0 = rb * BS, b0 = ks * KT;
    double s[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] = 0.0;
    // a product needs c >= max(a, b) >= max(a0, b0) and c < Mc; everything else enters as an exact zero
    for (int c0 = a0 > b0 ? a0 : b0; c0 < Mc; c0 += KT) {
        {
            const int aa = tid >> 1, ga = a0 + aa;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int cc = (tid & 1) * 8 + q, c = c0 + cc;
                const double u = U[(int64_t)ga * Mp + c];
                Ua[cc][aa] = (c >= ga && c < Mc && ga < Mc) ? u : 0.0;
            }
            const int bb = tid >> 4, gb = b0 + bb, cc = tid & 15, c = c0 + cc;
            const double u = U[(int64_t)gb * Mp + c];
            Ub[cc][bb] = (c >= gb && c < Mc && gb < Mc) ? u : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int cc = 0; cc < KT; ++cc) {
            const double ua = Ua[cc][row];
#pragma unroll
            for (int j = 0; j < 8; ++j) s[j] = fma(ua, Ub[cc][plane * 8 + j], s[j]);
        }
        __syncthreads();
    }
    const int a = a0 + row;
    h8 hi, lo;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int b = b0 + plane * 8 + j;
        const double w = (a == b && a < Mc) ? s[j] - 1.0 : s[j];
        tile_split(hi, lo, j, (float)(w * 32768.0)); // 2^kUExp
    }
    const int64_t o = (((int64_t)l * nrb + rb) * nks + ks) * 256 + tid;
    Wh[o] = hi;
    Wl[o] = lo;
}

// One 128-point tile of the chunk's image per workgroup (4 waves, 64 rows of W x 64 points each).  Th / Tl: the image of
// 2^e W Phi_b in the layout of Ph / Pl (se_build_kernel's marginal image).  Wh / Wl: this latent's image.
__global__ __launch_bounds__(256, 2) void joint_t_kernel(int Mp, const h8 *__restrict__ Ph, const h8 *__restrict__ Pl,
                                                         const h8 *__restrict__ Wh, const h8 *__restrict__ Wl, h8 *__restrict__ Th,
                                                         h8 *__restrict__ Tl) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    h8 *st = reinterpret_cast<h8 *>(smem_raw);     // [2][kStageH8]
    float *E = reinterpret_cast<float *>(smem_raw); // [128 rows of W][128 points]
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int li = lane & 31, lk = lane >> 5;
    const int nks = Mp / KT, nrb = Mp / BS;
    const int64_t tile = blockIdx.x;
    const int fa = lk * 128 + wr * 64 + li;       // W hi fragment of rows wr 64 + li (+ 32), plane lk
    const int fb = 512 + lk * 128 + wc * 64 + li; // Phi hi fragment of points wc 64 + li (+ 32)
    const h8 *psrc_h = Ph + tile * nks * 256 + tid, *psrc_l = Pl + tile * nks * 256 + tid;
    const float un = 1.f / 32768.f; // 2^-kUExp: the tile holds 2^e T
    for (int rb = 0; rb < nrb; ++rb) {
        f32x16 acc[2][2];
        tile_product_images<false, false>(Wh + (int64_t)rb * nks * 256 + tid, Wl + (int64_t)rb * nks * 256 + tid, psrc_h, psrc_l, nks / KU, st,
                                          tid, fa, fb, acc);
        AGPL_TILE_SCATTER(E, BS, un, acc); // [row of W][point]
        __syncthreads();
        // block (tile, k-slice) = [plane][row = point][8 features]
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int g = tid + 256 * k, fg = g >> 7, pl = g & 127;
            h8 hi, lo;
#pragma unroll
            for (int j = 0; j < 8; ++j) tile_split(hi, lo, j, E[(fg * 8 + j) * BS + pl]);
            const int64_t o = (tile * nks + rb * 8 + (fg >> 1)) * 256 + (fg & 1) * 128 + pl;
            Th[o] = hi;
            Tl[o] = lo;
        }
        __syncthreads();
    }
}

// grid (b tiles, a tiles) of one (a chunk, b chunk) pair.  na, nb: the chunks' points; xa, xb, out at the chunks' first points
// (out[i ld + j]); un = 2^-2e.  sym: entry (i, j) is stored where i + goff >= j (goff = the a chunk's first point - the b chunk's),
// and where i + goff > j also at outT[j ld + i].
// LDS: the tile (over the two stage buffers) | xa [128][D] | xb [D][128], float64, x / ell (NaN for a non-finite x).
// The body, inlined into the two kernels below (which carry the __restrict__ qualifiers: restated here they would
// reach the compiler as scoped-alias metadata and reorder the existing kinds' instruction streams).  A kind whose distance is warped (agpl::kernel_warp: the periodic kinds) takes its
// parameter in float64 (`period`) and keeps the rule's constants ell_d / period | 1 / ell_d in 32 more doubles of LDS, as the
// generator does (agpl_se_build.h).
template <int KIND>
__device__ __forceinline__ void joint_cov_body(int64_t na, int64_t nb, int Mp, int D, const h8 *Pah,
                                               const h8 *Pal, const h8 *Th,
                                               const h8 *Tl, const double *xa,
                                               const double *xb, const double *ell, float s2,
                                               float kparam, double period, float un, float *out, float *outT,
                                               int64_t ld, int sym, int64_t goff) {
    constexpr bool WARPED = agpl::kernel_kind_warps(KIND);
    constexpr bool LAST = KIND == AGPL_KERNEL_SE_PERIODIC; // only the last dimension is warped: peeled out of the pair loop
    constexpr bool MOD = agpl::kernel_kind_modulated(KIND); // kappa times a factor of the last dimension's difference (agpl::kernel_modulation)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int64_t tb = blockIdx.x, ta = blockIdx.y;
    if (sym && ta * BS + (BS - 1) + goff < tb * BS) return; // wholly above the diagonal: its mirror tile stores these entries
    h8 *st = reinterpret_cast<h8 *>(smem_raw);
    float *E = reinterpret_cast<float *>(smem_raw); // [128 a points][EP]
    double *xa_s = reinterpret_cast<double *>(smem_raw + kCovTileBytes);
    double *xb_s = xa_s + BS * D;
    double *wt = xb_s + BS * D; // WARPED: [2][16]; MOD: ell_d / period of the modulated d
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int li = lane & 31, lk = lane >> 5;
    const int nks = Mp / KT;
    if constexpr (WARPED) {
        if (tid < D && agpl::kernel_dim_warped(KIND, tid, D)) {
            wt[tid] = ell[tid] / period;
            wt[16 + tid] = 1.0 / ell[tid];
        }
    }
    if constexpr (MOD) {
        if (tid < D && agpl::kernel_dim_modulated(KIND, tid, D)) wt[tid] = ell[tid] / period;
    }
    const int fa = lk * 128 + wr * 64 + li;       // Phi_a hi fragment of points wr 64 + li (+ 32), plane lk
    const int fb = 512 + lk * 128 + wc * 64 + li; // T hi fragment of points wc 64 + li (+ 32)

    for (int t = tid; t < BS * D; t += 256) {
        const int n = t / D, d = t - n * D;
        double va = 0.0, vb = 0.0;
        if (ta * BS + n < na) {
            const double xv = xa[(ta * BS + n) * D + d];
            va = fabs(xv) <= 1.79e308 ? xv / ell[d] : __builtin_nan("");
        }
        if (tb * BS + n < nb) {
            const double xv = xb[(tb * BS + n) * D + d];
            vb = fabs(xv) <= 1.79e308 ? xv / ell[d] : __builtin_nan("");
        }
        xa_s[t] = va;
        xb_s[d * BS + n] = vb;
    }
    f32x16 acc[2][2];
    tile_product_images<false, false>(Pah + ta * nks * 256 + tid, Pal + ta * nks * 256 + tid, Th + tb * nks * 256 + tid,
                                      Tl + tb * nks * 256 + tid, nks / KU, st, tid, fa, fb, acc);
    AGPL_TILE_SCATTER(E, EP, un, acc); // [a point][b point]
    __syncthreads();
    const int p = tid & 127, hh = tid >> 7;
    {
        const int64_t gj = tb * BS + p;
        const bool livej = gj < nb;
        for (int i = hh * 64; i < hh * 64 + 64; ++i) {
            const int64_t gi = ta * BS + i;
            if (gi >= na) break;
            double r2 = 0.0;
            [[maybe_unused]] double mod = 1.0;
            if constexpr (LAST) {
                const int dl = D - 1;
                for (int d = 0; d < dl; ++d) {
                    const double us = xa_s[i * D + d] - xb_s[d * BS + p];
                    r2 += us * us;
                }
                const double u = agpl::kernel_warp<KIND>(xa_s[i * D + dl] - xb_s[dl * BS + p], wt[dl], wt[16 + dl]);
                r2 += u * u;
            } else if constexpr (MOD) { // the squared exponential's sum, the last term peeled: its difference also feeds the factor.
                // The difference of (j, i) is the negative of (i, j)'s to the bit and cospi is even: the factor is symmetric to the bit
                const int dl = D - 1;
                for (int d = 0; d < dl; ++d) {
                    const double us = xa_s[i * D + d] - xb_s[d * BS + p];
                    r2 += us * us;
                }
                const double us = xa_s[i * D + dl] - xb_s[dl * BS + p];
                r2 += us * us;
                mod = agpl::kernel_modulation(us, wt[dl]);
            } else {
                for (int d = 0; d < D; ++d) {
                    const double us = xa_s[i * D + d] - xb_s[d * BS + p];
                    const double u = agpl::kernel_warp<KIND>(us, WARPED ? wt[d] : 0.0, WARPED ? wt[16 + d] : 0.0);
                    r2 += u * u;
                }
            }
            float val;
            if constexpr (MOD)
                val = E[i * EP + p] + s2 * agpl::kernel_rule<KIND, float>(r2, kparam) * (float)mod;
            else
                val = E[i * EP + p] + s2 * agpl::kernel_rule<KIND, float>(r2, kparam);
            if (sym) E[i * EP + p] = val;
            if (livej && (!sym || gi + goff >= gj)) out[gi * ld + gj] = val;
        }
    }
    if (!sym) return;
    __syncthreads();
    const int64_t gi = ta * BS + p; // the mirror: this thread's a point is the column, stores coalesced along it
    if (gi >= na) return;
    for (int j = hh * 64; j < hh * 64 + 64; ++j) {
        const int64_t gj = tb * BS + j;
        if (gj >= nb) break;
        if (gi + goff > gj) outT[gj * ld + gi] = E[p * EP + j];
    }
}

template <int KIND>
__global__ __launch_bounds__(256, 2) void joint_cov_kernel(int64_t na, int64_t nb, int Mp, int D, const h8 *__restrict__ Pah,
                                                           const h8 *__restrict__ Pal, const h8 *__restrict__ Th,
                                                           const h8 *__restrict__ Tl, const double *__restrict__ xa,
                                                           const double *__restrict__ xb, const double *__restrict__ ell, float s2,
                                                           float kparam, float un, float *__restrict__ out, float *__restrict__ outT,
                                                           int64_t ld, int sym, int64_t goff) {
    joint_cov_body<KIND>(na, nb, Mp, D, Pah, Pal, Th, Tl, xa, xb, ell, s2, kparam, 0.0, un, out, outT, ld, sym, goff);
}

// the periodic kind's: the same body, the period in float64
__global__ __launch_bounds__(256, 2) void joint_cov_periodic_kernel(int64_t na, int64_t nb, int Mp, int D, const h8 *__restrict__ Pah,
                                                                    const h8 *__restrict__ Pal, const h8 *__restrict__ Th,
                                                                    const h8 *__restrict__ Tl, const double *__restrict__ xa,
                                                                    const double *__restrict__ xb, const double *__restrict__ ell,
                                                                    float s2, double period, float un, float *__restrict__ out,
                                                                    float *__restrict__ outT, int64_t ld, int sym, int64_t goff) {
    joint_cov_body<AGPL_KERNEL_PERIODIC>(na, nb, Mp, D, Pah, Pal, Th, Tl, xa, xb, ell, s2, 0.f, period, un, out, outT, ld, sym, goff);
}

// the squared exponential x periodic kind's: the same body, the last dimension's term peeled, the period in float64
__global__ __launch_bounds__(256, 2) void joint_cov_se_periodic_kernel(int64_t na, int64_t nb, int Mp, int D, const h8 *__restrict__ Pah,
                                                                       const h8 *__restrict__ Pal, const h8 *__restrict__ Th,
                                                                       const h8 *__restrict__ Tl, const double *__restrict__ xa,
                                                                       const double *__restrict__ xb, const double *__restrict__ ell,
                                                                       float s2, double period, float un, float *__restrict__ out,
                                                                       float *__restrict__ outT, int64_t ld, int sym, int64_t goff) {
    joint_cov_body<AGPL_KERNEL_SE_PERIODIC>(na, nb, Mp, D, Pah, Pal, Th, Tl, xa, xb, ell, s2, 0.f, period, un, out, outT, ld, sym, goff);
}

// the squared exponential x cosine kind's: the squared exponential's body times the factor of the last dimension's difference, the
// period in float64
__global__ __launch_bounds__(256, 2) void joint_cov_se_cosine_kernel(int64_t na, int64_t nb, int Mp, int D, const h8 *__restrict__ Pah,
                                                                     const h8 *__restrict__ Pal, const h8 *__restrict__ Th,
                                                                     const h8 *__restrict__ Tl, const double *__restrict__ xa,
                                                                     const double *__restrict__ xb, const double *__restrict__ ell,
                                                                     float s2, double period, float un, float *__restrict__ out,
                                                                     float *__restrict__ outT, int64_t ld, int sym, int64_t goff) {
    joint_cov_body<AGPL_KERNEL_SE_COSINE>(na, nb, Mp, D, Pah, Pal, Th, Tl, xa, xb, ell, s2, 0.f, period, un, out, outT, ld, sym, goff);
}

size_t joint_cov_lds(const agpl_plan *p) {
    return (size_t)kCovTileBytes + sizeof(double) * 2 * BS * (size_t)p->D + (agpl::kernel_kind_warps(p->kind) || agpl::kernel_kind_modulated(p->kind) ? 32 * sizeof(double) : 0);
}

// once per call: the dynamic LDS the plan's instantiation of joint_cov_kernel will be launched with
int32_t joint_prepare_cov(agpl_ctx *ctx, const agpl_plan *p) {
    const void *fn = nullptr;
    switch (p->kind) {
    case AGPL_KERNEL_SE: fn = reinterpret_cast<const void *>(&joint_cov_kernel<AGPL_KERNEL_SE>); break;
    case AGPL_KERNEL_MATERN12: fn = reinterpret_cast<const void *>(&joint_cov_kernel<AGPL_KERNEL_MATERN12>); break;
    case AGPL_KERNEL_MATERN32: fn = reinterpret_cast<const void *>(&joint_cov_kernel<AGPL_KERNEL_MATERN32>); break;
    case AGPL_KERNEL_MATERN52: fn = reinterpret_cast<const void *>(&joint_cov_kernel<AGPL_KERNEL_MATERN52>); break;
    case AGPL_KERNEL_RQ: fn = reinterpret_cast<const void *>(&joint_cov_kernel<AGPL_KERNEL_RQ>); break;
    case AGPL_KERNEL_PERIODIC: fn = reinterpret_cast<const void *>(&joint_cov_periodic_kernel); break;
    case AGPL_KERNEL_SE_PERIODIC: fn = reinterpret_cast<const void *>(&joint_cov_se_periodic_kernel); break;
    case AGPL_KERNEL_SE_COSINE: fn = reinterpret_cast<const void *>(&joint_cov_se_cosine_kernel); break;
    default: AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "predict_cov: unknown kernel kind %d", p->kind);
    }
    AGPL_HIP(ctx, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)joint_cov_lds(p)));
    return AGPL_OK;
}

int32_t joint_launch_cov(agpl_ctx *ctx, const agpl_plan *p, int64_t na, int64_t nb, const h8 *Pah, const h8 *Pal, const h8 *Th,
                         const h8 *Tl, const double *xa, const double *xb, float *out, float *outT, int64_t ld, int sym, int64_t goff) {
    const size_t lds = joint_cov_lds(p);
    const dim3 grid((unsigned)agpl_cdiv(nb, BS), (unsigned)agpl_cdiv(na, BS));
    const float un = ldexpf(1.f, -2 * p->scale_exp);
    switch (p->kind) { // the one dispatch on the kind, as the generator's
#define AGPL_JT_KIND_(K)                                                                                                           \
    case K:                                                                                                                        \
        joint_cov_kernel<K><<<grid, 256, lds, ctx->stream>>>(na, nb, p->M, p->D, Pah, Pal, Th, Tl, xa, xb, p->ell, (float)p->s2,   \
                                                             (float)p->kparam, un, out, outT, ld, sym, goff);                     \
        break;
        AGPL_JT_KIND_(AGPL_KERNEL_SE)
        AGPL_JT_KIND_(AGPL_KERNEL_MATERN12)
        AGPL_JT_KIND_(AGPL_KERNEL_MATERN32)
        AGPL_JT_KIND_(AGPL_KERNEL_MATERN52)
        AGPL_JT_KIND_(AGPL_KERNEL_RQ)
#undef AGPL_JT_KIND_
    case AGPL_KERNEL_PERIODIC:
        joint_cov_periodic_kernel<<<grid, 256, lds, ctx->stream>>>(na, nb, p->M, p->D, Pah, Pal, Th, Tl, xa, xb, p->ell, (float)p->s2,
                                                                   p->kparam, un, out, outT, ld, sym, goff);
        break;
    case AGPL_KERNEL_SE_PERIODIC:
        joint_cov_se_periodic_kernel<<<grid, 256, lds, ctx->stream>>>(na, nb, p->M, p->D, Pah, Pal, Th, Tl, xa, xb, p->ell, (float)p->s2,
                                                                      p->kparam, un, out, outT, ld, sym, goff);
        break;
    case AGPL_KERNEL_SE_COSINE:
        joint_cov_se_cosine_kernel<<<grid, 256, lds, ctx->stream>>>(na, nb, p->M, p->D, Pah, Pal, Th, Tl, xa, xb, p->ell, (float)p->s2,
                                                                    p->kparam, un, out, outT, ld, sym, goff);
        break;
    default: AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "predict_cov: unknown kernel kind %d", p->kind);
    }
    AGPL_LAUNCH_CHECK(ctx);
    return AGPL_OK;
}

} // namespace

extern "C" int32_t agpl_plan_predict_cov(agpl_plan *p, int64_t Na, const double *x_a, int64_t Nb, const double *x_b, float *cov_out,
                                         int64_t ld) {
    if (!p || !p->ctx) return AGPL_ERR_INVALID_ARGUMENT;
    agpl_ctx *ctx = p->ctx;
    if (p->flags & AGPL_PLAN_NO_MARGINALS)
        AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "this plan was created without the marginal image (AGPL_PLAN_NO_MARGINALS)");
    if (!p->se) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "agpl_plan_predict_cov needs a plan made from raw inputs (agpl_plan_create_se)");
    if (Na < 0 || Nb < 0) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "Na = %lld, Nb = %lld: negative", (long long)Na, (long long)Nb);
    const int sym = x_b == nullptr;
    if (sym && Nb != Na)
        AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "x_b = NULL (the symmetric form) needs Nb = Na (got %lld, %lld)", (long long)Nb,
                  (long long)Na);
    if (ld < Nb) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "ld = %lld < Nb = %lld", (long long)ld, (long long)Nb);
    if (Na == 0 || Nb == 0) return AGPL_OK;
    if (!x_a || !cov_out) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "null argument");
    if (sym) x_b = x_a;
    const int L = p->L, M = p->M, D = p->D;
    const int64_t Ca = Na < kJointChunk ? Na : kJointChunk, Cb = Nb < kJointChunk ? Nb : kJointChunk;
    const bool own_a = !(sym && Na <= kJointChunk); // one symmetric chunk: Phi_a is Phi_b
    const auto al = agpl_align256;
    const size_t imga = own_a ? al((size_t)agpl_split_features_bytes(Ca, M)) : 0; // one plane of a chunk's image
    const size_t imgb = al((size_t)agpl_split_features_bytes(Cb, M));
    const size_t rsb = al(sizeof(float) * (size_t)(Ca > Cb ? Ca : Cb));
    const size_t wimg = al(sizeof(_Float16) * (size_t)L * M * M); // one plane of the W images
    const size_t need = 2 * imga + 4 * imgb + rsb + 2 * wimg + 256;
    if (int32_t rc_ = agpl_pred_reserve(p, need, "prediction")) return rc_; // (every call carves the scratch anew)
    char *w = (char *)p->pred;
    h8 *Pbh = (h8 *)w, *Pbl = (h8 *)(w + imgb), *Th = (h8 *)(w + 2 * imgb), *Tl = (h8 *)(w + 3 * imgb);
    h8 *Pah = own_a ? (h8 *)(w + 4 * imgb) : Pbh, *Pal = own_a ? (h8 *)(w + 4 * imgb + imga) : Pbl;
    float *rs = (float *)(w + 4 * imgb + 2 * imga);
    h8 *Wh = (h8 *)(w + 4 * imgb + 2 * imga + rsb), *Wl = (h8 *)(w + 4 * imgb + 2 * imga + rsb + wimg);
    unsigned long long *words = (unsigned long long *)(w + 4 * imgb + 2 * imga + rsb + 2 * wimg); // the generator's status words
    unsigned *maxbits = (unsigned *)(words + 8);                                                   // (not reported: NaN outputs)

    joint_w_kernel<<<dim3((unsigned)(M / KT), (unsigned)(M / BS), (unsigned)L), 256, 0, ctx->stream>>>(p->Mc, M, p->A_work, Wh, Wl);
    AGPL_LAUNCH_CHECK(ctx);
    AGPL_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&joint_t_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      kStageBytes));
    const int64_t wstride = (int64_t)M * M / 8; // h8 per latent and plane
    int32_t rc = joint_prepare_cov(ctx, p);
    if (rc) return rc;
    for (int64_t b0 = 0; b0 < Nb; b0 += Cb) {
        const int64_t nb = Nb - b0 < Cb ? Nb - b0 : Cb;
        rc = agpl_se_build(ctx, p->kind, p->kparam, nb, M, p->Mc, D, x_b + b0 * D, p->zs, p->ell, p->s2, p->Lt, p->scale_exp, Pbh, Pbl,
                           nullptr, rs, maxbits, words);
        if (rc) return rc;
        for (int64_t a0 = sym ? b0 : 0; a0 < Na; a0 += Ca) { // symmetric form: the chunk pairs on and below the diagonal
            const int64_t na = Na - a0 < Ca ? Na - a0 : Ca;
            const bool shared = sym && a0 == b0;
            if (!shared) {
                rc = agpl_se_build(ctx, p->kind, p->kparam, na, M, p->Mc, D, x_a + a0 * D, p->zs, p->ell, p->s2, p->Lt, p->scale_exp, Pah,
                                   Pal, nullptr, rs, maxbits, words);
                if (rc) return rc;
            }
            for (int l = 0; l < L; ++l) {
                joint_t_kernel<<<(unsigned)agpl_cdiv(nb, BS), 256, kStageBytes, ctx->stream>>>(M, Pbh, Pbl, Wh + l * wstride,
                                                                                               Wl + l * wstride, Th, Tl);
                AGPL_LAUNCH_CHECK(ctx);
                float *base = cov_out + (int64_t)l * Na * ld;
                rc = joint_launch_cov(ctx, p, na, nb, shared ? Pbh : Pah, shared ? Pbl : Pal, Th, Tl, x_a + a0 * D, x_b + b0 * D,
                                      base + a0 * ld + b0, base + b0 * ld + a0, ld, sym, a0 - b0);
                if (rc) return rc;
            }
        }
    }
    return AGPL_OK;
}
