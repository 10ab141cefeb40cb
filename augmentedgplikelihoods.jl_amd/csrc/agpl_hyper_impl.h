// agpl_hyper_impl.h -- the gradients of the sweep's bound at a plan's q(v), stated once for the two libraries that export them:
//   libagpl_hyper.so (agpl_hyper.hip: agpl_plan_hyper_grad, include/agpl_hyper.h)  log lengthscales and log variance, D + 1 numbers
//   libagpl_zgrad.so (agpl_zgrad.hip: agpl_plan_inducing_grad, include/agpl_zgrad.h)  the inducing inputs, [Mc][D], and the D + 1 too
// Each includes this header and instantiates hy_grad<ZG> once (ZG: the inducing-input gradient is formed as well).
//
//   float64, M x M, once per call (row-major [a][b] at the caller's feature count Mc):
//     hy_lower_kernel     the column-major lower triangle a factor route leaves (L^-1 from K_ZZ; the plan's U) -> row-major, upper zero
//     hy_gemm_kernel      C = alpha op(A) op(B) + beta C through 16 x 16 LDS tiles (k ascending: fixed order)
//     hy_w_kernel         S -> Q = I - S (in place) and W = I - S - m m'
//     hy_max_kernel / hy_pack_kernel   C_l = L^-T W_l as a split-float16 image (agpl_chain.hip's V image: row block of 128, k-slice
//                         of 16 = [plane 2][row 128][8 halves]) at 2^ec, 2^ec max |C_l| in [2^13, 2^14); unscale[l] = 2^-(e_phi + ec)
//     hy_t_kernel, hy_rank1_kernel, hy_tril_kernel, hy_kt_kernel, hy_sym_kernel, hy_kzz_grad_kernel   the K_ZZ part
//     hy_kzz_zgrad_kernel (ZG)   the K_ZZ part of the inducing-input gradient: one workgroup per row a of Kbar
//   per chunk of 65536 points (the plan's generator writes the chunk's marginal image, agpl_se_build.h):
//     hy_points_kernel    one 128-point tile per workgroup (4 waves, 64 rows x 64 points each); per latent and per 128-row block of
//                         C_l the product R = C_l Phi (the tile product of agpl_tile_product.h), through LDS once as [row][point], then one
//                         thread per point and half block contracts it with kappa and kappa'/r generated on the fly: D + 1 float64
//                         sums per thread, reduced over the workgroup in thread order -> part[tile][D + 1].  R is never stored.
//                         ZG: the contraction leaves cq = -w variance kappa'/r (float32) in the [row][point] slot it read, and a
//                         second phase, one thread per (row, half of the points), sums cq (xs - zs) over the tile's points in
//                         float64 -> part_z[tile][Mc][D] (scaled coordinates).
//     hy_h_kernel         h_l = sum_i gamma_li mu0_li phi_i from the same image (mu0 given only): float64, tile groups in a fixed order
//     hy_reduce_kernel    grad += the chunk's partial sums, tiles ascending (one thread per component)
//     hy_zreduce_kernel (ZG)   accz[a][d] += part_z[tile][a][d], tiles ascending (one thread per component), after every group of
//                         tiles whose part_z fits kZPartBudget
//     hy_zfinal_kernel (ZG)    grad_z[a][d] = (accz + the K_ZZ part) / ell_d: scaled coordinates -> the caller's units
// No float atomics; no sum depends on the launch.
#pragma once
#include "../../include/agpl_hyper.h"
#include "agpl_se_create.h"
#include "agpl_tile_product.h"

namespace {

static_assert(256 * 17 * 8 <= kStageBytes, "the workgroup reduction reuses the two stage buffers");
constexpr int64_t kHyperChunk = 1 << 16; // points per step (agpl_plan_predict's chunk)
constexpr int kHGroups = 8;              // tile groups of hy_h_kernel

// out[a][b] (row-major, n x n) = F[b ld + a] for a >= b, else 0
__global__ __launch_bounds__(256) void hy_lower_kernel(int n, int ld, const double *__restrict__ F, double *__restrict__ out) {
    const int64_t total = (int64_t)n * n;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int a = (int)(t / n), b = (int)(t - (int64_t)a * n);
        out[t] = a >= b ? F[(int64_t)b * ld + a] : 0.0;
    }
}

// Kt[a][b] = Gk[a Mp + b] + (a == b): K_ZZ + jitter I from se_kzz_kernel's K_ZZ + (jitter - 1) I
__global__ __launch_bounds__(256) void hy_kt_kernel(int n, int Mp, const double *__restrict__ Gk, double *__restrict__ Kt) {
    const int64_t total = (int64_t)n * n;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int a = (int)(t / n), b = (int)(t - (int64_t)a * n);
        Kt[t] = Gk[(int64_t)a * Mp + b] + (a == b ? 1.0 : 0.0);
    }
}

// C [m x n] = alpha op(A) op(B) + beta C, row-major; op(A)[i][k] = ta ? A[k lda + i] : A[i lda + k], op(B)[k][j] likewise
__global__ __launch_bounds__(256) void hy_gemm_kernel(int m, int n, int k, const double *__restrict__ A, int lda, int ta,
                                                      const double *__restrict__ B, int ldb, int tb, double *__restrict__ Cm, int ldc,
                                                      double alpha, double beta) {
    __shared__ double As[16][17], Bs[16][17];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int i = blockIdx.y * 16 + ty, j = blockIdx.x * 16 + tx;
    double s = 0.0;
    for (int k0 = 0; k0 < k; k0 += 16) {
        {
            const int ai = blockIdx.y * 16 + ty, ak = k0 + tx;
            As[ty][tx] = (ai < m && ak < k) ? (ta ? A[(int64_t)ak * lda + ai] : A[(int64_t)ai * lda + ak]) : 0.0;
            const int bk = k0 + ty, bj = blockIdx.x * 16 + tx;
            Bs[ty][tx] = (bk < k && bj < n) ? (tb ? B[(int64_t)bj * ldb + bk] : B[(int64_t)bk * ldb + bj]) : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) s += As[ty][kk] * Bs[kk][tx];
        __syncthreads();
    }
    if (i < m && j < n) {
        double *c = Cm + (int64_t)i * ldc + j;
        *c = beta == 0.0 ? alpha * s : alpha * s + beta * *c;
    }
}

// S -> Q = I - S (in place); W = I - S - m m'
__global__ __launch_bounds__(256) void hy_w_kernel(int n, double *__restrict__ S, const double *__restrict__ m, double *__restrict__ W) {
    const int64_t total = (int64_t)n * n;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int a = (int)(t / n), b = (int)(t - (int64_t)a * n);
        const double q = (a == b ? 1.0 : 0.0) - S[t];
        S[t] = q;
        W[t] = q - m[a] * m[b];
    }
}

// word <- max |Cm| (bit patterns of non-negative doubles order as the values; NaNs are skipped)
__global__ __launch_bounds__(256) void hy_max_kernel(int64_t total, const double *__restrict__ Cm, unsigned long long *__restrict__ word) {
    double mx = 0.0;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const double c = fabs(Cm[t]);
        mx = c > mx ? c : mx;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ot = __shfl_xor(mx, o);
        mx = ot > mx ? ot : mx;
    }
    if ((threadIdx.x & 63) == 0 && mx > 0.0) atomicMax(word, (unsigned long long)__double_as_longlong(mx));
}

// grid (Mp / 16 k-slices, Mp / 128 row blocks): the image of one latent's C (Mc x Mc row-major; zero beyond Mc); *unscale = 2^-(e_phi + ec)
__global__ __launch_bounds__(256) void hy_pack_kernel(int Mc, int Mp, const double *__restrict__ Cm,
                                                      const unsigned long long *__restrict__ word, int e_phi, h8 *__restrict__ Ch,
                                                      h8 *__restrict__ Cl, float *__restrict__ unscale) {
    const int nks = Mp / KT;
    const int ks = blockIdx.x, rb = blockIdx.y;
    const int plane = threadIdx.x >> 7, row = threadIdx.x & 127;
    const int ec = tile_scale_exp(__longlong_as_double((long long)*word));
    if (ks == 0 && rb == 0 && threadIdx.x == 0) *unscale = ldexpf(1.f, -(e_phi + ec));
    const double sc = ldexp(1.0, ec);
    const int a = rb * BS + row;
    h8 hi, lo;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int b = ks * KT + plane * 8 + j;
        const double x = (a < Mc && b < Mc) ? Cm[(int64_t)a * Mc + b] * sc : 0.0;
        tile_split(hi, lo, j, (float)x);
    }
    const int64_t o = ((int64_t)rb * nks + ks) * 256 + threadIdx.x;
    Ch[o] = hi;
    Cl[o] = lo;
}

// t[b] = (g[b] - Gm[b], when the naturals are given) - (h[b], when mu0 is given)
__global__ __launch_bounds__(256) void hy_t_kernel(int n, const double *__restrict__ g, const double *__restrict__ Gm,
                                                   const double *__restrict__ h, double *__restrict__ t) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n) return;
    double v = 0.0;
    if (g) v = g[b] - Gm[b];
    if (h) v -= h[b];
    t[b] = v;
}

// A[a][b] += m[a] t[b]
__global__ __launch_bounds__(256) void hy_rank1_kernel(int n, const double *__restrict__ m, const double *__restrict__ t, double *__restrict__ A) {
    const int64_t total = (int64_t)n * n;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int a = (int)(e / n), b = (int)(e - (int64_t)a * n);
        A[e] += m[a] * t[b];
    }
}

// B -> -tril(B) (mode 0: Lbar);  X -> its lower triangle with the diagonal halved (mode 1: the Phi of the Cholesky reverse rule)
__global__ __launch_bounds__(256) void hy_tril_kernel(int n, int mode, double *__restrict__ B) {
    const int64_t total = (int64_t)n * n;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int a = (int)(e / n), b = (int)(e - (int64_t)a * n);
        const double v = B[e];
        B[e] = a < b ? 0.0 : (mode == 0 ? -v : (a == b ? 0.5 * v : v));
    }
}

// out = (Kb + Kb') / 2
__global__ __launch_bounds__(256) void hy_sym_kernel(int n, const double *__restrict__ Kb, double *__restrict__ out) {
    const int64_t total = (int64_t)n * n;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int a = (int)(e / n), b = (int)(e - (int64_t)a * n);
        out[e] = 0.5 * (Kb[e] + Kb[(int64_t)b * n + a]);
    }
}

// block j (j < D: log ell_j, j == D: log variance): grad[j] += sum_ab Kbar_ab dK_ab / dtheta_j; pairs strided over the 256 threads,
// then a fixed tree over the threads.  The diagonal (r = 0) carries no lengthscale term and the variance term s2 (no jitter).
// ell: the plan's lengthscales, read by the distance rule of a warped kind only (agpl::kernel_warp_value).
__global__ __launch_bounds__(256) void hy_kzz_grad_kernel(int kind, double kparam, int n, int D, const double *__restrict__ zs,
                                                          const double *__restrict__ ell, double s2,
                                                          const double *__restrict__ Kbar, double *__restrict__ grad) {
    __shared__ double red[256];
    const int j = blockIdx.x;
    const int64_t total = (int64_t)n * n;
    double s = 0.0;
    for (int64_t e = threadIdx.x; e < total; e += 256) {
        const int a = (int)(e / n), b = (int)(e - (int64_t)a * n);
        double r2 = 0.0, uj = 0.0, mod = 1.0;
        for (int d = 0; d < D; ++d) {
            const double us = zs[(int64_t)a * D + d] - zs[(int64_t)b * D + d];
            const double u = agpl::kernel_warp_value(kind, d, D, us, ell[d], kparam);
            r2 += u * u;
            if (d == j) uj = u * u;
            if (agpl::kernel_dim_modulated(kind, d, D)) mod = agpl::kernel_modulation(us, ell[d] / kparam);
        }
        double dk = j == D ? s2 * agpl::kernel_value<double>(kind, r2, kparam)
                           : (a == b ? 0.0 : -s2 * agpl::kernel_dvalue<double>(kind, r2, kparam) * uj);
        if (agpl::kernel_kind_modulated(kind)) dk *= mod; // (the factor does not depend on ell or the variance: both derivatives carry it)
        s += Kbar[e] * dk;
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) grad[j] += red[0];
}

// grid (Mp / 16 k-slices, kHGroups tile groups, L): hp[group][l][a] = 2^-e sum over the group's tiles and their points of
// gamma mu0 phi_a, from the chunk's marginal image (block (tile, k-slice) = [plane 2][point 128][8 features])
__global__ __launch_bounds__(256) void hy_h_kernel(int64_t n, int64_t pitch, int Mp, int L, const h8 *__restrict__ Ph,
                                                   const h8 *__restrict__ Pl, float unphi, const float *__restrict__ mu0,
                                                   const float *__restrict__ gamma, double *__restrict__ hp) {
    __shared__ double red[256][9];
    const int nks = Mp / KT;
    const int ks = blockIdx.x, grp = blockIdx.y, l = blockIdx.z;
    const int pt = threadIdx.x & 127; // (thread = (plane, point), the image's order)
    const int64_t ntile = (n + BS - 1) / BS, per = (ntile + kHGroups - 1) / kHGroups;
    const int64_t t0 = grp * per, t1 = t0 + per < ntile ? t0 + per : ntile;
    double acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.0;
    for (int64_t tile = t0; tile < t1; ++tile) {
        const int64_t np = tile * BS + pt;
        if (np >= n) continue;
        const double w = (double)gamma[(int64_t)l * pitch + np] * (double)mu0[(int64_t)l * pitch + np];
        const int64_t o = (tile * nks + ks) * 256 + threadIdx.x;
        const h8 hi = Ph[o], lo = Pl[o];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += w * ((double)(float)hi[j] + (double)(float)lo[j]);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) red[threadIdx.x][j] = acc[j];
    __syncthreads();
    if (threadIdx.x < 16) {
        const int pl = threadIdx.x >> 3, j = threadIdx.x & 7;
        double s = 0.0;
        for (int q = 0; q < 128; ++q) s += red[pl * 128 + q][j];
        hp[((int64_t)grp * L + l) * Mp + ks * KT + pl * 8 + j] = s * (double)unphi;
    }
}

// h[l][a] += the groups of hp in ascending order
__global__ __launch_bounds__(256) void hy_hsum_kernel(int64_t LM, const double *__restrict__ hp, double *__restrict__ h) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= LM) return;
    double s = h[i];
    for (int gI = 0; gI < kHGroups; ++gI) s += hp[(int64_t)gI * LM + i];
    h[i] = s;
}

// grad[j] += part[tile][j], tiles ascending
__global__ void hy_reduce_kernel(int64_t ntile, int D1, const double *__restrict__ part, double *__restrict__ grad) {
    const int j = threadIdx.x;
    if (j >= D1 || blockIdx.x != 0) return;
    double s = grad[j];
    for (int64_t t = 0; t < ntile; ++t) s += part[t * D1 + j];
    grad[j] = s;
}

// accz[e] += part_z[tile][e], tiles ascending; e = a D + d (one thread per component)
__global__ __launch_bounds__(256) void hy_zreduce_kernel(int64_t ntile, int64_t MD, const double *__restrict__ part_z,
                                                         double *__restrict__ accz) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= MD) return;
    double s = accz[e];
    for (int64_t t = 0; t < ntile; ++t) s += part_z[t * MD + e];
    accz[e] = s;
}

// block a: gk[a][d] = 2 sum_{b != a} Kbar_ab s2 (kappa'(r_ab) / r_ab) u_d u'_d, the K_ZZ part of dLb / d(z_ad / ell_d), with u_d the
// distance rule's term of r^2 and u'_d its derivative for the scaled difference (agpl_kernel_rules.h; zs_ad - zs_bd and 1 for the unwarped kinds): the
// columns b strided over the 256 threads, then a fixed tree over the threads.  The diagonal of K_ZZ does not depend on z.
__global__ __launch_bounds__(256) void hy_kzz_zgrad_kernel(int kind, double kparam, int n, int D, const double *__restrict__ zs,
                                                           const double *__restrict__ ell, double s2,
                                                           const double *__restrict__ Kbar, double *__restrict__ gk) {
    __shared__ double red[256];
    const int a = blockIdx.x;
    double acc[16];
#pragma unroll
    for (int d = 0; d < 16; ++d) acc[d] = 0.0;
    for (int b = threadIdx.x; b < n; b += 256) {
        if (b == a) continue;
        double u[16], r2 = 0.0; // u[d]: u_d for r^2, then u_d u'_d
        double mod = 1.0, dmod = 0.0; // a modulated kind's factor and its derivative for the scaled difference (else 1, 0)
#pragma unroll
        for (int d = 0; d < 16; ++d) {
            u[d] = 0.0;
            if (d < D) {
                const double us = zs[(int64_t)a * D + d] - zs[(int64_t)b * D + d];
                const double w = agpl::kernel_warp_value(kind, d, D, us, ell[d], kparam);
                r2 += w * w;
                u[d] = w * agpl::kernel_dwarp_value(kind, d, D, us, ell[d], kparam);
                if (agpl::kernel_dim_modulated(kind, d, D)) {
                    mod = agpl::kernel_modulation(us, ell[d] / kparam);
                    dmod = agpl::kernel_dmodulation(us, ell[d] / kparam);
                }
            }
        }
        if (agpl::kernel_kind_modulated(kind)) { // d (kappa m) / d zs_ad over kappa' / r: u_d m, and u_d m - m' in the modulated dimension
#pragma unroll
            for (int d = 0; d < 16; ++d)
                if (d < D) u[d] = agpl::kernel_dim_modulated(kind, d, D) ? u[d] * mod - dmod : u[d] * mod;
        }
        const double c = Kbar[(int64_t)a * n + b] * s2 * agpl::kernel_dvalue<double>(kind, r2, kparam);
#pragma unroll
        for (int d = 0; d < 16; ++d) acc[d] += c * u[d];
    }
#pragma unroll
    for (int d = 0; d < 16; ++d) {
        if (d < D) { // (uniform over the workgroup)
            __syncthreads();
            red[threadIdx.x] = acc[d];
            __syncthreads();
            for (int o = 128; o > 0; o >>= 1) {
                if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
                __syncthreads();
            }
            if (threadIdx.x == 0) gk[(int64_t)a * D + d] = 2.0 * red[0];
        }
    }
}

// out[a][d] = (accz[a][d] + gk[a][d]) / ell[d] (gk: NULL without the K_ZZ part): from the plan's scaled z / ell to the caller's z
__global__ __launch_bounds__(256) void hy_zfinal_kernel(int64_t MD, int D, const double *__restrict__ accz, const double *__restrict__ gk,
                                                        const double *__restrict__ ell, double *__restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= MD) return;
    const double s = gk ? accz[e] + gk[e] : accz[e];
    out[e] = s / ell[e % D];
}

// n: the chunk's points; pitch: N (mu0, beta, gamma point at the chunk's first point); x: the chunk's inputs.
// LDS: two stage buffers (reused by the epilogue tile and the final reduction) | xs [D][128] float64.
// DT: a compile-time bound of D (1, 4 or 16): the D + 1 sums of a thread stay in registers.
// ZG: also part_z[tile][Mc][D] = sum over the tile's points (and the latents) of cq_ai (xs_id - zs_ad), cq = -w variance kappa'/r:
// the tile's share of dLb / d(z_ad / ell_d) (include/agpl_zgrad.h).  The contraction and its D + 1 sums are the same code either way.
// A warped kind (the periodic kinds) replaces xs_id - zs_ad by the rule's u_d in r^2 and by u_d u'_d in part_z, in the dimensions it
// warps (agpl::kernel_warp_dim); it reads
// the rule's constants in float64 from the plan's lengthscale block, ell[16 + d] = ell_d / period (agpl_plan_impl.h), not from kparam.
template <int KIND, int DT, bool ZG>
__global__ __launch_bounds__(256) void hy_points_kernel(int64_t n, int64_t pitch, int Mp, int Mc, int D, int L,
                                                        const h8 *__restrict__ Ph, const h8 *__restrict__ Pl,
                                                        const h8 *__restrict__ Ch, const h8 *__restrict__ Cl,
                                                        const float *__restrict__ unscale, const double *__restrict__ pv,
                                                        const double *__restrict__ x, const double *__restrict__ zs,
                                                        const double *__restrict__ ell, float s2, float kparam,
                                                        const float *__restrict__ mu0, const float *__restrict__ beta,
                                                        const float *__restrict__ gamma, double *__restrict__ part,
                                                        double *__restrict__ part_z) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    h8 *st = reinterpret_cast<h8 *>(smem_raw);       // [2][kStageH8]
    float *E = reinterpret_cast<float *>(smem_raw);   // [128 rows][128 points]
    double *red = reinterpret_cast<double *>(smem_raw); // [D + 1][256]
    double *xs = reinterpret_cast<double *>(smem_raw + kStageBytes); // [D][128]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int li = lane & 31, lk = lane >> 5;
    const int nks = Mp / KT;
    const int nst = ((Mc + KT - 1) / KT + KU - 1) / KU; // stages that carry anything: C_l and Phi are zero from feature Mc on
    const int nrb = (Mc + BS - 1) / BS; // row blocks of C that carry anything
    const int64_t tile = blockIdx.x;
    const int p = tid & 127, hh = tid >> 7; // epilogue: this thread's point and half block
    const int64_t np = tile * BS + p;
    const bool livep = np < n;
    const h8 *psrc_h = Ph + tile * nks * 256 + tid, *psrc_l = Pl + tile * nks * 256 + tid;
    const int fa = lk * 128 + wr * 64 + li;       // C hi fragment of rows wr 64 + li (+ 32), plane lk
    const int fb = 512 + lk * 128 + wc * 64 + li; // Phi hi fragment of points wc 64 + li (+ 32)

    for (int t = tid; t < BS * D; t += 256) {
        const int q = t / D, d = t - q * D;
        xs[d * BS + q] = tile * BS + q < n ? x[(tile * BS + q) * D + d] / ell[d] : 0.0;
    }

    double accd[DT], accv = 0.0;
#pragma unroll
    for (int d = 0; d < DT; ++d) accd[d] = 0.0;
    double wd[DT], il[DT]; // the distance rule's constants (the dimensions the kind warps only)
#pragma unroll
    for (int d = 0; d < DT; ++d) {
        const bool warped = d < D && agpl::kernel_dim_warped(KIND, d, D);
        wd[d] = warped ? ell[16 + d] : 0.0;
        il[d] = warped ? 1.0 / ell[d] : 0.0;
    }
    // A modulated kind (agpl::kernel_dim_modulated: the last dimension of the squared exponential x cosine kind): k = s2 kappa m, with the
    // factor m of the last dimension's scaled difference and its constant ell[16 + D - 1] = ell / period.  d k / d log ell_d = u_d^2 k in
    // every dimension (m does not depend on ell); d k / d zs_ad = s2 kappa u_d m, and s2 kappa (u_d m - m') in the modulated dimension:
    // the second phase gets cq without the factor and forms m and m' per (inducing input, point) itself.
    constexpr bool MOD = agpl::kernel_kind_modulated(KIND);
    [[maybe_unused]] const double wl = MOD ? ell[16 + D - 1] : 0.0;

    for (int l = 0; l < L; ++l) {
        double gd = 0.0, bd = 0.0;
        if (livep) {
            gd = (double)gamma[(int64_t)l * pitch + np];
            bd = (double)beta[(int64_t)l * pitch + np];
            if (mu0) bd -= gd * (double)mu0[(int64_t)l * pitch + np];
            if (hh == 0) accv -= 0.5 * gd * (double)s2;
        }
        const float un = unscale[l];
        const double *pl_ = pv + (int64_t)l * Mp;
        for (int rb = 0; rb < nrb; ++rb) {
            const int64_t cb = ((int64_t)l * (Mp / BS) + rb) * nks * 256 + tid;
            f32x16 acc[2][2];
            // (the barrier before the first store: the epilogue of the block before, and the xs fill, are done with LDS)
            tile_product_images<false, true>(Ch + cb, Cl + cb, psrc_h, psrc_l, nst, st, tid, fa, fb, acc);
            AGPL_TILE_SCATTER(E, BS, un, acc); // as [row][point]
            __syncthreads();
            // the contraction: rows a0 .. a0 + cnt - 1 of this half block against the kernel's derivative at (x_p, z_a)
            const int a0 = rb * BS + hh * 64;
            const int cnt = Mc - a0 < 64 ? (Mc - a0 < 0 ? 0 : Mc - a0) : 64;
            for (int i = 0; i < cnt; ++i) {
                const int a = a0 + i;
                const double w = gd * (double)E[(hh * 64 + i) * BS + p] + bd * pl_[a];
                double u2[DT], r2 = 0.0;
#pragma unroll
                for (int d = 0; d < DT; ++d) {
                    u2[d] = 0.0;
                    if (d < D) {
                        const double u = agpl::kernel_warp_dim<KIND>(d, D, xs[d * BS + p] - zs[(int64_t)a * D + d], wd[d], il[d]);
                        u2[d] = u * u;
                        r2 += u2[d];
                    }
                }
                const float kf = s2 * agpl::kernel_rule<KIND, float>(r2, kparam);
                const float qf = s2 * agpl::kernel_drule<KIND, float>(r2, kparam);
                [[maybe_unused]] double mod = 1.0;
                if constexpr (MOD) {
                    mod = agpl::kernel_modulation(xs[(D - 1) * BS + p] - zs[(int64_t)a * D + (D - 1)], wl);
                    accv += w * (double)kf * mod;
                } else {
                    accv += w * (double)kf;
                }
                const double cq = -w * (double)qf;
                if constexpr (MOD) {
                    const double cqm = cq * mod;
#pragma unroll
                    for (int d = 0; d < DT; ++d) accd[d] += cqm * u2[d];
                } else {
#pragma unroll
                    for (int d = 0; d < DT; ++d) accd[d] += cq * u2[d];
                }
                if constexpr (ZG) E[(hh * 64 + i) * BS + p] = (float)cq; // (the slot this thread just read; nobody else's)
            }
            if constexpr (ZG) {
                // second phase, transposed ownership: thread = (row zr_, half zh of the points).  The points are walked rotated by
                // row + 32 zh, so that the 64 lanes of a wave read 64 different LDS banks (rows are 128 floats apart).
                __syncthreads();
                const int zr_ = tid >> 1, zh = tid & 1;
                const int a = rb * BS + zr_;
                double za[DT], sz[DT];
#pragma unroll
                for (int d = 0; d < DT; ++d) {
                    za[d] = (d < D && a < Mc) ? zs[(int64_t)a * D + d] : 0.0;
                    sz[d] = 0.0;
                }
                if (a < Mc) {
                    [[maybe_unused]] const double zl = MOD ? zs[(int64_t)a * D + (D - 1)] : 0.0;
                    for (int j = 0; j < 64; ++j) {
                        const int q = zh * 64 + ((j + zr_ + 32 * zh) & 63);
                        const double c = (double)E[zr_ * BS + q];
                        if constexpr (MOD) {
                            const double ul = xs[(D - 1) * BS + q] - zl;
                            const double mod = agpl::kernel_modulation(ul, wl), dmod = agpl::kernel_dmodulation(ul, wl);
#pragma unroll
                            for (int d = 0; d < DT; ++d)
                                if (d < D) {
                                    const double us = xs[d * BS + q] - za[d];
                                    sz[d] += c * (agpl::kernel_dim_modulated(KIND, d, D) ? us * mod - dmod : us * mod);
                                }
                            continue;
                        }
#pragma unroll
                        for (int d = 0; d < DT; ++d)
                            if (d < D) {
                                const double us = xs[d * BS + q] - za[d];
                                sz[d] += c * (agpl::kernel_warp_dim<KIND>(d, D, us, wd[d], il[d]) * agpl::kernel_dwarp_dim<KIND>(d, D, us, wd[d], il[d]));
                            }
                    }
                }
#pragma unroll
                for (int d = 0; d < DT; ++d) sz[d] += __shfl_xor(sz[d], 1); // (half 0 + half 1 in both lanes: the same sum)
                if (zh == 0 && a < Mc) {
                    double *dst = part_z + ((int64_t)tile * Mc + a) * D;
#pragma unroll
                    for (int d = 0; d < DT; ++d)
                        if (d < D) dst[d] = l == 0 ? sz[d] : dst[d] + sz[d]; // (latents ascending, by the one thread that owns the slot)
                }
            }
        }
    }
    // the workgroup's D + 1 sums: every thread's share through LDS, added in thread order
    __syncthreads();
#pragma unroll
    for (int d = 0; d < DT; ++d)
        if (d < D) red[d * 256 + tid] = accd[d];
    red[D * 256 + tid] = accv;
    __syncthreads();
    if (tid <= D) {
        double s = 0.0;
        for (int t = 0; t < 256; ++t) s += red[tid * 256 + t];
        part[tile * (D + 1) + tid] = s;
    }
}

int32_t hy_gemm(agpl_ctx *ctx, int m, int n, int k, const double *A, int lda, int ta, const double *B, int ldb, int tb, double *Cm,
                int ldc, double alpha, double beta) {
    hy_gemm_kernel<<<dim3((unsigned)agpl_cdiv(n, 16), (unsigned)agpl_cdiv(m, 16)), 256, 0, ctx->stream>>>(m, n, k, A, lda, ta, B, ldb,
                                                                                                        tb, Cm, ldc, alpha, beta);
    AGPL_LAUNCH_CHECK(ctx);
    return AGPL_OK;
}

unsigned hy_blocks(int64_t total) {
    const int64_t nb = agpl_cdiv(total, 256);
    return (unsigned)(nb > 4096 ? 4096 : nb);
}

// L^-1 in float64, row-major [Mc][Mc] -> Li: K_ZZ + (jitter - 1) I from the scaled inducing inputs the plan holds (-> Gk [Mp][Mp];
// zsc <- the plan's z / ell), then the library's float64 factor route (-> Fw, column-major lower triangle at Mp) with the plan's
// stored jitter.  ones: 16 unit lengthscales (the plan holds z / ell); gz: Mp zeros; kw: se_kzz_kernel's eight words, set to ~0.
// Stated once for agpl_plan_hyper_grad, agpl_plan_inducing_grad and agpl_plan_sample_paths (agpl_pathwise.hip).
int32_t hy_linv(agpl_ctx *ctx, const agpl_plan *p, const double *ones, double *Gk, const double *gz, double *Fw, double *Li, double *zsc,
                unsigned long long *kw) {
    int32_t rc = agpl_se_kzz(ctx, p->kind, p->kparam, p->M, p->Mc, p->D, p->zs, ones, p->ell, nullptr, p->s2, p->jitter, Gk, zsc, kw);
    if (rc) return rc;
    rc = agpl_gaussian_factor(ctx, p->M, 1, Gk, gz, nullptr, Fw, nullptr, nullptr);
    if (rc) return rc;
    hy_lower_kernel<<<hy_blocks((int64_t)p->Mc * p->Mc), 256, 0, ctx->stream>>>(p->Mc, p->M, Fw, Li);
    AGPL_LAUNCH_CHECK(ctx);
    return AGPL_OK;
}

template <int KIND, int DT, bool ZG>
int32_t hy_points_launch(agpl_ctx *ctx, int64_t n, int64_t pitch, const agpl_plan *p, const h8 *Ph, const h8 *Pl, const h8 *Ch,
                         const h8 *Cl, const float *unscale, const double *pv, const double *x, const float *mu0, const float *beta,
                         const float *gamma, double *part, double *part_z) {
    const size_t lds = (size_t)kStageBytes + sizeof(double) * BS * (size_t)p->D;
    AGPL_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&hy_points_kernel<KIND, DT, ZG>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hy_points_kernel<KIND, DT, ZG><<<(unsigned)agpl_cdiv(n, BS), 256, lds, ctx->stream>>>(
        n, pitch, p->M, p->Mc, p->D, p->L, Ph, Pl, Ch, Cl, unscale, pv, x, p->zs, p->ell, (float)p->s2, (float)p->kparam, mu0, beta,
        gamma, part, part_z);
    AGPL_LAUNCH_CHECK(ctx);
    return AGPL_OK;
}

template <int KIND, bool ZG, typename... Args>
int32_t hy_points_kind(agpl_ctx *ctx, int D, Args... args) {
    if (D == 1) return hy_points_launch<KIND, 1, ZG>(ctx, args...);
    if (D <= 4) return hy_points_launch<KIND, 4, ZG>(ctx, args...);
    return hy_points_launch<KIND, 16, ZG>(ctx, args...);
}

constexpr size_t kZPartBudget = (size_t)16 << 20; // bytes of part_z in flight (never less than one tile's Mc D float64)

// The body of agpl_plan_hyper_grad (ZG = false: grad_z_out unused) and of agpl_plan_inducing_grad (ZG = true: grad_out may be NULL,
// the D + 1 numbers then go to the scratch).  fn: the entry point's name, for the messages.
template <bool ZG>
int32_t hy_grad(const char *fn, agpl_plan *p, int64_t N, const double *x, const float *mu0, const float *beta, const float *gamma,
                const double *G, const double *g, double *grad_out, double *grad_z_out) {
    if (!p || !p->ctx) return AGPL_ERR_INVALID_ARGUMENT;
    agpl_ctx *ctx = p->ctx;
    if (!p->se) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "%s needs a plan made from raw inputs (agpl_plan_create_se / agpl_plan_create_stationary)", fn);
    if (p->flags & AGPL_PLAN_NO_MARGINALS)
        AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "%s needs a plan with the marginal image (its q(v) in factor form)", fn);
    if (N != p->N) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "N = %lld, the plan holds %lld points", (long long)N, (long long)p->N);
    if (!x || !beta || !gamma || (ZG ? !grad_z_out : !grad_out)) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "null argument");
    if ((G == nullptr) != (g == nullptr)) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "G and g are given together or not at all");
    const int L = p->L, Mp = p->M, Mc = p->Mc, D = p->D, D1 = D + 1;
    const int64_t C = N < kHyperChunk ? N : kHyperChunk;
    const int64_t ctiles = agpl_cdiv(C, BS);
    const bool kzz = G != nullptr || mu0 != nullptr;
    const auto al = agpl_align256;
    const size_t img = al((size_t)agpl_split_features_bytes(C, Mp));          // one plane of the chunk's marginal image
    const size_t cimg = al(sizeof(_Float16) * (size_t)L * Mp * Mp);           // one plane of the C images
    const size_t rsb = al(sizeof(float) * (size_t)C);
    const size_t partb = al(sizeof(double) * (size_t)ctiles * D1);
    const size_t vecb = al(sizeof(double) * (size_t)L * Mp);                  // pv, h, m (each), one group of hp
    const size_t matp = al(sizeof(double) * (size_t)Mp * Mp), matc = al(sizeof(double) * (size_t)Mc * Mc);
    const size_t zsb = al(sizeof(double) * (size_t)Mp * D);
    const int nmat = kzz ? 9 : 5; // (the K_ZZ part's four matrices only when it runs)
    // ZG: part_z of one group of tiles (kZPartBudget bounds it), the [Mc][D] accumulator, the K_ZZ part, the D + 1 numbers
    const int64_t MD = (int64_t)Mc * D;
    const int64_t zfit = (int64_t)(kZPartBudget / (sizeof(double) * (size_t)MD));
    const int64_t gtiles = ZG ? (zfit < 1 ? 1 : (zfit < ctiles ? zfit : ctiles)) : ctiles; // tiles per launch of the points kernel
    const size_t zpartb = ZG ? al(sizeof(double) * (size_t)gtiles * MD) : 0, zvecb = ZG ? al(sizeof(double) * (size_t)MD) : 0;
    const size_t need = 2 * img + 2 * cimg + rsb + partb + (3 + kHGroups) * vecb + 2 * matp + nmat * matc + zsb + 3 * al(8 * (size_t)Mp) + 4096 +
                        zpartb + 2 * zvecb + (ZG ? 256 : 0);
    if (int32_t rc_ = agpl_pred_reserve(p, need, "gradient")) return rc_; // (every call carves the scratch anew)
    char *w = (char *)p->pred;
    auto take = [&](size_t b) { char *r = w; w += b; return r; };
    void *Ph = take(img), *Pl = take(img);
    h8 *Ch = (h8 *)take(cimg), *Cl = (h8 *)take(cimg);
    float *rs = (float *)take(rsb);
    double *part = (double *)take(partb);
    double *pv = (double *)take(vecb), *hv = (double *)take(vecb), *mv = (double *)take(vecb), *hp = (double *)take(kHGroups * vecb);
    double *Gk = (double *)take(matp), *Fw = (double *)take(matp);
    double *Li = (double *)take(matc), *Um = (double *)take(matc), *Sm = (double *)take(matc), *Wm = (double *)take(matc),
           *Cm = (double *)take(matc);
    const size_t matk = kzz ? matc : 0;
    double *Am = (double *)take(matk), *T1 = (double *)take(matk), *T2 = (double *)take(matk), *T3 = (double *)take(matk);
    double *zsc = (double *)take(zsb);
    double *gz = (double *)take(al(8 * (size_t)Mp)), *tv = (double *)take(al(8 * (size_t)Mp)), *Gmv = (double *)take(al(8 * (size_t)Mp));
    char *tail = take(4096);
    unsigned long long *words = (unsigned long long *)tail; // the generators' eight status words ([2]: first non-finite x)
    unsigned *maxbits = (unsigned *)(words + 8);
    unsigned long long *kw = (unsigned long long *)(tail + 128); // se_kzz_kernel's words (not reported: the plan was made from this z)
    unsigned long long *cw = (unsigned long long *)(tail + 256); // [L] max |C_l|
    float *unscale = (float *)(tail + 1024);                     // [L]
    double *ones = (double *)(tail + 2048);                      // [16] unit lengthscales: the plan holds z / ell
    double *part_z = (double *)take(zpartb), *accz = (double *)take(zvecb), *gk = (double *)take(zvecb);
    if constexpr (ZG) {
        double *th = (double *)take(256); // [D + 1] when the caller does not want them
        if (!grad_out) grad_out = th;
        AGPL_HIP(ctx, hipMemsetAsync(accz, 0, sizeof(double) * (size_t)MD, ctx->stream));
    }

    AGPL_HIP(ctx, hipMemsetAsync(grad_out, 0, sizeof(double) * D1, ctx->stream));
    AGPL_HIP(ctx, hipMemsetAsync(words, 0xff, 8 * sizeof(unsigned long long), ctx->stream));
    AGPL_HIP(ctx, hipMemsetAsync(maxbits, 0, sizeof(unsigned), ctx->stream));
    AGPL_HIP(ctx, hipMemsetAsync(kw, 0xff, 8 * sizeof(unsigned long long), ctx->stream));
    AGPL_HIP(ctx, hipMemsetAsync(cw, 0, sizeof(unsigned long long) * L, ctx->stream));
    AGPL_HIP(ctx, hipMemsetAsync(gz, 0, sizeof(double) * Mp, ctx->stream));
    AGPL_HIP(ctx, hipMemsetAsync(pv, 0, sizeof(double) * (size_t)L * Mp, ctx->stream));
    AGPL_HIP(ctx, hipMemsetAsync(hv, 0, sizeof(double) * (size_t)L * Mp, ctx->stream));
    if (kzz) AGPL_HIP(ctx, hipMemsetAsync(Am, 0, sizeof(double) * (size_t)Mc * Mc, ctx->stream));
    static const double host_ones[16] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1};
    AGPL_HIP(ctx, hipMemcpyAsync(ones, host_ones, sizeof(host_ones), hipMemcpyHostToDevice, ctx->stream));
#define AGPL_HY_RC(call_)      \
    do {                       \
        rc = (call_);          \
        if (rc) return rc;     \
    } while (0)
    int32_t rc;
    AGPL_HY_RC(hy_linv(ctx, p, ones, Gk, gz, Fw, Li, zsc, kw));
    const int64_t mm = (int64_t)Mc * Mc;
    const int nks = Mp / KT;
    for (int l = 0; l < L; ++l) {
        double *ml = mv + (size_t)l * Mp;
        hy_lower_kernel<<<hy_blocks(mm), 256, 0, ctx->stream>>>(Mc, Mp, p->A_work + (size_t)l * Mp * Mp, Um);
        AGPL_LAUNCH_CHECK(ctx);
        AGPL_HY_RC(hy_gemm(ctx, Mc, Mc, Mc, Um, Mc, 1, Um, Mc, 0, Sm, Mc, 1.0, 0.0));                  // S = U'U
        AGPL_HY_RC(hy_gemm(ctx, Mc, 1, Mc, Um, Mc, 1, p->v + (size_t)l * Mp, 1, 0, ml, 1, 1.0, 0.0));   // m = U'v
        hy_w_kernel<<<hy_blocks(mm), 256, 0, ctx->stream>>>(Mc, Sm, ml, Wm);                           // Sm = I - S, W
        AGPL_LAUNCH_CHECK(ctx);
        AGPL_HY_RC(hy_gemm(ctx, Mc, Mc, Mc, Li, Mc, 1, Wm, Mc, 0, Cm, Mc, 1.0, 0.0));                  // C = L^-T W
        AGPL_HY_RC(hy_gemm(ctx, Mc, 1, Mc, Li, Mc, 1, ml, 1, 0, pv + (size_t)l * Mp, 1, 1.0, 0.0));     // p = L^-T m
        hy_max_kernel<<<hy_blocks(mm), 256, 0, ctx->stream>>>(mm, Cm, cw + l);
        AGPL_LAUNCH_CHECK(ctx);
        hy_pack_kernel<<<dim3((unsigned)nks, (unsigned)(Mp / BS)), 256, 0, ctx->stream>>>(
            Mc, Mp, Cm, cw + l, p->scale_exp, Ch + (size_t)l * (Mp / BS) * nks * 256, Cl + (size_t)l * (Mp / BS) * nks * 256, unscale + l);
        AGPL_LAUNCH_CHECK(ctx);
        if (G) AGPL_HY_RC(hy_gemm(ctx, Mc, Mc, Mc, Sm, Mc, 0, G + (size_t)l * mm, Mc, 0, Am, Mc, 1.0, 1.0)); // A += (I - S) G
    }

    // the points' part, chunk by chunk
    for (int64_t c0 = 0; c0 < N; c0 += C) {
        const int64_t n = N - c0 < C ? N - c0 : C;
        AGPL_HY_RC(agpl_se_build(ctx, p->kind, p->kparam, n, Mp, Mc, D, x + c0 * D, p->zs, p->ell, p->s2, p->Lt, p->scale_exp, Ph, Pl,
                                 nullptr, rs, maxbits, words));
        const float *mu0c = mu0 ? mu0 + c0 : nullptr;
        // one launch per group of gtiles tiles (ZG = false: the whole chunk); every index of the kernel is linear in the tile, so a
        // group is the same kernel on pointers moved to its first tile
        const int64_t ntile = agpl_cdiv(n, BS);
        for (int64_t t0 = 0; t0 < ntile; t0 += gtiles) {
            const int64_t q0 = t0 * BS, nq = n - q0 < gtiles * BS ? n - q0 : gtiles * BS;
            const h8 *Phg = (const h8 *)Ph + t0 * (Mp / KT) * 256, *Plg = (const h8 *)Pl + t0 * (Mp / KT) * 256;
            switch (p->kind) {
#define AGPL_HY_KIND_(K)                                                                                                          \
    case K:                                                                                                                       \
        AGPL_HY_RC((hy_points_kind<K, ZG>(ctx, D, nq, N, (const agpl_plan *)p, Phg, Plg, (const h8 *)Ch, (const h8 *)Cl,           \
                                          (const float *)unscale, (const double *)pv, x + (c0 + q0) * D,                          \
                                          mu0c ? mu0c + q0 : nullptr, beta + c0 + q0, gamma + c0 + q0, part + t0 * D1, part_z))); \
        break;
                AGPL_HY_KIND_(AGPL_KERNEL_SE)
                AGPL_HY_KIND_(AGPL_KERNEL_MATERN12)
                AGPL_HY_KIND_(AGPL_KERNEL_MATERN32)
                AGPL_HY_KIND_(AGPL_KERNEL_MATERN52)
                AGPL_HY_KIND_(AGPL_KERNEL_RQ)
                AGPL_HY_KIND_(AGPL_KERNEL_PERIODIC)
                AGPL_HY_KIND_(AGPL_KERNEL_SE_PERIODIC)
                AGPL_HY_KIND_(AGPL_KERNEL_SE_COSINE)
#undef AGPL_HY_KIND_
            default: AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "unknown kernel kind %d", p->kind);
            }
            if constexpr (ZG) {
                hy_zreduce_kernel<<<(unsigned)agpl_cdiv(MD, 256), 256, 0, ctx->stream>>>(agpl_cdiv(nq, BS), MD, part_z, accz);
                AGPL_LAUNCH_CHECK(ctx);
            }
        }
        hy_reduce_kernel<<<1, 64, 0, ctx->stream>>>(agpl_cdiv(n, BS), D1, part, grad_out);
        AGPL_LAUNCH_CHECK(ctx);
        if (mu0) {
            hy_h_kernel<<<dim3((unsigned)nks, kHGroups, (unsigned)L), 256, 0, ctx->stream>>>(
                n, N, Mp, L, (const h8 *)Ph, (const h8 *)Pl, ldexpf(1.f, -p->scale_exp), mu0c, gamma + c0, hp);
            AGPL_LAUNCH_CHECK(ctx);
            hy_hsum_kernel<<<(unsigned)agpl_cdiv((int64_t)L * Mp, 256), 256, 0, ctx->stream>>>((int64_t)L * Mp, hp, hv);
            AGPL_LAUNCH_CHECK(ctx);
        }
    }

    // the K_ZZ part: A += m_l t_l', Lbar, the reverse rule of the factorisation, the contraction with dK_ZZ
    if (kzz) {
        for (int l = 0; l < L; ++l) {
            const double *ml = mv + (size_t)l * Mp;
            if (G) AGPL_HY_RC(hy_gemm(ctx, Mc, 1, Mc, G + (size_t)l * mm, Mc, 0, ml, 1, 0, Gmv, 1, 1.0, 0.0));
            hy_t_kernel<<<(unsigned)agpl_cdiv(Mc, 256), 256, 0, ctx->stream>>>(Mc, g ? g + (size_t)l * Mc : nullptr, Gmv,
                                                                                mu0 ? hv + (size_t)l * Mp : nullptr, tv);
            AGPL_LAUNCH_CHECK(ctx);
            hy_rank1_kernel<<<hy_blocks(mm), 256, 0, ctx->stream>>>(Mc, ml, tv, Am);
            AGPL_LAUNCH_CHECK(ctx);
        }
        AGPL_HY_RC(hy_gemm(ctx, Mc, Mc, Mc, Li, Mc, 1, Am, Mc, 0, T1, Mc, 1.0, 0.0)); // L^-T A
        hy_tril_kernel<<<hy_blocks(mm), 256, 0, ctx->stream>>>(Mc, 0, T1);            // Lbar
        AGPL_LAUNCH_CHECK(ctx);
        hy_kt_kernel<<<hy_blocks(mm), 256, 0, ctx->stream>>>(Mc, Mp, Gk, T2);          // K_ZZ + jitter I
        AGPL_LAUNCH_CHECK(ctx);
        AGPL_HY_RC(hy_gemm(ctx, Mc, Mc, Mc, T2, Mc, 0, Li, Mc, 1, T3, Mc, 1.0, 0.0)); // L = (K_ZZ + jitter I) L^-T
        AGPL_HY_RC(hy_gemm(ctx, Mc, Mc, Mc, T3, Mc, 1, T1, Mc, 0, Um, Mc, 1.0, 0.0)); // L' Lbar
        hy_tril_kernel<<<hy_blocks(mm), 256, 0, ctx->stream>>>(Mc, 1, Um);            // Phi(.)
        AGPL_LAUNCH_CHECK(ctx);
        AGPL_HY_RC(hy_gemm(ctx, Mc, Mc, Mc, Li, Mc, 1, Um, Mc, 0, Sm, Mc, 1.0, 0.0)); // L^-T P
        AGPL_HY_RC(hy_gemm(ctx, Mc, Mc, Mc, Sm, Mc, 0, Li, Mc, 0, Wm, Mc, 1.0, 0.0)); // L^-T P L^-1
        hy_sym_kernel<<<hy_blocks(mm), 256, 0, ctx->stream>>>(Mc, Wm, Cm);
        AGPL_LAUNCH_CHECK(ctx);
        hy_kzz_grad_kernel<<<(unsigned)D1, 256, 0, ctx->stream>>>(p->kind, p->kparam, Mc, D, zsc, p->ell, p->s2, Cm, grad_out);
        AGPL_LAUNCH_CHECK(ctx);
        if constexpr (ZG) {
            hy_kzz_zgrad_kernel<<<(unsigned)Mc, 256, 0, ctx->stream>>>(p->kind, p->kparam, Mc, D, zsc, p->ell, p->s2, Cm, gk);
            AGPL_LAUNCH_CHECK(ctx);
        }
    }
    if constexpr (ZG) {
        hy_zfinal_kernel<<<(unsigned)agpl_cdiv(MD, 256), 256, 0, ctx->stream>>>(MD, D, accz, kzz ? gk : nullptr, p->ell, grad_z_out);
        AGPL_LAUNCH_CHECK(ctx);
    }
#undef AGPL_HY_RC
    unsigned long long hw[8];
    AGPL_HIP(ctx, hipMemcpyAsync(hw, words, sizeof(hw), hipMemcpyDeviceToHost, ctx->stream));
    const int32_t synced = agpl_ctx_synchronize(ctx); // waits, and collects the outcome of the factorisation
    if (hw[2] != ~0ull) AGPL_FAIL(ctx, AGPL_ERR_DOMAIN, "an input x is not finite (point %llu of its 65536-point chunk)", hw[2]);
    return synced;
}

} // namespace
