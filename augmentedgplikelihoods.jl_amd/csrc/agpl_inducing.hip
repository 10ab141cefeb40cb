// agpl_inducing.hip -- inducing inputs from the data: Lloyd's k-means in the metric u = x / ell (include/agpl_inducing.h).
//
//   km_seed_kernel     one thread per centre: the stratified index from the reserved Philox sub-stream, the row if this range owns it.
//   km_bound_kernel    max |x_d / ell_d| over a range: wave and workgroup maxima, then one 64-bit integer atomicMax of the bit pattern
//                      (non-negative float64 order as their bit patterns).
//   km_step_kernel     the pass over the points.  A workgroup of 512 lanes takes tiles of 512 P points (P = 4 for D <= 8, else 2), a
//                      lane owning the D scaled coordinates of its P points in registers.  The scaled centres z / ell go through LDS
//                      in chunks of 256 (<= 32 KB); every lane of a wave reads the same centre address (a broadcast) and feeds P
//                      fused multiply-adds per LDS operand; the running (min, argmin) stay in registers across chunks, strict `<`
//                      over ascending centres = lowest index on a tie.  Then D + 2 64-bit integer atomic adds per point: into a
//                      per-workgroup accumulator in LDS while M (D + 2) 8 bytes fit beside the chunk (kLdsBudget), flushed once at
//                      the workgroup's end by global integer atomics of its non-zero words; straight into global memory beyond.
//   km_centres_kernel  one workgroup: the divisions, the empty count, the largest movement and the INTEGER sum of the cost column.
// No floating-point sum crosses a point: acc is a sum of integers, independent of the split, the order, the grid and the launches.
#include "../../include/agpl_inducing.h"
#include "agpl_common.h"
#include "agpl_random.h"

#include <math.h>

namespace {

constexpr int kThreads = 512;            // lanes of a step workgroup: two waves per SIMD
constexpr int kChunk = 256;              // centres per LDS chunk
constexpr int kLdsBudget = 144 * 1024;   // of the CU's 160 KB: the chunk, 16 lengthscales and the accumulator
constexpr int kMaxM = 2048, kMaxD = 16;
constexpr uint32_t kSubInducing = 0xFFFFFFu; // the Philox sub-stream of the stratified start (agpl_random.h: the samplers' end below 2^22)

struct KmEll {
    double v[kMaxD];
};

struct KmRule {
    int sx, sd;
    double qx, qd, rx, rd, dmax, bound;
};

__host__ __device__ inline int km_ceil_log2(int64_t n) {
    int c = 0;
    while (((int64_t)1 << c) < n) ++c;
    return c;
}

// the fixed-point rule of include/agpl_inducing.h
__host__ __device__ inline KmRule km_rule(double bound, int64_t N_total, int D) {
    KmRule r;
    int eb = 0;
    (void)frexp(bound, &eb);
    const int cl = km_ceil_log2(N_total), cd = km_ceil_log2(D);
    int sx = 61 - cl - eb, sd = 61 - cl - 2 * eb - 2 - cd;
    sx = sx > 1000 ? 1000 : (sx < -1000 ? -1000 : sx);
    sd = sd > 1000 ? 1000 : (sd < -1000 ? -1000 : sd);
    r.sx = sx;
    r.sd = sd;
    r.qx = ldexp(1.0, sx);
    r.qd = ldexp(1.0, sd);
    r.rx = ldexp(1.0, -sx);
    r.rd = ldexp(1.0, -sd);
    const double dm = 4.0 * D * bound * bound;
    r.dmax = dm <= 1.79e308 ? dm : 1.79e308;
    r.bound = bound;
    return r;
}

// the bound a kernel works with: the caller's, or the one a max pass left on the device (zero, an all-zero x, counts as 1)
__device__ __forceinline__ double km_bound(double bound, const unsigned long long *bound_dev) {
    if (!bound_dev) return bound;
    const double b = __longlong_as_double((long long)*bound_dev);
    return b > 0.0 ? b : 1.0;
}

__global__ __launch_bounds__(256) void km_seed_kernel(uint64_t seed, int64_t N_total, int64_t i0, int64_t n, int M, int D,
                                                      const double *__restrict__ x, double *__restrict__ z, int64_t *__restrict__ idx) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= M) return;
    const int64_t lo = (int64_t)j * N_total / M, hi = ((int64_t)j + 1) * N_total / M;
    agpl::Philox g;
    g.init(seed, (uint64_t)j, 0u);
    agpl::Philox s = g.sub(kSubInducing);
    const double u = s.u01();                                      // (k + 1/2) 2^-52
    const unsigned long long k = (unsigned long long)(u * 0x1.0p52); // k < 2^52
    const int64_t at = lo + (int64_t)__umul64hi(k << 12, (unsigned long long)(hi - lo)); // floor(k (hi - lo) / 2^52)
    const bool own = at >= i0 && at < i0 + n;
    for (int d = 0; d < D; ++d) z[(int64_t)j * D + d] = own ? x[(at - i0) * D + d] : 0.0;
    if (idx) idx[j] = at;
}

__global__ __launch_bounds__(256) void km_bound_kernel(int64_t n, int D, const double *__restrict__ x, KmEll ell,
                                                       unsigned long long *__restrict__ out) {
    __shared__ double ells[kMaxD];
    __shared__ unsigned long long part[4];
    if (threadIdx.x < kMaxD) ells[threadIdx.x] = threadIdx.x < D ? ell.v[threadIdx.x] : 1.0;
    __syncthreads();
    const int64_t total = n * D;
    double m = 0.0;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const double v = fabs(x[e] / ells[(int)(e % D)]);
        if (v <= 1.79e308 && v > m) m = v;
    }
    unsigned long long b = (unsigned long long)__double_as_longlong(m);
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(b, o, 64);
        b = other > b ? other : b;
    }
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = b;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) b = part[w] > b ? part[w] : b;
        if (b) atomicMax(out, b);
    }
}

// words: [0] first non-finite x, [1] first point beyond the bound, [2] first non-finite z (all ones: none)
template <int D, int P>
__global__ __launch_bounds__(kThreads) void km_step_kernel(int64_t n, int M, const double *__restrict__ x, KmEll ell,
                                                           const double *__restrict__ z, double bound_arg,
                                                           const unsigned long long *__restrict__ bound_dev, int64_t N_total,
                                                           unsigned long long *__restrict__ acc, int *__restrict__ assign,
                                                           unsigned long long *__restrict__ words, int lds_acc) {
    extern __shared__ __attribute__((aligned(16))) double km_smem[];
    constexpr int W = D + 2;
    double *zc = km_smem;                 // [kChunk][D]
    double *ells = km_smem + kChunk * D;  // [16]
    unsigned long long *lacc = reinterpret_cast<unsigned long long *>(ells + kMaxD); // [M][W] when lds_acc
    const int tid = threadIdx.x;
    const KmRule rule = km_rule(km_bound(bound_arg, bound_dev), N_total, D);
    if (tid < kMaxD) ells[tid] = tid < D ? ell.v[tid] : 1.0;
    if (lds_acc)
        for (int t = tid; t < M * W; t += kThreads) lacc[t] = 0ull;
    const int nchunks = (M + kChunk - 1) / kChunk;
    const int64_t tile_pts = (int64_t)kThreads * P;
    const int64_t ntiles = (n + tile_pts - 1) / tile_pts;
    bool loaded = false;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        double u[P][D], best[P];
        int arg[P];
        bool live[P];
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const int64_t i = tile * tile_pts + (int64_t)p * kThreads + tid;
            live[p] = i < n;
            best[p] = __builtin_inf();
            arg[p] = 0;
            bool finite = true, inside = true;
#pragma unroll
            for (int d = 0; d < D; ++d) {
                const double xv = live[p] ? x[i * D + d] : 0.0;
                u[p][d] = xv / ell.v[d];
                finite = finite && fabs(xv) <= 1.79e308;
                inside = inside && fabs(u[p][d]) <= rule.bound;
            }
            if (live[p] && !finite) {
                atomicMin(&words[0], (unsigned long long)i);
                live[p] = false;
            } else if (live[p] && !inside) {
                atomicMin(&words[1], (unsigned long long)i);
                live[p] = false;
            }
            if (!live[p]) {
                if (assign && i < n) assign[i] = -1;
#pragma unroll
                for (int d = 0; d < D; ++d) u[p][d] = 0.0;
            }
        }
        for (int ch = 0; ch < nchunks; ++ch) {
            const int c0 = ch * kChunk;
            const int cn = M - c0 < kChunk ? M - c0 : kChunk;
            if (!(nchunks == 1 && loaded)) { // one chunk: it stays in LDS across this workgroup's tiles
                __syncthreads();
                for (int t = tid; t < cn * D; t += kThreads) {
                    const double zv = z[(int64_t)c0 * D + t];
                    if (!(fabs(zv) <= 1.79e308)) atomicMin(&words[2], (unsigned long long)(c0 + t / D));
                    zc[t] = zv / ells[t % D];
                }
                __syncthreads();
                loaded = true;
            }
            for (int c = 0; c < cn; ++c) {
                double r[P];
#pragma unroll
                for (int p = 0; p < P; ++p) r[p] = 0.0;
#pragma unroll
                for (int d = 0; d < D; ++d) {
                    const double zv = zc[c * D + d];
#pragma unroll
                    for (int p = 0; p < P; ++p) {
                        const double t = u[p][d] - zv;
                        r[p] = __builtin_fma(t, t, r[p]);
                    }
                }
#pragma unroll
                for (int p = 0; p < P; ++p)
                    if (r[p] < best[p]) {
                        best[p] = r[p];
                        arg[p] = c0 + c;
                    }
            }
        }
#pragma unroll
        for (int p = 0; p < P; ++p) {
            if (!live[p]) continue;
            const int64_t i = tile * tile_pts + (int64_t)p * kThreads + tid;
            if (assign) assign[i] = arg[p];
            const double dd = best[p] < rule.dmax ? best[p] : rule.dmax;
            const unsigned long long qd = (unsigned long long)__double2ll_rn(dd * rule.qd);
            if (lds_acc) {
                unsigned long long *row = lacc + arg[p] * W;
                atomicAdd(row, 1ull);
#pragma unroll
                for (int d = 0; d < D; ++d) atomicAdd(row + 1 + d, (unsigned long long)__double2ll_rn(u[p][d] * rule.qx));
                atomicAdd(row + 1 + D, qd);
            } else {
                unsigned long long *row = acc + (int64_t)arg[p] * W;
                atomicAdd(row, 1ull);
#pragma unroll
                for (int d = 0; d < D; ++d) atomicAdd(row + 1 + d, (unsigned long long)__double2ll_rn(u[p][d] * rule.qx));
                atomicAdd(row + 1 + D, qd);
            }
        }
    }
    if (lds_acc) {
        __syncthreads();
        for (int t = tid; t < M * W; t += kThreads) {
            const unsigned long long v = lacc[t];
            if (v) atomicAdd(acc + t, v);
        }
    }
}

// one workgroup.  update: move the centres and report all of info; otherwise (the final step) z and info[1] stay.
__global__ __launch_bounds__(256) void km_centres_kernel(int M, int D, int64_t N_total, KmEll ell, double bound_arg,
                                                         const unsigned long long *__restrict__ bound_dev,
                                                         const long long *__restrict__ acc, double *__restrict__ z,
                                                         double *__restrict__ info, int update) {
    __shared__ double ells[kMaxD];
    __shared__ double mv[256];
    __shared__ long long cs[256];
    __shared__ int em[256];
    const int tid = threadIdx.x;
    if (tid < kMaxD) ells[tid] = tid < D ? ell.v[tid] : 1.0;
    __syncthreads();
    const KmRule rule = km_rule(km_bound(bound_arg, bound_dev), N_total, D);
    const int W = D + 2;
    double move2 = 0.0;
    long long cost = 0;
    int empty = 0;
    for (int j = tid; j < M; j += 256) {
        const long long cnt = acc[(int64_t)j * W];
        cost += acc[(int64_t)j * W + 1 + D];
        if (cnt <= 0) {
            empty += 1;
            continue;
        }
        if (!update) continue;
        double m2 = 0.0;
        for (int d = 0; d < D; ++d) {
            const double un = ((double)acc[(int64_t)j * W + 1 + d] / (double)cnt) * rule.rx;
            const double zn = ells[d] * un;
            const double dz = (zn - z[(int64_t)j * D + d]) / ells[d];
            m2 = __builtin_fma(dz, dz, m2);
            z[(int64_t)j * D + d] = zn;
        }
        move2 = m2 > move2 ? m2 : move2;
    }
    mv[tid] = move2;
    cs[tid] = cost;
    em[tid] = empty;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            mv[tid] = mv[tid + o] > mv[tid] ? mv[tid + o] : mv[tid];
            cs[tid] += cs[tid + o];
            em[tid] += em[tid + o];
        }
        __syncthreads();
    }
    if (tid == 0 && info) {
        info[0] = (double)em[0];
        if (update) info[1] = sqrt(mv[0]);
        info[2] = (double)cs[0] * rule.rd;
    }
}

int km_grid(int64_t elems) { // the max pass: 256 CUs x 8 workgroups at the most, grid-stride beyond
    const int64_t b = agpl_cdiv(elems, 256);
    return (int)(b < 2048 ? (b < 1 ? 1 : b) : 2048);
}

int km_step_grid(int64_t n, int P, size_t lds) {
    const int64_t tiles = agpl_cdiv(n, (int64_t)kThreads * P);
    const int64_t cap = lds <= 80 * 1024 ? 512 : 256; // 256 CUs, two workgroups each while the LDS allows
    return (int)(tiles < cap ? tiles : cap);
}

// the step on the stream, no wait: words as km_step_kernel's (set to all ones by the caller)
int32_t km_step_launch(agpl_ctx *ctx, int64_t N_total, int64_t n, int M, int D, const double *x, const KmEll &ell, const double *z,
                       double bound, const unsigned long long *bound_dev, int64_t *acc, int32_t *assign, unsigned long long *words) {
    const size_t base = sizeof(double) * ((size_t)kChunk * D + kMaxD);
    const size_t accb = sizeof(long long) * (size_t)M * (D + 2);
    const int lds_acc = base + accb <= (size_t)kLdsBudget;
    const size_t lds = base + (lds_acc ? accb : 0);
    unsigned long long *a = reinterpret_cast<unsigned long long *>(acc);
    switch (D) {
#define AGPL_KM_D_(D_, P_)                                                                                                          \
    case D_: {                                                                                                                      \
        if (lds > 64 * 1024)                                                                                                        \
            AGPL_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&km_step_kernel<D_, P_>),                              \
                                              hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBudget));                             \
        km_step_kernel<D_, P_><<<km_step_grid(n, P_, lds), kThreads, lds, ctx->stream>>>(n, M, x, ell, z, bound, bound_dev, N_total, \
                                                                                         a, assign, words, lds_acc);               \
    } break;
        AGPL_KM_D_(1, 4)
        AGPL_KM_D_(2, 4)
        AGPL_KM_D_(3, 4)
        AGPL_KM_D_(4, 4)
        AGPL_KM_D_(5, 4)
        AGPL_KM_D_(6, 4)
        AGPL_KM_D_(7, 4)
        AGPL_KM_D_(8, 4)
        AGPL_KM_D_(9, 2)
        AGPL_KM_D_(10, 2)
        AGPL_KM_D_(11, 2)
        AGPL_KM_D_(12, 2)
        AGPL_KM_D_(13, 2)
        AGPL_KM_D_(14, 2)
        AGPL_KM_D_(15, 2)
        AGPL_KM_D_(16, 2)
#undef AGPL_KM_D_
    default: AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "the input dimension must be 1 ... 16 (got %d)", D);
    }
    AGPL_LAUNCH_CHECK(ctx);
    return AGPL_OK;
}

int32_t km_check_sizes(agpl_ctx *ctx, int64_t N_total, int32_t M, int32_t D) {
    if (D < 1 || D > kMaxD) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "the input dimension must be 1 ... 16 (got %d)", D);
    if (M < 1 || M > kMaxM) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "the number of centres must be 1 ... 2048 (got %d)", M);
    if (N_total < M || N_total >= ((int64_t)1 << 48))
        AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "M = %d centres need M <= N_total < 2^48 points (got %lld)", M, (long long)N_total);
    return AGPL_OK;
}

int32_t km_check_ell(agpl_ctx *ctx, int32_t D, const double *lengthscale, KmEll *out) {
    if (!lengthscale) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "null argument");
    for (int d = 0; d < kMaxD; ++d) out->v[d] = 1.0;
    for (int d = 0; d < D; ++d) {
        if (!(lengthscale[d] > 0.0 && lengthscale[d] <= 1.79e308))
            AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "lengthscale[%d] must be positive and finite", d);
        out->v[d] = lengthscale[d];
    }
    return AGPL_OK;
}

int32_t km_check_bound(agpl_ctx *ctx, double bound) {
    if (!(bound > 0.0 && bound <= 1.79e308)) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "bound must be positive and finite (got %g)", bound);
    return AGPL_OK;
}

// the outcome of the status words (host copies)
int32_t km_report(agpl_ctx *ctx, const unsigned long long *hw) {
    if (hw[0] != ~0ull) AGPL_FAIL(ctx, AGPL_ERR_DOMAIN, "input x[%llu] is not finite", hw[0]);
    if (hw[2] != ~0ull) AGPL_FAIL(ctx, AGPL_ERR_DOMAIN, "centre z[%llu] is not finite", hw[2]);
    if (hw[1] != ~0ull) AGPL_FAIL(ctx, AGPL_ERR_DOMAIN, "input x[%llu] / lengthscale lies beyond the bound", hw[1]);
    return AGPL_OK;
}

} // namespace

extern "C" int32_t agpl_kmeans_quanta(agpl_ctx *ctx, double bound, int64_t N_total, int32_t D, int32_t *sx_out, int32_t *sd_out) {
    if (!sx_out || !sd_out) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "null argument");
    if (D < 1 || D > kMaxD) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "the input dimension must be 1 ... 16 (got %d)", D);
    if (N_total < 1 || N_total >= ((int64_t)1 << 48))
        AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "N_total must be in [1, 2^48) (got %lld)", (long long)N_total);
    const int32_t rc = km_check_bound(ctx, bound);
    if (rc) return rc;
    const KmRule r = km_rule(bound, N_total, D);
    *sx_out = r.sx;
    *sd_out = r.sd;
    return AGPL_OK;
}

extern "C" int32_t agpl_kmeans_seed(agpl_ctx *ctx, int64_t N_total, int64_t i0, int64_t n, int32_t M, int32_t D,
                                    const double *x_local, double *z_out, int64_t *idx_out) {
    if (!ctx) return AGPL_ERR_INVALID_ARGUMENT;
    const int32_t rc = km_check_sizes(ctx, N_total, M, D);
    if (rc) return rc;
    if (i0 < 0 || n < 0 || i0 + n > N_total)
        AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "the range [%lld, %lld) is not inside the %lld points", (long long)i0, (long long)(i0 + n),
                  (long long)N_total);
    if (!z_out || (n > 0 && !x_local)) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "null argument");
    km_seed_kernel<<<(unsigned)agpl_cdiv(M, 256), 256, 0, ctx->stream>>>(ctx->seed, N_total, i0, n, M, D, x_local, z_out, idx_out);
    AGPL_LAUNCH_CHECK(ctx);
    return AGPL_OK;
}

extern "C" int32_t agpl_kmeans_bound(agpl_ctx *ctx, int64_t n, int32_t D, const double *x_local, const double *lengthscale,
                                     double *bound_inout) {
    if (!ctx) return AGPL_ERR_INVALID_ARGUMENT;
    if (D < 1 || D > kMaxD) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "the input dimension must be 1 ... 16 (got %d)", D);
    if (n < 0) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "n = %lld: negative", (long long)n);
    KmEll ell;
    const int32_t rc = km_check_ell(ctx, D, lengthscale, &ell);
    if (rc) return rc;
    if (!bound_inout) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "null argument");
    if (n == 0) return AGPL_OK;
    if (!x_local) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "null argument");
    km_bound_kernel<<<km_grid(n * D), 256, 0, ctx->stream>>>(n, D, x_local, ell,
                                                                           reinterpret_cast<unsigned long long *>(bound_inout));
    AGPL_LAUNCH_CHECK(ctx);
    return AGPL_OK;
}

extern "C" int32_t agpl_kmeans_step(agpl_ctx *ctx, int64_t N_total, int64_t n, int32_t M, int32_t D, const double *x_local,
                                    const double *lengthscale, const double *z, double bound, int64_t *acc, int32_t *assign_out) {
    if (!ctx) return AGPL_ERR_INVALID_ARGUMENT;
    int32_t rc = km_check_sizes(ctx, N_total, M, D);
    if (rc) return rc;
    if (n < 0 || n > N_total) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "n = %lld is not in [0, N_total = %lld]", (long long)n, (long long)N_total);
    KmEll ell;
    rc = km_check_ell(ctx, D, lengthscale, &ell);
    if (rc) return rc;
    rc = km_check_bound(ctx, bound);
    if (rc) return rc;
    if (n == 0) return AGPL_OK;
    if (!x_local || !z || !acc) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "null argument");
    unsigned long long *words = nullptr;
    if (hipMalloc((void **)&words, 4 * sizeof(unsigned long long)) != hipSuccess) {
        (void)hipGetLastError();
        AGPL_FAIL(ctx, AGPL_ERR_OUT_OF_MEMORY, "hipMalloc for the status words failed");
    }
    unsigned long long hw[4] = {~0ull, ~0ull, ~0ull, ~0ull};
    hipError_t e = hipMemsetAsync(words, 0xff, sizeof(hw), ctx->stream);
    if (e == hipSuccess) {
        rc = km_step_launch(ctx, N_total, n, M, D, x_local, ell, z, bound, nullptr, acc, assign_out, words);
        if (rc == AGPL_OK) e = hipMemcpyAsync(hw, words, sizeof(hw), hipMemcpyDeviceToHost, ctx->stream);
    }
    const hipError_t es = hipStreamSynchronize(ctx->stream);
    (void)hipFree(words);
    if (rc) return rc;
    if (e != hipSuccess || es != hipSuccess)
        AGPL_FAIL(ctx, AGPL_ERR_HIP, "k-means step: %s", hipGetErrorString(e != hipSuccess ? e : es));
    return km_report(ctx, hw);
}

extern "C" int32_t agpl_kmeans_centres(agpl_ctx *ctx, int64_t N_total, int32_t M, int32_t D, const double *lengthscale, double bound,
                                       const int64_t *acc, double *z_inout, double *info_out) {
    if (!ctx) return AGPL_ERR_INVALID_ARGUMENT;
    int32_t rc = km_check_sizes(ctx, N_total, M, D);
    if (rc) return rc;
    KmEll ell;
    rc = km_check_ell(ctx, D, lengthscale, &ell);
    if (rc) return rc;
    rc = km_check_bound(ctx, bound);
    if (rc) return rc;
    if (!acc || !z_inout) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "null argument");
    km_centres_kernel<<<1, 256, 0, ctx->stream>>>(M, D, N_total, ell, bound, nullptr, reinterpret_cast<const long long *>(acc), z_inout,
                                                  info_out, 1);
    AGPL_LAUNCH_CHECK(ctx);
    return AGPL_OK;
}

extern "C" int32_t agpl_select_inducing_kmeans(agpl_ctx *ctx, int64_t N, int32_t M, int32_t D, const double *x,
                                               const double *lengthscale, int32_t niter, const double *z0, double *z_out,
                                               double *info_out) {
    if (!ctx) return AGPL_ERR_INVALID_ARGUMENT;
    int32_t rc = km_check_sizes(ctx, N, M, D);
    if (rc) return rc;
    KmEll ell;
    rc = km_check_ell(ctx, D, lengthscale, &ell);
    if (rc) return rc;
    if (niter < 0) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "niter = %d: negative", niter);
    if (!x || !z_out) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "null argument");
    // one block: acc [M][D + 2] | four status words | the bound's bit pattern | info [3]
    const size_t accb = sizeof(int64_t) * (size_t)M * (D + 2);
    char *w = nullptr;
    if (hipMalloc((void **)&w, accb + 64) != hipSuccess) {
        (void)hipGetLastError();
        AGPL_FAIL(ctx, AGPL_ERR_OUT_OF_MEMORY, "hipMalloc(%zu) for the k-means accumulator failed", accb + 64);
    }
    int64_t *acc = (int64_t *)w;
    unsigned long long *words = (unsigned long long *)(w + accb), *bound_dev = words + 4;
    double *info = (double *)(words + 5);
    unsigned long long hw[4] = {~0ull, ~0ull, ~0ull, ~0ull};
    auto fail = [&](int32_t code) {
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipFree(w);
        return code;
    };
#define AGPL_KM_TRY(call_)                                                                                         \
    do {                                                                                                            \
        const hipError_t e_ = (call_);                                                                              \
        if (e_ != hipSuccess) {                                                                                     \
            snprintf(ctx->err, sizeof(ctx->err), "k-means: %s failed: %s", #call_, hipGetErrorString(e_));          \
            return fail(AGPL_ERR_HIP);                                                                              \
        }                                                                                                           \
    } while (0)
    AGPL_KM_TRY(hipMemsetAsync(words, 0xff, 4 * sizeof(unsigned long long), ctx->stream));
    AGPL_KM_TRY(hipMemsetAsync(bound_dev, 0, 4 * sizeof(unsigned long long), ctx->stream)); // the bound and info
    km_bound_kernel<<<km_grid(N * D), 256, 0, ctx->stream>>>(N, D, x, ell, bound_dev);
    AGPL_KM_TRY(hipGetLastError());
    if (z0) {
        AGPL_KM_TRY(hipMemcpyAsync(z_out, z0, sizeof(double) * (size_t)M * D, hipMemcpyDeviceToDevice, ctx->stream));
    } else {
        km_seed_kernel<<<(unsigned)agpl_cdiv(M, 256), 256, 0, ctx->stream>>>(ctx->seed, N, 0, N, M, D, x, z_out, nullptr);
        AGPL_KM_TRY(hipGetLastError());
    }
    for (int it = 0; it <= niter; ++it) { // the last round is the step for the final cost alone
        AGPL_KM_TRY(hipMemsetAsync(acc, 0, accb, ctx->stream));
        rc = km_step_launch(ctx, N, N, M, D, x, ell, z_out, 0.0, bound_dev, acc, nullptr, words);
        if (rc) return fail(rc);
        km_centres_kernel<<<1, 256, 0, ctx->stream>>>(M, D, N, ell, 0.0, bound_dev, reinterpret_cast<const long long *>(acc), z_out, info,
                                                      it < niter ? 1 : 0);
        AGPL_KM_TRY(hipGetLastError());
    }
    if (info_out) AGPL_KM_TRY(hipMemcpyAsync(info_out, info, 3 * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    AGPL_KM_TRY(hipMemcpyAsync(hw, words, sizeof(hw), hipMemcpyDeviceToHost, ctx->stream));
#undef AGPL_KM_TRY
    const hipError_t es = hipStreamSynchronize(ctx->stream);
    (void)hipFree(w);
    if (es != hipSuccess) AGPL_FAIL(ctx, AGPL_ERR_HIP, "k-means: %s", hipGetErrorString(es));
    return km_report(ctx, hw);
}
