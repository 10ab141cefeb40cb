// agpl_greedy.hip -- inducing inputs by greedy conditional variance: the partial pivoted Cholesky of K_XX (include/agpl_greedy.h).
//
//   gv_begin_kernel   d = variance over the range, the first non-finite x into a status word, the first argmax partial.
//   gv_step_kernel    the pass over the points, memory-bound (8 n j bytes of columns against n j fused multiply-adds).  A workgroup
//                     of 256 lanes strides over tiles of kGvTile = 1024 consecutive points, a lane holding 4 points 256 apart, so
//                     that every column load of a wave is one coalesced 512-byte stream and a lane runs 4 independent FMA chains.
//                     The t loop is unrolled by kGvUnroll = 8: 32 loads of 8 bytes per lane are issued before the first FMA needs
//                     one (64 KB per workgroup in flight); each point's FMAs stay in ascending t.  The pivot's row cols[t][p] sits
//                     in LDS and is read at a uniform address (a broadcast).  kappa once per point through the run-time-kind
//                     kernel_value of agpl_kernel_rules.h.  Then the per-workgroup argmax partial (bits of d, lowest index) and ONE
//                     64-bit integer atomic add of the workgroup's fixed-point sum of d / variance.
//   gv_pick_kernel    one workgroup: the partials -> the candidate record (max-with-lowest-index is associative and commutative:
//                     the grid cannot change it).  In the one-process call it also ends the selection (the device flag), gathers
//                     the pivot record and writes z_out[j], idx_out[j] and the info words.
//   gv_pivot_kernel   the pivot record of a range for the building-block path: the owner's values, zeros otherwise.
//   gv_trace_kernel   the integer sums decoded into info.
// No floating-point sum crosses a point and there is no float atomic: the bits do not depend on the split, the grid or the launches.
#include "../../include/agpl_greedy.h"
#include "agpl_common.h"
#include "agpl_kernel_rules.h"

#include <math.h>

namespace {

constexpr int kGvThreads = 256;   // lanes of a step workgroup
constexpr int kGvPoints = 4;      // points per lane
constexpr int kGvTile = 1024;     // points per tile
constexpr int kGvUnroll = 8;      // columns loaded per lane and point before their FMAs
constexpr int kGvPartials = 1024; // the step's grid at the most (256 CUs x 4 workgroups): argmax partials in the work area
constexpr int kGvMaxM = 2048, kGvMaxD = 16;
constexpr long long kGvNone = 0x7fffffffffffffffLL; // the index of "no holder"
static_assert(kGvTile == kGvThreads * kGvPoints, "a tile is one pass of the workgroup's lanes over their points");

struct GvEll {
    double v[kGvMaxD];
};

// the one-process call's extras of gv_pick_kernel (sel.done null: the building-block path)
struct GvSel {
    int *done;            // the end flag
    long long *index;     // [1] the pivot's index for the step
    double *pivot;        // [D + 1 + j]
    double *z_out, *info; // [M][D], [1 + 2 M]
    long long *idx_out;   // [M]
    const double *x, *cols;
    int64_t n;
    int D, j;
    double variance, threshold;
};

__host__ __device__ inline int gv_ceil_log2(int64_t n) {
    int c = 0;
    while (((int64_t)1 << c) < n) ++c;
    return c;
}

// (bits, index) a beats b: the larger d, on a tie the lower index
__device__ __forceinline__ bool gv_better(long long ab, long long ai, long long bb, long long bi) {
    return ab > bb || (ab == bb && ai < bi);
}

// the workgroup's best (bits, index) in lane 0 of wave 0; `sb`, `si` are LDS [kGvThreads / 64]
__device__ __forceinline__ void gv_block_best(long long &bb, long long &bi, long long *sb, long long *si) {
    for (int o = 32; o > 0; o >>= 1) {
        const long long ob = __shfl_xor(bb, o, 64), oi = __shfl_xor(bi, o, 64);
        if (gv_better(ob, oi, bb, bi)) {
            bb = ob;
            bi = oi;
        }
    }
    if ((threadIdx.x & 63) == 0) {
        sb[threadIdx.x >> 6] = bb;
        si[threadIdx.x >> 6] = bi;
    }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < kGvThreads / 64; ++w)
            if (gv_better(sb[w], si[w], bb, bi)) {
                bb = sb[w];
                bi = si[w];
            }
}

// word: the first non-finite x (all ones: none)
__global__ __launch_bounds__(256) void gv_begin_kernel(int64_t n, int D, const double *__restrict__ x, double variance,
                                                       double *__restrict__ d, long long *__restrict__ partials,
                                                       unsigned long long *__restrict__ word) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        bool finite = true;
        for (int e = 0; e < D; ++e) finite = finite && fabs(x[i * D + e]) <= 1.79e308;
        if (!finite) atomicMin(word, (unsigned long long)i);
        d[i] = variance;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { // every d is the variance: the first point holds the maximum
        partials[0] = __double_as_longlong(variance);
        partials[1] = 0;
    }
}

// WARPED: the kind's distance is warped in some dimension (agpl::kernel_dim_warped: the periodic kinds, param = the period) or its kappa
// carries a factor of one (agpl::kernel_dim_modulated: the squared exponential x cosine kind, the same constant ell_d / param), an instantiation of its own so
// that the other kinds' kernel carries none of it; the rule's constants ell_d / param and 1 / ell_d are formed once per workgroup.
template <bool WARPED>
__global__ __launch_bounds__(kGvThreads) void gv_step_kernel(int64_t n, int64_t i0, int D, int kind, double param, int j,
                                                             const double *__restrict__ x, GvEll ell, double variance, double tscale,
                                                             const long long *__restrict__ index, const double *__restrict__ pivot,
                                                             double *__restrict__ cols, double *__restrict__ d,
                                                             long long *__restrict__ partials, unsigned long long *__restrict__ trace,
                                                             const int *__restrict__ done) {
    __shared__ double prow[kGvMaxM]; // cols[t][p], t < j
    __shared__ double xp[kGvMaxD], ells[kGvMaxD];
    __shared__ double wsh[WARPED ? kGvMaxD : 1], ilsh[WARPED ? kGvMaxD : 1];
    __shared__ long long sb[kGvThreads / 64], si[kGvThreads / 64], st[kGvThreads / 64];
    if (done && *done) return;
    const int tid = threadIdx.x;
    for (int t = tid; t < j; t += kGvThreads) prow[t] = pivot[D + 1 + t];
    if (tid < kGvMaxD) {
        ells[tid] = tid < D ? ell.v[tid] : 1.0;
        xp[tid] = tid < D ? pivot[tid] / ell.v[tid] : 0.0;
        if constexpr (WARPED) {
            wsh[tid] = tid < D ? ell.v[tid] / param : 0.0;
            ilsh[tid] = tid < D ? 1.0 / ell.v[tid] : 0.0;
        }
    }
    __syncthreads();
    const double root = sqrt(pivot[D]);
    const int64_t pl = (int64_t)index[0] - i0; // the pivot within this range, if it is there
    long long bb = -1, bi = kGvNone, tr = 0;
    const int64_t ntiles = (n + kGvTile - 1) / kGvTile;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        int64_t at[kGvPoints];
        const double *cp[kGvPoints];
        double acc[kGvPoints];
#pragma unroll
        for (int p = 0; p < kGvPoints; ++p) {
            at[p] = tile * kGvTile + (int64_t)p * kGvThreads + tid;
            cp[p] = cols + (at[p] < n ? at[p] : n - 1); // a lane past the end reads the last point and writes nothing
            acc[p] = 0.0;
        }
        int t = 0;
        for (; t + kGvUnroll <= j; t += kGvUnroll) {
            double v[kGvUnroll][kGvPoints];
#pragma unroll
            for (int u = 0; u < kGvUnroll; ++u)
#pragma unroll
                for (int p = 0; p < kGvPoints; ++p) v[u][p] = cp[p][(int64_t)(t + u) * n];
#pragma unroll
            for (int u = 0; u < kGvUnroll; ++u) {
                const double w = prow[t + u];
#pragma unroll
                for (int p = 0; p < kGvPoints; ++p) acc[p] = __builtin_fma(v[u][p], w, acc[p]);
            }
        }
        for (; t < j; ++t) {
            const double w = prow[t];
#pragma unroll
            for (int p = 0; p < kGvPoints; ++p) acc[p] = __builtin_fma(cp[p][(int64_t)t * n], w, acc[p]);
        }
#pragma unroll
        for (int p = 0; p < kGvPoints; ++p) {
            const int64_t i = at[p];
            if (i >= n) continue;
            double r2 = 0.0;
            [[maybe_unused]] double mod = 1.0;
            for (int e = 0; e < D; ++e) {
                double s = x[i * D + e] / ells[e] - xp[e];
                if constexpr (WARPED) {
                    if (agpl::kernel_dim_modulated(kind, e, D)) mod = agpl::kernel_modulation(s, wsh[e]);
                    if (agpl::kernel_dim_warped(kind, e, D)) s = agpl::kernel_warp<AGPL_KERNEL_PERIODIC>(s, wsh[e], ilsh[e]);
                }
                r2 = __builtin_fma(s, s, r2);
            }
            double k = variance * agpl::kernel_value<double>(kind, r2, param);
            if constexpr (WARPED)
                if (agpl::kernel_kind_modulated(kind)) k *= mod; // (variance kappa, then the factor: two roundings, in this order)
            const double c = (k - acc[p]) / root;
            cols[(int64_t)j * n + i] = c;
            double dn = d[i] - c * c;
            dn = dn > 0.0 ? dn : 0.0;
            if (i == pl) dn = 0.0;
            d[i] = dn;
            const long long bits = __double_as_longlong(dn);
            if (bits > bb) { // a lane meets its points in ascending order: the first holder stays
                bb = bits;
                bi = i;
            }
            tr += __double2ll_rn(dn / variance * tscale);
        }
    }
    for (int o = 32; o > 0; o >>= 1) tr += __shfl_xor(tr, o, 64);
    if ((tid & 63) == 0) st[tid >> 6] = tr;
    gv_block_best(bb, bi, sb, si); // (its barrier covers st)
    if (tid == 0) {
        partials[2 * blockIdx.x] = bb;
        partials[2 * blockIdx.x + 1] = bi;
        for (int w = 1; w < kGvThreads / 64; ++w) tr += st[w];
        if (tr) atomicAdd(trace, (unsigned long long)tr);
    }
}

__global__ __launch_bounds__(kGvThreads) void gv_pick_kernel(int nparts, const long long *__restrict__ partials, int64_t i0,
                                                             long long *__restrict__ cand, GvSel sel) {
    __shared__ long long sb[kGvThreads / 64], si[kGvThreads / 64], best[2];
    if (sel.done && *sel.done) return;
    const int tid = threadIdx.x;
    long long bb = -1, bi = kGvNone;
    for (int w = tid; w < nparts; w += kGvThreads) {
        const long long ob = partials[2 * w], oi = partials[2 * w + 1];
        if (gv_better(ob, oi, bb, bi)) {
            bb = ob;
            bi = oi;
        }
    }
    gv_block_best(bb, bi, sb, si);
    if (tid == 0) {
        best[0] = bb;
        best[1] = bb < 0 ? kGvNone : i0 + bi;
        if (cand) {
            cand[0] = best[0];
            cand[1] = best[1];
        }
    }
    if (!sel.done) return;
    __syncthreads();
    const double dp = __longlong_as_double(best[0]);
    const int64_t p = best[1]; // (one range: i0 = 0)
    if (best[0] < 0 || dp <= sel.threshold * sel.variance) {
        if (tid == 0) *sel.done = 1;
        return;
    }
    const int D = sel.D, j = sel.j;
    if (tid == 0) {
        sel.index[0] = p;
        sel.idx_out[j] = p;
        sel.info[0] = (double)(j + 1);
        sel.info[1 + j] = dp / sel.variance;
        sel.pivot[D] = dp;
    }
    if (tid < D) {
        const double xv = sel.x[p * D + tid];
        sel.pivot[tid] = xv;
        sel.z_out[(int64_t)j * D + tid] = xv;
    }
    for (int t = tid; t < j; t += kGvThreads) sel.pivot[D + 1 + t] = sel.cols[(int64_t)t * sel.n + p];
}

__global__ __launch_bounds__(256) void gv_pivot_kernel(int64_t n, int64_t i0, int D, int j, const double *__restrict__ x,
                                                       const double *__restrict__ cols, const double *__restrict__ d,
                                                       const long long *__restrict__ index, double *__restrict__ pivot) {
    const int64_t p = (int64_t)index[0] - i0;
    const bool own = p >= 0 && p < n;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < D + 1 + j; e += gridDim.x * 256) {
        double v = 0.0;
        if (own) v = e < D ? x[p * D + e] : (e == D ? d[p] : cols[(int64_t)(e - D - 1) * n + p]);
        pivot[e] = v;
    }
}

__global__ __launch_bounds__(256) void gv_trace_kernel(int M, double rscale, const long long *__restrict__ trace,
                                                       double *__restrict__ info) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j < M) info[1 + M + j] = (double)trace[j] * rscale;
}

int64_t gv_bytes(int64_t n, int32_t Mmax) { return (int64_t)sizeof(double) * ((int64_t)Mmax + 1) * n + 16 * (int64_t)kGvPartials; }

// the regions of a work area
struct GvWork {
    double *cols, *d;
    long long *partials;
};

GvWork gv_work(void *work, int64_t n, int32_t Mmax) {
    GvWork w;
    w.cols = (double *)work;
    w.d = w.cols + (int64_t)Mmax * n;
    w.partials = (long long *)(w.d + n);
    return w;
}

int gv_step_grid(int64_t n) {
    const int64_t tiles = agpl_cdiv(n, kGvTile);
    return (int)(tiles < kGvPartials ? tiles : kGvPartials);
}

int gv_fill_grid(int64_t n) {
    const int64_t b = agpl_cdiv(n, 256);
    return (int)(b < 2048 ? (b < 1 ? 1 : b) : 2048);
}

int32_t gv_check_range(agpl_ctx *ctx, int64_t N_total, int64_t i0, int64_t n, int32_t Mmax, int32_t D, const void *x,
                       const void *work, int64_t work_bytes) {
    if (D < 1 || D > kGvMaxD) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "the input dimension must be 1 ... 16 (got %d)", D);
    if (Mmax < 1 || Mmax > kGvMaxM)
        AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "the number of inducing inputs must be 1 ... 2048 (got %d)", Mmax);
    if (N_total < 1 || N_total >= ((int64_t)1 << 48))
        AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "N_total must be in [1, 2^48) (got %lld)", (long long)N_total);
    if (i0 < 0 || n < 0 || i0 + n > N_total)
        AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "the range [%lld, %lld) is not inside the %lld points", (long long)i0,
                  (long long)(i0 + n), (long long)N_total);
    if (!work || (n > 0 && !x)) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "null argument");
    if (work_bytes < gv_bytes(n, Mmax))
        AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "the work area has %lld bytes, agpl_greedy_bytes(%lld, %d) = %lld", (long long)work_bytes,
                  (long long)n, Mmax, (long long)gv_bytes(n, Mmax));
    return AGPL_OK;
}

// the one dispatch of the step kernel on whether the kind's distance is warped
template <typename... Args>
void gv_launch_step(agpl_ctx *ctx, int grid, int64_t n, int64_t i0, int D, int kind, Args... args) {
    if (agpl::kernel_kind_warps(kind) || agpl::kernel_kind_modulated(kind))
        gv_step_kernel<true><<<grid, kGvThreads, 0, ctx->stream>>>(n, i0, D, kind, args...);
    else
        gv_step_kernel<false><<<grid, kGvThreads, 0, ctx->stream>>>(n, i0, D, kind, args...);
}

int32_t gv_check_variance(agpl_ctx *ctx, double variance) {
    if (!(variance > 0.0 && variance <= 1.79e308))
        AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "variance must be positive and finite (got %g)", variance);
    return AGPL_OK;
}

int32_t gv_check_kernel(agpl_ctx *ctx, int32_t D, int32_t kind, double param, const double *lengthscale, GvEll *out) {
    if (!agpl::kernel_kind_known(kind)) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "unknown kernel kind %d", kind);
    if (const char *what = agpl::kernel_param_refused(kind, param, 1.79e308, true))
        AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "%s must be positive and finite (got %g)", what, param);
    if (!lengthscale) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "null argument");
    for (int e = 0; e < kGvMaxD; ++e) out->v[e] = 1.0;
    for (int e = 0; e < D; ++e) {
        if (!(lengthscale[e] > 0.0 && lengthscale[e] <= 1.79e308))
            AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "lengthscale[%d] must be positive and finite", e);
        out->v[e] = lengthscale[e];
    }
    return AGPL_OK;
}

double gv_tscale(int64_t N_total) { return ldexp(1.0, 61 - gv_ceil_log2(N_total)); }

GvSel gv_no_sel() {
    GvSel s;
    memset(&s, 0, sizeof(s));
    return s;
}

} // namespace

extern "C" int32_t agpl_greedy_bytes(int64_t n, int32_t Mmax, int64_t *bytes_out) {
    if (!bytes_out || n < 0 || n >= ((int64_t)1 << 48) || Mmax < 1 || Mmax > kGvMaxM) return AGPL_ERR_INVALID_ARGUMENT;
    *bytes_out = gv_bytes(n, Mmax);
    return AGPL_OK;
}

extern "C" int32_t agpl_greedy_begin(agpl_ctx *ctx, int64_t N_total, int64_t i0, int64_t n, int32_t Mmax, int32_t D,
                                     const double *x_local, double variance, void *work, int64_t work_bytes, int64_t *cand_out) {
    if (!ctx) return AGPL_ERR_INVALID_ARGUMENT;
    int32_t rc = gv_check_range(ctx, N_total, i0, n, Mmax, D, x_local, work, work_bytes);
    if (rc) return rc;
    rc = gv_check_variance(ctx, variance);
    if (rc) return rc;
    if (!cand_out) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "null argument");
    const GvWork w = gv_work(work, n, Mmax);
    long long *cand = reinterpret_cast<long long *>(cand_out);
    if (n == 0) {
        gv_pick_kernel<<<1, kGvThreads, 0, ctx->stream>>>(0, w.partials, i0, cand, gv_no_sel());
        AGPL_LAUNCH_CHECK(ctx);
        return AGPL_OK;
    }
    unsigned long long *word = nullptr;
    if (hipMalloc((void **)&word, sizeof(unsigned long long)) != hipSuccess) {
        (void)hipGetLastError();
        AGPL_FAIL(ctx, AGPL_ERR_OUT_OF_MEMORY, "hipMalloc for the status word failed");
    }
    unsigned long long hw = ~0ull;
    hipError_t e = hipMemsetAsync(word, 0xff, sizeof(hw), ctx->stream);
    if (e == hipSuccess) {
        gv_begin_kernel<<<gv_fill_grid(n), 256, 0, ctx->stream>>>(n, D, x_local, variance, w.d, w.partials, word);
        gv_pick_kernel<<<1, kGvThreads, 0, ctx->stream>>>(1, w.partials, i0, cand, gv_no_sel());
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&hw, word, sizeof(hw), hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t es = hipStreamSynchronize(ctx->stream);
    (void)hipFree(word);
    if (e != hipSuccess || es != hipSuccess)
        AGPL_FAIL(ctx, AGPL_ERR_HIP, "greedy selection, start: %s", hipGetErrorString(e != hipSuccess ? e : es));
    if (hw != ~0ull) AGPL_FAIL(ctx, AGPL_ERR_DOMAIN, "input x[%llu] is not finite", hw);
    return AGPL_OK;
}

extern "C" int32_t agpl_greedy_pivot(agpl_ctx *ctx, int64_t N_total, int64_t i0, int64_t n, int32_t Mmax, int32_t D, int32_t j,
                                     const double *x_local, const void *work, int64_t work_bytes, const int64_t *index,
                                     double *pivot_out) {
    if (!ctx) return AGPL_ERR_INVALID_ARGUMENT;
    const int32_t rc = gv_check_range(ctx, N_total, i0, n, Mmax, D, x_local, work, work_bytes);
    if (rc) return rc;
    if (j < 0 || j >= Mmax) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "step %d is not in [0, %d)", j, Mmax);
    if (!index || !pivot_out) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "null argument");
    const GvWork w = gv_work(const_cast<void *>(work), n, Mmax);
    gv_pivot_kernel<<<(unsigned)agpl_cdiv(D + 1 + j, 256), 256, 0, ctx->stream>>>(n, i0, D, j, x_local, w.cols, w.d,
                                                                                  reinterpret_cast<const long long *>(index), pivot_out);
    AGPL_LAUNCH_CHECK(ctx);
    return AGPL_OK;
}

extern "C" int32_t agpl_greedy_step(agpl_ctx *ctx, int64_t N_total, int64_t i0, int64_t n, int32_t Mmax, int32_t D, int32_t kind,
                                    double param, int32_t j, const double *x_local, const double *lengthscale, double variance,
                                    const int64_t *index, const double *pivot, void *work, int64_t work_bytes, int64_t *cand_out,
                                    int64_t *trace_acc) {
    if (!ctx) return AGPL_ERR_INVALID_ARGUMENT;
    int32_t rc = gv_check_range(ctx, N_total, i0, n, Mmax, D, x_local, work, work_bytes);
    if (rc) return rc;
    GvEll ell;
    rc = gv_check_kernel(ctx, D, kind, param, lengthscale, &ell);
    if (rc) return rc;
    rc = gv_check_variance(ctx, variance);
    if (rc) return rc;
    if (j < 0 || j >= Mmax) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "step %d is not in [0, %d)", j, Mmax);
    if (!index || !pivot || !cand_out || !trace_acc) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "null argument");
    const GvWork w = gv_work(work, n, Mmax);
    const int grid = n > 0 ? gv_step_grid(n) : 0;
    if (n > 0)
        gv_launch_step(ctx, grid, n, i0, D, kind, param, j, x_local, ell, variance, gv_tscale(N_total),
                       reinterpret_cast<const long long *>(index), pivot, w.cols, w.d, w.partials,
                       reinterpret_cast<unsigned long long *>(trace_acc) + j, nullptr);
    gv_pick_kernel<<<1, kGvThreads, 0, ctx->stream>>>(grid, w.partials, i0, reinterpret_cast<long long *>(cand_out), gv_no_sel());
    AGPL_LAUNCH_CHECK(ctx);
    return AGPL_OK;
}

extern "C" int32_t agpl_select_inducing_greedy(agpl_ctx *ctx, int64_t N, int32_t M, int32_t D, int32_t kind, double param,
                                               const double *x, const double *lengthscale, double variance, double threshold,
                                               void *work, int64_t work_bytes, double *z_out, int64_t *idx_out, double *info_out) {
    if (!ctx) return AGPL_ERR_INVALID_ARGUMENT;
    if (N < 1) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "N must be in [1, 2^48) (got %lld)", (long long)N);
    int32_t rc = gv_check_range(ctx, N, 0, N, M, D, x, work, work_bytes);
    if (rc) return rc;
    GvEll ell;
    rc = gv_check_kernel(ctx, D, kind, param, lengthscale, &ell);
    if (rc) return rc;
    rc = gv_check_variance(ctx, variance);
    if (rc) return rc;
    if (!(threshold >= 1e-12 && threshold < 1.0))
        AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "threshold must be in [1e-12, 1) (got %g)", threshold);
    if (!z_out || !idx_out || !info_out) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "null argument");
    // one block: trace_acc [M] | the status word | the pivot's index | the end flag (8 bytes) | the pivot record [D + 1 + M]
    const size_t small = sizeof(int64_t) * ((size_t)M + 3) + sizeof(double) * ((size_t)D + 1 + M);
    char *s = nullptr;
    if (hipMalloc((void **)&s, small) != hipSuccess) {
        (void)hipGetLastError();
        AGPL_FAIL(ctx, AGPL_ERR_OUT_OF_MEMORY, "hipMalloc(%zu) for the selection's state failed", small);
    }
    long long *trace = (long long *)s;
    unsigned long long *word = (unsigned long long *)(trace + M);
    long long *index = (long long *)(word + 1);
    int *done = (int *)(index + 1);
    double *pivot = (double *)(index + 2);
    const GvWork w = gv_work(work, N, M);
    unsigned long long hw = ~0ull;
    auto fail = [&](int32_t code) {
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipFree(s);
        return code;
    };
#define AGPL_GV_TRY(call_)                                                                                          \
    do {                                                                                                             \
        const hipError_t e_ = (call_);                                                                               \
        if (e_ != hipSuccess) {                                                                                      \
            snprintf(ctx->err, sizeof(ctx->err), "greedy selection: %s failed: %s", #call_, hipGetErrorString(e_)); \
            return fail(AGPL_ERR_HIP);                                                                               \
        }                                                                                                            \
    } while (0)
    AGPL_GV_TRY(hipMemsetAsync(s, 0, small, ctx->stream));
    AGPL_GV_TRY(hipMemsetAsync(word, 0xff, sizeof(hw), ctx->stream));
    AGPL_GV_TRY(hipMemsetAsync(z_out, 0, sizeof(double) * (size_t)M * D, ctx->stream));
    AGPL_GV_TRY(hipMemsetAsync(idx_out, 0, sizeof(int64_t) * (size_t)M, ctx->stream));
    AGPL_GV_TRY(hipMemsetAsync(info_out, 0, sizeof(double) * (1 + 2 * (size_t)M), ctx->stream));
    gv_begin_kernel<<<gv_fill_grid(N), 256, 0, ctx->stream>>>(N, D, x, variance, w.d, w.partials, word);
    AGPL_GV_TRY(hipGetLastError());
    GvSel sel;
    sel.done = done;
    sel.index = index;
    sel.pivot = pivot;
    sel.z_out = z_out;
    sel.info = info_out;
    sel.idx_out = reinterpret_cast<long long *>(idx_out);
    sel.x = x;
    sel.cols = w.cols;
    sel.n = N;
    sel.D = D;
    sel.variance = variance;
    sel.threshold = threshold;
    const int grid = gv_step_grid(N);
    const double tscale = gv_tscale(N);
    for (int j = 0; j < M; ++j) {
        sel.j = j;
        gv_pick_kernel<<<1, kGvThreads, 0, ctx->stream>>>(j == 0 ? 1 : grid, w.partials, 0, nullptr, sel);
        gv_launch_step(ctx, grid, N, 0, D, kind, param, j, x, ell, variance, tscale, index, pivot, w.cols, w.d, w.partials,
                       reinterpret_cast<unsigned long long *>(trace) + j, done);
        AGPL_GV_TRY(hipGetLastError());
    }
    gv_trace_kernel<<<(unsigned)agpl_cdiv(M, 256), 256, 0, ctx->stream>>>(M, 1.0 / tscale, trace, info_out);
    AGPL_GV_TRY(hipGetLastError());
    AGPL_GV_TRY(hipMemcpyAsync(&hw, word, sizeof(hw), hipMemcpyDeviceToHost, ctx->stream));
#undef AGPL_GV_TRY
    const hipError_t es = hipStreamSynchronize(ctx->stream);
    (void)hipFree(s);
    if (es != hipSuccess) AGPL_FAIL(ctx, AGPL_ERR_HIP, "greedy selection: %s", hipGetErrorString(es));
    if (hw != ~0ull) AGPL_FAIL(ctx, AGPL_ERR_DOMAIN, "input x[%llu] is not finite", hw);
    return AGPL_OK;
}
