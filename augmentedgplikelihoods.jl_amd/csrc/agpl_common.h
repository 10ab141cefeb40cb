// agpl_common.h -- context, error plumbing and small device helpers shared by the libagpl.so sources.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <utility>
#include <vector>

#include "../../include/agpl.h"

struct rocblas_handle_s; // fwd (rocblas_handle is a pointer to an opaque struct)

struct agpl_ctx {
    int device = 0;
    uint64_t seed = 0;
    int64_t point_offset = 0; // global index of local point 0 (agpl_ctx_set_point_offset): per-point Philox streams
                              // are keyed on point_offset + i, so that N sharded over ranks draws what one rank would
    hipStream_t stream = nullptr;
    bool own_stream = false;
    void *rocblas = nullptr; // rocblas_handle, created lazily by agpl_update.hip
    hipStream_t aux_stream = nullptr; // high-priority side stream of the dense Cholesky's look-ahead (agpl_dense.hip), lazily created
    hipEvent_t aux_ev[2] = {nullptr, nullptr};
    // scratch (lazily grown)
    void *ws = nullptr;
    size_t ws_bytes = 0;
    void *ws2 = nullptr; // small persistent scratch: the map is agpl_ws2.h, the accessors are below
    size_t ws2_bytes = 0;
    unsigned *pg_retry = nullptr; // PG(1) kernels: [0] entries, [1] workgroups done (both zero between launches), [2 ..] the point list
    size_t pg_retry_entries = 0;
    unsigned *red_cnt = nullptr; // arrival counters of the slab reduction (one per 1 KB of G and per half block of g), zero between launches
    size_t red_cnt_entries = 0;
    double *logtheta_dev = nullptr; // categorical link parameters mirrored on device
    int logtheta_cap = 0;
    double logtheta_host[128];      // last uploaded values (skip the copy when unchanged)
    int logtheta_n = 0;
    // optional kernel timing (agpl_timing_*): event pairs per kernel family
    int ncu = 0;              // compute units of `device` (queried once, by the first queue-served launch)
    int strip_attr = 0;       // the accumulation kernels' dynamic-LDS attributes are set (once)
    int queue_attr = 0;       // marginal_factor_queue_kernel's dynamic-LDS attribute is set (once)
    int pipe_attr = 0;        // factor_pipe_kernel's dynamic-LDS attribute is set (once)
    const void *checked_image = nullptr; // the accumulate image whose header agpl_syrk_image_launch has validated last, and for which (N, M)
    int64_t checked_image_N = 0;
    int32_t checked_image_M = 0;
    double *elbo_part = nullptr;  // per-workgroup partial sums of the ELBO terms that ride the per-point kernel (1024 doubles)
    int live_plans = 0;           // agpl_plan objects created on this context and not yet destroyed (agpl_ctx_destroy refuses while > 0)
    bool debug_force_rescue = false; // agpl_debug_force_factor_rescue (test hook)
    bool timing = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev[4]; // 0 marginal, 1 syrk, 2 gibbs point pass, 3 aux_sample
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
    // deferred outcome of the last agpl_gaussian_factor_async: info words in pinned host memory, ready once the event
    // has passed (agpl_pending_resolve waits for the event only, not for work enqueued behind it)
    bool pend = false;
    int pend_n = 0;          // info words (one per latent)
    int pend_latents = 0;
    int *pend_host = nullptr; // hipHostMalloc (mapped), 128 ints
    bool pend_gamma_word = false; // pend_host[127] carries the sweep's bad-gamma word
    int *pend_host_dev = nullptr; // the same memory as the device addresses it
    hipEvent_t pend_ev = nullptr;
    char err[512] = {0};
};

#include "agpl_slices.h" // agpl_slice_plan / agpl_slice_range: how one accumulation cuts N into slices (host-testable, no HIP)
#include "agpl_ws2.h"    // the map of ctx->ws2: the head's regions and the layouts of the tail (host-testable, no HIP)

// the typed view of ctx->ws2: one accessor per region of the head, and agpl_ws2_at for the offsets of a tail layout
template <typename T> inline T *agpl_ws2_at(agpl_ctx *ctx, size_t offset) { return (T *)((char *)ctx->ws2 + offset); }
inline double *agpl_ws2_result(agpl_ctx *ctx) { return agpl_ws2_at<double>(ctx, agpl::kWs2Result); }
inline int *agpl_ws2_bad(agpl_ctx *ctx) { return agpl_ws2_at<int>(ctx, agpl::kWs2Result); }
inline unsigned *agpl_ws2_range(agpl_ctx *ctx) { return agpl_ws2_at<unsigned>(ctx, agpl::kWs2Range); }
inline unsigned long long *agpl_ws2_plan_bad(agpl_ctx *ctx) { return agpl_ws2_at<unsigned long long>(ctx, agpl::kWs2PlanBad); }
inline double *agpl_ws2_partials(agpl_ctx *ctx) { return agpl_ws2_at<double>(ctx, agpl::kWs2Partials); }
inline unsigned *agpl_ws2_queues(agpl_ctx *ctx) { return agpl_ws2_at<unsigned>(ctx, agpl::kWs2Queues); }
inline unsigned *agpl_ws2_bad_gamma(agpl_ctx *ctx) { return agpl_ws2_at<unsigned>(ctx, agpl::kWs2BadGamma); }
inline unsigned *agpl_ws2_factor_flags(agpl_ctx *ctx) { return agpl_ws2_at<unsigned>(ctx, agpl::kWs2Flags); }

// reports (and clears) the deferred outcome of the last asynchronous factorisation; AGPL_OK when none is pending
int32_t agpl_pending_resolve(agpl_ctx *ctx);

// RAII-less helpers: record a start event now, and the matching stop event after the launch
int32_t agpl_timing_begin(agpl_ctx *ctx, int which);
int32_t agpl_timing_end(agpl_ctx *ctx, int which);

#define AGPL_FAIL(ctx, code, ...)                                   \
    do {                                                            \
        if (ctx) snprintf((ctx)->err, sizeof((ctx)->err), __VA_ARGS__); \
        return (code);                                              \
    } while (0)

#define AGPL_HIP(ctx, call)                                                                   \
    do {                                                                                      \
        hipError_t e__ = (call);                                                              \
        if (e__ != hipSuccess)                                                                \
            AGPL_FAIL(ctx, AGPL_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), \
                      __FILE__, __LINE__);                                                    \
    } while (0)

#define AGPL_LAUNCH_CHECK(ctx)                                                              \
    do {                                                                                    \
        hipError_t e__ = hipGetLastError();                                                 \
        if (e__ != hipSuccess)                                                              \
            AGPL_FAIL(ctx, AGPL_ERR_HIP, "kernel launch failed: %s (%s:%d)",                \
                      hipGetErrorString(e__), __FILE__, __LINE__);                          \
    } while (0)

// grow-only scratch
int32_t agpl_ws_reserve(agpl_ctx *ctx, size_t bytes);
int32_t agpl_ws2_reserve(agpl_ctx *ctx, size_t bytes);
int32_t agpl_red_cnt_reserve(agpl_ctx *ctx, int64_t n); // the slab reduction's arrival counters (agpl_core.hip)
int32_t agpl_pg_retry_reserve(agpl_ctx *ctx, int64_t n); // the retry list of the PG(1) kernels for n points (agpl_core.hip)

// device-side view of a likelihood descriptor (logtheta mirrored to device memory)
struct agpl_lik_dev {
    int32_t kind;
    int32_t nlatent;
    double p[4];
    const double *logtheta; // device
    double sum_theta;       // categorical.jl:16-20
    double cat_const;       // categorical.jl:12-14 (bijective only)
};
int32_t agpl_lik_to_device(agpl_ctx *ctx, const agpl_lik_desc *lik, agpl_lik_dev *out); // (checks the descriptor first)

#include "agpl_lik_desc.h" // the list of kinds, the descriptor check, the host switch over the kind (host-testable, no HIP)

// the descriptor check of agpl_lik_desc.h for an entry point: the message goes to the context, a refusal ends the call
#define AGPL_LIK_CHECK(ctx, lik)                                                                             \
    do {                                                                                                     \
        const int32_t rc__ = agpl_lik_desc_check((lik), (ctx) ? (ctx)->err : nullptr, sizeof((ctx)->err));   \
        if (rc__ != AGPL_OK) return rc__;                                                                    \
    } while (0)

// trials of one point of the per-point binomial kind (agpl.h, AGPL_LIK_BINOMIAL_N), stated once for every source that reads column 1
// of its y [N][2]: NaN outside 1 <= n < 2^22, so that the point's outputs are NaN
namespace agpl {
template <typename T>
__host__ __device__ __forceinline__ T binomial_trials(T n) { return (n >= T(1) && n < T(4194304)) ? n : T(__builtin_nan("")); }
} // namespace agpl

// bytes of the plan's two kinds of image (layouts: agpl_split.hip, agpl_syrk.hip)
// ONE marginal image (hi or lo): N points in 128-point tiles, M features (M % 128 == 0)
static inline int64_t agpl_split_features_bytes(int64_t N, int32_t M) {
    if (N <= 0 || M <= 0 || M % 128) return 0;
    return (int64_t)sizeof(_Float16) * ((N + 127) / 128) * 128 * M;
}
// the accumulate image: 256-byte header + 4 KB blocks (16-point slice x 128 features x hi | lo) over whole 32-point stages
static inline int64_t agpl_accumulate_image_bytes(int64_t N, int32_t M) {
    if (N <= 0 || M <= 0 || M % 128) return 0;
    const int64_t nps = ((N + 31) / 32) * 2;
    return 256 + nps * (M / 128) * 2 * 4096;
}

static inline int64_t agpl_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
