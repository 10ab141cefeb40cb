// agpl_ws2.h -- the map of the context's small workspace (ctx->ws2), stated once: a fixed head whose regions live across calls, then a
// tail that each call carves for itself.  No HIP dependency: tests/test_ws2_layout_cpu.py compiles this header with g++.  The typed
// accessors over agpl_ctx (agpl_ws2_queues(ctx), ...) are beside the context in agpl_common.h; nothing else adds to ctx->ws2.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace agpl {
// ---- the head: [offset, offset + bytes) of every region ---------------------------------------------------------------------------
constexpr size_t kWs2Result = 0, kWs2ResultBytes = 8;   // the ELBO reductions' result (double); the sampler's / Gibbs pass's `bad` (int)
constexpr size_t kWs2Range = 8, kWs2RangeBytes = 24;    // range check: max |Phi| (word 0), the first bad feature (8 bytes at + 8)
constexpr size_t kWs2PlanBad = 32, kWs2PlanBadBytes = 8; // agpl_plan_create: the first bad residual (bytes 40..63 are nobody's)
constexpr size_t kWs2Partials = 64, kWs2PartialsBytes = 8128; // the reduction partials, one double per workgroup
constexpr int kRedParts = (int)(kWs2PartialsBytes / sizeof(double));
// zero between launches: the kernels that use these words leave them zero again (no memset per sweep); a fresh allocation is zeroed
constexpr size_t kWs2Zero = 8192, kWs2ZeroBytes = 8192;
constexpr int kWs2QueueWords = 8; // the marginal pass's item queues, one per XCD
constexpr size_t kWs2Queues = kWs2Zero, kWs2QueuesBytes = sizeof(unsigned) * kWs2QueueWords;
// the sweep's bad-gamma word: NOT zero between launches -- it waits for the update that forwards it.  It sits behind the queues because
// the per-point kernel takes one pointer for both: word kWs2BadGammaWord from the queues.
constexpr int kWs2BadGammaWord = kWs2QueueWords;
constexpr size_t kWs2BadGamma = kWs2Queues + sizeof(unsigned) * kWs2BadGammaWord, kWs2BadGammaBytes = sizeof(unsigned);
// the factorisation's hand-off flags: 32 PipeFlags records (factor_pipe_kernel) or four words per latent (factor_kernel), asserted in
// agpl_factor.hip; the rescue launch clears all kWs2FlagWords of them
constexpr size_t kWs2Flags = 8448, kWs2FlagsBytes = 7936;
constexpr int kWs2FlagWords = (int)(kWs2FlagsBytes / sizeof(unsigned));
// the head's size: what every allocation has at least and what moves with a reallocation (agpl_ws2_reserve)
constexpr size_t kWs2Head = 16384;

// the regions in ascending order, none reaching the next: pairwise disjoint, all inside the head
static_assert(kWs2Result + kWs2ResultBytes <= kWs2Range && kWs2Range + kWs2RangeBytes <= kWs2PlanBad &&
                  kWs2PlanBad + kWs2PlanBadBytes <= kWs2Partials && kWs2Partials + kWs2PartialsBytes <= kWs2Queues &&
                  kWs2Queues + kWs2QueuesBytes <= kWs2BadGamma && kWs2BadGamma + kWs2BadGammaBytes <= kWs2Flags &&
                  kWs2Flags + kWs2FlagsBytes <= kWs2Head,
              "regions of the small workspace's head overlap");
constexpr bool ws2_within(size_t a, size_t na, size_t b, size_t nb) { return b <= a && a + na <= b + nb; }
static_assert(ws2_within(kWs2Zero, kWs2ZeroBytes, 0, kWs2Head) && ws2_within(kWs2Queues, kWs2QueuesBytes, kWs2Zero, kWs2ZeroBytes) &&
                  ws2_within(kWs2Flags, kWs2FlagsBytes, kWs2Zero, kWs2ZeroBytes),
              "what must be zero between launches lies in the one zero range of the head");
static_assert(kWs2Range % 8 == 0 && kWs2PlanBad % 8 == 0 && kWs2Partials % 8 == 0 && kWs2Flags % 256 == 0, "alignment of the head");
} // namespace agpl

// ---- the hand-written factorisation's feature counts (agpl_factor.hip; beyond 1024 agpl_factor_two_block) -------------------------
// it takes a multiple of 32 up to 512, of 128 up to 2048, and at most 64 latents; everything else goes to rocSOLVER
inline bool agpl_factor_takes(int32_t M, int32_t L) { return M % 32 == 0 && L <= 64 && (M <= 512 || (M <= 2048 && M % 128 == 0)); }
// the next count it takes (zero features change nothing: agpl_gibbs_draw_v pads to it); M itself beyond 2048
inline int32_t agpl_factor_pad_m(int32_t M) { return M <= 512 ? (M + 31) / 32 * 32 : (M <= 2048 ? (M + 127) / 128 * 128 : M); }

// ---- the tail: one layout per user, byte offsets from ctx->ws2, every one a multiple of 256; `total` is what the call reserves.  The
// members are carved in the order they are declared (a braced list is evaluated left to right); a region of no bytes takes none.
struct agpl_ws2_carve {
    size_t at = agpl::kWs2Head;
    size_t take(size_t bytes) { const size_t o = at; at += (bytes + 255) & ~(size_t)255; return o; }
};
// the info words of a factorisation: one int per latent from the hand-written kernels, a (potrf, second call) pair from rocSOLVER
inline size_t agpl_ws2_info_bytes(int32_t L, bool hand) { return sizeof(int32_t) * (size_t)(hand ? L : 2 * L); }
inline size_t agpl_ws2_mat_bytes(int32_t M, int32_t L) { return sizeof(double) * (size_t)L * M * M; }

// agpl_gaussian_update.  hand (agpl_factor_takes(M, L)): T, A (the factor), Uz (its clean copy), S and `work` (work_bytes for the factor
// kernels); the library route: S alone (potrf / potri in place).  own_S: the caller gave no S_out
struct agpl_ws2_update_layout { size_t info, T, A, Uz, S, work, total; };
inline agpl_ws2_update_layout agpl_ws2_update(int32_t M, int32_t L, bool hand, bool own_S, size_t work_bytes) {
    agpl_ws2_carve c;
    const size_t mat = agpl_ws2_mat_bytes(M, L), hmat = hand ? mat : 0;
    return {c.take(agpl_ws2_info_bytes(L, hand)), c.take(hmat), c.take(hmat), c.take(hmat), c.take(own_S ? mat : 0),
            c.take(hand ? work_bytes : 0), c.at};
}
// agpl_gaussian_factor and the plan's update: the factor goes to the caller's A_work
struct agpl_ws2_factor_layout { size_t info, T, work, total; };
inline agpl_ws2_factor_layout agpl_ws2_factor(int32_t M, int32_t L, bool hand, size_t work_bytes) {
    agpl_ws2_carve c;
    return {c.take(agpl_ws2_info_bytes(L, hand)), c.take(hand ? agpl_ws2_mat_bytes(M, L) : 0), c.take(hand ? work_bytes : 0), c.at};
}
// agpl_gibbs_draw_v at Mf = agpl_factor_pad_m(M).  hand (agpl_factor_takes(Mf, L)): T, A, vf = U r and the draw z at Mf, and for
// Mf != M the zero-padded G, g, eta0; the library route: A, vf (there m) and z at M
struct agpl_ws2_draw_layout { int32_t Mf; bool hand; size_t info, T, A, vf, z, work, Gp, gp, ep, total; };
inline agpl_ws2_draw_layout agpl_ws2_draw(int32_t M, int32_t L, size_t work_bytes) {
    agpl_ws2_carve c;
    const int32_t Mf = agpl_factor_pad_m(M);
    const bool hand = agpl_factor_takes(Mf, L), pad = hand && Mf != M;
    const size_t mat = agpl_ws2_mat_bytes(hand ? Mf : M, L), vec = sizeof(double) * (size_t)L * (hand ? Mf : M);
    return {Mf, hand, c.take(agpl_ws2_info_bytes(L, hand)), c.take(hand ? mat : 0), c.take(mat), c.take(vec), c.take(vec),
            c.take(hand ? work_bytes : 0), c.take(pad ? mat : 0), c.take(pad ? vec : 0), c.take(pad ? vec : 0), c.at};
}
// the dense Cholesky (agpl_dense.hip): two info words and the 64 x 64 block of own_block_potrf
struct agpl_ws2_dense_layout { size_t info, Ubuf, total; };
inline agpl_ws2_dense_layout agpl_ws2_dense() {
    agpl_ws2_carve c;
    return {c.take(2 * sizeof(int32_t)), c.take(sizeof(double) * 64 * 64), c.at};
}
