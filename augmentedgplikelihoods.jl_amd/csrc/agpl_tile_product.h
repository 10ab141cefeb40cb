// agpl_tile_product.h -- the 128 x 128 split-float16 tile product of the extension libraries, stated once for the kernels that
// project images "at new inputs": chain_project_kernel (agpl_chain.hip), joint_t_kernel and joint_cov_kernel (agpl_joint.hip),
// pw_project_kernel (agpl_pathwise.hip) and hy_points_kernel (agpl_hyper_impl.h).  Both operands are images in the blocked layout of
// agpl_split.hip: blocks (tile of 128 rows, k-slice of 16) = [plane 2][row 128][8 halves], one h8 per thread of a 256-thread
// workgroup.  Four waves, 64 rows of A x 64 rows of B each; two k-slices per stage through LDS, register-staged double buffer;
// hi hi + hi lo + lo hi on v_mfma_f32_32x32x16_f16, float32 accumulation.  What differs per library stays there: where slice k of
// the operands comes from (the loader), how many stages run, which rows are live, and the epilogue that reads the tile back.
// A kernel forms its lane indices itself, ahead of its loops (tid = threadIdx.x; lane = tid & 63, wave = tid >> 6; wr = wave >> 1,
// wc = wave & 1: the wave's 64 rows of A and of B; li = lane & 31, lk = lane >> 5; fa = lk 128 + wr 64 + li and
// fb = 512 + lk 128 + wc 64 + li: the h8 index of its A hi / B hi fragment in a staged slice, lo at + 256).
// Beside it: the scale exponent of a packed operand and the float -> (hi, lo) float16 split of the pack kernels.
// Internal: every including source gets its own copy (anonymous namespace).
#pragma once
#include "agpl_se_build.h"

namespace {

constexpr int KU = 2;                  // k-slices per stage
constexpr int kSliceH8 = 4 * 256;      // one slice in LDS: A hi | A lo | B hi | B lo, 4 KB each
constexpr int kStageH8 = KU * kSliceH8;
constexpr int kStageBytes = 2 * kStageH8 * 16; // two stages = 64 KB = the [128][128] float32 epilogue tile
static_assert(kStageBytes == BS * BS * 4, "the epilogue tile reuses the two stage buffers");
static_assert(KT == 16, "k-slices of 16 features (the blocked images' slice)");

__device__ __forceinline__ f32x16 mfma16(h8 a, h8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }

// e with 2^e mx in [2^13, 2^14), within +-90 (0 for mx = 0 or a non-finite mx: the callers refuse or never meet such an operand)
__device__ __forceinline__ int tile_scale_exp(double mx) {
    if (!(mx > 0.0 && mx <= 1.79e308)) return 0;
    const int e = 13 - ilogb(mx);
    return e > 90 ? 90 : (e < -90 ? -90 : e);
}

// hi[j] + lo[j] <- xf as two float16: the nearest half and the nearest half of what it leaves.  One element of a pack kernel's
// 8-wide loop; the arithmetic that forms xf is the caller's.
__device__ __forceinline__ void tile_split(h8 &hi, h8 &lo, int j, float xf) {
    const _Float16 h = (_Float16)xf;
    hi[j] = h;
    lo[j] = (_Float16)(xf - (float)h);
}

// acc[ii][jj] <- sum over nst stages (2 nst k-slices) of (rows of A) x (rows of B).  load(k, rg): this thread's h8 of slice k as
// rg[0 .. 3] = A hi, A lo, B hi, B lo (a slice past the operands' last one: zeros).  st: the two stage buffers; fa, fb: above.
// MASKED: only the rows of A that carry anything are multiplied -- act1: all 64 rows of this wave, else act0: its rows 0 .. 31,
// else none (uniform over the wave).  SYNC_FIRST: a barrier before the first store, for a caller whose LDS may still be read.
// Ends behind a barrier: the stage buffers are free for the epilogue tile.
template <bool MASKED, bool SYNC_FIRST, typename Load>
__device__ __forceinline__ void tile_product(Load &&load, int nst, h8 *st, int tid, int fa, int fb, f32x16 (&acc)[2][2], bool act0 = true,
                                             bool act1 = true) {
#pragma unroll
    for (int ii = 0; ii < 2; ++ii)
#pragma unroll
        for (int jj = 0; jj < 2; ++jj)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[ii][jj][r] = 0.f;
    h8 rg[KU][4];
#pragma unroll
    for (int u = 0; u < KU; ++u) load(u, rg[u]); // stage 0
    if constexpr (SYNC_FIRST) __syncthreads();
#pragma unroll
    for (int u = 0; u < KU; ++u)
#pragma unroll
        for (int q = 0; q < 4; ++q) st[u * kSliceH8 + q * 256 + tid] = rg[u][q];
    __syncthreads();
    for (int s = 0; s < nst; ++s) {
        const int buf = s & 1;
        if (s + 1 < nst) {
#pragma unroll
            for (int u = 0; u < KU; ++u) load((s + 1) * KU + u, rg[u]);
        }
#pragma unroll
        for (int u = 0; u < KU; ++u) {
            const h8 *sl = st + buf * kStageH8 + u * kSliceH8;
            if (!MASKED || act1) { // all 64 rows of this wave
                const h8 bh0 = sl[fb], bh1 = sl[fb + 32], ah0 = sl[fa], ah1 = sl[fa + 32];
                acc[0][0] = mfma16(ah0, bh0, acc[0][0]);
                acc[0][1] = mfma16(ah0, bh1, acc[0][1]);
                acc[1][0] = mfma16(ah1, bh0, acc[1][0]);
                acc[1][1] = mfma16(ah1, bh1, acc[1][1]);
                const h8 bl0 = sl[256 + fb], bl1 = sl[256 + fb + 32];
                acc[0][0] = mfma16(ah0, bl0, acc[0][0]);
                acc[0][1] = mfma16(ah0, bl1, acc[0][1]);
                acc[1][0] = mfma16(ah1, bl0, acc[1][0]);
                acc[1][1] = mfma16(ah1, bl1, acc[1][1]);
                const h8 al0 = sl[256 + fa], al1 = sl[256 + fa + 32];
                acc[0][0] = mfma16(al0, bh0, acc[0][0]);
                acc[0][1] = mfma16(al0, bh1, acc[0][1]);
                acc[1][0] = mfma16(al1, bh0, acc[1][0]);
                acc[1][1] = mfma16(al1, bh1, acc[1][1]);
            } else if (act0) { // rows 0 .. 31 only
                const h8 bh0 = sl[fb], bh1 = sl[fb + 32], ah0 = sl[fa];
                const h8 bl0 = sl[256 + fb], bl1 = sl[256 + fb + 32], al0 = sl[256 + fa];
                acc[0][0] = mfma16(ah0, bh0, acc[0][0]);
                acc[0][1] = mfma16(ah0, bh1, acc[0][1]);
                acc[0][0] = mfma16(ah0, bl0, acc[0][0]);
                acc[0][1] = mfma16(ah0, bl1, acc[0][1]);
                acc[0][0] = mfma16(al0, bh0, acc[0][0]);
                acc[0][1] = mfma16(al0, bh1, acc[0][1]);
            }
        }
        if (s + 1 < nst) {
#pragma unroll
            for (int u = 0; u < KU; ++u)
#pragma unroll
                for (int q = 0; q < 4; ++q) st[(buf ^ 1) * kStageH8 + u * kSliceH8 + q * 256 + tid] = rg[u][q];
        }
        __syncthreads();
    }
}

// The plain case: A and B are one 128-row tile each of an image, [slice][plane 2][row 128] h8 (pointers at the tile, + tid)
template <bool MASKED, bool SYNC_FIRST>
__device__ __forceinline__ void tile_product_images(const h8 *__restrict__ ah, const h8 *__restrict__ al, const h8 *__restrict__ bh,
                                                    const h8 *__restrict__ bl, int nst, h8 *st, int tid, int fa, int fb,
                                                    f32x16 (&acc)[2][2], bool act0 = true, bool act1 = true) {
    tile_product<MASKED, SYNC_FIRST>(
        [&](int k, h8(&rg)[4]) __attribute__((always_inline)) {
            rg[0] = ah[k * 256];
            rg[1] = al[k * 256];
            rg[2] = bh[k * 256];
            rg[3] = bl[k * 256];
        },
        nst, st, tid, fa, fb, acc, act0, act1);
}

} // namespace

// E[row][col] (row pitch pitch_ floats: BS, or agpl_joint.hip's EP) <- un_ acc_: this lane holds row wr 64 + ii 32 + 8 g4 + 4 lk +
// (r & 3) of A's tile against row wc 64 + jj 32 + li of B's.  The caller's barrier comes before the tile is read back.
// A macro over the kernel's own wr, wc, li, lk: as a function of those four the scatter compiles to another instruction stream
// (the kernel's wc * 64 + li no longer folds to one mask of threadIdx.x once wc is also an argument).
#define AGPL_TILE_SCATTER(E_, pitch_, un_, acc_)                                                                                    \
    do {                                                                                                                            \
        _Pragma("unroll") for (int ii_ = 0; ii_ < 2; ++ii_)                                                                         \
            _Pragma("unroll") for (int jj_ = 0; jj_ < 2; ++jj_)                                                                     \
                _Pragma("unroll") for (int r_ = 0; r_ < 16; ++r_)                                                                   \
                    (E_)[(wr * 64 + ii_ * 32 + 8 * (r_ >> 2) + 4 * lk + (r_ & 3)) * (pitch_) + wc * 64 + jj_ * 32 + li] =           \
                        (un_) * (acc_)[ii_][jj_][r_];                                                                               \
    } while (0)
