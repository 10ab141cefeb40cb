// agpl_chain.hip -- the posterior of f at new inputs from a chain of inducing draws (agpl_plan_predict_chain, include/agpl_chain.h):
// with Phi* the features of the new points, the per-draw conditional means are ONE product Phi*' V, [Ns x M] . [M x T L], whose left
// operand is the chunk's marginal image that se_build_kernel (agpl_se_build.h) writes, and whose right operand is packed here in the
// same blocked split-float16 layout (agpl_split.hip): blocks (row block of 128, k-slice of 16) = [plane 2][row 128][8 halves].
//
//   chain_mean_kernel     vbar[l][a] = (1/T) sum_t V[t][l][a] in float64 (t ascending); the first draw with a non-finite entry.
//   chain_max_kernel      max |V - vbar| and max |vbar| (integer atomicMax on the bit patterns of non-negative doubles).
//   chain_pack_kernel     row block 0: vbar (rows l < L), scale 2^eb;  row blocks 1 ..: the CENTRED draws v_t - vbar, row t L + l, scale
//                         2^ec;  each 2^e max in [2^13, 2^14) (the images' rule, agpl_syrk.hip); rows past T L and features past M zero.
//                         Writes the two factors that undo the scales (with the point image's 2^e) for the projection.
//   chain_project_kernel  one 128-point tile of the chunk's marginal image per workgroup (4 waves, 64 draws x 64 points each); for each
//                         128-row block of the V image the tile product of agpl_tile_product.h (where the pipeline is stated: two
//                         k-slices per stage through LDS, register-staged double buffer, hi hi + hi lo + lo hi on
//                         v_mfma_f32_32x32x16_f16, float32 accumulation), in its row-masked form.  The 128 x 128 result
//                         goes through LDS once ([draw][point]) and is read back with one thread per point and half block:
//                             block 0  : base[l][n] = mu0 + phi' vbar                          -> mean_out
//                             block >= 1: q = phi' (v_t - vbar);  F_out = base + q (coalesced along the points);  ssq[l][n] += q^2
//                         in ascending t within a half block (rows 0 .. 63 | 64 .. 127 of every block); spread = (ssq0 + ssq1) / T.
//                         No float atomics, no sum depends on the launch: a point's outputs depend on its x and on V alone.
//                         The spread is the mean square of centred projections, never a difference of two sums.
#include "../../include/agpl_chain.h"
#include "agpl_se_build.h"
#include "agpl_tile_product.h"

namespace {

constexpr int64_t kChainChunk = 1 << 16; // points per step (agpl_plan_predict's chunk)

// words[0] <- first draw with a non-finite entry (min); vbar [L Mc]
__global__ __launch_bounds__(256) void chain_mean_kernel(int T, int64_t LM, const double *__restrict__ V, double *__restrict__ vbar,
                                                         unsigned long long *__restrict__ words) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= LM) return;
    double s = 0.0;
    int bad = -1;
    for (int t = 0; t < T; ++t) {
        const double v = V[(int64_t)t * LM + i];
        if (!(fabs(v) <= 1.79e308) && bad < 0) bad = t;
        s += v;
    }
    vbar[i] = s / (double)T;
    if (bad >= 0) atomicMin(&words[0], (unsigned long long)bad);
}

// words[1] <- max |V - vbar|, words[2] <- max |vbar| (bit patterns of non-negative doubles order as the values; NaNs are skipped)
__global__ __launch_bounds__(256) void chain_max_kernel(int T, int64_t LM, const double *__restrict__ V, const double *__restrict__ vbar,
                                                        unsigned long long *__restrict__ words) {
    const int64_t total = (int64_t)T * LM;
    double mc = 0.0, mb = 0.0;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const double b = vbar[e % LM];
        const double c = fabs(V[e] - b);
        mc = c > mc ? c : mc;
        if (e < LM) mb = fabs(b) > mb ? fabs(b) : mb;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double oc = __shfl_xor(mc, o), ob = __shfl_xor(mb, o);
        mc = oc > mc ? oc : mc;
        mb = ob > mb ? ob : mb;
    }
    if ((threadIdx.x & 63) == 0) {
        if (mc > 0.0) atomicMax(&words[1], (unsigned long long)__double_as_longlong(mc));
        if (mb > 0.0) atomicMax(&words[2], (unsigned long long)__double_as_longlong(mb));
    }
}

// grid (Mp / 16 k-slices, 1 + draw blocks); scal[0] = 2^-(e_phi + ec) (centred blocks), scal[1] = 2^-(e_phi + eb) (block 0)
__global__ __launch_bounds__(256) void chain_pack_kernel(int T, int L, int Mc, int Mp, const double *__restrict__ V,
                                                         const double *__restrict__ vbar, const unsigned long long *__restrict__ words,
                                                         int e_phi, h8 *__restrict__ Vh, h8 *__restrict__ Vl, float *__restrict__ scal) {
    const int nks = Mp / KT;
    const int ks = blockIdx.x, rb = blockIdx.y;
    const int plane = threadIdx.x >> 7, row = threadIdx.x & 127;
    const int ec = tile_scale_exp(__longlong_as_double((long long)words[1]));
    const int eb = tile_scale_exp(__longlong_as_double((long long)words[2]));
    if (ks == 0 && rb == 0 && threadIdx.x == 0) {
        scal[0] = ldexpf(1.f, -(e_phi + ec));
        scal[1] = ldexpf(1.f, -(e_phi + eb));
    }
    const double sc = ldexp(1.0, rb ? ec : eb);
    const int64_t g = rb ? (int64_t)(rb - 1) * BS + row : row; // row of V as [T L][Mc]
    const bool valid = rb ? g < (int64_t)T * L : row < L;
    const int l = rb ? (int)(g % L) : row;
    h8 hi, lo;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int a = ks * KT + plane * 8 + j;
        double x = 0.0;
        if (valid && a < Mc) {
            const double b = vbar[(int64_t)l * Mc + a];
            x = (rb ? V[g * Mc + a] - b : b) * sc;
        }
        tile_split(hi, lo, j, (float)x);
    }
    const int64_t o = ((int64_t)rb * nks + ks) * 256 + threadIdx.x;
    Vh[o] = hi;
    Vl[o] = lo;
}

// n: the chunk's points; pitch: Ns (the outputs' row pitch; mu0, mean_out, spread_out, F_out point at the chunk's first point).
// LDS: two stage buffers (reused by the epilogue tile) | base [L][128] | ssq [2][L][128].
__global__ __launch_bounds__(256, 2) void chain_project_kernel(int64_t n, int64_t pitch, int Mp, int T, int L, int nblk,
                                                               const h8 *__restrict__ Ph, const h8 *__restrict__ Pl,
                                                               const h8 *__restrict__ Vh, const h8 *__restrict__ Vl,
                                                               const float *__restrict__ scal, const float *__restrict__ mu0,
                                                               float *__restrict__ mean_out, float *__restrict__ spread_out,
                                                               float *__restrict__ F_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    h8 *st = reinterpret_cast<h8 *>(smem_raw);     // [2][kStageH8]
    float *E = reinterpret_cast<float *>(smem_raw); // [128 draws][128 points]
    float *base_s = reinterpret_cast<float *>(smem_raw + kStageBytes);
    float *ssq_s = base_s + L * BS;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int li = lane & 31, lk = lane >> 5;
    const int nks = Mp / KT, nst = nks / KU;
    const int64_t tile = blockIdx.x;
    const int p = tid & 127, hh = tid >> 7; // epilogue: this thread's point and half block
    const int64_t np = tile * BS + p;
    const bool livep = np < n;
    const int64_t TL = (int64_t)T * L;
    const float unc = scal[0], unb = scal[1];
    const h8 *psrc_h = Ph + tile * nks * 256 + tid, *psrc_l = Pl + tile * nks * 256 + tid;
    const int fa = lk * 128 + wr * 64 + li;       // V hi fragment of rows wr 64 + li (+ 32), plane lk
    const int fb = 512 + lk * 128 + wc * 64 + li; // Phi hi fragment of points wc 64 + li (+ 32)

    for (int rb = 0; rb <= nblk; ++rb) {
        // rows of this block that carry anything: L of block 0, the chain's tail in the last block
        const int rows_live = rb == 0 ? L : (int)(TL - (int64_t)(rb - 1) * BS < BS ? TL - (int64_t)(rb - 1) * BS : BS);
        const bool act0 = wr * 64 < rows_live, act1 = wr * 64 + 32 < rows_live;
        const h8 *vsrc_h = Vh + (int64_t)rb * nks * 256 + tid, *vsrc_l = Vl + (int64_t)rb * nks * 256 + tid;
        f32x16 acc[2][2];
        tile_product_images<true, false>(vsrc_h, vsrc_l, psrc_h, psrc_l, nst, st, tid, fa, fb, acc, act0, act1);
        const float un = rb ? unc : unb;
        AGPL_TILE_SCATTER(E, BS, un, acc); // as [row][point]
        __syncthreads();
        if (rb == 0) {
            for (int l = hh; l < L; l += 2) {
                float b = E[l * BS + p];
                if (mu0 && livep) b += mu0[(int64_t)l * pitch + np];
                base_s[l * BS + p] = b;
                ssq_s[l * BS + p] = 0.f;
                ssq_s[(L + l) * BS + p] = 0.f;
                if (livep) mean_out[(int64_t)l * pitch + np] = b;
            }
        } else {
            const int64_t g0 = (int64_t)(rb - 1) * BS + hh * 64;
            const int cnt = (int)(TL - g0 < 64 ? (TL - g0 < 0 ? 0 : TL - g0) : 64);
            int l = (int)(g0 % L);
            for (int i = 0; i < cnt; ++i) {
                const float q = E[(hh * 64 + i) * BS + p];
                float *sq = ssq_s + (hh * L + l) * BS + p;
                *sq = fmaf(q, q, *sq);
                if (F_out && livep) F_out[(g0 + i) * pitch + np] = base_s[l * BS + p] + q;
                if (++l == L) l = 0;
            }
        }
        __syncthreads();
    }
    for (int l = hh; l < L; l += 2)
        if (livep) spread_out[(int64_t)l * pitch + np] = (ssq_s[l * BS + p] + ssq_s[(L + l) * BS + p]) / (float)T;
}

} // namespace

extern "C" int32_t agpl_plan_predict_chain(agpl_plan *p, int32_t T, const double *V, int64_t Ns, const double *x_s, const float *mu0_s,
                                           float *mean_out, float *spread_out, float *resid_out, float *F_out) {
    if (!p || !p->ctx) return AGPL_ERR_INVALID_ARGUMENT;
    agpl_ctx *ctx = p->ctx;
    if (!p->se) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "agpl_plan_predict_chain needs a plan made by agpl_plan_create_se");
    if (T < 1) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "T = %d: the chain needs at least one draw", T);
    if (Ns < 0) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "Ns = %lld < 0", (long long)Ns);
    if (Ns == 0) return AGPL_OK;
    if (!V || !x_s || !mean_out || !spread_out) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "null argument");
    const int L = p->L, M = p->M, Mc = p->Mc;
    const int64_t TL = (int64_t)T * L, LM = (int64_t)L * Mc;
    const int64_t nblk = agpl_cdiv(TL, BS);
    if (nblk + 1 > 65535) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "T L = %lld rows are too many for one launch", (long long)TL);
    const int64_t C = Ns < kChainChunk ? Ns : kChainChunk;
    const auto al = agpl_align256;
    const size_t img = al((size_t)agpl_split_features_bytes(C, M));           // one plane of the chunk's marginal image
    const size_t vimg = al(sizeof(_Float16) * (size_t)(nblk + 1) * BS * M);    // one plane of the V image
    const size_t rsb = al(sizeof(float) * (size_t)C), vbb = al(sizeof(double) * (size_t)LM);
    const size_t need = 2 * img + rsb + 2 * vimg + vbb + 512;
    if (int32_t rc_ = agpl_pred_reserve(p, need, "prediction")) return rc_; // (every call carves the scratch anew)
    char *w = (char *)p->pred;
    void *Ph = w, *Pl = w + img;
    float *rs = (float *)(w + 2 * img);
    h8 *Vh = (h8 *)(w + 2 * img + rsb), *Vl = (h8 *)(w + 2 * img + rsb + vimg);
    double *vbar = (double *)(w + 2 * img + rsb + 2 * vimg);
    char *tail = w + 2 * img + rsb + 2 * vimg + vbb;
    unsigned long long *words = (unsigned long long *)tail;          // the generator's eight status words (not reported: NaN outputs)
    unsigned *maxbits = (unsigned *)(words + 8);
    unsigned long long *cw = (unsigned long long *)(tail + 256);      // [0] first bad draw, [1] max |V - vbar|, [2] max |vbar|
    float *scal = (float *)(cw + 4);

    // the pass over V: vbar, the scales, the image; the one wait of the call is for its domain check
    AGPL_HIP(ctx, hipMemsetAsync(cw, 0xff, sizeof(unsigned long long), ctx->stream));
    AGPL_HIP(ctx, hipMemsetAsync(cw + 1, 0, 2 * sizeof(unsigned long long), ctx->stream));
    chain_mean_kernel<<<(unsigned)agpl_cdiv(LM, 256), 256, 0, ctx->stream>>>(T, LM, V, vbar, cw);
    AGPL_LAUNCH_CHECK(ctx);
    int64_t nbm = agpl_cdiv((int64_t)T * LM, 256);
    if (nbm > 4096) nbm = 4096;
    chain_max_kernel<<<(unsigned)nbm, 256, 0, ctx->stream>>>(T, LM, V, vbar, cw);
    AGPL_LAUNCH_CHECK(ctx);
    chain_pack_kernel<<<dim3((unsigned)(M / KT), (unsigned)(nblk + 1)), 256, 0, ctx->stream>>>(T, L, Mc, M, V, vbar, cw, p->scale_exp, Vh,
                                                                                              Vl, scal);
    AGPL_LAUNCH_CHECK(ctx);
    unsigned long long bad = ~0ull;
    AGPL_HIP(ctx, hipMemcpyAsync(&bad, cw, sizeof(bad), hipMemcpyDeviceToHost, ctx->stream));
    AGPL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (bad != ~0ull) AGPL_FAIL(ctx, AGPL_ERR_DOMAIN, "draw %llu of the chain has a non-finite entry", bad);

    const size_t lds = (size_t)kStageBytes + sizeof(float) * 3 * (size_t)L * BS;
    AGPL_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&chain_project_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)lds));
    for (int64_t c0 = 0; c0 < Ns; c0 += C) {
        const int64_t n = Ns - c0 < C ? Ns - c0 : C;
        int32_t rc = agpl_se_build(ctx, p->kind, p->kparam, n, M, Mc, p->D, x_s + c0 * p->D, p->zs, p->ell, p->s2, p->Lt, p->scale_exp,
                                   Ph, Pl, nullptr, resid_out ? resid_out + c0 : rs, maxbits, words);
        if (rc) return rc;
        chain_project_kernel<<<(unsigned)agpl_cdiv(n, BS), 256, lds, ctx->stream>>>(
            n, Ns, M, T, L, (int)nblk, (const h8 *)Ph, (const h8 *)Pl, Vh, Vl, scal, mu0_s ? mu0_s + c0 : nullptr, mean_out + c0,
            spread_out + c0, F_out ? F_out + c0 : nullptr);
        AGPL_LAUNCH_CHECK(ctx);
    }
    return AGPL_OK;
}
