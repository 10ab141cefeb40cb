// agpl_dense.hip -- the full-rank Gibbs step the reference actually executes (`gibbs_sample`,
// examples/bernoulli/script.jl:76-87; examples/studentt/script.jl is the same loop), for N points with a dense
// N x N prior covariance K (BASELINE config C5: StudentT, N = 65 536).
//
//   Omega <- aux_sample!(lik, y, f)                                              script.jl:81
//   Sigma  = inv(Symmetric(inv(K) + Diagonal(gamma)))                            script.jl:82
//   mu     = Sigma * (beta + K \ mu0)                                            script.jl:83
//   f      ~ MvNormal(mu, Sigma)                                                 script.jl:84
//
// evaluated without any inverse (the reference forms two O(N^3) inverses and a Cholesky per sweep):
//   B = I + D^1/2 K D^1/2 = C C'      (D = Diag(gamma); ONE float64 Cholesky per sweep: rocSOLVER potrf)
//   f = f0 + K D^1/2 B^-1 (D^-1/2 beta - D^1/2 f0 - z2),   f0 = mu0 + L_K z1,  z1, z2 ~ N(0, I)
// which is an exact draw from N(mu, Sigma) (Matheron's rule with pseudo-observations yhat = D^-1 beta of noise
// variance D^-1).  The Cholesky is hand-written: the N^3 / 3 as a float64-MFMA trailing update, the 2048-wide diagonal blocks
// by own kernels overlapped with it on a side stream (look-ahead); the panel solves (dtrsm) and the matrix-vector products are
// rocBLAS calls; the sampler (agpl_sampler.hip) and the fused elementwise steps are hand-written.
#include <rocblas/rocblas.h>
#include <rocsolver/rocsolver.h>

#include "agpl_internal.h"

namespace {

#define AGPL_ROCBLAS(ctx, call)                                                                     \
    do {                                                                                            \
        rocblas_status s__ = (call);                                                                \
        if (s__ != rocblas_status_success)                                                          \
            AGPL_FAIL(ctx, AGPL_ERR_HIP, "%s failed: rocblas_status %d (%s:%d)", #call, (int)s__,   \
                      __FILE__, __LINE__);                                                          \
    } while (0)

// B[i][j] = (i == j) + sqrt(gamma_i) K[i][j] sqrt(gamma_j) : one streaming pass, 16 B per lane
__global__ __launch_bounds__(256) void build_b_kernel(int64_t N, const double *__restrict__ K,
                                                      const double *__restrict__ gamma, double *__restrict__ B) {
    const int64_t row = blockIdx.y;
    const double sr = sqrt(gamma[row]);
    const double *Kr = K + row * N;
    double *Br = B + row * N;
    // only the triangle every factorisation below reads: LAPACK-lower of the column-major view = columns c >= row of this row
    for (int64_t c = (row & ~(int64_t)1) + ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 2; c < N;
         c += (int64_t)gridDim.x * blockDim.x * 2) {
        if (c + 1 < N) {
            const double2 k = *reinterpret_cast<const double2 *>(Kr + c);
            double2 o;
            o.x = sr * k.x * sqrt(gamma[c]) + (c == row ? 1.0 : 0.0);
            o.y = sr * k.y * sqrt(gamma[c + 1]) + (c + 1 == row ? 1.0 : 0.0);
            *reinterpret_cast<double2 *>(Br + c) = o;
        } else {
            Br[c] = sr * Kr[c] * sqrt(gamma[c]) + (c == row ? 1.0 : 0.0);
        }
    }
}

// f0 = mu0 + (L_K z1) ; r = beta / sqrt(gamma) - sqrt(gamma) f0 - z2.  gamma_i = 0 happens (Poisson: y_i = 0 and a
// drawn n_i = 0 give omega_i = PG(0, c) = 0) and implies beta_i = 0: row i of B is then e_i and D^1/2 zeroes that
// component of the solve on output, so beta / sqrt(gamma) := 0 there is exact, not a patch.
__global__ void prep_rhs_kernel(int64_t N, const double *__restrict__ mu0, const double *__restrict__ lz,
                                const double *__restrict__ beta, const double *__restrict__ gamma,
                                const double *__restrict__ z2, double *__restrict__ f0, double *__restrict__ r) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const double f = lz[i] + (mu0 ? mu0[i] : 0.0);
    const double sg = sqrt(gamma[i]);
    f0[i] = f;
    r[i] = (sg > 0.0 ? beta[i] / sg : 0.0) - sg * f - z2[i];
}
// t = sqrt(gamma) .* s
__global__ void scale_kernel(int64_t N, const double *__restrict__ gamma, double *__restrict__ s) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) s[i] *= sqrt(gamma[i]);
}
__global__ void copy_kernel(int64_t n, const double *__restrict__ a, double *__restrict__ b) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        b[i] = a[i];
}

// or_info: info[0] |= info[1] (keeps the first failing block's flag across the blocked factorisation)
__global__ void or_info_kernel(rocblas_int *info, int block_start) {
    if (threadIdx.x == 0 && blockIdx.x == 0 && info[1] != 0 && info[0] == 0) info[0] = block_start + info[1];
}

// ------------------------------------------------------------------------------------------------
// trailing_update_kernel: the N^3 of the factorisation, hand-written on the float64 matrix cores.
//   A[r][c] -= sum_{q < w} A[r][k0 + q] A[c][k0 + q]   for e <= c <= r < N   (column-major, ld = N; e = k0 + w)
// i.e. the symmetric rank-w update of the LOWER triangle of the trailing matrix by the panel P = A[e:, k0:e] that the
// triangular solve has just produced -- only the lower triangle is computed (tiles with row block >= column block).
// One workgroup = one 128 x 128 tile, four waves as 2 x 2 of 64 x 64 = 4 x 4 accumulators of v_mfma_f64_16x16x4_f64 (128
// VGPRs).  Both operands are rows of P ([panel row][q], the row index contiguous in memory): 16 columns of P at a time go
// through a double-buffered LDS tile [q][row] (row pitch 144 doubles: the four q-groups of a fragment read fall in distinct
// bank halves), the next tile's global loads in flight during the 64 MFMAs of the current one.  An MFMA of this shape takes
// 64 cycles for 2 x 8 bytes of operands per lane: the kernel is bound by the matrix pipe, not by LDS or HBM
// (16 KB + 16 KB per 4096 MFMA-cycles and workgroup).  The product is formed transposed, D[c][r], so that the 16 lanes of a
// result register run along the contiguous (row) index of A: 128-byte read-modify-writes.  The fixed summation order makes
// the factor bitwise reproducible.
// ------------------------------------------------------------------------------------------------
typedef double d4t __attribute__((ext_vector_type(4)));
constexpr int kTT = 128;      // tile edge
constexpr int kTK = 16;       // panel columns per stage
constexpr int kTPitch = 144;  // doubles per LDS row of a stage
constexpr int kTStage = kTK * kTPitch; // doubles per operand and stage

// The tile routine in its general form:  C[r][c] (-)= sum_{q < w} X[r][q] Y[c][q]  for the 128 x 128 tile at (r0, c0).
// X[r][q] = Xp[r + q ldx], Y[c][q] = Yp[c + q ldy], C[r][c] = Cp[r + c ldc]; rows r < rmax and columns c < cmax exist (loads beyond
// are clamped, stores guarded).  DIAG: X and Y are the same rows (one load) and only r >= c is stored.  ASSIGN: C = X Y' instead of
// C -= X Y' (the in-block panel solve B <- B U': C may alias X because a tile reads all of its X rows before it writes).
// COPY: the new value of every stored element with r >= r2, c < c2 also goes to C2[(r - r2) + c ld2] (the update's tiles of the next
// block column leave the raw panel of the next step where its panel product reads it: no copy pass)
template <bool DIAG, bool ASSIGN, bool COPY = false>
__device__ __forceinline__ void gemm_nt_tile(double *smem, const double *Xp, int64_t ldx, const double *Yp, int64_t ldy,
                                             double *Cp, int64_t ldc, int w, int64_t r0, int64_t c0, int64_t rmax,
                                             int64_t cmax, double *C2 = nullptr, int64_t ld2 = 0, int64_t r2 = 0,
                                             int64_t c2 = 0) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave & 1, wc = wave >> 1;
    const int li = lane & 15, lq = lane >> 4;
    // staging role: rows (tid & 63) * 2, +1 of the tile; panel columns (tid >> 6) + 4 i
    const int srow = (tid & 63) * 2, sq = tid >> 6;
    int64_t gr = r0 + srow, gc = c0 + srow;
    // A thread stages the row pair (gr, gr + 1).  Pairs beyond the limit are never stored: any in-range address will do.  The pair
    // that STRADDLES the limit (gr == rmax - 1: an odd number of rows is left) is read as (rmax - 2, rmax - 1) and its second
    // value moved into the first slot, so that the LDS slot of row rmax - 1 holds row rmax - 1
    const bool tailr = gr == rmax - 1, tailc = gc == cmax - 1;
    if (gr > rmax - 2) gr = rmax - 2;
    if (gc > cmax - 2) gc = cmax - 2;
    const double *pr = Xp + gr + sq * ldx, *pc = Yp + gc + sq * ldy;
    double *sR = smem, *sC = smem + 2 * kTStage; // [stage][q][row]
    double2 vr0, vr1, vr2, vr3, vc0, vc1, vc2, vc3; // the next stage, in flight during the MFMAs of the current one
#define AGPL_T_GLOAD(kt_)                                                                                       \
    do {                                                                                                        \
        const double *qr_ = pr + (int64_t)(kt_) * kTK * ldx, *qc_ = pc + (int64_t)(kt_) * kTK * ldy;            \
        vr0 = *reinterpret_cast<const double2 *>(qr_);                                                          \
        vr1 = *reinterpret_cast<const double2 *>(qr_ + 4 * ldx);                                                \
        vr2 = *reinterpret_cast<const double2 *>(qr_ + 8 * ldx);                                                \
        vr3 = *reinterpret_cast<const double2 *>(qr_ + 12 * ldx);                                               \
        if (!DIAG) {                                                                                            \
            vc0 = *reinterpret_cast<const double2 *>(qc_);                                                      \
            vc1 = *reinterpret_cast<const double2 *>(qc_ + 4 * ldy);                                            \
            vc2 = *reinterpret_cast<const double2 *>(qc_ + 8 * ldy);                                            \
            vc3 = *reinterpret_cast<const double2 *>(qc_ + 12 * ldy);                                           \
            if (tailc) vc0.x = vc0.y, vc1.x = vc1.y, vc2.x = vc2.y, vc3.x = vc3.y;                              \
        }                                                                                                       \
        if (tailr) vr0.x = vr0.y, vr1.x = vr1.y, vr2.x = vr2.y, vr3.x = vr3.y;                                  \
    } while (0)
#define AGPL_T_SWRITE(st_)                                                                                      \
    do {                                                                                                        \
        double *dr_ = sR + (st_) * kTStage + sq * kTPitch + srow, *dc_ = sC + (st_) * kTStage + sq * kTPitch + srow; \
        *reinterpret_cast<double2 *>(dr_) = vr0;                                                                \
        *reinterpret_cast<double2 *>(dr_ + 4 * kTPitch) = vr1;                                                  \
        *reinterpret_cast<double2 *>(dr_ + 8 * kTPitch) = vr2;                                                  \
        *reinterpret_cast<double2 *>(dr_ + 12 * kTPitch) = vr3;                                                 \
        if (!DIAG) {                                                                                            \
            *reinterpret_cast<double2 *>(dc_) = vc0;                                                            \
            *reinterpret_cast<double2 *>(dc_ + 4 * kTPitch) = vc1;                                              \
            *reinterpret_cast<double2 *>(dc_ + 8 * kTPitch) = vc2;                                              \
            *reinterpret_cast<double2 *>(dc_ + 12 * kTPitch) = vc3;                                             \
        }                                                                                                       \
    } while (0)
    d4t acc[4][4];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[m][n] = d4t{0.0, 0.0, 0.0, 0.0};
    const int nkt = w / kTK;
    AGPL_T_GLOAD(0);
    AGPL_T_SWRITE(0);
    __syncthreads();
    for (int kt = 0; kt < nkt; ++kt) {
        const int st = kt & 1;
        AGPL_T_GLOAD(kt + 1 < nkt ? kt + 1 : kt); // (unconditional: the last iteration re-reads its own stage, unused)
        const double *bR = sR + st * kTStage + lq * kTPitch + wr * 64 + li;           // B operand: rows of the row block
        const double *bC = (DIAG ? sR : sC) + st * kTStage + lq * kTPitch + wc * 64 + li; // A operand: rows of the column block
#pragma unroll
        for (int ks = 0; ks < kTK / 4; ++ks) {
            double a[4], b[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) a[m] = bC[ks * 4 * kTPitch + 16 * m];
#pragma unroll
            for (int n = 0; n < 4; ++n) b[n] = bR[ks * 4 * kTPitch + 16 * n];
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int n = 0; n < 4; ++n) acc[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[m], b[n], acc[m][n], 0, 0, 0);
        }
        AGPL_T_SWRITE(st ^ 1);
        __syncthreads();
    }
#undef AGPL_T_GLOAD
#undef AGPL_T_SWRITE
    // C[r][c] (-)= D[c][r]: register rr of lane l holds D[16 m + 4 rr + lq][16 n + li]
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int64_t c = c0 + wc * 64 + 16 * m + 4 * rr + lq;
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                const int64_t r = r0 + wr * 64 + 16 * n + li;
                if (r < rmax && c < cmax && (!DIAG || r >= c)) {
                    if (ASSIGN) Cp[r + c * ldc] = acc[m][n][rr];
                    else if (!COPY) Cp[r + c * ldc] -= acc[m][n][rr];
                    else {
                        const double v = Cp[r + c * ldc] - acc[m][n][rr];
                        Cp[r + c * ldc] = v;
                        if (r >= r2 && c < c2) C2[(r - r2) + c * ld2] = v;
                    }
                }
            }
        }
}

// The update on a 1-D grid of the lower-triangle tiles only, column by column: tile (I, J), J <= I < nt, of A[e:lim, e:lim], e = k0 + w,
// has index J nt - J (J - 1) / 2 + (I - J); the launch covers the indices base .. base + gridDim.x - 1 (whole columns: the look-ahead
// route launches the next block column first).  Rounds 3-5 used a 2-D grid whose upper half exits at once: nt^2 / 2 workgroups that
// each still take a slot with 74 KB of LDS for a few microseconds -- 70 ms of a C5 step.
// Pnext (may be null): the tiles of the next block column below the next diagonal block also store their new values there, as the
// next step's raw panel P_next[r - (e + w)][c - e] (ld = N): the inverse-block route's panel product reads it, no copy pass.
__global__ __launch_bounds__(256, 2) void trailing_update_kernel(int64_t N, double *__restrict__ A, int64_t k0, int w, int nt,
                                                                 int64_t base, int64_t lim, double *__restrict__ Pnext) {
    extern __shared__ __attribute__((aligned(16))) double tsm[];
    const int64_t idx = base + blockIdx.x;
    const double bq = 2.0 * nt + 1.0;
    int64_t J = (int64_t)((bq - sqrt(bq * bq - 8.0 * (double)idx)) * 0.5); // from the quadratic, then corrected for rounding
    if (J < 0) J = 0;
    if (J > nt - 1) J = nt - 1;
    while (J > 0 && J * nt - J * (J - 1) / 2 > idx) --J;
    while (J + 1 < nt && (J + 1) * nt - (J + 1) * J / 2 <= idx) ++J;
    const int64_t I = J + (idx - (J * nt - J * (J - 1) / 2));
    const int64_t e = k0 + w;
    const double *P = A + k0 * N;
    if (Pnext && J * kTT < w && (I + 1) * kTT > w) {
        double *C2 = Pnext - e * N; // (the tile routine indexes the second destination with the absolute column)
        gemm_nt_tile<false, false, true>(tsm, P, N, P, N, A, N, w, e + I * kTT, e + J * kTT, lim, lim, C2, N, e + w, e + w);
        return;
    }
    if (I == J) gemm_nt_tile<true, false>(tsm, P, N, P, N, A, N, w, e + I * kTT, e + J * kTT, lim, lim);
    else gemm_nt_tile<false, false>(tsm, P, N, P, N, A, N, w, e + I * kTT, e + J * kTT, lim, lim);
}
__host__ __device__ inline int64_t tri_tiles_before(int64_t nt, int64_t J) { return J * nt - J * (J - 1) / 2; }

// ------------------------------------------------------------------------------------------------
// The diagonal blocks, by our own kernels (round 3).  rocsolver_dpotrf may not run beside another kernel (its results then
// differ from run to run: DESIGN 4.7), and the look-ahead wants exactly that.  A 2048-wide diagonal block is factored 64 columns
// at a time: potrf64_kernel (one workgroup: Cholesky of the 64 x 64 block in LDS, and its inverse U = R^-1), the rows below it
// within the block by B <- B U' (panel_solve_kernel, the tile routine in ASSIGN mode) and the rest of the block by the trailing
// update above with w = 64.  About 100 us per step, 3 ms per block -- hidden behind the previous step's update.
// ------------------------------------------------------------------------------------------------
constexpr int kPB = 64;
__device__ __forceinline__ double readlane_f64(double x, int srclane) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), srclane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(x), srclane);
    return __hiloint2double(hi, lo);
}
// One WAVE, no barriers: lane r keeps row r of the block in registers; column step c reads the pivot and the multipliers of the
// other rows by v_readlane (the loop is fully unrolled: register and lane indices are constants) -- 2016 readlane + FMA pairs, ~12 k
// instructions.  A first version with 256 threads, the block in LDS and three barriers per column took 240 us beside the update
// kernel (profiles/r03_c5_kernel_stats_lookahead_v1.csv).  Then U = R^-1, lane j owning column j: R is read back from LDS at
// wave-uniform addresses (broadcast reads).
__global__ __launch_bounds__(64) void potrf64_kernel(int64_t ld, double *__restrict__ D, double *__restrict__ Uout,
                                                     rocblas_int *__restrict__ info, int first_row) {
    __shared__ double rs[kPB][kPB + 1]; // rs[c][r] = R[r][c]
    __shared__ double rinv[kPB];        // 1 / R[c][c]
    __builtin_amdgcn_s_setprio(3); // this wave is the critical path of the side stream; the update's waves fill every SIMD around it
    const int lane = threadIdx.x;
    double a[kPB];
#pragma unroll
    for (int c = 0; c < kPB; ++c) a[c] = c <= lane ? D[lane + (int64_t)c * ld] : 0.0;
    int bad = 0;
#pragma unroll
    for (int c = 0; c < kPB; ++c) {
        const double p = readlane_f64(a[c], c);
        if (!(p > 0.0) && bad == 0) bad = c + 1;
        // 1 / sqrt(p) by v_rsq_f64 + two Newton steps (rounding-limited; the sqrt + divide sequences are ~150 dependent
        // instructions per column on this single wave's critical path)
        double r0 = __builtin_amdgcn_rsq(p);
        r0 = r0 * (1.5 - 0.5 * p * r0 * r0);
        r0 = r0 * (1.5 - 0.5 * p * r0 * r0);
        if (lane == 0) rinv[c] = r0;
        const double l = lane == c ? p * r0 : a[c] * r0; // R[lane][c] (rows above the diagonal carry zeros, then harmless leftovers)
        a[c] = l;
#pragma unroll
        for (int j = c + 1; j < kPB; ++j) a[j] -= l * readlane_f64(l, j);
    }
#pragma unroll
    for (int c = 0; c < kPB; ++c) {
        const double v = c <= lane ? a[c] : 0.0;
        rs[c][lane] = v;
        if (c <= lane) D[lane + (int64_t)c * ld] = v;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // U = R^-1, column `lane`: u_i = (delta_{i,lane} - sum_{k < i} R[i][k] u_k) / R[i][i]   (u_k = 0 for k < lane falls out)
    double u[kPB];
#pragma unroll
    for (int i = 0; i < kPB; ++i) {
        double acc = i == lane ? 1.0 : 0.0;
#pragma unroll
        for (int k = 0; k < i; ++k) acc -= rs[k][i] * u[k];
        u[i] = acc * rinv[i];
    }
#pragma unroll
    for (int i = 0; i < kPB; ++i) Uout[i + lane * kPB] = i >= lane ? u[i] : 0.0; // U[i][lane] at i + 64 lane
    if (lane == 0 && bad && info[0] == 0) info[0] = first_row + bad;
}

// B <- B U' for the rows r0 .. rmax of the 64 columns at Bp (ld): one workgroup per 128 rows
__global__ __launch_bounds__(256, 2) void panel_solve_kernel(int64_t ld, double *__restrict__ Bp, const double *__restrict__ U,
                                                             int64_t r0, int64_t rmax) {
    extern __shared__ __attribute__((aligned(16))) double tsm[];
    __builtin_amdgcn_s_setprio(3);
    gemm_nt_tile<false, true>(tsm, Bp, ld, U, kPB, Bp, ld, kPB, r0 + (int64_t)blockIdx.x * kTT, 0, rmax, kPB);
}

// one diagonal block A[k : k + W, k : k + W] (W a multiple of 64) on `st`, by the three kernels above
int32_t own_block_potrf(agpl_ctx *ctx, hipStream_t st, int64_t N, double *A, int64_t k, int64_t W, double *Ubuf,
                        rocblas_int *info) {
    const size_t lds = sizeof(double) * 4 * kTStage;
    for (int64_t j = 0; j < W; j += kPB) {
        const int64_t kj = k + j, rem = k + W - (kj + kPB);
        potrf64_kernel<<<1, 64, 0, st>>>(N, A + kj + kj * N, Ubuf, info, (int)kj);
        if (rem > 0) {
            const unsigned nt = (unsigned)((rem + kTT - 1) / kTT);
            panel_solve_kernel<<<nt, 256, lds, st>>>(N, A + kj * N, Ubuf, kj + kPB, k + W);
            trailing_update_kernel<<<(unsigned)tri_tiles_before(nt, nt), 256, lds, st>>>(N, A, kj, kPB, (int)nt, 0, k + W, nullptr);
        }
    }
    AGPL_LAUNCH_CHECK(ctx);
    return AGPL_OK;
}

// Lower Cholesky (column-major view, in place) of an N x N float64 matrix as a right-looking blocked factorisation with
// look-ahead on two streams.  Per 2048-wide step k: the diagonal block (own_block_potrf), the panel solve (one rocblas dtrsm)
// and the update of the trailing lower triangle -- the N^3 / 3 -- by trailing_update_kernel (rounds 1-2: one rocblas dgemm per
// block column, 54.7 TF/s at C5).  The update by panel k is launched in two parts: first the tile columns that form block column
// k + 1, then the rest; as soon as the first part is done, block k + 1 is factored and panel k + 1 solved on a high-priority side
// stream WHILE the rest of update k keeps the matrix pipes busy on the main stream (disjoint columns; events both ways).  Without
// the look-ahead the chain of small kernels sat between the updates: 1741 ms per C5 step, 1404 of them in the update kernel.
// A last block that is not a multiple of 64 wide goes to rocsolver_dpotrf (alone on the device by then).
// info[0] = 0 or 1-based index of the first non-positive pivot, as potrf.
#ifndef AGPL_DENSE_NB
#define AGPL_DENSE_NB 2048 // measured at C5 on one box without look-ahead (profiles/r03_c5_block_width.txt): 512 / 1024 / 2048 / 4096 -> 1876 / 1763 / 1741 / 1743 ms per step
#endif
int32_t blocked_potrf_steps(agpl_ctx *ctx, rocblas_handle h, int64_t N, double *A, rocblas_int *info) {
    constexpr int64_t nb = AGPL_DENSE_NB;
    static_assert(nb % kTK == 0 && nb % kTT == 0 && nb % kPB == 0, "panel width must be whole stages, tiles and blocks");
    hipStream_t S = ctx->stream;
    if (!ctx->aux_stream) {
        int least = 0, greatest = 0;
        AGPL_HIP(ctx, hipDeviceGetStreamPriorityRange(&least, &greatest));
        AGPL_HIP(ctx, hipStreamCreateWithPriority(&ctx->aux_stream, hipStreamNonBlocking, greatest));
        for (int i = 0; i < 2; ++i) AGPL_HIP(ctx, hipEventCreateWithFlags(&ctx->aux_ev[i], hipEventDisableTiming));
    }
    hipStream_t X = ctx->aux_stream;
    hipEvent_t ev_col = ctx->aux_ev[0], ev_panel = ctx->aux_ev[1];
    double *Ubuf = agpl_ws2_at<double>(ctx, agpl_ws2_dense().Ubuf); // (the callers have reserved agpl_ws2_dense().total)
    AGPL_HIP(ctx, hipMemsetAsync(info, 0, 2 * sizeof(rocblas_int), S));
    AGPL_ROCBLAS(ctx, rocblas_set_pointer_mode(h, rocblas_pointer_mode_host));
    const double one = 1.0;
    const size_t lds = sizeof(double) * 4 * kTStage;
    AGPL_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&trailing_update_kernel),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    AGPL_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&panel_solve_kernel),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipStream_t cur = S; // the stream the diagonal block / panel of this step run on
    for (int64_t k = 0; k < N; k += nb) {
        const int64_t e = k + nb < N ? k + nb : N, w = e - k;
        double *Akk = A + k + k * N;
        if (w % kPB == 0) {
            int32_t rc = own_block_potrf(ctx, cur, N, A, k, w, Ubuf, info);
            if (rc) return rc;
        } else { // (only the last block can be ragged)
            AGPL_ROCBLAS(ctx, rocblas_set_stream(h, cur));
            AGPL_ROCBLAS(ctx, rocsolver_dpotrf(h, rocblas_fill_lower, (rocblas_int)w, Akk, (rocblas_int)N, info + 1));
            or_info_kernel<<<1, 64, 0, cur>>>(info, (int)k);
            AGPL_LAUNCH_CHECK(ctx);
        }
        if (e < N) {
            const int64_t m = N - e;
            double *A21 = A + e + k * N;
            // A21 <- A21 L11^-T
            AGPL_ROCBLAS(ctx, rocblas_set_stream(h, cur));
            AGPL_ROCBLAS(ctx, rocblas_dtrsm(h, rocblas_side_right, rocblas_fill_lower, rocblas_operation_transpose,
                                            rocblas_diagonal_non_unit, (rocblas_int)m, (rocblas_int)w, &one, Akk,
                                            (rocblas_int)N, A21, (rocblas_int)N));
        }
        if (cur == X) { // the main stream continues once this panel is there
            AGPL_HIP(ctx, hipEventRecord(ev_panel, X));
            AGPL_HIP(ctx, hipStreamWaitEvent(S, ev_panel, 0));
        }
        if (e == N) break;
        // trailing lower triangle: A[e:, e:] -= A21 A21', block column k + 1 first
        const int64_t m = N - e, nt = (m + kTT - 1) / kTT;
        const int64_t ncol1 = nt < nb / kTT ? nt : nb / kTT;
        trailing_update_kernel<<<(unsigned)tri_tiles_before(nt, ncol1), 256, lds, S>>>(N, A, k, (int)w, (int)nt, 0, N, nullptr);
        AGPL_LAUNCH_CHECK(ctx);
        AGPL_HIP(ctx, hipEventRecord(ev_col, S));
        AGPL_HIP(ctx, hipStreamWaitEvent(X, ev_col, 0));
        if (nt > ncol1) {
            trailing_update_kernel<<<(unsigned)(tri_tiles_before(nt, nt) - tri_tiles_before(nt, ncol1)), 256, lds, S>>>(
                N, A, k, (int)w, (int)nt, tri_tiles_before(nt, ncol1), N, nullptr);
            AGPL_LAUNCH_CHECK(ctx);
        }
        cur = X;
    }
    AGPL_ROCBLAS(ctx, rocblas_set_stream(h, S));
    return AGPL_OK;
}
// On an error in the middle of the steps the library handle may be bound to the side stream and the side stream may still be
// working: put both back (the handle on the main stream, the main stream behind whatever the side stream was given) before
// the error is reported, so that the context stays usable.
int32_t blocked_potrf(agpl_ctx *ctx, rocblas_handle h, int64_t N, double *A, rocblas_int *info) {
    const int32_t rc = blocked_potrf_steps(ctx, h, N, A, info);
    if (rc != AGPL_OK) {
        (void)rocblas_set_stream(h, ctx->stream);
        if (ctx->aux_stream && ctx->aux_ev[1] && hipEventRecord(ctx->aux_ev[1], ctx->aux_stream) == hipSuccess)
            (void)hipStreamWaitEvent(ctx->stream, ctx->aux_ev[1], 0);
    }
    return rc;
}

} // namespace

namespace {
// x <- (L L')^-1 x for one right-hand side, L the lower Cholesky factor (column-major, ld N) -- rocsolver_dpotrs /
// rocblas_dtrsv walk a single dependent chain down the whole matrix (188 ms per triangular solve at N = 65 536:
// 90 GB/s); here only the 2048-wide diagonal blocks are solved that way and everything off the diagonal is a dgemv at
// HBM speed (two sweeps over the 17 GB triangle).
int32_t blocked_potrs_vec(agpl_ctx *ctx, rocblas_handle h, int64_t N, const double *L, double *x) {
    constexpr int64_t nb = 2048;
    AGPL_ROCBLAS(ctx, rocblas_set_pointer_mode(h, rocblas_pointer_mode_host));
    const double one = 1.0, mone = -1.0;
    // forward: L y = x
    for (int64_t k = 0; k < N; k += nb) {
        const int64_t e = k + nb < N ? k + nb : N, w = e - k;
        AGPL_ROCBLAS(ctx, rocblas_dtrsv(h, rocblas_fill_lower, rocblas_operation_none, rocblas_diagonal_non_unit,
                                        (rocblas_int)w, L + k + k * N, (rocblas_int)N, x + k, 1));
        if (e < N)
            AGPL_ROCBLAS(ctx, rocblas_dgemv(h, rocblas_operation_none, (rocblas_int)(N - e), (rocblas_int)w, &mone,
                                            L + e + k * N, (rocblas_int)N, x + k, 1, &one, x + e, 1));
    }
    // backward: L' z = y
    const int64_t last = ((N - 1) / nb) * nb;
    for (int64_t k = last; k >= 0; k -= nb) {
        const int64_t e = k + nb < N ? k + nb : N, w = e - k;
        AGPL_ROCBLAS(ctx, rocblas_dtrsv(h, rocblas_fill_lower, rocblas_operation_transpose, rocblas_diagonal_non_unit,
                                        (rocblas_int)w, L + k + k * N, (rocblas_int)N, x + k, 1));
        if (k > 0)
            AGPL_ROCBLAS(ctx, rocblas_dgemv(h, rocblas_operation_transpose, (rocblas_int)w, (rocblas_int)k, &mone,
                                            L + k, (rocblas_int)N, x + k, 1, &one, x, 1));
    }
    return AGPL_OK;
}

// ------------------------------------------------------------------------------------------------
// Round 6: the solve of the Gibbs step WITHOUT a chain of small kernels beside the update.  The step needs
// x = B^-1 r, not the factor: per 1024-wide block k
//     U_k = chol(D_k)^-1            the sparse sweep's one-launch factorisation (factor_pipe_kernel: 0.43 ms; D_k >= I because B >= I)
//     A[e:, k] <- A[e:, k] U_k'     the panel, ONE launch of the tile routine (U_k lower triangular: a column tile stops at its diagonal)
//     A[e:, e:] -= panel panel'     trailing_update_kernel, one launch
// all in stream order on one stream: every flop of the panels runs at the matrix rate (rocBLAS dtrsm: 258 ms of kernel time beside
// the update), nothing shares the device with the update, and the 2 x 1024 dependent 64-column steps of the look-ahead chain
// (potrf64 83 us each) are 64 launches of 0.43 ms.  The diagonal blocks of A are left as they were (the triangular solves use U_k,
// which is kept: 64 x 8 MB); below them A holds the factor's panels.  Needs N % 1024 == 0 (C5: 65 536).
// ------------------------------------------------------------------------------------------------
constexpr int kDB = 1024;

// G (row-major, lower triangle and diagonal; the factorisation reads nothing else) = A[k + r][k + c] - (r == c)
__global__ __launch_bounds__(256) void extract_block_kernel(int64_t N, const double *__restrict__ A, int64_t k, double *__restrict__ G) {
    __shared__ double t[32][33];
    const int bc = blockIdx.x, br = blockIdx.y;
    if (bc > br) return;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int j = ty; j < 32; j += 8) t[j][tx] = A[(k + 32 * br + tx) + (k + 32 * bc + j) * N]; // [column j][row tx]
    __syncthreads();
    for (int j = ty; j < 32; j += 8) {
        const int r = 32 * br + j, c = 32 * bc + tx;
        G[(int64_t)r * kDB + c] = t[tx][j] - (r == c ? 1.0 : 0.0);
    }
}
// the factor kernels leave I + G in the other triangle of their output: U(a, b) sits at U[b * M + a] for b <= a; zero the rest
__global__ __launch_bounds__(256) void zero_upper_kernel(double *__restrict__ U) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int b = (int)(i / kDB), a = (int)(i % kDB);
    if (a < b) U[i] = 0.0;
}
__global__ void merge_info_kernel(const int *__restrict__ blk, rocblas_int *__restrict__ info, int k) {
    if (threadIdx.x == 0 && info[0] == 0 && blk[0] != 0) info[0] = blk[0] > 0 ? k + blk[0] : -1;
}
// P[r + q ldp] = A[(e + r) + (k + q) N]: the raw panel, set aside (the tile routine cannot write a row block in place while
// other column tiles of the same rows still read it)
__global__ __launch_bounds__(256) void copy_panel_kernel(int64_t N, const double *__restrict__ A, int64_t e, int64_t k, int64_t m,
                                                         double *__restrict__ P, int64_t ldp) {
    const int64_t q = blockIdx.y;
    const double *src = A + e + (k + q) * N;
    double *dst = P + q * ldp;
    for (int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 2; r < m; r += (int64_t)gridDim.x * blockDim.x * 2) {
        if (r + 1 < m) *reinterpret_cast<double2 *>(dst + r) = *reinterpret_cast<const double2 *>(src + r);
        else dst[r] = src[r];
    }
}
// C = X Y' on the tile routine: C[r][c], r < rows, c < cols, w columns of X and Y; ytri: Y[c][q] = 0 for q > c
__global__ __launch_bounds__(256, 2) void gemm_nt_assign_kernel(const double *__restrict__ X, int64_t ldx, const double *__restrict__ Y,
                                                                int64_t ldy, double *__restrict__ Cm, int64_t ldc, int64_t rows,
                                                                int64_t cols, int w, int ytri) {
    extern __shared__ __attribute__((aligned(16))) double tsm[];
    // (ytri: a column tile's cost grows with its column; the longest first, so that the launch ends on the short ones)
    const int64_t r0 = (int64_t)blockIdx.x * kTT, c0 = (int64_t)(ytri ? gridDim.y - 1 - blockIdx.y : blockIdx.y) * kTT;
    int we = w;
    if (ytri && c0 + kTT < we) we = (int)(c0 + kTT);
    gemm_nt_tile<false, true>(tsm, X, ldx, Y, ldy, Cm, ldc, we, r0, c0, rows, cols);
}

struct InvBlocks { // where the pieces of the inverse-block route live in the workspace (doubles from `base`)
    double *U, *G, *T, *P, *gz, *vo;
    void *coop;
    int *info_blk;
    size_t bytes;
};
InvBlocks inv_blocks_layout(int64_t N, char *base) {
    InvBlocks o;
    const size_t nblk = (size_t)(N / kDB), bb = (size_t)kDB * kDB;
    size_t at = 0;
    auto take = [&](size_t bytes) { char *p = base ? base + at : nullptr; at += (bytes + 255) & ~(size_t)255; return p; };
    o.U = (double *)take(sizeof(double) * nblk * bb);
    o.G = (double *)take(sizeof(double) * bb);
    o.T = (double *)take(sizeof(double) * bb);
    o.P = (double *)take(sizeof(double) * (size_t)N * kDB);
    o.gz = (double *)take(sizeof(double) * kDB);
    o.vo = (double *)take(sizeof(double) * kDB);
    o.coop = take(agpl_factor_coop_bytes(kDB, 1));
    o.info_blk = (int *)take(256);
    o.bytes = at;
    return o;
}

// the factor in the form above; info[0] = 0, the 1-based index of the first non-positive pivot, or -1 (an internal loss of the
// factor pipeline's co-residency: cannot happen in stream order on a device this process has to itself)
int32_t inverse_block_factor(agpl_ctx *ctx, int64_t N, double *A, const InvBlocks &w, rocblas_int *info) {
    hipStream_t S = ctx->stream;
    const size_t lds = sizeof(double) * 4 * kTStage;
    AGPL_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&trailing_update_kernel),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    AGPL_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&gemm_nt_assign_kernel),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    AGPL_HIP(ctx, hipMemsetAsync(info, 0, 2 * sizeof(rocblas_int), S));
    AGPL_HIP(ctx, hipMemsetAsync(w.gz, 0, sizeof(double) * kDB, S));
    for (int64_t k = 0; k < N; k += kDB) {
        const int64_t e = k + kDB, m = N - e;
        double *Uk = w.U + (size_t)(k / kDB) * kDB * kDB;
        extract_block_kernel<<<dim3(kDB / 32, kDB / 32), 256, 0, S>>>(N, A, k, w.G);
        AGPL_LAUNCH_CHECK(ctx);
        const int32_t rc = agpl_factor_fused(ctx, kDB, 1, w.G, w.gz, nullptr, w.T, Uk, w.vo, nullptr, nullptr, w.info_blk, w.coop);
        if (rc) return rc;
        zero_upper_kernel<<<kDB * kDB / 256, 256, 0, S>>>(Uk);
        merge_info_kernel<<<1, 64, 0, S>>>(w.info_blk, info, (int)k);
        AGPL_LAUNCH_CHECK(ctx);
        if (m > 0) {
            const unsigned nt = (unsigned)((m + kTT - 1) / kTT);
            unsigned cb = (unsigned)((m + 511) / 512);
            if (cb > 256) cb = 256;
            if (k == 0) copy_panel_kernel<<<dim3(cb, kDB), 256, 0, S>>>(N, A, e, k, m, w.P, N); // (later panels: left there by the update)
            gemm_nt_assign_kernel<<<dim3(nt, kDB / kTT), 256, lds, S>>>(w.P, N, Uk, kDB, A + e + k * N, N, m, kDB, kDB, 1);
            trailing_update_kernel<<<(unsigned)tri_tiles_before(nt, nt), 256, lds, S>>>(N, A, k, kDB, (int)nt, 0, N, w.P);
            AGPL_LAUNCH_CHECK(ctx);
        }
    }
    return AGPL_OK;
}

// x <- B^-1 x with that factor: L_kk^-1 = U_k (dtrmv on the kept blocks), everything below the diagonal blocks a dgemv at HBM speed
int32_t inverse_block_solve_vec(agpl_ctx *ctx, rocblas_handle h, int64_t N, const double *A, const double *U, double *x) {
    AGPL_ROCBLAS(ctx, rocblas_set_pointer_mode(h, rocblas_pointer_mode_host));
    const double one = 1.0, mone = -1.0;
    for (int64_t k = 0; k < N; k += kDB) { // L y = x
        const int64_t e = k + kDB;
        AGPL_ROCBLAS(ctx, rocblas_dtrmv(h, rocblas_fill_lower, rocblas_operation_none, rocblas_diagonal_non_unit, kDB,
                                        U + (size_t)(k / kDB) * kDB * kDB, kDB, x + k, 1));
        if (e < N)
            AGPL_ROCBLAS(ctx, rocblas_dgemv(h, rocblas_operation_none, (rocblas_int)(N - e), kDB, &mone, A + e + k * N,
                                            (rocblas_int)N, x + k, 1, &one, x + e, 1));
    }
    for (int64_t k = N - kDB; k >= 0; k -= kDB) { // L' z = y
        const int64_t e = k + kDB;
        if (e < N)
            AGPL_ROCBLAS(ctx, rocblas_dgemv(h, rocblas_operation_transpose, (rocblas_int)(N - e), kDB, &mone, A + e + k * N,
                                            (rocblas_int)N, x + e, 1, &one, x + k, 1));
        AGPL_ROCBLAS(ctx, rocblas_dtrmv(h, rocblas_fill_lower, rocblas_operation_transpose, rocblas_diagonal_non_unit, kDB,
                                        U + (size_t)(k / kDB) * kDB * kDB, kDB, x + k, 1));
    }
    return AGPL_OK;
}

} // namespace

// ------------------------------------------------------------------------------------------------
// U = chol(I + G)^-1 for 1024 < M <= 2048 (M % 128 == 0) WITHOUT a library call (round 6): two block rows around
// the one-launch factorisation, the products on the float64 tile routine above.  With I + G = [A11 . ; A21 A22], M1 = 1024:
//     U11 = chol(A11)^-1                         agpl_factor_fused on G11
//     R21 = A21 U11'                             (U11 lower triangular: a column tile stops at its diagonal)
//     U22 = chol(A22 - R21 R21')^-1              agpl_factor_fused on G22 - R21 R21'  (the Schur complement is I + that)
//     U21 = -U22 (R21 U11)                       as two products in the tile routine's X Y' form: T' = U11' R21', U21 = 0 - U22 (T')'
// ~2 ms at M = 2048 against 3.4+ ms for rocSOLVER's potrf + trtri (~300 dependent launches).  One latent after the other (the
// configurations with many latents have M = 256).  A_work [L][M][M] takes U as the one-launch kernels leave it (U[a][b] at
// [b M + a], b <= a; the other triangle is not read by anyone); info[l] = 0, the 1-based first non-positive pivot, or -1.
// ------------------------------------------------------------------------------------------------
namespace {
__global__ __launch_bounds__(256) void copy_block_kernel(double *__restrict__ dst, int64_t ldd, const double *__restrict__ src,
                                                         int64_t lds, int rows, int cols) { // column c of `rows` contiguous doubles
    const int c = blockIdx.y;
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += gridDim.x * blockDim.x) dst[r + c * ldd] = src[r + c * lds];
    (void)cols;
}
__global__ __launch_bounds__(256) void zero_block_kernel(double *__restrict__ dst, int64_t ldd, int rows) {
    const int c = blockIdx.y;
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += gridDim.x * blockDim.x) dst[r + c * ldd] = 0.0;
}
__global__ __launch_bounds__(256) void zero_foreign_triangle_kernel(int M, double *__restrict__ U) { // keep U[b M + a], b <= a
    const int b = blockIdx.y;
    for (int a = blockIdx.x * blockDim.x + threadIdx.x; a < b; a += gridDim.x * blockDim.x) U[(int64_t)b * M + a] = 0.0;
}
__global__ __launch_bounds__(256) void transpose_kernel(int n, const double *__restrict__ in, double *__restrict__ out) {
    __shared__ double t[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int r0 = 32 * blockIdx.x, c0 = 32 * blockIdx.y;
    for (int j = ty; j < 32; j += 8) t[j][tx] = in[(r0 + tx) + (int64_t)(c0 + j) * n];
    __syncthreads();
    for (int j = ty; j < 32; j += 8) out[(c0 + tx) + (int64_t)(r0 + j) * n] = t[tx][j];
}
__global__ void merge_two_block_kernel(int M1, const int *__restrict__ i1, const int *__restrict__ i2, const double *__restrict__ ld,
                                       int *__restrict__ info, double *__restrict__ logdet) {
    if (threadIdx.x == 0) {
        info[0] = i1[0] ? i1[0] : (i2[0] > 0 ? M1 + i2[0] : i2[0]);
        if (logdet) logdet[0] = ld[0] + ld[1];
    }
}
__global__ __launch_bounds__(256, 2) void gemm_nt_sub_kernel(const double *__restrict__ X, int64_t ldx, const double *__restrict__ Y,
                                                             int64_t ldy, double *__restrict__ Cm, int64_t ldc, int64_t rows,
                                                             int64_t cols, int w) {
    extern __shared__ __attribute__((aligned(16))) double tsm[];
    gemm_nt_tile<false, false>(tsm, X, ldx, Y, ldy, Cm, ldc, w, (int64_t)blockIdx.x * kTT, (int64_t)blockIdx.y * kTT, rows, cols);
}
struct TwoBlock {
    double *G11, *U11, *U11t, *R21, *G22, *U22, *T1t, *gz, *vt, *ld;
    int *i12;
    void *coop;
    size_t bytes;
};
TwoBlock two_block_layout(int32_t M, char *base) {
    const size_t M1 = 1024, M2 = (size_t)M - 1024;
    TwoBlock o;
    size_t at = 0;
    auto take = [&](size_t bytes) { char *p = base ? base + at : nullptr; at += (bytes + 255) & ~(size_t)255; return p; };
    o.G11 = (double *)take(8 * M1 * M1);
    o.U11 = (double *)take(8 * M1 * M1);
    o.U11t = (double *)take(8 * M1 * M1);
    o.R21 = (double *)take(8 * M2 * M1);
    o.G22 = (double *)take(8 * M2 * M2);
    o.U22 = (double *)take(8 * M2 * M2);
    o.T1t = (double *)take(8 * M1 * M2);
    o.gz = (double *)take(8 * M1);
    o.vt = (double *)take(8 * M1);
    o.ld = (double *)take(256);
    o.i12 = (int *)take(256);
    o.coop = take(agpl_factor_coop_bytes(1024, 1));
    o.bytes = at;
    return o;
}
} // namespace

size_t agpl_factor_two_block_bytes(int32_t M) { return two_block_layout(M, nullptr).bytes; }

int32_t agpl_factor_two_block(agpl_ctx *ctx, int32_t M, int32_t L, const double *G, double *T_work, double *A_work, double *logdet_out,
                              int *info_dev, void *work) {
    if (M <= 1024 || M > 2048 || M % 128 || L <= 0 || !work) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "agpl_factor_two_block: M = %d", M);
    const int M1 = 1024, M2 = M - 1024;
    const TwoBlock w = two_block_layout(M, (char *)work);
    hipStream_t S = ctx->stream;
    const size_t lds = sizeof(double) * 4 * kTStage;
    AGPL_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&gemm_nt_assign_kernel),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    AGPL_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(&gemm_nt_sub_kernel),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    AGPL_HIP(ctx, hipMemsetAsync(w.gz, 0, sizeof(double) * M1, S));
    const unsigned t1 = (unsigned)(M1 / kTT), t2 = (unsigned)((M2 + kTT - 1) / kTT);
    for (int l = 0; l < L; ++l) {
        const double *Gl = G + (size_t)l * M * M; // symmetric: row-major = column-major
        double *Al = A_work + (size_t)l * M * M, *Tl = T_work + (size_t)l * M * M;
        copy_block_kernel<<<dim3(4, M1), 256, 0, S>>>(w.G11, M1, Gl, M, M1, M1);
        AGPL_LAUNCH_CHECK(ctx);
        int32_t rc = agpl_factor_fused(ctx, M1, 1, w.G11, w.gz, nullptr, Tl, w.U11, w.vt, nullptr, w.ld, w.i12, w.coop);
        if (rc) return rc;
        zero_foreign_triangle_kernel<<<dim3(4, M1), 256, 0, S>>>(M1, w.U11);
        // R21 = A21 U11' (A21[r][k] = G[M1 + r][k])
        gemm_nt_assign_kernel<<<dim3(t2, t1), 256, lds, S>>>(Gl + M1, M, w.U11, M1, w.R21, M2, M2, M1, M1, 1);
        // G22 - R21 R21' (both triangles: the factorisation reads the row-major lower one)
        copy_block_kernel<<<dim3(4, M2), 256, 0, S>>>(w.G22, M2, Gl + (size_t)M1 * M + M1, M, M2, M2);
        gemm_nt_sub_kernel<<<dim3(t2, t2), 256, lds, S>>>(w.R21, M2, w.R21, M2, w.G22, M2, M2, M2, M1);
        AGPL_LAUNCH_CHECK(ctx);
        rc = agpl_factor_fused(ctx, M2, 1, w.G22, w.gz, nullptr, Tl, w.U22, w.vt, nullptr, w.ld + 1, w.i12 + 1, w.coop);
        if (rc) return rc;
        zero_foreign_triangle_kernel<<<dim3(4, M2), 256, 0, S>>>(M2, w.U22);
        // T' = U11' R21'  (M1 x M2):  T'[c][r] = sum_k U11[k][c] R21[r][k]
        transpose_kernel<<<dim3(M1 / 32, M1 / 32), 256, 0, S>>>(M1, w.U11, w.U11t);
        gemm_nt_assign_kernel<<<dim3(t1, t2), 256, lds, S>>>(w.U11t, M1, w.R21, M2, w.T1t, M1, M1, M2, M1, 0);
        // U21 = 0 - U22 T:  U21[r][c] = -sum_k U22[r][k] T'[c][k], straight into its place in A
        zero_block_kernel<<<dim3(4, M1), 256, 0, S>>>(Al + M1, M, M2);
        gemm_nt_sub_kernel<<<dim3(t2, t1), 256, lds, S>>>(w.U22, M2, w.T1t, M1, Al + M1, M, M2, M1, M2);
        copy_block_kernel<<<dim3(4, M1), 256, 0, S>>>(Al, M, w.U11, M1, M1, M1);
        copy_block_kernel<<<dim3(4, M2), 256, 0, S>>>(Al + (size_t)M1 * M + M1, M, w.U22, M2, M2, M2);
        zero_block_kernel<<<dim3(4, M2), 256, 0, S>>>(Al + (size_t)M1 * M, M, M1); // (the block above the diagonal: zeros, not leftovers)
        merge_two_block_kernel<<<1, 64, 0, S>>>(M1, w.i12, w.i12 + 1, w.ld, info_dev + l, logdet_out ? logdet_out + l : nullptr);
        AGPL_LAUNCH_CHECK(ctx);
    }
    return AGPL_OK;
}

extern "C" int32_t agpl_dense_cholesky(agpl_ctx *ctx, int64_t N, const double *A, double *L_out) {
    if (!ctx) return AGPL_ERR_INVALID_ARGUMENT;
    if (N <= 0 || N > 0x7fffffff || !A || !L_out) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "bad argument");
    void *hv;
    int32_t rc = agpl_get_rocblas(ctx, &hv);
    if (rc) return rc;
    rocblas_handle h = (rocblas_handle)hv;
    if (A != L_out) {
        copy_kernel<<<4096, 256, 0, ctx->stream>>>(N * N, A, L_out);
        AGPL_LAUNCH_CHECK(ctx);
    }
    rc = agpl_ws2_reserve(ctx, agpl_ws2_dense().total);
    if (rc) return rc;
    rocblas_int *info = agpl_ws2_at<rocblas_int>(ctx, agpl_ws2_dense().info);
    if (N >= 8192) {
        rc = blocked_potrf(ctx, h, N, L_out, info);
        if (rc) return rc;
    } else {
        AGPL_ROCBLAS(ctx, rocsolver_dpotrf(h, rocblas_fill_lower, (rocblas_int)N, L_out, (rocblas_int)N, info));
    }
    rocblas_int hinfo = 0;
    AGPL_HIP(ctx, hipMemcpyAsync(&hinfo, info, sizeof(hinfo), hipMemcpyDeviceToHost, ctx->stream));
    AGPL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (hinfo != 0) AGPL_FAIL(ctx, AGPL_ERR_NOT_POSDEF, "matrix is not positive definite (potrf info = %d)", (int)hinfo);
    return AGPL_OK;
}

extern "C" int32_t agpl_dense_gibbs_step(agpl_ctx *ctx, const agpl_lik_desc *lik, int64_t N, const double *K,
                                         const double *Lk, const double *mu0, const void *y, double *f_inout,
                                         double *B_work, uint32_t sweep, double *omega_out, int64_t *n_out) {
    if (!ctx) return AGPL_ERR_INVALID_ARGUMENT;
    if (!lik) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "null likelihood descriptor");
    if (lik->nlatent != 1)
        AGPL_FAIL(ctx, AGPL_ERR_UNSUPPORTED, "the dense Gibbs step handles single-latent likelihoods (nlatent = %d)",
                  lik->nlatent);
    if (N <= 0 || N > 0x7fffffff || !K || !Lk || !f_inout || !B_work || !omega_out)
        AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "bad argument");
    if (sweep & 0x80000000u) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "sweep must be < 2^31");
    void *hv;
    int32_t rc = agpl_get_rocblas(ctx, &hv);
    if (rc) return rc;
    rocblas_handle h = (rocblas_handle)hv;
    // scratch: beta, gamma, z (2N), f0, r; then the kept inverse blocks and the panel buffer of the inverse-block route
    bool inv_route = N >= 8192 && N % kDB == 0;
    const size_t vec_bytes = (sizeof(double) * 6 * (size_t)N + 1024 + 255) & ~(size_t)255;
    rc = agpl_ws_reserve(ctx, vec_bytes + (inv_route ? inv_blocks_layout(N, nullptr).bytes : 0));
    if (rc == AGPL_ERR_OUT_OF_MEMORY && inv_route) { // (8 N^2 / 1024 + 8192 N bytes more than the look-ahead route needs: 1 GB at C5)
        inv_route = false;
        rc = agpl_ws_reserve(ctx, vec_bytes);
    }
    if (rc) return rc;
    double *beta = (double *)ctx->ws, *gamma = beta + N, *z = gamma + N, *f0 = z + 2 * N, *r = f0 + N;
    const InvBlocks ib = inv_route ? inv_blocks_layout(N, (char *)ctx->ws + vec_bytes) : InvBlocks{};

    // 1. Omega <- aux_sample!(lik, y, f) ; beta, gamma = auglik_potential / auglik_precision     script.jl:81-83
    rc = agpl_aux_sample(ctx, lik, N, y, f_inout, omega_out, n_out, sweep, nullptr, nullptr);
    if (rc) return rc;
    rc = agpl_potential_precision(ctx, lik, N, y, omega_out, n_out, nullptr, beta, gamma);
    if (rc) return rc;
    // 2. z1 | z2 from the streams (seed, 0..2N-1, sweep | 2^31)
    rc = agpl_launch_randn(ctx, 2 * N, sweep | 0x80000000u, z);
    if (rc) return rc;
    // 3. f0 = mu0 + L_K z1   (in place on z1)
    AGPL_ROCBLAS(ctx, rocblas_dtrmv(h, rocblas_fill_lower, rocblas_operation_none, rocblas_diagonal_non_unit,
                                    (rocblas_int)N, Lk, (rocblas_int)N, z, 1));
    const unsigned nb = (unsigned)agpl_cdiv(N, 256);
    prep_rhs_kernel<<<nb, 256, 0, ctx->stream>>>(N, mu0, z, beta, gamma, z + N, f0, r);
    AGPL_LAUNCH_CHECK(ctx);
    // 4. B = I + D^1/2 K D^1/2, Cholesky, solve
    dim3 gb((unsigned)(agpl_cdiv(N, 512) < 64 ? agpl_cdiv(N, 512) : 64), (unsigned)N);
    build_b_kernel<<<gb, 256, 0, ctx->stream>>>(N, K, gamma, B_work);
    AGPL_LAUNCH_CHECK(ctx);
    rc = agpl_ws2_reserve(ctx, agpl_ws2_dense().total);
    if (rc) return rc;
    rocblas_int *info = agpl_ws2_at<rocblas_int>(ctx, agpl_ws2_dense().info);
    if (inv_route) {
        rc = inverse_block_factor(ctx, N, B_work, ib, info);
        if (rc) return rc;
        rc = inverse_block_solve_vec(ctx, h, N, B_work, ib.U, r);
        if (rc) return rc;
    } else if (N >= 8192) {
        rc = blocked_potrf(ctx, h, N, B_work, info);
        if (rc) return rc;
        rc = blocked_potrs_vec(ctx, h, N, B_work, r);
        if (rc) return rc;
    } else {
        AGPL_ROCBLAS(ctx, rocsolver_dpotrf(h, rocblas_fill_lower, (rocblas_int)N, B_work, (rocblas_int)N, info));
    }
    if (N < 8192) {
        AGPL_ROCBLAS(ctx, rocsolver_dpotrs(h, rocblas_fill_lower, (rocblas_int)N, 1, B_work, (rocblas_int)N, r,
                                           (rocblas_int)N));
    }
    // 5. f = f0 + K (D^1/2 s)
    scale_kernel<<<nb, 256, 0, ctx->stream>>>(N, gamma, r);
    AGPL_LAUNCH_CHECK(ctx);
    const double one = 1.0;
    AGPL_ROCBLAS(ctx, rocblas_set_pointer_mode(h, rocblas_pointer_mode_host));
    AGPL_ROCBLAS(ctx, rocblas_dsymv(h, rocblas_fill_lower, (rocblas_int)N, &one, K, (rocblas_int)N, r, 1, &one, f0, 1));
    copy_kernel<<<nb, 256, 0, ctx->stream>>>(N, f0, f_inout);
    AGPL_LAUNCH_CHECK(ctx);
    rocblas_int hinfo = 0;
    AGPL_HIP(ctx, hipMemcpyAsync(&hinfo, info, sizeof(hinfo), hipMemcpyDeviceToHost, ctx->stream));
    AGPL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (hinfo < 0) AGPL_FAIL(ctx, AGPL_ERR_HIP, "the block factorisation lost its co-resident workgroups (another process on the device?)");
    if (hinfo != 0)
        AGPL_FAIL(ctx, AGPL_ERR_NOT_POSDEF, "I + D^1/2 K D^1/2 is not positive definite (potrf info = %d)", (int)hinfo);
    return AGPL_OK;
}

// ------------------------------------------------------------------------------------------------
// agpl_probe_mfma_f64: the float64 matrix rate this device sustains (the local hardware guide gives no FP64 MFMA
// peak: "measure, don't assume") -- v_mfma_f64_16x16x4_f64 issued back to back on four independent
// accumulators by one wave per SIMD of every CU, on non-trivial operands; 2 * 16 * 16 * 4 flop per instruction.
// ------------------------------------------------------------------------------------------------
namespace {
typedef double d4v __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void mfma_f64_probe_kernel(int iters, double *__restrict__ sink) {
    const int lane = threadIdx.x & 63;
    double a = 1.0 + 1e-3 * lane, b = 1.0 - 1e-3 * lane;
    d4v c0 = {0, 0, 0, 0}, c1 = {0, 0, 0, 0}, c2 = {0, 0, 0, 0}, c3 = {0, 0, 0, 0};
    for (int i = 0; i < iters; ++i) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            c0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c0, 0, 0, 0);
            c1 = __builtin_amdgcn_mfma_f64_16x16x4f64(b, a, c1, 0, 0, 0);
            c2 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, a, c2, 0, 0, 0);
            c3 = __builtin_amdgcn_mfma_f64_16x16x4f64(b, b, c3, 0, 0, 0);
        }
        a = -a; // keeps the sums bounded and the operands changing
    }
    const d4v s = c0 + c1 + c2 + c3;
    if (s[0] + s[1] + s[2] + s[3] == 1.2345e300) sink[0] = s[0]; // never true: keeps the chain alive
}
} // namespace

// the float64 half of agpl_probe_mfma (agpl_mfma.hip holds the entry point)
int32_t agpl_probe_mfma_f64_impl(agpl_ctx *ctx, int32_t iters, double *tflops_host) {
    if (!ctx) return AGPL_ERR_INVALID_ARGUMENT;
    if (iters <= 0 || !tflops_host) AGPL_FAIL(ctx, AGPL_ERR_INVALID_ARGUMENT, "bad argument");
    int32_t rc = agpl_ws2_reserve(ctx, agpl::kWs2Head);
    if (rc) return rc;
    hipDeviceProp_t prop;
    AGPL_HIP(ctx, hipGetDeviceProperties(&prop, ctx->device));
    hipEvent_t e0, e1;
    AGPL_HIP(ctx, hipEventCreate(&e0));
    AGPL_HIP(ctx, hipEventCreate(&e1));
    double best_tf = 0.0;
    // 1, 2 and 4 waves per SIMD (4-wave workgroups, 1 / 2 / 4 per CU): the rate a wave alone cannot reach because of the
    // instruction's dependent-issue latency shows up with more waves; the best of the three is the device's rate
    for (int per_cu = 1; per_cu <= 4; per_cu *= 2) {
        const int blocks = prop.multiProcessorCount * per_cu;
        float best = 1e30f;
        for (int rep = 0; rep < 3; ++rep) { // first launch warms the clocks; the fastest of the rest counts
            AGPL_HIP(ctx, hipEventRecord(e0, ctx->stream));
            mfma_f64_probe_kernel<<<blocks, 256, 0, ctx->stream>>>(iters, agpl_ws2_result(ctx));
            AGPL_HIP(ctx, hipEventRecord(e1, ctx->stream));
            AGPL_HIP(ctx, hipEventSynchronize(e1));
            float ms = 0.f;
            AGPL_HIP(ctx, hipEventElapsedTime(&ms, e0, e1));
            if (rep > 0 && ms < best) best = ms;
        }
        const double flop = (double)blocks * 4.0 * (double)iters * 16.0 * (2.0 * 16 * 16 * 4);
        const double tf = flop / ((double)best * 1e-3) / 1e12;
        if (tf > best_tf) best_tf = tf;
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    AGPL_LAUNCH_CHECK(ctx);
    *tflops_host = best_tf;
    return AGPL_OK;
}
