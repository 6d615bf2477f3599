// Closed-form solve of the dense system (sigma_K K + shift I) x = b: the reference's
// Analytic.solve (src/sGDML/sgdml/solvers/analytic.py:129-153: K[diag] -= 1e-10,
// cho_factor(-K), alphas = -cho_solve(...)) on the device.
//   k_chol_copy_lower      the lower triangle of the context's dense rows, sign and shift applied
//   potrf_lower_blocked    two-level right-looking Cholesky: potrf_lower's 64-wide steps inside
//                          an NB-wide panel, one trailing update of depth NB per panel
//   trsv_lower_fwd / _bwd  L z = b and L^T x = z with one right-hand side, 64 unknowns per step
// The factor is row-major lower (ld = n), as potrf_lower leaves it.
#include "common.h"

#include <algorithm>
#include <cstdlib>

namespace mlff {

// ---------------------------------------------------------------------------
// A[i, j] = sigma K[i, j] + shift delta_ij for j <= i, one 64 x 64 tile of the lower block
// triangle per workgroup (blockIdx.x <= blockIdx.y); the strict upper part of the diagonal
// tiles is zeroed, the upper blocks are never read by the factorisation and stay unwritten.
__global__ __launch_bounds__(256) void k_chol_copy_lower(const double *__restrict__ K, int64_t ld,
                                                         int64_t n, double sigma, double shift,
                                                         double *__restrict__ A) {
  if (blockIdx.x > blockIdx.y) return;
  const int64_t i0 = (int64_t)blockIdx.y * 64, j0 = (int64_t)blockIdx.x * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int64_t j = j0 + tx;
  if (j >= n) return;
#pragma unroll 4
  for (int r = ty; r < 64; r += 4) {
    const int64_t i = i0 + r;
    if (i >= n) break;
    double v = 0.0;
    if (j <= i) {
      v = __dmul_rn(sigma, K[i * ld + j]);
      if (j == i) v = __dadd_rn(v, shift);
    }
    A[i * n + j] = v;
  }
}

// ---------------------------------------------------------------------------
// outer panel width of potrf_lower_blocked: MLFF_POTRF_OUTER (a multiple of 64, read once);
// 64 is potrf_lower's one-level order
static int potrf_outer() {
  static const int nb = [] {
    const char *e = std::getenv("MLFF_POTRF_OUTER");
    int v = e != nullptr ? std::atoi(e) : 256;
    if (v < 64) v = 64;
    if (v > 4096) v = 4096;
    return v / 64 * 64;
  }();
  return nb;
}

int potrf_lower_blocked(mlff_ctx *ctx, double *A, int64_t n, bool *ok_out) {
  int *err = &ctx->st->linalg_err;
  hipStream_t s = ctx->stream;
  MLFF_HIP(ctx, hipMemsetAsync(err, 0, sizeof(int), s));
  const int64_t NB = potrf_outer();
  for (int64_t p0 = 0; p0 < n; p0 += NB) {
    const int64_t pend = std::min<int64_t>(p0 + NB, n);
    for (int64_t j0 = p0; j0 < pend; j0 += 64) {
      const int jb = (int)std::min<int64_t>(64, n - j0);
      launch_potrf_diag_wave(A, n, j0, jb, err, s);
      const int64_t rest = n - j0 - jb;
      if (rest <= 0) continue;
      launch_trsm_panel(A, n, n, j0, jb, s);
      // inside the panel only its remaining columns [j0 + jb, pend) are brought up to date
      const int64_t pc = pend - (j0 + jb);
      if (pc > 0) {
        const double *P = A + (j0 + jb) * n + j0;
        launch_gemm_tri(false, true, rest, pc, jb, -1.0, P, n, P, n, 1.0,
                        A + (j0 + jb) * n + j0 + jb, n, s);
      }
    }
    // the trailing matrix: one update of depth pend - p0, read and written once per panel
    const int64_t rest = n - pend;
    if (rest > 0) {
      const double *P = A + pend * n + p0;
      launch_gemm_tri(false, true, rest, rest, pend - p0, -1.0, P, n, P, n, 1.0,
                      A + pend * n + pend, n, s);
    }
  }
  launch_zero_upper(A, n, s);
  MLFF_HIP(ctx, hipGetLastError());
  int h_err = 0;
  MLFF_HIP(ctx, hipMemcpyAsync(&h_err, err, sizeof(int), hipMemcpyDeviceToHost, s));
  MLFF_HIP(ctx, hipStreamSynchronize(s));
  if (ok_out != nullptr) {
    *ok_out = h_err == 0;
    return MLFF_OK;
  }
  if (h_err)
    return set_error(ctx, MLFF_ERR_LINALG,
                     "Cholesky factorization failed: matrix is not positive definite");
  return MLFF_OK;
}

// ---------------------------------------------------------------------------
// One right-hand side.  x holds b on entry, z = L^-1 b after the forward sweep and
// L^-T z after the backward sweep.  Every entry of x is a fixed chain of fmas (the columns of
// its row in ascending order), whatever the grid: no atomics, no cross-workgroup sums.

// lane `src`'s double in every lane (src uniform): two v_readlane
__device__ __forceinline__ double lane_bcast(double v, int src) {
  const unsigned long long bits = __builtin_bit_cast(unsigned long long, v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(bits & 0xffffffffull), src);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(bits >> 32), src);
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// rows [r0, r0 + 64) x columns [c0, c0 + ib) of L into LDS (zero outside the matrix / the ib
// columns), one wave, lane = column: 16 row loads in flight at a time, each a 512-B segment
__device__ __forceinline__ void trsv_stage_rows(const double *__restrict__ L, int64_t n,
                                                int64_t r0, int64_t c0, int ib, double (*T)[65]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int rb = 0; rb < 64; rb += 16) {
    double tmp[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int64_t gr = r0 + rb + k;
      tmp[k] = (gr < n && t < ib) ? L[gr * n + c0 + t] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) T[rb + k][t] = tmp[k];
  }
  __syncthreads();
}

// x[i0 : i0 + ib] <- L_dd^-1 x[i0 : i0 + ib], one wave: lane i holds row i of the block and
// x_i; column sweep, x_c = (lane c's value) / L_cc broadcast by readlane, then the fma of every
// row below.  Rows and columns past ib are zero and take no part.
__global__ __launch_bounds__(64) void k_trsv_diag_fwd(const double *__restrict__ L, int64_t n,
                                                      int64_t i0, int ib, double *__restrict__ x) {
  __shared__ double D[64][65];
  trsv_stage_rows(L, n, i0, i0, ib, D);
  const int i = threadIdx.x;
  double row[64];
#pragma unroll
  for (int c = 0; c < 64; ++c) row[c] = D[i][c];
  const double dg = i < ib ? D[i][i] : 1.0;
  double v = i < ib ? x[i0 + i] : 0.0;
#pragma unroll
  for (int c = 0; c < 64; ++c) {
    if (c < ib) {
      const double xc = lane_bcast(v, c) / lane_bcast(dg, c);
      if (i == c) v = xc;
      if (i > c) v = fma(-row[c], xc, v);
    }
  }
  if (i < ib) x[i0 + i] = v;
}

// x[i0 : i0 + ib] <- L_dd^-T x[i0 : i0 + ib]: lane i holds column i of the block, the same
// sweep from the last column up
__global__ __launch_bounds__(64) void k_trsv_diag_bwd(const double *__restrict__ L, int64_t n,
                                                      int64_t i0, int ib, double *__restrict__ x) {
  __shared__ double D[64][65];
  trsv_stage_rows(L, n, i0, i0, ib, D);
  const int i = threadIdx.x;
  double col[64];
#pragma unroll
  for (int c = 0; c < 64; ++c) col[c] = D[c][i];
  const double dg = i < ib ? D[i][i] : 1.0;
  double v = i < ib ? x[i0 + i] : 0.0;
#pragma unroll
  for (int c = 63; c >= 0; --c) {
    if (c < ib) {
      const double xc = lane_bcast(v, c) / lane_bcast(dg, c);
      if (i == c) v = xc;
      if (i < c) v = fma(-col[c], xc, v);
    }
  }
  if (i < ib) x[i0 + i] = v;
}

// forward update, rows r >= i0 + ib: x[r] -= L[r, i0 : i0 + ib] . x[i0 : i0 + ib].  A wave
// stages its 64 rows of the column panel through LDS, then lane t runs row t's chain.
__global__ __launch_bounds__(64) void k_trsv_update_fwd(const double *__restrict__ L, int64_t n,
                                                        int64_t i0, int ib,
                                                        double *__restrict__ x) {
  __shared__ double T[64][65];
  __shared__ double xs[64];
  const int t = threadIdx.x;
  const int64_t r0 = i0 + ib + (int64_t)blockIdx.x * 64;
  xs[t] = t < ib ? x[i0 + t] : 0.0;
  trsv_stage_rows(L, n, r0, i0, ib, T);
  const int64_t gr = r0 + t;
  if (gr >= n) return;
  double acc = x[gr];
#pragma unroll
  for (int c = 0; c < 64; ++c) acc = fma(-T[t][c], xs[c], acc);  // columns past ib: -0 * 0
  x[gr] = acc;
}

// backward update, entries r < i0: x[r] -= sum_c L[i0 + c, r] x[i0 + c].  One thread per
// column r of the row band left of the block: consecutive threads read consecutive doubles,
// the band's 64 entries of a column all in flight before the chain starts.
__global__ __launch_bounds__(128) void k_trsv_update_bwd(const double *__restrict__ L, int64_t n,
                                                         int64_t i0, int ib,
                                                         double *__restrict__ x) {
  __shared__ double xs[64];
  if (threadIdx.x < 64) xs[threadIdx.x] = threadIdx.x < ib ? x[i0 + threadIdx.x] : 0.0;
  __syncthreads();
  const int64_t r = (int64_t)blockIdx.x * 128 + threadIdx.x;
  if (r >= i0) return;
  const double *col = L + i0 * n + r;
  double l[64];
#pragma unroll
  for (int c = 0; c < 64; ++c) l[c] = c < ib ? col[(int64_t)c * n] : 0.0;
  double acc = x[r];
#pragma unroll
  for (int c = 0; c < 64; ++c) acc = fma(-l[c], xs[c], acc);
  x[r] = acc;
}

int trsv_lower_fwd(mlff_ctx *ctx, const double *L, int64_t n, double *x) {
  hipStream_t s = ctx->stream;
  for (int64_t i0 = 0; i0 < n; i0 += 64) {
    const int ib = (int)std::min<int64_t>(64, n - i0);
    hipLaunchKernelGGL(k_trsv_diag_fwd, dim3(1), dim3(64), 0, s, L, n, i0, ib, x);
    const int64_t rest = n - i0 - ib;
    if (rest > 0)
      hipLaunchKernelGGL(k_trsv_update_fwd, dim3((unsigned)((rest + 63) / 64)), dim3(64), 0, s, L,
                         n, i0, ib, x);
  }
  MLFF_HIP(ctx, hipGetLastError());
  return MLFF_OK;
}

int trsv_lower_bwd(mlff_ctx *ctx, const double *L, int64_t n, double *x) {
  hipStream_t s = ctx->stream;
  for (int64_t i0 = (n - 1) / 64 * 64; i0 >= 0; i0 -= 64) {
    const int ib = (int)std::min<int64_t>(64, n - i0);
    hipLaunchKernelGGL(k_trsv_diag_bwd, dim3(1), dim3(64), 0, s, L, n, i0, ib, x);
    if (i0 > 0)
      hipLaunchKernelGGL(k_trsv_update_bwd, dim3((unsigned)((i0 + 127) / 128)), dim3(128), 0, s, L,
                         n, i0, ib, x);
  }
  MLFF_HIP(ctx, hipGetLastError());
  return MLFF_OK;
}

// ---------------------------------------------------------------------------
namespace {
// start / stop event pairs of the three phases; destroyed on every exit path
struct PhaseEvents {
  hipEvent_t ev[6] = {};
  int n = 0;
  ~PhaseEvents() {
    for (int i = 0; i < n; ++i) (void)hipEventDestroy(ev[i]);
  }
  hipError_t init(int count) {
    for (; n < count; ++n) {
      const hipError_t e = hipEventCreate(&ev[n]);
      if (e != hipSuccess) return e;
    }
    return hipSuccess;
  }
};
}  // namespace

int dense_cho_solve(mlff_ctx *ctx, double sigma_K, double shift, const double *b_host,
                    double *x_host, double *seconds_out) {
  const int64_t n = ctx->N;
  hipStream_t s = ctx->stream;
  // the N x N scratch next to K: refuse before the allocation when it cannot fit
  size_t free_b = 0, total_b = 0;
  MLFF_HIP(ctx, hipMemGetInfo(&free_b, &total_b));
  const double need = 8.0 * (double)n * (double)n + 8.0 * (double)n;
  if (need > (double)free_b)
    return set_error(ctx, MLFF_ERR_NOMEM,
                     "dense_cho_solve: the N x N factor (" + std::to_string((long long)(need / 1e6)) +
                         " MB) does not fit the device's free memory (" +
                         std::to_string((long long)(free_b / 1000000)) + " MB)");
  ScratchScope scope(ctx);
  double *A = nullptr, *x = nullptr;
  MLFF_TRY(scratch_alloc(ctx, &A, (size_t)(n * n)));
  MLFF_TRY(scratch_alloc(ctx, &x, (size_t)n));
  PhaseEvents pe;
  MLFF_HIP(ctx, pe.init(6));
  MLFF_HIP(ctx, hipMemcpyAsync(x, b_host, sizeof(double) * n, hipMemcpyHostToDevice, s));
  MLFF_HIP(ctx, hipEventRecord(pe.ev[0], s));
  const unsigned nt = (unsigned)((n + 63) / 64);
  hipLaunchKernelGGL(k_chol_copy_lower, dim3(nt, nt), dim3(256), 0, s, ctx->K, ctx->ld, n, sigma_K,
                     shift, A);
  MLFF_HIP(ctx, hipGetLastError());
  MLFF_HIP(ctx, hipEventRecord(pe.ev[1], s));
  MLFF_HIP(ctx, hipEventRecord(pe.ev[2], s));
  bool ok = true;
  MLFF_TRY(potrf_lower_blocked(ctx, A, n, &ok));
  MLFF_HIP(ctx, hipEventRecord(pe.ev[3], s));
  if (!ok)
    return set_error(ctx, MLFF_ERR_LINALG,
                     "dense_cho_solve: Cholesky factorization failed: sigma_K K + shift I is not "
                     "positive definite");
  MLFF_HIP(ctx, hipEventRecord(pe.ev[4], s));
  MLFF_TRY(trsv_lower_fwd(ctx, A, n, x));
  MLFF_TRY(trsv_lower_bwd(ctx, A, n, x));
  MLFF_HIP(ctx, hipEventRecord(pe.ev[5], s));
  MLFF_HIP(ctx, hipMemcpyAsync(x_host, x, sizeof(double) * n, hipMemcpyDeviceToHost, s));
  MLFF_HIP(ctx, hipStreamSynchronize(s));
  if (seconds_out != nullptr)
    for (int p = 0; p < 3; ++p) {
      float ms = 0.f;
      MLFF_HIP(ctx, hipEventElapsedTime(&ms, pe.ev[2 * p], pe.ev[2 * p + 1]));
      seconds_out[p] = 1e-3 * (double)ms;
    }
  return MLFF_OK;
}

int test_potrf(mlff_ctx *ctx, const double *A_host, int64_t n, int variant, double *L_host,
               double *seconds_out) {
  hipStream_t s = ctx->stream;
  ScratchScope scope(ctx);
  double *A = nullptr;
  MLFF_TRY(scratch_alloc(ctx, &A, (size_t)(n * n)));
  PhaseEvents pe;
  MLFF_HIP(ctx, pe.init(2));
  MLFF_HIP(ctx, hipMemcpyAsync(A, A_host, sizeof(double) * n * n, hipMemcpyHostToDevice, s));
  MLFF_HIP(ctx, hipEventRecord(pe.ev[0], s));
  MLFF_TRY(variant == 0 ? potrf_lower(ctx, A, n) : potrf_lower_blocked(ctx, A, n, nullptr));
  MLFF_HIP(ctx, hipEventRecord(pe.ev[1], s));
  MLFF_HIP(ctx, hipMemcpyAsync(L_host, A, sizeof(double) * n * n, hipMemcpyDeviceToHost, s));
  MLFF_HIP(ctx, hipStreamSynchronize(s));
  if (seconds_out != nullptr) {
    float ms = 0.f;
    MLFF_HIP(ctx, hipEventElapsedTime(&ms, pe.ev[0], pe.ev[1]));
    *seconds_out = 1e-3 * (double)ms;
  }
  return MLFF_OK;
}

}  // namespace mlff
