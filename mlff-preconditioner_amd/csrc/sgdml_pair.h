// What the sGDML kernel families share, one copy each: the descriptor-pair index and its inversion,
// the Matern 5/2 constants and row scalars of the pair-tile family (operator, prediction, Hessians),
// the descriptor kernel, the fixed-order sum of chunk partials, the rows of J^T Fd.  The bit guarantees (alphas_E = 0
// gives the unconstrained bits, the Hessian's fused Fd equals the prediction's) hold because every
// user rounds through these functions.  __forceinline__ with arithmetic arguments by value: that
// shape left the compiled code of the tuned kernels as it was (profiles/sgdml_shared/README.txt,
// which lists what had to stay written out, the "twins").  Not users, on purpose: k_mf_reduce,
// k_sgdml_uv and k_sgdml_kee round m in the reference's order, exp(-norm / sig) 5 / (3 sig^4).
#pragma once

#include "common.h"

namespace mlff {

constexpr double kSqrt5 = 2.23606797749978969640917366873127623544;

// tril_indices(n, -1) ordering, a != b
__device__ __forceinline__ int64_t pair_idx(int a, int b) {
  return a > b ? (int64_t)a * (a - 1) / 2 + b : (int64_t)b * (b - 1) / 2 + a;
}
__device__ __forceinline__ double pair_sign(int a, int b) {  // sign of J[pair(a,b), atom a]
  return a > b ? -1.0 : 1.0;
}
struct TriIdx { int a, b; };
// the inverse of pair_idx, d = a (a - 1) / 2 + b with a > b >= 0: the sqrt estimate, corrected
__device__ __forceinline__ TriIdx tri_invert(int64_t d) {
  int a = (int)((1.0 + sqrt(1.0 + 8.0 * (double)d)) * 0.5);
  while ((int64_t)a * (a - 1) / 2 > d) --a;
  while ((int64_t)(a + 1) * a / 2 <= d) ++a;
  return {a, (int)(d - (int64_t)a * (a - 1) / 2)};
}

// Matern 5/2 scalars of the pair-tile family
struct MaternConsts { double sig, sig2, inv_sig, k5; };  // k5 = 5 / (3 sig^4)
inline MaternConsts matern_consts(double sig) {
  return {sig, sig * sig, 1.0 / sig, 5.0 / (3.0 * sig * sig * sig * sig)};
}
struct MaternM { double nrm, ex, m; };
struct MaternRow { double nrm, ex, m, w; };
// rs = |diff|^2:  nrm = sqrt5 |diff|,  ex = exp(-nrm / sig),  m = ex 5 / (3 sig^4),  w = (sig^2 +
// sig nrm) m; in two steps, since hess_row forms its scalars between them (the order matters)
__device__ __forceinline__ MaternM matern_m(double rs, MaternConsts c) {
  const double nrm = kSqrt5 * sqrt(rs);
  const double ex = exp(-nrm * c.inv_sig);
  return {nrm, ex, ex * c.k5};
}
__device__ __forceinline__ double matern_w(double nrm, double m, MaternConsts c) {
  return fma(c.sig, nrm, c.sig2) * m;
}
__device__ __forceinline__ MaternRow matern_row(double rs, MaternConsts c) {
  const MaternM mm = matern_m(rs, c);
  return {mm.nrm, mm.ex, mm.m, matern_w(mm.nrm, mm.m, c)};
}
// K_ee = (1 + x (1 + nrm / (3 sig))) exp(-x), x = nrm / sig (energy-constrained models)
__device__ __forceinline__ double kee_of(double nrm, double ex, double inv_sig, double inv_3sig) {
  return fma(nrm * inv_sig, fma(nrm, inv_3sig, 1.0), 1.0) * ex;
}
// The Hessian's row scalars from rs and aa = diff . z:  m5 = 5 m,  cdd = beta + 5 m e with beta =
// 25 m aa / (sig nrm) (0 at nrm = 0, its limit),  ci = 5 m aa + e w.  hess_row is the row of e = 0;
// hess_row_ecstr adds the terms of e = ej by fma, so ej = 0 gives the unconstrained bits.
struct HessRow { double m5, cdd, ci, w; };
__device__ __forceinline__ HessRow hess_row(double rs, double aa, MaternConsts c) {
  const MaternM mr = matern_m(rs, c);
  const double m5 = 5.0 * mr.m;
  const double cdd = mr.nrm > 0.0 ? 5.0 * m5 * aa / (c.sig * mr.nrm) : 0.0;
  const double ci = m5 * aa;
  return {m5, cdd, ci, matern_w(mr.nrm, mr.m, c)};
}
__device__ __forceinline__ HessRow hess_row_ecstr(HessRow h, double ej) {
  return {h.m5, fma(h.m5, ej, h.cdd), fma(ej, h.w, h.ci), h.w};
}

// Entry d = pair(a, b), a > b, of the geometry r (n x 3): rd = 1 / |r_a - r_b|, rdd = (x, y, z) =
// (r_a - r_b) / |r_a - r_b|^3 (desc.py:80-200 without cutoff / PBC).  CUBE_ONCE: dist^3 rounded once
// (the fma residuals of the products added back), as the reference's pow; else two multiplications.
struct DescEntry { double rd, x, y, z; };
template <bool CUBE_ONCE>
__device__ __forceinline__ DescEntry desc_entry(const double *__restrict__ r, int a, int b) {
  const double dx = r[a * 3 + 0] - r[b * 3 + 0];
  const double dy = r[a * 3 + 1] - r[b * 3 + 1];
  const double dz = r[a * 3 + 2] - r[b * 3 + 2];
  const double dist = sqrt(__dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz)));
  double d3 = dist * dist * dist;
  if (CUBE_ONCE) {
    const double p2 = dist * dist, e2 = fma(dist, dist, -p2);
    const double p3 = p2 * dist, e3 = fma(p2, dist, -p3);
    d3 = p3 + fma(e2, dist, e3);
  }
  return {1.0 / dist, dx / d3, dy / d3, dz / d3};
}
// R_desc / R_d_desc of grid.y geometries: k_desc = k_desc_t<false> (training set), k_pr_desc = <true>
template <bool CUBE_ONCE>
__global__ __launch_bounds__(256) void k_desc_t(const double *__restrict__ R, int n,
                                                double *__restrict__ Rd, double *__restrict__ Rdd) {
  const int64_t D = (int64_t)n * (n - 1) / 2, m = blockIdx.y;
  for (int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x; d < D; d += (int64_t)gridDim.x * 256) {
    const TriIdx ab = tri_invert(d);
    const DescEntry de = desc_entry<CUBE_ONCE>(R + m * n * 3, ab.a, ab.b);
    Rd[m * D + d] = de.rd;
    Rdd[(m * D + d) * 3 + 0] = de.x;
    Rdd[(m * D + d) * 3 + 1] = de.y;
    Rdd[(m * D + d) * 3 + 2] = de.z;
  }
}

constexpr int kSumE = 16, kSumG = 16;  // entries per workgroup of 256 threads, chunk groups
// The sum of group g < kSumG of an entry: its chunks [S g / 16, S (g + 1) / 16) in chunk order
// (src: the entry in chunk 0, zs: the chunk stride; batches of 8 predicated loads in flight)
__device__ __forceinline__ double chunk_group_sum(const double *__restrict__ src, int64_t zs, int S, bool ok,
                                                  int g) {
  const int z0 = (int)(((int64_t)S * g) / kSumG), z1 = (int)(((int64_t)S * (g + 1)) / kSumG);
  double sum = 0.0;
  for (int z = z0; z < z1; z += 8) {
    double t[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) t[u] = (ok && z + u < z1) ? src[(int64_t)(z + u) * zs] : 0.0;
#pragma unroll
    for (int u = 0; u < 8; ++u) sum += t[u];
  }
  return sum;
}
// the group sums sP[0 .. kSumG)[el] of an entry in group order
__device__ __forceinline__ double chunk_groups_total(const double (*sP)[kSumE], int el) {
  double fsum = sP[0][el];
  for (int h = 1; h < kSumG; ++h) fsum += sP[h][el];
  return fsum;
}
// The sum of the S chunk partials of an entry, by a workgroup of 256: thread (el = tid % kSumE,
// g = tid / kSumE) forms the sum of group g of its entry (chunk_group_sum), then group 0 adds the
// group sums in group order and returns the sum (others: 0)
__device__ __forceinline__ double chunk_sum(const double *__restrict__ src, int64_t zs, int S, bool ok) {
  __shared__ double sP[kSumG][kSumE];
  const int el = threadIdx.x % kSumE, g = threadIdx.x / kSumE;
  sP[g][el] = chunk_group_sum(src, zs, S, ok, g);
  __syncthreads();
  if (g != 0 || !ok) return 0.0;
  return chunk_groups_total(sP, el);
}

// E = std E_q + c from the summed energy partial (predict.py:1106-1108: E_F *= std; E = E_F[:, 0] + c)
__device__ __forceinline__ double pred_energy(double esum, double std, double cint) {
  return __dadd_rn(__dmul_rn(esum, std), cint);
}

// Row 3 at + c of J^T Fd: sum_b (+-) Rdd[pair(at, b)][c] Fd[pair(at, b)], partners b in increasing
// order (jr: the geometry's Rdd + c, fr: its Fd).  Batches of 8 partners: their loads in flight
// together, the fmas in partner order (the partner b == at is skipped by a zero Jacobian entry:
// fma(0, f, acc) leaves acc as it is)
__device__ __forceinline__ double jt_row(const double *__restrict__ jr, const double *__restrict__ fr,
                                         int n, int at) {
  double acc = 0.0;
  for (int b0 = 0; b0 < n; b0 += 8) {
    double rv[8], fv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int b = b0 + u;
      const bool ok = b < n && b != at;
      const int64_t d = ok ? pair_idx(at, b) : 0;
      const double v = ok ? jr[d * 3] : 0.0;
      rv[u] = at > b ? -v : v;
      fv[u] = ok ? fr[d] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (b0 + u < n && b0 + u != at) acc = fma(rv[u], fv[u], acc);
  }
  return acc;
}

}  // namespace mlff
