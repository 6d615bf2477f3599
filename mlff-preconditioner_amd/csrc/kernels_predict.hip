// Energy and force prediction of a trained sGDML model at arbitrary query geometries
// (GDMLPredict.predict, predict.py:997-1110; the worker _predict_wkr, predict.py:72-234).
//
// Per model the device holds the permuted training descriptors Rt[jp] = R_desc_j[P_p] and the
// permuted Jacobian-coefficient products Zt[jp] = R_d_desc_alpha_j[P_p] (GDMLPredict.__init__,
// predict.py:345-362), jp = j n_perms + p.  For a query q with descriptor rd_q and compact
// Jacobian J_q (k_pr_desc: Desc.from_R, desc.py:203-358, no cut-off, no lattice):
//   diff = rd_q - Rt[jp],  nrm = sqrt5 |diff|,  a = diff . Zt[jp]
//   m    = exp(-nrm / sig) 5 / (3 sig^4),  w = (sig^2 + sig nrm) m,  c = 5 m a
//   Fd_q = sum_jp c diff - w Zt[jp]        (predict.py:185-204: (5 / sig) a m' diff - m' (nrm + sig) Zt)
//   E_q  = sum_jp a w                      (predict.py:207: a m' (nrm + sig)),  m' = sig m
//   F_q  = J_q^T Fd_q                      (vec_dot_d_desc, desc.py:408-428)
//   E = std E_q + c_int,  F = std F_q      (predict.py:1106-1108)
// The pair arithmetic is k_pt_pair's with one more fma per pair for the energy: both take the row
// scalars from matern_row (sgdml_pair.h).
//
// Energy-constrained models (use_E_cstr: alphas_E, predict.py:206-218, alphas_E_lin at :364-368)
// add, with e_jp = alphas_E[j] and x = nrm / sig,
//   Fd_q += sum_jp e_jp w diff             (K_fe: the coefficient of diff becomes c + e_jp w)
//   E_q  += sum_jp e_jp K_ee,  K_ee = (1 + x (1 + nrm / (3 sig))) exp(-x)
// in the ECSTR instantiations of both pair stages (a template flag: the unconstrained ones are the
// code they were).  The new terms enter as fma(e, w, c) and fma(e, K_ee, .) after the existing
// ones, so alphas_E = 0 adds exact zeros and gives the unconstrained model's bits.  e_jp arrives
// as an MP-long device array Et (alphas_E[j] repeated over p, the reference's alphas_E_lin): it
// is 1 / (2 D) of the Rt / Zt rows it rides with, and the kernels need no division of a 64-bit
// row index by n_perms.  The tile form stages it with the tile (rows past the chunk's end get 0,
// as Rt / Zt do), the stream form reads it as one more per-row scalar (after the first pass: a
// load ahead of the row stream cost a single query 4 %).
//
// Two forms of the pair stage, chosen by D (MLFF_PRED_FORM=tile|stream overrides):
//  - tile (D <= 288), k_pr_pair<L, DL>: a workgroup of 128 threads holds G = 128 / L queries in
//    registers, L lanes per query, DL entries per lane (interleaved pairs as in k_pt_pair), and
//    streams one chunk of the (j, p) range through LDS tiles that every query group reads by
//    broadcast; the L partial sums of |diff|^2 and diff . Zt meet in a DPP butterfly.  Bound by the
//    fp64 vector pipe.  Workgroups of two waves keep G at 64 for ethanol, so that a batch of one
//    query wastes little, and four of them fit a CU at two waves per SIMD.  The (j, p) range is cut
//    into S = min(256, MP / 64) chunks, so that one query alone still runs up to 256 workgroups.
//  - stream (any D), k_pr_stream: 256 lanes over the descriptor entries, kPrQB queries per
//    workgroup sharing every Rt / Zt row loaded, kPrTB rows per step and chunk: one pass for the
//    row scalars (fixed-order block reduction), one for the entries of Fd.  Bound by the Rt / Zt
//    stream.
// Both write the chunk partials part[s][q][0 .. D) and the energy partial (column ecol), no
// Q x M n_perms array.  k_pr_sum adds the S chunk partials of every entry in an order fixed by S
// (chunk_sum, sgdml_pair.h), k_pr_jt forms J_q^T Fd_q with the partners in increasing order
// (k_pt_fin's order, both through pair_idx) and scales.
//
// Determinism: no atomics; the chunk count S, the tile shape and every reduction order depend on
// the model (M n_perms, D, form, constrained or not) only, and no sum runs across queries: a
// query's E, F have the same bits whatever the batch, its position in it, the slab size or the
// device split.
#include "common.h"
#include "sgdml_pair.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace mlff {

namespace {

constexpr int kPrThreads = 128;     // tile form: threads per workgroup
constexpr int kPrChunkRows = 64;    // tile form: (j, p) rows per chunk, at least
constexpr int kPrMaxChunks = 256;   // tile form: chunks, at most (one workgroup per CU at Q = 1)
constexpr int kPrQB = 4;            // stream form: queries per workgroup
constexpr int kPrTB = 2;            // stream form: (j, p) rows per step (and per chunk: S = MP / 2)
constexpr int kPrSU = 2;            // stream form: entries per thread in flight (d, d + 256)
constexpr int kPrStreamMaxChunks = 4096;

struct PrArgs {
  const double *Rdq;  // nq x D query descriptors
  const double *Rt;   // MP x D
  const double *Zt;   // MP x D
  int64_t D, nq, MP;
  int S;              // chunks of the (j, p) range (gridDim.y)
  MaternConsts mc;    // sgdml_pair.h
  double *part;       // S x nq x PS
  int64_t PS, ecol;   // row stride of part and the column of the energy partial
  const double *Et;   // MP energy coefficients alphas_E[j] (ECSTR kernels only)
  double inv_3sig;    // 1 / (3 sig)
};

// Desc.from_R for the queries on the context's stream: k_desc_t (sgdml_pair.h), dist^3 rounded once
constexpr auto k_pr_desc = k_desc_t<true>;

// rows of Rt / Zt per LDS tile: 16, fewer for long descriptors (<= 9 KB per array: half of
// k_pt_pair's tile for half its threads, so the staging registers per thread stay the same)
constexpr int pr_tile_rows(int DP) { return DP <= 72 ? 16 : DP <= 144 ? 8 : 4; }

// KEEP: diff and the Zt row stay in registers between the two passes over the lane's entries
// (else they are formed / read from LDS again); WPE: waves per SIMD the registers are held to;
// ECSTR: the model has energy coefficients (Et, staged with the tile)
template <int L, int DL, bool KEEP, int WPE = 2, bool ECSTR = false>
__global__ __launch_bounds__(kPrThreads) __attribute__((amdgpu_waves_per_eu(WPE, 8)))
void k_pr_pair(PrArgs a) {
  static_assert(DL % 2 == 0 && 64 % L == 0, "lane layout");
  constexpr int DP = L * DL;          // padded descriptor length
  constexpr int G = kPrThreads / L;   // queries per workgroup
  constexpr int TJ = pr_tile_rows(DP);
  constexpr int kStage = TJ * DP;     // doubles per staged array
  constexpr int kPer = (kStage + kPrThreads - 1) / kPrThreads;
  constexpr int KD = KEEP ? DL : 2;
  __shared__ double sR[kStage];
  __shared__ double sZ[kStage];
  __shared__ double sE[ECSTR ? TJ : 1];
  const int tid = threadIdx.x;
  const int l = tid % L, g = tid / L;
  const int64_t q = (int64_t)blockIdx.x * G + g;
  const bool live = q < a.nq;
  // the query's descriptor entries in registers (zero past D and for idle lanes)
  double rd[DL], f[DL];
  {
    const double *row = a.Rdq + (live ? q : 0) * a.D;
#pragma unroll
    for (int e = 0; e < DL / 2; ++e) {
      const int64_t d = 2 * (l + L * e);
      rd[2 * e] = (live && d < a.D) ? row[d] : 0.0;
      rd[2 * e + 1] = (live && d + 1 < a.D) ? row[d + 1] : 0.0;
      f[2 * e] = f[2 * e + 1] = 0.0;
    }
  }
  double en = 0.0;
  const int64_t s = blockIdx.y;
  const int64_t jb0 = (a.MP * s) / a.S, jb1 = (a.MP * (s + 1)) / a.S;
  const int64_t ntile = (jb1 - jb0 + TJ - 1) / TJ;
  // staging of tile t: rows jb0 + t TJ ..., entries past D and rows past jb1 zero
  double vr[kPer], vz[kPer];
  double ve = 0.0;
  auto load_tile = [&](int64_t t) {
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const int e = tid + kPrThreads * u;
      const int jj = e / DP, d = e % DP;
      const int64_t jp = jb0 + t * TJ + jj;
      const bool ok = e < kStage && jp < jb1 && d < a.D;
      vr[u] = ok ? a.Rt[jp * a.D + d] : 0.0;
      vz[u] = ok ? a.Zt[jp * a.D + d] : 0.0;
    }
    if (ECSTR) {
      const int64_t jp = jb0 + t * TJ + tid;
      ve = (tid < TJ && jp < jb1) ? a.Et[jp] : 0.0;
    }
  };
  if (ntile > 0) load_tile(0);
  for (int64_t t = 0; t < ntile; ++t) {
    __syncthreads();  // the previous tile is consumed
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
      const int e = tid + kPrThreads * u;
      if (kStage % kPrThreads == 0 || e < kStage) {
        sR[e] = vr[u];
        sZ[e] = vz[u];
      }
    }
    if (ECSTR && tid < TJ) sE[tid] = ve;
    __syncthreads();
    if (t + 1 < ntile) load_tile(t + 1);  // in flight during this tile's pairs
    const int64_t rem = jb1 - jb0 - t * TJ;
    const int cnt = (int)(rem < TJ ? rem : TJ);
#pragma unroll 1
    for (int j = 0; j < cnt; ++j) {
      const double *rr = sR + j * DP + 2 * l;
      const double *zr = sZ + j * DP + 2 * l;
      double df[KD], zz[KD];
      double r2a = 0.0, r2b = 0.0, aa = 0.0, ab = 0.0;
#pragma unroll
      for (int e = 0; e < DL / 2; ++e) {
        const double2 tv = *reinterpret_cast<const double2 *>(rr + 2 * L * e);
        const double2 zv = *reinterpret_cast<const double2 *>(zr + 2 * L * e);
        const double d0 = rd[2 * e] - tv.x, d1 = rd[2 * e + 1] - tv.y;
        if (KEEP) {
          df[(2 * e) % KD] = d0;
          df[(2 * e + 1) % KD] = d1;
          zz[(2 * e) % KD] = zv.x;
          zz[(2 * e + 1) % KD] = zv.y;
        }
        r2a = fma(d0, d0, r2a);
        r2b = fma(d1, d1, r2b);
        aa = fma(d0, zv.x, aa);
        ab = fma(d1, zv.y, ab);
      }
      const double rs = group_sum<L>(r2a + r2b), as = group_sum<L>(aa + ab);
      const MaternRow mr = matern_row(rs, a.mc);
      const double w = mr.w;
      double c = 5.0 * mr.m * as;
      en = fma(as, w, en);
      if (ECSTR) {
        const double ej = sE[j];
        const double kee = kee_of(mr.nrm, mr.ex, a.mc.inv_sig, a.inv_3sig);
        c = fma(ej, w, c);
        en = fma(ej, kee, en);
      }
      // the second pass re-reads what it does not keep (no CSE of the LDS loads across this)
      if (!KEEP) asm volatile("" ::: "memory");
#pragma unroll
      for (int e = 0; e < DL / 2; ++e) {
        double d0, d1, z0, z1;
        if (KEEP) {
          d0 = df[(2 * e) % KD];
          d1 = df[(2 * e + 1) % KD];
          z0 = zz[(2 * e) % KD];
          z1 = zz[(2 * e + 1) % KD];
        } else {
          const double2 tv = *reinterpret_cast<const double2 *>(rr + 2 * L * e);
          const double2 zv = *reinterpret_cast<const double2 *>(zr + 2 * L * e);
          d0 = rd[2 * e] - tv.x;
          d1 = rd[2 * e + 1] - tv.y;
          z0 = zv.x;
          z1 = zv.y;
        }
        f[2 * e] = fma(-w, z0, fma(c, d0, f[2 * e]));
        f[2 * e + 1] = fma(-w, z1, fma(c, d1, f[2 * e + 1]));
      }
    }
  }
  if (!live) return;
  double *out = a.part + (s * a.nq + q) * a.PS;
#pragma unroll
  for (int e = 0; e < DL / 2; ++e)
    *reinterpret_cast<double2 *>(out + 2 * (l + L * e)) = make_double2(f[2 * e], f[2 * e + 1]);
  if (l == 0) out[a.ecol] = en;  // every lane of the query holds the same bits
}

// Stream form.  Workgroup (query block, chunk): the chunk's rows in steps of kPrTB; per step the
// partial |diff|^2 and diff . Zt of every (query, row) over this thread's entries (d = tid, tid +
// 256, ...: a fixed order), summed over the workgroup wave by wave (shuffle tree) and the four
// wave sums in wave order; then c, w per (query, row) and the entries of Fd, rows in increasing
// order.  A thread owns the same entries in every step, so the chunk's partial accumulates in
// part with plain loads and stores of its own entries (first step: stores only).  ECSTR: the row's
// energy coefficient joins c and the energy sum.
template <bool ECSTR>
__global__ __launch_bounds__(256) void k_pr_stream(PrArgs a) {
  constexpr int NV = 2 * kPrQB * kPrTB;
  __shared__ double sh[4][NV];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t q0 = (int64_t)blockIdx.x * kPrQB;
  const int64_t s = blockIdx.y;
  const int64_t jb0 = (a.MP * s) / a.S, jb1 = (a.MP * (s + 1)) / a.S;
  const double *rq[kPrQB];
  bool qok[kPrQB];
#pragma unroll
  for (int u = 0; u < kPrQB; ++u) {
    qok[u] = q0 + u < a.nq;
    rq[u] = a.Rdq + (qok[u] ? q0 + u : q0) * a.D;
  }
  double en[kPrQB];
#pragma unroll
  for (int u = 0; u < kPrQB; ++u) en[u] = 0.0;
  for (int64_t j0 = jb0; j0 < jb1; j0 += kPrTB) {
    const double *rt[kPrTB], *zt[kPrTB];
    bool rok[kPrTB];
#pragma unroll
    for (int t = 0; t < kPrTB; ++t) {
      rok[t] = j0 + t < jb1;
      rt[t] = a.Rt + (rok[t] ? j0 + t : j0) * a.D;
      zt[t] = a.Zt + (rok[t] ? j0 + t : j0) * a.D;
    }
    double acc[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[v] = 0.0;
    for (int64_t d0 = tid; d0 < a.D; d0 += 256 * kPrSU) {
      // kPrSU entries per thread with their loads issued together; an entry past D adds exact
      // zeros (x = rv = zv = 0)
      double x[kPrSU][kPrQB], rv[kPrSU][kPrTB], zv[kPrSU][kPrTB];
#pragma unroll
      for (int i = 0; i < kPrSU; ++i) {
        const int64_t d = d0 + 256 * i;
        const bool in = d < a.D;
#pragma unroll
        for (int u = 0; u < kPrQB; ++u) x[i][u] = in ? rq[u][d] : 0.0;
#pragma unroll
        for (int t = 0; t < kPrTB; ++t) {
          rv[i][t] = in ? rt[t][d] : 0.0;
          zv[i][t] = in ? zt[t][d] : 0.0;
        }
      }
#pragma unroll
      for (int i = 0; i < kPrSU; ++i)
#pragma unroll
        for (int t = 0; t < kPrTB; ++t)
#pragma unroll
          for (int u = 0; u < kPrQB; ++u) {
            const double df = x[i][u] - rv[i][t];
            acc[2 * (u * kPrTB + t)] = fma(df, df, acc[2 * (u * kPrTB + t)]);
            acc[2 * (u * kPrTB + t) + 1] = fma(df, zv[i][t], acc[2 * (u * kPrTB + t) + 1]);
          }
    }
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[v] = wave_sum(acc[v]);
    // the rows' energy coefficients: in flight across the two barriers
    double ej[kPrTB];
#pragma unroll
    for (int t = 0; t < kPrTB; ++t) ej[t] = (ECSTR && rok[t]) ? a.Et[j0 + t] : 0.0;
    __syncthreads();  // sh of the previous step is consumed
    if (lane == 0) {
#pragma unroll
      for (int v = 0; v < NV; ++v) sh[wv][v] = acc[v];
    }
    __syncthreads();
    double c[kPrQB][kPrTB], w[kPrQB][kPrTB];
#pragma unroll
    for (int u = 0; u < kPrQB; ++u) {
#pragma unroll
      for (int t = 0; t < kPrTB; ++t) {
        const int v = 2 * (u * kPrTB + t);
        const double rs = (sh[0][v] + sh[1][v]) + (sh[2][v] + sh[3][v]);
        const double as = (sh[0][v + 1] + sh[1][v + 1]) + (sh[2][v + 1] + sh[3][v + 1]);
        const MaternRow mr = matern_row(rs, a.mc);
        // a row past the chunk's end contributes nothing
        w[u][t] = rok[t] ? mr.w : 0.0;
        c[u][t] = rok[t] ? 5.0 * mr.m * as : 0.0;
        if (rok[t]) en[u] = fma(as, w[u][t], en[u]);
        if (ECSTR) {  // ej = 0 past the chunk's end (w = c = 0 there)
          const double kee = kee_of(mr.nrm, mr.ex, a.mc.inv_sig, a.inv_3sig);
          c[u][t] = fma(ej[t], w[u][t], c[u][t]);
          if (rok[t]) en[u] = fma(ej[t], kee, en[u]);
        }
      }
    }
    const bool first = j0 == jb0;
    for (int64_t d0 = tid; d0 < a.D; d0 += 256 * kPrSU) {
      double x[kPrSU][kPrQB], fd[kPrSU][kPrQB], rv[kPrSU][kPrTB], zv[kPrSU][kPrTB];
#pragma unroll
      for (int i = 0; i < kPrSU; ++i) {
        const int64_t d = d0 + 256 * i;
        const bool in = d < a.D;
#pragma unroll
        for (int u = 0; u < kPrQB; ++u) {
          x[i][u] = in ? rq[u][d] : 0.0;
          fd[i][u] = (first || !qok[u] || !in) ? 0.0 : a.part[(s * a.nq + q0 + u) * a.PS + d];
        }
#pragma unroll
        for (int t = 0; t < kPrTB; ++t) {
          rv[i][t] = in ? rt[t][d] : 0.0;
          zv[i][t] = in ? zt[t][d] : 0.0;
        }
      }
#pragma unroll
      for (int i = 0; i < kPrSU; ++i) {
        const int64_t d = d0 + 256 * i;
#pragma unroll
        for (int t = 0; t < kPrTB; ++t)
#pragma unroll
          for (int u = 0; u < kPrQB; ++u)
            fd[i][u] = fma(-w[u][t], zv[i][t], fma(c[u][t], x[i][u] - rv[i][t], fd[i][u]));
#pragma unroll
        for (int u = 0; u < kPrQB; ++u)
          if (qok[u] && d < a.D) a.part[(s * a.nq + q0 + u) * a.PS + d] = fd[i][u];
      }
    }
  }
  if (tid == 0) {
#pragma unroll
    for (int u = 0; u < kPrQB; ++u)
      if (qok[u]) a.part[(s * a.nq + q0 + u) * a.PS + a.ecol] = en[u];
  }
}

// Fd[q][e] = sum_s part[s][q][e] and E[q] = std sum_s part[s][q][ecol] + c: a workgroup per
// (kSumE entries, query), summed by chunk_sum (sgdml_pair.h).  Entry D stands for the energy
// column.
__global__ __launch_bounds__(256) void k_pr_sum(const double *__restrict__ part, int64_t PS,
                                                int64_t ecol, int64_t D, int64_t nq, int S,
                                                double std, double cint, double *__restrict__ Fd,
                                                double *__restrict__ E) {
  const int64_t e = (int64_t)blockIdx.x * kSumE + threadIdx.x % kSumE, q = blockIdx.y;
  const int64_t col = e < D ? e : ecol;
  const bool ok = e <= D;
  const double fsum = chunk_sum(part + q * PS + col, nq * PS, S, ok);
  if (threadIdx.x >= kSumE || !ok) return;
  if (e < D)
    Fd[q * D + e] = fsum;
  else
    E[q] = pred_energy(fsum, std, cint);
}

// F[q][3 at + c] = std sum_b (+-) Rdd_q[pair(at, b)][c] Fd_q[pair(at, b)], partners b in
// increasing order (jt_row, sgdml_pair.h): one thread per row
__global__ __launch_bounds__(64) void k_pr_jt(const double *__restrict__ Rdd,
                                              const double *__restrict__ Fd, int n, int64_t D,
                                              double std, double *__restrict__ F) {
  const int r = blockIdx.x * 64 + threadIdx.x;
  if (r >= 3 * n) return;
  const int64_t q = blockIdx.y;
  const int at = r / 3, c = r % 3;
  F[q * 3 * n + r] = std * jt_row(Rdd + q * D * 3 + c, Fd + q * D, n, at);
}

using PrFn = void (*)(PrArgs);

struct PrVariant {
  int L, DL;
  PrFn fn, fn_e;  // without / with energy coefficients
};

// L lanes per query, DL entries per lane; the first variant that covers D is used (k_pt_pair's
// shapes: DL = 18 fits the 36 entries of ethanol into two lanes)
const PrVariant kPrVariants[] = {
    {2, 18, k_pr_pair<2, 18, true>, k_pr_pair<2, 18, true, 2, true>},      // D <= 36  (n <= 9)
    {4, 18, k_pr_pair<4, 18, false>, k_pr_pair<4, 18, false, 2, true>},    // D <= 72  (n <= 12)
    {4, 28, k_pr_pair<4, 28, false>, k_pr_pair<4, 28, false, 2, true>},    // D <= 112 (n <= 15)
    {8, 28, k_pr_pair<8, 28, false>, k_pr_pair<8, 28, false, 2, true>},    // D <= 224 (n <= 21)
    {8, 36, k_pr_pair<8, 36, false, 1>, k_pr_pair<8, 36, false, 1, true>}, // D <= 288 (n <= 24)
};

const PrVariant *pr_variant(int64_t D) {
  for (const PrVariant &v : kPrVariants)
    if (D <= (int64_t)v.L * v.DL) return &v;
  return nullptr;
}

}  // namespace

bool pred_tile_supported(int64_t D) { return pr_variant(D) != nullptr; }

int pred_set_model(mlff_ctx *ctx, const double *R_desc, const double *R_d_desc_alpha, int64_t M,
                   int n, const int32_t *perms, int n_perms, double sig, double std, double cint) {
  const int64_t D = (int64_t)n * (n - 1) / 2;
  const int64_t MP = M * n_perms;
  // the form first: a request that cannot be met leaves the context's model as it is
  int form = pr_variant(D) != nullptr ? 0 : 1;
  if (const char *e = std::getenv("MLFF_PRED_FORM")) {
    if (std::strcmp(e, "tile") == 0) {
      if (pr_variant(D) == nullptr)
        return set_error(ctx, MLFF_ERR_ARG, "predict: MLFF_PRED_FORM=tile needs D <= 288");
      form = 0;
    } else if (std::strcmp(e, "stream") == 0) {
      form = 1;
    } else if (e[0] != '\0') {
      return set_error(ctx, MLFF_ERR_ARG, "predict: MLFF_PRED_FORM must be tile or stream");
    }
  }
  std::vector<int32_t> Pt, piinv;
  MLFF_TRY(desc_perm_tables(ctx, perms, n, n_perms, Pt, piinv));
  std::vector<double> hR((size_t)MP * D), hZ((size_t)MP * D);
  for (int64_t j = 0; j < M; ++j)
    for (int p = 0; p < n_perms; ++p) {
      double *dr = hR.data() + (size_t)(j * n_perms + p) * D;
      double *dz = hZ.data() + (size_t)(j * n_perms + p) * D;
      const int32_t *pp = Pt.data() + (size_t)p * D;
      for (int64_t d = 0; d < D; ++d) {
        dr[d] = R_desc[j * D + pp[d]];
        dz[d] = R_d_desc_alpha[j * D + pp[d]];
      }
    }
  hipStream_t s = ctx->stream;
  MLFF_HIP(ctx, hipStreamSynchronize(s));
  PredData &pd = ctx->pred;
  pd = PredData{};
  pd.M = M;
  pd.D = D;
  pd.MP = MP;
  pd.n = n;
  pd.n_perms = n_perms;
  pd.sig = sig;
  pd.std = std;
  pd.c = cint;
  pd.form = form;
  int64_t budget;
  if (form == 0) {
    const PrVariant *v = pr_variant(D);
    pd.G = kPrThreads / v->L;
    pd.S = (int)std::max<int64_t>(1, std::min<int64_t>(kPrMaxChunks, MP / kPrChunkRows));
    pd.PS = (int64_t)v->L * v->DL + 2;
    pd.ecol = (int64_t)v->L * v->DL;
    budget = (int64_t)256 << 20;
  } else {
    pd.G = kPrQB;
    pd.S = (int)std::min<int64_t>(kPrStreamMaxChunks, (MP + kPrTB - 1) / kPrTB);
    pd.PS = round_up(D + 1, 2);
    pd.ecol = D;
    budget = (int64_t)1 << 30;
  }
  // slabs of queries: whole workgroups, the chunk partials within the budget
  int64_t slab = budget / ((int64_t)pd.S * pd.PS * 8);
  slab = std::max<int64_t>(pd.G, slab / pd.G * pd.G);
  slab = std::min<int64_t>(slab, 8192);
  if (const char *e = std::getenv("MLFF_PRED_SLAB")) {
    const long long v = std::atoll(e);
    if (v < 1 || v > 65535) return set_error(ctx, MLFF_ERR_ARG, "predict: MLFF_PRED_SLAB out of range");
    slab = v;
  }
  pd.slab = slab;
  auto fail = [&](int rc) {
    pd = PredData{};
    return rc;
  };
  const std::pair<DevBuf<double> *, int64_t> bufs[] = {
      {&pd.Rt, MP * D},         {&pd.Zt, MP * D},           {&pd.Rq, slab * 3 * n},
      {&pd.Rdq, slab * D},      {&pd.Rddq, slab * D * 3},   {&pd.part, (int64_t)pd.S * slab * pd.PS},
      {&pd.Fd, slab * D},       {&pd.EF, slab * (3 * n + 1)}};
  for (const auto &b : bufs)
    if (const int rc = b.first->alloc(ctx, b.second, "predict")) return fail(rc);
  if (const int rc = pd.h_in.alloc(ctx, slab * 3 * n, "predict")) return fail(rc);
  if (const int rc = pd.h_out.alloc(ctx, slab * (3 * n + 1), "predict")) return fail(rc);
  if (hipMemcpy(pd.Rt, hR.data(), sizeof(double) * MP * D, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(pd.Zt, hZ.data(), sizeof(double) * MP * D, hipMemcpyHostToDevice) != hipSuccess)
    return fail(set_error(ctx, MLFF_ERR_HIP, "predict: model upload failed"));
  pd.ready = true;
  return MLFF_OK;
}

int pred_set_energy_coefficients(mlff_ctx *ctx, const double *alphas_E) {
  PredData &pd = ctx->pred;
  MLFF_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (alphas_E == nullptr) {
    pd.Et.reset();
    return MLFF_OK;
  }
  // alphas_E_lin (predict.py:364-368): alphas_E[j] for every permuted copy jp = j n_perms + p
  std::vector<double> hE((size_t)pd.MP);
  for (int64_t j = 0; j < pd.M; ++j)
    for (int p = 0; p < pd.n_perms; ++p) hE[(size_t)(j * pd.n_perms + p)] = alphas_E[j];
  if (pd.Et == nullptr) MLFF_TRY(pd.Et.alloc(ctx, pd.MP, "predict"));
  if (hipMemcpy(pd.Et, hE.data(), sizeof(double) * pd.MP, hipMemcpyHostToDevice) != hipSuccess) {
    pd.Et.reset();
    return set_error(ctx, MLFF_ERR_HIP, "predict: upload of the energy coefficients failed");
  }
  return MLFF_OK;
}

// the model part of the pair stage's arguments
static PrArgs pr_model_args(const PredData &pd) {
  PrArgs a{};
  a.Rt = pd.Rt;
  a.Zt = pd.Zt;
  a.Et = pd.Et;
  a.D = pd.D;
  a.MP = pd.MP;
  a.mc = matern_consts(pd.sig);
  a.inv_3sig = 1.0 / (3.0 * pd.sig);
  return a;
}

// the stages in `stages` (kPrStage*, common.h) for the nq queries of the slab, in this order:
// descriptors of the geometries in pd.Rq (Rdq, Rddq), the pair stage (part), the chunk sum (Fd, E)
void pr_launch_fd(const PredData &pd, int64_t nq, int stages, hipStream_t s) {
  const int64_t D = pd.D;
  PrArgs a = pr_model_args(pd);
  a.Rdq = pd.Rdq;
  a.nq = nq;
  a.S = pd.S;
  a.part = pd.part;
  a.PS = pd.PS;
  a.ecol = pd.ecol;
  const bool ecstr = pd.Et != nullptr;
  const unsigned gx = (unsigned)std::min<int64_t>((D + 255) / 256, 64);
  if (stages & kPrStageDesc)
    hipLaunchKernelGGL(k_pr_desc, dim3(gx, (unsigned)nq), dim3(256), 0, s, pd.Rq, pd.n, pd.Rdq, pd.Rddq);
  if ((stages & kPrStagePair) && pd.form == 0) {
    const PrVariant *v = pr_variant(D);
    hipLaunchKernelGGL(ecstr ? v->fn_e : v->fn,
                       dim3((unsigned)((nq + pd.G - 1) / pd.G), (unsigned)pd.S), dim3(kPrThreads),
                       0, s, a);
  } else if (stages & kPrStagePair) {
    hipLaunchKernelGGL(ecstr ? k_pr_stream<true> : k_pr_stream<false>,
                       dim3((unsigned)((nq + kPrQB - 1) / kPrQB), (unsigned)pd.S), dim3(256), 0, s,
                       a);
  }
  if (stages & kPrStageSum)
    hipLaunchKernelGGL(k_pr_sum, dim3((unsigned)((D + 1 + kSumE - 1) / kSumE), (unsigned)nq),
                       dim3(256), 0, s, pd.part, pd.PS, pd.ecol, D, nq, pd.S, pd.std, pd.c, pd.Fd, pd.EF);
}

int pred_fd_slab(mlff_ctx *ctx, const double *R, int64_t nq, bool with_fd) {
  const PredData &pd = ctx->pred;
  hipStream_t s = ctx->stream;
  const int64_t n3 = 3 * (int64_t)pd.n;
  // through the pinned staging buffer: one asynchronous copy per slab
  std::memcpy(pd.h_in, R, sizeof(double) * nq * n3);
  MLFF_HIP(ctx, hipMemcpyAsync(pd.Rq, pd.h_in, sizeof(double) * nq * n3, hipMemcpyHostToDevice, s));
  pr_launch_fd(pd, nq, with_fd ? kPrStageAll : kPrStageDesc, s);
  MLFF_HIP(ctx, hipGetLastError());
  return MLFF_OK;
}

int pred_run(mlff_ctx *ctx, const double *R, int64_t Q, double *E_out, double *F_out) {
  const PredData &pd = ctx->pred;
  hipStream_t s = ctx->stream;
  const int64_t n3 = 3 * (int64_t)pd.n, D = pd.D;
  for (int64_t q0 = 0; q0 < Q; q0 += pd.slab) {
    const int64_t nq = std::min<int64_t>(pd.slab, Q - q0);
    MLFF_TRY(pred_fd_slab(ctx, R + q0 * n3, nq, true));
    hipLaunchKernelGGL(k_pr_jt, dim3((unsigned)((n3 + 63) / 64), (unsigned)nq), dim3(64), 0, s, pd.Rddq,
                       pd.Fd, pd.n, D, pd.std, pd.EF + nq);
    MLFF_HIP(ctx, hipGetLastError());
    MLFF_HIP(ctx, hipMemcpyAsync(pd.h_out, pd.EF, sizeof(double) * nq * (n3 + 1), hipMemcpyDeviceToHost, s));
    // the slab buffers are reused by the next slab: the copy out must have left them
    MLFF_HIP(ctx, hipStreamSynchronize(s));
    std::memcpy(E_out + q0, pd.h_out, sizeof(double) * nq);
    std::memcpy(F_out + q0 * n3, pd.h_out + nq, sizeof(double) * nq * n3);
  }
  return MLFF_OK;
}

// algorithmic work of one query: 9 D + 10 flops per (j, p) pair (k_pt_pair's 9 D + 8 and the
// energy fma), and the Rt / Zt rows every query block streams.  With energy coefficients 9 more
// per pair: x = nrm / sig (1), K_ee = fma(x, fma(nrm, 1 / (3 sig), 1), 1) exp(-x) (2 + 2 + 1),
// fma(e, w, c) (2) and fma(e, K_ee, en) (2); and the Et entry of every row.
void pred_work(const PredData &pd, double *flops, double *bytes) {
  const bool ecstr = pd.Et != nullptr;
  *flops = (double)pd.MP * (9.0 * (double)pd.D + (ecstr ? 19.0 : 10.0));
  *bytes = 8.0 * (double)pd.MP * (2.0 * (double)pd.D + (ecstr ? 1.0 : 0.0));
}

}  // namespace mlff
