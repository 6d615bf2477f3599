// Analytic Hessians d2E / dR2 of a trained sGDML model at arbitrary query geometries
// (mlff_predict_hessian).  The reference implementation has no counterpart: the formulas are the
// second derivative of the prediction of kernels_predict.hip, whose notation this file keeps.
//
// For a query with descriptor rd and compact Jacobian Rdd (k_pr_desc) and every permuted training
// row jp (Rt, Zt, and e = alphas_E[j] of a constrained model, else 0):
//   diff = rd - Rt[jp],  nrm = sqrt5 |diff|,  a = diff . Zt[jp]
//   m = exp(-nrm / sig) 5 / (3 sig^4),  w = (sig^2 + sig nrm) m
//   G = d2E_q / drd2 = sum_jp -5 m (z diff^T + diff z^T) - (5 m a + e w) I + (beta + 5 m e) diff diff^T
//   beta = 25 m a / (sig nrm) for nrm > 0 and 0 for nrm = 0 (its limit: a = O(nrm); a query equal
//   to a training geometry has diff = 0 exactly, so the guard is needed)
//   H = std [J^T G J + sum_d g_d d2rd_d / dR2],  g = -Fd (the pair stage of the prediction)
// J = drd / dR has the row (a, b), a > b: -Rdd in the columns of atom a, +Rdd in those of b (the
// sign k_pr_jt applies), and d2(1 / r) / dR2 has the 3 x 3 blocks +B at (a, a), (b, b) and -B at
// (a, b), (b, a), B = (3 v v^T / r^2 - I) / r^3 = 3 Rdd Rdd^T / rd - rd^3 I.
//
// The D x D matrix G is never formed (38 226 accumulators per query at 24 atoms).  With
// p = J^T diff and s = J^T z (3n entries each, n - 1 partners per entry),
//   J^T G J = sum_jp [p u^T + t p^T] - (sum_jp 5 m a + e w) J^T J,
//   u = (beta + 5 m e) p - 5 m s,  t = -5 m s,
// which needs the 3n (3n + 1) / 2 entries of the lower triangle: 378 for ethanol.
//
// k_hs_pair<TB, ECSTR, FD>: a workgroup of 256 threads owns one query, one chunk of the (j, p) range
// and one tile of at most 256 blocks of 4 x 4 entries of the lower triangle (block rows bi >= bk,
// diagonal blocks whole; 3n <= 88 is one tile, further tiles on gridDim.z).  Per step of TB rows:
//   1. wave v forms |diff|^2 and a of the rows v, v + 4, ... (lanes over the entries d = lane,
//      lane + 64, ..., then the shuffle tree) and lane 0 the row's scalars 5 m, beta + 5 m e and
//      5 m a + e w;
//   2. thread (row, t < 3n) sums p_t and s_t over the n - 1 partners in increasing partner order
//      (k_pr_jt's order) and writes p, u, t of the row to LDS;
//   3. thread (block, slot) adds the rows slot, slot + RS, ... of the step to its 16 accumulators:
//      8 LDS reads of 16 bytes for 32 fmas.  RS = min(TB, 256 / blocks of the tile) row slots
//      share a block when the tile has few blocks (ethanol: 28 blocks, 8 slots), so that a small
//      molecule still fills the workgroup; the slots are added in slot order at the end.
// k_hs_pair_s<TB, ECSTR> (below) is the same stage for molecules whose rows fit LDS (up to 24
// atoms), with the lanes of steps 1 and 2 on different rows; hs_staged_tb chooses between them.
// Chunk partials part[s][q][PS] (the blocks, then sum 5 m a + e w, then Fd where the pair stage
// forms it: D <= 512, else the prediction's pair stage runs first), k_hs_sum adds the chunks with
// chunk_sum (k_pr_sum's fixed order), k_hs_fin subtracts the scalar times J^T J, adds the second-
// derivative term, scales by std and writes the full matrix: entry (i, k) and (k, i) are the same
// expression of (max, min), so H equals its transpose bit for bit.
//
// Determinism: no atomics; the chunk count, the tiles, the row slots and every reduction order
// depend on the model (M n_perms, n, constrained or not) only, and no sum runs across queries: a
// query's Hessian has the same bits whatever the batch, its position in it, the slab size or the
// device split.  The ECSTR terms enter as fma(5 m, e, beta) and fma(e, w, 5 m a): alphas_E = 0
// gives the unconstrained model's bits.
//
// hess_row (the prediction's matern_m / matern_w, so the fused Fd has its bits), pair_idx and
// chunk_sum are sgdml_pair.h's; the pair stages share hs_map.  "twin": the same text in both stages,
// because as a function it changed their compiled code (profiles/sgdml_shared/README.txt).
#include "common.h"
#include "sgdml_pair.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace mlff {

namespace {

constexpr int kHsThreads = 256;
constexpr int kHsChunkRows = 32;   // (j, p) rows per chunk, at least
constexpr int kHsMaxChunks = 256;
constexpr int kHsTB = 8;           // rows per step while 3 TB N3P doubles fit 48 KB of LDS
constexpr int kHsMaxN3P = 2048;    // TB = 1: 3 N3P doubles within 48 KB
constexpr int kHsFdU = 2;          // Fd entries per thread of the fused form: D <= 512

struct HsArgs {
  const double *Rdq;   // nq x D
  const double *Rddq;  // nq x D x 3
  const double *Rt, *Zt, *Et;
  int64_t D, nq, MP;
  int S;               // chunks (gridDim.y)
  int n, N3, N3P;      // atoms, 3 n, 3 n rounded up to 4
  int nblk;            // 4 x 4 blocks of the lower triangle
  MaternConsts mc;     // sgdml_pair.h
  double *part;        // S x nq x PS
  int64_t PS;          // 16 nblk + 2 (the blocks, the scalar, padding), + D rounded up to 2 with FD
};

// both pair stages: tile `tile` holds the blocks [b0, b0 + nbt), RS row slots share a block
struct HsMap { int b0, nbt, RS, blk, slot; };
__device__ __forceinline__ HsMap hs_map(int TB, int nblk, int tile, int tid) {
  const int b0 = tile * 256;
  const int nbt = min(256, nblk - b0);
  return {b0, nbt, min(TB, 256 / nbt), tid % nbt, tid / nbt};
}

// FD: the workgroups of tile 0 also accumulate the chunk's Fd = sum (5 m a + e w) diff - w z
// (k_pr_pair's fmas), kHsFdU entries per thread, into the columns [16 nblk + 2, .. + D) of part
template <int TB, bool ECSTR, bool FD>
__global__ __launch_bounds__(kHsThreads) void k_hs_pair(HsArgs a) {
  extern __shared__ double lds[];
  __shared__ double sc5m[TB], scdd[TB], sci[TB], scw[TB];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t q = blockIdx.x, s = blockIdx.y;
  const int N3 = a.N3, N3P = a.N3P, n = a.n;
  const int64_t D = a.D;
  double *sp = lds, *su = lds + TB * N3P, *st = lds + 2 * TB * N3P;
  // the padding entries [N3, N3P) of every row stay zero
  for (int e = tid; e < 3 * TB * N3P; e += kHsThreads) lds[e] = 0.0;
  // this thread's block of the tile and its row slot
  const HsMap hm = hs_map(TB, a.nblk, (int)blockIdx.z, tid);
  const int b0 = hm.b0, nbt = hm.nbt, RS = hm.RS, blk = hm.blk, slot = hm.slot;
  const bool act = slot < RS;
  int bi, bk;
  {  // twin (k_hs_pair / k_hs_pair_s): B = bi (bi + 1) / 2 + bk inverted, the sqrt estimate corrected
    const int B = b0 + blk;
    bi = (int)((sqrt(8.0 * (double)B + 1.0) - 1.0) * 0.5);
    while (bi * (bi + 1) / 2 > B) --bi;
    while ((bi + 1) * (bi + 2) / 2 <= B) ++bi;
    bk = B - bi * (bi + 1) / 2;
  }
  double acc[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.0;
  double scal = 0.0;
  double fd[kHsFdU];
#pragma unroll
  for (int u = 0; u < kHsFdU; ++u) fd[u] = 0.0;
  const double *rd = a.Rdq + q * D;
  const double *jq = a.Rddq + q * D * 3;
  const int64_t jb0 = (a.MP * s) / a.S, jb1 = (a.MP * (s + 1)) / a.S;
  __syncthreads();
  for (int64_t j0 = jb0; j0 < jb1; j0 += TB) {
    const int cnt = (int)min((int64_t)TB, jb1 - j0);
    // 1. the rows' scalars: a wave per row
    for (int r = wv; r < cnt; r += 4) {
      const double *rt = a.Rt + (j0 + r) * D, *zt = a.Zt + (j0 + r) * D;
      double r2 = 0.0, aa = 0.0;
      for (int64_t d = lane; d < D; d += 64) {
        const double df = rd[d] - rt[d];
        r2 = fma(df, df, r2);
        aa = fma(df, zt[d], aa);
      }
      r2 = wave_sum(r2);
      aa = wave_sum(aa);
      if (lane == 0) {
        HessRow hr = hess_row(r2, aa, a.mc);
        if (ECSTR) hr = hess_row_ecstr(hr, a.Et[j0 + r]);
        sc5m[r] = hr.m5;
        scdd[r] = hr.cdd;
        sci[r] = hr.ci;
        if (FD) scw[r] = hr.w;
      }
    }
    __syncthreads();  // the scalars are written; the previous step's p, u, t are consumed
    if (FD && blockIdx.z == 0) {
#pragma unroll
      for (int u = 0; u < kHsFdU; ++u) {
        const int64_t d = tid + kHsThreads * u;
        if (d < D) {
          const double x = rd[d];
          for (int r = 0; r < cnt; ++r)
            fd[u] = fma(-scw[r], a.Zt[(j0 + r) * D + d], fma(sci[r], x - a.Rt[(j0 + r) * D + d], fd[u]));
        }
      }
    }
    // 2. p = J^T diff, s = J^T z of every row, partners in increasing order
    for (int it = tid; it < cnt * N3; it += kHsThreads) {
      const int r = it / N3, t = it % N3;
      const int at = t / 3, c = t % 3;
      const double *rt = a.Rt + (j0 + r) * D, *zt = a.Zt + (j0 + r) * D;
      double pp = 0.0, ss = 0.0;
#pragma unroll 4
      for (int b = 0; b < n; ++b) {
        if (b == at) continue;
        const int64_t d = pair_idx(at, b);
        const double v = jq[d * 3 + c];
        const double jv = at > b ? -v : v;
        pp = fma(jv, rd[d] - rt[d], pp);
        ss = fma(jv, zt[d], ss);
      }
      const double ts = -sc5m[r] * ss;
      sp[r * N3P + t] = pp;
      su[r * N3P + t] = fma(scdd[r], pp, ts);
      st[r * N3P + t] = ts;
    }
    __syncthreads();
    // 3. H_ik += p_i u_k + t_i p_k on this thread's block, the rows of its slot
    if (act) {
      for (int r = slot; r < cnt; r += RS) {  // twin (k_hs_pair / k_hs_pair_s): the 4 x 4 update
        const double2 *pi = reinterpret_cast<const double2 *>(sp + r * N3P + 4 * bi);
        const double2 *ti = reinterpret_cast<const double2 *>(st + r * N3P + 4 * bi);
        const double2 *uk = reinterpret_cast<const double2 *>(su + r * N3P + 4 * bk);
        const double2 *pk = reinterpret_cast<const double2 *>(sp + r * N3P + 4 * bk);
        const double2 p0 = pi[0], p1 = pi[1], t0 = ti[0], t1 = ti[1];
        const double2 u0 = uk[0], u1 = uk[1], k0 = pk[0], k1 = pk[1];
        const double pv[4] = {p0.x, p0.y, p1.x, p1.y}, tv[4] = {t0.x, t0.y, t1.x, t1.y};
        const double uv[4] = {u0.x, u0.y, u1.x, u1.y}, kv[4] = {k0.x, k0.y, k1.x, k1.y};
#pragma unroll
        for (int x = 0; x < 4; ++x)
#pragma unroll
          for (int y = 0; y < 4; ++y)
            acc[4 * x + y] = fma(tv[x], kv[y], fma(pv[x], uv[y], acc[4 * x + y]));
      }
    }
    if (tid == 0)
      for (int r = 0; r < cnt; ++r) scal += sci[r];
    __syncthreads();  // thread 0 has read this step's scalars: the next step writes them
  }
  double *out = a.part + (s * a.nq + q) * a.PS;
  if (RS > 1) {  // twin (k_hs_pair / k_hs_pair_s): the slot merge and the store of the block
    // the slots of a block in slot order (lds is free: the loop ends with a barrier)
    if (act) {
#pragma unroll
      for (int e = 0; e < 16; ++e) lds[(slot * nbt + blk) * 16 + e] = acc[e];
    }
    __syncthreads();
    if (slot == 0) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        double v = lds[blk * 16 + e];
        for (int h = 1; h < RS; ++h) v += lds[(h * nbt + blk) * 16 + e];
        acc[e] = v;
      }
    }
  }
  if (slot == 0) {
    double2 *o = reinterpret_cast<double2 *>(out + (int64_t)(b0 + blk) * 16);
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = make_double2(acc[2 * e], acc[2 * e + 1]);
  }
  if (blockIdx.z != 0) return;
  const int64_t c0 = 16 * (int64_t)a.nblk;
  if (tid == 0) {  // twin (k_hs_pair / k_hs_pair_s): the scalar, the padding and Fd
    out[c0] = scal;
    out[c0 + 1] = 0.0;                               // padding: k_hs_sum adds whole rows
    if (FD && (D & 1)) out[c0 + 2 + D] = 0.0;
  }
  if (FD) {
#pragma unroll
    for (int u = 0; u < kHsFdU; ++u) {
      const int64_t d = tid + kHsThreads * u;
      if (d < D) out[c0 + 2 + d] = fd[u];
    }
  }
}

// The staged form of the pair stage, for molecules whose rows fit LDS (hs_staged_tb: ethanol with
// TB = 32, 24 atoms with TB = 8): the same sums per row as k_hs_pair, organised so that the lanes
// work on different rows of a step of TB rows.
//   A. diff and z of the step's rows go to LDS (coalesced reads of Rt / Zt; row stride DS odd, so
//      that lanes on consecutive rows hit different banks);
//   B. thread (row, part) adds |diff|^2 and a over the entries d = part, part + 256 / TB, ...;
//   C. thread (row) adds the 256 / TB parts in part order and forms the row's scalars: one exp
//      per step and lane instead of one per row and wave;
//   D. thread (t, row) forms p_t, s_t from LDS, partners in increasing order; the threads of the
//      first D entries add the step's rows to Fd (always fused here: D <= 512);
//   E. the update of k_hs_pair.
// The chunk partials have k_hs_pair's layout.
template <int TB, bool ECSTR>
__global__ __launch_bounds__(kHsThreads) void k_hs_pair_s(HsArgs a) {
  constexpr int PARTS = kHsThreads / TB;
  extern __shared__ double lds[];
  __shared__ double spart[2][kHsThreads];
  __shared__ double sc5m[TB], scdd[TB], sci[TB], scw[TB];
  const int tid = threadIdx.x;
  const int64_t q = blockIdx.x, s = blockIdx.y;
  const int N3 = a.N3, N3P = a.N3P, n = a.n;
  const int D = (int)a.D, DS = D | 1;
  double *sp = lds, *su = lds + TB * N3P, *st = lds + 2 * TB * N3P;
  double *sd = lds + 3 * TB * N3P, *sz = sd + TB * DS, *sj = sz + TB * DS;
  // the padding entries [N3, N3P) of every row of p, u, t stay zero
  for (int e = tid; e < 3 * TB * N3P; e += kHsThreads) lds[e] = 0.0;
  // the query's compact Jacobian, read by every thread of D. in every step
  for (int e = tid; e < 3 * D; e += kHsThreads) sj[e] = a.Rddq[q * (int64_t)D * 3 + e];
  const HsMap hm = hs_map(TB, a.nblk, (int)blockIdx.z, tid);
  const int b0 = hm.b0, nbt = hm.nbt, RS = hm.RS, blk = hm.blk, slot = hm.slot;
  const bool act = slot < RS;
  int bi, bk;
  {  // twin (k_hs_pair / k_hs_pair_s): B = bi (bi + 1) / 2 + bk inverted, the sqrt estimate corrected
    const int B = b0 + blk;
    bi = (int)((sqrt(8.0 * (double)B + 1.0) - 1.0) * 0.5);
    while (bi * (bi + 1) / 2 > B) --bi;
    while ((bi + 1) * (bi + 2) / 2 <= B) ++bi;
    bk = B - bi * (bi + 1) / 2;
  }
  double acc[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.0;
  double scal = 0.0;
  double fd[kHsFdU];
#pragma unroll
  for (int u = 0; u < kHsFdU; ++u) fd[u] = 0.0;
  const double *rd = a.Rdq + q * D;
  const int64_t jb0 = (a.MP * s) / a.S, jb1 = (a.MP * (s + 1)) / a.S;
  const int step_r = kHsThreads / D, step_d = kHsThreads % D;
  const int pr = tid % TB, pp0 = tid / TB;  // B.: this thread's row and part
  for (int64_t j0 = jb0; j0 < jb1; j0 += TB) {
    const int cnt = (int)min((int64_t)TB, jb1 - j0);
    // A. entry e of the step is entry d = e % D of its row r = e / D: contiguous in Rt / Zt
    {
      const double *rt = a.Rt + j0 * D, *zt = a.Zt + j0 * D;
      int r = tid / D, d = tid % D;
      for (int e = tid; e < cnt * D; e += kHsThreads) {
        sd[r * DS + d] = rd[d] - rt[e];
        sz[r * DS + d] = zt[e];
        r += step_r;
        d += step_d;
        if (d >= D) {
          d -= D;
          ++r;
        }
      }
    }
    __syncthreads();
    // B.
    {
      double r2 = 0.0, aa = 0.0;
      if (pr < cnt) {
        const double *dr = sd + pr * DS, *zr = sz + pr * DS;
        for (int d = pp0; d < D; d += PARTS) {
          const double df = dr[d];
          r2 = fma(df, df, r2);
          aa = fma(df, zr[d], aa);
        }
      }
      spart[0][tid] = r2;
      spart[1][tid] = aa;
    }
    __syncthreads();
    // C.
    if (tid < cnt) {
      double r2 = spart[0][tid], aa = spart[1][tid];
      for (int h = 1; h < PARTS; ++h) {
        r2 += spart[0][h * TB + tid];
        aa += spart[1][h * TB + tid];
      }
      HessRow hr = hess_row(r2, aa, a.mc);
      if (ECSTR) hr = hess_row_ecstr(hr, a.Et[j0 + tid]);
      sc5m[tid] = hr.m5;
      scdd[tid] = hr.cdd;
      sci[tid] = hr.ci;
      scw[tid] = hr.w;
      scal += hr.ci;  // row tid of every step; the TB partial sums meet in row order at the end
    }
    __syncthreads();
    // D.
    if (blockIdx.z == 0) {
#pragma unroll
      for (int u = 0; u < kHsFdU; ++u) {
        const int d = tid + kHsThreads * u;
        if (d < D)
          for (int r = 0; r < cnt; ++r)
            fd[u] = fma(-scw[r], sz[r * DS + d], fma(sci[r], sd[r * DS + d], fd[u]));
      }
    }
    for (int it = tid; it < N3 * TB; it += kHsThreads) {
      const int t = it / TB, r = it % TB;
      if (r >= cnt) continue;
      const int at = t / 3, c = t % 3;
      const double *dr = sd + r * DS, *zr = sz + r * DS;
      double pp = 0.0, ss = 0.0;
#pragma unroll 4
      for (int b = 0; b < n; ++b) {
        if (b == at) continue;
        // twin of pair_idx (sgdml_pair.h) in 32-bit arithmetic (D <= 512 here)
        const int d = at > b ? at * (at - 1) / 2 + b : b * (b - 1) / 2 + at;
        const double v = sj[d * 3 + c];
        const double jv = at > b ? -v : v;
        pp = fma(jv, dr[d], pp);
        ss = fma(jv, zr[d], ss);
      }
      const double ts = -sc5m[r] * ss;
      sp[r * N3P + t] = pp;
      su[r * N3P + t] = fma(scdd[r], pp, ts);
      st[r * N3P + t] = ts;
    }
    __syncthreads();
    // E. H_ik += p_i u_k + t_i p_k on this thread's block, the rows of its slot
    if (act) {
      for (int r = slot; r < cnt; r += RS) {  // twin (k_hs_pair / k_hs_pair_s): the 4 x 4 update
        const double2 *pi = reinterpret_cast<const double2 *>(sp + r * N3P + 4 * bi);
        const double2 *ti = reinterpret_cast<const double2 *>(st + r * N3P + 4 * bi);
        const double2 *uk = reinterpret_cast<const double2 *>(su + r * N3P + 4 * bk);
        const double2 *pk = reinterpret_cast<const double2 *>(sp + r * N3P + 4 * bk);
        const double2 p0 = pi[0], p1 = pi[1], t0 = ti[0], t1 = ti[1];
        const double2 u0 = uk[0], u1 = uk[1], k0 = pk[0], k1 = pk[1];
        const double pv[4] = {p0.x, p0.y, p1.x, p1.y}, tv[4] = {t0.x, t0.y, t1.x, t1.y};
        const double uv[4] = {u0.x, u0.y, u1.x, u1.y}, kv[4] = {k0.x, k0.y, k1.x, k1.y};
#pragma unroll
        for (int x = 0; x < 4; ++x)
#pragma unroll
          for (int y = 0; y < 4; ++y)
            acc[4 * x + y] = fma(tv[x], kv[y], fma(pv[x], uv[y], acc[4 * x + y]));
      }
    }
    // no barrier here: the next step writes diff / z (read in B. and D., behind barriers), its
    // parts and scalars behind its own barriers, and p, u, t only after three of them
  }
  double *out = a.part + (s * a.nq + q) * a.PS;
  __syncthreads();  // every thread is through with the last step: lds and spart are free
  if (tid < TB) spart[0][tid] = scal;
  if (RS > 1) {  // twin (k_hs_pair / k_hs_pair_s): the slot merge and the store of the block
    if (act) {
#pragma unroll
      for (int e = 0; e < 16; ++e) lds[(slot * nbt + blk) * 16 + e] = acc[e];
    }
    __syncthreads();
    if (slot == 0) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        double v = lds[blk * 16 + e];
        for (int h = 1; h < RS; ++h) v += lds[(h * nbt + blk) * 16 + e];
        acc[e] = v;
      }
    }
  }
  if (slot == 0) {
    double2 *o = reinterpret_cast<double2 *>(out + (int64_t)(b0 + blk) * 16);
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = make_double2(acc[2 * e], acc[2 * e + 1]);
  }
  if (blockIdx.z != 0) return;
  const int64_t c0 = 16 * (int64_t)a.nblk;
  if (RS <= 1) __syncthreads();  // spart (the slots' barrier above serves otherwise)
  if (tid == 0) {  // twin (k_hs_pair / k_hs_pair_s): the scalar, the padding and Fd
    double v = spart[0][0];
    for (int r = 1; r < TB; ++r) v += spart[0][r];
    out[c0] = v;
    out[c0 + 1] = 0.0;
    if (D & 1) out[c0 + 2 + D] = 0.0;
  }
#pragma unroll
  for (int u = 0; u < kHsFdU; ++u) {
    const int d = tid + kHsThreads * u;
    if (d < D) out[c0 + 2 + d] = fd[u];
  }
}

// sum[q][e] = sum_s part[s][q][e], e < PS: chunk_sum (sgdml_pair.h), the order of k_pr_sum
__global__ __launch_bounds__(256) void k_hs_sum(const double *__restrict__ part, int64_t PS, int64_t nq,
                                                int S, double *__restrict__ sum) {
  const int64_t e = (int64_t)blockIdx.x * kSumE + threadIdx.x % kSumE, q = blockIdx.y;
  const bool ok = e < PS;
  const double fsum = chunk_sum(part + q * PS + (ok ? e : 0), nq * PS, S, ok);
  if (threadIdx.x >= kSumE || !ok) return;
  sum[q * PS + e] = fsum;
}

// H[q][i][k] = std (sum[block(I, K)] - scal (J^T J)_IK + sum_d g_d (d2rd_d / dR2)_IK), I = max(i, k),
// K = min(i, k), g = -Fd: one thread per entry of the full matrix.  Atoms A = I / 3 >= B = K / 3.
// A != B: the pair d = (A, B) alone, (J^T J)_IK = -x y and the block -g B, with x = Rdd_d[c_I],
// y = Rdd_d[c_K];  A == B: every partner b != A in increasing order, +x y and +g B.
__global__ __launch_bounds__(256) void k_hs_fin(const double *__restrict__ sum, int64_t PS,
                                                const double *__restrict__ Rd,
                                                const double *__restrict__ Rdd,
                                                const double *__restrict__ Fd, int64_t fds, int n,
                                                int64_t D, int64_t c0, double std,
                                                double *__restrict__ H) {
  const int N3 = 3 * n;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)N3 * N3) return;
  const int64_t q = blockIdx.y;
  const int i = (int)(e / N3), k = (int)(e % N3);
  const int I = max(i, k), K = min(i, k);
  const int A = I / 3, cI = I % 3, B = K / 3, cK = K % 3;
  const int bi = I / 4, bk = K / 4;
  const double *sq = sum + q * PS;
  const double hs = sq[(int64_t)(bi * (bi + 1) / 2 + bk) * 16 + (I % 4) * 4 + (K % 4)];
  const double scal = sq[c0];  // c0 = 16 nblk
  const double *rd = Rd + q * D, *jr = Rdd + q * D * 3, *fd = Fd + q * fds;  // row stride of Fd
  double val;
  if (A != B) {
    const int64_t d = pair_idx(A, B);
    const double xy = jr[d * 3 + cI] * jr[d * 3 + cK];
    const double r1 = rd[d];
    double bm = 3.0 * xy / r1;
    if (cI == cK) bm -= r1 * r1 * r1;
    // g = -Fd: -g B = +Fd B
    val = fma(fd[d], bm, fma(scal, xy, hs));
  } else {
    double jtj = 0.0, d2 = 0.0;
    for (int b = 0; b < n; ++b) {
      if (b == A) continue;
      const int64_t d = pair_idx(A, b);
      const double xy = jr[d * 3 + cI] * jr[d * 3 + cK];
      const double r1 = rd[d];
      double bm = 3.0 * xy / r1;
      if (cI == cK) bm -= r1 * r1 * r1;
      jtj += xy;
      d2 = fma(-fd[d], bm, d2);
    }
    val = fma(-scal, jtj, hs) + d2;
  }
  H[q * N3 * N3 + e] = std * val;
}

// the pair stage forms Fd itself while kHsFdU entries per thread cover D; above, the
// prediction's pair stage and chunk sum run first (pred_fd_slab)
bool hs_fused(int64_t D) { return D <= (int64_t)kHsFdU * kHsThreads; }

// rows per step of the staged form: the largest of 32, 16, 8 whose diff / z rows (stride D | 1),
// p, u, t rows and the query's Jacobian fit 56 KB of LDS beside the static 5 KB; 0: the rows do not fit (k_hs_pair)
int hs_staged_tb(int n, int64_t D) {
  if (!hs_fused(D)) return 0;
  const int64_t N3P = round_up(3 * (int64_t)n, 4), DS = D | 1;
  for (int tb : {32, 16, 8})
    if (8 * (tb * (2 * DS + 3 * N3P) + 3 * D) <= 56 * 1024) return tb;
  return 0;
}

int hs_n3p(int n) { return (int)round_up(3 * (int64_t)n, 4); }

// the slab buffers, on the first call after a model is set
int hs_prepare(mlff_ctx *ctx) {
  PredData &pd = ctx->pred;
  if (pd.hs.ready) return MLFF_OK;
  const int N3P = hs_n3p(pd.n);
  if (N3P > kHsMaxN3P) return set_error(ctx, MLFF_ERR_ARG, "predict hessian: more than 682 atoms");
  const int64_t N3 = 3 * (int64_t)pd.n, NB = N3P / 4;
  pd.hs.nblk = NB * (NB + 1) / 2;
  pd.hs.stage = hs_staged_tb(pd.n, pd.D);
  pd.hs.tb = pd.hs.stage > 0 ? pd.hs.stage : 3 * kHsTB * N3P * 8 <= 48 * 1024 ? kHsTB : 1;
  pd.hs.S = (int)std::max<int64_t>(1, std::min<int64_t>(kHsMaxChunks, pd.MP / kHsChunkRows));
  pd.hs.fd = hs_fused(pd.D);
  pd.hs.PS = 16 * pd.hs.nblk + 2 + (pd.hs.fd ? round_up(pd.D, 2) : 0);
  const int64_t PS = pd.hs.PS;
  // queries per pass: the chunk partials within 256 MB, the results within 256 MB, and no more
  // than the prediction's slab (its buffers hold the queries' descriptors and Fd; MLFF_PRED_SLAB
  // thereby bounds this slab too)
  int64_t slab = ((int64_t)256 << 20) / std::max<int64_t>((int64_t)pd.hs.S * PS * 8, N3 * N3 * 8);
  slab = std::max<int64_t>(1, std::min<int64_t>(slab, pd.slab));
  pd.hs.slab = slab;
  int rc;
  if ((rc = pd.hs.part.alloc(ctx, (int64_t)pd.hs.S * slab * PS, "predict hessian")) != MLFF_OK ||
      (rc = pd.hs.sum.alloc(ctx, slab * PS, "predict hessian")) != MLFF_OK ||
      (rc = pd.hs.H.alloc(ctx, slab * N3 * N3, "predict hessian")) != MLFF_OK ||
      (rc = pd.hs.h_out.alloc(ctx, slab * N3 * N3, "predict hessian")) != MLFF_OK) {
    pd.hs = PredData::Hess{};
    return rc;
  }
  pd.hs.ready = true;
  return MLFF_OK;
}

using HsFn = void (*)(HsArgs);

// the model part of the pair stage's arguments (after hs_prepare)
HsArgs hs_model_args(const PredData &pd) {
  HsArgs a{};
  a.Rt = pd.Rt;
  a.Zt = pd.Zt;
  a.Et = pd.Et;
  a.D = pd.D;
  a.MP = pd.MP;
  a.n = pd.n;
  a.N3 = 3 * pd.n;
  a.N3P = hs_n3p(pd.n);
  a.nblk = (int)pd.hs.nblk;
  a.mc = matern_consts(pd.sig);
  return a;
}

}  // namespace

int pred_hess_run(mlff_ctx *ctx, const double *R, int64_t Q, double *H_out) {
  MLFF_TRY(hs_prepare(ctx));
  const PredData &pd = ctx->pred;
  hipStream_t s = ctx->stream;
  const int64_t N3 = 3 * (int64_t)pd.n, D = pd.D;
  HsArgs a = hs_model_args(pd);
  a.Rdq = pd.Rdq;
  a.Rddq = pd.Rddq;
  a.S = pd.hs.S;
  a.part = pd.hs.part;
  a.PS = pd.hs.PS;
  const bool ecstr = pd.Et != nullptr;
  const int TB = pd.hs.tb;
  // one row per step means 3n > 256, far past the fused form's D
  const HsFn fn = pd.hs.stage == 32 ? (ecstr ? k_hs_pair_s<32, true> : k_hs_pair_s<32, false>)
                  : pd.hs.stage == 16 ? (ecstr ? k_hs_pair_s<16, true> : k_hs_pair_s<16, false>)
                  : pd.hs.stage == 8 ? (ecstr ? k_hs_pair_s<8, true> : k_hs_pair_s<8, false>)
                  : TB == kHsTB ? (pd.hs.fd ? (ecstr ? k_hs_pair<kHsTB, true, true> : k_hs_pair<kHsTB, false, true>)
                                          : (ecstr ? k_hs_pair<kHsTB, true, false> : k_hs_pair<kHsTB, false, false>))
                              : (ecstr ? k_hs_pair<1, true, false> : k_hs_pair<1, false, false>);
  const int64_t c0 = 16 * pd.hs.nblk;
  // p, u, t of a step, and the row slots' accumulators at the end (at most 256 x 16 doubles)
  // of the first and of the last tile (the tiles between them have 256 blocks and one slot)
  const unsigned ntile = (unsigned)((pd.hs.nblk + 255) / 256);
  int slots = 0;
  for (int nb : {(int)std::min<int64_t>(256, pd.hs.nblk), (int)(pd.hs.nblk - 256 * (int64_t)(ntile - 1))}) {
    const int rs = std::min(TB, 256 / nb);
    if (rs > 1) slots = std::max(slots, rs * nb * 16);
  }
  // diff and z of a step and the query's Jacobian
  const int staged = pd.hs.stage > 0 ? 2 * TB * (int)(D | 1) + 3 * (int)D : 0;
  const size_t lds = sizeof(double) * (size_t)std::max(3 * TB * a.N3P + staged, slots);
  for (int64_t q0 = 0; q0 < Q; q0 += pd.hs.slab) {
    const int64_t nq = std::min<int64_t>(pd.hs.slab, Q - q0);
    a.nq = nq;
    MLFF_TRY(pred_fd_slab(ctx, R + q0 * N3, nq, !pd.hs.fd));
    hipLaunchKernelGGL(fn, dim3((unsigned)nq, (unsigned)pd.hs.S, ntile), dim3(kHsThreads), lds, s, a);
    hipLaunchKernelGGL(k_hs_sum, dim3((unsigned)((a.PS + kSumE - 1) / kSumE), (unsigned)nq), dim3(256),
                       0, s, pd.hs.part, a.PS, nq, pd.hs.S, pd.hs.sum);
    hipLaunchKernelGGL(k_hs_fin, dim3((unsigned)((N3 * N3 + 255) / 256), (unsigned)nq), dim3(256), 0, s,
                       pd.hs.sum, a.PS, pd.Rdq, pd.Rddq, pd.hs.fd ? pd.hs.sum + c0 + 2 : pd.Fd,
                       pd.hs.fd ? a.PS : D, pd.n, D, c0, pd.std, pd.hs.H);
    MLFF_HIP(ctx, hipGetLastError());
    MLFF_HIP(ctx, hipMemcpyAsync(pd.hs.h_out, pd.hs.H, sizeof(double) * nq * N3 * N3,
                                 hipMemcpyDeviceToHost, s));
    // the slab buffers are reused by the next slab: the copy out must have left them
    MLFF_HIP(ctx, hipStreamSynchronize(s));
    std::memcpy(H_out + q0 * N3 * N3, pd.hs.h_out, sizeof(double) * nq * N3 * N3);
  }
  return MLFF_OK;
}

// algorithmic work of one Hessian, per (j, p) pair:
//   row scalars   5 D (diff, two fmas per entry) + 20 (sqrt, exp, m, beta, the sums' tails)
//   p and s       3n entries x (n - 1) partners x 5 (diff, two fmas) = 30 D, and 3 per entry
//                 for u and t: 9 n
//   the update    two fmas for each of the T = 3n (3n + 1) / 2 entries of the lower triangle: 4 T
//   g = -Fd       fused (D <= 512): 5 D (diff, two fmas per entry) + 2 (w); otherwise the
//                 prediction's pair stage, 9 D + 10 (19 with energy coefficients; pred_work)
// and 5 more with energy coefficients (w, two fmas).  The kernel computes whole 4 x 4 blocks, the
// diagonal ones included: 16 nblk entries instead of T (448 against 378 for ethanol); the count
// is of the triangle.  Ethanol: 36 x 40 + 81 + 1512 + 22 = 3055 flops per pair against the 334
// of a prediction.  Bytes: the Rt / Zt rows, streamed once by every pair stage that runs.
void pred_hess_work(const PredData &pd, double *flops, double *bytes) {
  const bool ecstr = pd.Et != nullptr;
  double pf = 0.0, pb = 0.0;
  pred_work(pd, &pf, &pb);
  const double D = (double)pd.D, n3 = 3.0 * pd.n;
  const double T = n3 * (n3 + 1.0) / 2.0;
  const bool fused = hs_fused(pd.D);
  *flops = (double)pd.MP * (35.0 * D + 3.0 * n3 + 4.0 * T + (ecstr ? 25.0 : 20.0) + (fused ? 5.0 * D + 2.0 : 0.0)) +
           (fused ? 0.0 : pf);
  *bytes = fused ? pb : 2.0 * pb;
}

}  // namespace mlff
