// Hessian-vector products H(R) v of a trained sGDML model at arbitrary query geometries, the
// Hessian never formed (mlff_predict_hvp).  The reference implementation has no counterpart: the
// formulas are those of kernels_predict_hess.hip applied to a vector, in the notation of that
// file and of kernels_predict.hip.
//
// For a query with descriptor rd and compact Jacobian Rdd (k_pr_desc) and a vector v (3n):
//   y = J v (D entries): row d = (a, b), a > b, is y_d = Rdd_d . (v_b - v_a)   (k_pr_jt's sign)
// and for every permuted training row jp (diff = rd - Rt[jp], z = Zt[jp], e = Et[jp] or 0):
//   rs = |diff|^2,  aa = diff . z,  bb = diff . y,  cc = z . y
//   h = hess_row(rs, aa) (hess_row_ecstr(h, e) for a constrained model: sgdml_pair.h)
//   Gy  += (h.cdd bb - h.m5 cc) diff - (h.m5 bb) z        (= G y without the -sci y term)
//   sci += h.ci,   Fd += h.ci diff - h.w z                (the prediction's Fd: the same fmas)
// after the rows Gy -= sci y, and with g = -Fd
//   H v = std [J^T Gy + sum_d g_d (B_d (v_a - v_b) to atom a, -B_d (v_a - v_b) to atom b)],
//   B_d w = 3 Rdd_d (Rdd_d . w) / rd_d - rd_d^3 w.
// One product costs about 17 D flops per row against the 64 D of the Hessian's pair stage, needs
// (KB + 1) D + 1 accumulators instead of 3n (3n + 1) / 2, and has no limit on the number of atoms.
//
// k_hv_y forms y for every (query, vector).  The pair stage shares a row among the vectors of a
// block: a workgroup owns one query, one block of at most KB of its vectors and one chunk of the
// (j, p) range; it loads every Rt / Zt (/ Et) row of the chunk once, forms rs, aa and the row's
// scalars once and uses them for all KB vectors.  KB is 4, and 1 for a pass with a single
// vector (the same arithmetic per vector, so the same bits).  Two forms, chosen by D only, as the
// prediction's (pd.form, MLFF_PRED_FORM included):
//  - register (tile form's range, D <= 288), k_hv_pair_r<L, NI, KB>: a workgroup is one wave; L
//    lanes (16 or 64) hold a row, NI entries per lane (d = l + L i), so 64 / L rows are in flight,
//    one per lane group.  rd, y, Gy and Fd of the lane's entries stay in registers; the 2 + 2 KB
//    dot products of a row meet in an xor butterfly (four DPP steps within 16 lanes, two shuffles
//    beyond), so every lane of the group holds the same bits and forms the row scalars itself.
//    No LDS, no barrier.  The lane groups' sums are added in group order at the end.
//  - stream (any D), k_hv_pair_st<KB>: 256 lanes over the descriptor entries (d = tid, tid + 256,
//    ...), a row at a time: one pass for the dots (shuffle tree per wave, the four wave sums in
//    wave order: k_pr_stream's reduction), one for the entries of Gy and Fd, which accumulate in
//    the chunk's partial with plain loads and stores of the thread's own entries.
// Chunk partials part[s][q, block][PS]: Gy of the block's vectors (KB x D), Fd (D), sci.  k_hv_sum
// adds the chunks with chunk_sum (k_pr_sum's fixed order; a model of one chunk needs no sum: its
// partial is read in place); k_hv_fin subtracts sci y, forms J^T Gy with the partners in
// increasing order (k_pr_jt's order), adds the second-derivative term and the std scale and
// writes HV[q][k][0 .. 3n).  A pass (at most slab queries x kHvPass vectors each) uploads its
// geometries and vectors in one copy; the descriptors come from the prediction's own kernel
// (k_desc_t<true>, sgdml_pair.h) and go to the prediction's slab buffers.
//
// Determinism: no atomics; the chunk count and every reduction order depend on the model (M
// n_perms, D, form, constrained or not) only; no sum runs across queries or across vectors, and
// a vector's arithmetic does not depend on its slot in the block: HV[q][k] has the same bits
// whatever K, the position of k, the batch, the slab or the device split.  A vector slot past K
// carries y = 0 and writes zeros.  The ECSTR terms enter through hess_row_ecstr's fmas:
// alphas_E = 0 gives the unconstrained model's bits.  All instantiations must round alike, so
// every product that feeds a sum does so as the addend or a factor of an explicit fma (into which
// the compiler contracts nothing further; __dmul_rn and __dadd_rn are plain * and + to it), and
// the one plain sum of a product, sci += h.ci, takes it through hv_opaque.
#include "common.h"
#include "sgdml_pair.h"

#include <algorithm>
#include <cstring>

namespace mlff {

namespace {

constexpr int kHvKB = 4;                 // vectors per block of the pair stage
constexpr int kHvPass = 8;               // vectors of a query per pass: two blocks
constexpr int kHvChunkRows = 32;         // register form: (j, p) rows per chunk, at least
constexpr int kHvMaxChunks = 256;        // register form: chunks, at most
constexpr int kHvStreamRows = 2;         // stream form: rows per chunk
constexpr int kHvStreamMaxChunks = 4096;
constexpr int64_t kHvMaxSlab = 4096;     // queries per pass: kHvPass x slab products fit gridDim.y

struct HvArgs {
  const double *Rdq;   // nq x D
  const double *Y;     // nq x kk x D
  const double *Rt, *Zt, *Et;
  int64_t D, nq, MP;
  int S;               // chunks (gridDim.y)
  int kk;              // vectors of every query in this pass
  int nkb;             // vector blocks per query: kk / KB rounded up (gridDim.x = nq nkb)
  MaternConsts mc;     // sgdml_pair.h
  double *part;        // S x (nq nkb) x PS
  int64_t PS;          // (KB + 1) D + 1 rounded up to 2
};

// Y[q, k][d] = Rdd_q[d] . (v_b - v_a), d = pair(a, b), a > b, for the nq x kk vectors V
__global__ __launch_bounds__(256) void k_hv_y(const double *__restrict__ Rdd,
                                              const double *__restrict__ V, int n, int64_t D, int kk,
                                              double *__restrict__ Y) {
  const int64_t p = blockIdx.y, q = p / kk;
  const double *v = V + p * 3 * n;
  const double *jr = Rdd + q * D * 3;
  for (int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x; d < D; d += (int64_t)gridDim.x * 256) {
    const TriIdx ab = tri_invert(d);
    const double w0 = v[ab.b * 3 + 0] - v[ab.a * 3 + 0];
    const double w1 = v[ab.b * 3 + 1] - v[ab.a * 3 + 1];
    const double w2 = v[ab.b * 3 + 2] - v[ab.a * 3 + 2];
    Y[p * D + d] = fma(jr[d * 3 + 2], w2, fma(jr[d * 3 + 1], w1, __dmul_rn(jr[d * 3 + 0], w0)));
  }
}

// the coefficients of diff and of -z in a vector's Gy for one row
struct HvCoef { double c1, c2; };
__device__ __forceinline__ HvCoef hv_coef(HessRow h, double bb, double cc) {
  return {fma(h.cdd, bb, -__dmul_rn(h.m5, cc)), __dmul_rn(h.m5, bb)};
}

// h.ci is a bare product in the unconstrained instantiations and an fma in the constrained ones:
// behind this barrier neither is contracted into the sum sci += h.ci (__dadd_rn is a plain +)
__device__ __forceinline__ double hv_opaque(double x) {
  asm volatile("" : "+v"(x));
  return x;
}

// sum over the L lanes of a row's group (16: a DPP row; 64: the wave), xor partners: each step
// adds a commutative pair, so every lane ends with the same bits.  All 64 lanes take part.
template <int L>
__device__ __forceinline__ double lanes_sum(double v) {
  static_assert(L == 16 || L == 64, "a DPP row or the wave");
  v += dpp_f64<0xB1>(v);   // quad_perm(1, 0, 3, 2)
  v += dpp_f64<0x4E>(v);   // quad_perm(2, 3, 0, 1)
  v += dpp_f64<0x141>(v);  // row_half_mirror
  v += dpp_f64<0x140>(v);  // row_mirror
  if (L == 64) {
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
  }
  return v;
}

// Register form: see the head of the file.  Lane (g, l) = (lane / L, lane % L) works on the rows
// jb0 + g, jb0 + g + 64 / L, ... of the chunk and on the entries d = l + L i, i < NI.  A row past
// the chunk's end and an entry past D load zeros (so the butterflies run with every lane) and
// add nothing.
template <int L, int NI, int KB, bool ECSTR>
__global__ __launch_bounds__(64) void k_hv_pair_r(HvArgs a) {
  constexpr int RW = 64 / L;  // rows in flight
  const int lane = threadIdx.x, l = lane % L, g = lane / L;
  const int64_t pb = blockIdx.x, s = blockIdx.y;
  const int64_t q = pb / a.nkb;
  const int kb = (int)(pb % a.nkb);
  const int64_t D = a.D;
  double rd[NI], fd[NI], y[KB][NI], gy[KB][NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int64_t d = l + L * i;
    rd[i] = d < D ? a.Rdq[q * D + d] : 0.0;
    fd[i] = 0.0;
#pragma unroll
    for (int u = 0; u < KB; ++u) {
      const int k = kb * KB + u;
      y[u][i] = (k < a.kk && d < D) ? a.Y[(q * a.kk + k) * D + d] : 0.0;
      gy[u][i] = 0.0;
    }
  }
  double sci = 0.0;
  const int64_t jb0 = (a.MP * s) / a.S, jb1 = (a.MP * (s + 1)) / a.S;
  for (int64_t j0 = jb0; j0 < jb1; j0 += RW) {
    const int64_t j = j0 + g;
    const bool live = j < jb1;
    const double *rt = a.Rt + (live ? j : jb0) * D, *zt = a.Zt + (live ? j : jb0) * D;
    double df[NI], z[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int64_t d = l + L * i;
      const bool ok = live && d < D;
      df[i] = ok ? rd[i] - rt[d] : 0.0;
      z[i] = ok ? zt[d] : 0.0;
    }
    const double ej = (ECSTR && live) ? a.Et[j] : 0.0;
    double rs = 0.0, aa = 0.0, bb[KB], cc[KB];
#pragma unroll
    for (int u = 0; u < KB; ++u) bb[u] = cc[u] = 0.0;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      rs = fma(df[i], df[i], rs);
      aa = fma(df[i], z[i], aa);
#pragma unroll
      for (int u = 0; u < KB; ++u) {
        bb[u] = fma(df[i], y[u][i], bb[u]);
        cc[u] = fma(z[i], y[u][i], cc[u]);
      }
    }
    rs = lanes_sum<L>(rs);
    aa = lanes_sum<L>(aa);
#pragma unroll
    for (int u = 0; u < KB; ++u) {
      bb[u] = lanes_sum<L>(bb[u]);
      cc[u] = lanes_sum<L>(cc[u]);
    }
    HessRow h = hess_row(rs, aa, a.mc);
    if (ECSTR) h = hess_row_ecstr(h, ej);
    h.ci = hv_opaque(h.ci);
    if (live) {
      sci = __dadd_rn(sci, h.ci);
#pragma unroll
      for (int u = 0; u < KB; ++u) {
        const HvCoef c = hv_coef(h, bb[u], cc[u]);
#pragma unroll
        for (int i = 0; i < NI; ++i) gy[u][i] = fma(-c.c2, z[i], fma(c.c1, df[i], gy[u][i]));
      }
#pragma unroll
      for (int i = 0; i < NI; ++i) fd[i] = fma(-h.w, z[i], fma(h.ci, df[i], fd[i]));
    }
  }
  // the lane groups in group order (every lane of group 0 ends with the sums of its entries)
  auto merge = [&](double x) {
    double v = __shfl(x, l, 64);
#pragma unroll
    for (int h = 1; h < RW; ++h) v += __shfl(x, l + L * h, 64);
    return v;
  };
  if (RW > 1) {
    sci = merge(sci);
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      fd[i] = merge(fd[i]);
#pragma unroll
      for (int u = 0; u < KB; ++u) gy[u][i] = merge(gy[u][i]);
    }
  }
  if (g != 0) return;
  double *out = a.part + (s * a.nq * a.nkb + pb) * a.PS;
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int64_t d = l + L * i;
    if (d < D) {
#pragma unroll
      for (int u = 0; u < KB; ++u) out[u * D + d] = gy[u][i];
      out[KB * D + d] = fd[i];
    }
  }
  if (l == 0) {
    out[(KB + 1) * D] = sci;
    if ((KB + 1) * D + 1 < a.PS) out[(KB + 1) * D + 1] = 0.0;  // padding: k_hv_sum adds whole rows
  }
}

// Stream form: see the head of the file.  A thread owns the same entries in every row, so the
// chunk's partial accumulates in part (first row: stores only).
template <int KB, bool ECSTR>
__global__ __launch_bounds__(256) void k_hv_pair_st(HvArgs a) {
  constexpr int NV = 2 + 2 * KB;
  __shared__ double sh[4][NV];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t pb = blockIdx.x, s = blockIdx.y;
  const int64_t q = pb / a.nkb;
  const int kb = (int)(pb % a.nkb);
  const int64_t D = a.D;
  const double *__restrict__ rd = a.Rdq + q * D;
  const double *__restrict__ yk[KB];
  bool kok[KB];
#pragma unroll
  for (int u = 0; u < KB; ++u) {
    const int k = kb * KB + u;
    kok[u] = k < a.kk;
    yk[u] = a.Y + (q * a.kk + (kok[u] ? k : 0)) * D;
  }
  double *__restrict__ out = a.part + (s * a.nq * a.nkb + pb) * a.PS;
  double sci = 0.0;
  const int64_t jb0 = (a.MP * s) / a.S, jb1 = (a.MP * (s + 1)) / a.S;
  for (int64_t j = jb0; j < jb1; ++j) {
    const double *__restrict__ rt = a.Rt + j * D;
    const double *__restrict__ zt = a.Zt + j * D;
    double acc[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[v] = 0.0;
#pragma unroll 2
    for (int64_t d = tid; d < D; d += 256) {
      const double df = rd[d] - rt[d], z = zt[d];
      acc[0] = fma(df, df, acc[0]);
      acc[1] = fma(df, z, acc[1]);
#pragma unroll
      for (int u = 0; u < KB; ++u) {
        const double yv = kok[u] ? yk[u][d] : 0.0;
        acc[2 + 2 * u] = fma(df, yv, acc[2 + 2 * u]);
        acc[3 + 2 * u] = fma(z, yv, acc[3 + 2 * u]);
      }
    }
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[v] = wave_sum(acc[v]);
    const double ej = ECSTR ? a.Et[j] : 0.0;  // in flight across the two barriers
    __syncthreads();  // sh of the previous row is consumed
    if (lane == 0) {
#pragma unroll
      for (int v = 0; v < NV; ++v) sh[wv][v] = acc[v];
    }
    __syncthreads();
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[v] = (sh[0][v] + sh[1][v]) + (sh[2][v] + sh[3][v]);
    HessRow h = hess_row(acc[0], acc[1], a.mc);
    if (ECSTR) h = hess_row_ecstr(h, ej);
    h.ci = hv_opaque(h.ci);
    sci = __dadd_rn(sci, h.ci);
    HvCoef c[KB];
#pragma unroll
    for (int u = 0; u < KB; ++u) c[u] = hv_coef(h, acc[2 + 2 * u], acc[3 + 2 * u]);
    const bool first = j == jb0;
#pragma unroll 2
    for (int64_t d = tid; d < D; d += 256) {
      const double df = rd[d] - rt[d], z = zt[d];
#pragma unroll
      for (int u = 0; u < KB; ++u) {
        const double g0 = first ? 0.0 : out[u * D + d];
        out[u * D + d] = fma(-c[u].c2, z, fma(c[u].c1, df, g0));
      }
      const double f0 = first ? 0.0 : out[KB * D + d];
      out[KB * D + d] = fma(-h.w, z, fma(h.ci, df, f0));
    }
  }
  if (tid == 0) {
    out[(KB + 1) * D] = sci;
    if ((KB + 1) * D + 1 < a.PS) out[(KB + 1) * D + 1] = 0.0;  // padding: k_hv_sum adds whole rows
  }
}

// sum[b][e] = sum_s part[s][b][e], e < PS, for the nb (query, block) rows: chunk_sum
// (sgdml_pair.h), the order of k_pr_sum and k_hs_sum
__global__ __launch_bounds__(256) void k_hv_sum(const double *__restrict__ part, int64_t PS, int64_t nb,
                                                int S, double *__restrict__ sum) {
  const int64_t e = (int64_t)blockIdx.x * kSumE + threadIdx.x % kSumE, b = blockIdx.y;
  const bool ok = e < PS;
  const double fsum = chunk_sum(part + b * PS + (ok ? e : 0), nb * PS, S, ok);
  if (threadIdx.x >= kSumE || !ok) return;
  sum[b * PS + e] = fsum;
}

// HV[q, k][3 at + c] = std (sum_b (+-) Rdd[pair(at, b)][c] (Gy - sci y)[pair(at, b)]
//                           + sum_b g (B (v_at - v_b))[c]),  g = -Fd,
// partners b in increasing order: one thread per entry.  The sign of the second sum is the same
// for at > b and at < b: atom a of the pair takes +B (v_a - v_b), atom b takes -B (v_a - v_b).
__global__ __launch_bounds__(64) void k_hv_fin(const double *__restrict__ sum, int64_t PS, int KB, int kk,
                                               int nkb, const double *__restrict__ Rd,
                                               const double *__restrict__ Rdd,
                                               const double *__restrict__ Y, const double *__restrict__ V,
                                               int n, int64_t D, double std, double *__restrict__ HV) {
  const int r = blockIdx.x * 64 + threadIdx.x;
  if (r >= 3 * n) return;
  const int64_t p = blockIdx.y, q = p / kk;
  const int k = (int)(p % kk);
  const double *sq = sum + (q * nkb + k / KB) * PS;
  const double *gy = sq + (int64_t)(k % KB) * D, *fd = sq + (int64_t)KB * D;
  const double sci = sq[(int64_t)(KB + 1) * D];
  const double *rd = Rd + q * D, *jr = Rdd + q * D * 3, *y = Y + p * D, *v = V + p * 3 * n;
  const int at = r / 3, c = r % 3;
  const double va0 = v[at * 3 + 0], va1 = v[at * 3 + 1], va2 = v[at * 3 + 2];
  double jt = 0.0, d2 = 0.0;
  for (int b = 0; b < n; ++b) {
    if (b == at) continue;
    const int64_t d = pair_idx(at, b);
    const double x0 = jr[d * 3 + 0], x1 = jr[d * 3 + 1], x2 = jr[d * 3 + 2];
    const double xc = c == 0 ? x0 : c == 1 ? x1 : x2;
    jt = fma(at > b ? -xc : xc, fma(-sci, y[d], gy[d]), jt);
    const double w0 = va0 - v[b * 3 + 0], w1 = va1 - v[b * 3 + 1], w2 = va2 - v[b * 3 + 2];
    const double wc = c == 0 ? w0 : c == 1 ? w1 : w2;
    const double dot = fma(x2, w2, fma(x1, w1, __dmul_rn(x0, w0)));
    const double r1 = rd[d];
    const double bw = fma(-__dmul_rn(__dmul_rn(r1, r1), r1), wc, __dmul_rn(__dmul_rn(3.0, xc), dot) / r1);
    d2 = fma(-fd[d], bw, d2);
  }
  HV[p * 3 * n + r] = __dmul_rn(std, __dadd_rn(jt, d2));
}

using HvFn = void (*)(HvArgs);

struct HvVariant {
  int L, NI;
  HvFn fn[2][2];  // [a block of kHvKB vectors, else one][energy coefficients]
};
template <int L, int NI>
constexpr HvVariant hv_variant() {
  return {L, NI,
          {{k_hv_pair_r<L, NI, 1, false>, k_hv_pair_r<L, NI, 1, true>},
           {k_hv_pair_r<L, NI, kHvKB, false>, k_hv_pair_r<L, NI, kHvKB, true>}}};
}
// L lanes per row, NI entries per lane; the first variant that covers D is used
const HvVariant kHvVariants[] = {
    hv_variant<16, 3>(),  // D <= 48  (n <= 10; ethanol: 36 of 48 entries)
    hv_variant<64, 2>(),  // D <= 128 (n <= 16)
    hv_variant<64, 3>(),  // D <= 192 (n <= 20)
    hv_variant<64, 5>(),  // D <= 320 (n <= 25: past the tile form's 288)
};
const HvVariant *hv_variant_of(int64_t D) {
  for (const HvVariant &v : kHvVariants)
    if (D <= (int64_t)v.L * v.NI) return &v;
  return nullptr;
}

int64_t hv_ps(int KB, int64_t D) { return round_up((int64_t)(KB + 1) * D + 1, 2); }

// the chunk count and the slab buffers, on the first call after a model is set
int hv_prepare(mlff_ctx *ctx) {
  PredData &pd = ctx->pred;
  if (pd.hv.ready) return MLFF_OK;
  const int64_t D = pd.D, N3 = 3 * (int64_t)pd.n;
  constexpr int64_t kBlocks = kHvPass / kHvKB;  // vector blocks of a query per pass
  const int64_t PS = hv_ps(kHvKB, D);
  const int64_t per_chunk = kBlocks * PS * 8;   // bytes of one query's partials per chunk
  int64_t S;
  if (pd.form == 0) {
    if (hv_variant_of(D) == nullptr) return set_error(ctx, MLFF_ERR_ARG, "predict hvp: no register form for this D");
    S = std::max<int64_t>(1, std::min<int64_t>(kHvMaxChunks, pd.MP / kHvChunkRows));
  } else {
    // one query's partials within 512 MB (long descriptors)
    S = std::min<int64_t>(kHvStreamMaxChunks, (pd.MP + kHvStreamRows - 1) / kHvStreamRows);
    S = std::max<int64_t>(1, std::min<int64_t>(S, ((int64_t)512 << 20) / per_chunk));
  }
  // queries per pass: the chunk partials within 256 MB, and no more than the prediction's slab
  // (its buffers hold the queries' descriptors; MLFF_PRED_SLAB thereby bounds this slab too)
  int64_t slab = ((int64_t)256 << 20) / (S * per_chunk);
  slab = std::max<int64_t>(1, std::min<int64_t>(slab, std::min<int64_t>(pd.slab, kHvMaxSlab)));
  pd.hv.S = (int)S;
  pd.hv.PS = PS;
  pd.hv.slab = slab;
  int rc;
  if ((rc = pd.hv.V.alloc(ctx, slab * (kHvPass + 1) * N3, "predict hvp")) != MLFF_OK ||
      (rc = pd.hv.Y.alloc(ctx, slab * kHvPass * D, "predict hvp")) != MLFF_OK ||
      (rc = pd.hv.part.alloc(ctx, S * slab * kBlocks * PS, "predict hvp")) != MLFF_OK ||
      (rc = pd.hv.sum.alloc(ctx, slab * kBlocks * PS, "predict hvp")) != MLFF_OK ||
      (rc = pd.hv.HV.alloc(ctx, slab * kHvPass * N3, "predict hvp")) != MLFF_OK ||
      (rc = pd.hv.h_v.alloc(ctx, slab * (kHvPass + 1) * N3, "predict hvp")) != MLFF_OK ||
      (rc = pd.hv.h_out.alloc(ctx, slab * kHvPass * N3, "predict hvp")) != MLFF_OK) {
    pd.hv = PredData::Hvp{};
    return rc;
  }
  pd.hv.ready = true;
  return MLFF_OK;
}

}  // namespace

int pred_hvp_run(mlff_ctx *ctx, const double *R, const double *V, int64_t Q, int64_t K, double *HV_out) {
  MLFF_TRY(hv_prepare(ctx));
  const PredData &pd = ctx->pred;
  hipStream_t s = ctx->stream;
  const int64_t N3 = 3 * (int64_t)pd.n, D = pd.D;
  const bool ecstr = pd.Et != nullptr;
  HvArgs a{};
  a.Rdq = pd.Rdq;
  a.Y = pd.hv.Y;
  a.Rt = pd.Rt;
  a.Zt = pd.Zt;
  a.Et = pd.Et;
  a.D = D;
  a.MP = pd.MP;
  a.S = pd.hv.S;
  a.mc = matern_consts(pd.sig);
  a.part = pd.hv.part;
  const unsigned gd = (unsigned)std::min<int64_t>((D + 255) / 256, 64);
  double *Rq = pd.hv.V, *Vq = nullptr;  // a pass's geometries, then its vectors: one copy in
  for (int64_t q0 = 0; q0 < Q; q0 += pd.hv.slab) {
    const int64_t nq = std::min<int64_t>(pd.hv.slab, Q - q0);
    for (int64_t k0 = 0; k0 < K; k0 += kHvPass) {
      const int kk = (int)std::min<int64_t>(kHvPass, K - k0);
      const int KB = kk == 1 ? 1 : kHvKB;
      const int nkb = (kk + KB - 1) / KB;
      const int64_t nb = nq * nkb, np = nq * kk;
      a.nq = nq;
      a.kk = kk;
      a.nkb = nkb;
      a.PS = hv_ps(KB, D);
      Vq = Rq + nq * N3;
      std::memcpy(pd.hv.h_v, R + q0 * N3, sizeof(double) * nq * N3);
      for (int64_t i = 0; i < nq; ++i)
        std::memcpy(pd.hv.h_v + (nq + i * kk) * N3, V + ((q0 + i) * K + k0) * N3, sizeof(double) * kk * N3);
      MLFF_HIP(ctx, hipMemcpyAsync(Rq, pd.hv.h_v, sizeof(double) * (nq + np) * N3, hipMemcpyHostToDevice, s));
      // the queries' descriptors into the prediction's slab buffers: its kernel, so its bits
      // (once per slab: a later pass over the vectors finds them there)
      if (k0 == 0)
        hipLaunchKernelGGL(k_desc_t<true>, dim3(gd, (unsigned)nq), dim3(256), 0, s, Rq, pd.n, pd.Rdq.get(),
                           pd.Rddq.get());
      hipLaunchKernelGGL(k_hv_y, dim3(gd, (unsigned)np), dim3(256), 0, s, pd.Rddq, Vq, pd.n, D, kk, pd.hv.Y);
      if (pd.form == 0) {
        hipLaunchKernelGGL(hv_variant_of(D)->fn[KB != 1][ecstr], dim3((unsigned)nb, (unsigned)a.S), dim3(64),
                           0, s, a);
      } else {
        const HvFn fn = KB == 1 ? (ecstr ? k_hv_pair_st<1, true> : k_hv_pair_st<1, false>)
                                : (ecstr ? k_hv_pair_st<kHvKB, true> : k_hv_pair_st<kHvKB, false>);
        hipLaunchKernelGGL(fn, dim3((unsigned)nb, (unsigned)a.S), dim3(256), 0, s, a);
      }
      // one chunk (a model of fewer than two chunks' rows): its partial is the sum
      if (a.S > 1)
        hipLaunchKernelGGL(k_hv_sum, dim3((unsigned)((a.PS + kSumE - 1) / kSumE), (unsigned)nb), dim3(256), 0,
                           s, pd.hv.part, a.PS, nb, a.S, pd.hv.sum);
      hipLaunchKernelGGL(k_hv_fin, dim3((unsigned)((N3 + 63) / 64), (unsigned)np), dim3(64), 0, s,
                         a.S > 1 ? pd.hv.sum.get() : pd.hv.part.get(), a.PS, KB, kk, nkb, pd.Rdq, pd.Rddq,
                         pd.hv.Y, Vq, pd.n, D, pd.std, pd.hv.HV);
      MLFF_HIP(ctx, hipGetLastError());
      MLFF_HIP(ctx, hipMemcpyAsync(pd.hv.h_out, pd.hv.HV, sizeof(double) * np * N3, hipMemcpyDeviceToHost, s));
      // the pass buffers are reused by the next pass: the copy out must have left them
      MLFF_HIP(ctx, hipStreamSynchronize(s));
      for (int64_t i = 0; i < nq; ++i)
        std::memcpy(HV_out + ((q0 + i) * K + k0) * N3, pd.hv.h_out + i * kk * N3, sizeof(double) * kk * N3);
    }
  }
  return MLFF_OK;
}

// algorithmic work per (j, p) row.  Shared by the vectors of a block:
//   diff, rs, aa   5 D       the row scalars  22 (hess_row: sqrt, exp, m, beta, w; 27 with energy
//   Fd             4 D                            coefficients)
// per vector:
//   bb, cc         4 D       Gy  4 D          the two coefficients  5
// One product alone (K = 1, what is reported) costs 17 D + 27 per row: 639 for ethanol against
// the Hessian's 3055 and the prediction's 334; a vector of a full block (9 D + 22) / kHvKB +
// 8 D + 5.  Bytes: the Rt / Zt (/ Et) rows, which every vector block of a query streams once in
// the register form and twice in the stream form (a pass for the dots, one for the entries).
void pred_hvp_work(const PredData &pd, double *flops, double *bytes) {
  const bool ecstr = pd.Et != nullptr;
  double pf = 0.0, pb = 0.0;
  pred_work(pd, &pf, &pb);
  *flops = (double)pd.MP * (17.0 * (double)pd.D + (ecstr ? 32.0 : 27.0));
  *bytes = pd.form == 0 ? pb : 2.0 * pb;
}

}  // namespace mlff
