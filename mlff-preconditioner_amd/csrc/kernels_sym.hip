// Symmetric tiled kernel operator: y = sigma * K v + lam * v reading only the
// lower block triangle of K (half the HBM bytes of the dense row GEMV).
//
// Reference operator: K_op (src/sGDML/sgdml/solvers/iterative_solver.py:383-445),
// the sGDML kernel is symmetric by construction (train.py:81-236 mirrors the lower
// block triangle); the RBF kernel (src/tools/utils.py:173-187) is symmetric entry
// by entry.  SURVEY §8d: "if symmetric (half) storage is ever used, still report
// against 8 N^2 and state it".
//
// Storage: the padded global index space [0, Np) (Np = nb * B, the rank-block
// `pos` coordinates of the dense layout) is cut into B x B tiles; tile (I, J),
// I >= J, is stored contiguously (B x B row-major) once, by exactly one rank.
// Diagonal tiles are stored full.
//
// Mat-vec: one workgroup per stored tile.  Each wave streams B/4 rows of the tile
// (lane = 4 double2 columns, non-temporal 16-B loads) and forms
//   row partials  s_i = sum_c A[i, c] v[J B + c]      -> slot J of row I B + i
//   column partials t_c = sum_i A[i, c] v[I B + i]    -> slot I of row J B + c (I > J)
// Row partials of a batch of 8 rows are summed across the 64 lanes through a
// wave-private LDS transpose (8 stores, 4 loads, 3 exchanges per batch); column
// partials stay in registers for the whole tile and are combined across the 4
// waves through LDS.
// Every (slot, row) of the slot buffer P (nb x Np) is written by exactly one tile
// (no atomics), and a second kernel sums the nb slots of each row in a fixed
// order -> the result is bitwise deterministic.
//
// Tiles that were generated from the RBF points (k_sym_gen_rbf) need not all be read
// again: in k_symv_dyn<true> two of the three resident workgroups of every CU evaluate the
// entries of their tiles from the points (the stored bits) on the fp64 pipe that the stream
// leaves idle, while the third one streams.
#include "common.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace mlff {

typedef double d2 __attribute__((ext_vector_type(2)));

namespace {

constexpr int B = kSymTile;  // 512
constexpr int kRB = 8;  // rows per batch (loads in flight per wave: kRB x 4 KB)
constexpr int kBatches = B / kRB;  // 8-row batches per tile
// LDS doubles of a tile workgroup: v[I B .. I B + B) | the tile's row partials | 4 x B column
// partials | the 4 waves' private kRB x 64 transpose buffers (| the generating role's row points)
constexpr int kTileRed = 6 * B;  // the transpose buffers' offset
constexpr int kTileLds = kTileRed + 4 * kRB * 64;
// the generating role's row points behind them: 3 doubles per row, then one bit per row (inside
// [0, N) / padding) in B / 32 words.  53,328 bytes in all: three workgroups fit the CU's 160 KB
// (allocated in units of 1280 bytes, so at most 53,760 each)
constexpr int kGenRowLds = kSymGenMaxD * B + B / 64;

// Work units: [0, nwhole) one whole tile each, then 2^lsub units per remaining tile, one row
// slice (512 >> lsub rows, batches [gb0, gb1)) each, so a launch ends on sub-tile units instead
// of a partial round of whole tiles (a lone 2-MB tile streams at one CU's rate).  Sub-unit
// h > 0 writes its column partials to plane h - 1 of Pq (sym_build).
__device__ __forceinline__ void decode_unit(long long u, int nwhole, int lsub, int &tile, int &h,
                                            int &gb0, int &gb1) {
  if (u < nwhole) {
    tile = (int)u;
    h = 0;
    gb0 = 0;
    gb1 = kBatches;
  } else {
    const long long q = u - nwhole;
    tile = nwhole + (int)(q >> lsub);
    h = (int)(q & ((1 << lsub) - 1));
    gb0 = h * (kBatches >> lsub);
    gb1 = gb0 + (kBatches >> lsub);
  }
}

// rho of the gathered partials (every rank's kVecGrid rho partials in its gb block, after z):
// k_update_p_gathered's sum -- thread f adds partials f, f + 256, ... in order (8 in flight),
// then block_sum256 -- so every workgroup that forms it holds the same bits
__device__ __forceinline__ double gathered_rho(const PGather &pg, double *sh) {
  double v = 0.0;
  const int np = pg.world * kVecGrid;
  int f = threadIdx.x;
  for (; f + 7 * 256 < np; f += 8 * 256) {
    double t[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int g = f + u * 256;
      t[u] = pg.gb[(int64_t)(g / kVecGrid) * pg.gstride + pg.blk + (g % kVecGrid)];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) v += t[u];
  }
  for (; f < np; f += 256) v += pg.gb[(int64_t)(f / kVecGrid) * pg.gstride + pg.blk + (f % kVecGrid)];
  v = block_sum256(v, sh);
  __syncthreads();
  if (threadIdx.x == 0) sh[4] = v;
  __syncthreads();
  const double rho = sh[4];
  __syncthreads();
  return rho;
}

// operand entries of the fused form: p = fma(beta, p_old, z) (z at iteration 1), z from the
// gather buffer -- k_update_p_gathered's arithmetic, the same bits.  Entries past the ranks'
// blocks (one rank: blk = round_up(n, 64) < Np = round_up(n, 512), the tile padding) are zero,
// as the unfused operand's padding is: the gather buffer holds world blocks only.  blk is a
// multiple of 64, so a d2 pair never straddles two blocks.
__device__ __forceinline__ double pg_z(const PGather &pg, int64_t i) {
  const int64_t rk = i / pg.blk;
  return rk < pg.world ? pg.gb[rk * pg.gstride + i % pg.blk] : 0.0;
}
__device__ __forceinline__ double pg_val(const PGather &pg, const double *v, int64_t i, double beta) {
  return pg.it > 1 ? fma(beta, v[i], pg_z(pg, i)) : pg_z(pg, i);
}
__device__ __forceinline__ d2 pg_val2(const PGather &pg, const double *v, int64_t i, double beta) {
  if (pg.gb == nullptr) return *reinterpret_cast<const d2 *>(v + i);
  const int64_t rk = i / pg.blk;
  const d2 z = rk < pg.world ? *reinterpret_cast<const d2 *>(pg.gb + rk * pg.gstride + i % pg.blk)
                             : d2{0.0, 0.0};
  if (pg.it <= 1) return z;
  const d2 po = *reinterpret_cast<const d2 *>(v + i);
  return d2{fma(beta, po.x, z.x), fma(beta, po.y, z.y)};
}

// beta of the fused p update from the iteration's rho; block 0 passes rho on (k_symv_dyn, which
// summed it: to st->rho_new for the slot reduction; the slot reduction, which writes p after
// every tile has read p_old: to st->rho)
__device__ __forceinline__ double fused_p_beta(const PGather &pg, double rho, double *publish) {
  const double beta = pg.it > 1 ? rho / pg.st->rho1 : 0.0;
  if (blockIdx.x == 0 && threadIdx.x == 0) *publish = rho;
  return beta;
}

// Work counters of k_symv_dyn (sp.ticket): [0] the streaming role's whole tiles (every unit
// when nothing is generated), [1] k_sym_reduce_w's arrival counter, [2] the generating role's
// whole tiles, [3] the quarter units either role takes once its own range is exhausted.
// Every slot reduction resets the three work counters for the next launch.  Behind them the
// kSymCuWords per-CU arrival words of the role rule (zeroed at allocation, never reset).
constexpr int kTicketWords = 4;
__device__ __forceinline__ void reset_work_counters(unsigned long long *ticket) {
  ticket[0] = 0ull;
  ticket[2] = 0ull;
  ticket[3] = 0ull;
}

// The unit ranges a workgroup takes from, in its order: range r is [base_r + count, hi_r)
// through counter c_r.  A role's first range is its own; the others are the other role's whole
// tiles and the quarter units, so every range is finished however many workgroups hold either
// role (all of them in one role included).
struct UnitQueue {
  unsigned long long *c0, *c1, *c2;
  long long base0, hi0, base1, hi1, base2, hi2;
  int stage;
};
__device__ __forceinline__ bool take_unit(unsigned long long *c, long long base, long long hi,
                                          long long &u) {
  if (base >= hi) return false;
  u = base + (long long)atomicAdd(c, 1ull);
  return u < hi;
}
// next unit (thread 0); >= nunits: nothing left.  Nobody waits for anybody: a wrong count
// gives a wrong sum, never a hang.
__device__ __forceinline__ long long next_unit(UnitQueue &q, long long nunits) {
  long long u;
  if (q.stage == 0) {
    if (take_unit(q.c0, q.base0, q.hi0, u)) return u;
    q.stage = 1;
  }
  if (q.stage == 1) {
    if (take_unit(q.c1, q.base1, q.hi1, u)) return u;
    q.stage = 2;
  }
  if (q.stage == 2) {
    if (take_unit(q.c2, q.base2, q.hi2, u)) return u;
    q.stage = 3;
  }
  return nunits;
}

// global index of padded position pos (k_sym_gen_rbf's mapping); false: padding (K is zero)
__device__ __forceinline__ bool gen_index(const SymGen &gs, int64_t pos, int64_t &g) {
  const int64_t off = pos % gs.blk;
  g = (pos / gs.blk) * gs.rows_per + off;
  return off < gs.rows_per && g < gs.N;
}

// The lane's 8 columns (2 (lane + 64 q) + e) of a generated tile: their points, zero past d
// and in the padding (a zero difference adds nothing to the squared distance: fma(0, 0, s)
// == s), and which of them are inside [0, N)
struct GenCols {
  double x[8][kSymGenMaxD];
  unsigned valid;
};
__device__ __forceinline__ void gen_load_cols(const SymGen &gs, int J, int lane, GenCols &gc) {
  gc.valid = 0u;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    int64_t g;
    const bool ok = gen_index(gs, (int64_t)J * B + 2 * (lane + 64 * (j >> 1)) + (j & 1), g);
    if (ok) gc.valid |= 1u << j;
#pragma unroll
    for (int t = 0; t < kSymGenMaxD; ++t) gc.x[j][t] = (ok && t < gs.d) ? gs.Xs[g * gs.d + t] : 0.0;
  }
}
// row points of rows [r0, r0 + nr) of tile row block I into LDS: 3 doubles per row, the point
// (zero past d and in the padding), and behind the B rows' points bit r of the row mask: inside
// / padding.  r0 and nr are multiples of 32 (a unit is at least a 16th of a tile), so a wave's
// rows fill whole mask words: 64 rows two of them, the 32 rows of a 16th one.
__device__ __forceinline__ bool gen_row_inside(const double *xrow, int r) {
  const unsigned *mask = reinterpret_cast<const unsigned *>(xrow + kSymGenMaxD * B);
  return ((mask[r >> 5] >> (r & 31)) & 1u) != 0u;
}
__device__ __forceinline__ void gen_stage_rows(const SymGen &gs, int I, int r0, int nr,
                                               double *__restrict__ xrow) {
  unsigned *mask = reinterpret_cast<unsigned *>(xrow + kSymGenMaxD * B);
  for (int i = threadIdx.x; i < nr; i += 256) {
    int64_t g;
    const bool ok = gen_index(gs, (int64_t)I * B + r0 + i, g);
#pragma unroll
    for (int t = 0; t < kSymGenMaxD; ++t)
      xrow[kSymGenMaxD * (r0 + i) + t] = (ok && t < gs.d) ? gs.Xs[g * gs.d + t] : 0.0;
    const unsigned long long m = __ballot(ok);
    if ((threadIdx.x & 63) == 0) {
      mask[(r0 + i) >> 5] = (unsigned)m;
      if (nr - i > 32) mask[((r0 + i) >> 5) + 1] = (unsigned)(m >> 32);
    }
  }
}
// every position of block Jb inside [0, N) (positions are valid up to a first padded one)
__device__ __forceinline__ bool gen_block_full(const SymGen &gs, int Jb) {
  int64_t g;
  const int64_t p0 = (int64_t)Jb * B, p1 = p0 + B - 1;
  return p0 / gs.blk == p1 / gs.blk && gen_index(gs, p0, g) && gen_index(gs, p1, g);
}
// row r (tile-local) of a generated tile: the 8 entries of the lane's columns, the bits
// k_sym_gen_rbf stores (rbf_of_sqdist_lean: exp's bits, common.h).  PLAIN: an off-diagonal tile
// without padding, which nearly every tile is -- no select and no compare in the row.  CLAMP:
// the entry's form (rbf_of_sqdist_lean); false only in plain tiles of an operator whose points
// keep every squared distance in that form's domain (SymGen::noclamp) -- a padding row is the
// zero point, which need not lie inside the points' box, so the other kinds keep the clamp
template <bool PLAIN, bool DIAG, bool CLAMP>
__device__ __forceinline__ void gen_row(const SymGen &gs, const GenCols &gc,
                                        const double *__restrict__ xrow, int r, int lane,
                                        d2 (&ar)[4]) {
  static_assert(!(PLAIN && DIAG), "a diagonal tile is not plain");
  static_assert(PLAIN || CLAMP, "only a plain tile may drop the clamp");
  const double *xr = xrow + kSymGenMaxD * r;
  double x[kSymGenMaxD];
#pragma unroll
  for (int t = 0; t < kSymGenMaxD; ++t) x[t] = xr[t];
  double v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    double s = 0.0;
#pragma unroll
    for (int t = 0; t < kSymGenMaxD; ++t) s = rbf_sqdist_step(s, __dsub_rn(gc.x[j][t], x[t]), t == 0);
    v[j] = rbf_of_sqdist_lean<CLAMP>(s);
  }
  if constexpr (!PLAIN) {
    const bool rv = gen_row_inside(xrow, r);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = 2 * (lane + 64 * (j >> 1)) + (j & 1);
      if (DIAG && c == r) v[j] = 1.0 + gs.jitter;
      if (!(rv && ((gc.valid >> j) & 1u))) v[j] = 0.0;
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) ar[q] = d2{v[2 * q], v[2 * q + 1]};
}

// ---- the tile body: what both schedules (k_symv_tiles, k_symv_dyn) and both roles do with a
// unit, written once so that they all store the same bits ----

// RB rows [rbase, rbase + RB) of the stored tile A, the lane's 4 double2 columns of each.  RB:
// the rows a wave holds in registers at once, 8 (a whole batch) or 4 (a half batch: 64 VGPRs
// less, the third workgroup of a CU, k_symv_dyn)
template <int RB>
__device__ __forceinline__ void tile_load_batch(const double *A, int64_t rbase, int lane,
                                                d2 (&a)[RB][4]) {
  const d2 *rowp = reinterpret_cast<const d2 *>(A + rbase * B) + lane;
#pragma unroll
  for (int rr = 0; rr < RB; ++rr)
#pragma unroll
    for (int q = 0; q < 4; ++q) a[rr][q] = __builtin_nontemporal_load(rowp + rr * (B / 2) + 64 * q);
}

// One batch of 8 rows against the operand columns pc: the rows' partials summed over the 64
// lanes into rows[] (wave-private LDS transpose: lane 8 r + c adds lanes 8c .. 8c + 7 of row
// r, then xor over c), the lane's column partials into acc (off the diagonal).  GEN: the
// entries are evaluated from the points row by row instead of taken from the loaded batch a.
// The tile's kind is uniform over a unit.  The generating role is instantiated per kind (PLAIN,
// DIAG: gen_row); the streaming role keeps `diag` as a run-time value -- one copy of its 8-row
// batch loop per kind would cost it 140 VGPRs, i.e. the second workgroup of the CU.
// RB (streaming): the rows held at once.  RB = 4 takes the batch as two half batches, the
// second loaded (from A) when the first has been used; each row's s0 / s1 chain, its place in
// the transpose and the row order of acc are those of RB = 8, so the sums are the same bits.
template <bool GEN, bool PLAIN, bool DIAG, int RB, bool CLAMP = true>
__device__ __forceinline__ void tile_batch(d2 (&a)[GEN ? 1 : RB][4], const double *A,
                                           const SymGen &gs,
                                           const GenCols &gc, const double *xrow,
                                           bool diag_rt, const d2 (&pc)[4],
                                           const double *vrow, int rbase, int lane,
                                           double *red, double *rows,
                                           d2 (&acc)[4]) {
  const bool diag = GEN ? DIAG : diag_rt;
#pragma unroll(GEN ? 2 : kRB)
  for (int rr = 0; rr < kRB; ++rr) {
    d2 ar[4];
    if constexpr (GEN) {
      gen_row<PLAIN, DIAG, CLAMP>(gs, gc, xrow, rbase + rr, lane, ar);
    } else {
      if constexpr (RB < kRB)
        if (rr == RB) tile_load_batch<RB>(A, rbase + RB, lane, a);
#pragma unroll
      for (int q = 0; q < 4; ++q) ar[q] = a[rr % RB][q];
    }
    double s0 = ar[0].x * pc[0].x;
    double s1 = ar[0].y * pc[0].y;
#pragma unroll
    for (int q = 1; q < 4; ++q) {
      s0 = fma(ar[q].x, pc[q].x, s0);
      s1 = fma(ar[q].y, pc[q].y, s1);
    }
    red[rr * 64 + lane] = s0 + s1;
    if (!diag) {
      const double pr = vrow[rbase + rr];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        acc[q].x = fma(ar[q].x, pr, acc[q].x);
        acc[q].y = fma(ar[q].y, pr, acc[q].y);
      }
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const d2 *rp = reinterpret_cast<const d2 *>(red + (lane >> 3) * 64 + (lane & 7) * 8);
  const d2 t0 = rp[0], t1 = rp[1], t2 = rp[2], t3 = rp[3];
  double tt = ((t0.x + t0.y) + (t1.x + t1.y)) + ((t2.x + t2.y) + (t3.x + t3.y));
  tt += __shfl_xor(tt, 1, 64);
  tt += __shfl_xor(tt, 2, 64);
  tt += __shfl_xor(tt, 4, 64);
  if ((lane & 7) == 0) rows[rbase + (lane >> 3)] = tt;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The wave's batches gb0 + w, gb0 + w + 4, ... of a unit (the first one's entries are already
// loaded when streaming), and the one uniform branch per unit that picks the generated tile's
// kind and, for a plain tile, the entry's form (gs.noclamp: without the clamp; the clamped plain
// loop stays an instantiation of its own, so an operator that needs the clamp pays no select)
template <bool GEN, bool PLAIN, bool DIAG, int RB, bool CLAMP = true>
__device__ __forceinline__ void tile_batches(d2 (&a)[GEN ? 1 : RB][4], const double *A,
                                             const SymGen &gs, const GenCols &gc, const double *xrow,
                                             bool diag_rt, const d2 (&pc)[4], const double *vrow,
                                             int gb0, int gb1, int w, int lane, double *red,
                                             double *rows, d2 (&acc)[4]) {
#pragma unroll 1
  for (int g = gb0 + w; g < gb1; g += 4) {
    if constexpr (!GEN)
      if (g != gb0 + w) tile_load_batch<RB>(A, g * kRB, lane, a);
    tile_batch<GEN, PLAIN, DIAG, RB, CLAMP>(a, A, gs, gc, xrow, diag_rt, pc, vrow, g * kRB, lane, red,
                                            rows, acc);
  }
}
template <bool GEN, int RB>
__device__ __forceinline__ void tile_unit(d2 (&a)[GEN ? 1 : RB][4], const double *A,
                                          const SymGen &gs, const GenCols &gc, const double *xrow,
                                          bool plain, bool diag, const d2 (&pc)[4],
                                          const double *vrow, int gb0, int gb1, int w, int lane,
                                          double *red, double *rows, d2 (&acc)[4]) {
  if (GEN && plain && gs.noclamp != 0)
    tile_batches<GEN, GEN, false, RB, !GEN>(a, A, gs, gc, xrow, diag, pc, vrow, gb0, gb1, w, lane, red, rows, acc);
  else if (GEN && plain)
    tile_batches<GEN, GEN, false, RB>(a, A, gs, gc, xrow, diag, pc, vrow, gb0, gb1, w, lane, red, rows, acc);
  else if (GEN && diag)
    tile_batches<GEN, false, GEN, RB>(a, A, gs, gc, xrow, diag, pc, vrow, gb0, gb1, w, lane, red, rows, acc);
  else
    tile_batches<GEN, false, false, RB>(a, A, gs, gc, xrow, diag, pc, vrow, gb0, gb1, w, lane, red, rows, acc);
}

// The wave's column partials of a unit into LDS for the 4-wave combine of tile_store_slots
__device__ __forceinline__ void tile_stage_cols(const d2 (&acc)[4], double *cs, int w, int lane) {
  d2 *cs2 = reinterpret_cast<d2 *>(cs);
#pragma unroll
  for (int q = 0; q < 4; ++q) cs2[w * (B / 2) + lane + 64 * q] = acc[q];
}

// The unit's slot stores: row partials to slot J of rows I B + .., the 4 waves' column partials
// combined to slot I of rows J B + .. (plane P for sub-unit 0, else Pq plane h - 1).
// Non-temporal: interleaved with the tile stream they cost ~4 % of the kernel as ordinary
// stores (scripts/probe_symv.hip)
__device__ __forceinline__ void tile_store_slots(double *P, double *Pq,
                                                 int64_t Np, int nb, int2 t, int h, int gb0, int gb1,
                                                 bool diag, const double *sh) {
  const double *rows = sh + B, *cs = sh + 2 * B;
  const int row0 = gb0 * kRB, nr = (gb1 - gb0) * kRB;
  double *Prow = P + (int64_t)t.y * Np + (int64_t)t.x * B + row0;
  for (int c = threadIdx.x; c < nr; c += 256) __builtin_nontemporal_store(rows[row0 + c], Prow + c);
  if (!diag) {
    double *Pc = h == 0 ? P : Pq + (int64_t)(h - 1) * nb * Np;
    double *Pcol = Pc + (int64_t)t.x * Np + (int64_t)t.y * B;
    for (int c = threadIdx.x; c < B; c += 256)
      __builtin_nontemporal_store((cs[c] + cs[B + c]) + (cs[2 * B + c] + cs[3 * B + c]), Pcol + c);
  }
}

// MLFF_SYM_SCHED=static: one workgroup per unit, the tile body once
__global__ __launch_bounds__(256) void k_symv_tiles(const double *__restrict__ tiles,
                                                    const int2 *__restrict__ list,
                                                    const double *__restrict__ v,
                                                    double *__restrict__ P,
                                                    double *__restrict__ Pq, int64_t Np,
                                                    int nwhole, int nb, int lsub,
                                                    const int *__restrict__ status) {
  if (status != nullptr && *status != ST_RUNNING) return;
  __shared__ double sh[kTileLds];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int tile, h, gb0, gb1;
  decode_unit(blockIdx.x, nwhole, lsub, tile, h, gb0, gb1);
  const int2 t = list[tile];
  const double *A = tiles + (int64_t)tile * B * B;
  d2 pc[4], a[kRB][4];
#pragma unroll
  for (int q = 0; q < 4; ++q)
    pc[q] = *reinterpret_cast<const d2 *>(v + (int64_t)t.y * B + 2 * (lane + 64 * q));
  tile_load_batch<kRB>(A, (int64_t)(gb0 + w) * kRB, lane, a);
  for (int i = gb0 * kRB + threadIdx.x; i < gb1 * kRB; i += 256) sh[i] = v[(int64_t)t.x * B + i];
  __syncthreads();
  const bool diag = t.x == t.y;
  const GenCols none{};
  d2 acc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) acc[q] = d2{0.0, 0.0};
  tile_unit<false, kRB>(a, A, SymGen{}, none, nullptr, false, diag, pc, sh, gb0, gb1, w, lane,
                   sh + kTileRed + w * kRB * 64, sh + B, acc);
  if (!diag) tile_stage_cols(acc, sh + 2 * B, w, lane);
  __syncthreads();
  tile_store_slots(P, Pq, Np, nb, t, h, gb0, gb1, diag, sh);
}

// what a k_symv_dyn workgroup needs besides its role
struct SymvArgs {
  const double *tiles;
  const int2 *list;
  const double *v;
  double *P, *Pq;
  int64_t Np;
  int nwhole;
  long long nunits;
  int nb, lsub;
  PGather pg;
  double beta;
};

// Dynamic persistent schedule with cross-tile prefetch: C resident workgroups take work
// units (whole tiles, then the quarter units of the tail) from a ticket counter; before
// finishing a tile (LDS combine + slot stores) a workgroup already has the first batch
// of its next unit and the next p segment in flight, so the HBM stream of a workgroup
// slot does not stop at tile boundaries.  The counter is reset by the slot reduction.
//
// The units of one workgroup, first unit u.  Both roles run the tile body above; they differ
// in where a unit's entries come from (GEN: the points, else the stream 8 rows ahead).
// (The operand reads -- pc before a unit, vrow after the previous one's stores -- stay spelled
// out at their two places each: as helpers they are scheduled differently, 2 VGPRs more.)
template <bool GEN, int RB>
__device__ __forceinline__ long long symv_units(const SymvArgs &k, const SymGen &gs, long long u,
                                                UnitQueue q, double *__restrict__ sh,
                                                long long *s_next) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double *vrow = sh, *rows = sh + B, *cs = sh + 2 * B;
  double *red = sh + kTileRed + w * kRB * 64;
  double *xrow = sh + kTileLds;  // GEN: the unit's row points
  const PGather &pg = k.pg;
  const double *v = k.v;
  const double beta = k.beta;
  long long units_done = 0;
  int tile, h, gb0, gb1;
  decode_unit(u, k.nwhole, k.lsub, tile, h, gb0, gb1);
  int2 t = k.list[tile];
  const double *A = k.tiles + (int64_t)tile * B * B;
  d2 pc[4], a[GEN ? 1 : RB][4];
  GenCols gc;
#pragma unroll
  for (int q = 0; q < 4; ++q) pc[q] = pg_val2(pg, v, (int64_t)t.y * B + 2 * (lane + 64 * q), beta);
  if constexpr (!GEN) tile_load_batch<RB>(A, (int64_t)(gb0 + w) * kRB, lane, a);
  if (threadIdx.x == 0) *s_next = next_unit(q, k.nunits);
  for (int i = threadIdx.x; i < (gb1 - gb0) * kRB; i += 256) {
    const int64_t gi = (int64_t)t.x * B + gb0 * kRB + i;
    vrow[gb0 * kRB + i] = pg.gb != nullptr ? pg_val(pg, v, gi, beta) : v[gi];
  }
  if (GEN) {
    gen_stage_rows(gs, t.x, gb0 * kRB, (gb1 - gb0) * kRB, xrow);
    gen_load_cols(gs, t.y, lane, gc);
  }
  __syncthreads();
  while (true) {
    const bool diag = t.x == t.y;
    const bool plain = GEN && !diag && gen_block_full(gs, t.x) && gen_block_full(gs, t.y);
    d2 acc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = d2{0.0, 0.0};
    tile_unit<GEN, RB>(a, A, gs, gc, xrow, plain, diag, pc, vrow, gb0, gb1, w, lane, red, rows, acc);
    if (!diag) tile_stage_cols(acc, cs, w, lane);
    __syncthreads();  // rows / cs complete; s_next visible
    const long long un = *s_next;
    int tile2 = 0, h2 = 0, gb02 = 0, gb12 = 0;
    int2 t2 = t;
    const double *A2 = A;
    if (un < k.nunits) {  // next unit: p segment and first batch in flight during the stores
      decode_unit(un, k.nwhole, k.lsub, tile2, h2, gb02, gb12);
      t2 = k.list[tile2];
      A2 = k.tiles + (int64_t)tile2 * B * B;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        pc[q] = pg_val2(pg, v, (int64_t)t2.y * B + 2 * (lane + 64 * q), beta);
      if constexpr (GEN)
        gen_load_cols(gs, t2.y, lane, gc);
      else
        tile_load_batch<RB>(A2, (int64_t)(gb02 + w) * kRB, lane, a);
    }
    tile_store_slots(k.P, k.Pq, k.Np, k.nb, t, h, gb0, gb1, diag, sh);
    __syncthreads();  // LDS consumed, s_next read by everyone
    ++units_done;
    if (un >= k.nunits) break;
    if (threadIdx.x == 0) *s_next = next_unit(q, k.nunits);
    tile = tile2;
    h = h2;
    gb0 = gb02;
    gb1 = gb12;
    t = t2;
    A = A2;
    for (int i = threadIdx.x; i < (gb1 - gb0) * kRB; i += 256) {
      const int64_t gi = (int64_t)t.x * B + gb0 * kRB + i;
      vrow[gb0 * kRB + i] = pg.gb != nullptr ? pg_val(pg, v, gi, beta) : v[gi];
    }
    if (GEN) gen_stage_rows(gs, t.x, gb0 * kRB, (gb1 - gb0) * kRB, xrow);
    __syncthreads();
  }
  return units_done;
}

// The CU a workgroup runs on as an index below kSymCuWords: the XCC id and HW_ID bits [15:8]
// (gfx9: CU_ID [11:8], SH_ID [12], SE_ID from bit 13)
__device__ __forceinline__ unsigned cu_key() {
  unsigned xcc = 0, hw = 0;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
  return ((xcc & 0xfu) << 8) | ((hw >> 8) & 0xffu);
}

// MLFF_SYM_TRACE record of a workgroup: start, end, units taken, 1 | role << 1 | CU key << 2
constexpr int kTraceWords = 4;
// ... and, behind the records of all workgroups, the shader clock (clock64) at its start and end
// stamps: the clock the launch ran at is their difference over that of the wall stamps.  Role
// kernels only, and a region of its own, so that k_symv_dyn<false> stays as it is
constexpr int kTraceClockWords = 2;

// ROLES false: every workgroup streams, one counter over all units (sp.gen off: matrices set
// by the host, MLFF_SYM_GEN=0, d above kSymGenMaxD); the first unit is blockIdx.x, without an
// atomic.  ROLES true (tiles generated from the RBF points): a streaming workgroup reads the
// stored whole tiles [0, gs.n_s), a generating one evaluates the whole tiles [gs.n_s, nwhole)
// from the points; the quarter units are a third range, either role's (gs.qmode 0), the
// streaming (1) or the generating role's (2).  The role comes from the order of arrival on the
// CU (gs.roles), so the dispatcher's placement cannot put two of a kind on one CU and none on
// another; it is therefore not known at launch how many workgroups hold a role, and every unit,
// the first included, comes from a counter.  A workgroup done with its role's ranges goes on
// with the other role's, in its own manner (the bits are the same, tile_batch<GEN>).
// RB: the rows the streaming role holds at once (tile_load_batch).  8: 220 VGPRs, two workgroups
// on a CU, one of each role.  4 (ROLES only): at most 168 VGPRs and a third of the CU's LDS,
// three workgroups on a CU, one streaming and two generating (gs.wgs).
template <bool ROLES, int RB = kRB>
__global__ __launch_bounds__(256, RB < kRB ? 3 : 1) void k_symv_dyn(const double *__restrict__ tiles,
                                                  const int2 *__restrict__ list,
                                                  const double *__restrict__ v,
                                                  double *__restrict__ P,
                                                  double *__restrict__ Pq, int64_t Np,
                                                  int nwhole, long long nunits, int nb,
                                                  int lsub,
                                                  unsigned long long *__restrict__ ticket,
                                                  const int *__restrict__ status, PGather pg,
                                                  SymGen gs,
                                                  unsigned long long *wgtrace = nullptr) {
  if (status != nullptr && *status != ST_RUNNING) return;
  // MLFF_SYM_TRACE (diagnostic): per workgroup its start, end, units taken, role and CU
  unsigned long long *tr = wgtrace != nullptr ? wgtrace + kTraceWords * blockIdx.x : nullptr;
  unsigned long long *trc = nullptr;
  if constexpr (ROLES)
    if (tr != nullptr) trc = wgtrace + kTraceWords * gridDim.x + kTraceClockWords * blockIdx.x;
  if (tr != nullptr && threadIdx.x == 0) tr[0] = wall_clock64();
  if (trc != nullptr && threadIdx.x == 0) trc[0] = clock64();
  __shared__ double sh[kTileLds + (ROLES ? kGenRowLds : 0)];
  __shared__ long long s_next;
  __shared__ int s_role;
  if (!ROLES && (long long)blockIdx.x >= nunits) return;
  if (ROLES && threadIdx.x == 0) {
    int r = gs.roles == kSymRolesGen ? 1 : 0;
    // of every gs.wgs workgroups (by index, or as they arrive on the CU) the first one streams.
    // The arrival words are never reset, and a launch that ended early leaves them out of
    // phase: that moves roles between workgroups, never a result
    const unsigned wgs = (unsigned)gs.wgs;
    if (gs.roles == kSymRolesIndex) r = blockIdx.x % wgs != 0u;
    if (gs.roles == kSymRolesCu) r = atomicAdd(ticket + kTicketWords + cu_key(), 1ull) % wgs != 0ull;
    s_role = r;
  }
  if (!ROLES && tr != nullptr && threadIdx.x == 0) tr[3] = 1ull | (unsigned long long)cu_key() << 2;
  const double beta = pg.gb != nullptr ? fused_p_beta(pg, gathered_rho(pg, sh), &pg.st->rho_new) : 0.0;
  UnitQueue q{ticket, ticket, ticket, (long long)gridDim.x, nunits, 0, 0, 0, 0, 0};
  long long u = blockIdx.x;
  bool gen = false;
  if (ROLES) {
    __syncthreads();
    gen = __builtin_amdgcn_readfirstlane(s_role) != 0;
    // own whole tiles, then the other role's whole tiles and the quarter units: the quarters
    // last where they are the other role's (qmode), else in the order of gs.pool_first
    const bool pool_first = gs.pool_first != 0 && gs.qmode != (gen ? 1 : 2);
    unsigned long long *cs = ticket, *cg = ticket + 2, *cq = ticket + 3;
    const long long ns = gs.n_s;
    q.c0 = gen ? cg : cs;
    q.base0 = gen ? ns : 0;
    q.hi0 = gen ? nwhole : ns;
    unsigned long long *co = gen ? cs : cg;
    const long long olo = gen ? 0 : ns, ohi = gen ? ns : nwhole;
    q.c1 = pool_first ? cq : co;
    q.base1 = pool_first ? nwhole : olo;
    q.hi1 = pool_first ? nunits : ohi;
    q.c2 = pool_first ? co : cq;
    q.base2 = pool_first ? olo : nwhole;
    q.hi2 = pool_first ? ohi : nunits;
    if (threadIdx.x == 0) {
      s_next = next_unit(q, nunits);
      if (tr != nullptr) tr[3] = 1ull | (gen ? 2ull : 0ull) | (unsigned long long)cu_key() << 2;
    }
    __syncthreads();
    u = s_next;
    __syncthreads();
    if (u >= nunits) {
      if (tr != nullptr && threadIdx.x == 0) tr[1] = wall_clock64();
      if (trc != nullptr && threadIdx.x == 0) trc[1] = clock64();
      return;
    }
  }
  const SymvArgs k{tiles, list, v, P, Pq, Np, nwhole, nunits, nb, lsub, pg, beta};
  long long units_done;
  if constexpr (ROLES) {
    if (gen)
      units_done = symv_units<true, RB>(k, gs, u, q, sh, &s_next);
    else
      units_done = symv_units<false, RB>(k, gs, u, q, sh, &s_next);
  } else {
    units_done = symv_units<false, RB>(k, gs, u, q, sh, &s_next);
  }
  if (tr != nullptr && threadIdx.x == 0) {
    tr[1] = wall_clock64();
    tr[2] = (unsigned long long)units_done;
    if (trc != nullptr) trc[1] = clock64();
  }
}

// one rank: y[i] = the sum of the nb slots of row i in slot order, a split slot as
// ((P + Pq0) + Pq1) + ...; EPI: y = sigma y + lam vloc for rows < n_out; PQ (with EPI): also the
// p.q partial sum (vloc = p) of each workgroup -> pq_part (grid = kVecGrid workgroups,
// grid-stride over the rows)
template <bool EPI, bool PQ>
__global__ __launch_bounds__(256) void k_sym_reduce(const double *__restrict__ P,
                                                    const double *__restrict__ Pq,
                                                    const unsigned char *__restrict__ split,
                                                    int t_split, int64_t Np, int nb, int nq,
                                                    int64_t n_out, double *__restrict__ y,
                                                    double sigma, double lam,
                                                    const double *__restrict__ vloc,
                                                    double *__restrict__ pq_part,
                                                    unsigned long long *__restrict__ ticket,
                                                    const int *__restrict__ status,
                                                    PGather pg = PGather{},
                                                    double *pw = nullptr) {
  if (status != nullptr && *status != ST_RUNNING) return;
  if (blockIdx.x == 0 && threadIdx.x == 0) reset_work_counters(ticket);
  double apq = 0.0;
  // fused p update (PGather): p = fma(beta, p_old, z) written here and used as the epilogue's v
  // -- k_update_p's bits
  const double beta = PQ && pg.gb != nullptr ? fused_p_beta(pg, pg.st->rho_new, &pg.st->rho) : 0.0;
  const int64_t pl = (int64_t)nb * Np;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_out;
       i += (int64_t)gridDim.x * 256) {
    const int bi = (int)(i / B);
    double s = 0.0;
    // slots below t_split hold no split tile for this row block (t_split: the smallest
    // row-block index of a split tile, nb if none).  8 slot loads in flight per
    // thread; the additions stay in slot order
    const int tend = t_split > bi ? t_split : bi + 1;
    const int t8 = tend < nb ? tend : nb;
    // (16 in flight: at one row per thread the 512-workgroup PQ grid leaves 1 wave per SIMD,
    // so the slot loads' round trips are the kernel's time)
    int t = 0;
    for (; t + 15 < t8; t += 16) {
      double v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) v[u] = __builtin_nontemporal_load(P + (int64_t)(t + u) * Np + i);
#pragma unroll
      for (int u = 0; u < 16; ++u) s += v[u];
    }
    for (; t + 7 < t8; t += 8) {
      double v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = __builtin_nontemporal_load(P + (int64_t)(t + u) * Np + i);
#pragma unroll
      for (int u = 0; u < 8; ++u) s += v[u];
    }
    // the remaining slots (split tiles among them) in batches of 8 as well; every slot
    // value is ((P + Pq0) + Pq1) + ... + Pq_{nq-1}, added in slot order
    for (; t < nb; t += 8) {
      double v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        v[u] = 0.0;
        const int tu = t + u;
        if (tu < nb) {
          v[u] = P[(int64_t)tu * Np + i];
          if (tu > bi && split[(int64_t)tu * nb + bi])
            for (int hq = 0; hq < nq; ++hq) v[u] += Pq[hq * pl + (int64_t)tu * Np + i];
        }
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (t + u < nb) s += v[u];
    }
    if (EPI) {
      double pv = 0.0;
      if (PQ && pg.gb != nullptr) {  // (vloc is p itself: read through pw only)
        pv = pg_val(pg, pw, i, beta);
        pw[i] = pv;
      } else if (vloc != nullptr) {
        pv = vloc[i];
      }
      double yv = sigma * s;
      if (vloc != nullptr) yv += lam * pv;
      y[i] = yv;
      if (PQ) apq = fma(pv, yv, apq);
    } else {
      y[i] = s;
    }
  }
  if (PQ) {
    __shared__ double sh[4];
    apq = block_sum256(apq, sh);
    if (threadIdx.x == 0) pq_part[blockIdx.x] = apq;
  }
}

// ---- p.q of the sharded iteration: every rank publishes its share, sigma p.y_g + lam
// ||p_loc||^2, from the (apq, app) partial pairs of its reduction's workgroups ----
struct PqPublish {
  double sigma = 0.0, lam = 0.0;
  int world = 0;  // 0: the separate k_pq_publish launch follows (MLFF_PQ_PUBLISH=1)
  bool ordered = true;  // the arrival's form (pq_put), k_sym_reduce_wl only
};

// How a workgroup's pair travels to the workgroup that arrives last (pq_arrive):
//  ORDERED   plain stores, an agent-scope release before the ticket add, an agent-scope acquire
//            in the last workgroup, plain loads: the pairs' stores happen before their loads
//            under the HIP memory model (the adds on the one word form a release sequence).
//  !ORDERED  relaxed agent-scope atomic stores (write-through, sc1) drained with s_waitcnt
//            vmcnt(0) before a relaxed add, relaxed agent-scope atomic loads (sc1, past the L1)
//            in the last workgroup.  Nothing synchronises in the language's model; on gfx950 it
//            is the counter form of cdna_hip_programming.md Guideline 16 (R1: every payload
//            store sc1 and drained by the storing wave before the add; every load of it sc1)
//            and the first row of the sc1 hand-off table in MI355X_MICROARCH.md, "inter-
//            workgroup visibility" (one lane of each workgroup signals for its own stores by
//            an agent-scope add on one counter, the last adder's workgroup loads behind a
//            barrier; measured there at one workgroup per CU, this grid puts two on a CU).
//            Observed behaviour of gfx950, not an architectural guarantee.  It spares
//            every workgroup the release's L2 write-back: one rank of 8 at N = 65536, rank 0 /
//            rank 3, 0.3528 / 0.3490 ms per iteration against 0.3583 / 0.3621 ms ORDERED
//            (medians of three interleaved pairs, profiles/symrefactor/ab/summary.txt).
//            k_sym_reduce_wl's default; MLFF_SYM_PQ_ORDERED=1 at the operator's build selects
//            ORDERED there.  k_sym_reduce_w is always ORDERED.
template <bool ORDERED>
__device__ __forceinline__ void pq_put(double *p, double v) {
  if (ORDERED)
    *p = v;
  else
    __hip_atomic_store(reinterpret_cast<unsigned long long *>(p), __builtin_bit_cast(unsigned long long, v),
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <bool ORDERED>
__device__ __forceinline__ double pq_get(const double *p) {
  if (ORDERED) return *p;
  return __builtin_bit_cast(double, __hip_atomic_load(reinterpret_cast<const unsigned long long *>(p),
                                                      __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

// s_rank = sigma * sum(pq_part) + lam * sum(pp_part) (one workgroup; fixed order: thread f adds
// partials f, f + 256, ..., then block_sum256_pair), put into tail slot `rank` of every rank
// block of the reduce-scatter operand; the other tail slots stay zero, so the reduce-scatter
// hands every rank the exact vector of shares (x + 0 is exact in any order) and each rank sums
// it in rank order: p.q is bitwise identical on all ranks without a separate allreduce.
template <bool ORDERED = true>
__device__ __forceinline__ void pq_publish_share(const double *pq_part, const double *pp_part, int np,
                                                 double sigma, double lam, int rank, int world,
                                                 int64_t blk, int64_t bstride, double *yg, double *sh) {
  double a = 0.0, b = 0.0;
  for (int i = threadIdx.x; i < np; i += 256) {
    a += pq_get<ORDERED>(pq_part + i);
    b += pq_get<ORDERED>(pp_part + i);
  }
  block_sum256_pair(a, b, sh);
  const double share = sigma * a + lam * b;
  for (int g = threadIdx.x; g < world; g += 256) yg[(int64_t)g * bstride + blk + rank] = share;
}

// Arrival of a workgroup whose pair (a, b) thread 0 holds: the pair is stored, then the
// workgroup takes a ticket (ticket[1]).  True in every thread of the workgroup that arrived
// last, which resets the ticket for the next launch and may read every pair (pq_get).
template <bool ORDERED>
__device__ __forceinline__ bool pq_arrive(double a, double b, double *pq_part, double *pp_part,
                                          unsigned long long *ticket, int *s_last) {
  if (threadIdx.x == 0) {
    pq_put<ORDERED>(pq_part + blockIdx.x, a);
    pq_put<ORDERED>(pp_part + blockIdx.x, b);
    if (ORDERED)
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    else
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const bool last = __hip_atomic_fetch_add(ticket + 1, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ==
                      (unsigned long long)(gridDim.x - 1);
    if (last) __hip_atomic_store(ticket + 1, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *s_last = last;
  }
  __syncthreads();
  if (!*s_last) return false;
  // !ORDERED: no instruction, it only keeps the compiler from moving the loads above the ticket
  if (ORDERED)
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  else
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  return true;
}

// The end of a rank reduction's workgroup: its pair summed over the workgroup and stored; with
// the folded publish the last workgroup to arrive also does k_pq_publish's work -- the same
// sums in the same order, so the same share bits -- one launch less per sharded iteration (the
// publish was a 4.9 us single-workgroup launch at W = 8).  sh: 8 doubles.
template <bool ORDERED>
__device__ __forceinline__ void pq_tail(double apq, double app, double *pq_part, double *pp_part,
                                        unsigned long long *ticket, const PqPublish &pub, int rank,
                                        int64_t blk, int64_t bstride, double *yg, double *sh,
                                        int *s_last) {
  block_sum256_pair(apq, app, sh);
  if (pub.world == 0) {
    if (threadIdx.x == 0) {
      pq_part[blockIdx.x] = apq;
      pp_part[blockIdx.x] = app;
    }
    return;
  }
  if (!pq_arrive<ORDERED>(apq, app, pq_part, pp_part, ticket, s_last)) return;
  pq_publish_share<ORDERED>(pq_part, pp_part, (int)gridDim.x, pub.sigma, pub.lam, rank, pub.world, blk,
                            bstride, yg, sh);
}

// several ranks: y_g = sum over this rank's slots for every row of [0, ld), written
// into rank blocks of stride `bstride` (= blk + tail: the reduce-scatter operand).
// PQ: also the partial p.y_g (all rows) + (lam/sigma-free) ||p_loc||^2 partials, one
// pair per workgroup (pq_tail).
template <bool PQ>
__global__ __launch_bounds__(256) void k_sym_reduce_w(const double *__restrict__ P,
                                                      const double *__restrict__ Pq,
                                                      const unsigned char *__restrict__ split,
                                                      int64_t Np, int nq,
                                                      int nb, int rank,
                                                      const int *__restrict__ own,
                                                      int64_t ld, int64_t blk, int64_t bstride,
                                                      double *__restrict__ yg,
                                                      double *p,  // read, and written when fused
                                                      double *__restrict__ pq_part,
                                                      double *__restrict__ pp_part,
                                                      unsigned long long *__restrict__ ticket,
                                                      const int *__restrict__ status,
                                                      PGather pg, PqPublish pub) {
  if (status != nullptr && *status != ST_RUNNING) return;
  if (blockIdx.x == 0 && threadIdx.x == 0) reset_work_counters(ticket);
  __shared__ double sh[8];
  __shared__ int s_last;
  double apq = 0.0, app = 0.0;
  // fused p update: p written here (every tile has read p_old)
  const double beta = PQ && pg.gb != nullptr ? fused_p_beta(pg, pg.st->rho_new, &pg.st->rho) : 0.0;
  const int64_t lo = (int64_t)rank * blk, hi = lo + blk;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < ld;
       i += (int64_t)gridDim.x * 256) {
    // a wave's 64 rows lie in one 512-row block: bi, the slot list and its split flags are
    // wave-uniform (scalar loads), so no slot load waits on a flag or index load
    const int bi = __builtin_amdgcn_readfirstlane((int)(i / B));
    double s = 0.0;
    // this rank's slots of row block bi (own: ascending sym_own_entry slots, the flag marks a
    // split tile; built at setup) in batches of 16 whose loads are all in flight before the
    // first addition; every slot value is ((P + Pq0) + Pq1) + ... (nq planes), added in
    // slot order
    const int *ol = own + (int64_t)bi * nb;
    const int cnt = own[(int64_t)nb * nb + bi];
    const int64_t pl = (int64_t)nb * Np;
    for (int c = 0; c < cnt; c += 16) {
      double v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        v[u] = 0.0;
        if (c + u < cnt) {
          const int e = ol[c + u];
          const int64_t at = (int64_t)sym_own_slot(e) * Np + i;
          v[u] = P[at];
          if (sym_own_split(e))
            for (int hq = 0; hq < nq; ++hq) v[u] += Pq[hq * pl + at];
        }
      }
#pragma unroll
      for (int u = 0; u < 16; ++u)
        if (c + u < cnt) s += v[u];
    }
    yg[(i / blk) * bstride + i % blk] = s;
    if (PQ) {
      double pv;
      if (pg.gb != nullptr) {
        pv = pg_val(pg, p, i, beta);
        p[i] = pv;
      } else {
        pv = p[i];
      }
      apq = fma(pv, s, apq);
      if (i >= lo && i < hi) app = fma(pv, pv, app);
    }
  }
  if (PQ) pq_tail<true>(apq, app, pq_part, pp_part, ticket, pub, rank, blk, bstride, yg, sh, &s_last);
}

// k_sym_reduce_w with the slot loads of a row all in flight (round 6): at
// W = 8 a rank's own row blocks hold 72 slots (+ the split tiles' planes) against 8 elsewhere,
// and k_sym_reduce_w took them as 5 dependent batches of 16, each behind a scalar load of its
// slot entries and a wait per split plane -- 25 us of the 0.38 ms per-rank step.  Here the
// workgroup's row block (256 rows lie in one 512-row block) stages its flat load list (every
// slot and, after a split slot, its planes: SymPack::plist) in LDS once, and a row's loads go
// out in batches of kRwBatch with the next batch in flight while the current one is added:
// unconditional loads (entries past the count re-read the last one), the additions in list
// order -- each slot ((P + Pq0) + Pq1) + ..., the slots in ascending order: k_sym_reduce_w's
// sums, the same bits (MLFF_SYM_REDUCE_LIST=0 restores it; test_sym_reduce_list_bitwise)
constexpr int kRwBatch = 32;
constexpr int kRwMaxList = 2048;  // list entries per row block staged in LDS

template <bool PQ>
__global__ __launch_bounds__(256) void k_sym_reduce_wl(const double *__restrict__ P,
                                                       const double *__restrict__ Pq,
                                                       int64_t Np, int nb,
                                                       const int *__restrict__ plist,
                                                       int64_t pstride, int rank,
                                                       int64_t ld, int64_t blk, int64_t bstride,
                                                       double *__restrict__ yg, double *p,
                                                       double *__restrict__ pq_part,
                                                       double *__restrict__ pp_part,
                                                       unsigned long long *__restrict__ ticket,
                                                       const int *__restrict__ status,
                                                       PGather pg, PqPublish pub) {
  if (status != nullptr && *status != ST_RUNNING) return;
  if (blockIdx.x == 0 && threadIdx.x == 0) reset_work_counters(ticket);
  __shared__ double sh[8];
  __shared__ int s_last;
  __shared__ int sl[kRwMaxList];
  double apq = 0.0, app = 0.0;
  // fused p update: p written here (every tile has read p_old)
  const double beta = PQ && pg.gb != nullptr ? fused_p_beta(pg, pg.st->rho_new, &pg.st->rho) : 0.0;
  const int64_t lo = (int64_t)rank * blk, hi = lo + blk;
  const int64_t plane = (int64_t)nb * Np;
  for (int64_t c0 = (int64_t)blockIdx.x * 256; c0 < ld; c0 += (int64_t)gridDim.x * 256) {
    const int64_t i = c0 + threadIdx.x;
    const int bi = (int)(c0 / B);  // the workgroup's 256 rows lie in one row block
    // the list, its count and the p update's operands are requested together (none waits for
    // another): the list's whole stride (entries past the count are zeros, slot 0 of P)
    const int cnt = plist[(int64_t)nb * pstride + bi];
    int le[kRwMaxList / 256];
#pragma unroll
    for (int q = 0; q < kRwMaxList / 256; ++q) {
      const int e = threadIdx.x + 256 * q;
      le[q] = e < pstride ? plist[(int64_t)bi * pstride + e] : 0;
    }
    double pz = 0.0, pold = 0.0;
    if (PQ && i < ld) {
      if (pg.gb != nullptr) {
        pz = pg_z(pg, i);
        if (pg.it > 1) pold = p[i];
      } else {
        pold = p[i];
      }
    }
    __syncthreads();  // the previous chunk's list reads are done
#pragma unroll
    for (int q = 0; q < kRwMaxList / 256; ++q)
      if (threadIdx.x + 256 * q < pstride) sl[threadIdx.x + 256 * q] = le[q];
    __syncthreads();
    // a batch's list entries one per lane (lane & 31), read out with v_readlane: no LDS round
    // trip between a batch's loads
    const int lane32 = (int)(threadIdx.x & 31);
    auto entries = [&](int e0) { return sl[e0 + lane32 < cnt ? e0 + lane32 : cnt - 1]; };
    auto load = [&](int ent, int u) {
      const int x = __builtin_amdgcn_readlane(ent, u);
      const int h = sym_plist_plane(x);
      const double *base = h == 0 ? P : Pq + (int64_t)(h - 1) * plane;
      return base[(int64_t)sym_plist_slot(x) * Np + i];
    };
    double s = 0.0, cur = 0.0;
    if (cnt > 0 && i < ld) {
      double v[kRwBatch];
      int ev = entries(0);
#pragma unroll
      for (int u = 0; u < kRwBatch; ++u) v[u] = load(ev, u);
      for (int e0 = 0; e0 < cnt; e0 += kRwBatch) {
        double w[kRwBatch];
        const int ew = entries(e0 + kRwBatch < cnt ? e0 + kRwBatch : e0);
        if (e0 + kRwBatch < cnt) {  // uniform: the whole next batch in flight
#pragma unroll
          for (int u = 0; u < kRwBatch; ++u) w[u] = load(ew, u);
        } else {
#pragma unroll
          for (int u = 0; u < kRwBatch; ++u) w[u] = 0.0;
        }
#pragma unroll
        for (int u = 0; u < kRwBatch; ++u) {
          if (e0 + u < cnt) {
            if (sym_plist_plane(__builtin_amdgcn_readlane(ev, u))) {
              cur += v[u];  // a split slot's next plane
            } else {
              s += cur;  // the previous slot is complete
              cur = v[u];
            }
          }
        }
#pragma unroll
        for (int u = 0; u < kRwBatch; ++u) v[u] = w[u];
        ev = ew;
      }
    }
    s += cur;
    if (i >= ld) continue;
    yg[(i / blk) * bstride + i % blk] = s;
    if (PQ) {
      double pv;
      if (pg.gb != nullptr) {  // pg_val's arithmetic on the operands loaded above
        pv = pg.it > 1 ? fma(beta, pold, pz) : pz;
        p[i] = pv;
      } else {
        pv = pold;
      }
      apq = fma(pv, s, apq);
      if (i >= lo && i < hi) app = fma(pv, pv, app);
    }
  }
  if (PQ) {
    if (pub.ordered)
      pq_tail<true>(apq, app, pq_part, pp_part, ticket, pub, rank, blk, bstride, yg, sh, &s_last);
    else
      pq_tail<false>(apq, app, pq_part, pp_part, ticket, pub, rank, blk, bstride, yg, sh, &s_last);
  }
}

// MLFF_PQ_PUBLISH=1 (A/B): pq_publish_share as a launch of its own, one workgroup
__global__ __launch_bounds__(256) void k_pq_publish(const double *__restrict__ pq_part,
                                                    const double *__restrict__ pp_part, int np,
                                                    double sigma, double lam, int rank, int world,
                                                    int64_t blk, int64_t bstride,
                                                    double *__restrict__ yg,
                                                    const int *__restrict__ status) {
  if (status != nullptr && *status != ST_RUNNING) return;
  __shared__ double sh[8];
  pq_publish_share(pq_part, pp_part, np, sigma, lam, rank, world, blk, bstride, yg, sh);
}

// y[i] = sigma * src[i] + lam * vloc[i]  (src may alias y)
__global__ __launch_bounds__(256) void k_axpby_loc(const double *__restrict__ src, double *y,
                                                   int64_t n, double sigma, double lam,
                                                   const double *__restrict__ vloc,
                                                   const int *__restrict__ status) {
  if (status != nullptr && *status != ST_RUNNING) return;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double yv = sigma * src[i];
  if (vloc != nullptr) yv += lam * vloc[i];
  y[i] = yv;
}

// Pack (COMPARE = false) or verify symmetry (COMPARE = true) of one stored tile per
// workgroup, 64 x 64 sub-blocks through LDS.  Source rows are this rank's dense
// rows (row stride ld, global row g at local row g - rowbase).  TRANS: the tile is
// read from rows J B + c (symmetric mirror) instead of rows I B + r.
template <bool COMPARE>
__global__ __launch_bounds__(256) void k_sym_pack(const double *__restrict__ K, int64_t ld,
                                                  int64_t rowbase, int64_t nloc, const int2 *__restrict__ list,
                                                  const unsigned char *__restrict__ trans,
                                                  double *__restrict__ tiles,
                                                  int *__restrict__ mismatch) {
  __shared__ double S[64][65];
  const int2 t = list[blockIdx.x];
  const bool tr = trans[blockIdx.x] != 0;
  double *T = tiles + (int64_t)blockIdx.x * B * B;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  int bad = 0;
  for (int sb = 0; sb < (B / 64) * (B / 64); ++sb) {
    const int br = (sb / (B / 64)) * 64, bc = (sb % (B / 64)) * 64;  // sub-block of the tile
    // source sub-block rows / cols
    const int64_t srow = tr ? (int64_t)t.y * B + bc : (int64_t)t.x * B + br;
    const int64_t scol = tr ? (int64_t)t.x * B + br : (int64_t)t.y * B + bc;
    __syncthreads();
    // outside the dense block (rows beyond this rank's, columns beyond ld: the
    // padding of Np = round_up(ld, B) on one rank) the matrix is zero
    for (int a = ty; a < 64; a += 4) {
      const int64_t lr = srow + a - rowbase, c = scol + tx;
      S[a][tx] = (lr >= 0 && lr < nloc && c < ld) ? K[lr * ld + c] : 0.0;
    }
    __syncthreads();
    for (int a = ty; a < 64; a += 4) {
      const double val = tr ? S[tx][a] : S[a][tx];  // tile(br + a, bc + tx)
      double *dst = T + (int64_t)(br + a) * B + bc + tx;
      if (COMPARE) {
        if (*dst != val) bad = 1;
      } else {
        *dst = val;
      }
    }
  }
  if (COMPARE && bad) atomicOr(mismatch, 1);
}

// Generate one stored tile per workgroup directly from the RBF points (no dense rows):
// tile (I, J) element (r, c) = K[pos I B + r, pos J B + c] in the padded rank-block index
// space (zero outside [0, N)); each thread owns 2 columns and walks the 512 rows
// (non-temporal 4-KB row stores)
__global__ __launch_bounds__(256) void k_sym_gen_rbf(const int2 *__restrict__ list,
                                                     const double *__restrict__ Xs, int d,
                                                     double jitter, int64_t N, int64_t rows_per,
                                                     int64_t blk, double *__restrict__ tiles) {
  const int2 t = list[blockIdx.x];
  double *T = tiles + (int64_t)blockIdx.x * B * B;
  double xc[2][8];
  int64_t gc[2];
  bool vc[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int64_t pos = (int64_t)t.y * B + threadIdx.x + 256 * h;
    const int64_t off = pos % blk;
    gc[h] = (pos / blk) * rows_per + off;
    vc[h] = off < rows_per && gc[h] < N;
#pragma unroll
    for (int u = 0; u < 8; ++u) xc[h][u] = (vc[h] && u < d) ? Xs[gc[h] * d + u] : 0.0;
  }
  for (int r = 0; r < B; ++r) {
    const int64_t pos = (int64_t)t.x * B + r;
    const int64_t off = pos % blk;
    const int64_t gr = (pos / blk) * rows_per + off;
    const bool vr = off < rows_per && gr < N;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      double val = 0.0;
      // K[gr, gc] evaluated from the column point (rbf_value(x_gc, gr)): bitwise the same
      // as from the row point, see common.h
      if (vr && vc[h]) val = (gr == gc[h]) ? 1.0 + jitter : rbf_value(xc[h], Xs, gr, d);
      __builtin_nontemporal_store(val, T + (int64_t)r * B + threadIdx.x + 256 * h);
    }
  }
}

// test hook (mlff_test_rbf_exp, mlff_test_rbf_exp_noclamp): the library's exp and one form of the
// generating role's over an array of squared distances
template <bool CLAMP>
__global__ __launch_bounds__(256) void k_rbf_exp_probe(const double *__restrict__ s, int64_t n,
                                                       double *__restrict__ lib_out,
                                                       double *__restrict__ lean_out) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    lib_out[i] = rbf_of_sqdist(s[i]);
    lean_out[i] = rbf_of_sqdist_lean<CLAMP>(s[i]);
  }
}

}  // namespace

void launch_rbf_exp_probe(const double *s, int64_t n, double *lib_out, double *lean_out, bool clamp,
                          hipStream_t st) {
  if (n <= 0) return;
  const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, 4096);
  if (clamp)
    hipLaunchKernelGGL(k_rbf_exp_probe<true>, dim3(grid), dim3(256), 0, st, s, n, lib_out, lean_out);
  else
    hipLaunchKernelGGL(k_rbf_exp_probe<false>, dim3(grid), dim3(256), 0, st, s, n, lib_out, lean_out);
}

// The MLFF_SYM_* environment knobs (all A/B or diagnostic; the defaults are the measured
// choices).  Read at every operator build, so a process may change them between contexts.
struct SymKnobs {
  // MLFF_SYM_WHOLE_ROUNDS=<r>: at most r rounds of whole tiles, the rest split (finer units for
  // the dynamic schedule where a rank holds only ~2 tiles per resident workgroup, W = 8)
  int64_t whole_rounds = -1;
  // Sub-units per split tile: 4 (quarters).  MLFF_SYM_LSUB=3|4 slices the split tiles
  // into 8 / 16 row slices instead (the count that would fill the C slots when the nt mod
  // C tail tiles are few, e.g. 8 of a rank's 1032 at 8 ranks).  Measured on one MI355X
  // (scripts/gpu_sym_lsub_ab.sh, profiles/r02/final3e): no gain -- the dynamic schedule
  // already overlaps the tail (k_symv_dyn 323.9 vs 323.6 us at W = 8) while the reduce
  // reads 15 instead of 3 planes of the split slots (12.7 -> 17.9 us): the step got 1 %
  // slower at W = 8 / 4, 0.2 % at W = 1.  Kept selectable, not default.
  int lsub = 2;
  // launch schedule: k_symv_dyn (C resident workgroups taking units from a counter, next
  // unit prefetched across tile boundaries) -- measured on one MI355X: 2.51 ms at 8256
  // tiles where one-workgroup-per-unit launches took 2.51-2.61 ms (bimodal across runs),
  // equal at 528 / 1035 tiles.  MLFF_SYM_SCHED=static selects the one-workgroup-per-unit
  // launch (k_symv_tiles).
  // (A persistent schedule -- exactly C workgroups streaming equal batch ranges, tiles
  // cut at range boundaries -- measured slower at every size on one MI355X: 2.67 vs
  // 2.61 ms at 8256 tiles, 0.366 vs 0.338 ms at 1035: the hardware dispatcher's dynamic
  // whole-tile balance beats a static equal-byte split.)
  bool dynamic = true;
  // Generating role (k_symv_dyn<true>).  MLFF_SYM_GEN=0: off (every unit streamed on the old
  // grid); MLFF_SYM_GEN_TILES=<n>: n generated whole tiles (clamped) instead of the modelled
  // share; MLFF_SYM_GEN_QUARTERS=0|1|2: the quarter units to either role / streamed / generated.
  bool gen = true;
  int64_t gen_tiles = -1;
  int gen_quarters = 0;
  // MLFF_SYM_ROLES=cu|index|stream|gen: a workgroup's role by its arrival count on its CU; by
  // the parity of blockIdx.x (the first rule, A/B: the dispatcher deals blocks round-robin over
  // the XCDs, so parity put each role on half of the chip); every workgroup
  // streaming / generating (tests).  MLFF_SYM_STEAL=other|pool: what a workgroup whose own
  // range is exhausted takes first, the other role's whole tiles or the quarter units.
  int roles = kSymRolesCu;
  int pool_first = 0;
  // MLFF_SYM_WGS=2|3: the form of k_symv_dyn<true>, two resident workgroups per CU (8-row
  // streaming batches, one workgroup of each role) or three (4-row half batches, one streaming
  // and two generating); 0, the default: three where the operator has kSymThreeWgMinUnits
  // units per workgroup, else two (sym_plan)
  int wgs = 0;
  // MLFF_SYM_GEN_CLAMP=1: the generating role clamps the squared distance in every tile, also
  // where the points' extent says it cannot matter (SymGen::noclamp; A/B, tests)
  bool gen_clamp = false;
  // MLFF_SYM_REDUCE_LIST=0: k_sym_reduce_w instead of k_sym_reduce_wl (W > 1)
  bool reduce_list = true;
  // MLFF_SYM_PQ_ORDERED=1: k_sym_reduce_wl's arrival in the formally ordered form (pq_put)
  bool pq_ordered = false;
  // MLFF_SYM_TRACE=<n> (diagnostic): the n-th k_symv_dyn launch of the
  // process records each workgroup's start / end / units and prints where the tile stream's
  // time goes (print_symv_trace); launch_symv keeps the value of its first call
  long long trace_at = 0;
};

static SymKnobs sym_knobs() {
  SymKnobs k;
  if (const char *e = std::getenv("MLFF_SYM_WHOLE_ROUNDS")) k.whole_rounds = std::max<int64_t>(0, std::atoll(e));
  if (const char *e = std::getenv("MLFF_SYM_LSUB")) {
    const int v = std::atoi(e);
    if (v >= 1 && v <= 4) k.lsub = v;
  }
  if (const char *e = std::getenv("MLFF_SYM_SCHED")) k.dynamic = std::strcmp(e, "static") != 0;
  if (const char *e = std::getenv("MLFF_SYM_GEN")) k.gen = std::atoi(e) != 0;
  if (const char *e = std::getenv("MLFF_SYM_GEN_TILES")) k.gen_tiles = std::max<int64_t>(0, std::atoll(e));
  if (const char *e = std::getenv("MLFF_SYM_GEN_QUARTERS")) {
    const int v = std::atoi(e);
    if (v >= 0 && v <= 2) k.gen_quarters = v;
  }
  if (const char *e = std::getenv("MLFF_SYM_ROLES")) {
    if (std::strcmp(e, "index") == 0) k.roles = kSymRolesIndex;
    if (std::strcmp(e, "stream") == 0) k.roles = kSymRolesStream;
    if (std::strcmp(e, "gen") == 0) k.roles = kSymRolesGen;
  }
  if (const char *e = std::getenv("MLFF_SYM_STEAL")) k.pool_first = std::strcmp(e, "pool") == 0;
  if (const char *e = std::getenv("MLFF_SYM_WGS")) {
    const int v = std::atoi(e);
    if (v == 2 || v == 3) k.wgs = v;
  }
  if (const char *e = std::getenv("MLFF_SYM_GEN_CLAMP")) k.gen_clamp = std::atoi(e) != 0;
  if (const char *e = std::getenv("MLFF_SYM_REDUCE_LIST")) k.reduce_list = std::atoi(e) != 0;
  if (const char *e = std::getenv("MLFF_SYM_PQ_ORDERED")) k.pq_ordered = std::atoi(e) != 0;
  if (const char *e = std::getenv("MLFF_SYM_TRACE")) k.trace_at = std::atoll(e);
  return k;
}

// MLFF_SYM_TRACE: the ramp until every workgroup runs, the tail after the median one is done
// (tr: start, end (10-ns ticks), units, role and CU of each of the G workgroups; one sync),
// where the dispatcher put the two roles, and (role kernels) the shader clock each role's
// workgroups ran at: shader ticks over wall ticks between a workgroup's two stamps
static void print_symv_trace(const unsigned long long *tr, unsigned G, int64_t units, int wgs,
                             hipStream_t s) {
  std::vector<unsigned long long> h((size_t)(kTraceWords + kTraceClockWords) * G);
  if (hipStreamSynchronize(s) != hipSuccess ||
      hipMemcpy(h.data(), tr, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost) != hipSuccess)
    return;
  unsigned long long t0 = ~0ull, t1 = 0;
  std::vector<double> st, en, un;
  for (unsigned g = 0; g < G; ++g) {
    const unsigned long long *r = &h[(size_t)kTraceWords * g];
    if (r[0] == 0) continue;
    t0 = std::min(t0, r[0]);
    t1 = std::max(t1, r[1]);
  }
  double idle = 0.0;
  // per CU key and per XCC id: streaming / generating workgroups seen
  std::vector<int> cu_s(kSymCuWords, 0), cu_g(kSymCuWords, 0);
  int xs[16] = {0}, xg[16] = {0};
  double un_s = 0.0, un_g = 0.0;
  std::vector<double> mhz_s, mhz_g;  // shader clock of the workgroups of either role
  for (unsigned g = 0; g < G; ++g) {
    const unsigned long long *r = &h[(size_t)kTraceWords * g];
    if (r[0] == 0) continue;
    st.push_back(10.0 * (double)(r[0] - t0));
    en.push_back(10.0 * (double)(r[1] - t0));
    un.push_back((double)r[2]);
    idle += 10.0 * (double)(t1 - r[1]) + 10.0 * (double)(r[0] - t0);
    if (!(r[3] & 1ull)) continue;
    const bool gen = (r[3] & 2ull) != 0;
    const unsigned key = (unsigned)(r[3] >> 2) & (kSymCuWords - 1);
    ++(gen ? cu_g : cu_s)[key];
    ++(gen ? xg : xs)[key >> 8];
    (gen ? un_g : un_s) += (double)r[2];
    // shader ticks per 10-ns wall tick, times 100 MHz
    const unsigned long long *c = &h[(size_t)kTraceWords * G + (size_t)kTraceClockWords * g];
    if (c[0] != 0 && c[1] > c[0] && r[1] > r[0])
      (gen ? mhz_g : mhz_s).push_back(100.0 * (double)(c[1] - c[0]) / (double)(r[1] - r[0]));
  }
  auto q = [](std::vector<double> v, double f) {
    std::sort(v.begin(), v.end());
    return v.empty() ? 0.0 : v[(size_t)(f * (double)(v.size() - 1))];
  };
  const double span = 10.0 * (double)(t1 - t0);
  std::fprintf(stderr,
               "[sym trace] units %lld on %zu workgroups (units per wg p0/p50/p100 %.0f/%.0f/%.0f); "
               "span %.1f us; starts p50/p100 %.1f/%.1f us; ends p0/p10/p50/p90/p100 "
               "%.1f/%.1f/%.1f/%.1f/%.1f us; idle (ramp + tail) %.1f %% of wg-time\n",
               (long long)units, st.size(), q(un, 0.0), q(un, 0.5), q(un, 1.0), 1e-3 * span,
               1e-3 * q(st, 0.5), 1e-3 * q(st, 1.0), 1e-3 * q(en, 0.0), 1e-3 * q(en, 0.1),
               1e-3 * q(en, 0.5), 1e-3 * q(en, 0.9), 1e-3 * q(en, 1.0),
               100.0 * idle / (span * (double)st.size()));
  int cus = 0, paired = 0, two_s = 0, two_g = 0, other = 0;
  for (int k = 0; k < kSymCuWords; ++k) {
    if (cu_s[k] + cu_g[k] == 0) continue;
    ++cus;
    if (cu_s[k] == 1 && cu_g[k] == wgs - 1)
      ++paired;
    else if (cu_s[k] == wgs && cu_g[k] == 0)
      ++two_s;
    else if (cu_s[k] == 0 && cu_g[k] == wgs)
      ++two_g;
    else
      ++other;
  }
  std::string per_xcc;
  for (int x = 0; x < 16; ++x)
    if (xs[x] + xg[x] > 0)
      per_xcc += " " + std::to_string(x) + ":" + std::to_string(xs[x]) + "s+" + std::to_string(xg[x]) + "g";
  std::fprintf(stderr,
               "[sym trace] roles: %d distinct CU keys; CUs holding {1 stream + %d gen} %d, {%d stream} "
               "%d, {%d gen} %d, other %d; units taken stream / gen %.0f / %.0f (%.0f / %.0f per ms "
               "of the span); per XCC id%s\n",
               cus, wgs - 1, paired, wgs, two_s, wgs, two_g, other, un_s, un_g, 1e6 * un_s / span,
               1e6 * un_g / span, per_xcc.c_str());
  if (!mhz_s.empty() || !mhz_g.empty())
    std::fprintf(stderr,
                 "[sym trace] shader clock over a workgroup's life, median per role: stream %.0f MHz "
                 "(%zu workgroups), gen %.0f MHz (%zu workgroups)\n",
                 q(mhz_s, 0.5), mhz_s.size(), q(mhz_g, 0.5), mhz_g.size());
}

void launch_symv(const SymPack &sp, const double *v_full, double *P, const int *status,
                 hipStream_t s, PGather pg) {
  if (sp.ntiles == 0) return;
  const int64_t grid = sp.nwhole + ((sp.ntiles - sp.nwhole) << sp.lsub);
  if (sp.dyn == 0) {
    hipLaunchKernelGGL(k_symv_tiles, dim3((unsigned)grid), dim3(256), 0, s, sp.tiles, sp.list, v_full,
                       P, sp.Pq, sp.Np, (int)sp.nwhole, (int)sp.nb, sp.lsub, status);
    return;
  }
  const unsigned G = (unsigned)std::min<int64_t>(sp.dyn, grid);
  static const long long trace_at = sym_knobs().trace_at;
  static long long launches = 0;
  DevBuf<unsigned long long> tr;
  constexpr int kWords = kTraceWords + kTraceClockWords;
  if (trace_at > 0 && ++launches == trace_at && tr.alloc((int64_t)kWords * G) == hipSuccess)
    (void)hipMemsetAsync(tr, 0, sizeof(unsigned long long) * kWords * G, s);
  if (sp.gen && sp.rb4)
    hipLaunchKernelGGL((k_symv_dyn<true, 4>), dim3(G), dim3(256), 0, s,
                       sp.tiles, sp.list, v_full, P, sp.Pq, sp.Np, (int)sp.nwhole, (long long)grid,
                       (int)sp.nb, sp.lsub, sp.ticket, status, pg, sp.gsrc, tr);
  else if (sp.gen)
    hipLaunchKernelGGL(k_symv_dyn<true>, dim3(G), dim3(256), 0, s,
                       sp.tiles, sp.list, v_full, P, sp.Pq, sp.Np, (int)sp.nwhole, (long long)grid,
                       (int)sp.nb, sp.lsub, sp.ticket, status, pg, sp.gsrc, tr);
  else
    hipLaunchKernelGGL(k_symv_dyn<false>, dim3(G), dim3(256), 0, s,
                       sp.tiles, sp.list, v_full, P, sp.Pq, sp.Np, (int)sp.nwhole, (long long)grid,
                       (int)sp.nb, sp.lsub, sp.ticket, status, pg, SymGen{}, tr);
  if (tr != nullptr) print_symv_trace(tr, G, grid, sp.wgs, s);
}

void launch_sym_reduce(const SymPack &sp, int64_t n_out, double *y, bool epilogue, double sigma,
                       double lam, const double *vloc, const int *status, hipStream_t s) {
  if (n_out <= 0) return;
  const dim3 grid((unsigned)((n_out + 255) / 256));
  if (epilogue)
    hipLaunchKernelGGL((k_sym_reduce<true, false>), grid, dim3(256), 0, s, sp.P, sp.Pq, sp.split,
                       (int)sp.t_split, sp.Np, (int)sp.nb, (1 << sp.lsub) - 1, n_out, y, sigma, lam, vloc,
                       (double *)nullptr, sp.ticket, status);
  else
    hipLaunchKernelGGL((k_sym_reduce<false, false>), grid, dim3(256), 0, s, sp.P, sp.Pq, sp.split,
                       (int)sp.t_split, sp.Np, (int)sp.nb, (1 << sp.lsub) - 1, n_out, y, sigma, lam, vloc,
                       (double *)nullptr, sp.ticket, status);
}

void launch_sym_reduce_pq(const SymPack &sp, int64_t n_out, double *y, double sigma, double lam,
                          const double *p, double *pq_part, const int *status, hipStream_t s,
                          PGather pg) {
  hipLaunchKernelGGL((k_sym_reduce<true, true>), dim3(kVecGrid), dim3(256), 0, s, sp.P, sp.Pq,
                     sp.split, (int)sp.t_split, sp.Np, (int)sp.nb, (1 << sp.lsub) - 1, n_out, y, sigma,
                     lam, p, pq_part,
                     sp.ticket, status, pg, pg.gb != nullptr ? const_cast<double *>(p) : nullptr);
}

// k_sym_reduce_wl where the operator's build made its list (not with MLFF_SYM_REDUCE_LIST=0,
// A/B: k_sym_reduce_w) and the list fits: a row block's entries in LDS, the slot in an entry
static bool sym_reduce_list(const SymPack &sp) {
  return sp.plist != nullptr && sp.pstride <= kRwMaxList && sp.nb <= kSymPlistMaxSlots;
}

void launch_sym_reduce_ranks(const SymPack &sp, int rank, int world, int64_t blk,
                             const double *p_full, double *pq_part, double *pp_part,
                             double sigma, double lam, const int *status, hipStream_t s,
                             PGather pg, bool separate_publish) {
  const int64_t ld = (int64_t)world * blk;
  const dim3 grid(kVecGrid);
  double *pw = const_cast<double *>(p_full);  // written only when the p update is fused
  const PqPublish pub = p_full == nullptr
                            ? PqPublish{}
                            : PqPublish{sigma, lam, separate_publish ? 0 : world, sp.pq_ordered};
  const PGather pgu = p_full == nullptr ? PGather{} : pg;
  if (sym_reduce_list(sp)) {
    if (p_full == nullptr)
      hipLaunchKernelGGL((k_sym_reduce_wl<false>), grid, dim3(256), 0, s, sp.P, sp.Pq, sp.Np,
                         (int)sp.nb, sp.plist, sp.pstride, rank, ld, blk, sp.ystride, sp.yg, pw,
                         pq_part, pp_part, sp.ticket, status, pgu, pub);
    else
      hipLaunchKernelGGL((k_sym_reduce_wl<true>), grid, dim3(256), 0, s, sp.P, sp.Pq, sp.Np,
                         (int)sp.nb, sp.plist, sp.pstride, rank, ld, blk, sp.ystride, sp.yg, pw,
                         pq_part, pp_part, sp.ticket, status, pgu, pub);
  } else if (p_full == nullptr) {
    hipLaunchKernelGGL((k_sym_reduce_w<false>), grid, dim3(256), 0, s, sp.P, sp.Pq, sp.split, sp.Np,
                       (1 << sp.lsub) - 1, (int)sp.nb, rank,
                       sp.own, ld, blk, sp.ystride, sp.yg, pw, pq_part, pp_part,
                       sp.ticket, status, pgu, pub);
  } else {
    hipLaunchKernelGGL((k_sym_reduce_w<true>), grid, dim3(256), 0, s, sp.P, sp.Pq, sp.split, sp.Np,
                       (1 << sp.lsub) - 1, (int)sp.nb, rank,
                       sp.own, ld, blk, sp.ystride, sp.yg, pw, pq_part, pp_part,
                       sp.ticket, status, pgu, pub);
  }
  if (p_full != nullptr && separate_publish)  // MLFF_PQ_PUBLISH=1 (ctx->pq_publish): A/B
    hipLaunchKernelGGL(k_pq_publish, dim3(1), dim3(256), 0, s, pq_part, pp_part, kVecGrid, sigma, lam,
                       rank, world, blk, sp.ystride, sp.yg, status);
}

void launch_axpby_loc(const double *src, double *y, int64_t n, double sigma, double lam,
                      const double *vloc, const int *status, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_axpby_loc, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, y, n,
                     sigma, lam, vloc, status);
}

// tile assignment: tile (I, J), I >= J, is stored by the rank of row block I when both
// blocks are one rank's, else by I's or J's rank by the parity of I + J (balanced to a tile)
static int owner_host(int I, int J, int tpr) {
  const int a = I / tpr, c = J / tpr;
  if (a == c) return a;
  return ((I + J) & 1) ? a : c;
}

// ---- sym_build: plan, allocate, slot tables, fill ----

// What this rank stores and how the mat-vec runs over it
struct SymPlan {
  int64_t Np = 0;
  int nb = 0, tpr = 0;              // row blocks; tiles per rank block
  std::vector<int2> list;           // the rank's tiles
  std::vector<unsigned char> trans; // packed from the mirror rows (the row block is another rank's)
  int64_t nt = 0, nwhole = 0;
  int lsub = 2;
  int64_t nq = 3;                   // Pq planes: 2^lsub - 1
  int64_t dyn = 0;                  // resident workgroups of k_symv_dyn, 0: k_symv_tiles
  int wgs = 2;                      // ... per CU
  bool rb4 = false;                 // k_symv_dyn<true, 4>, the three-workgroup form
  bool gen = false;
  SymGen gsrc;
};

static SymPlan sym_plan(const mlff_ctx *ctx, const SymKnobs &kn) {
  SymPlan pl;
  pl.Np = round_up(ctx->ld, B);
  pl.nb = (int)(pl.Np / B);
  // tiles per rank block: blk is a multiple of B when world > 1 (mlff_ctx_create)
  pl.tpr = ctx->world > 1 ? (int)(ctx->blk / B) : pl.nb;
  for (int I = 0; I < pl.nb; ++I)
    for (int J = 0; J <= I; ++J) {
      if (owner_host(I, J, pl.tpr) != ctx->rank) continue;
      pl.list.push_back(make_int2(I, J));
      pl.trans.push_back(ctx->world > 1 && (I / pl.tpr) != ctx->rank ? 1 : 0);
    }
  pl.nt = (int64_t)pl.list.size();
  // Tail split: with C workgroups resident at once (2 per CU: 208 VGPRs -> 2 waves per
  // SIMD), whole tiles fill floor(nt / C) full rounds and the nt mod C remaining tiles
  // run as quarters instead of a partial round of lone 2-MB tiles.  Measured (one
  // MI355X, round 1): 1035 tiles 0.354 -> 0.338 ms, 528 tiles 0.198 -> 0.181 ms; more
  // quarters cost more than they save (all tiles as quarters: 2.51 -> 2.67 ms at 8256).
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess ||
      cus < 1)
    cus = 256;
  const int64_t C = 2 * (int64_t)cus;
  pl.nwhole = (pl.nt / C) * C;
  if (kn.whole_rounds >= 0) pl.nwhole = std::min<int64_t>(pl.nwhole, kn.whole_rounds * C);
  pl.lsub = kn.lsub;
  pl.nq = ((int64_t)1 << pl.lsub) - 1;
  pl.dyn = kn.dynamic ? C : 0;
  // Generating role (k_symv_dyn<true>): only where the tiles come from the RBF points, which
  // stay resident, and their dimension fits the role's registers.  The last n_gen whole tiles
  // are evaluated instead of read; the share follows the two roles' measured rates
  // (kSymStreamRate / kSymGenRate, common.h).
  if (pl.dyn > 0 && pl.nt > 0 && !ctx->has_matrix && ctx->rbf.ready && ctx->rbf.d >= 1 &&
      ctx->rbf.d <= kSymGenMaxD) {
    int64_t n_s = (int64_t)((double)pl.nwhole * kSymStreamRate / (kSymStreamRate + kSymGenRate) + 0.5);
    if (kn.gen_tiles >= 0) n_s = pl.nwhole - std::min<int64_t>(pl.nwhole, kn.gen_tiles);
    const int qmode = kn.gen_quarters;
    bool on = kn.gen;
    if (pl.nwhole == pl.nt && n_s == pl.nwhole) on = false;  // nothing to generate
    if (n_s == pl.nwhole && qmode == 1) on = false;          // every unit streamed
    if (on) {
      pl.gen = true;
      // the three-workgroup form: as many workgroups per CU as the runtime says are resident
      // (registers and LDS of the 4-row instantiation: 3), and that many times the CUs in all.
      // The unit set (nwhole, C) stays the two-workgroup form's, so the slots sum alike.
      // It pays from kSymThreeWgMinUnits units per workgroup: with fewer, the launch ends on
      // generating workgroups that took one more whole tile at their 0.15 ms each (two of them
      // share a CU's SIMDs), as one rank of 8 at N = 65536 does -- 1056 units on 768
      // workgroups, 0.349 against 0.300 ms per iteration -- while one rank of 4 (2112 units)
      // gains 7 %, as one rank of 2 and the single GPU do (profiles/symlean/).
      if (kn.wgs != 2) {
        int occ = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k_symv_dyn<true, 4>, 256, 0) != hipSuccess ||
            occ < 1)
          occ = 2;
        const int64_t nunits = pl.nwhole + ((pl.nt - pl.nwhole) << pl.lsub);
        pl.rb4 = kn.wgs == 3 || (occ > 2 && nunits >= kSymThreeWgMinUnits * occ * cus);
        if (pl.rb4) {
          pl.wgs = occ;
          pl.dyn = (int64_t)occ * cus;
        }
      }
      // every rank holds the same points, so every rank takes the same decision
      const bool noclamp = !kn.gen_clamp && ctx->rbf.finite && ctx->rbf.extent2 <= kSymGenNoClampExtent2;
      pl.gsrc = SymGen{ctx->rbf.Xs, ctx->rbf.d, ctx->rbf.jitter, ctx->N, ctx->rows_per, ctx->blk,
                       (int)n_s, qmode, kn.roles, kn.pool_first, pl.wgs, noclamp ? 1 : 0};
    }
  }
  return pl;
}

// device buffers for the plan (kept when the sizes did not change), and the plan into sp
static int sym_alloc(mlff_ctx *ctx, const SymPlan &pl, const SymKnobs &kn) {
  SymPack &sp = ctx->sym;
  hipStream_t s = ctx->stream;
  const int64_t nt = pl.nt, nb = pl.nb, Np = pl.Np, nq = pl.nq;
  if (sp.tiles == nullptr || sp.ntiles != nt || sp.Np != Np || sp.pq_planes != nq) {
    sp = SymPack{};
    if (nt > 0) {
      MLFF_HIP(ctx, sp.tiles.alloc(nt * B * B));
      MLFF_HIP(ctx, sp.list.alloc(nt));
    }
    MLFF_HIP(ctx, sp.P.alloc(nb * Np));
    MLFF_HIP(ctx, hipMemsetAsync(sp.P, 0, sizeof(double) * nb * Np, s));
    MLFF_HIP(ctx, sp.Pq.alloc(nq * nb * Np));
    MLFF_HIP(ctx, hipMemsetAsync(sp.Pq, 0, sizeof(double) * nq * nb * Np, s));
    sp.pq_planes = nq;
    MLFF_HIP(ctx, sp.split.alloc(nb * nb));
    MLFF_HIP(ctx, sp.own.alloc(nb * (nb + 1)));
    // k_symv_dyn's work counters and the rank reductions' arrival counter (kTicketWords), then
    // the per-CU arrival words of its role rule
    const size_t tw = (kTicketWords + kSymCuWords) * sizeof(unsigned long long);
    MLFF_HIP(ctx, sp.ticket.alloc(kTicketWords + kSymCuWords));
    MLFF_HIP(ctx, hipMemsetAsync(sp.ticket, 0, tw, s));
    if (ctx->world > 1) {
      // reduce-scatter operand: rank blocks of blk rows + a tail of p.q shares
      sp.ystride = ctx->blk + round_up(ctx->world, kPad);
      const int64_t ny = (int64_t)ctx->world * sp.ystride;
      MLFF_HIP(ctx, sp.yg.alloc(ny));
      MLFF_HIP(ctx, sp.yr.alloc(sp.ystride));
      MLFF_HIP(ctx, hipMemsetAsync(sp.yg, 0, sizeof(double) * ny, s));
      MLFF_HIP(ctx, hipMemsetAsync(sp.yr, 0, sizeof(double) * sp.ystride, s));
    }
  }
  sp.ntiles = nt;
  sp.Np = Np;
  sp.nb = nb;
  sp.tiles_per_rank = pl.tpr;
  sp.nwhole = pl.nwhole;
  sp.lsub = pl.lsub;
  sp.dyn = pl.dyn;
  sp.wgs = pl.dyn > 0 ? pl.wgs : 0;
  sp.rb4 = pl.rb4;
  sp.gen = pl.gen;
  sp.gsrc = pl.gsrc;
  sp.pq_ordered = kn.pq_ordered;
  return MLFF_OK;
}

// the slot reductions' tables: split flags (k_sym_reduce), owned slots (k_sym_reduce_w) and
// the flat load list (k_sym_reduce_wl)
static int sym_slot_tables(mlff_ctx *ctx, const SymPlan &pl, const SymKnobs &kn) {
  SymPack &sp = ctx->sym;
  hipStream_t s = ctx->stream;
  const int nb = pl.nb;
  std::vector<unsigned char> split((size_t)nb * nb, 0);
  sp.t_split = nb;
  for (int64_t t = pl.nwhole; t < pl.nt; ++t) {
    split[(size_t)pl.list[t].x * nb + pl.list[t].y] = 1;
    sp.t_split = std::min<int64_t>(sp.t_split, pl.list[t].x);
  }
  MLFF_HIP(ctx, hipMemcpyAsync(sp.split, split.data(), split.size(), hipMemcpyHostToDevice, s));
  // owned slots per row block: row bi's slot t is this rank's when it stores tile
  // (max(bi, t), min(bi, t)); rows of nb ascending entries, then nb counts
  std::vector<int> own((size_t)nb * (nb + 1), 0);
  for (int bi = 0; bi < nb; ++bi) {
    int c = 0;
    for (int t = 0; t < nb; ++t)
      if (owner_host(std::max(bi, t), std::min(bi, t), pl.tpr) == ctx->rank)
        own[(size_t)bi * nb + c++] = sym_own_entry(t, t > bi && split[(size_t)t * nb + bi]);
    own[(size_t)nb * nb + bi] = c;
  }
  MLFF_HIP(ctx, hipMemcpyAsync(sp.own, own.data(), sizeof(int) * own.size(), hipMemcpyHostToDevice, s));
  // the flat load list: each owned slot, a split slot followed by its planes; row blocks at a
  // stride of the longest list (rounded to 64 entries)
  std::vector<std::vector<int>> lists((size_t)nb);
  sp.pmax = 0;
  for (int bi = 0; bi < nb; ++bi) {
    for (int j = 0; j < own[(size_t)nb * nb + bi]; ++j) {
      const int e = own[(size_t)bi * nb + j];
      for (int h = 0; h <= (sym_own_split(e) ? pl.nq : 0); ++h)
        lists[bi].push_back(sym_plist_entry(sym_own_slot(e), h));
    }
    sp.pmax = std::max(sp.pmax, (int)lists[bi].size());
  }
  sp.pstride = round_up(std::max(sp.pmax, 1), 64);
  std::vector<int> plist((size_t)nb * (sp.pstride + 1), 0);
  for (int bi = 0; bi < nb; ++bi) {
    std::copy(lists[bi].begin(), lists[bi].end(), plist.begin() + (size_t)bi * sp.pstride);
    plist[(size_t)nb * sp.pstride + bi] = (int)lists[bi].size();
  }
  sp.plist.reset();
  if (ctx->world > 1 && kn.reduce_list) {
    MLFF_HIP(ctx, sp.plist.alloc((int64_t)plist.size()));
    MLFF_HIP(ctx, hipMemcpyAsync(sp.plist, plist.data(), sizeof(int) * plist.size(),
                                 hipMemcpyHostToDevice, s));
  }
  MLFF_HIP(ctx, hipStreamSynchronize(s));  // the host vectors go out of scope
  return MLFF_OK;
}

// the tiles: generated from the RBF points, or packed from the dense rows and, on request,
// compared with their mirror
static int sym_fill(mlff_ctx *ctx, const SymPlan &pl, bool check_symmetry, bool *symmetric_out) {
  SymPack &sp = ctx->sym;
  hipStream_t s = ctx->stream;
  const int64_t nt = pl.nt;
  if (symmetric_out) *symmetric_out = true;
  if (nt == 0) return MLFF_OK;
  MLFF_HIP(ctx, hipMemcpyAsync(sp.list, pl.list.data(), sizeof(int2) * nt, hipMemcpyHostToDevice, s));
  if (!ctx->has_matrix && ctx->rbf.ready) {  // generated from the points (no dense rows)
    hipLaunchKernelGGL(k_sym_gen_rbf, dim3((unsigned)nt), dim3(256), 0, s, sp.list, ctx->rbf.Xs,
                       ctx->rbf.d, ctx->rbf.jitter, ctx->N, ctx->rows_per, ctx->blk, sp.tiles);
    MLFF_HIP(ctx, hipGetLastError());
    MLFF_HIP(ctx, hipStreamSynchronize(s));
    return MLFF_OK;
  }
  DevBuf<unsigned char> dtrans;  // both released on every return
  DevBuf<int> dflag;
  MLFF_HIP(ctx, dtrans.alloc(nt));
  MLFF_HIP(ctx, dflag.alloc(1));
  MLFF_HIP(ctx, hipMemcpyAsync(dtrans, pl.trans.data(), nt, hipMemcpyHostToDevice, s));
  MLFF_HIP(ctx, hipMemsetAsync(dflag, 0, sizeof(int), s));
  const int64_t rowbase = (int64_t)ctx->rank * ctx->blk;
  hipLaunchKernelGGL(k_sym_pack<false>, dim3((unsigned)nt), dim3(256), 0, s, ctx->K, ctx->ld, rowbase,
                     ctx->blk, sp.list, dtrans, sp.tiles, dflag);
  int mism = 0;
  if (check_symmetry) {
    // mirror read: every tile compared against rows J B + c (one rank holds all rows)
    MLFF_HIP(ctx, hipMemsetAsync(dtrans, 1, nt, s));
    hipLaunchKernelGGL(k_sym_pack<true>, dim3((unsigned)nt), dim3(256), 0, s, ctx->K, ctx->ld, rowbase,
                       ctx->blk, sp.list, dtrans, sp.tiles, dflag);
    MLFF_HIP(ctx, hipMemcpyAsync(&mism, dflag, sizeof(int), hipMemcpyDeviceToHost, s));
  }
  MLFF_HIP(ctx, hipGetLastError());
  MLFF_HIP(ctx, hipStreamSynchronize(s));
  if (symmetric_out) *symmetric_out = (mism == 0);
  return MLFF_OK;
}

int sym_build(mlff_ctx *ctx, bool check_symmetry, bool *symmetric_out) {
  const SymKnobs kn = sym_knobs();
  const SymPlan pl = sym_plan(ctx, kn);
  if (int rc = sym_alloc(ctx, pl, kn); rc != MLFF_OK) return rc;
  if (int rc = sym_slot_tables(ctx, pl, kn); rc != MLFF_OK) return rc;
  if (int rc = sym_fill(ctx, pl, check_symmetry, symmetric_out); rc != MLFF_OK) return rc;
  ctx->sym.ready = true;
  return MLFF_OK;
}

}  // namespace mlff
