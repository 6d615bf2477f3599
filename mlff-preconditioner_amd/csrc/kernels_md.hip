// Molecular dynamics with a trained sGDML model, the trajectory kept on the device (mlff_md_run):
// Q independent replicas, n_steps steps of synchronous velocity Verlet, every stride-th step
// recorded.  The reference implementation has no counterpart (ASE drives its predictor one step
// at a time through the host).
//
// The step, with h_i = (dt acc_unit / 2) / m_i from the host, one value per atom:
//   v <- v + h_i F          (md_kick: the product rounded, then the sum; no fma)
//   R <- R + dt v           (the same)
//   E, F <- the model at R  (mlff_predict's E and F, bit for bit)
//   v <- v + h_i F
// E and F come from the prediction's own code: k_desc_t<true>, the pair stage and its arguments
// (pr_launch_fd, kernels_predict.hip), chunk_sum's order, pred_energy and jt_row (sgdml_pair.h).
// A numpy loop over mlff_predict with the two updates written as above therefore reproduces a run
// exactly, whatever the batch, the slab, the frame capacity, the device split or the form below.
//
// Two forms of the per-step work, chosen by the model (mlff_md_set_form overrides):
//  - four launches, any D: k_pr_desc, the pair stage, k_pr_sum and k_md_step in the place of
//    k_pr_jt: one thread per row 3 at + c forms F, completes the velocity of the step, records the
//    frame if the step is one, applies the next half kick and the drift and writes the new R into
//    pd.Rq for the next step's k_pr_desc.
//  - two launches, tile models (D <= 288): the pair stage and k_md_mid, one workgroup per replica.
//    It adds the S chunk partials of the replica's D + 1 columns into LDS (chunk_sum's two halves:
//    chunk_group_sum of the entry blocks, four of them at a time on the four quarters of the
//    workgroup, then chunk_groups_total), forms J^T Fd from the Jacobian the previous
//    launch left in pd.Rddq, finishes the step as k_md_step does and forms the descriptor and the
//    Jacobian of the new R (desc_entry<true> from LDS).  A run starts with one k_pr_desc.
//
// Between frame flushes there is no host copy and no stream synchronisation: R, V and the
// Jacobian stay in device buffers, frames (rows R, V, E and, when asked for, F per replica) are
// written by the step kernel into a device frame buffer of md.cap frames and copied out through
// pinned memory, one copy and one synchronisation, when the buffer is full and at the end.  Q
// larger than the prediction's slab runs slab after slab, each through all its steps.
//
// Safety: no index and no trip count depends on a value of R, V or F.  A replica that blows up
// (coinciding atoms, inf / NaN) carries its NaNs into its own frames; no sum runs across replicas.
// No atomics.
#include "common.h"
#include "sgdml_pair.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace mlff {

namespace {

constexpr int kMdMaxBlocks = 19;  // two-launch form: entry blocks of kSumE, D + 1 <= 304
constexpr int kMdMaxRows = 72;    // two-launch form: 3n of the tile models (n <= 24)
constexpr int kMdMidThreads = 1024;  // two-launch form: threads of k_md_mid (D + 1 <= 304 of them sum)
constexpr int64_t kMdFrameBudget = (int64_t)256 << 20;

struct MdArgs {
  const double *part;  // two launches: the chunk partials S x nq x PS
  int64_t PS, ecol, nq;
  int S;
  const double *Fd, *E;  // four launches: the slab's Fd and E (k_pr_sum)
  double *Rd, *Rdd;      // the slab's descriptors and Jacobians (written by the two-launch form)
  double *R, *V;         // nq x 3n positions (pd.Rq) and velocities
  const double *h;       // n
  int n;
  int64_t D;
  double std, cint, dt;
  double *frame;         // the frame this step records (nq rows of W), or null
  int64_t W;
  int want_f;            // the rows carry F
  int complete;          // the step has a first half (every step but 0): v += h F
  int advance;           // a step follows: v += h F, R += dt v
};

// x + a b with the product rounded on its own: behind this barrier it is not contracted into
// the sum (__dmul_rn and __dadd_rn are a plain * and + to the compiler)
__device__ __forceinline__ double md_kick(double x, double a, double b) {
  double p = __dmul_rn(a, b);
  asm volatile("" : "+v"(p));
  return __dadd_rn(x, p);
}

// Row r of replica q with its force F: completes the velocity, records, kicks and drifts.
// Returns the row's position for the next step.
__device__ __forceinline__ double md_row(const MdArgs &a, int64_t q, int r, double x, double v, double hi,
                                         double F, double E) {
  const int64_t n3 = 3 * (int64_t)a.n, i = q * n3 + r;
  if (a.complete) v = md_kick(v, hi, F);
  if (a.frame != nullptr) {
    double *fr = a.frame + q * a.W;
    fr[r] = x;
    fr[n3 + r] = v;
    if (r == 0) fr[2 * n3] = E;
    if (a.want_f) fr[2 * n3 + 1 + r] = F;
  }
  if (a.advance) {
    v = md_kick(v, hi, F);
    x = md_kick(x, a.dt, v);
    a.R[i] = x;
  }
  a.V[i] = v;
  return x;
}

// four launches: k_pr_jt's grid, one thread per row
__global__ __launch_bounds__(64) void k_md_step(MdArgs a) {
  const int r = blockIdx.x * 64 + threadIdx.x;
  if (r >= 3 * a.n) return;
  const int64_t q = blockIdx.y, i = q * 3 * a.n + r;
  const int at = r / 3, c = r % 3;
  const double x = a.R[i], v = a.V[i], hi = a.h[at], E = a.E[q];
  const double F = a.std * jt_row(a.Rdd + q * a.D * 3 + c, a.Fd + q * a.D, a.n, at);
  md_row(a, q, r, x, v, hi, F, E);
}

// two launches: one workgroup per replica, see the head of the file.  Its kMdMidThreads / 256
// quarters each take every fourth entry block of the chunk sums, so that four blocks' batches of
// loads are in flight at once (ethanol's three blocks: all of them).
__global__ __launch_bounds__(kMdMidThreads) void k_md_mid(MdArgs a) {
  __shared__ double sP[kMdMaxBlocks][kSumG][kSumE];
  __shared__ double sF[kMdMaxBlocks * kSumE];  // Fd (D entries), then the summed energy partial
  __shared__ double sX[kMdMaxRows];
  const int tid = threadIdx.x, el = tid % kSumE, g = (tid % 256) / kSumE;
  const int64_t q = blockIdx.x, D = a.D;
  const int n3 = 3 * a.n;
  const bool row = tid < n3;
  const int at = row ? tid / 3 : 0, c = tid % 3;
  // the row's state: in flight during the chunk sums
  const int64_t i = q * n3 + (row ? tid : 0);
  const double x0 = a.R[i], v0 = a.V[i], hi = a.h[at];
  const int nb = (int)((D + 1 + kSumE - 1) / kSumE);
  for (int b = tid / 256; b < nb; b += kMdMidThreads / 256) {
    const int64_t e = (int64_t)b * kSumE + el;
    sP[b][g][el] = chunk_group_sum(a.part + q * a.PS + (e < D ? e : a.ecol), a.nq * a.PS, a.S, e <= D, g);
  }
  __syncthreads();
  if (tid <= D) sF[tid] = chunk_groups_total(sP[tid / kSumE], el);
  __syncthreads();
  if (row) {
    const double F = a.std * jt_row(a.Rdd + q * D * 3 + c, sF, a.n, at);
    sX[tid] = md_row(a, q, tid, x0, v0, hi, F, pred_energy(sF[D], a.std, a.cint));
  }
  if (!a.advance) return;
  __syncthreads();  // the old Jacobian is consumed, the new positions are in sX
  if (tid < D) {
    const TriIdx ab = tri_invert(tid);
    const DescEntry de = desc_entry<true>(sX, ab.a, ab.b);
    a.Rd[q * D + tid] = de.rd;
    a.Rdd[(q * D + tid) * 3 + 0] = de.x;
    a.Rdd[(q * D + tid) * 3 + 1] = de.y;
    a.Rdd[(q * D + tid) * 3 + 2] = de.z;
  }
}

bool md_two_launch_ok(const PredData &pd) {
  return pd.form == 0 && pd.D + 1 <= (int64_t)kMdMaxBlocks * kSumE && 3 * pd.n <= kMdMaxRows;
}

// the form and the frame capacity, on the first call after a model is set (no allocation)
int md_configure(mlff_ctx *ctx) {
  PredData &pd = ctx->pred;
  PredData::Md &md = pd.md;
  md.launches = md.want != 0 ? md.want : (md_two_launch_ok(pd) ? 2 : 4);
  if (md.cap > 0) return MLFF_OK;
  // frames of a full slab with forces within the budget, at least 2
  const int64_t n3 = 3 * (int64_t)pd.n;
  int64_t cap = std::max<int64_t>(2, kMdFrameBudget / (pd.slab * (3 * n3 + 1) * 8));
  if (const char *e = std::getenv("MLFF_MD_FRAMES")) {
    const long long v = std::atoll(e);
    if (v < 1 || v > ((long long)1 << 24)) return set_error(ctx, MLFF_ERR_ARG, "md: MLFF_MD_FRAMES out of range");
    cap = v;
  }
  md.cap = cap;
  return MLFF_OK;
}

}  // namespace

int md_set_form(mlff_ctx *ctx, int launches) {
  PredData &pd = ctx->pred;
  if (launches != 0 && launches != 2 && launches != 4)
    return set_error(ctx, MLFF_ERR_ARG, "md: the form is 0 (default), 2 or 4 launches per step");
  if (launches == 2 && !md_two_launch_ok(pd))
    return set_error(ctx, MLFF_ERR_ARG, "md: two launches per step need a tile model (D <= 288)");
  pd.md.want = launches;
  return md_configure(ctx);
}

int md_info(mlff_ctx *ctx, int *launches_per_step, int64_t *frame_capacity, int64_t *syncs_last_run) {
  MLFF_TRY(md_configure(ctx));
  const PredData::Md &md = ctx->pred.md;
  if (launches_per_step) *launches_per_step = md.launches;
  if (frame_capacity) *frame_capacity = md.cap;
  if (syncs_last_run) *syncs_last_run = md.syncs;
  return MLFF_OK;
}

int md_run(mlff_ctx *ctx, const double *R0, const double *V0, const double *h, int64_t Q, double dt,
           int64_t n_steps, int64_t stride, bool want_forces, double *R_out, double *V_out,
           double *E_out, double *F_out) {
  MLFF_TRY(md_configure(ctx));
  PredData &pd = ctx->pred;
  PredData::Md &md = pd.md;
  hipStream_t s = ctx->stream;
  const int64_t n3 = 3 * (int64_t)pd.n, D = pd.D, n = pd.n;
  const int64_t T = n_steps / stride + 1;
  const int64_t W = (want_forces ? 3 : 2) * n3 + 1;
  md.syncs = 0;
  if (Q == 0) return MLFF_OK;
  if (!md.ready) {
    int rc;
    if ((rc = md.hV.alloc(ctx, n + pd.slab * n3, "md")) != MLFF_OK ||
        (rc = md.h_in.alloc(ctx, n + pd.slab * n3, "md")) != MLFF_OK) {
      md.hV.reset();
      return rc;
    }
    md.ready = true;
  }
  // the frame buffers: what this run needs of the capacity, kept for later runs
  const int64_t need = std::min(T, md.cap) * std::min(Q, pd.slab) * W;
  if (need > md.frame_len) {
    md.frame_len = 0;
    int rc;
    if ((rc = md.frames.alloc(ctx, need, "md")) != MLFF_OK || (rc = md.h_frames.alloc(ctx, need, "md")) != MLFF_OK) {
      md.frames.reset();
      return rc;
    }
    md.frame_len = need;
  }
  MdArgs a{};
  a.part = pd.part;
  a.PS = pd.PS;
  a.ecol = pd.ecol;
  a.S = pd.S;
  a.Fd = pd.Fd;
  a.E = pd.EF;
  a.Rd = pd.Rdq;
  a.Rdd = pd.Rddq;
  a.R = pd.Rq;
  a.h = md.hV;
  a.V = md.hV + n;
  a.n = pd.n;
  a.D = D;
  a.std = pd.std;
  a.cint = pd.c;
  a.dt = dt;
  a.W = W;
  a.want_f = want_forces ? 1 : 0;
  const bool two = md.launches == 2;
  for (int64_t q0 = 0; q0 < Q; q0 += pd.slab) {
    const int64_t nq = std::min<int64_t>(pd.slab, Q - q0);
    a.nq = nq;
    // R0 into the prediction's geometry buffer, h and V0 behind each other: two copies in
    std::memcpy(pd.h_in, R0 + q0 * n3, sizeof(double) * nq * n3);
    std::memcpy(md.h_in, h, sizeof(double) * n);
    std::memcpy(md.h_in + n, V0 + q0 * n3, sizeof(double) * nq * n3);
    MLFF_HIP(ctx, hipMemcpyAsync(pd.Rq, pd.h_in, sizeof(double) * nq * n3, hipMemcpyHostToDevice, s));
    MLFF_HIP(ctx, hipMemcpyAsync(md.hV, md.h_in, sizeof(double) * (n + nq * n3), hipMemcpyHostToDevice, s));
    if (two) pr_launch_fd(pd, nq, kPrStageDesc, s);
    int64_t t0 = 0, held = 0;  // the first frame in the buffer and the frames in it
    for (int64_t k = 0; k <= n_steps; ++k) {
      const bool rec = k % stride == 0;
      a.frame = rec ? md.frames + held * nq * W : nullptr;
      a.complete = k > 0;
      a.advance = k < n_steps;
      if (two) {
        pr_launch_fd(pd, nq, kPrStagePair, s);
        hipLaunchKernelGGL(k_md_mid, dim3((unsigned)nq), dim3(kMdMidThreads), 0, s, a);
      } else {
        pr_launch_fd(pd, nq, kPrStageAll, s);
        hipLaunchKernelGGL(k_md_step, dim3((unsigned)((n3 + 63) / 64), (unsigned)nq), dim3(64), 0, s, a);
      }
      if (!rec) continue;
      held += 1;
      if (held < md.cap && k < n_steps) continue;
      // flush: one copy, one synchronisation
      MLFF_HIP(ctx, hipGetLastError());
      MLFF_HIP(ctx, hipMemcpyAsync(md.h_frames, md.frames, sizeof(double) * held * nq * W, hipMemcpyDeviceToHost, s));
      MLFF_HIP(ctx, hipStreamSynchronize(s));
      md.syncs += 1;
      for (int64_t f = 0; f < held; ++f)
        for (int64_t u = 0; u < nq; ++u) {
          const double *fr = md.h_frames + (f * nq + u) * W;
          const int64_t o = (q0 + u) * T + t0 + f;
          std::memcpy(R_out + o * n3, fr, sizeof(double) * n3);
          std::memcpy(V_out + o * n3, fr + n3, sizeof(double) * n3);
          E_out[o] = fr[2 * n3];
          if (want_forces) std::memcpy(F_out + o * n3, fr + 2 * n3 + 1, sizeof(double) * n3);
        }
      t0 += held;
      held = 0;
    }
  }
  return MLFF_OK;
}

}  // namespace mlff
