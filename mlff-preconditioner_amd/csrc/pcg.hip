// The scipy-1.7.3-compatible PCG driver of libmlffpcg.so: the low-rank apply, the iteration,
// its timed segments and the mlff_pcg_* / mlff_timing_* entry points (include/mlffpcg.h).
//
// PCG driver (restating scipy.sparse.linalg.cg 1.7.3 = CGREVCOM template + python
// wrapper, as called at src/sGDML/sgdml/solvers/iterative_solver.py:995-1005):
//   atol = tol * ||b||                      (legacy atol=None; ||A x0 - b|| <= tol exits early)
//   r = b - A x0;  if ||r|| < atol: done
//   ITER = ITER + 1:  z = M r; rho = r.z; p = z + (rho/rho1) p (p = z at ITER 1)
//                     q = A p; alpha = rho / p.q; x += alpha p; r -= alpha q
//                     stop test ||r|| <= atol, re-checked with r = b - A x when ITER > 1
//                     ITER == maxiter -> info = maxiter
// Every iteration is 5-7 launches on one stream with all scalars kept on the
// device; the host polls the status word once per chunk of iterations, and
// kernels of iterations past convergence return immediately (status gating),
// so the iteration count is exact without a per-iteration host sync.
#include "common.h"

#include <algorithm>
#include <cmath>

using namespace mlff;

namespace mlff {

// The halves of the two-pass apply.  lowrank_tr: tpart = T r, summed over the ranks unless the
// caller's own collective carries it (reduce = false: the ranks iteration's merged all-reduce);
// lowrank_z: z = sigma_p / lam (r - T^T tpart) with the rho partials r . z (rho may be null).
int lowrank_tr(mlff_ctx *ctx, const double *r, const int *status, StopFold fold, bool reduce) {
  const LowRank &lr = ctx->lr;
  launch_gemv_split(lr.T, ctx->blk, lr.k, ctx->blk, lr.tsplit, r, lr.tpart, status, ctx->stream, fold);
  if (reduce) MLFF_TRY(comm_allreduce(ctx, lr.tpart, (size_t)(lr.k * lr.tsplit)));
  return MLFF_OK;
}

void lowrank_z(mlff_ctx *ctx, const double *r, double *z, double *rho, const int *status,
               StopFold fold) {
  const LowRank &lr = ctx->lr;
  launch_precon_z(lr.T, ctx->blk, lr.k, lr.tsplit, lr.tpart, r, z, ctx->nrows, lr.sigma_p,
                  1.0 / ctx->lam, rho, status, ctx->stream, lr.zpart, lr.zsplit, fold);
}

// z = sigma_p / lam (r - T^T T r) and the rho partials r . z (rho may be null) in the form the
// build chose (the one-pass forms: one rank only).  status gates the kernels (null: ungated),
// fold / xf ride in the apply's first kernel, fault is the cluster form's time-out word (ST_FAULT).
int lowrank_apply(mlff_ctx *ctx, const double *r, double *z, double *rho, const int *status,
                  int *fault, StopFold fold, XrFold xf) {
  LowRank &lr = ctx->lr;
  hipStream_t s = ctx->stream;
  const double lam_inv = 1.0 / ctx->lam;
  if (ctx->exact_sums) {  // measurement anchor: two double-double passes, stop test and rho separately
    if (fold.st != nullptr) launch_stoptest(fold.rr_part, fold.st, fold.trace, fold.it, s);
    launch_dd_lowrank(lr.T, ctx->blk, lr.k, r, z, ctx->nrows, lr.sigma_p, lam_inv, lr.tpart, status, s);
    if (rho != nullptr) launch_dot_part(r, z, ctx->nrows, rho, status, s);
  } else if (lr.form == LowRank::kRows) {
    launch_lr_apply_rows(lr.T, ctx->blk, lr.k, r, z, ctx->nrows, lr.sigma_p, lam_inv, rho, status, s,
                         lr.gpart, fold, xf);
  } else if (lr.form == LowRank::kCluster) {
    launch_lr_apply_cluster(lr.T, ctx->blk, lr.k, lr.q, r, z, ctx->nrows, lr.sigma_p, lam_inv, rho,
                            status, s, lr.gpart, lr.slots, lr.next_epoch(), fault, fold);
  } else {
    MLFF_TRY(lowrank_tr(ctx, r, status, fold));
    lowrank_z(ctx, r, z, rho, status);
  }
  return MLFF_OK;
}

}  // namespace mlff

namespace {

constexpr int kTimingPool = 4096;

double *rho_part(mlff_ctx *c) { return c->part + 0 * kMaxPart; }
double *pq_part(mlff_ctx *c) { return c->part + 1 * kMaxPart; }
double *rr_part(mlff_ctx *c) { return c->part + 2 * kMaxPart; }

// sum of kVecGrid partials (device) as a host double, synchronous
int sum_parts_sync(mlff_ctx *ctx, const double *part, double *out) {
  launch_reduce_to(part, kVecGrid, &ctx->st->pad0, ctx->stream);
  MLFF_HIP(ctx, hipMemcpyAsync(out, &ctx->st->pad0, sizeof(double), hipMemcpyDeviceToHost,
                               ctx->stream));
  MLFF_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MLFF_OK;
}

// scalar = sum over ranks of a . b (local), synchronous
int dot_sync(mlff_ctx *ctx, const double *a, const double *b, double *out) {
  double *part = ctx->part;  // slot 0 region
  launch_dot_part(a, b, ctx->nrows, part, nullptr, ctx->stream);
  MLFF_TRY(comm_allreduce(ctx, part, kVecGrid));
  return sum_parts_sync(ctx, part, out);
}

hipEvent_t timing_event(mlff_ctx *ctx) {
  Timing &t = ctx->timing;
  if (t.used >= t.ev.size()) {
    hipEvent_t e;
    if (hipEventCreateWithFlags(&e, timing_event_flags()) != hipSuccess) return nullptr;
    t.ev.push_back(e);
  }
  return t.ev[t.used++];
}

// a timed segment of one iteration: events ev0 -> ev1 of the pool and what ran between them
struct GemvMark {
  size_t ev0, ev1;
  long long it;
  SegKind kind;
};

constexpr size_t kNoMark = (size_t)-1;

size_t mark_begin(mlff_ctx *ctx, std::vector<GemvMark> *marks) {
  if (!ctx->timing.on || marks == nullptr || !ctx->timing.sample) return kNoMark;
  hipEvent_t e0 = timing_event(ctx);
  if (e0 == nullptr) return kNoMark;
  hipEventRecord(e0, ctx->stream);
  return ctx->timing.used - 1;
}

void mark_end(mlff_ctx *ctx, std::vector<GemvMark> *marks, size_t i0, long long it,
              SegKind kind = kSegOperator) {
  if (i0 == kNoMark) return;
  hipEvent_t e1 = timing_event(ctx);
  if (e1) {
    hipEventRecord(e1, ctx->stream);
    marks->push_back({i0, ctx->timing.used - 1, it, kind});
  }
}

// Which CG vector updates ride inside other kernels.  Decided once per chunk of
// iterations: every input is host state that only entry points change, or demote_cluster
// after the chunk's poll, so none of it can move between two iterations of a chunk.
struct IterPlan {
  bool lowrank;  // the low-rank preconditioner is active
  // one rank, matrix-free operator (default form): p = z + beta p formed inside the operator
  // kernels (k_update_p's bits, one launch less)
  bool p_in_operator;
  // ... with the one-pass rows apply also k_update_xr of iteration it - 1 folded into iteration
  // it's apply (x, r, rr partials written by k_lr_fin) and its stop test into the operator's
  // first kernel: 4 launches per iteration instead of 6
  bool xr_in_apply;
  // symmetric tiles, dynamic schedule (configs[2]): p = z + beta p formed by the tile workgroups
  // (k_symv_dyn, PGather) from z and the rho partials in the gather buffer and written by the
  // slot reduction -- k_update_p's / k_update_p_gathered's bits, one launch less
  bool p_in_tiles;
};

IterPlan plan_iteration(const mlff_ctx *ctx) {
  IterPlan pl;
  pl.lowrank = ctx->lr.active();
  pl.p_in_operator = ctx->use_mf && mf_can_fuse_p(ctx);
  pl.xr_in_apply = pl.p_in_operator && pl.lowrank && ctx->lr.form == LowRank::kRows && ctx->fuse_xr;
  pl.p_in_tiles = ctx->fuse_p && ctx->use_sym && ctx->sym.dyn > 0 && ctx->sym.ntiles > 0;
  // The tile workgroups read z and its rho partials from the gather buffer.  On several ranks
  // every iteration puts them there (the apply or k_copy_dot writes this rank's gather block);
  // on one rank only the low-rank apply can be pointed at it -- without a preconditioner z is r
  // itself and k_dot_part's partials go to rho_part -- and the exact-sum anchor (one rank only)
  // keeps every update a launch of its own.
  if (ctx->world == 1) pl.p_in_tiles = pl.p_in_tiles && pl.lowrank && !ctx->exact_sums;
  return pl;
}

// One PCG iteration on several ranks: three collectives instead of five:
//   allgather(z_g | rho partials)  -> rho and the whole p on every rank
//   [symmetric tiles] reduce-scatter(K p partial rows | p.q shares) -> q rows and p.q
//   [other storages]  allreduce(p.q partials)
//   allreduce(rr partials | T r partials of the next iteration)   (low-rank precon)
// Same recurrence as launch_iteration; the sums are over the same terms in another
// (fixed) order, bitwise identical on all ranks.
int launch_iteration_ranks(mlff_ctx *ctx, const IterPlan &plan, long long it,
                           std::vector<GemvMark> *marks, bool fold_in, bool stop_out) {
  hipStream_t s = ctx->stream;
  const int *status = &ctx->st->status;
  double *p_loc = ctx->p_full + (int64_t)ctx->rank * ctx->blk;
  double *zg = ctx->gb + (int64_t)ctx->rank * ctx->gstride;  // this rank's gather block
  LowRank &lr = ctx->lr;
  double *rrp = plan.lowrank ? lr.tpart_base : rr_part(ctx);
  StopFold fold;  // stop test of iteration it - 1 in this iteration's first kernel
  if (fold_in) fold = StopFold{rrp, ctx->st, ctx->trace, it - 1};
  if (plan.lowrank) {
    if (!lr.spec_t) {
      MLFF_TRY(lowrank_tr(ctx, ctx->r, status, fold));
      fold = StopFold{};
    }
    // the low-rank apply: T r (issued at the end of the previous iteration, kSegPreconTail) + z here
    const size_t pm = mark_begin(ctx, marks);
    lowrank_z(ctx, ctx->r, zg, zg + ctx->blk, status, fold);
    mark_end(ctx, marks, pm, it, kSegPrecon);
  } else {
    launch_copy_dot(ctx->r, ctx->nrows, zg, zg + ctx->blk, status, s, fold);
  }
  size_t c0 = mark_begin(ctx, marks);
  MLFF_TRY(comm_allgather(ctx, zg, ctx->gb, (size_t)ctx->gstride));
  mark_end(ctx, marks, c0, it, kSegComm);
  PGather pg;  // p formed by the tile workgroups from the gathered z (IterPlan::p_in_tiles)
  if (plan.p_in_tiles)
    pg = PGather{ctx->gb, ctx->gstride, ctx->blk, ctx->world, ctx->st, it};
  else
    launch_update_p_gathered(ctx->gb, ctx->gstride, ctx->blk, ctx->world, ctx->p_full, ctx->st, it,
                             status, s);
  const size_t e0 = mark_begin(ctx, marks);
  if (ctx->use_sym) {
    SymPack &sp = ctx->sym;
    launch_symv(sp, ctx->p_full, sp.P, status, s, pg);
    launch_sym_reduce_ranks(sp, ctx->rank, ctx->world, ctx->blk, ctx->p_full, pq_part(ctx),
                            pq_part(ctx) + kVecGrid, ctx->sigma_K, ctx->lam, status, s, pg,
                            ctx->pq_publish);
    mark_end(ctx, marks, e0, it);
    c0 = mark_begin(ctx, marks);
    MLFF_TRY(comm_reduce_scatter(ctx, sp.yg, sp.yr, (size_t)sp.ystride));
    mark_end(ctx, marks, c0, it, kSegComm);
    launch_update_xr_shares(ctx->x, ctx->r, p_loc, sp.yr, sp.yr + ctx->blk, ctx->world, ctx->nrows,
                            ctx->sigma_K, ctx->lam, rrp, ctx->st, status, s);
  } else {
    MLFF_TRY(launch_operator(ctx, ctx->p_full, ctx->q, p_loc, status, pq_part(ctx)));
    mark_end(ctx, marks, e0, it);
    c0 = mark_begin(ctx, marks);
    MLFF_TRY(comm_allreduce(ctx, pq_part(ctx), kVecGrid));
    mark_end(ctx, marks, c0, it, kSegComm);
    launch_update_xr(ctx->x, ctx->r, p_loc, ctx->q, ctx->nrows, pq_part(ctx), rrp, ctx->st, status, s);
  }
  if (plan.lowrank) {
    // the T r half of iteration it + 1's apply: bracketed with that iteration (its
    // z half, kSegPrecon) so a sampled apply is always timed whole
    ctx->timing.sample = (it + 1) % ctx->timing.every == 0;
    const size_t tm = mark_begin(ctx, marks);
    MLFF_TRY(lowrank_tr(ctx, ctx->r, status, StopFold{}, false));
    mark_end(ctx, marks, tm, it, kSegPreconTail);
    c0 = mark_begin(ctx, marks);
    MLFF_TRY(comm_allreduce(ctx, lr.tpart_base, (size_t)(kVecGrid + lr.k * lr.tsplit)));
    mark_end(ctx, marks, c0, it, kSegComm);
    lr.spec_t = true;
  } else {
    c0 = mark_begin(ctx, marks);
    MLFF_TRY(comm_allreduce(ctx, rrp, kVecGrid));
    mark_end(ctx, marks, c0, it, kSegComm);
  }
  if (stop_out) launch_stoptest(rrp, ctx->st, ctx->trace, it, s);
  return MLFF_OK;
}

// one PCG iteration (ITER = it), all launches status gated.  fold_in: the stop test of
// iteration it - 1 runs in this iteration's first kernel (StopFold); stop_out: the stop
// test of this iteration runs as its own launch (last iteration of a chunk)
int launch_iteration(mlff_ctx *ctx, const IterPlan &plan, long long it, std::vector<GemvMark> *marks,
                     bool fold_in, bool stop_out) {
  // events cost GPU time between the kernels they bracket: only every timing.every-th
  // iteration is bracketed (the averages are over the sampled iterations)
  ctx->timing.sample = it % ctx->timing.every == 0;
  if (ctx->world > 1) return launch_iteration_ranks(ctx, plan, it, marks, fold_in, stop_out);
  hipStream_t s = ctx->stream;
  const int *status = &ctx->st->status;
  double *p_loc = ctx->p_full + (int64_t)ctx->rank * ctx->blk;
  StopFold fold;
  if (fold_in) fold = StopFold{rr_part(ctx), ctx->st, ctx->trace, it - 1};
  XrFold xf;
  StopFold fold_op;
  if (plan.xr_in_apply && fold_in) {  // iteration it - 1 left its x, r update to this iteration
    xf = XrFold{ctx->x, ctx->r, p_loc, ctx->q, pq_part(ctx), rr_part(ctx), ctx->st};
    fold_op = fold;
    fold = StopFold{};
  }
  // p formed by the tile workgroups: the apply writes z and its rho partials into the gather
  // block for them
  double *zout = plan.p_in_tiles ? ctx->gb : ctx->z;
  double *rhoout = plan.p_in_tiles ? ctx->gb + ctx->blk : rho_part(ctx);
  const double *zsrc;
  if (plan.lowrank) {
    const size_t pm = mark_begin(ctx, marks);
    MLFF_TRY(lowrank_apply(ctx, ctx->r, zout, rhoout, status, &ctx->st->status, fold, xf));
    mark_end(ctx, marks, pm, it, kSegPrecon);
    zsrc = zout;
  } else {
    launch_dot_part(ctx->r, ctx->r, ctx->nrows, rho_part(ctx), status, s, fold);
    zsrc = ctx->r;
  }
  const PFuse pf{zsrc, rho_part(ctx), ctx->st, it, fold_op};
  if (!plan.p_in_operator && !plan.p_in_tiles)
    launch_update_p(zsrc, p_loc, ctx->nrows, rho_part(ctx), ctx->st, it, status, s);
  const size_t e0 = mark_begin(ctx, marks);
  if (ctx->use_sym) {
    // q = sigma K p + lam p and the p.q partials from the slot reduction (no dot launch)
    const PGather pg1 = plan.p_in_tiles ? PGather{ctx->gb, ctx->gstride, ctx->blk, 1, ctx->st, it}
                                        : PGather{};
    launch_symv(ctx->sym, ctx->p_full, ctx->sym.P, status, s, pg1);
    launch_sym_reduce_pq(ctx->sym, ctx->nrows, ctx->q, ctx->sigma_K, ctx->lam, p_loc,
                         pq_part(ctx), status, s, pg1);
    mark_end(ctx, marks, e0, it);
  } else {
    MLFF_TRY(launch_operator(ctx, ctx->p_full, ctx->q, p_loc, status, pq_part(ctx),
                             plan.p_in_operator ? &pf : nullptr));
    mark_end(ctx, marks, e0, it);
  }
  if (!plan.xr_in_apply || stop_out)  // else: done by iteration it + 1 (same chunk, fold_in)
    launch_update_xr(ctx->x, ctx->r, p_loc, ctx->q, ctx->nrows, pq_part(ctx), rr_part(ctx), ctx->st,
                     status, s);
  if (stop_out) launch_stoptest(rr_part(ctx), ctx->st, ctx->trace, it, s);
  return MLFF_OK;
}

// r = b - A x with the all-reduced ||r||^2 partials left in rr_part(ctx) (stream ordered):
// the solve's start from x0 != 0 and the true-residual recheck
int true_residual(mlff_ctx *ctx) {
  hipStream_t s = ctx->stream;
  MLFF_HIP(ctx, hipMemcpyAsync(ctx->xg + (int64_t)ctx->rank * ctx->blk, ctx->x,
                               sizeof(double) * ctx->blk, hipMemcpyDeviceToDevice, s));
  MLFF_TRY(allgather_blocks(ctx, ctx->xg));
  MLFF_TRY(launch_operator(ctx, ctx->xg, ctx->q, ctx->x, nullptr));
  launch_residual(ctx->b, ctx->q, ctx->r, ctx->nrows, rr_part(ctx), s);
  return comm_allreduce(ctx, rr_part(ctx), kVecGrid);
}

// true-residual recheck of the python wrapper: r = b - A x, resid = ||r||
int do_recheck(mlff_ctx *ctx) {
  MLFF_TRY(true_residual(ctx));
  launch_recheck_finish(rr_part(ctx), ctx->st, ctx->trace, ctx->stream);
  MLFF_HIP(ctx, hipGetLastError());
  return MLFF_OK;
}

int poll_state(mlff_ctx *ctx) {
  MLFF_HIP(ctx, hipMemcpyAsync(ctx->h_st, ctx->st, sizeof(DevState), hipMemcpyDeviceToHost,
                               ctx->stream));
  MLFF_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MLFF_OK;
}

// launch iterations first .. last on the stream, between the chunk's two events (timing on)
int launch_chunk(mlff_ctx *ctx, const IterPlan &plan, int64_t first, int64_t last,
                 std::vector<GemvMark> *marks, hipEvent_t *c0, hipEvent_t *c1) {
  hipStream_t s = ctx->stream;
  ctx->timing.used = 0;
  marks->clear();
  if (ctx->timing.on) {
    *c0 = timing_event(ctx);
    if (*c0) hipEventRecord(*c0, s);
  }
  for (int64_t it = first; it <= last; ++it)
    MLFF_TRY(launch_iteration(ctx, plan, it, marks, it > first, it == last));
  if (ctx->timing.on) {
    *c1 = timing_event(ctx);
    if (*c1) hipEventRecord(*c1, s);
  }
  return MLFF_OK;
}

// after the chunk's poll: a timed-out cluster apply is demoted and the solve set running again
int demote_on_cluster_fault(mlff_ctx *ctx) {
  if (ctx->h_st->status != ST_FAULT || ctx->lr.form != LowRank::kCluster) return MLFF_OK;
  // the cluster apply could not complete its hand-offs (its workgroups were not all
  // resident, e.g. another process's kernels held CUs): nothing of iteration iters + 1
  // was written past its (idempotent) stop test, so the solve continues from there on
  // the two-pass apply
  ctx->lr.demote_cluster();
  ctx->h_st->status = ST_RUNNING;
  MLFF_HIP(ctx, hipMemsetAsync(&ctx->st->status, 0, sizeof(int), ctx->stream));  // ST_RUNNING
  return MLFF_OK;
}

// add the polled chunk's segments and its whole span (c0 -> c1) to the context's Timing
void book_chunk(mlff_ctx *ctx, const std::vector<GemvMark> &marks, hipEvent_t c0, hipEvent_t c1) {
  Timing &t = ctx->timing;
  if (!t.on || !c0 || !c1) return;
  const int64_t done_now = ctx->h_st->iters;
  for (const GemvMark &mk : marks) {
    if (mk.it > done_now) continue;  // gated launches after convergence
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, t.ev[mk.ev0], t.ev[mk.ev1]) != hipSuccess) continue;
    const bool tail = mk.kind == kSegPreconTail;  // second part of one apply: its time only
    Timing::Bucket &b = t.seg[tail ? kSegPrecon : mk.kind];
    b.ms += ms;
    if (!tail) b.count += 1;
  }
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, c0, c1) == hipSuccess) {
    t.iter.ms += ms;
    t.iter.count += done_now - ctx->pcg_done;
  }
}

// the wrapper's true-residual rechecks, until the device leaves ST_RECHECK
int run_rechecks(mlff_ctx *ctx) {
  while (ctx->h_st->status == ST_RECHECK) {
    MLFF_TRY(do_recheck(ctx));
    MLFF_TRY(poll_state(ctx));
    ctx->lr.drop_speculative_t();  // r was recomputed
  }
  return MLFF_OK;
}

void read_bucket(const Timing::Bucket &b, double *ms, int64_t *count) {
  if (ms) *ms = b.ms;
  if (count) *count = b.count;
}

}  // namespace

extern "C" {

int mlff_pcg_start(mlff_ctx *ctx, const double *b_local, const double *x0_local, double tol,
                   int64_t maxiter, int *early_exit_out) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  MLFF_TRY(require_operator(ctx));
  if ((b_local == nullptr && ctx->nrows > 0) || maxiter < 1 || !(tol >= 0.0))
    return set_error(ctx, MLFF_ERR_ARG, "pcg_start: need b, maxiter >= 1, tol >= 0");
  MLFF_TRY(resolve_storage(ctx));
  hipStream_t s = ctx->stream;
  if (ctx->trace_cap < maxiter + 1) {
    MLFF_HIP(ctx, ctx->trace.alloc(maxiter + 1));
    ctx->trace_cap = maxiter + 1;
  }
  for (double *v : {ctx->b.get(), ctx->x.get(), ctx->r.get(), ctx->z.get(), ctx->q.get()})
    MLFF_HIP(ctx, hipMemsetAsync(v, 0, sizeof(double) * ctx->blk, s));
  MLFF_HIP(ctx, hipMemsetAsync(ctx->p_full, 0, sizeof(double) * ctx->ld, s));
  if (ctx->gb != nullptr)
    MLFF_HIP(ctx, hipMemsetAsync(ctx->gb, 0, sizeof(double) * ctx->world * ctx->gstride, s));
  if (ctx->nrows > 0) {
    MLFF_HIP(ctx, hipMemcpyAsync(ctx->b, b_local, sizeof(double) * ctx->nrows, hipMemcpyHostToDevice, s));
    if (x0_local)
      MLFF_HIP(ctx, hipMemcpyAsync(ctx->x, x0_local, sizeof(double) * ctx->nrows, hipMemcpyHostToDevice, s));
  }
  double bb = 0.0, xx = 0.0;
  MLFF_TRY(dot_sync(ctx, ctx->b, ctx->b, &bb));
  MLFF_TRY(dot_sync(ctx, ctx->x, ctx->x, &xx));
  const double bnorm = std::sqrt(bb);
  double r0 = bnorm;
  if (xx != 0.0) {
    // r = b - A x0
    double rr = 0.0;
    MLFF_TRY(true_residual(ctx));
    MLFF_TRY(sum_parts_sync(ctx, rr_part(ctx), &rr));
    r0 = std::sqrt(rr);
  } else {
    MLFF_HIP(ctx, hipMemcpyAsync(ctx->r, ctx->b, sizeof(double) * ctx->blk, hipMemcpyDeviceToDevice, s));
  }
  DevState h{};
  h.maxiter = maxiter;
  h.atol = (bnorm == 0.0) ? tol : tol * bnorm;
  h.status = ST_RUNNING;
  h.resid = r0;
  int early = 0;
  if (r0 <= tol) {          // _get_atol legacy: ||A x0 - b|| <= tol -> return x0
    h.status = ST_CONVERGED;
    early = 1;
  } else if (r0 < h.atol) {  // CGREVCOM: ||r0|| < TOL -> converged before the first iteration
    h.status = ST_CONVERGED;
  }
  MLFF_HIP(ctx, hipMemcpyAsync(ctx->st, &h, sizeof(DevState), hipMemcpyHostToDevice, s));
  MLFF_HIP(ctx, hipMemcpyAsync(ctx->trace, &r0, sizeof(double), hipMemcpyHostToDevice, s));
  MLFF_HIP(ctx, hipStreamSynchronize(s));
  *ctx->h_st = h;
  ctx->lr.drop_speculative_t();
  ctx->tol = tol;
  ctx->bnorm = bnorm;
  ctx->pcg_done = 0;
  ctx->pcg_active = true;
  if (early_exit_out) *early_exit_out = early;
  return MLFF_OK;
  MLFF_API_END(ctx)
}

int mlff_pcg_run(mlff_ctx *ctx, int64_t n_iter, int64_t chunk, int *status_out) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  if (!ctx->pcg_active) return set_error(ctx, MLFF_ERR_STATE, "mlff_pcg_start not called");
  if (n_iter < 0) return set_error(ctx, MLFF_ERR_ARG, "n_iter < 0");
  if (chunk <= 0) chunk = 32;
  const long long maxiter = ctx->h_st->maxiter;
  const int64_t target = std::min<int64_t>(ctx->pcg_done + n_iter, maxiter);
  std::vector<GemvMark> marks;
  while (ctx->h_st->status == ST_RUNNING && ctx->pcg_done < target) {
    const int64_t first = ctx->pcg_done + 1;
    const int64_t last = std::min<int64_t>(first + chunk - 1, target);
    const IterPlan plan = plan_iteration(ctx);  // per chunk: the demotion below changes its inputs
    hipEvent_t c0 = nullptr, c1 = nullptr;
    MLFF_TRY(launch_chunk(ctx, plan, first, last, &marks, &c0, &c1));
    MLFF_HIP(ctx, hipGetLastError());
    MLFF_TRY(poll_state(ctx));
    MLFF_TRY(demote_on_cluster_fault(ctx));
    book_chunk(ctx, marks, c0, c1);
    MLFF_TRY(run_rechecks(ctx));
    ctx->pcg_done = ctx->h_st->iters;
  }
  if (ctx->h_st->status == ST_FAULT)
    return set_error(ctx, MLFF_ERR_HIP, "PCG: a cluster hand-off of the one-pass apply timed out");
  if (status_out) *status_out = ctx->h_st->status;
  return MLFF_OK;
  MLFF_API_END(ctx)
}

int mlff_pcg_result(mlff_ctx *ctx, int64_t *iters_out, int *status_out, double *resid_out,
                    int *info_out) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  if (!ctx->pcg_active) return set_error(ctx, MLFF_ERR_STATE, "mlff_pcg_start not called");
  MLFF_TRY(poll_state(ctx));
  const DevState &h = *ctx->h_st;
  if (iters_out) *iters_out = h.iters;
  if (status_out) *status_out = h.status;
  if (resid_out) *resid_out = h.resid;
  if (info_out) *info_out = (h.status == ST_CONVERGED) ? 0 : (int)h.iters;
  return MLFF_OK;
  MLFF_API_END(ctx)
}

int mlff_pcg_get_x(mlff_ctx *ctx, double *x_local) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  if (ctx->nrows > 0) {
    if (x_local == nullptr) return set_error(ctx, MLFF_ERR_ARG, "null x");
    MLFF_HIP(ctx, hipMemcpyAsync(x_local, ctx->x, sizeof(double) * ctx->nrows, hipMemcpyDeviceToHost, ctx->stream));
  }
  MLFF_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MLFF_OK;
  MLFF_API_END(ctx)
}

int mlff_pcg_get_trace(mlff_ctx *ctx, double *trace_out, int64_t n) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  if (!ctx->pcg_active || ctx->trace == nullptr) return set_error(ctx, MLFF_ERR_STATE, "no solve");
  if (trace_out == nullptr || n < 0) return set_error(ctx, MLFF_ERR_ARG, "bad output");
  MLFF_TRY(poll_state(ctx));
  const int64_t avail = ctx->h_st->iters + 1;
  const int64_t cnt = std::min<int64_t>(n, avail);
  if (cnt > 0)
    MLFF_HIP(ctx, hipMemcpy(trace_out, ctx->trace, sizeof(double) * cnt, hipMemcpyDeviceToHost));
  return MLFF_OK;
  MLFF_API_END(ctx)
}

int mlff_timing_enable(mlff_ctx *ctx, int on) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  ctx->timing.on = on != 0;
  ctx->timing.every = on > 1 ? on : 1;
  if (ctx->timing.on && ctx->timing.ev.size() < kTimingPool) ctx->timing.ev.reserve(kTimingPool);
  return MLFF_OK;
  MLFF_API_END(ctx)
}

int mlff_timing_read(mlff_ctx *ctx, double *gemv_ms, int64_t *gemv_count, double *iter_ms,
                     int64_t *iter_count) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  read_bucket(ctx->timing.seg[kSegOperator], gemv_ms, gemv_count);
  read_bucket(ctx->timing.iter, iter_ms, iter_count);
  return MLFF_OK;
  MLFF_API_END(ctx)
}

int mlff_timing_read_precon(mlff_ctx *ctx, double *ms, int64_t *count) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  read_bucket(ctx->timing.seg[kSegPrecon], ms, count);
  return MLFF_OK;
  MLFF_API_END(ctx)
}

int mlff_timing_read_comm(mlff_ctx *ctx, double *ms, int64_t *count) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  read_bucket(ctx->timing.seg[kSegComm], ms, count);
  return MLFF_OK;
  MLFF_API_END(ctx)
}

int mlff_timing_reset(mlff_ctx *ctx) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  for (Timing::Bucket &b : ctx->timing.seg) b = Timing::Bucket{};
  ctx->timing.iter = Timing::Bucket{};
  return MLFF_OK;
  MLFF_API_END(ctx)
}

}  // extern "C"
