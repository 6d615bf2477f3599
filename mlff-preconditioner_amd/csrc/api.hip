// C ABI of libmlffpcg.so (declared in include/mlffpcg.h): context, kernel
// matrix, collectives, operator storage and preconditioner builds.  The PCG driver and the
// timing entry points are in pcg.hip.
#include "common.h"

#include <cstdlib>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstring>
#include <limits>
#include <map>
#include <mutex>

using namespace mlff;

static thread_local std::string g_last_error;

namespace mlff {

int set_error(mlff_ctx *ctx, int code, const std::string &msg) {
  if (ctx != nullptr) ctx->err = msg;
  g_last_error = msg;
  return code;
}

void local_abort(mlff_ctx *ctx);

int api_exception(mlff_ctx *ctx, int code, const char *what) {
  try {
    local_abort(ctx);
    return set_error(ctx, code, std::string("C++ exception in libmlffpcg: ") + (what ? what : ""));
  } catch (...) {
    return code;
  }
}

constexpr size_t kScratchChunk = size_t(64) << 20;

ScratchScope::ScratchScope(mlff_ctx *c) : ctx(c), chunk(c->scratch_cur), off(c->scratch_off) {
  ++ctx->scratch_depth;
}

// Closing the outermost scope returns every chunk but one standard-size chunk to the device
// (after the stream has drained the kernels that used them): build temporaries such as the
// k x k Woodbury Gram, eigensolver panels or split-K slabs do not stay allocated through the
// PCG that follows.
ScratchScope::~ScratchScope() {
  ctx->scratch_cur = chunk;
  ctx->scratch_off = off;
  if (--ctx->scratch_depth != 0) return;
  auto &ch = ctx->scratch_chunks;
  const bool keep_first = !ch.empty() && ch[0].size == kScratchChunk;
  if (ch.size() > (keep_first ? 1u : 0u)) {
    (void)hipStreamSynchronize(ctx->stream);
    ch.resize(keep_first ? 1 : 0);
  }
  ctx->scratch_cur = 0;
  ctx->scratch_off = 0;
}

int scratch_get(mlff_ctx *ctx, size_t bytes, void **out) {
  constexpr size_t kAlign = 256, kChunk = kScratchChunk;
  bytes = (bytes + kAlign - 1) / kAlign * kAlign;
  auto &ch = ctx->scratch_chunks;
  while (true) {
    if (ctx->scratch_cur < ch.size()) {
      const auto &c = ch[ctx->scratch_cur];
      if (ctx->scratch_off + bytes <= c.size) {
        *out = c.p + ctx->scratch_off;
        ctx->scratch_off += bytes;
        return MLFF_OK;
      }
      ++ctx->scratch_cur;  // the rest of this chunk stays unused until the scope closes
      ctx->scratch_off = 0;
      continue;
    }
    DevBuf<char> p;
    MLFF_HIP(ctx, p.alloc((int64_t)std::max(bytes, kChunk)));
    ch.push_back({std::move(p), std::max(bytes, kChunk)});
    ctx->scratch_cur = ch.size() - 1;
    ctx->scratch_off = 0;
  }
}

// A device failure on one rank of an in-process group aborts the group, so its peers
// return MLFF_ERR_COMM from their next collective instead of waiting forever.
int hip_check(mlff_ctx *ctx, hipError_t e, const char *what) {
  const int code = (e == hipErrorOutOfMemory) ? MLFF_ERR_NOMEM : MLFF_ERR_HIP;
  local_abort(ctx);
  return set_error(ctx, code, std::string(what) + ": " + hipGetErrorString(e));
}

int nccl_check(mlff_ctx *ctx, ncclResult_t e, const char *what) {
  return set_error(ctx, MLFF_ERR_COMM, std::string(what) + ": " + ncclGetErrorString(e));
}

// In-process transport: `world` contexts of one process (one host thread each,
// any devices) joined by a comm_id "LOCAL:<key>".  Collectives are host-staged
// and reduce in rank order.  Used to exercise the multi-rank code path on a
// single GPU (RCCL refuses two ranks on one device); production multi-GPU runs
// use RCCL.
struct LocalGroup {
  int world = 0;
  std::mutex m;
  std::condition_variable cv;
  int arrived = 0;
  long long gen = 0;
  bool aborted = false;
  std::vector<double> buf;  // world * count staging
  // false once any member has aborted the group
  bool barrier() {
    std::unique_lock<std::mutex> lk(m);
    if (aborted) return false;
    const long long g = gen;
    if (++arrived == world) {
      arrived = 0;
      ++gen;
      cv.notify_all();
    } else {
      cv.wait(lk, [&] { return gen != g || aborted; });
    }
    return !aborted;
  }
  void abort() {
    std::lock_guard<std::mutex> lk(m);
    aborted = true;
    cv.notify_all();
  }
};

void local_abort(mlff_ctx *ctx) {
  if (ctx != nullptr && ctx->local) ctx->local->abort();
}

#define LOCAL_BARRIER(ctx, g)                                                        \
  do {                                                                               \
    if (!(g).barrier())                                                              \
      return set_error((ctx), MLFF_ERR_COMM, "in-process group aborted by a peer rank"); \
  } while (0)

static std::mutex g_groups_m;
static std::map<std::string, std::weak_ptr<LocalGroup>> g_groups;

std::shared_ptr<LocalGroup> join_local_group(const std::string &key, int world) {
  std::lock_guard<std::mutex> lk(g_groups_m);
  auto it = g_groups.find(key);
  std::shared_ptr<LocalGroup> gp = (it != g_groups.end()) ? it->second.lock() : nullptr;
  if (!gp) {
    gp = std::make_shared<LocalGroup>();
    gp->world = world;
    g_groups[key] = gp;
  }
  return gp;
}

__global__ void k_selftest_fill(double *p, size_t n, double scale) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    p[i] = scale * (1.0 + 0.5 * (double)i);
}

// RCCL transport: the collectives are enqueued on the context's stream, so they are ordered
// after the kernels that produced `send` and before the ones that read `recv` with no host
// synchronisation.  Semantics are those of the LOCAL branches below: allreduce in place over
// n doubles; allgather of `count` doubles per rank into recv[rank*count ...] (in place when
// send == recv + rank*count); reduce-scatter of world*count doubles into this rank's `count`.
// mlff_comm_selftest drives these three functions on a one-rank communicator, the only RCCL
// configuration a one-GPU box can run.
static int rccl_allreduce(mlff_ctx *ctx, double *buf, size_t n) {
  MLFF_NCCL(ctx, ncclAllReduce(buf, buf, n, ncclDouble, ncclSum, ctx->comm, ctx->stream));
  return MLFF_OK;
}

static int rccl_allgather(mlff_ctx *ctx, const double *send, double *recv, size_t count) {
  MLFF_NCCL(ctx, ncclAllGather(send, recv, count, ncclDouble, ctx->comm, ctx->stream));
  return MLFF_OK;
}

static int rccl_reduce_scatter(mlff_ctx *ctx, const double *send, double *recv, size_t count) {
  MLFF_NCCL(ctx, ncclReduceScatter(send, recv, count, ncclDouble, ncclSum, ctx->comm, ctx->stream));
  return MLFF_OK;
}

// SOLO transport (comm_id "SOLO:..."): ONE rank of a W-way split runs alone and every
// collective keeps only this rank's own contribution (no data from peers, no wait).  The
// numbers are meaningless; the kernels, their sizes and their launch sequence are those of
// rank `rank` of W, so a one-GPU kernel trace shows the per-rank compute of the sharded
// iteration without the collectives (bench.py --solo-world).  Profiling only.
int comm_allreduce(mlff_ctx *ctx, double *buf, size_t n) {
  if (ctx->world <= 1 || n == 0 || ctx->solo) return MLFF_OK;
  if (ctx->comm != nullptr) return rccl_allreduce(ctx, buf, n);
  LocalGroup &g = *ctx->local;
  std::vector<double> mine(n), sum(n, 0.0);
  MLFF_HIP(ctx, hipMemcpyAsync(mine.data(), buf, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
  MLFF_HIP(ctx, hipStreamSynchronize(ctx->stream));
  LOCAL_BARRIER(ctx, g);  // previous users of g.buf are done
  if (ctx->rank == 0) g.buf.assign((size_t)g.world * n, 0.0);
  LOCAL_BARRIER(ctx, g);
  std::memcpy(g.buf.data() + (size_t)ctx->rank * n, mine.data(), sizeof(double) * n);
  LOCAL_BARRIER(ctx, g);
  for (int r = 0; r < g.world; ++r)
    for (size_t i = 0; i < n; ++i) sum[i] += g.buf[(size_t)r * n + i];
  LOCAL_BARRIER(ctx, g);
  MLFF_HIP(ctx, hipMemcpyAsync(buf, sum.data(), sizeof(double) * n, hipMemcpyHostToDevice, ctx->stream));
  MLFF_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MLFF_OK;
}

int comm_allgather(mlff_ctx *ctx, const double *send, double *recv, size_t count) {
  if (ctx->world <= 1) {
    if (send != recv)
      MLFF_HIP(ctx, hipMemcpyAsync(recv, send, sizeof(double) * count, hipMemcpyDeviceToDevice, ctx->stream));
    return MLFF_OK;
  }
  if (ctx->solo) {
    double *own = recv + (size_t)ctx->rank * count;
    if (send != own)
      MLFF_HIP(ctx, hipMemcpyAsync(own, send, sizeof(double) * count, hipMemcpyDeviceToDevice, ctx->stream));
    return MLFF_OK;
  }
  if (ctx->comm != nullptr) return rccl_allgather(ctx, send, recv, count);
  LocalGroup &g = *ctx->local;
  std::vector<double> mine(count);
  MLFF_HIP(ctx, hipMemcpyAsync(mine.data(), send, sizeof(double) * count, hipMemcpyDeviceToHost, ctx->stream));
  MLFF_HIP(ctx, hipStreamSynchronize(ctx->stream));
  LOCAL_BARRIER(ctx, g);
  if (ctx->rank == 0) g.buf.assign((size_t)g.world * count, 0.0);
  LOCAL_BARRIER(ctx, g);
  std::memcpy(g.buf.data() + (size_t)ctx->rank * count, mine.data(), sizeof(double) * count);
  LOCAL_BARRIER(ctx, g);
  std::vector<double> all(g.buf);
  LOCAL_BARRIER(ctx, g);
  MLFF_HIP(ctx, hipMemcpyAsync(recv, all.data(), sizeof(double) * all.size(), hipMemcpyHostToDevice, ctx->stream));
  MLFF_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MLFF_OK;
}

int comm_reduce_scatter(mlff_ctx *ctx, const double *send, double *recv, size_t count) {
  if (ctx->world <= 1) {
    if (send != recv)
      MLFF_HIP(ctx, hipMemcpyAsync(recv, send, sizeof(double) * count, hipMemcpyDeviceToDevice, ctx->stream));
    return MLFF_OK;
  }
  if (ctx->solo) {
    MLFF_HIP(ctx, hipMemcpyAsync(recv, send + (size_t)ctx->rank * count, sizeof(double) * count,
                                 hipMemcpyDeviceToDevice, ctx->stream));
    return MLFF_OK;
  }
  if (ctx->comm != nullptr) return rccl_reduce_scatter(ctx, send, recv, count);
  LocalGroup &g = *ctx->local;
  const size_t n = count * (size_t)g.world;
  std::vector<double> mine(n), out(count, 0.0);
  MLFF_HIP(ctx, hipMemcpyAsync(mine.data(), send, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
  MLFF_HIP(ctx, hipStreamSynchronize(ctx->stream));
  LOCAL_BARRIER(ctx, g);
  if (ctx->rank == 0) g.buf.assign((size_t)g.world * n, 0.0);
  LOCAL_BARRIER(ctx, g);
  std::memcpy(g.buf.data() + (size_t)ctx->rank * n, mine.data(), sizeof(double) * n);
  LOCAL_BARRIER(ctx, g);
  for (int r = 0; r < g.world; ++r)
    for (size_t i = 0; i < count; ++i) out[i] += g.buf[(size_t)r * n + (size_t)ctx->rank * count + i];
  LOCAL_BARRIER(ctx, g);
  MLFF_HIP(ctx, hipMemcpyAsync(recv, out.data(), sizeof(double) * count, hipMemcpyHostToDevice, ctx->stream));
  MLFF_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MLFF_OK;
}

}  // namespace mlff

namespace {

int ensure_matrix(mlff_ctx *ctx) {
  if (ctx->K == nullptr) MLFF_HIP(ctx, ctx->K.alloc(ctx->blk * ctx->ld));
  return MLFF_OK;
}

void rbf_free(mlff_ctx *ctx) {
  ctx->rbf = RbfData();
  ctx->sym.gen = false;  // tiles generated from these points stay valid, but are only streamed
  ctx->sym.gsrc = SymGen{};
}

// the dense rows of the RBF source, generated on first use (DENSE storage, the masked
// eigen build); the symmetric tiles and every column access go without them
int ensure_rows(mlff_ctx *ctx) {
  if (ctx->has_matrix || !ctx->rbf.ready) return MLFF_OK;
  MLFF_TRY(ensure_matrix(ctx));
  if (ctx->blk > ctx->nrows)  // zero padding rows
    MLFF_HIP(ctx, hipMemsetAsync(ctx->K + ctx->nrows * ctx->ld, 0,
                                 sizeof(double) * (ctx->blk - ctx->nrows) * ctx->ld, ctx->stream));
  if (ctx->nrows > 0)
    launch_gen_rbf(ctx->K, ctx->ld, ctx->nrows, ctx->row0, ctx->rows_per, ctx->blk, ctx->N,
                   ctx->rbf.Xs, ctx->rbf.d, ctx->rbf.jitter, ctx->stream);
  MLFF_HIP(ctx, hipGetLastError());
  MLFF_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ctx->has_matrix = true;
  return MLFF_OK;
}

// scatter a global host vector (N) into a padded device vector (ld)
int scatter_global(mlff_ctx *ctx, const double *v, double *dev_full) {
  MLFF_HIP(ctx, hipMemsetAsync(dev_full, 0, sizeof(double) * ctx->ld, ctx->stream));
  for (int r = 0; r < ctx->world; ++r) {
    const int64_t g0 = (int64_t)r * ctx->rows_per;
    if (g0 >= ctx->N) break;
    const int64_t cnt = std::min<int64_t>(ctx->rows_per, ctx->N - g0);
    MLFF_HIP(ctx, hipMemcpyAsync(dev_full + (int64_t)r * ctx->blk, v + g0, sizeof(double) * cnt,
                                 hipMemcpyHostToDevice, ctx->stream));
  }
  return MLFF_OK;
}

// Opens a preconditioner build: none until it commits (LowRank::commit); the zeroed panel with
// its k, the apply's buffers for k rows and the apply's form.
int alloc_panel(mlff_ctx *ctx, int64_t k) {
  LowRank &lr = ctx->lr;
  lr.kind = MLFF_PRECON_NONE;
  lr.k = 0;
  lr.tpart_base.reset();
  lr.tpart = nullptr;
  lr.drop_speculative_t();
  MLFF_HIP(ctx, lr.T.alloc(round_up(k, 8) * ctx->blk));
  lr.k = k;
  MLFF_HIP(ctx, hipMemsetAsync(lr.T, 0, sizeof(double) * round_up(k, 8) * ctx->blk, ctx->stream));
  lr.tsplit = choose_tsplit(k, ctx->blk);
  if (const char *e = std::getenv("MLFF_TSPLIT")) lr.tsplit = std::max(1, std::atoi(e));  // sweeps
  MLFF_HIP(ctx, lr.tpart_base.alloc(kVecGrid + k * lr.tsplit));
  lr.tpart = lr.tpart_base + kVecGrid;
  lr.zsplit = choose_zsplit(k, ctx->blk);
  if (const char *e = std::getenv("MLFF_ZSPLIT"))  // sweeps
    lr.zsplit = (int)std::min<int64_t>(std::max(1, std::atoi(e)), (k + 15) / 16);
  MLFF_HIP(ctx, lr.zpart.alloc(lr.zsplit * ctx->blk));
  // one rank, rows that fit a workgroup's registers: the one-pass apply (at >= 7 rows per
  // workgroup its G partial vectors are <= 2/7 of a panel pass) from k = 768, and at any k on
  // short rows (N_loc <= 4096), where the launches it saves dominate the step: ethanol M = 111
  // (N = 2997), k = 50 / 150 / 398: PCG step 33.7 / 33.2 / 35.3 -> 29.5 / 29.5 / 30.1 us; M = 23
  // (N = 621), k = 30 / 132: 30.2 / 30.2 -> 28.7 / 28.4 us; at N = 15741, k = 300 the step is
  // the same either way (52.3 / 52.0 us), and k = 554 keeps the two-pass order its golden
  // fixture's crossings were measured with (profiles/r05/lr_small/).  MLFF_LR_ROWS=0 / 1
  // forces the two-pass / one-pass apply (A/B, tests)
  lr.gpart.reset();
  lr.slots.reset();
  lr.fault.reset();
  lr.form = LowRank::kTwoPass;
  const char *lr_env = std::getenv("MLFF_LR_ROWS");
  const bool lr_on = lr_env == nullptr || std::atoi(lr_env) != 0;
  if (ctx->world == 1 && lr_rows_fits(ctx->blk) && (lr_env ? lr_on : (k >= 768 || ctx->blk <= 4096))) {
    lr.form = LowRank::kRows;
  } else if (ctx->world == 1 && lr_on && lr_cluster_fits(ctx->blk)) {
    // longer rows: clusters of workgroups share a row (lr_cluster_count of them resident);
    // worth it from ~4 rows per cluster (the Q partial vectors against the second pass)
    lr.q = lr_cluster_count(ctx->blk, ctx->device);
    if (const char *e = std::getenv("MLFF_LR_CLUSTERS"))  // A/B: fewer clusters
      lr.q = std::min(lr.q, std::max(1, std::atoi(e)));
    if (lr.q >= 1 && k >= 4 * (int64_t)lr.q) lr.form = LowRank::kCluster;
  }
  if (lr.form == LowRank::kRows)
    MLFF_HIP(ctx, lr.gpart.alloc(lr_rows_groups(k) * ctx->blk));
  if (lr.form == LowRank::kCluster) {
    const size_t ns = (size_t)k * lr_cluster_members(ctx->blk) * 2;
    MLFF_HIP(ctx, lr.gpart.alloc(lr.q * ctx->blk));
    MLFF_HIP(ctx, lr.slots.alloc((int64_t)ns));
    MLFF_HIP(ctx, hipMemsetAsync(lr.slots, 0, sizeof(unsigned long long) * ns, ctx->stream));
    MLFF_HIP(ctx, lr.fault.alloc(1));
    MLFF_HIP(ctx, hipMemsetAsync(lr.fault, 0, sizeof(int), ctx->stream));
    lr.epoch = 0;
  }
  return MLFF_OK;
}

// _cho_factor_stable (iterative_solver.py:555-583; :584-618 are unreachable after `if True:`):
// lo_eig = the smallest eigenvalue of M (eigh of the lower triangle, :577 -- here the
// device tridiagonalisation + Sturm bisection of kernels_syev.hip), M += (+1e-15 if lo_eig
// <= 0 else -1e-15) I (:578-579), then the Cholesky factor (:580-582; LinAlgError when it
// fails).  A (k x k, device) is overwritten with the lower factor; lo_eig_out: the value used.
//
// Inside the builds (lo_eig_out == nullptr) the downward shift is tried first: when M - 1e-15 I
// factors, M's smallest eigenvalue is above 1e-15 (to the factorisation's backward error), so
// the reference takes the lo_eig > 0 branch and factors this same matrix -- the same factor,
// without the eigenvalue (whose tridiagonalisation is most of a Nystrom build: 2 x 5.3 s of 13 s
// at k = 14670, profiles/r04/syev/).  Otherwise (lo_eig at or below 1e-15, where the sign
// decides) the eigenvalue path runs as before.  MLFF_CHO_FAST=0 (read at context creation):
// always the eigenvalue path.
int cho_factor_stable(mlff_ctx *ctx, double *A, int64_t k, double *lo_eig_out,
                      double *shift_out = nullptr) {
  if (shift_out) *shift_out = -1e-15;
  if (lo_eig_out == nullptr && ctx->cho_fast) {
    ScratchScope scope(ctx);
    double *B = nullptr;
    MLFF_TRY(scratch_alloc(ctx, &B, (size_t)(k * k)));
    MLFF_HIP(ctx, hipMemcpyAsync(B, A, sizeof(double) * k * k, hipMemcpyDeviceToDevice, ctx->stream));
    launch_add_diag(B, k, -1e-15, ctx->stream);
    bool ok = false;
    MLFF_TRY(potrf_lower(ctx, B, k, &ok));
    if (ok) {
      MLFF_HIP(ctx, hipMemcpyAsync(A, B, sizeof(double) * k * k, hipMemcpyDeviceToDevice, ctx->stream));
      ctx->last_lo_eig = std::numeric_limits<double>::quiet_NaN();  // above 1e-15, not computed
      return MLFF_OK;
    }
  }
  double lo = 0.0;
  std::vector<double> d((size_t)k), e((size_t)(k > 1 ? k - 1 : 0));
  MLFF_TRY(sym_min_eig(ctx, A, k, &lo, d.data(), e.data()));
  // |lo| <= 2 eps ||M|| (||M|| bounded by Gershgorin on the tridiagonal, which is similar to M):
  // eigh's own rounding (~eps ||M||, tests/golden/cho_stable_ethanol.npz delta = 0) decides the
  // sign there, so the device's sign may differ from LAPACK's.  When such a lo > 0 makes the
  // downward shift fail, the upward one the reference takes for lo <= 0 is tried before
  // LinAlgError.  (The fixture's lo = 1.26e-16 at ||M|| ~ 0.03 is 20x above the bound and still
  // raises like the reference.)  MLFF_CHO_TEST_NOISY_POSITIVE=1: a noisy lo is taken as > 0
  // (the test of this retry; never set in production).
  double gersh = 0.0;
  for (int64_t i = 0; i < k; ++i)
    gersh = std::max(gersh, std::fabs(d[i]) + (i > 0 ? std::fabs(e[i - 1]) : 0.0) +
                                (i + 1 < k ? std::fabs(e[i]) : 0.0));
  const bool noisy = std::fabs(lo) <= 2.0 * std::numeric_limits<double>::epsilon() * gersh;
  if (noisy && lo <= 0.0) {
    const char *t = std::getenv("MLFF_CHO_TEST_NOISY_POSITIVE");
    if (t != nullptr && std::atoi(t) == 1) lo = std::fabs(lo) > 0.0 ? std::fabs(lo) : 1e-300;
  }
  ctx->last_lo_eig = lo;
  if (lo_eig_out) *lo_eig_out = lo;
  if (!(noisy && lo > 0.0)) {
    launch_add_diag(A, k, lo <= 0.0 ? 1e-15 : -1e-15, ctx->stream);
    if (shift_out) *shift_out = lo <= 0.0 ? 1e-15 : -1e-15;
    return potrf_lower(ctx, A, k);
  }
  ScratchScope scope(ctx);
  double *keep = nullptr;
  MLFF_TRY(scratch_alloc(ctx, &keep, (size_t)(k * k)));
  MLFF_HIP(ctx, hipMemcpyAsync(keep, A, sizeof(double) * k * k, hipMemcpyDeviceToDevice, ctx->stream));
  launch_add_diag(A, k, -1e-15, ctx->stream);
  bool ok = false;
  MLFF_TRY(potrf_lower(ctx, A, k, &ok));
  if (ok) return MLFF_OK;
  MLFF_HIP(ctx, hipMemcpyAsync(A, keep, sizeof(double) * k * k, hipMemcpyDeviceToDevice, ctx->stream));
  launch_add_diag(A, k, 1e-15, ctx->stream);
  if (shift_out) *shift_out = 1e-15;
  ctx->cho_flipped = true;
  return potrf_lower(ctx, A, k);
}

// Woodbury panel from a wide factor W = L^T (k x blk) in place:
//   G = lam I + W W^T; L2 = chol(G); W <- L2^-1 W   (iterative_cholesky.py:141-143)
//
// ctx->wb_refine (MLFF_WB_REFINE): W is the top block of Q1 = A R1^-1, A = [L; sqrt(lam) I],
// R1 = L2^T -- one CholeskyQR step.  A second step re-orthogonalises it: G2 = Q1^T Q1 =
// W W^T + lam L2^-1 L2^-T (= I in exact arithmetic, so the preconditioner is unchanged),
// C C^T = G2, W <- C^-1 W.  At lam = 1e-10 the PCG count depends on how accurately the
// Woodbury apply's r - W^T W r cancels (DESIGN.md 2, configs[1] at full size).
// The second CholeskyQR step of a panel W = L2^-1 X^T (k x blk, this rank's columns) built
// from L2 L2^T = X^T X + mu I: W is the top block of Q1 = [X; sqrt(mu) I] L2^-T, so
// G2 = Q1^T Q1 = W W^T + mu L2^-1 L2^-T (= I in exact arithmetic), C C^T = G2, W <- C^-1 W.
// L2: the lower factor (k x k, the same on every rank).
// steps > 1 (MLFF_WB_REFINE=<steps>): CholeskyQR3 and beyond -- step s uses the accumulated
// factor (L2 C_1 ... C_{s-1}), whose inverse is C_{s-1}^-1 ... C_1^-1 L2^-1 (Li updated by one
// k x k triangular solve per step)
int reorthogonalise_panel(mlff_ctx *ctx, double *W, const double *L2, int64_t k, double mu,
                          int steps = 1) {
  ScratchScope scope(ctx);
  hipStream_t s = ctx->stream;
  double *Li = nullptr, *G2 = nullptr;
  MLFF_TRY(scratch_alloc(ctx, &Li, k * k));
  MLFF_TRY(scratch_alloc(ctx, &G2, k * k));
  MLFF_HIP(ctx, hipMemsetAsync(Li, 0, sizeof(double) * k * k, s));
  launch_add_diag(Li, k, 1.0, s);
  MLFF_TRY(trsm_lower_wide(ctx, L2, k, Li, k, k));  // Li = L2^-1
  for (int st = 0; st < steps; ++st) {
    if (ctx->wb_gram_dd)
      MLFF_TRY(gram_wide_dd(ctx, W, k, ctx->blk, ctx->blk, G2, ctx->wb_gram_dd == 2));
    else
      MLFF_TRY(syrk_wide(ctx, W, k, ctx->blk, ctx->blk, G2));
    MLFF_TRY(comm_allreduce(ctx, G2, (size_t)(k * k)));
    launch_gemm(false, true, k, k, k, mu, Li, k, Li, k, 1.0, G2, k, s);  // + mu Li Li^T
    MLFF_TRY(potrf_lower(ctx, G2, k));
    MLFF_TRY(trsm_lower_wide(ctx, G2, k, W, ctx->blk, ctx->blk));
    if (st + 1 < steps) MLFF_TRY(trsm_lower_wide(ctx, G2, k, Li, k, k));  // Li <- C^-1 Li
  }
  return MLFF_OK;
}

int woodbury_inplace(mlff_ctx *ctx, double *W, int64_t k) {
  ScratchScope scope(ctx);
  hipStream_t s = ctx->stream;
  double *G = nullptr;
  MLFF_TRY(scratch_alloc(ctx, &G, k * k));
  if (ctx->wb_gram_dd)  // L^T L rounded once per entry (DESIGN.md 2, configs[1])
    MLFF_TRY(gram_wide_dd(ctx, W, k, ctx->blk, ctx->blk, G, ctx->wb_gram_dd == 2));
  else
    MLFF_TRY(syrk_wide(ctx, W, k, ctx->blk, ctx->blk, G));
  MLFF_TRY(comm_allreduce(ctx, G, (size_t)(k * k)));
  launch_add_diag(G, k, ctx->lam, s);
  MLFF_TRY(potrf_lower(ctx, G, k));
  MLFF_TRY(trsm_lower_wide(ctx, G, k, W, ctx->blk, ctx->blk));
  if (ctx->wb_refine > 0) MLFF_TRY(reorthogonalise_panel(ctx, W, G, k, ctx->lam, ctx->wb_refine));
  MLFF_HIP(ctx, hipStreamSynchronize(s));
  return MLFF_OK;
}

__global__ void k_unit_idx(double *__restrict__ x, const int64_t *__restrict__ idx, int64_t j,
                           int64_t rows_per, int64_t blk, double val) {
  if (threadIdx.x == 0) {
    const int64_t g = idx[j];
    x[(g / rows_per) * blk + g % rows_per] = val;
  }
}

// W[j, i] = (sigma_K K)[row0 + i, idx_j] for the local rows: a gather from the
// dense rows, evaluated from the RBF points, or from the matrix-free sGDML operator (the
// reference's own column access, K_op.matvec(e_i), iterative_cholesky.py:152-156)
int fetch_cols(mlff_ctx *ctx, const int64_t *didx, int64_t k, double *W, int64_t ldw) {
  hipStream_t s = ctx->stream;
  if (ctx->has_matrix) {
    launch_gather_cols(ctx->K, ctx->ld, ctx->nrows, didx, k, ctx->rows_per, ctx->blk, ctx->sigma_K,
                       W, ldw, s);
    MLFF_HIP(ctx, hipGetLastError());
    return MLFF_OK;
  }
  if (ctx->rbf.ready) {
    launch_rbf_cols(ctx->rbf, ctx->N, ctx->row0, ctx->nrows, didx, k, nullptr, ctx->sigma_K, W, ldw, s);
    MLFF_HIP(ctx, hipGetLastError());
    return MLFF_OK;
  }
  if (!ctx->mf.ready) return set_error(ctx, MLFF_ERR_STATE, "no kernel matrix / operator set");
  if (mf_columns(ctx, didx, k, ctx->sigma_K, W, ldw)) {  // single-column path, one launch
    MLFF_HIP(ctx, hipGetLastError());
    return MLFF_OK;
  }
  MLFF_HIP(ctx, hipMemsetAsync(ctx->xg, 0, sizeof(double) * ctx->ld, s));
  for (int64_t j = 0; j < k; ++j) {
    hipLaunchKernelGGL(k_unit_idx, dim3(1), dim3(64), 0, s, ctx->xg, didx, j, ctx->rows_per,
                       ctx->blk, 1.0);
    launch_mf_operator(ctx, ctx->xg, W + j * ldw, nullptr, nullptr, ctx->sigma_K, 0.0);
    hipLaunchKernelGGL(k_unit_idx, dim3(1), dim3(64), 0, s, ctx->xg, didx, j, ctx->rows_per,
                       ctx->blk, 0.0);
    if ((j & 255) == 255) MLFF_HIP(ctx, hipGetLastError());
  }
  MLFF_HIP(ctx, hipGetLastError());
  return MLFF_OK;
}

// Nystrom panel (iterative_solver.py:112-283 for variant 0, :343-374 for variant 1,
// :489-550 for the leverage scores which follow variant 0).  W: k x blk, zeroed.
int nystrom_panel(mlff_ctx *ctx, const int64_t *idx_host, int64_t k, int variant, double lam,
                  double *W) {
  hipStream_t s = ctx->stream;
  ScratchScope scope(ctx);
  int64_t *didx = nullptr;
  double *Smm = nullptr, *G = nullptr;
  MLFF_TRY(scratch_alloc(ctx, &didx, k));
  MLFF_TRY(scratch_alloc(ctx, &Smm, k * k));
  MLFF_TRY(scratch_alloc(ctx, &G, k * k));
  MLFF_HIP(ctx, hipMemcpyAsync(didx, idx_host, sizeof(int64_t) * k, hipMemcpyHostToDevice, s));
  // K_nm^T (sign convention S = sigma_K K; sign flips cancel in B^T B)
  MLFF_TRY(fetch_cols(ctx, didx, k, W, ctx->blk));
  launch_gather_mm(W, ctx->blk, didx, k, ctx->row0, ctx->nrows, Smm, s);
  MLFF_TRY(comm_allreduce(ctx, Smm, (size_t)(k * k)));
  int rc;
  if (variant == 0) {
    rc = cho_factor_stable(ctx, Smm, k, nullptr);  // U^T U = -K_mm (+-1e-15)
  } else {
    launch_add_diag(Smm, k, 1e-16, s);            // cholesky(K_mm + 1e-16 I, lower=True)
    rc = potrf_lower(ctx, Smm, k);
  }
  if (rc != MLFF_OK) return rc;
  MLFF_TRY(trsm_lower_wide(ctx, Smm, k, W, ctx->blk, ctx->blk));   // C^T = U^-T K_nm^T
  MLFF_TRY(syrk_wide(ctx, W, k, ctx->blk, ctx->blk, G));           // C^T C
  MLFF_TRY(comm_allreduce(ctx, G, (size_t)(k * k)));
  launch_add_diag(G, k, lam, s);
  double shift = 0.0;
  if (variant == 0)
    rc = cho_factor_stable(ctx, G, k, nullptr, &shift);
  else
    rc = potrf_lower(ctx, G, k);
  if (rc != MLFF_OK) return rc;
  MLFF_TRY(trsm_lower_wide(ctx, G, k, W, ctx->blk, ctx->blk));     // B = V^-T C^T
  // B is the top block of [C; sqrt(lam + shift) I] V^-T: the same second CholeskyQR step as
  // the Woodbury panel (MLFF_NYS_REFINE)
  if (ctx->nys_refine) MLFF_TRY(reorthogonalise_panel(ctx, W, G, k, lam + shift));
  MLFF_HIP(ctx, hipStreamSynchronize(s));
  return MLFF_OK;
}

int check_idx(mlff_ctx *ctx, const int64_t *idx, int64_t k) {
  if (idx == nullptr || k < 1 || k > ctx->N) return set_error(ctx, MLFF_ERR_ARG, "bad column index set");
  for (int64_t j = 0; j < k; ++j) {
    if (idx[j] < 0 || idx[j] >= ctx->N) return set_error(ctx, MLFF_ERR_ARG, "column index out of range");
    if (j > 0 && idx[j] <= idx[j - 1])
      return set_error(ctx, MLFF_ERR_ARG, "column indices must be sorted and unique (train.py:1197-1201)");
  }
  return MLFF_OK;
}

// preconditioner builds read columns of the dense K
int require_matrix(mlff_ctx *ctx) {
  MLFF_TRY(require_operator(ctx));
  MLFF_TRY(ensure_rows(ctx));
  if (!ctx->has_matrix)
    return set_error(ctx, MLFF_ERR_STATE,
                     "this build needs the dense kernel matrix (assemble it first)");
  return MLFF_OK;
}

}  // namespace

// gather the rank blocks of an ld-long padded vector (in place)
int mlff::allgather_blocks(mlff_ctx *ctx, double *full) {
  if (ctx->world > 1)
    return comm_allgather(ctx, full + ctx->rank * ctx->blk, full, (size_t)ctx->blk);
  return MLFF_OK;
}

// the operator needs K (dense rows), the RBF points or the matrix-free sGDML data
int mlff::require_operator(mlff_ctx *ctx) {
  if (!ctx->has_matrix && !ctx->mf.ready && !ctx->rbf.ready)
    return set_error(ctx, MLFF_ERR_STATE, "no kernel matrix / operator set");
  if (!ctx->has_operator) return set_error(ctx, MLFF_ERR_STATE, "mlff_set_operator not called");
  return MLFF_OK;
}

// Decide the operator storage (mlff_set_storage) and build the symmetric tiles
// if they are to be used and not current.
int mlff::resolve_storage(mlff_ctx *ctx) {
  ctx->use_mf = false;
  if (ctx->exact_sums) {
    // the exact-sum anchor (kernels_dd.hip) is a dense-row operator on one rank: refused for
    // every other storage before any of them is chosen, so the fused matrix-free iteration
    // (which moves the x / r update into the next apply) can never run beside its apply
    if (ctx->world > 1 || ctx->storage == MLFF_STORAGE_MATFREE ||
        ctx->storage == MLFF_STORAGE_SYMTILE || (!ctx->has_matrix && !ctx->rbf.ready))
      return set_error(ctx, MLFF_ERR_STATE,
                       "MLFF_EXACT_SUMS: dense-row storage (a matrix or RBF points) on one rank only");
    MLFF_TRY(ensure_rows(ctx));
    ctx->use_sym = false;
    return MLFF_OK;
  }
  if (ctx->storage == MLFF_STORAGE_MATFREE) {
    if (!ctx->mf.ready)
      return set_error(ctx, MLFF_ERR_STATE, "MLFF_STORAGE_MATFREE needs mlff_sgdml_operator / mlff_assemble_sgdml");
    ctx->use_sym = false;
    ctx->use_mf = true;
    return MLFF_OK;
  }
  if (!ctx->has_matrix && !ctx->rbf.ready) {  // only the matrix-free operator exists
    ctx->use_sym = false;
    ctx->use_mf = true;
    return MLFF_OK;
  }
  if (ctx->storage == MLFF_STORAGE_AUTO && ctx->mf.ready) {
    // the matrix-free operator or the stored K (tiles, rows): whichever the time model of
    // the measured rates (mf_seconds) puts first for this rank's share
    const double Np = (double)round_up(ctx->ld, kSymTile);
    const double t_tiles = 10e-6 + 4.0 * Np * Np / ctx->world / 6.9e12;  // 2 launches + stream
    double t_mf = mf_seconds(ctx);
    if (ctx->world > 1) {
      // one decision for all ranks (each models its own share; the slowest rank paces the
      // iteration): the modelled times are all-reduced as a world-long vector and every rank
      // takes the same maximum -- ranks that chose differently would run mismatched collectives
      if (ctx->world > kMaxPart) return set_error(ctx, MLFF_ERR_ARG, "world too large");
      std::vector<double> t(ctx->world, 0.0);
      t[ctx->rank] = t_mf;
      double *buf = ctx->part + 3 * kMaxPart;
      MLFF_HIP(ctx, hipMemcpyAsync(buf, t.data(), sizeof(double) * ctx->world, hipMemcpyHostToDevice,
                                   ctx->stream));
      MLFF_TRY(comm_allreduce(ctx, buf, ctx->world));
      MLFF_HIP(ctx, hipMemcpyAsync(t.data(), buf, sizeof(double) * ctx->world, hipMemcpyDeviceToHost,
                                   ctx->stream));
      MLFF_HIP(ctx, hipStreamSynchronize(ctx->stream));
      t_mf = *std::max_element(t.begin(), t.end());
    }
    if (t_mf < t_tiles) {
      ctx->use_sym = false;
      ctx->use_mf = true;
      return MLFF_OK;
    }
  }
  if (ctx->storage == MLFF_STORAGE_DENSE) {
    MLFF_TRY(ensure_rows(ctx));
    ctx->use_sym = false;
    return MLFF_OK;
  }
  if (ctx->sym.ready) {
    ctx->use_sym = true;
    return MLFF_OK;
  }
  if (!ctx->has_matrix) {  // RBF source: the tiles are generated from the points
    bool symmetric = true;
    MLFF_TRY(sym_build(ctx, false, &symmetric));
    ctx->use_sym = true;
    return MLFF_OK;
  }
  const bool explicit_sym = ctx->storage == MLFF_STORAGE_SYMTILE;
  if (ctx->world > 1 && !ctx->K_symmetric && !explicit_sym) {
    ctx->use_sym = false;  // a sharded host matrix cannot be checked locally
    return MLFF_OK;
  }
  const bool check = !ctx->K_symmetric && ctx->world == 1;
  bool symmetric = true;
  int rc = sym_build(ctx, check, &symmetric);
  if (ctx->world > 1) {
    // every rank must take the same path (the tiled operator has a collective)
    const double fail_here = (rc != MLFF_OK || !symmetric) ? 1.0 : 0.0;
    double *flag = ctx->part + 3 * kMaxPart;
    MLFF_HIP(ctx, hipMemcpyAsync(flag, &fail_here, sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    MLFF_TRY(comm_allreduce(ctx, flag, 1));
    double fails = 0.0;
    MLFF_HIP(ctx, hipMemcpyAsync(&fails, flag, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    MLFF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (fails > 0.0 && rc == MLFF_OK) symmetric = false;
  }
  if (rc != MLFF_OK || !symmetric) {
    ctx->sym = SymPack{};
    (void)hipGetLastError();
    ctx->use_sym = false;
    if (explicit_sym) {
      if (rc != MLFF_OK) return rc;
      return set_error(ctx, MLFF_ERR_ARG, "MLFF_STORAGE_SYMTILE: K is not symmetric");
    }
    ctx->err.clear();
    return MLFF_OK;  // AUTO: dense row GEMV
  }
  ctx->use_sym = true;
  return MLFF_OK;
}

// y_loc = sigma_K K v_full + lam v_loc over this rank's rows (status gated).
// pq_part: also the v_loc . y_loc partials of the CG step (kVecGrid, k_dot_part's layout;
// fused into the last operator kernel where it can be)
int mlff::launch_operator(mlff_ctx *ctx, const double *v_full, double *y_loc, const double *v_loc,
                          const int *status, double *pq_part, const PFuse *pf) {
  hipStream_t s = ctx->stream;
  if (ctx->exact_sums) {  // measurement anchor (kernels_dd.hip): dense rows, one rank
    if (ctx->use_mf || ctx->use_sym || ctx->world > 1)
      return set_error(ctx, MLFF_ERR_STATE, "MLFF_EXACT_SUMS: dense-row storage on one rank only");
    launch_dd_gemv_rows(ctx->K, ctx->ld, ctx->nrows, ctx->N, v_full, y_loc, ctx->sigma_K, ctx->lam,
                        v_loc, status, s);
    if (pq_part != nullptr) launch_dot_part(v_loc, y_loc, ctx->nrows, pq_part, status, s);
    return MLFF_OK;
  }
  if (ctx->use_mf) {
    launch_mf_operator(ctx, v_full, y_loc, v_loc, status, ctx->sigma_K, ctx->lam, pq_part, pf);
    return MLFF_OK;
  }
  if (!ctx->use_sym) {
    launch_gemv_rows(ctx->K, ctx->ld, ctx->nrows, v_full, y_loc, ctx->sigma_K, ctx->lam, v_loc,
                     status, s);
    if (pq_part != nullptr) launch_dot_part(v_loc, y_loc, ctx->nrows, pq_part, status, s);
    return MLFF_OK;
  }
  if (pq_part != nullptr) return set_error(ctx, MLFF_ERR_STATE, "launch_operator: pq with tiles");
  SymPack &sp = ctx->sym;
  launch_symv(sp, v_full, sp.P, status, s);
  if (ctx->world == 1) {
    launch_sym_reduce(sp, ctx->nrows, y_loc, true, ctx->sigma_K, ctx->lam, v_loc, status, s);
    return MLFF_OK;
  }
  launch_sym_reduce_ranks(sp, ctx->rank, ctx->world, ctx->blk, nullptr, nullptr, nullptr, 0.0, 0.0,
                          status, s);
  MLFF_TRY(comm_reduce_scatter(ctx, sp.yg, sp.yr, (size_t)sp.ystride));
  launch_axpby_loc(sp.yr, y_loc, ctx->nrows, ctx->sigma_K, ctx->lam, v_loc, status, s);
  return MLFF_OK;
}

// y_loc = S x = sigma_K K x (no ridge) for this rank's rows, x given as this rank's block
// of a distributed vector (blk entries, zero padded): the block is all-gathered into the
// operand xg first (one collective).  resolve_storage must have run.  Stream ordered.
int mlff::operator_apply_local(mlff_ctx *ctx, const double *x_loc, double *y_loc) {
  MLFF_HIP(ctx, hipMemcpyAsync(ctx->xg + (int64_t)ctx->rank * ctx->blk, x_loc,
                               sizeof(double) * ctx->blk, hipMemcpyDeviceToDevice, ctx->stream));
  MLFF_TRY(allgather_blocks(ctx, ctx->xg));
  return launch_operator(ctx, ctx->xg, y_loc, nullptr, nullptr);
}

int mlff::operator_prepare(mlff_ctx *ctx) {
  MLFF_TRY(require_operator(ctx));
  return resolve_storage(ctx);
}

int mlff::operator_diag(mlff_ctx *ctx, double *out) {
  if (ctx->has_matrix) {
    launch_diag_of(ctx->K, ctx->ld, ctx->nrows, ctx->row0, ctx->rows_per, ctx->blk, ctx->sigma_K,
                   out, ctx->stream);
    MLFF_HIP(ctx, hipGetLastError());
    return MLFF_OK;
  }
  if (ctx->rbf.ready) {  // K[i, i] = 1 + jitter
    launch_fill(out, ctx->nrows, ctx->sigma_K * (1.0 + ctx->rbf.jitter), ctx->stream);
    MLFF_HIP(ctx, hipGetLastError());
    return MLFF_OK;
  }
  if (!ctx->mf.ready) return set_error(ctx, MLFF_ERR_STATE, "no kernel matrix / operator set");
  return mf_diag(ctx, out);
}

namespace {

double operator_bytes(const mlff_ctx *ctx) {
  if (ctx->use_mf) return mf_bytes(ctx);
  if (ctx->use_sym) {
    // tiles streamed: all of them, or -- with a generating role (SymPack::gen) -- the whole
    // tiles [0, n_s) and the quarter units unless all of those are generated; quarter units
    // shared by the two roles count as streamed (an upper bound, by less than the resident
    // workgroups' worth of quarter tiles)
    const SymPack &sp = ctx->sym;
    double tiles = (double)sp.ntiles;
    if (sp.gen)
      tiles = (double)sp.gsrc.n_s + (sp.gsrc.qmode == 2 ? 0.0 : (double)(sp.ntiles - sp.nwhole));
    return 8.0 * tiles * kSymTile * kSymTile + 16.0 * (double)ctx->nrows;
  }
  return 8.0 * (double)ctx->nrows * (double)ctx->N + 16.0 * (double)ctx->nrows;
}

}  // namespace

extern "C" {

int mlff_version(void) { return 100; }

int mlff_device_count(int *n_out) {
  MLFF_API_BEGIN
  if (n_out == nullptr) return set_error(nullptr, MLFF_ERR_ARG, "null pointer");
  int n = 0;
  const hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    *n_out = 0;
    return hip_check(nullptr, e, "hipGetDeviceCount");
  }
  *n_out = n;
  return MLFF_OK;
  MLFF_API_END(nullptr)
}

int mlff_comm_unique_id(unsigned char id_out[128]) {
  MLFF_API_BEGIN
  if (id_out == nullptr) return set_error(nullptr, MLFF_ERR_ARG, "null pointer");
  ncclUniqueId id;
  MLFF_NCCL(nullptr, ncclGetUniqueId(&id));
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
  std::memcpy(id_out, &id, 128);
  return MLFF_OK;
  MLFF_API_END(nullptr)
}

int mlff_comm_selftest(int device, int64_t count, double *max_err_out) {
  MLFF_API_BEGIN
  if (max_err_out == nullptr || count < 1) return set_error(nullptr, MLFF_ERR_ARG, "bad arguments");
  *max_err_out = -1.0;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
    return set_error(nullptr, MLFF_ERR_ARG, "bad device id");
  // every exit (error returns of the MLFF_HIP checks, exceptions caught by MLFF_API_END)
  // releases the buffers, the communicator, the stream and the context
  struct Owned {
    mlff_ctx *ctx = new mlff_ctx();
    ~Owned() { mlff_ctx_destroy(ctx); }
  } own;
  DevBuf<double> a, b;  // declared after the context: released before it
  mlff_ctx *ctx = own.ctx;
  ctx->device = device;
  ctx->rank = 0;
  ctx->world = 1;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&ctx->stream.h, hipStreamNonBlocking) != hipSuccess)
    return set_error(nullptr, MLFF_ERR_HIP, "stream create failed");
  ncclUniqueId id;
  ncclResult_t e = ncclGetUniqueId(&id);
  if (e == ncclSuccess) e = ncclCommInitRank(&ctx->comm.h, 1, id, 0);
  if (e != ncclSuccess) {
    ctx->comm.h = nullptr;
    return set_error(nullptr, MLFF_ERR_COMM, std::string("ncclCommInitRank: ") + ncclGetErrorString(e));
  }
  const size_t n = (size_t)count;
  if (a.alloc(count) != hipSuccess || b.alloc(count) != hipSuccess)
    return set_error(nullptr, MLFF_ERR_NOMEM, "device allocation failed");
  std::vector<double> h(n);
  double worst = 0.0;
  // every collective sits between a producing kernel and a consuming copy on the same stream
  // (no host synchronisation in between), so a transport that ran off-stream would read the
  // input before it is written or leave the poisoned output in place
  auto check = [&](const double *src, double scale) -> int {
    MLFF_HIP(ctx, hipMemcpyAsync(h.data(), src, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
    MLFF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < n; ++i) {
      const double d = std::fabs(h[i] - scale * (1.0 + 0.5 * (double)i));
      worst = std::isfinite(d) ? std::max(worst, d) : INFINITY;
    }
    return MLFF_OK;
  };
  auto fill = [&](double *p, double scale) {
    hipLaunchKernelGGL(k_selftest_fill, dim3(256), dim3(256), 0, ctx->stream, p, n, scale);
  };
  auto poison = [&](double *p) { return hipMemsetAsync(p, 0xff, sizeof(double) * n, ctx->stream); };
  // allreduce in place
  fill(a, 1.0);
  if (int rc = rccl_allreduce(ctx, a, n)) return rc;
  if (int rc = check(a, 1.0)) return rc;
  // allgather out of place, then in place (send == recv + rank * count)
  fill(a, 2.0);
  MLFF_HIP(ctx, poison(b));
  if (int rc = rccl_allgather(ctx, a, b, n)) return rc;
  if (int rc = check(b, 2.0)) return rc;
  fill(b, 3.0);
  if (int rc = rccl_allgather(ctx, b, b, n)) return rc;
  if (int rc = check(b, 3.0)) return rc;
  // reduce-scatter out of place
  fill(b, 4.0);
  MLFF_HIP(ctx, poison(a));
  if (int rc = rccl_reduce_scatter(ctx, b, a, n)) return rc;
  if (int rc = check(a, 4.0)) return rc;
  *max_err_out = worst;
  return MLFF_OK;
  MLFF_API_END(nullptr)
}

const char *mlff_last_error(mlff_ctx *ctx) {
  if (ctx != nullptr) return ctx->err.c_str();
  return g_last_error.c_str();
}

int mlff_ctx_create(int device, int rank, int world, const unsigned char *comm_id,
                    int64_t n_global, mlff_ctx **ctx_out) {
  MLFF_API_BEGIN
  if (ctx_out == nullptr) return set_error(nullptr, MLFF_ERR_ARG, "null ctx_out");
  *ctx_out = nullptr;
  if (world < 1 || rank < 0 || rank >= world) return set_error(nullptr, MLFF_ERR_ARG, "bad rank/world");
  if (n_global < 1) return set_error(nullptr, MLFF_ERR_ARG, "N must be >= 1");
  if (world > 1 && comm_id == nullptr) return set_error(nullptr, MLFF_ERR_ARG, "comm_id required for world > 1");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
    return set_error(nullptr, MLFF_ERR_HIP, "no HIP device available");
  if (device < 0 || device >= ndev) return set_error(nullptr, MLFF_ERR_ARG, "bad device id");
  if (world > 1 && std::getenv("MLFF_EXACT_SUMS") != nullptr && std::atoi(std::getenv("MLFF_EXACT_SUMS")) != 0)
    return set_error(nullptr, MLFF_ERR_ARG, "MLFF_EXACT_SUMS runs on one rank");
  mlff_ctx *ctx = new mlff_ctx();
  ctx->device = device;
  for (auto [name, flag] : {std::pair<const char *, bool *>{"MLFF_FUSE_P", &ctx->fuse_p},
                            std::pair<const char *, bool *>{"MLFF_FUSE_XR", &ctx->fuse_xr},
                            std::pair<const char *, bool *>{"MLFF_CHO_FAST", &ctx->cho_fast}}) {
    const char *e = std::getenv(name);
    *flag = e == nullptr || std::atoi(e) != 0;
  }
  if (const char *e = std::getenv("MLFF_PQ_PUBLISH")) ctx->pq_publish = std::atoi(e) != 0;
  if (const char *e = std::getenv("MLFF_WB_REFINE")) ctx->wb_refine = std::max(0, std::atoi(e));
  if (const char *e = std::getenv("MLFF_NYS_REFINE")) ctx->nys_refine = std::atoi(e) != 0;
  if (const char *e = std::getenv("MLFF_WB_GRAM")) ctx->wb_gram_dd = std::max(0, std::min(2, std::atoi(e)));
  if (const char *e = std::getenv("MLFF_EXACT_SUMS")) ctx->exact_sums = std::atoi(e) != 0;
  ctx->rank = rank;
  ctx->world = world;
  ctx->N = n_global;
  ctx->rows_per = (n_global + world - 1) / world;
  ctx->row0 = std::min<int64_t>((int64_t)rank * ctx->rows_per, n_global);
  ctx->nrows = std::max<int64_t>(0, std::min<int64_t>(ctx->rows_per, n_global - ctx->row0));
  // world > 1: rank blocks hold whole tiles of the symmetric operator
  ctx->blk = round_up(ctx->rows_per, world > 1 ? kSymTile : kPad);
  ctx->ld = (int64_t)world * ctx->blk;
  auto fail = [&](int rc) {
    mlff_ctx_destroy(ctx);
    return rc;
  };
  if (hipSetDevice(device) != hipSuccess) return fail(set_error(nullptr, MLFF_ERR_HIP, "hipSetDevice failed"));
  if (hipStreamCreateWithFlags(&ctx->stream.h, hipStreamNonBlocking) != hipSuccess)
    return fail(set_error(nullptr, MLFF_ERR_HIP, "hipStreamCreate failed"));
  if (world > 1 && std::memcmp(comm_id, "SOLO:", 5) == 0) {
    ctx->solo = true;
  } else if (world > 1 && std::memcmp(comm_id, "LOCAL:", 6) == 0) {
    const std::string key((const char *)comm_id, strnlen((const char *)comm_id, 128));
    ctx->local = join_local_group(key, world);
    if (ctx->local->world != world) return fail(set_error(nullptr, MLFF_ERR_ARG, "LOCAL group size mismatch"));
  } else if (world > 1) {
    ncclUniqueId id;
    std::memcpy(&id, comm_id, 128);
    const ncclResult_t e = ncclCommInitRank(&ctx->comm.h, world, id, rank);
    if (e != ncclSuccess) {
      ctx->comm.h = nullptr;
      return fail(set_error(nullptr, MLFF_ERR_COMM, std::string("ncclCommInitRank: ") + ncclGetErrorString(e)));
    }
  }
  for (DevBuf<double> *v : {&ctx->x, &ctx->r, &ctx->z, &ctx->q, &ctx->b}) {
    if (v->alloc(ctx->blk) != hipSuccess) return fail(set_error(nullptr, MLFF_ERR_NOMEM, "alloc"));
    hipMemset(v->get(), 0, sizeof(double) * ctx->blk);
  }
  // full-length operands are padded to whole tiles (entries >= ld stay zero)
  const int64_t ldp = round_up(ctx->ld, kSymTile);
  if (ctx->p_full.alloc(ldp) != hipSuccess || ctx->xg.alloc(ldp) != hipSuccess ||
      ctx->part.alloc(4 * kMaxPart) != hipSuccess || ctx->st.alloc(1) != hipSuccess ||
      ctx->h_st.alloc(1) != hipSuccess || ctx->dwork.alloc(ctx->blk) != hipSuccess ||
      ctx->pivflag.alloc(ctx->blk) != hipSuccess || ctx->perm.alloc(n_global) != hipSuccess)
    return fail(set_error(nullptr, MLFF_ERR_NOMEM, "device allocation failed"));
  {
    // the gather buffer: z | rho partials per rank (one rank: the fused tile iteration's operand)
    ctx->gstride = ctx->blk + kVecGrid;
    if (ctx->gb.alloc(world * ctx->gstride) != hipSuccess)
      return fail(set_error(nullptr, MLFF_ERR_NOMEM, "device allocation failed"));
    hipMemset(ctx->gb, 0, sizeof(double) * world * ctx->gstride);
  }
  hipMemset(ctx->p_full, 0, sizeof(double) * ldp);
  hipMemset(ctx->xg, 0, sizeof(double) * ldp);
  hipMemset(ctx->part, 0, sizeof(double) * 4 * kMaxPart);
  hipMemset(ctx->st, 0, sizeof(DevState));
  std::memset(ctx->h_st.get(), 0, sizeof(DevState));
  if (hipDeviceSynchronize() != hipSuccess) return fail(set_error(nullptr, MLFF_ERR_HIP, "init sync failed"));
  *ctx_out = ctx;
  return MLFF_OK;
  MLFF_API_END(nullptr)
}

int mlff_ctx_destroy(mlff_ctx *ctx) {
  MLFF_API_BEGIN
  if (ctx == nullptr) return MLFF_OK;
  hipSetDevice(ctx->device);
  if (ctx->stream) hipStreamSynchronize(ctx->stream);
  // the members release themselves in the order mlff_ctx declares (common.h)
  delete ctx;
  return MLFF_OK;
  MLFF_API_END(ctx)
}

int mlff_comm_abort(mlff_ctx *ctx) {
  MLFF_API_BEGIN
  if (ctx == nullptr) return set_error(nullptr, MLFF_ERR_ARG, "null ctx");
  ctx->aborted = true;
  if (ctx->local) ctx->local->abort();
  if (ctx->comm != nullptr) {
    (void)hipSetDevice(ctx->device);
    ncclCommAbort(ctx->comm);
    ctx->comm.h = nullptr;
  }
  return MLFF_OK;
  MLFF_API_END(ctx)
}

int mlff_shard_range(mlff_ctx *ctx, int64_t *row0_out, int64_t *nrows_out) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  if (row0_out) *row0_out = ctx->row0;
  if (nrows_out) *nrows_out = ctx->nrows;
  return MLFF_OK;
  MLFF_API_END(ctx)
}

int mlff_matrix_ld(mlff_ctx *ctx, int64_t *ld_out) {
  MLFF_API_BEGIN
  if (ctx == nullptr || ld_out == nullptr) return set_error(ctx, MLFF_ERR_ARG, "null pointer");
  *ld_out = ctx->ld;
  return MLFF_OK;
  MLFF_API_END(ctx)
}

int mlff_synchronize(mlff_ctx *ctx) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  MLFF_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MLFF_OK;
  MLFF_API_END(ctx)
}

int mlff_stream(mlff_ctx *ctx, void **stream_out) {
  MLFF_API_BEGIN
  if (ctx == nullptr || stream_out == nullptr) return set_error(ctx, MLFF_ERR_ARG, "null pointer");
  *stream_out = (void *)ctx->stream;
  return MLFF_OK;
  MLFF_API_END(ctx)
}

int mlff_set_matrix_host(mlff_ctx *ctx, const double *K_local, int64_t ld_host) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  if (K_local == nullptr && ctx->nrows > 0) return set_error(ctx, MLFF_ERR_ARG, "null K");
  if (ld_host < ctx->N) return set_error(ctx, MLFF_ERR_ARG, "ld_host < N");
  MLFF_TRY(ensure_matrix(ctx));
  MLFF_HIP(ctx, hipMemsetAsync(ctx->K, 0, sizeof(double) * ctx->blk * ctx->ld, ctx->stream));
  for (int r = 0; r < ctx->world && ctx->nrows > 0; ++r) {
    const int64_t g0 = (int64_t)r * ctx->rows_per;
    if (g0 >= ctx->N) break;
    const int64_t cnt = std::min<int64_t>(ctx->rows_per, ctx->N - g0);
    MLFF_HIP(ctx, hipMemcpy2DAsync(ctx->K + (int64_t)r * ctx->blk, sizeof(double) * ctx->ld,
                                   K_local + g0, sizeof(double) * ld_host, sizeof(double) * cnt,
                                   ctx->nrows, hipMemcpyHostToDevice, ctx->stream));
  }
  MLFF_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ctx->has_matrix = true;
  ctx->K_symmetric = false;
  ctx->sym.ready = false;
  ctx->mf = MfData();
  rbf_free(ctx);
  return MLFF_OK;
  MLFF_API_END(ctx)
}

int mlff_get_matrix_rows(mlff_ctx *ctx, int64_t r0, int64_t nr, double *out, int64_t ld_out) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  if (out == nullptr) return set_error(ctx, MLFF_ERR_ARG, "null pointer");
  if (!ctx->has_matrix && !ctx->rbf.ready) return set_error(ctx, MLFF_ERR_STATE, "no kernel matrix set");
  if (r0 < 0 || nr < 0 || r0 + nr > ctx->nrows || ld_out < ctx->N)
    return set_error(ctx, MLFF_ERR_ARG, "row range / ld_out");
  // rows of the dense K, or of the RBF source generated chunk-wise into scratch
  ScratchScope scope(ctx);
  const int64_t chunk = ctx->has_matrix ? nr : std::max<int64_t>(1, std::min<int64_t>(nr, (int64_t)(256e6 / (8.0 * ctx->ld))));
  double *tmp = nullptr;
  if (!ctx->has_matrix) MLFF_TRY(scratch_alloc(ctx, &tmp, (size_t)chunk * ctx->ld));
  for (int64_t c0 = 0; c0 < nr; c0 += chunk) {
    const int64_t cn = std::min<int64_t>(chunk, nr - c0);
    const double *src = ctx->K + (r0 + c0) * ctx->ld;
    if (!ctx->has_matrix) {
      launch_gen_rbf(tmp, ctx->ld, cn, ctx->row0 + r0 + c0, ctx->rows_per, ctx->blk, ctx->N,
                     ctx->rbf.Xs, ctx->rbf.d, ctx->rbf.jitter, ctx->stream);
      MLFF_HIP(ctx, hipGetLastError());
      src = tmp;
    }
    for (int r = 0; r < ctx->world; ++r) {
      const int64_t g0 = (int64_t)r * ctx->rows_per;
      if (g0 >= ctx->N) break;
      const int64_t cnt = std::min<int64_t>(ctx->rows_per, ctx->N - g0);
      MLFF_HIP(ctx, hipMemcpy2DAsync(out + c0 * ld_out + g0, sizeof(double) * ld_out,
                                     src + (int64_t)r * ctx->blk, sizeof(double) * ctx->ld,
                                     sizeof(double) * cnt, cn, hipMemcpyDeviceToHost, ctx->stream));
    }
    MLFF_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  return MLFF_OK;
  MLFF_API_END(ctx)
}

int mlff_gen_rbf(mlff_ctx *ctx, const double *X, int d, double length_scale, double jitter) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  if (X == nullptr || d < 1 || d > 8 || !(length_scale > 0.0))
    return set_error(ctx, MLFF_ERR_ARG, "gen_rbf: need X, 1 <= d <= 8, length_scale > 0");
  // the points (scaled as sklearn does, X / length_scale) are the kernel: tiles, columns,
  // diagonal and (for the DENSE storage only) the rows are evaluated from them on device
  std::vector<double> Xs((size_t)ctx->N * d);
  for (size_t i = 0; i < Xs.size(); ++i) Xs[i] = X[i] / length_scale;
  // the squared diagonal of the scaled points' box bounds every squared distance: where it is
  // small enough the tile mat-vec's generating role drops its clamp (SymGen::noclamp)
  bool finite = true;
  double extent2 = 0.0;
  for (int t = 0; t < d; ++t) {
    double lo = INFINITY, hi = -INFINITY;
    for (int64_t i = 0; i < ctx->N; ++i) {
      const double x = Xs[(size_t)i * d + t];
      finite = finite && std::isfinite(x);
      lo = std::min(lo, x);
      hi = std::max(hi, x);
    }
    extent2 += (hi - lo) * (hi - lo);
  }
  ctx->sym = SymPack{};
  ctx->mf = MfData();
  rbf_free(ctx);
  ctx->K.reset();  // a dense matrix set earlier is not this kernel
  ctx->has_matrix = false;
  MLFF_HIP(ctx, ctx->rbf.Xs.alloc((int64_t)Xs.size()));
  MLFF_HIP(ctx, hipMemcpy(ctx->rbf.Xs, Xs.data(), sizeof(double) * Xs.size(), hipMemcpyHostToDevice));
  ctx->rbf.d = d;
  ctx->rbf.jitter = jitter;
  ctx->rbf.extent2 = extent2;
  ctx->rbf.finite = finite;
  ctx->rbf.ready = true;
  ctx->K_symmetric = true;
  return MLFF_OK;
  MLFF_API_END(ctx)
}

int mlff_assemble_sgdml(mlff_ctx *ctx, const double *R_desc, const double *R_d_desc, int64_t M,
                        int n_atoms, const int32_t *perms, int n_perms, double sig) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  if (R_desc == nullptr || R_d_desc == nullptr || perms == nullptr || !(sig > 0.0))
    return set_error(ctx, MLFF_ERR_ARG, "assemble_sgdml: null input or sig <= 0");
  rbf_free(ctx);
  MLFF_TRY(ensure_matrix(ctx));
  MLFF_TRY(assemble_sgdml(ctx, R_desc, R_d_desc, M, n_atoms, perms, n_perms, sig));
  // the matrix-free form of the same operator (chosen by MLFF_STORAGE_AUTO when cheaper)
  MLFF_TRY(mf_setup(ctx, R_desc, R_d_desc, M, n_atoms, perms, n_perms, sig));
  ctx->has_matrix = true;
  ctx->K_symmetric = true;  // the assembly mirrors the lower block triangle
  ctx->sym.ready = false;
  return MLFF_OK;
  MLFF_API_END(ctx)
}

int mlff_sgdml_operator(mlff_ctx *ctx, const double *R_desc, const double *R_d_desc, int64_t M,
                        int n_atoms, const int32_t *perms, int n_perms, double sig) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  if (R_desc == nullptr || R_d_desc == nullptr || perms == nullptr || !(sig > 0.0))
    return set_error(ctx, MLFF_ERR_ARG, "sgdml_operator: null input or sig <= 0");
  rbf_free(ctx);
  MLFF_TRY(mf_setup(ctx, R_desc, R_d_desc, M, n_atoms, perms, n_perms, sig));
  ctx->use_mf = false;
  ctx->has_matrix = false;  // a dense K set earlier is not this operator
  ctx->sym.ready = false;
  return MLFF_OK;
  MLFF_API_END(ctx)
}

int mlff_test_gemm(mlff_ctx *ctx, int ta, int tb, int64_t M, int64_t N, int64_t K, double alpha,
                   const double *A, int64_t lda, const double *B, int64_t ldb, double beta,
                   double *C, int64_t ldc, int splits) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  if (A == nullptr || B == nullptr || C == nullptr || M < 0 || N < 0 || K < 0 || splits < 1 ||
      lda < (ta ? M : K) || ldb < (tb ? K : N) || ldc < N)
    return set_error(ctx, MLFF_ERR_ARG, "test_gemm: bad arguments");
  return test_gemm(ctx, ta, tb, M, N, K, alpha, A, lda, B, ldb, beta, C, ldc, splits);
  MLFF_API_END(ctx)
}

int mlff_test_potrf(mlff_ctx *ctx, const double *A, int64_t n, int variant, double *L_out,
                    double *seconds_out) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  if (A == nullptr || L_out == nullptr || n < 1 || variant < 0 || variant > 1)
    return set_error(ctx, MLFF_ERR_ARG, "test_potrf: bad arguments");
  return test_potrf(ctx, A, n, variant, L_out, seconds_out);
  MLFF_API_END(ctx)
}

int mlff_dense_cho_solve(mlff_ctx *ctx, double sigma_K, double shift, const double *b,
                         double *x_out, double *seconds_out) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  if (b == nullptr || x_out == nullptr) return set_error(ctx, MLFF_ERR_ARG, "null pointer");
  if (ctx->world > 1)
    return set_error(ctx, MLFF_ERR_ARG, "dense_cho_solve: the closed-form solve runs on one rank");
  if (!ctx->has_matrix)
    return set_error(ctx, MLFF_ERR_STATE,
                     "dense_cho_solve: no dense kernel matrix (mlff_set_matrix_host / "
                     "mlff_assemble_sgdml); a matrix-free operator alone cannot be factored");
  return dense_cho_solve(ctx, sigma_K, shift, b, x_out, seconds_out);
  MLFF_API_END(ctx)
}

int mlff_test_gram(mlff_ctx *ctx, const double *W, int64_t k, int64_t ncols, int mode,
                   double *G_out) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  if (W == nullptr || G_out == nullptr || k < 1 || ncols < 1 || mode < 0 || mode > 2)
    return set_error(ctx, MLFF_ERR_ARG, "test_gram: bad arguments");
  ScratchScope scope(ctx);
  double *dW = nullptr, *dG = nullptr;
  MLFF_TRY(scratch_alloc(ctx, &dW, (size_t)(k * ncols)));
  MLFF_TRY(scratch_alloc(ctx, &dG, (size_t)(k * k)));
  MLFF_HIP(ctx, hipMemcpyAsync(dW, W, sizeof(double) * k * ncols, hipMemcpyHostToDevice, ctx->stream));
  if (mode == 0)
    MLFF_TRY(syrk_wide(ctx, dW, k, ncols, ncols, dG));
  else
    MLFF_TRY(gram_wide_dd(ctx, dW, k, ncols, ncols, dG, mode == 2));
  MLFF_HIP(ctx, hipMemcpyAsync(G_out, dG, sizeof(double) * k * k, hipMemcpyDeviceToHost, ctx->stream));
  MLFF_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MLFF_OK;
  MLFF_API_END(ctx)
}

int mlff_sym_min_eig(mlff_ctx *ctx, const double *M, int64_t m, double *lo_eig_out,
                     double *d_out, double *e_out) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  if (M == nullptr || m < 1 || lo_eig_out == nullptr)
    return set_error(ctx, MLFF_ERR_ARG, "sym_min_eig: bad arguments");
  ScratchScope scope(ctx);
  double *dM = nullptr;
  MLFF_TRY(scratch_alloc(ctx, &dM, (size_t)(m * m)));
  MLFF_HIP(ctx, hipMemcpyAsync(dM, M, sizeof(double) * m * m, hipMemcpyHostToDevice, ctx->stream));
  return sym_min_eig(ctx, dM, m, lo_eig_out, d_out, e_out);
  MLFF_API_END(ctx)
}

int mlff_cho_factor_stable(mlff_ctx *ctx, const double *M, int64_t m, double *L_out,
                           double *lo_eig_out) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  if (M == nullptr || m < 1 || L_out == nullptr)
    return set_error(ctx, MLFF_ERR_ARG, "cho_factor_stable: bad arguments");
  ScratchScope scope(ctx);
  double *dM = nullptr;
  MLFF_TRY(scratch_alloc(ctx, &dM, (size_t)(m * m)));
  MLFF_HIP(ctx, hipMemcpyAsync(dM, M, sizeof(double) * m * m, hipMemcpyHostToDevice, ctx->stream));
  MLFF_TRY(cho_factor_stable(ctx, dM, m, lo_eig_out));
  MLFF_HIP(ctx, hipMemcpyAsync(L_out, dM, sizeof(double) * m * m, hipMemcpyDeviceToHost, ctx->stream));
  MLFF_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MLFF_OK;
  MLFF_API_END(ctx)
}

int mlff_spectrum(mlff_ctx *ctx, int preconditioned, double *eig_out) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  if (eig_out == nullptr) return set_error(ctx, MLFF_ERR_ARG, "null pointer");
  MLFF_TRY(require_operator(ctx));
  return spectrum(ctx, preconditioned != 0, eig_out);
  MLFF_API_END(ctx)
}

int mlff_set_energy_constraints(mlff_ctx *ctx, int use_E_cstr) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  if (use_E_cstr && ctx->world > 1)
    return set_error(ctx, MLFF_ERR_ARG, "use_E_cstr: energy constraints run on one rank");
  ctx->use_E_cstr = use_E_cstr != 0;
  return MLFF_OK;
  MLFF_API_END(ctx)
}

// both probe hooks: the library's exp and the generating role's, with or without its clamp
static int test_rbf_exp(mlff_ctx *ctx, const double *s, int64_t n, double *lib_out, double *lean_out,
                        bool clamp) {
  if (s == nullptr || lib_out == nullptr || lean_out == nullptr || n < 1)
    return set_error(ctx, MLFF_ERR_ARG, "test_rbf_exp: bad arguments");
  if (!clamp)
    for (int64_t i = 0; i < n; ++i)
      if (!(s[i] >= 0.0 && s[i] <= 2150.0))
        return set_error(ctx, MLFF_ERR_ARG, "test_rbf_exp_noclamp: need 0 <= s <= 2150");
  ScratchScope scope(ctx);
  double *ds = nullptr, *da = nullptr, *db = nullptr;
  MLFF_TRY(scratch_alloc(ctx, &ds, (size_t)n));
  MLFF_TRY(scratch_alloc(ctx, &da, (size_t)n));
  MLFF_TRY(scratch_alloc(ctx, &db, (size_t)n));
  MLFF_HIP(ctx, hipMemcpyAsync(ds, s, sizeof(double) * n, hipMemcpyHostToDevice, ctx->stream));
  launch_rbf_exp_probe(ds, n, da, db, clamp, ctx->stream);
  MLFF_HIP(ctx, hipGetLastError());
  MLFF_HIP(ctx, hipMemcpyAsync(lib_out, da, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
  MLFF_HIP(ctx, hipMemcpyAsync(lean_out, db, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
  MLFF_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MLFF_OK;
}

int mlff_test_rbf_exp(mlff_ctx *ctx, const double *s, int64_t n, double *lib_out, double *lean_out) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  return test_rbf_exp(ctx, s, n, lib_out, lean_out, true);
  MLFF_API_END(ctx)
}

int mlff_test_rbf_exp_noclamp(mlff_ctx *ctx, const double *s, int64_t n, double *lib_out,
                              double *lean_out) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  return test_rbf_exp(ctx, s, n, lib_out, lean_out, false);
  MLFF_API_END(ctx)
}

int mlff_sgdml_descriptors(const double *R, int64_t M, int n_atoms, double *R_desc_out,
                           double *R_d_desc_out) {
  MLFF_API_BEGIN
  if (R == nullptr || R_desc_out == nullptr || R_d_desc_out == nullptr || M < 1 || n_atoms < 2)
    return set_error(nullptr, MLFF_ERR_ARG, "sgdml_descriptors: bad arguments");
  const int rc = sgdml_descriptors(R, M, n_atoms, R_desc_out, R_d_desc_out);
  if (rc != MLFF_OK) return set_error(nullptr, rc, "sgdml_descriptors: HIP failure");
  return MLFF_OK;
  MLFF_API_END(nullptr)
}

int mlff_sgdml_energies(mlff_ctx *ctx, const double *alphas, double *E_out, int64_t *i0_out,
                        int64_t *ni_out) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  if (alphas == nullptr || E_out == nullptr) return set_error(ctx, MLFF_ERR_ARG, "null pointer");
  if (!ctx->mf.ready) return set_error(ctx, MLFF_ERR_STATE, "no sGDML operator set");
  const MfData &mf = ctx->mf;
  const int64_t MP = mf.M * mf.n_perms;
  std::vector<double> pairs((size_t)std::max<int64_t>(mf.ni, 1) * MP);
  MLFF_TRY(mf_energies(ctx, alphas, pairs.data()));
  for (int64_t i = 0; i < mf.ni; ++i) {
    double e = 0.0;
    for (int64_t jp = 0; jp < MP; ++jp) e += pairs[(size_t)i * MP + jp];
    E_out[i] = e;
  }
  if (i0_out) *i0_out = mf.i0;
  if (ni_out) *ni_out = mf.ni;
  return MLFF_OK;
  MLFF_API_END(ctx)
}

int mlff_predict_set_model(mlff_ctx *ctx, const double *R_desc, const double *R_d_desc_alpha,
                           int64_t M, int n_atoms, const int32_t *perms, int n_perms, double sig,
                           double std, double c) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  if (ctx->world > 1) return set_error(ctx, MLFF_ERR_ARG, "predict: runs on a one-rank context");
  if (R_desc == nullptr || R_d_desc_alpha == nullptr || perms == nullptr)
    return set_error(ctx, MLFF_ERR_ARG, "predict: null pointer");
  if (n_atoms < 2 || M < 1 || n_perms < 1 || n_perms > 1024)
    return set_error(ctx, MLFF_ERR_ARG, "predict: bad sizes");
  if (3 * (int64_t)n_atoms * M != ctx->N)
    return set_error(ctx, MLFF_ERR_ARG, "predict: N != 3 * n_atoms * M");
  if (!(sig > 0.0)) return set_error(ctx, MLFF_ERR_ARG, "predict: sig must be > 0");
  return pred_set_model(ctx, R_desc, R_d_desc_alpha, M, n_atoms, perms, n_perms, sig, std, c);
  MLFF_API_END(ctx)
}

int mlff_predict_set_energy_coefficients(mlff_ctx *ctx, const double *alphas_E) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  if (!ctx->pred.ready) return set_error(ctx, MLFF_ERR_STATE, "predict: no model set (mlff_predict_set_model)");
  return pred_set_energy_coefficients(ctx, alphas_E);
  MLFF_API_END(ctx)
}

int mlff_predict(mlff_ctx *ctx, const double *R, int64_t Q, double *E_out, double *F_out) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  if (ctx->world > 1) return set_error(ctx, MLFF_ERR_ARG, "predict: runs on a one-rank context");
  if (!ctx->pred.ready) return set_error(ctx, MLFF_ERR_STATE, "predict: no model set (mlff_predict_set_model)");
  if (Q < 0) return set_error(ctx, MLFF_ERR_ARG, "predict: Q < 0");
  if (Q == 0) return MLFF_OK;
  if (R == nullptr || E_out == nullptr || F_out == nullptr)
    return set_error(ctx, MLFF_ERR_ARG, "predict: null pointer");
  return pred_run(ctx, R, Q, E_out, F_out);
  MLFF_API_END(ctx)
}

int mlff_predict_info(mlff_ctx *ctx, int *form_out, int64_t *slab_out, double *flops_per_query_out,
                      double *bytes_per_query_out) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  if (!ctx->pred.ready) return set_error(ctx, MLFF_ERR_STATE, "predict: no model set (mlff_predict_set_model)");
  double fl = 0.0, by = 0.0;
  pred_work(ctx->pred, &fl, &by);
  if (form_out) *form_out = ctx->pred.form;
  if (slab_out) *slab_out = ctx->pred.slab;
  if (flops_per_query_out) *flops_per_query_out = fl;
  if (bytes_per_query_out) *bytes_per_query_out = by;
  return MLFF_OK;
  MLFF_API_END(ctx)
}

int mlff_predict_hessian(mlff_ctx *ctx, const double *R, int64_t Q, double *H_out) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  if (ctx->world > 1) return set_error(ctx, MLFF_ERR_ARG, "predict hessian: runs on a one-rank context");
  if (!ctx->pred.ready)
    return set_error(ctx, MLFF_ERR_STATE, "predict hessian: no model set (mlff_predict_set_model)");
  if (Q < 0) return set_error(ctx, MLFF_ERR_ARG, "predict hessian: Q < 0");
  if (Q == 0) return MLFF_OK;
  if (R == nullptr || H_out == nullptr) return set_error(ctx, MLFF_ERR_ARG, "predict hessian: null pointer");
  return pred_hess_run(ctx, R, Q, H_out);
  MLFF_API_END(ctx)
}

int mlff_predict_hessian_info(mlff_ctx *ctx, double *flops_per_query_out, double *bytes_per_query_out) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  if (!ctx->pred.ready)
    return set_error(ctx, MLFF_ERR_STATE, "predict hessian: no model set (mlff_predict_set_model)");
  double fl = 0.0, by = 0.0;
  pred_hess_work(ctx->pred, &fl, &by);
  if (flops_per_query_out) *flops_per_query_out = fl;
  if (bytes_per_query_out) *bytes_per_query_out = by;
  return MLFF_OK;
  MLFF_API_END(ctx)
}

int mlff_predict_hvp(mlff_ctx *ctx, const double *R, const double *V, int64_t Q, int64_t K, double *HV_out) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  if (ctx->world > 1) return set_error(ctx, MLFF_ERR_ARG, "predict hvp: runs on a one-rank context");
  if (!ctx->pred.ready)
    return set_error(ctx, MLFF_ERR_ARG, "predict hvp: no model set (mlff_predict_set_model)");
  if (Q < 0) return set_error(ctx, MLFF_ERR_ARG, "predict hvp: Q < 0");
  if (K < 0) return set_error(ctx, MLFF_ERR_ARG, "predict hvp: K < 0");
  if (Q == 0 || K == 0) return MLFF_OK;
  if (R == nullptr || V == nullptr || HV_out == nullptr)
    return set_error(ctx, MLFF_ERR_ARG, "predict hvp: null pointer");
  return pred_hvp_run(ctx, R, V, Q, K, HV_out);
  MLFF_API_END(ctx)
}

int mlff_predict_hvp_info(mlff_ctx *ctx, double *flops_per_product_out, double *bytes_per_query_out) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  if (!ctx->pred.ready)
    return set_error(ctx, MLFF_ERR_ARG, "predict hvp: no model set (mlff_predict_set_model)");
  double fl = 0.0, by = 0.0;
  pred_hvp_work(ctx->pred, &fl, &by);
  if (flops_per_product_out) *flops_per_product_out = fl;
  if (bytes_per_query_out) *bytes_per_query_out = by;
  return MLFF_OK;
  MLFF_API_END(ctx)
}

int mlff_md_run(mlff_ctx *ctx, const double *R0, const double *V0, const double *h, int64_t Q, double dt,
                int64_t n_steps, int64_t stride, int want_forces, double *R_out, double *V_out,
                double *E_out, double *F_out) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  if (ctx->world > 1) return set_error(ctx, MLFF_ERR_ARG, "md: runs on a one-rank context");
  if (!ctx->pred.ready) return set_error(ctx, MLFF_ERR_STATE, "md: no model set (mlff_predict_set_model)");
  if (Q < 0) return set_error(ctx, MLFF_ERR_ARG, "md: Q < 0");
  if (n_steps < 0) return set_error(ctx, MLFF_ERR_ARG, "md: n_steps < 0");
  if (stride < 1) return set_error(ctx, MLFF_ERR_ARG, "md: stride < 1");
  if (n_steps % stride != 0) return set_error(ctx, MLFF_ERR_ARG, "md: n_steps is not a multiple of stride");
  if (!std::isfinite(dt)) return set_error(ctx, MLFF_ERR_ARG, "md: dt is not finite");
  if (Q > 0 && (R0 == nullptr || V0 == nullptr || h == nullptr || R_out == nullptr || V_out == nullptr ||
                E_out == nullptr || (want_forces != 0 && F_out == nullptr)))
    return set_error(ctx, MLFF_ERR_ARG, "md: null pointer");
  return md_run(ctx, R0, V0, h, Q, dt, n_steps, stride, want_forces != 0, R_out, V_out, E_out, F_out);
  MLFF_API_END(ctx)
}

int mlff_md_info(mlff_ctx *ctx, int *launches_per_step_out, int64_t *frame_capacity_out,
                 int64_t *syncs_last_run_out) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  if (!ctx->pred.ready) return set_error(ctx, MLFF_ERR_STATE, "md: no model set (mlff_predict_set_model)");
  return md_info(ctx, launches_per_step_out, frame_capacity_out, syncs_last_run_out);
  MLFF_API_END(ctx)
}

int mlff_md_set_form(mlff_ctx *ctx, int launches_per_step) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  if (!ctx->pred.ready) return set_error(ctx, MLFF_ERR_STATE, "md: no model set (mlff_predict_set_model)");
  return md_set_form(ctx, launches_per_step);
  MLFF_API_END(ctx)
}

int mlff_set_operator(mlff_ctx *ctx, double sigma_K, double lam) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  if (!(lam > 0.0)) return set_error(ctx, MLFF_ERR_ARG, "lam must be > 0");
  if (sigma_K != 1.0 && sigma_K != -1.0) return set_error(ctx, MLFF_ERR_ARG, "sigma_K must be +-1");
  ctx->sigma_K = sigma_K;
  ctx->lam = lam;
  ctx->has_operator = true;
  return MLFF_OK;
  MLFF_API_END(ctx)
}

int mlff_set_storage(mlff_ctx *ctx, int mode) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  if (mode != MLFF_STORAGE_DENSE && mode != MLFF_STORAGE_SYMTILE && mode != MLFF_STORAGE_AUTO &&
      mode != MLFF_STORAGE_MATFREE)
    return set_error(ctx, MLFF_ERR_ARG, "bad storage mode");
  if (mode != ctx->storage) {
    ctx->storage = mode;
    ctx->use_sym = false;
    ctx->use_mf = false;
    if (mode == MLFF_STORAGE_DENSE || mode == MLFF_STORAGE_MATFREE) ctx->sym = SymPack{};
  }
  return MLFF_OK;
  MLFF_API_END(ctx)
}

int mlff_operator_form(mlff_ctx *ctx, int *form_out) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  if (form_out == nullptr) return set_error(ctx, MLFF_ERR_ARG, "null form_out");
  *form_out = ctx->mf.ready ? mf_form(ctx) : -1;
  return MLFF_OK;
  MLFF_API_END(ctx)
}

int mlff_storage_info(mlff_ctx *ctx, int *mode_out, double *bytes_per_matvec_out) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  MLFF_TRY(require_operator(ctx));
  MLFF_TRY(resolve_storage(ctx));
  if (mode_out)
    *mode_out = ctx->use_mf ? MLFF_STORAGE_MATFREE
                            : (ctx->use_sym ? MLFF_STORAGE_SYMTILE : MLFF_STORAGE_DENSE);
  if (bytes_per_matvec_out) *bytes_per_matvec_out = operator_bytes(ctx);
  return MLFF_OK;
  MLFF_API_END(ctx)
}

int mlff_sym_launch_info(mlff_ctx *ctx, int *wgs_per_cu_out, int64_t *grid_out) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  MLFF_TRY(require_operator(ctx));
  MLFF_TRY(resolve_storage(ctx));
  if (!ctx->use_sym || !ctx->sym.ready) return set_error(ctx, MLFF_ERR_STATE, "no symmetric tile operator");
  if (wgs_per_cu_out) *wgs_per_cu_out = ctx->sym.wgs;
  if (grid_out) *grid_out = ctx->sym.dyn;
  return MLFF_OK;
  MLFF_API_END(ctx)
}

int mlff_sym_gen_info(mlff_ctx *ctx, int *noclamp_out, double *extent2_out) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  MLFF_TRY(require_operator(ctx));
  MLFF_TRY(resolve_storage(ctx));
  if (!ctx->use_sym || !ctx->sym.ready) return set_error(ctx, MLFF_ERR_STATE, "no symmetric tile operator");
  if (!ctx->rbf.ready) return set_error(ctx, MLFF_ERR_STATE, "the tiles were not generated from RBF points");
  if (noclamp_out) *noclamp_out = ctx->sym.gen ? ctx->sym.gsrc.noclamp : 0;
  if (extent2_out) *extent2_out = ctx->rbf.extent2;
  return MLFF_OK;
  MLFF_API_END(ctx)
}

int mlff_matvec(mlff_ctx *ctx, const double *v_global, double *y_local) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  MLFF_TRY(require_operator(ctx));
  if (v_global == nullptr || (y_local == nullptr && ctx->nrows > 0)) return set_error(ctx, MLFF_ERR_ARG, "null vector");
  MLFF_TRY(resolve_storage(ctx));
  MLFF_TRY(scatter_global(ctx, v_global, ctx->xg));
  MLFF_TRY(launch_operator(ctx, ctx->xg, ctx->q, ctx->xg + (int64_t)ctx->rank * ctx->blk, nullptr));
  MLFF_HIP(ctx, hipGetLastError());
  if (ctx->nrows > 0)
    MLFF_HIP(ctx, hipMemcpyAsync(y_local, ctx->q, sizeof(double) * ctx->nrows, hipMemcpyDeviceToHost, ctx->stream));
  MLFF_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MLFF_OK;
  MLFF_API_END(ctx)
}

int mlff_get_diag(mlff_ctx *ctx, double *diag_local) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  if (!ctx->has_matrix && !ctx->mf.ready && !ctx->rbf.ready)
    return set_error(ctx, MLFF_ERR_STATE, "no kernel matrix set");
  MLFF_TRY(operator_diag(ctx, ctx->dwork));
  if (ctx->nrows > 0)
    MLFF_HIP(ctx, hipMemcpyAsync(diag_local, ctx->dwork, sizeof(double) * ctx->nrows, hipMemcpyDeviceToHost, ctx->stream));
  MLFF_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MLFF_OK;
  MLFF_API_END(ctx)
}

int mlff_precon_none(mlff_ctx *ctx) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  ctx->lr.kind = MLFF_PRECON_NONE;  // the panel's buffers stay until the next build
  ctx->lr.k = 0;
  return MLFF_OK;
  MLFF_API_END(ctx)
}

int mlff_precon_pivchol(mlff_ctx *ctx, int64_t k, int build_woodbury, int64_t *index_columns_out,
                        double *seconds_out) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  MLFF_TRY(require_operator(ctx));
  if (k < 1 || k > ctx->N || k > 65536)
    return set_error(ctx, MLFF_ERR_ARG, "pivoted Cholesky rank k must satisfy 1 <= k <= min(N, 65536)");
  const auto t0 = std::chrono::steady_clock::now();
  MLFF_TRY(alloc_panel(ctx, k));
  MLFF_HIP(ctx, ctx->prow.alloc(k + 1));
  MLFF_TRY(pivoted_cholesky(ctx, k, index_columns_out));
  // without Woodbury the panel holds L^T (mlff_precon_get_panel), unused by PCG
  ctx->piv_woodbury_s = 0.0;
  if (build_woodbury) {
    const auto tw = std::chrono::steady_clock::now();
    MLFF_TRY(woodbury_inplace(ctx, ctx->lr.T, k));
    ctx->piv_woodbury_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - tw).count();
    ctx->lr.commit(MLFF_PRECON_PIVCHOL, 1.0);
  }
  MLFF_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (seconds_out)
    *seconds_out = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return MLFF_OK;
  MLFF_API_END(ctx)
}

int mlff_pivchol_times(mlff_ctx *ctx, double *col_seconds_out, int64_t k,
                       double *woodbury_seconds_out) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  if (k < 0 || (k > 0 && col_seconds_out == nullptr)) return set_error(ctx, MLFF_ERR_ARG, "bad output");
  const int64_t n = std::min<int64_t>(k, (int64_t)ctx->piv_col_s.size());
  for (int64_t c = 0; c < n; ++c) col_seconds_out[c] = ctx->piv_col_s[c];
  for (int64_t c = n; c < k; ++c) col_seconds_out[c] = 0.0;
  if (woodbury_seconds_out) *woodbury_seconds_out = ctx->piv_woodbury_s;
  return MLFF_OK;
  MLFF_API_END(ctx)
}

int mlff_precon_nystrom(mlff_ctx *ctx, const int64_t *idx, int64_t k, int variant,
                        double *seconds_out) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  MLFF_TRY(require_operator(ctx));
  if (variant != 0 && variant != 1) return set_error(ctx, MLFF_ERR_ARG, "variant must be 0 or 1");
  MLFF_TRY(check_idx(ctx, idx, k));
  const auto t0 = std::chrono::steady_clock::now();
  MLFF_TRY(alloc_panel(ctx, k));
  MLFF_TRY(nystrom_panel(ctx, idx, k, variant, ctx->lam, ctx->lr.T));
  // _P_vec returns (B^T B v - v)/lam; _sb returns -(v - P^T P v)/lam
  ctx->lr.commit(variant == 0 ? MLFF_PRECON_NYSTROM : MLFF_PRECON_NYSTROM_SB, -1.0);
  if (seconds_out)
    *seconds_out = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return MLFF_OK;
  MLFF_API_END(ctx)
}

int mlff_precon_lowrank(mlff_ctx *ctx, const double *Lt_local, int64_t k) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  MLFF_TRY(require_operator(ctx));
  if (k < 1 || k > ctx->N || (Lt_local == nullptr && ctx->nrows > 0))
    return set_error(ctx, MLFF_ERR_ARG, "lowrank: bad factor");
  MLFF_TRY(alloc_panel(ctx, k));
  if (ctx->nrows > 0)
    MLFF_HIP(ctx, hipMemcpy2DAsync(ctx->lr.T, sizeof(double) * ctx->blk, Lt_local,
                                   sizeof(double) * ctx->nrows, sizeof(double) * ctx->nrows, k,
                                   hipMemcpyHostToDevice, ctx->stream));
  MLFF_TRY(woodbury_inplace(ctx, ctx->lr.T, k));
  ctx->lr.commit(MLFF_PRECON_LOWRANK, 1.0);
  return MLFF_OK;
  MLFF_API_END(ctx)
}

int mlff_precon_eig(mlff_ctx *ctx, int64_t k, int mask_mode, int64_t dim_i, int build_woodbury,
                    double *evals_out, double *rowlev_out) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  if (mask_mode < 0 || mask_mode > 2 || (mask_mode == 2 && (dim_i < 3 || dim_i % 3 != 0)))
    return set_error(ctx, MLFF_ERR_ARG, "eig: bad mask_mode / dim_i");
  if (mask_mode == 2) {  // the masked matrix is formed from this rank's rows of the dense K
    MLFF_TRY(require_matrix(ctx));
  } else {
    MLFF_TRY(require_operator(ctx));
  }
  if (k < 1 || k > ctx->N) return set_error(ctx, MLFF_ERR_ARG, "eig: need 1 <= k <= N");
  MLFF_TRY(alloc_panel(ctx, k));
  MLFF_TRY(eig_lowrank(ctx, k, mask_mode, dim_i, ctx->lr.T, evals_out, rowlev_out));
  if (build_woodbury) {
    MLFF_TRY(woodbury_inplace(ctx, ctx->lr.T, k));
    ctx->lr.commit(MLFF_PRECON_EIG, 1.0);
  }
  return MLFF_OK;
  MLFF_API_END(ctx)
}

int mlff_eig_info(mlff_ctx *ctx, int *converged_out, double *rel_resid_out) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  if (converged_out) *converged_out = ctx->eig_converged ? 1 : 0;
  if (rel_resid_out) *rel_resid_out = ctx->eig_rel_resid;
  return MLFF_OK;
  MLFF_API_END(ctx)
}

int mlff_precon_info(mlff_ctx *ctx, int *kind_out, int64_t *k_out) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  if (kind_out) *kind_out = ctx->lr.kind;
  if (k_out) *k_out = ctx->lr.k;
  return MLFF_OK;
  MLFF_API_END(ctx)
}

int mlff_precon_apply_traffic(mlff_ctx *ctx, int *one_pass_out, double *bytes_out) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  if (one_pass_out) *one_pass_out = ctx->lr.apply_form();
  if (bytes_out) *bytes_out = ctx->lr.apply_bytes(ctx->blk, ctx->nrows);
  return MLFF_OK;
  MLFF_API_END(ctx)
}

int mlff_precon_apply(mlff_ctx *ctx, const double *r_local, double *z_local) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  MLFF_TRY(require_operator(ctx));
  hipStream_t s = ctx->stream;
  ScratchScope scope(ctx);
  double *rd = nullptr, *zd = nullptr;
  MLFF_TRY(scratch_alloc(ctx, &rd, ctx->blk));
  MLFF_TRY(scratch_alloc(ctx, &zd, ctx->blk));
  MLFF_HIP(ctx, hipMemsetAsync(rd, 0, sizeof(double) * ctx->blk, s));
  if (ctx->nrows > 0)
    MLFF_HIP(ctx, hipMemcpyAsync(rd, r_local, sizeof(double) * ctx->nrows, hipMemcpyHostToDevice, s));
  LowRank &lr = ctx->lr;
  if (!lr.active()) {
    MLFF_HIP(ctx, hipMemcpyAsync(zd, rd, sizeof(double) * ctx->blk, hipMemcpyDeviceToDevice, s));
  } else {
    lr.drop_speculative_t();  // tpart is reused below
    const bool cluster = !ctx->exact_sums && lr.form == LowRank::kCluster;
    if (cluster) MLFF_HIP(ctx, hipMemsetAsync(lr.fault, 0, sizeof(int), s));
    MLFF_TRY(lowrank_apply(ctx, rd, zd, nullptr, nullptr, lr.fault));
    if (cluster) {
      MLFF_HIP(ctx, hipGetLastError());
      int fault = 0;
      MLFF_HIP(ctx, hipMemcpyAsync(&fault, lr.fault, sizeof(int), hipMemcpyDeviceToHost, s));
      MLFF_HIP(ctx, hipStreamSynchronize(s));
      if (fault != 0) {  // hand-offs timed out (members not all resident): two passes
        lr.demote_cluster();
        MLFF_TRY(lowrank_tr(ctx, rd, nullptr));
        lowrank_z(ctx, rd, zd, nullptr, nullptr);
      }
    }
  }
  MLFF_HIP(ctx, hipGetLastError());
  if (ctx->nrows > 0)
    MLFF_HIP(ctx, hipMemcpyAsync(z_local, zd, sizeof(double) * ctx->nrows, hipMemcpyDeviceToHost, s));
  MLFF_HIP(ctx, hipStreamSynchronize(s));
  return MLFF_OK;
  MLFF_API_END(ctx)
}

int mlff_precon_get_panel(mlff_ctx *ctx, double *T_local, int64_t ld_out) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  if (ctx->lr.T == nullptr || ctx->lr.k < 1) return set_error(ctx, MLFF_ERR_STATE, "no low-rank panel");
  if (T_local == nullptr || ld_out < ctx->nrows) return set_error(ctx, MLFF_ERR_ARG, "bad output");
  if (ctx->nrows > 0)
    MLFF_HIP(ctx, hipMemcpy2DAsync(T_local, sizeof(double) * ld_out, ctx->lr.T, sizeof(double) * ctx->blk,
                                   sizeof(double) * ctx->nrows, ctx->lr.k, hipMemcpyDeviceToHost, ctx->stream));
  MLFF_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MLFF_OK;
  MLFF_API_END(ctx)
}

int mlff_lev_scores(mlff_ctx *ctx, const int64_t *idx, int64_t k, double lam, double *scores_out) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  if (!ctx->has_matrix && !ctx->mf.ready && !ctx->rbf.ready)
    return set_error(ctx, MLFF_ERR_STATE, "no kernel matrix set");
  if (!(lam > 0.0) || scores_out == nullptr) return set_error(ctx, MLFF_ERR_ARG, "lev_scores: bad args");
  MLFF_TRY(check_idx(ctx, idx, k));
  hipStream_t s = ctx->stream;
  DevBuf<double> W;  // released on every return
  MLFF_HIP(ctx, W.alloc(round_up(k, 8) * ctx->blk));
  MLFF_HIP(ctx, hipMemsetAsync(W, 0, sizeof(double) * round_up(k, 8) * ctx->blk, s));
  MLFF_TRY(nystrom_panel(ctx, idx, k, 0, lam, W));
  MLFF_HIP(ctx, hipMemsetAsync(ctx->xg, 0, sizeof(double) * ctx->ld, s));
  launch_colsumsq(W, k, ctx->nrows, ctx->blk, ctx->xg + (int64_t)ctx->rank * ctx->blk, s);
  MLFF_TRY(allgather_blocks(ctx, ctx->xg));
  for (int r = 0; r < ctx->world; ++r) {
    const int64_t g0 = (int64_t)r * ctx->rows_per;
    if (g0 >= ctx->N) break;
    const int64_t cnt = std::min<int64_t>(ctx->rows_per, ctx->N - g0);
    MLFF_HIP(ctx, hipMemcpyAsync(scores_out + g0, ctx->xg + (int64_t)r * ctx->blk,
                                 sizeof(double) * cnt, hipMemcpyDeviceToHost, s));
  }
  MLFF_HIP(ctx, hipStreamSynchronize(s));
  return MLFF_OK;
  MLFF_API_END(ctx)
}

int mlff_device_memory(mlff_ctx *ctx, int64_t *free_out, int64_t *total_out) {
  MLFF_API_BEGIN
  MLFF_ENTER(ctx);
  size_t fr = 0, tot = 0;
  MLFF_HIP(ctx, hipMemGetInfo(&fr, &tot));
  if (free_out) *free_out = (int64_t)fr;
  if (total_out) *total_out = (int64_t)tot;
  return MLFF_OK;
  MLFF_API_END(ctx)
}

int mlff_live_bytes(int64_t *bytes_out) {
  MLFF_API_BEGIN
  if (bytes_out == nullptr) return set_error(nullptr, MLFF_ERR_ARG, "null pointer");
  *bytes_out = live_bytes.load();
  return MLFF_OK;
  MLFF_API_END(nullptr)
}

}  // extern "C"
