// Shared definitions of the gfx950 PCG library: context layout, device scalar
// block, launcher prototypes.  Everything here is private to libmlffpcg.so; the
// public surface is include/mlffpcg.h.
#pragma once

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <atomic>
#include <cstdint>
#include <memory>
#include <string>
#include <cstdlib>
#include <vector>

#include "../../include/mlffpcg.h"

namespace mlff {

constexpr int kWave = 64;
constexpr int kBlock = 256;       // threads per workgroup for streaming kernels
constexpr int kPad = 64;          // row / vector padding (doubles) = 512 B
constexpr int kMaxPart = 1024;    // partial-sum slots per reduction
constexpr int kVecGrid = 512;     // workgroups of the grid-stride vector kernels
constexpr int kSymTile = 512;     // tile edge of the symmetric tiled operator

__host__ __device__ inline int64_t round_up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }

}  // namespace mlff

struct mlff_ctx;

namespace mlff {

int set_error(mlff_ctx *ctx, int code, const std::string &msg);

// Owner of one device allocation (Pinned: of one pinned host allocation); null by default,
// move-only, freed by its destructor.  It converts to the raw pointer, so launches, copies and
// pointer arithmetic take it as they take a pointer (.get() where a template deduces from it).
// Every owning pointer of the library is one of these; views into a buffer and the structs handed
// to kernels by value hold raw pointers (the deleted copy refuses an owner inside one).
inline std::atomic<int64_t> live_bytes{0};  // held by all owners of the process (mlff_live_bytes)
template <typename T, bool Pinned = false>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  DevBuf(DevBuf &&o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr; }
  DevBuf &operator=(DevBuf &&o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_;
      bytes_ = o.bytes_;
      o.p_ = nullptr;
    }
    return *this;
  }
  ~DevBuf() { reset(); }
  void reset() {
    if (p_ == nullptr) return;
    (void)(Pinned ? hipHostFree(p_) : hipFree(p_));
    live_bytes -= (int64_t)bytes_;
    p_ = nullptr;
  }
  T *get() const { return p_; }
  operator T *() const { return p_; }
  T *operator->() const { return p_; }  // ctx->st->status, ctx->h_st->iters
  // release what is held, then allocate `count` elements (0: one); failure leaves null.  The
  // first form is for MLFF_HIP (hip_check's code and text), the second reports MLFF_ERR_NOMEM
  hipError_t alloc(int64_t count) {
    reset();
    const size_t bytes = sizeof(T) * (size_t)(count > 0 ? count : 1);
    void *p = nullptr;
    const hipError_t e = Pinned ? hipHostMalloc(&p, bytes, hipHostMallocDefault) : hipMalloc(&p, bytes);
    if (e != hipSuccess) return e;
    p_ = static_cast<T *>(p);
    bytes_ = bytes;
    live_bytes += (int64_t)bytes;
    return hipSuccess;
  }
  int alloc(mlff_ctx *ctx, int64_t count, const char *what) {
    if (alloc(count) == hipSuccess) return MLFF_OK;
    return set_error(ctx, MLFF_ERR_NOMEM,
                     std::string(what) + (Pinned ? ": pinned host allocation failed" : ": device allocation failed"));
  }

 private:
  T *p_ = nullptr;
  size_t bytes_ = 0;
};
template <typename T>
using PinBuf = DevBuf<T, true>;

// PCG status values kept on the device (status gating: every kernel of an
// iteration returns immediately unless status == RUNNING).
enum : int { ST_RUNNING = 0, ST_RECHECK = 1, ST_CONVERGED = 2, ST_MAXITER = 3, ST_FAULT = 4 };

// Device-resident scalars of the solver.  One instance per context.
struct DevState {
  double rho, rho1, alpha, pq, rr, resid, atol, pad0;
  long long iters;     // completed CG iterations (scipy ITER)
  long long maxiter;
  int status;
  int linalg_err;      // set by the Cholesky kernels on a non-positive pivot
  int pivot_err;       // set by the pivoted-Cholesky finaliser (pivot <= 0)
  int pad1;
  long long m_pi;      // current pivot (global index) of the pivoted Cholesky
  double sqrt_piv;     // its sqrt(pivot)
  double best_val;     // argmax of this rank
  long long best_pos;
  double rho_new;      // fused p update: rho of the iteration, published by k_rec_g for k_rec_fin
};

// Generating role of the tile mat-vec (kernels_sym.hip k_symv_dyn): where the tiles were
// generated from the RBF points (k_sym_gen_rbf's inputs, resident in RbfData), part of the
// workgroups evaluate their tiles' entries from the points -- the stored bits -- instead of
// streaming them, on the fp64 pipe the stream leaves idle.
constexpr int kSymGenMaxD = 3;  // point dimensions the role keeps in registers (above: all streamed)
// The static share n_s = nwhole R_s / (R_s + R_g) of the two roles, one streaming and two
// generating workgroups on every CU of one MI355X, d = 3.  Since a workgroup that is done goes
// on with the other role's range, the share only says where each role starts: R_s and R_g are
// the units per ms at which the kernel finishes when the whole range is the streaming role's
// ("0:2" of tools/sweep_symgen.py: 8256 tiles in 1.47 ms, the step's 1.540 less the 0.07 ms
// of its other kernels) and when it is the generating role's ("8192:2": 1.48 ms).  They are
// equal within the timings' scatter, so half of the whole tiles start in either role; the
// sweep is flat within 1.5 % from 4096 to 7168 generated tiles (profiles/symlean/, DESIGN.md
// 3.1: side by side the roles themselves run at 2700 and 2960 tiles/ms and end up with 48 and
// 52 % of the units).
constexpr double kSymStreamRate = 5600.0;
constexpr double kSymGenRate = 5600.0;
// units per resident workgroup from which the three-workgroup form runs (below: two workgroups
// per CU; measured at 1.4, where it loses, and at 2.75, 5.5 and 11, where it wins)
constexpr int kSymThreeWgMinUnits = 2;
struct SymGen {
  const double *Xs = nullptr;
  int d = 0;
  double jitter = 0.0;
  int64_t N = 0, rows_per = 0, blk = 0;
  int n_s = 0;    // whole tiles [0, n_s) are streamed, [n_s, nwhole) generated
  int qmode = 0;  // quarter units: 0 either role, 1 the streaming role's, 2 the generating role's
  int roles = 0;  // how a workgroup gets its role (SymRoles, MLFF_SYM_ROLES)
  int pool_first = 0;  // a role done with its own range: 0 the other role's range, then the
                       // quarter units; 1 the quarter units first (MLFF_SYM_STEAL=pool)
  int wgs = 2;    // resident workgroups per CU: one of them streams, the others generate
  int noclamp = 0;  // plain tiles evaluate their entries without the clamp of the squared
                    // distance: every point finite and RbfData::extent2 <= kSymGenNoClampExtent2
                    // (decided at the operator's build; MLFF_SYM_GEN_CLAMP=1: never)
};
// Largest squared diagonal of the scaled points' bounding box for which no squared distance can
// reach the 2150 that rbf_of_sqdist_lean<false> is good for: 5 % below it, the fma chain that
// forms a squared distance being 1e-15 relative
constexpr double kSymGenNoClampExtent2 = 2048.0;
// A workgroup's role: by its arrival count on its CU (of every SymGen::wgs arrivals the first
// streams, the others generate: one streaming workgroup on every CU whatever the dispatcher's
// placement), by blockIdx.x in the same way (the first rule, A/B), or every workgroup in one
// role (tests).  The result does not depend on it.
enum SymRoles : int { kSymRolesCu = 0, kSymRolesIndex = 1, kSymRolesStream = 2, kSymRolesGen = 3 };
// per-CU arrival words of k_symv_dyn behind its work counters: indexed by XCC id (4 bits) and
// HW_ID bits [15:8] (CU, SH, SE), never reset (the count modulo SymGen::wgs is all that is read)
constexpr int kSymCuWords = 4096;

// Lower-block-triangle tiles of K owned by this rank (kernels_sym.hip).
struct SymPack {
  bool ready = false;
  DevBuf<double> tiles;      // ntiles x B x B
  DevBuf<int2> list;         // (I, J) of each stored tile, I >= J
  int64_t ntiles = 0;
  int64_t Np = 0;            // padded global length (multiple of B)
  int64_t nb = 0;            // Np / B
  int64_t tiles_per_rank = 0;
  DevBuf<double> P;          // slot buffer nb x Np
  // the last (ntiles - nwhole) tiles of `list` run as 2^lsub sub-unit workgroups each;
  // their column partials of sub-units 1.. go to Pq (2^lsub - 1 planes of nb x Np)
  int64_t nwhole = 0;
  int lsub = 2;              // split tiles run as 2^lsub sub-units (row slices) each
  int64_t pq_planes = 0;     // planes allocated in Pq (2^lsub - 1 needed)
  DevBuf<double> Pq;
  DevBuf<unsigned char> split;     // nb x nb: tile (I, J) is split
  // nb x nb owned slots per row block (sym_own_entry) + nb counts (W > 1)
  DevBuf<int> own;
  // the same slots as a flat load list per row block (W > 1, k_sym_reduce_wl): entries
  // sym_plist_entry(slot, plane) (plane 0 = P, h >= 1 = Pq plane h - 1; a split slot's planes
  // follow it), pstride entries per row block, then nb counts; pmax = the largest count
  DevBuf<int> plist;
  int64_t pstride = 0;
  int pmax = 0;
  bool pq_ordered = false;         // k_sym_reduce_wl's arrival ordered (MLFF_SYM_PQ_ORDERED=1)
  int64_t t_split = 0;             // smallest I of a split tile (nb if none)
  int64_t dyn = 0;                 // > 0: k_symv_dyn with this many workgroups
  int wgs = 0;                     // ... which is this many resident workgroups on every CU
  bool rb4 = false;                // the three-workgroup form (k_symv_dyn<true, 4>, MLFF_SYM_WGS)
  DevBuf<unsigned long long> ticket;     // its work counters (reset by the slot reduction)
  bool gen = false;                // k_symv_dyn with a generating role (RBF source, sym_build)
  SymGen gsrc;                     // its source and the share of the two roles
  DevBuf<double> yg;         // world > 1: this rank's partial y, rank blocks of ystride
  DevBuf<double> yr;         // world > 1: reduce-scatter result (ystride)
  int64_t ystride = 0;       // blk + tail (p.q shares of every rank)
};

// Entry formats of SymPack::own and SymPack::plist: the only place their bits are written.
// own: the slot, kSymOwnSplit set where the slot's tile is split (its planes in Pq);
// plist: the slot in the low 16 bits, the plane above them.
constexpr int kSymOwnSplit = 1 << 24;
constexpr int kSymPlistSlotBits = 16;
constexpr int kSymPlistMaxSlots = (1 << kSymPlistSlotBits) - 1;  // nb a plist entry can hold
__host__ __device__ inline int sym_own_entry(int slot, bool split) {
  return slot | (split ? kSymOwnSplit : 0);
}
__host__ __device__ inline int sym_own_slot(int e) { return e & (kSymOwnSplit - 1); }
__host__ __device__ inline bool sym_own_split(int e) { return (e & kSymOwnSplit) != 0; }
__host__ __device__ inline int sym_plist_entry(int slot, int plane) {
  return slot | (plane << kSymPlistSlotBits);
}
__host__ __device__ inline int sym_plist_slot(int e) { return e & kSymPlistMaxSlots; }
__host__ __device__ inline int sym_plist_plane(int e) { return e >> kSymPlistSlotBits; }

// Matrix-free sGDML operator data (kernels_mf.hip).
struct MfData {
  bool ready = false;
  int64_t M = 0, D = 0;
  int n = 0, n_perms = 0;
  double sig = 0.0;
  int64_t i0 = 0, ni = 0;            // training points touched by this rank's rows
  DevBuf<double> Rd, Rdd;                 // M x D, M x D x 3
  DevBuf<double> Rt, Zt;                  // (M n_perms) x D
  DevBuf<int32_t> Pt, ps, pt;
  bool ident = false;                     // one identity permutation: Rt == Rd, Pt unused
  DevBuf<double> m5, w;                   // ni x (M n_perms), x independent
  DevBuf<double> c, F;                    // ni x (M n_perms), ni x D scratch
  DevBuf<double> part;                    // nz x ni x (M n_perms) pair partial sums
  DevBuf<double> ypart;                   // J^T partial rows (slices x nrows)
  DevBuf<double> xc;                      // contiguous operand (world > 1)
  int nz = 1;                             // descriptor slices of the pair sums
  int64_t dslice = 0;
  std::vector<int32_t> perms, piinv;      // host copies (diagonal blocks)
  // single-column path (kernels_gen.hip k_sgdml_col): (r = i, s = j) records of every
  // (local point, point, permutation), ni x M x n_perms x (6 n + 2), and device atom maps;
  // null when the table would exceed kMfColTableBytes (columns then go through the
  // whole operator)
  DevBuf<double> uvk;
  DevBuf<int32_t> pi_d, piinv_d;
  // record-factored operator (kernels_mf.hip k_rec_g / k_rec_fin), used when uvk exists:
  // wt = w transposed ((M n_perms) x ni), sv = the per-application pair scalars
  // 5 m (v . x_j) (ni x M n_perms), rpart = J^T G partial rows of every pair block
  // (rblk slots x ni x 3n)
  bool rec = false;
  int rec_rg = 8;         // k_rec_g query points per workgroup, identity permutation (MLFF_REC_RG)
  bool rec_wc16 = true;   // k_rec_g w / x staged as one 16-slot chunk when MP <= 16 (MLFF_REC_WC16)
  int rblk = 0;
  int64_t ldw = 0;
  DevBuf<double> wt, sv, rpart;
  // pair-tile form (kernels_pt.hip k_pt_pair / k_pt_fin; few atoms, D <= 288): in use when
  // ptile is set (the default where it exists; MLFF_MF_FORM=rec|pair|pt overrides); pt_S chunks
  // of the (j, p) range, ptpart = pt_S x ni x (padded D) partial F
  bool ptile = false;
  int pt_S = 1;
  DevBuf<double> ptpart;
  // energy constraints (use_E_cstr, train.py:212-236; iterative_solver.py:423-440): the
  // operand and result carry M energy entries after the nF = 3 n M force entries (one rank)
  bool E = false;
  int64_t nF = 0;
  DevBuf<double> kee;       // ni x M: sum_p (1 + nrm/sig (1 + nrm/(3 sig))) exp(-nrm/sig)
  DevBuf<double> eterm;     // ni x (M n_perms): a_ijp w_ijp of the last application
};

// Trained sGDML model held for prediction at new geometries (kernels_predict.hip): the
// permuted training descriptors / Jacobian-coefficient products, the form of the pair stage and
// the per-slab work buffers.  Independent of the operator (MfData) and of the matrix.
struct PredData {
  bool ready = false;
  int64_t M = 0, D = 0, MP = 0;
  int n = 0, n_perms = 0;
  double sig = 0.0, std = 1.0, c = 0.0;
  int form = 0;            // 0 tile (k_pr_pair), 1 stream (k_pr_stream)
  int S = 1;               // chunks of the (j, p) range: fixed by MP and the form
  int G = 1;               // queries per workgroup of the pair stage
  int64_t slab = 0;        // queries per pass (bounds part)
  int64_t PS = 0, ecol = 0;  // row stride of part, column of the energy partial
  DevBuf<double> Rt, Zt;                    // MP x D
  DevBuf<double> Et;                        // MP: alphas_E[j] per row (use_E_cstr models), else null
  DevBuf<double> Rq;                       // slab x n x 3 query geometries
  DevBuf<double> Rdq, Rddq;                 // slab x D, slab x D x 3
  DevBuf<double> part;                      // S x slab x PS chunk partials
  DevBuf<double> Fd;                        // slab x D
  DevBuf<double> EF;                        // results of a slab: E (slab) then F (slab x 3 n)
  PinBuf<double> h_in, h_out;               // pinned staging of Rq and EF: one copy each way
  // Hessians (kernels_predict_hess.hip): allocated by the first mlff_predict_hessian;
  // hs = Hess{} releases them
  struct Hess {
    bool ready = false;
    int S = 1;                             // chunks of the (j, p) range: fixed by MP
    int tb = 1;                            // rows per step of the pair stage: fixed by n
    int stage = 0;                         // > 0: the staged pair stage (k_hs_pair_s) with this many rows
    bool fd = false;                       // the Hessian's pair stage forms Fd itself (D <= 512)
    int64_t slab = 0;                      // queries per pass (<= the prediction's slab)
    int64_t nblk = 0;                      // 4 x 4 blocks of the lower triangle of H
    int64_t PS = 0;                        // row of the partials: 16 nblk + 2 (+ D for Fd)
    DevBuf<double> part;                   // S x slab x PS chunk partials
    DevBuf<double> sum;                    // slab x PS
    DevBuf<double> H;                      // slab x 3n x 3n
    PinBuf<double> h_out;                  // pinned staging of H
  } hs;
  // Hessian-vector products (kernels_predict_hvp.hip): allocated by the first mlff_predict_hvp;
  // hv = Hvp{} releases them
  struct Hvp {
    bool ready = false;
    int S = 1;                             // chunks of the (j, p) range: fixed by MP, D and the form
    int64_t slab = 0;                      // queries per pass (<= the prediction's slab)
    int64_t PS = 0;                        // row of the partials of a full vector block
    DevBuf<double> V, Y;                   // a pass's geometries (slab x 3n) then its vectors (slab x
                                           // kHvPass x 3n); slab x kHvPass x D: J v
    DevBuf<double> part;                   // S x (slab x blocks of a pass) x PS chunk partials
    DevBuf<double> sum;                    // (slab x blocks of a pass) x PS
    DevBuf<double> HV;                     // slab x kHvPass x 3n
    PinBuf<double> h_v, h_out;             // pinned staging of V (geometries included) and HV
  } hv;
  // Molecular dynamics (kernels_md.hip): configured and allocated by the first mlff_md_run;
  // md = Md{} releases it
  struct Md {
    bool ready = false;
    int launches = 4;                      // launches per step of the form in use (2: tile models)
    int want = 0;                          // 0: the default form, 2 / 4: asked for (mlff_md_set_form)
    int64_t cap = 0;                       // frames the device frame buffer holds (MLFF_MD_FRAMES)
    int64_t syncs = 0;                     // stream synchronisations of the last run
    int64_t frame_len = 0;                 // doubles the frame buffers hold
    DevBuf<double> hV;                     // h (n) then the slab's velocities (slab x 3n)
    DevBuf<double> frames;                 // cap frames of the slab: replica rows R, V, E (, F)
    PinBuf<double> h_in, h_frames;         // pinned staging of R0 / h, V0 and of the frames
  } md;
};

// Low-rank preconditioner z = sigma_p / lam (r - T^T T r): the panel, the form of its apply and
// that form's work buffers.  alloc_panel (api.hip) opens a build: kind NONE, k recorded with the
// panel, so T has round_up(k, 8) rows whether or not the build goes on to commit().
int lr_rows_groups(int64_t k);  // kernels_vec.hip, declared with the launchers below
struct LowRank {
  // the apply, as mlff_precon_apply_traffic reports it: T r then T^T t; one pass, a workgroup's
  // registers hold a row (launch_lr_apply_rows) or a cluster's do (launch_lr_apply_cluster)
  enum Form : int { kTwoPass = 0, kRows = 1, kCluster = 2 };
  int kind = MLFF_PRECON_NONE;  // MLFF_PRECON_*: NONE until a build commits
  int64_t k = 0;                // rows of T in use (0: mlff_precon_none)
  DevBuf<double> T;             // k x blk (row stride blk)
  double sigma_p = 1.0;
  Form form = kTwoPass;         // chosen per build; one rank only for the one-pass forms
  int tsplit = 1;               // column splits of the T GEMV
  int zsplit = 1;               // row splits of the T^T t GEMV
  DevBuf<double> zpart;         // zsplit x blk partials
  int q = 0;                    // kCluster: its clusters
  DevBuf<double> gpart;         // one pass: lr_rows_groups(k) (or q) x blk partials
  DevBuf<unsigned long long> slots;  // cluster hand-off granules (k x C x 2)
  unsigned epoch = 0;           // per cluster launch, never 0 in a launch
  DevBuf<int> fault;            // ST_FAULT when a cluster hand-off timed out (precon_apply)
  int fallbacks = 0;            // cluster applies that timed out and fell back to two passes
  // [rr partials (kVecGrid) | tpart (k x tsplit)]: on several ranks the end-of-iteration
  // ||r||^2 reduction and the next iteration's T r reduction share one all-reduce
  DevBuf<double> tpart_base;
  double *tpart = nullptr;      // view: tpart_base + kVecGrid
  bool spec_t = false;          // tpart already holds T r of the current r (merged collective)
  bool active() const { return kind != MLFF_PRECON_NONE; }
  void commit(int kind_, double sigma) { kind = kind_; sigma_p = sigma; }
  Form apply_form() const { return active() ? form : kTwoPass; }
  // bytes one apply moves, the counterpart of operator_bytes: the panel once or twice, the
  // one-pass forms' partial vectors written and read, r read and z written and read
  double apply_bytes(int64_t blk, int64_t nrows) const {
    const double N = (double)blk, n = (double)nrows, kd = (double)k;
    if (!active()) return 0.0;
    if (form == kTwoPass) return 16.0 * kd * N + 24.0 * n;
    return 8.0 * kd * N + 16.0 * (double)(form == kCluster ? q : lr_rows_groups(k)) * N + 24.0 * n;
  }
  // epoch of the next cluster-apply launch: never 0 (the value of a cleared hand-off slot)
  unsigned next_epoch() { return ++epoch != 0 ? epoch : ++epoch; }
  // a cluster hand-off timed out (the members were not all resident): two passes from here on
  void demote_cluster() { form = kTwoPass; fallbacks += 1; }
  // tpart no longer holds T r of the solver's r: the buffer was reallocated or reused for
  // another vector, or r was set anew (a solve's start, the true-residual recheck)
  void drop_speculative_t() { spec_t = false; }
};

// Synthetic RBF kernel source (tools/utils.py:173-187): the points, scaled by 1 / length
// scale, stay on the device and every consumer evaluates K from them -- the symmetric
// tiles are generated directly, columns / the diagonal / requested rows on demand -- so no
// dense N x N copy exists unless the DENSE storage asks for it (mlff_gen_rbf).
struct RbfData {
  bool ready = false;
  DevBuf<double> Xs;  // N x d
  int d = 0;
  double jitter = 0.0;
  // sum over the dimensions of (max - min)^2 of the scaled points: no squared distance between
  // two of them is larger.  finite: every coordinate is (else extent2 means nothing)
  double extent2 = 0.0;
  bool finite = false;
};

// K[i, g] (i != g) of the sklearn RBF kernel: exp(-0.5 * sum_t (xs_i - xs_g)^2).  The squared
// distance is the first square as a product and every further square through one fma --
// d0 d0, fma(d1, d1, .), fma(d2, d2, .), ... -- written out so that every site that evaluates
// an entry (the dense rows, the columns, the stored tiles and the tile mat-vec's generating
// role) rounds alike whatever the optimiser does where it is inlined.  (The separate
// multiply and add this replaced were contracted to exactly this by the compiler at every
// site, so no stored value changed; scipy's pdist 'sqeuclidean' rounds each product.)
// (xs_i - xs_g)^2 == (xs_g - xs_i)^2 exactly, so the generated kernel is exactly symmetric.
__device__ __forceinline__ double rbf_sqdist_step(double s, double df, bool first) {
  return first ? __dmul_rn(df, df) : fma(df, df, s);
}
__device__ __forceinline__ double rbf_of_sqdist(double s) { return exp(-0.5 * s); }
// rbf_of_sqdist for the tile mat-vec's generating role: the device library's exp written out --
// its constants and its order of operations (x log2e rounded to n, x - n ln2 in two fma, the
// degree-11 polynomial, ldexp by n) -- without its two range selects.  `x > 1024 ? inf` cannot
// fire for x = -0.5 s <= 0; `x < -1075 ? 0` is replaced by clamping x at -1075 first: there n =
// -1551 and ldexp gives +0, the select's value, and above it the select does nothing.  Domain:
// finite points, so s >= 0 or s = +inf (never NaN).  On that domain the bits are exp's
// (tests/test_gpu_rbf_exp_lean.py compares the two on the device); the kernels that store
// tiles, rows and columns keep calling exp, so no stored value can depend on this.
__device__ __forceinline__ double rbf_exp_c(unsigned long long bits) {
  return __builtin_bit_cast(double, bits);
}
//
// The sequence runs on s itself, without the multiply by -0.5.  Scaling by a power of two
// commutes with IEEE rounding (no intermediate or constant comes near the denormal range: the
// smallest coefficient is about 2.5e-8 * 2^-11), so with x = -0.5 s, R = -2 r and P_k =
// (-1/2)^k p_k the library's steps n = rint(x log2e), r = fma(-n, ln2_hi, x), r = fma(-n,
// ln2_lo, r), p_k = fma(r, p_{k+1}, c_k) become n = rint(s (-log2e / 2)), R = fma(n, 2 ln2_hi,
// s), R = fma(n, 2 ln2_lo, R), P_k = fma(R, P_{k+1}, (-1/2)^k c_k): every constant is the
// library's times an exact power of two (written beside it below), every intermediate the
// library's times an exact power of two, n and P_0 = p_0 the library's own.  The one place
// where the library's form rounds and this one does not is -0.5 s of a denormal s; n = 0 and
// the result 1.0 either way.  The clamp at x = -1075 is min(s, 2150) here.
// CLAMP false leaves it out: domain 0 <= s <= 2150, for the plain tiles of an operator whose
// point set is known to stay inside it (SymGen::noclamp); the same bits there.
template <bool CLAMP = true>
__device__ __forceinline__ double rbf_of_sqdist_lean(double s) {
  if constexpr (CLAMP) s = __builtin_fmin(s, 2150.0);
  // -log2e / 2 (log2e 0x3FF71547652B82FE)
  const double n = __builtin_rint(__dmul_rn(s, rbf_exp_c(0xBFE71547652B82FEull)));
  double r = fma(n, rbf_exp_c(0x3FF62E42FEFA39EFull), s);  // 2 ln2_hi (0x3FE62E42FEFA39EF)
  r = fma(n, rbf_exp_c(0x3C8ABC9E3B39803Full), r);         // 2 ln2_lo (0x3C7ABC9E3B39803F)
  // (-1/2)^11 c_11 (0x3E5ADE156A5DCB37), (-1/2)^10 c_10 (0x3E928AF3FCA7AB0C)
  double p = fma(r, rbf_exp_c(0xBDAADE156A5DCB37ull), rbf_exp_c(0x3DF28AF3FCA7AB0Cull));
  p = fma(r, p, rbf_exp_c(0xBE371DEE623FDE64ull));  // -2^-9 c_9 (0x3EC71DEE623FDE64)
  p = fma(r, p, rbf_exp_c(0x3E7A01997C89E6B0ull));  // 2^-8 c_8 (0x3EFA01997C89E6B0)
  p = fma(r, p, rbf_exp_c(0xBEBA01A014761F6Eull));  // -2^-7 c_7 (0x3F2A01A014761F6E)
  p = fma(r, p, rbf_exp_c(0x3EF6C16C1852B7B0ull));  // 2^-6 c_6 (0x3F56C16C1852B7B0)
  p = fma(r, p, rbf_exp_c(0xBF31111111122322ull));  // -2^-5 c_5 (0x3F81111111122322)
  p = fma(r, p, rbf_exp_c(0x3F655555555502A1ull));  // 2^-4 c_4 (0x3FA55555555502A1)
  p = fma(r, p, rbf_exp_c(0xBF95555555555511ull));  // -2^-3 c_3 (0x3FC5555555555511)
  p = fma(r, p, rbf_exp_c(0x3FC000000000000Bull));  // 2^-2 c_2 (0x3FE000000000000B)
  p = fma(r, p, -0.5);                              // -2^-1 c_1 (1.0)
  p = fma(r, p, 1.0);
  return __builtin_ldexp(p, (int)n);
}
__device__ __forceinline__ double rbf_value(const double (&xi)[8], const double *__restrict__ Xs,
                                            int64_t g, int d) {
  double s = 0.0;
#pragma unroll
  for (int t = 0; t < 8; ++t)
    if (t < d) s = rbf_sqdist_step(s, __dsub_rn(xi[t], Xs[g * d + t]), t == 0);
  return rbf_of_sqdist(s);
}

// The scipy stop test of iteration `it` (k_stoptest), done by every workgroup of the
// next iteration's first kernel instead of a launch of its own (rr_part == nullptr: none).
struct StopFold {
  const double *rr_part = nullptr;
  DevState *st = nullptr;
  double *trace = nullptr;
  long long it = 0;
};

// The CG update of the previous iteration (k_update_xr: alpha = rho / (p.q); x += alpha p;
// r -= alpha q; rr partials) folded into this iteration's one-pass low-rank apply: k_lr_rows
// forms r - alpha q on the fly, k_lr_fin writes x, r and the rr partials (x == nullptr: none)
struct XrFold {
  double *x = nullptr;
  double *r = nullptr;
  const double *p = nullptr;
  const double *q = nullptr;
  const double *pq_part = nullptr;
  double *rr_part = nullptr;
  DevState *st = nullptr;
};

// flags of the timing-only events (stamps read after a stream synchronisation): no
// system-scope fence, so recording one does not write back and invalidate the caches
// between the kernels it brackets (MLFF_EVENT_FENCE=1 restores the default, for A/B)
inline unsigned timing_event_flags() {
  static const unsigned f = std::getenv("MLFF_EVENT_FENCE") ? hipEventDefault
                                                            : hipEventDisableSystemFence;
  return f;
}

// What a timed segment of a PCG iteration brackets (pcg.hip mark_begin / mark_end): the operator,
// the low-rank preconditioner apply, a collective of the sharded iteration (one rank's stream),
// or the T r half that the ranks iteration issues ahead of the next apply -- its time goes to
// that apply, which is counted once, by its z half (kSegPrecon).  The first three index Timing::seg.
enum SegKind : int { kSegOperator = 0, kSegPrecon = 1, kSegComm = 2, kSegPreconTail = 3 };

struct Timing {
  bool on = false;
  int every = 1;        // bracket every `every`-th PCG iteration only (mlff_timing_enable)
  bool sample = true;   // the iteration being launched is bracketed
  std::vector<hipEvent_t> ev;  // pool, pairs (start, stop)
  size_t used = 0;             // events used in the current chunk
  struct Bucket {
    double ms = 0.0;
    int64_t count = 0;
  };
  Bucket seg[3];  // by SegKind: operator, preconditioner apply, collectives
  Bucket iter;    // whole chunks and the iterations completed in them
  Timing() = default;
  Timing(const Timing &) = delete;
  Timing &operator=(const Timing &) = delete;
  ~Timing() {
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
  }
};

// The context's stream and RCCL communicator, destroyed with the context (mlff_ctx: last).
struct StreamHandle {
  hipStream_t h = nullptr;
  StreamHandle() = default;
  StreamHandle(const StreamHandle &) = delete;
  StreamHandle &operator=(const StreamHandle &) = delete;
  ~StreamHandle() {
    if (h != nullptr) (void)hipStreamDestroy(h);
  }
  operator hipStream_t() const { return h; }
};
struct CommHandle {
  ncclComm_t h = nullptr;  // nulled by mlff_comm_abort
  CommHandle() = default;
  CommHandle(const CommHandle &) = delete;
  CommHandle &operator=(const CommHandle &) = delete;
  ~CommHandle() {
    if (h != nullptr) (void)ncclCommDestroy(h);
  }
  operator ncclComm_t() const { return h; }
};


// the search direction of the fused forms: p = z at ITER 1, else fma(beta, p_old, z)
// (k_update_p's arithmetic)
__device__ __forceinline__ double fused_p(double pold, double z, double beta, bool first) {
  return first ? z : fma(beta, pold, z);
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// xor-partner sum over the L lanes of a point with DPP moves (VALU, no LDS round trip):
// quad_perm [1,0,3,2] and [2,3,0,1] pair lanes 1 and 2 apart, row_half_mirror pairs every lane
// of a quad with one of the other quad of its 8 (each step adds a commutative pair: every lane
// of the group ends with the same bits)
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, false);
  return __hiloint2double(hi, lo);
}
template <int L>
__device__ __forceinline__ double group_sum(double v) {
  static_assert(L == 1 || L == 2 || L == 4 || L == 8, "DPP butterfly for L <= 8");
  if (L >= 2) v += dpp_f64<0xB1>(v);   // quad_perm(1, 0, 3, 2)
  if (L >= 4) v += dpp_f64<0x4E>(v);   // quad_perm(2, 3, 0, 1)
  if (L >= 8) v += dpp_f64<0x141>(v);  // row_half_mirror
  return v;
}

// Sum over a 256-thread block; result valid in thread 0.  Fixed order, so every
// workgroup that reduces the same values obtains the same bits.
__device__ __forceinline__ double block_sum256(double v, double *sh) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) sh[w] = v;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0) t = (sh[0] + sh[1]) + (sh[2] + sh[3]);
  return t;
}

// block_sum256 of two values at once (sh: 8 doubles), both sums valid in every thread
__device__ __forceinline__ void block_sum256_pair(double &a, double &b, double *sh) {
  a = wave_sum(a);
  b = wave_sum(b);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) {
    sh[w] = a;
    sh[4 + w] = b;
  }
  __syncthreads();
  a = (sh[0] + sh[1]) + (sh[2] + sh[3]);
  b = (sh[4] + sh[5]) + (sh[6] + sh[7]);
}

// Deterministic sum of np partials, broadcast to every thread of the block.
__device__ __forceinline__ double reduce_parts_bcast(const double *__restrict__ part, int np,
                                                     double *sh) {
  double v = 0.0;
  for (int i = threadIdx.x; i < np; i += 256) v += part[i];
  v = block_sum256(v, sh);
  __syncthreads();
  if (threadIdx.x == 0) sh[4] = v;
  __syncthreads();
  return sh[4];
}

// scipy's stop test of iteration f.it on the summed rr partials (k_stoptest); block (0, 0)
// writes the state.  True: the solver continues.
__device__ __forceinline__ bool stop_decide(const StopFold &f, double rr) {
  const double resid = sqrt(rr);
  DevState *st = f.st;
  int dec = ST_RUNNING;
  if (resid <= st->atol)
    dec = f.it > 1 ? ST_RECHECK : ST_CONVERGED;
  else if (f.it >= st->maxiter)
    dec = ST_MAXITER;
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
    st->rr = rr;
    st->resid = resid;
    st->iters = f.it;
    f.trace[f.it] = resid;
    if (dec != ST_RUNNING)
      st->status = dec;
    else
      st->rho1 = st->rho;
  }
  return dec == ST_RUNNING;
}

// reduce_parts_bcast for a workgroup of any multiple of 256 threads: the first 256 threads
// reduce the partials exactly as reduce_parts_bcast does (same bits), every thread gets it
__device__ __forceinline__ double reduce_parts_bcast_wide(const double *__restrict__ part, int np,
                                                          double *sh) {
  double v = 0.0;
  if (threadIdx.x < 256)
    for (int i = threadIdx.x; i < np; i += 256) v += part[i];
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0 && w < 4) sh[w] = v;
  __syncthreads();
  const double t = (sh[0] + sh[1]) + (sh[2] + sh[3]);
  __syncthreads();  // sh is reused by the caller
  return t;
}

// The same sum in two halves, so the loads can be issued long before the reduction:
// parts_thread_sum is the thread's share (the loop of reduce_parts_bcast), parts_bcast the
// block reduction of those shares (same bits as reduce_parts_bcast)
__device__ __forceinline__ double parts_thread_sum(const double *__restrict__ part, int np) {
  double v = 0.0;
  for (int i = threadIdx.x; i < np; i += 256) v += part[i];
  return v;
}
__device__ __forceinline__ double parts_bcast(double v, double *sh) {
  v = block_sum256(v, sh);
  __syncthreads();
  if (threadIdx.x == 0) sh[4] = v;
  __syncthreads();
  return sh[4];
}

}  // namespace mlff

namespace mlff {
struct LocalGroup;  // in-process transport (api.hip), see comm_allreduce
}

// The declaration order of the members is the teardown order, reversed: mlff_ctx_destroy sets
// the device, synchronises the stream and deletes, and C++ destroys the members last to first.
// So the stream, the local group and the communicator stand first (destroyed last: the
// communicator, then the group, then the stream), and every buffer and the timing events after
// them (released before the communicator, in no order that matters among themselves).
struct mlff_ctx {
  int device = 0, rank = 0, world = 1;
  int64_t N = 0;        // kernel size
  int64_t rows_per = 0; // ceil(N / world)
  int64_t row0 = 0, nrows = 0;
  int64_t blk = 0;      // padded local length (multiple of 64) = column block per rank
  int64_t ld = 0;       // world * blk: padded global length / K leading dimension
  mlff::StreamHandle stream;
  std::shared_ptr<mlff::LocalGroup> local;     // ranks as threads of one process
  mlff::CommHandle comm;                       // or: RCCL (one process per GPU)
  bool solo = false;                           // or: one rank alone (profiling, api.hip)

  // kernel matrix, blk rows x ld columns (padding rows/cols are zero)
  mlff::DevBuf<double> K;
  bool has_matrix = false;
  double sigma_K = 1.0, lam = 0.0;
  bool has_operator = false;
  bool K_symmetric = false;  // known symmetric by construction (generated / assembled)
  bool use_E_cstr = false;   // mlff_set_energy_constraints: sGDML systems of size 3 n M + M
  int storage = MLFF_STORAGE_AUTO;  // requested operator storage
  bool use_sym = false;             // resolved: symmetric tiles in use
  bool use_mf = false;              // resolved: matrix-free sGDML operator in use
  mlff::SymPack sym;
  mlff::MfData mf;                  // matrix-free sGDML operator (optional)
  mlff::RbfData rbf;                // synthetic RBF kernel from its points (optional)
  mlff::PredData pred;              // trained model for prediction (optional)

  // CG vectors.  local: blk entries; p_full / xg: ld entries (rank blocks)
  mlff::DevBuf<double> x, r, z, q, b;
  mlff::DevBuf<double> p_full, xg;
  mlff::DevBuf<double> gb; // world > 1: allgather buffer, world blocks of gstride
  int64_t gstride = 0;     // blk + kVecGrid (z block + its rho partials)
  mlff::DevBuf<double> part;  // partial sums: 3 * kMaxPart + tpart (k * S)
  mlff::DevBuf<mlff::DevState> st;
  mlff::PinBuf<mlff::DevState> h_st;  // pinned mirror
  mlff::DevBuf<double> trace;
  int64_t trace_cap = 0;
  bool pcg_active = false;
  int64_t pcg_done = 0;   // iterations known complete on the host side
  double tol = 0.0, bnorm = 0.0;

  mlff::LowRank lr;       // the preconditioner: z = sigma_p * (r - T^T T r) / lam
  // CG vector updates folded into the matrix-free nanotube iteration; read from
  // MLFF_FUSE_P / MLFF_FUSE_XR (=0: separate launches) when the context is created
  bool fuse_p = true, fuse_xr = true;
  bool cho_fast = true;  // cho_factor_stable: shifted Cholesky first inside builds (MLFF_CHO_FAST)
  bool pq_publish = false;       // MLFF_PQ_PUBLISH=1: the separate k_pq_publish launch (A/B)
  bool piv_persist_off = false;  // the persistent pivoted Cholesky timed out once (kernels_pivchol.hip)
  // Woodbury panel re-orthogonalised by a second CholeskyQR step (MLFF_WB_REFINE, woodbury_inplace;
  // configs[1] at full size: 571 -> 366 iterations, the oracle's 367) and the same for the
  // Nystrom panel (MLFF_NYS_REFINE)
  int wb_refine = 0;  // re-orthogonalisation steps (MLFF_WB_REFINE=1 / 2 ...; 0: the reference's one-step panel)
  // the Woodbury Gram matrices L^T L (and the refinement's T T^T): 0 the fp64 matrix-core GEMM,
  // 1 chunked double-double on the matrix cores, 2 exact products in double-double
  // (MLFF_WB_GRAM; kernels_dd.hip gram_wide_dd)
  int wb_gram_dd = 1;
  bool nys_refine = false;
  // exact-sum anchor (MLFF_EXACT_SUMS=1, kernels_dd.hip): dense-row operator and two-pass low-rank
  // apply with double-double dot products rounded once per entry; one rank; measurement only
  bool exact_sums = false;
  double last_lo_eig = 0.0;  // lo_eig of the last _cho_factor_stable (cho_factor_stable)
  bool cho_flipped = false;  // a cho_factor_stable retried upward after a noisy lo > 0
  bool eig_converged = true;   // last truncated eigensolve met kEigTol (kernels_eig.hip)
  double eig_rel_resid = 0.0;  // its worst Ritz residual / |theta_0|

  // pivoted Cholesky scratch
  mlff::DevBuf<int64_t> perm;  // global permutation (replicated)
  mlff::DevBuf<double> dwork;  // residual diagonal (local)
  mlff::DevBuf<int> pivflag;   // local rows already pivoted
  mlff::DevBuf<double> prow;   // L[m_pi, :m]
  std::vector<double> piv_col_s;  // device seconds per column of the last build
  double piv_woodbury_s = 0.0;    // its Woodbury build (G, chol, T)

  mlff::Timing timing;
  std::string err;
  bool aborted = false;  // mlff_comm_abort was called: every entry point fails

  // device scratch arena (ScratchScope / scratch_get): chunks, current chunk and offset
  struct ScratchChunk {
    mlff::DevBuf<char> p;
    size_t size;
  };
  std::vector<ScratchChunk> scratch_chunks;
  size_t scratch_cur = 0, scratch_off = 0;
  int scratch_depth = 0;  // open ScratchScopes
};

namespace mlff {

// ---- error helpers (api.hip) ------------------------------------------------
int set_error(mlff_ctx *ctx, int code, const std::string &msg);
int hip_check(mlff_ctx *ctx, hipError_t e, const char *what);
int nccl_check(mlff_ctx *ctx, ncclResult_t e, const char *what);

#define MLFF_HIP(ctx, call)                                   \
  do {                                                        \
    hipError_t e__ = (call);                                  \
    if (e__ != hipSuccess) return mlff::hip_check(ctx, e__, #call); \
  } while (0)
#define MLFF_NCCL(ctx, call)                                  \
  do {                                                        \
    ncclResult_t e__ = (call);                                \
    if (e__ != ncclSuccess) return mlff::nccl_check(ctx, e__, #call); \
  } while (0)
// every ABI entry point with a context: null check, then make the context's device
// current on the calling thread (one thread may drive contexts on several devices)
#define MLFF_ENTER(ctx)                                                        \
  do {                                                                         \
    if ((ctx) == nullptr) return mlff::set_error(nullptr, MLFF_ERR_ARG, "null ctx"); \
    if ((ctx)->aborted)                                                        \
      return mlff::set_error((ctx), MLFF_ERR_COMM, "communicator aborted (mlff_comm_abort)"); \
    (void)hipSetDevice((ctx)->device);                                         \
  } while (0)
#define MLFF_TRY(x)             \
  do {                          \
    int rc__ = (x);             \
    if (rc__ != MLFF_OK) return rc__; \
  } while (0)

// No C++ exception may cross the C ABI (ctypes would see std::terminate): every
// extern "C" body runs inside MLFF_API_BEGIN / MLFF_API_END(ctx), which maps
// std::bad_alloc to MLFF_ERR_NOMEM and anything else to MLFF_ERR_HIP, aborting the
// rank's in-process group so that its peers leave their collectives.
int api_exception(mlff_ctx *ctx, int code, const char *what);
#define MLFF_API_BEGIN try {
#define MLFF_API_END(ctx)                                                             \
  }                                                                                   \
  catch (const std::bad_alloc &) {                                                    \
    return mlff::api_exception((ctx), MLFF_ERR_NOMEM, "host allocation failed");      \
  }                                                                                   \
  catch (const std::exception &e__) {                                                 \
    return mlff::api_exception((ctx), MLFF_ERR_HIP, e__.what());                      \
  }                                                                                   \
  catch (...) {                                                                       \
    return mlff::api_exception((ctx), MLFF_ERR_HIP, "unknown C++ exception");         \
  }

// Device scratch of a build function, from the context's arena (mlff_ctx::scratch):
// a bump allocator over chunks allocated once and kept until mlff_ctx_destroy.  Every user runs on ctx->stream, so memory handed out again after a
// ScratchScope has closed is only touched by kernels ordered after the previous user's.
// (No stream-ordered allocator: its pools outlive the contexts' streams.)
struct ScratchScope {
  mlff_ctx *ctx;
  size_t chunk, off;
  explicit ScratchScope(mlff_ctx *c);
  ~ScratchScope();
  ScratchScope(const ScratchScope &) = delete;
  ScratchScope &operator=(const ScratchScope &) = delete;
};
// bytes (rounded up to 256) of scratch valid until the innermost open ScratchScope closes
int scratch_get(mlff_ctx *ctx, size_t bytes, void **out);
template <typename T>
int scratch_alloc(mlff_ctx *ctx, T **out, size_t count) {
  return scratch_get(ctx, sizeof(T) * (count > 0 ? count : 1), reinterpret_cast<void **>(out));
}

// ---- collectives (api.hip): RCCL, or the in-process transport ---------------
// sum-allreduce of n doubles in place (no-op on one rank)
int comm_allreduce(mlff_ctx *ctx, double *buf, size_t n);
// allgather: recv[r * count ...] = send of rank r; send may alias recv + rank * count
int comm_allgather(mlff_ctx *ctx, const double *send, double *recv, size_t count);

// ---- vector / GEMV kernels (kernels_vec.hip) ---------------------------------
// y = sigma * M v + lam * vloc  over `rows` rows of M (ld columns).
void launch_gemv_rows(const double *M, int64_t ld, int64_t rows, const double *v, double *y,
                      double sigma, double lam, const double *vloc, const int *status,
                      hipStream_t s);
// partial T GEMV: tpart[sp * k + j] = sum_{c in split sp} T[j, c] * r[c]
void launch_gemv_split(const double *T, int64_t ldt, int64_t k, int64_t ncols, int splits,
                       const double *r, double *tpart, const int *status, hipStream_t s,
                       StopFold fold = StopFold{});
int choose_tsplit(int64_t k, int64_t ncols);
// split factor of the apply's T^T t pass (choose_ksplit adjusted to fill whole waves)
int choose_zsplit(int64_t k, int64_t ncols);
// z = sigma_p/lam * (r - T^T t), t = sum_sp tpart; rho partials (r . z)
// (split-K over the k rows of T: zpart holds zsplit x ldt partial sums)
void launch_precon_z(const double *T, int64_t ldt, int64_t k, int splits, const double *tpart,
                     const double *r, double *z, int64_t n, double sigma_p, double lam_inv,
                     double *rho_part, const int *status, hipStream_t s, double *zpart,
                     int zsplit, StopFold fold = StopFold{});
// one-pass apply z = sigma_p/lam (r - T^T T r) with rho partials, one rank, for panels whose
// rows fit a workgroup's registers (lr_rows_fits); zpart: lr_rows_groups(k) x ldt scratch
bool lr_rows_fits(int64_t ldt);
int lr_rows_groups(int64_t k);
void launch_lr_apply_rows(const double *T, int64_t ldt, int64_t k, const double *r, double *z,
                          int64_t n, double sigma_p, double lam_inv, double *rho_part,
                          const int *status, hipStream_t s, double *zpart,
                          StopFold fold = StopFold{}, XrFold xf = XrFold{});
// the one-pass apply for long rows (clusters of lr_cluster_members(ldt) workgroups, one per
// CU, hand-offs of the per-row partial dots); lr_cluster_count = clusters resident at once
bool lr_cluster_fits(int64_t ldt);
int lr_cluster_members(int64_t ldt);
int lr_cluster_count(int64_t ldt, int device);
void launch_lr_apply_cluster(const double *T, int64_t ldt, int64_t k, int Q, const double *r,
                             double *z, int64_t n, double sigma_p, double lam_inv,
                             double *rho_part, const int *status, hipStream_t s, double *zpart,
                             unsigned long long *slots, unsigned epoch, int *fault,
                             StopFold fold = StopFold{});
// part[ks * ldw + c] = sum_{j in slice ks} W[j, c] * (sum_sp tsrc[sp * tstride + j])
void launch_colgemv_part(const double *W, int64_t ldw, int64_t k, const double *tsrc,
                         int tsplits, int64_t tstride, int ksplit, double *part,
                         const int *status, hipStream_t s, StopFold fold = StopFold{},
                         int64_t cached_rows = 0, const long long *tcol = nullptr,
                         const int *spec_hit = nullptr, int64_t spec_m0 = 0);
// C (M x N) = op(A) op(B) with K split over enough workgroups to fill the chip, the slices
// summed in a fixed order (deterministic); scratch from the context's arena
int gemm_splitk(mlff_ctx *ctx, bool ta, bool tb, int64_t M, int64_t N, int64_t K, const double *A,
                int64_t lda, const double *B, int64_t ldb, double *C, int64_t ldc);
int choose_ksplit(int64_t k, int64_t ncols);
// leading rows of a k x ldt panel read with default-policy (MALL-resident) loads
int64_t panel_cached_rows(int64_t k, int64_t ldt);
// rho partials of r . r (no preconditioner)
void launch_dot_part(const double *a, const double *b, int64_t n, double *part,
                     const int *status, hipStream_t s, StopFold fold = StopFold{});
// p = z + (rho/rho1) p   (p = z at iteration 1); rho = sum(rho_part)
void launch_update_p(const double *z, double *p, int64_t n, const double *rho_part,
                     DevState *st, long long it, const int *status, hipStream_t s);
// several ranks (gather buffer gb: rank blocks of gstride = blk + kVecGrid holding z_g
// and its rho partials): dst = r with r.r partials (no preconditioner);
// p_full = z_full + (rho/rho1) p_full with rho summed from all ranks' partials
void launch_copy_dot(const double *r, int64_t n, double *dst, double *part, const int *status,
                     hipStream_t s, StopFold fold = StopFold{});
void launch_update_p_gathered(const double *gb, int64_t gstride, int64_t blk, int world,
                              double *p_full, DevState *st, long long it, const int *status,
                              hipStream_t s);
// several ranks, symmetric tiles: pq = sum of the world shares; q = sigma y + lam p;
// alpha = rho/pq; x += alpha p; r -= alpha q; rr partials
void launch_update_xr_shares(double *x, double *r, const double *p, const double *y,
                             const double *shares, int world, int64_t n, double sigma, double lam,
                             double *rr_part, DevState *st, const int *status, hipStream_t s);
// kernels_dd.hip (MLFF_EXACT_SUMS): y = sigma fl(M v) + lam vloc with double-double row sums;
// z = sigma_p lam_inv (r - fl(T^T fl(T r))) with double-double dot products (t: k doubles)
void launch_dd_gemv_rows(const double *M, int64_t ld, int64_t rows, int64_t ncols, const double *v,
                         double *y, double sigma, double lam, const double *vloc, const int *status,
                         hipStream_t s);
void launch_dd_lowrank(const double *T, int64_t ldt, int64_t k, const double *r, double *z, int64_t n,
                       double sigma_p, double lam_inv, double *t, const int *status, hipStream_t s);
// G = W W^T (k x k, symmetric) of a wide k x ncols panel, each entry rounded once from a
// double-double sum: exact_products -- every product exact (correctly rounded but for ties);
// else 64-column chunks summed in fp64 on the matrix cores and the chunk partials added in
// double-double.  The Woodbury panel's Gram matrices (MLFF_WB_GRAM)
int gram_wide_dd(mlff_ctx *ctx, const double *W, int64_t k, int64_t ncols, int64_t ldw, double *G,
                 bool exact_products);
// pq = sum(pq_part); alpha = rho/pq; x += alpha p; r -= alpha q; rr partials
void launch_update_xr(double *x, double *r, const double *p, const double *q, int64_t n,
                      const double *pq_part, double *rr_part, DevState *st, const int *status,
                      hipStream_t s);
// rr -> resid, trace, status (scipy stop test)
void launch_stoptest(const double *rr_part, DevState *st, double *trace, long long it,
                     hipStream_t s);
// recheck: r = b - q, rr partials
void launch_residual(const double *b, const double *q, double *r, int64_t n, double *rr_part,
                     hipStream_t s);
void launch_recheck_finish(const double *rr_part, DevState *st, double *trace, hipStream_t s);
// sum of partials into a device double (1 workgroup)
void launch_reduce_to(const double *part, int np, double *out, hipStream_t s);
void launch_scale_copy(const double *a, double *y, int64_t n, double alpha, hipStream_t s);

// ---- dense linear algebra (kernels_dense.hip) -------------------------------
// C = alpha * op(A) op(B) + beta * C ; row-major; op(A): M x Kd, op(B): Kd x Nc
void launch_gemm(bool ta, bool tb, int64_t M, int64_t Nc, int64_t Kd, double alpha,
                 const double *A, int64_t lda, const double *B, int64_t ldb, double beta,
                 double *C, int64_t ldc, hipStream_t s);
// G = W W^T (k x k) over ncols columns of W (k x ncols, row stride ldw); split-K
// with a deterministic slab reduction; work: >= splits * k * k doubles
int syrk_wide(mlff_ctx *ctx, const double *W, int64_t k, int64_t ncols, int64_t ldw, double *G);
// G = A B^T (k x k) over ncols columns of the wide panels A, B (row stride ldw); split-K
// with a deterministic slab reduction (syrk_wide is gram_wide(W, W))
int gram_wide(mlff_ctx *ctx, const double *A, const double *B, int64_t k, int64_t ncols,
              int64_t ldw, double *G);
// in-place lower Cholesky of the k x k matrix A (row-major, ld = k)
// ok_out: report a matrix that is not positive definite there (MLFF_OK returned) instead of
// as MLFF_ERR_LINALG
int potrf_lower(mlff_ctx *ctx, double *A, int64_t k, bool *ok_out = nullptr);
// smallest eigenvalue of the lower triangle of a device m x m matrix (kernels_syev.hip:
// Householder tridiagonalisation + Sturm bisection, the eigh of _cho_factor_stable);
// d_host / e_host (optional): the tridiagonal
int sym_min_eig(mlff_ctx *ctx, const double *M, int64_t m, double *lo_eig, double *d_host,
                double *e_host);
// W <- L^-1 W, L k x k lower (ld = k), W k x ncols (row stride ldw)
int trsm_lower_wide(mlff_ctx *ctx, const double *L, int64_t k, double *W, int64_t ncols,
                    int64_t ldw);
void launch_add_diag(double *A, int64_t k, double v, hipStream_t s);
void launch_zero_upper(double *A, int64_t k, hipStream_t s);
// potrf_lower's steps on their own: the jb x jb diagonal block at (j0, j0) in one wave (err set
// on a non-positive pivot), the panel solve of the rows below it, and launch_gemm restricted
// to the tiles that touch the lower triangle of C
void launch_potrf_diag_wave(double *A, int64_t lda, int64_t j0, int jb, int *err, hipStream_t s);
void launch_trsm_panel(double *A, int64_t lda, int64_t k, int64_t j0, int jb, hipStream_t s);
void launch_gemm_tri(bool ta, bool tb, int64_t M, int64_t Nc, int64_t Kd, double alpha,
                     const double *A, int64_t lda, const double *B, int64_t ldb, double beta,
                     double *C, int64_t ldc, hipStream_t s);

// ---- closed-form dense solve (kernels_chol.hip) -------------------------------
// potrf_lower in a two-level order: its 64-wide steps inside a panel of MLFF_POTRF_OUTER
// columns (default 256; 64: potrf_lower's order), one trailing update per panel
int potrf_lower_blocked(mlff_ctx *ctx, double *A, int64_t n, bool *ok_out = nullptr);
// x <- L^-1 x and x <- L^-T x for a row-major lower factor (ld = n), one right-hand side
int trsv_lower_fwd(mlff_ctx *ctx, const double *L, int64_t n, double *x);
int trsv_lower_bwd(mlff_ctx *ctx, const double *L, int64_t n, double *x);
// (sigma_K K + shift I) x = b with the context's dense rows (one rank), host vectors;
// seconds_out (3, optional): copy / factor / solves
int dense_cho_solve(mlff_ctx *ctx, double sigma_K, double shift, const double *b_host,
                    double *x_host, double *seconds_out);
// test hook: lower factor of a host matrix, variant 0 potrf_lower / 1 potrf_lower_blocked
int test_potrf(mlff_ctx *ctx, const double *A_host, int64_t n, int variant, double *L_host,
               double *seconds_out);
// column sums of squares: out[c] = sum_j W[j, c]^2
void launch_colsumsq(const double *W, int64_t k, int64_t ncols, int64_t ldw, double *out,
                     hipStream_t s);

// ---- generators (kernels_gen.hip) -------------------------------------------
void launch_gen_rbf(double *K, int64_t ld, int64_t nrows, int64_t row0, int64_t rows_per,
                    int64_t blk, int64_t N, const double *Xs, int d, double jitter,
                    hipStream_t s);
void launch_diag_of(const double *K, int64_t ld, int64_t nrows, int64_t row0, int64_t rows_per,
                    int64_t blk, double sigma, double *out, hipStream_t s);
// gather columns idx (global) of the local rows: W[j, i] = sigma * K[i, pos(idx_j)]
void launch_gather_cols(const double *K, int64_t ld, int64_t nrows, const int64_t *idx,
                        int64_t k, int64_t rows_per, int64_t blk, double sigma, double *W,
                        int64_t ldw, hipStream_t s);
// Smm[j, j'] = W[j, idx_j' - row0] if idx_j' is local else 0
void launch_gather_mm(const double *W, int64_t ldw, const int64_t *idx, int64_t k,
                      int64_t row0, int64_t nrows, double *Smm, hipStream_t s);
// out[jc * ldo + r] = sigma K[row0 + r, col_jc] of the RBF source for the local rows;
// col_jc = cols[jc] (device, ncols) or, with cols == nullptr, st->m_pi
void launch_rbf_cols(const RbfData &rbf, int64_t N, int64_t row0, int64_t nrows,
                     const int64_t *cols, int64_t ncols, const DevState *st, double sigma,
                     double *out, int64_t ldo, hipStream_t s);
void launch_fill(double *y, int64_t n, double v, hipStream_t s);
int assemble_sgdml(mlff_ctx *ctx, const double *R_desc, const double *R_d_desc, int64_t M,
                   int n_atoms, const int32_t *perms, int n_perms, double sig);
int sgdml_descriptors(const double *R, int64_t M, int n_atoms, double *R_desc,
                      double *R_d_desc);
// kee[il * M + j] = sum_p Kee(sqrt5 |Rd_{i0+il} - Rd_j[P_p]|) (use_E_cstr, train.py:232-234)
void launch_sgdml_kee(const double *Rd, int64_t M, int64_t D, int64_t i0, int64_t ni,
                      const int32_t *Pt, int n_perms, double sig, double *kee, hipStream_t s);
// (r = i, s = j) point-pair records of the local points [i0, i0 + ni) (k_sgdml_uv, no mirror)
void launch_sgdml_records(const double *Rd, const double *Rdd, int64_t M, int n, int64_t D,
                          int64_t i0, int64_t ni, const int32_t *Pt, const int32_t *piinv,
                          int n_perms, double sig, double *uvk, hipStream_t s);
// out[jc * ldo + r] = sigma K_op[row0 + r, col_jc] for the local rows; col_jc = cols[jc]
// (device array, ncols entries) or, with cols == nullptr and ncols == 1, st->m_pi
void launch_sgdml_columns(const double *Rdd, int64_t M, int n, int64_t D, int64_t i0,
                          const int32_t *pi, const int32_t *piinv, int n_perms,
                          const double *uvk, int64_t row0, int64_t nrows, const int64_t *cols,
                          int64_t ncols, const DevState *st, double sigma, double *out,
                          int64_t ldo, hipStream_t s);

// ---- symmetric tiled operator (kernels_sym.hip) -----------------------------
// build the tiles this rank owns from the dense rows; check_symmetry compares
// every tile with its mirror (one rank only)
int sym_build(mlff_ctx *ctx, bool check_symmetry, bool *symmetric_out);
// The search-direction update of the sharded iteration (k_update_p_gathered: p = z + beta p,
// z and every rank's rho partials in the gather buffer gb) folded into the tile mat-vec: the
// tile workgroups form the operand entries they read, the slot reduction writes p (gb null:
// not fused)
struct PGather {
  const double *gb = nullptr;
  int64_t gstride = 0, blk = 0;
  int world = 1;
  DevState *st = nullptr;
  long long it = 0;
};
// test hook: lib_out[i] = rbf_of_sqdist(s[i]), lean_out[i] = rbf_of_sqdist_lean<clamp>(s[i])
// (device arrays; !clamp: every s[i] in [0, 2150])
void launch_rbf_exp_probe(const double *s, int64_t n, double *lib_out, double *lean_out, bool clamp,
                          hipStream_t st);
// P <- slot partials of K v_full over the stored tiles
void launch_symv(const SymPack &sp, const double *v_full, double *P, const int *status,
                 hipStream_t s, PGather pg = PGather{});
// one rank: y[i] = sum of the slots of row i (i < n_out); epilogue y = sigma y + lam vloc
void launch_sym_reduce(const SymPack &sp, int64_t n_out, double *y, bool epilogue, double sigma,
                       double lam, const double *vloc, const int *status, hipStream_t s);
// one rank, PCG: q = sigma (slot sums) + lam p over n_out rows, and the p.q partial sums
// of the kVecGrid workgroups into pq_part
void launch_sym_reduce_pq(const SymPack &sp, int64_t n_out, double *y, double sigma, double lam,
                          const double *p, double *pq_part, const int *status, hipStream_t s,
                          PGather pg = PGather{});
// several ranks: sp.yg = this rank's slot sums of every row (rank blocks of sp.ystride);
// with p_full: also this rank's share sigma p.y_g + lam ||p_loc||^2 published into the
// tail slot `rank` of every block (pq_part / pp_part: kVecGrid scratch each)
void launch_sym_reduce_ranks(const SymPack &sp, int rank, int world, int64_t blk,
                             const double *p_full, double *pq_part, double *pp_part,
                             double sigma, double lam, const int *status, hipStream_t s,
                             PGather pg = PGather{}, bool separate_publish = false);
// y = sigma * src + lam * vloc over n entries (src may alias y)
void launch_axpby_loc(const double *src, double *y, int64_t n, double sigma, double lam,
                      const double *vloc, const int *status, hipStream_t s);
// reduce-scatter (sum) of ld doubles into blk doubles per rank
int comm_reduce_scatter(mlff_ctx *ctx, const double *send, double *recv, size_t count);

// ---- matrix-free sGDML operator (kernels_mf.hip) ---------------------------
int mf_setup(mlff_ctx *ctx, const double *R_desc, const double *R_d_desc, int64_t M, int n_atoms,
             const int32_t *perms, int n_perms, double sig);
// pq_part != nullptr: also the x_loc . y_loc partials (kVecGrid, as launch_dot_part)
// the search-direction update p = z + (rho / rho1) p (k_update_p) fused into the
// matrix-free operator of a PCG iteration (x_full = x_loc = p_old on one rank)
struct PFuse {
  const double *z;
  const double *rho_part;
  DevState *st;
  long long it;
  StopFold sf;  // the previous iteration's stop test (after a folded k_update_xr), or none
};
bool mf_can_fuse_p(const mlff_ctx *ctx);
void launch_mf_operator(const mlff_ctx *ctx, const double *x_full, double *y_loc,
                        const double *x_loc, const int *status, double sigma, double lam,
                        double *pq_part = nullptr, const PFuse *pf = nullptr);
int mf_diag(mlff_ctx *ctx, double *out);
// Zt = (J_j x_j)[P_p] of every (j, p) (k_mf_z), status gated.  pf: the operand is the search
// direction p = z + beta p_old formed on the fly from xc = p_old (k_update_p's arithmetic, the
// same bits), and the previous iteration's stop test runs in its first workgroup (pf->sf)
void launch_mf_zt(const MfData &mf, const double *xc, const int *status, hipStream_t s,
                  const PFuse *pf = nullptr);
// pair-tile form (kernels_pt.hip): available for D <= 288; its (j, p) chunks, padded D and the
// operator y_loc = sigma K x + lam x_loc (+ the x_loc . y_loc partials when pq_part is set)
bool pt_supported(int64_t D);
int pt_chunks(int64_t D, int64_t ni, int64_t MP);
int64_t pt_padded_d(int64_t D);
// pf (one rank, every row here): the search-direction update fused (k_mf_z forms p on the fly,
// k_pt_fin writes it) and the previous iteration's stop test folded into k_mf_z
void launch_pt_operator(const MfData &mf, const double *Rt, const double *xc, int64_t row0,
                        int64_t nrows, const double *x_loc, double *y_loc, const int *status,
                        double sigma, double lam, double *pq_part, hipStream_t s,
                        const PFuse *pf = nullptr);
// operator form in use: 0 pair sums (k_mf_pair ...), 1 record-factored, 2 pair-tile
int mf_form(const mlff_ctx *ctx);
// sigma K_op columns through the single-column path (mf.uvk); false when it is not set up
bool mf_columns(const mlff_ctx *ctx, const int64_t *cols, int64_t ncols, double sigma,
                double *out, int64_t ldo);
// training-set energy pair terms for coefficients alphas (N, contiguous): ni x M n_perms
int mf_energies(mlff_ctx *ctx, const double *alphas, double *E_pairs_host);
// diag(sigma K) of this rank's rows: dense rows or the matrix-free sGDML data
int operator_diag(mlff_ctx *ctx, double *out);
int sgdml_diag(mlff_ctx *ctx, const double *dRd, const double *dRdd, int64_t M, int n,
               const int32_t *dP, const int32_t *perms_host, const int32_t *piinv_host,
               int n_perms, double sig, double *diag_out);
double mf_bytes(const mlff_ctx *ctx);
// modelled seconds of one application of the matrix-free operator in its form on this rank,
// from the rates measured on MI355X: the storage choice of MLFF_STORAGE_AUTO
double mf_seconds(const mlff_ctx *ctx);
int desc_perm_tables(mlff_ctx *ctx, const int32_t *perms, int n, int n_perms,
                     std::vector<int32_t> &Pt, std::vector<int32_t> &piinv);

// ---- prediction at new geometries (kernels_predict.hip) ----------------------
// hold a trained model (replaces the context's earlier one); MLFF_PRED_FORM / MLFF_PRED_SLAB
// are read here
int pred_set_model(mlff_ctx *ctx, const double *R_desc, const double *R_d_desc_alpha, int64_t M,
                   int n_atoms, const int32_t *perms, int n_perms, double sig, double std, double c);
// the model's energy coefficients alphas_E (M entries; use_E_cstr models), null to clear them:
// selects the constrained pair kernels
int pred_set_energy_coefficients(mlff_ctx *ctx, const double *alphas_E);
// E (Q), F (Q x 3 n) of the Q host geometries R, in slabs of pred.slab queries
int pred_run(mlff_ctx *ctx, const double *R, int64_t Q, double *E_out, double *F_out);
bool pred_tile_supported(int64_t D);
void pred_work(const PredData &pd, double *flops_per_query, double *bytes_per_query);
// upload nq <= pred.slab host geometries and run the descriptor stage and, with_fd, the pair and
// chunk-sum stages: pred.Rq, Rdq, Rddq (and Fd) of those queries are then on the device (in
// stream order)
int pred_fd_slab(mlff_ctx *ctx, const double *R, int64_t nq, bool with_fd);
// the stages of pred_fd_slab for the nq geometries already in pred.Rq, on stream s: any of the
// descriptors, the pair stage and the chunk sum, launched in this order
enum : int { kPrStageDesc = 1, kPrStagePair = 2, kPrStageSum = 4, kPrStageAll = 7 };
void pr_launch_fd(const PredData &pd, int64_t nq, int stages, hipStream_t s);

// ---- molecular dynamics with the held model (kernels_md.hip) ------------------
// n_steps velocity-Verlet steps of Q replicas; the work buffers are allocated by the first call
// (MLFF_MD_FRAMES is read there)
int md_run(mlff_ctx *ctx, const double *R0, const double *V0, const double *h, int64_t Q, double dt,
           int64_t n_steps, int64_t stride, bool want_forces, double *R_out, double *V_out,
           double *E_out, double *F_out);
// launches per step of the form a run would use, the frame capacity, the synchronisations of the
// last run; configures (no allocation) where no run has
int md_info(mlff_ctx *ctx, int *launches_per_step, int64_t *frame_capacity, int64_t *syncs_last_run);
// 0: the default form, 2 / 4: that many launches per step (2 needs a tile model)
int md_set_form(mlff_ctx *ctx, int launches);

// ---- Hessians of the held model (kernels_predict_hess.hip) -------------------
// H (Q x 3n x 3n) of the Q host geometries R; the slab buffers are allocated by the first call
// (MLFF_PRED_HESS_SLAB is read there)
int pred_hess_run(mlff_ctx *ctx, const double *R, int64_t Q, double *H_out);
void pred_hess_work(const PredData &pd, double *flops_per_query, double *bytes_per_query);

// ---- Hessian-vector products of the held model (kernels_predict_hvp.hip) ------
// HV (Q x K x 3n) = H(R_q) V[q][k] of the Q host geometries R and their K vectors each, H never
// formed; the slab buffers are allocated by the first call
int pred_hvp_run(mlff_ctx *ctx, const double *R, const double *V, int64_t Q, int64_t K, double *HV_out);
void pred_hvp_work(const PredData &pd, double *flops_per_product, double *bytes_per_query);

// ---- operator access for the builds and the PCG driver (api.hip) --------------
// require the operator and resolve its storage (builds the tiles if they are to be used)
int operator_prepare(mlff_ctx *ctx);
// y_loc = sigma_K K x over this rank's rows; x_loc = this rank's block (blk entries)
int operator_apply_local(mlff_ctx *ctx, const double *x_loc, double *y_loc);
// operator_prepare's two steps, for the PCG driver (pcg.hip)
int require_operator(mlff_ctx *ctx);
int resolve_storage(mlff_ctx *ctx);
// y_loc = sigma_K K v_full + lam v_loc over this rank's rows (status gated); pq_part: also the
// v_loc . y_loc partials of the CG step; pf: the fused search-direction update
int launch_operator(mlff_ctx *ctx, const double *v_full, double *y_loc, const double *v_loc,
                    const int *status, double *pq_part = nullptr, const PFuse *pf = nullptr);
// gather the rank blocks of an ld-long padded vector (in place)
int allgather_blocks(mlff_ctx *ctx, double *full);

// ---- low-rank preconditioner apply (pcg.hip) ----------------------------------
// the halves of the two-pass apply, and the apply in the form the build chose
int lowrank_tr(mlff_ctx *ctx, const double *r, const int *status, StopFold fold = StopFold{},
               bool reduce = true);
void lowrank_z(mlff_ctx *ctx, const double *r, double *z, double *rho, const int *status,
               StopFold fold = StopFold{});
int lowrank_apply(mlff_ctx *ctx, const double *r, double *z, double *rho, const int *status,
                  int *fault, StopFold fold = StopFold{}, XrFold xf = XrFold{});

// ---- eigen preconditioner (kernels_eig.hip) ----------------------------------
int eig_lowrank(mlff_ctx *ctx, int64_t k, int mask_mode, int64_t dim_i, double *Lt_out,
                double *evals_out, double *rowlev_out);
// eigenvalues (descending) of P_op A (preconditioned, the set low-rank preconditioner) or of
// A = sigma K + lam I: Iterative.solve(flag_eigvals=True) diagnostics, one rank
int spectrum(mlff_ctx *ctx, bool preconditioned, double *eig_out);
// test hook: C = alpha op(A) op(B) + beta C on the device from host arrays (splits > 1: the
// split-K slab path, returning C - alpha op(A) op(B) with beta = 1)
int test_gemm(mlff_ctx *ctx, int ta, int tb, int64_t M, int64_t Nc, int64_t Kd, double alpha,
              const double *A, int64_t lda, const double *B, int64_t ldb, double beta, double *C,
              int64_t ldc, int splits);

// ---- pivoted Cholesky (kernels_pivchol.hip) ---------------------------------
int pivoted_cholesky(mlff_ctx *ctx, int64_t k, int64_t *index_columns_out);

}  // namespace mlff
