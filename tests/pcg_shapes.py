"""Systems, stop cases and long-double references for the PCG-iteration sweep
(tests/test_gpu_pcg_shapes.py; every condition is checked on the CPU in
tests/test_oracle_pcg_longdouble.py).  A plain module: no fixtures, no pytest hooks.

A system is A = S + lam I with S = sigma_K K of precon_shapes.problem(inp, k) and
b = default_rng(N).standard_normal(N); its preconditioner is none (k = 0) or the Woodbury panel
of the long-double pivoted-Cholesky factor (the device gets precon_lowrank of that factor's
float64 rounding: no pivot decision enters).  The reference is oracle.pcg.cg_legacy in
np.longdouble on the long-double S; the float64 evaluations that define a band are the same
oracle in float64 on the float64 S, as is and with rows and columns reversed (every dot product,
mat-vec and apply sums backwards).  A device result is held by sgdml_shapes.held to 10 x that
band.  Everything is computed lazily, once per session.

Table A (smooth regime): J iterations at tol = 0.  Table B: the discrete stop decisions of
scipy 1.7.3, each with a 5 % margin on both sides of atol in every evaluation.
"""
from __future__ import annotations

from functools import cached_property

import numpy as np

from oracle import precon as op
from oracle.pcg import cg_legacy
from tests import precon_shapes as ps
from tests.sgdml_shapes import FLOOR, LD, SIG, held  # noqa: F401  (held, SIG: re-export)

BAND_X = 1e-10                # conditions on every Table A case (the factor 10 of `held` is fixed)
BAND_TRACE = 1e-8
TRACE_FLOOR = 1e-6            # long-double trace[J] >= TRACE_FLOOR trace[0]
MARGIN = 0.05                 # Table B: ||r_{m-1}|| >= 1.05 atol, ||r_m|| <= 0.95 atol
SGDML_COND = 100.0

# ---------------------------------------------------------------- Table A
# (input, k, lam, J).  k = 0: no preconditioner.  Host matrices ("spd", N): the double2 tails,
# one 256-thread block +- 1, one 512 tile +- 1, two tiles + 1; J is capped at N - 1 below N = 64
# and is 1 at N = 1 (where the residual after the first iteration is zero: see `converges_at_1`).
HOST_K = {1: 1, 2: 1, 63: 7, 64: 8, 65: 9, 255: 31, 257: 33, 511: 40, 512: 40, 513: 40, 1025: 40}
HOST_LAM = 1e-3
TABLE_A = [(("spd", N), k, HOST_LAM, max(1, min(8, N - 1))) for N, kN in HOST_K.items() for k in (0, kN)]
TABLE_A += [
    (("rbf", 65), 0, 1e-2, 8), (("rbf", 65), 9, 1e-2, 8),         # points: the generated tiles
    (("rbf", 513), 0, 1e-3, 6), (("rbf", 513), 81, 1e-3, 6),
]
# sGDML, A = -K + lam I, lam = |l_1| / (SGDML_COND - 10) so that cond(A) <= SGDML_COND:
# (case, k, J without / with the preconditioner, MLFF_MF_FORM, operator form, p update fused
# into the operator).  K has few eigenvalues above lam, so the solves are short: J is the last
# iteration whose long-double residual is still above TRACE_FLOOR (k = 24 on (9, 17, "c3")
# reaches 5e-15 in 8 iterations, k = 8 on (3, 4, "swap") 3e-11 in 2: k 8 and 4 there).
SGDML_A = [
    ((25, 3, "id"), 24, 8, 8, None, "rec", True),      # record-factored with the fused p update
    ((25, 3, "swap"), 24, 8, 8, None, "rec", False),   # record-factored, not fusable
    ((9, 17, "c3"), 8, 8, 8, None, "pt", True),        # pair-tile
    ((4, 33, "swap"), 4, 5, 3, None, "pt", True),      # pair-tile
    ((3, 4, "swap"), 4, 4, 2, "pair", "pair", False),  # pair sums
]
# energy constraints: N = 3 n M + M, the long-double KE; (case, k, J without / with)
ECSTR_A = ((9, 17, "id"), 4, 5, 5)   # J = 7 without: band of x 1e-9
RANKS_A = [(("spd", 65), 9, (2, 3)), (("spd", 513), 40, (2, 3)), (("spd", 2), 1, (5,))]
RANKS_SGDML = ((9, 17, "c3"), 8, 3)

# ---------------------------------------------------------------- Table B
# The stop cases run on three systems: (name, input, k, lam, m).  m: the iteration at which the
# B4 solve converges; its tol is derived from the long-double residual curve (System.tol_for).
# The host system is the condition-10 matrix of B6 (("spd", N) at condition 1e3 does not converge
# in 12 iterations without a preconditioner).
B_SYSTEMS = {
    "host": (("b6", 257), 0, None, 8),
    "host-lr": (("b6", 257), 33, None, 8),
    "sgdml-pt": (("sgdml", 9, 17, "c3"), 8, None, 8),
}
B6_N = 65
B6_LAM = 0.05                 # folded into the spectrum: A = Q diag(geomspace(1, 0.1, N)) Q^T
B6_KS = {65: 9, 257: 33}      # rank of the preconditioned forms
B6_K = B6_KS[B6_N]
# (input, k, tol).  Without a preconditioner the issue's measured case (j* = 55); with k = 9 the
# two float64 orders give ||r_50|| = 1.05e-11 and 3.1e-11, no margin at 1e-11: atol between
# ||r_51|| and ||r_52||; the sGDML system (b, x0 drawn the same way) falls tenfold per iteration
# there: atol between ||r_24|| (5.8e-12, 9.6e-12) and ||r_25|| (4.8e-13, 2.1e-13)
B6_CASES = {
    "none": (("b6", B6_N), 0, 1e-11),
    "lr": (("b6", B6_N), B6_K, 4e-12),
    "sgdml-pt": (("sgdml", 9, 17, "c3"), 8, 1.5e-12),
}
B6_X0_SCALE = 1e8
B6_MORE = 4                   # maxiter = j* + B6_MORE


def sys_id(inp, k):
    return "-".join(str(x) for x in inp) + (f"-k{k}" if k else "-none")


def _rel(v, ref):
    return ps._rel(v, ref)


class Run:
    """One oracle solve, in the system's original row order."""

    def __init__(self, x, info, trace, iters, record, un):
        self.x, self.info, self.iters = un(x), int(info), int(iters)
        self.trace = np.asarray(trace)
        self.xs = [un(v) for v in record["x"]]
        self.recheck = record["recheck"]
        self.callbacks = record["callbacks"]


class B6Problem(ps.Problem):
    """The host matrix of the failing-recheck case: S = Q diag(w - lam) Q^T, so that
    A = S + lam I has the spectrum w = geomspace(1, 0.1, N) (condition 10)."""

    def __init__(self, N, k, lam):
        super().__init__(("b6", N), k)
        self.fold = lam

    @cached_property
    def S_ld(self):
        N = self.inp[1]
        rng = np.random.default_rng(7000 + N)
        Q = np.linalg.qr(rng.standard_normal((N, N)))[0]
        S = (Q * (np.geomspace(1.0, 0.1, N) - self.fold)) @ Q.T
        S = ((S + S.T) / 2).astype(LD)                   # the float64 matrix is the input: exact
        S.setflags(write=False)
        self.b = rng.standard_normal(N)
        self.b /= np.linalg.norm(self.b)
        self.x0 = B6_X0_SCALE * rng.standard_normal(N) / np.sqrt(N)
        return S


class ECstrProblem(ps.Problem):
    """sGDML with energy constraints: S = -KE, N = 3 n M + M (the long-double KE of sgdml_shapes)."""

    def __init__(self, case, k):
        super().__init__(("sgdmlE",) + tuple(case), k)
        self.sigma_K = -1.0

    @cached_property
    def S_ld(self):
        S = -self.mol.ref("KE")
        S.setflags(write=False)
        return S


class System:
    """A = S + lam I of one problem, its preconditioner and its oracle solves."""

    def __init__(self, p, k, lam):
        self.p, self.k = p, int(k)
        self.lam = float(lam) if lam is not None else self._sgdml_lam()
        self.label = ps.label(p.inp, k) if k else "-".join(str(x) for x in p.inp) + "-none"
        self._cache = {}

    def _sgdml_lam(self):
        """|l_1| / (SGDML_COND - 10) from the float64 eigenvalues of the long-double S rounded
        (a long-double Jacobi run of N = 459 takes half a minute and moves |l_1| by 1e-16),
        rounded to three digits: cond(A) <= (|l_1| + lam) / lam = SGDML_COND - 9."""
        top = float(np.max(np.abs(np.linalg.eigvalsh(self.p.S64))))
        return float(f"{top / (SGDML_COND - 10):.3e}")

    @property
    def N(self):
        return self.p.N

    @property
    def sigma_K(self):
        return self.p.sigma_K

    @cached_property
    def b(self):
        b = np.random.default_rng(self.N).standard_normal(self.N)
        b.setflags(write=False)
        return b

    @cached_property
    def Lt64(self):
        """The device's input of precon_lowrank: float64 rounding of the long-double factor (k x N)."""
        Lt = np.ascontiguousarray(self.p.factor_ref().astype(np.float64).T)
        Lt.setflags(write=False)
        return Lt

    # ------------------------------------------------------------------ operators
    def operators(self, dtype, rev=False):
        """(matvec, psolve) in dtype; rev: of the system with rows and columns reversed."""
        key = ("ops", dtype is LD, rev)
        if key not in self._cache:
            S = self.p.S_ld if dtype is LD else self.p.S64
            S = ps.flip(S) if rev else S
            lam = dtype(self.lam)
            psolve = None
            if self.k:
                L = self.p.factor_ref() if dtype is LD else self.Lt64.T
                T, sp = op.woodbury_panel(L[::-1] if rev else L, self.lam, dtype=dtype)
                psolve = lambda r: op.apply_panel(T, sp, self.lam, r, dtype=dtype)  # noqa: E731
            self._cache[key] = ((lambda v: S @ v + lam * v), psolve)
        return self._cache[key]

    def A_ld(self):
        return self.p.S_ld + LD(self.lam) * np.eye(self.N, dtype=LD)

    def residual_ld(self, x, b=None):
        """b - A x in long double, from any x."""
        b = self.b if b is None else b
        return np.asarray(b, dtype=LD) - self.operators(LD)[0](np.asarray(x, dtype=LD))

    def precon_ld(self, r):
        psolve = self.operators(LD)[1]
        r = np.asarray(r, dtype=LD)
        return r if psolve is None else psolve(r)

    # ------------------------------------------------------------------ solves
    def solve(self, dtype, rev=False, b=None, x0=None, tol=0.0, maxiter=None):
        matvec, psolve = self.operators(dtype, rev)
        un = (lambda v: v[::-1].copy()) if rev else (lambda v: v)
        b = self.b if b is None else b
        b = np.asarray(b, dtype=dtype)
        x0 = None if x0 is None else np.asarray(x0, dtype=dtype)
        if rev:
            b, x0 = b[::-1], (None if x0 is None else x0[::-1])
        rec = {"callbacks": 0}

        def cb(_x):
            rec["callbacks"] += 1

        x, info, trace, it = cg_legacy(matvec, b, x0=x0, tol=tol, maxiter=maxiter, psolve=psolve,
                                       callback=cb, dtype=dtype, record=rec)
        rec.setdefault("x", [x])
        rec.setdefault("recheck", [])
        assert x.dtype == np.dtype(dtype) and trace.dtype == np.dtype(dtype)
        return Run(x, info, trace, it, rec, un)

    def runs(self, name, **kw):
        """(long-double run, [float64 run as is, float64 run reversed]) of one named solve."""
        if name not in self._cache:
            self._cache[name] = (self.solve(LD, **kw), [self.solve(np.float64, rev, **kw) for rev in (False, True)])
        return self._cache[name]

    def bands(self, name, **kw):
        """(band of the last iterate relative to max|x|, band of the trace per entry)."""
        ref, evals = self.runs(name, **kw)
        bx = max([FLOOR] + [_rel(e.x, ref.x) for e in evals])
        bt = FLOOR
        for e in evals:
            assert e.trace.shape == ref.trace.shape
            with np.errstate(divide="ignore", invalid="ignore"):
                d = np.abs(e.trace.astype(LD) - ref.trace) / ref.trace
            bt = max(bt, float(np.max(np.where(ref.trace == 0, LD(0), d))))
        return bx, bt

    # ------------------------------------------------------------------ Table A
    def smooth(self, J):
        return self.runs(("A", J), tol=0.0, maxiter=J)

    def smooth_bands(self, J):
        return self.bands(("A", J), tol=0.0, maxiter=J)

    # ------------------------------------------------------------------ Table B
    def tol_for(self, m, b=None, x0=None, name="curve"):
        """tol that puts atol at the geometric mean of the long-double ||r_{m-1}|| and ||r_m||
        (the recurrence residuals of a tol = 0 run), rounded to two digits."""
        key = ("tol", name, m)
        if key not in self._cache:
            t = self.solve(LD, b=b, x0=x0, tol=0.0, maxiter=m).trace
            bn = np.sqrt(np.sum(np.asarray(self.b if b is None else b, dtype=LD) ** 2))
            self._cache[key] = float(f"{float(np.sqrt(t[m - 1] * t[m]) / bn):.1e}")
        return self._cache[key]


_SYSTEMS: dict = {}


def system(inp, k, lam=None):
    key = (inp, k, lam)
    if key not in _SYSTEMS:
        if inp[0] == "b6":
            p = _SYSTEMS.setdefault(("p", inp), B6Problem(inp[1], B6_KS[inp[1]], B6_LAM))
            lam = B6_LAM
        elif inp[0] == "sgdmlE":
            p = _SYSTEMS.setdefault(("p", inp), ECstrProblem(inp[1:], ECSTR_A[1]))
        else:
            p = ps.problem(inp, k or _table_k(inp))       # k = 0: the same S as the table's k > 0
        _SYSTEMS[key] = System(p, k, lam)
    return _SYSTEMS[key]


def _table_k(inp):
    ks = [k for i, k, _, _ in TABLE_A if i == inp and k] + \
         [k for c, k, *_ in SGDML_A if ("sgdml",) + c == inp] + \
         [k for i, k, _, _ in B_SYSTEMS.values() if i == inp and k]
    return ks[0] if ks else 1


def sgdml_system(case, k):
    return system(("sgdml",) + tuple(case), k, None)


def b_system(name):
    inp, k, lam, m = B_SYSTEMS[name]
    return system(inp, k, lam), m


def converges_at_1(s):
    """N = 1: x_1 = b / a up to rounding, so r_1 = 0 wherever alpha q rounds to b; 0 <= atol = 0
    passes at ITER 1 without a recheck.  True when all three evaluations give exactly 0."""
    ref, evals = s.smooth(1)
    return all(r.trace[1] == 0 for r in [ref] + evals)


# ---------------------------------------------------------------- Table B cases
def b2_inputs(s):
    """||b|| = 100, x0 = x* + d with ||A d|| = 1e-5, tol 1e-6: resid0 = 1e-5 > tol, atol = 1e-4."""
    A = s.A_ld()
    b = s.b.astype(LD)
    b = (b * (100 / np.sqrt(b @ b))).astype(np.float64)
    xs = np.linalg.solve(A.astype(np.float64), b)
    d = np.random.default_rng(s.N + 1).standard_normal(s.N)
    d *= 1e-5 / float(np.sqrt(np.sum((A @ d.astype(LD)) ** 2)))
    return b, xs + d, 1e-6


def b3_inputs(s):
    """b with r_1 = 0 up to rounding, tol 1e-8.  No preconditioner: the eigenvector of the float64 S
    with the largest eigenvalue.  With P: A P b = mu b, b = R u for A = R R^T and the top
    eigenvector u of R^T P R (then q = A P b is parallel to b = r_0), all in float64."""
    if not s.k:
        return np.ascontiguousarray(np.linalg.eigh(s.p.S64)[1][:, -1]), 1e-8
    A = s.p.S64 + s.lam * np.eye(s.N)
    T, _ = op.woodbury_panel(s.Lt64.T, s.lam)
    R = np.linalg.cholesky(A)
    u = np.linalg.eigh(R.T @ ((np.eye(s.N) - T.T @ T) / s.lam) @ R)[1][:, -1]
    b = R @ u
    return np.ascontiguousarray(b / np.linalg.norm(b)), 1e-8


def b6_system(name):
    inp, k, _ = B6_CASES[name]
    return system(inp, k)


def b6_inputs(s):
    """(b of norm 1, x0 = 1e8 N(0, 1) / sqrt(N), tol): the host matrix's from its own generator
    after Q, any other system's from default_rng(7000 + N)."""
    tol = next(t for i, k, t in B6_CASES.values() if (i, k) == (s.p.inp, s.k))
    if s.p.kind == "b6":
        s.p.S_ld                  # draws b and x0 from the matrix's generator
        return s.p.b, s.p.x0, tol
    if "b6in" not in s._cache:
        rng = np.random.default_rng(7000 + s.N)
        b = rng.standard_normal(s.N)
        s._cache["b6in"] = (b / np.linalg.norm(b), B6_X0_SCALE * rng.standard_normal(s.N) / np.sqrt(s.N))
    return s._cache["b6in"] + (tol,)


def b6_runs(s):
    """The float64 oracles (as is, reversed) of the failing-recheck case, maxiter = j* + B6_MORE;
    j* = the first recheck's iteration of the as-is run."""
    key = "b6"
    if key not in s._cache:
        b, x0, tol = b6_inputs(s)
        first = s.solve(np.float64, b=b, x0=x0, tol=tol, maxiter=400)
        assert first.recheck, "no recheck in 400 iterations"
        j = first.recheck[0][0]
        s._cache[key] = (j, [s.solve(np.float64, rev, b=b, x0=x0, tol=tol, maxiter=j + B6_MORE)
                             for rev in (False, True)])
    return s._cache[key]


def b6_compared(s):
    """Entries j < j* whose recurrence residual is compared to 1 %: those before the first one at
    which the oracle's own two float64 orders differ by more than 0.1 % (a tenth of the bound, the
    factor of `held`).  The rounding that x0 puts into r0 (1e-8) is amplified from there on: the
    orders differ by up to 80 % around ||r|| = 1e-7 and no evaluation is a reference, although
    single later entries agree by chance."""
    j, runs = b6_runs(s)
    apart = np.abs(runs[0].trace[:j] / runs[1].trace[:j] - 1) > 1e-3
    first = int(np.argmax(apart)) if apart.any() else j
    return np.arange(j) < first


def projection_residual(s, xs, j, b):
    """||z - [d_{j+1} d_j] c|| / ||z|| minimised over c, z = P (b - A x_j) in long double from the
    given x_j and d_i = x_i - x_{i-1}: p_{j+1} = z + beta p_j after a failed recheck at j."""
    z = s.precon_ld(s.residual_ld(xs[j], b))
    D = np.stack([np.asarray(xs[j + 1], dtype=LD) - np.asarray(xs[j], dtype=LD),
                  np.asarray(xs[j], dtype=LD) - np.asarray(xs[j - 1], dtype=LD)], axis=1)
    D = D / np.sqrt(np.sum(D * D, axis=0))
    G = D.T @ D                                           # 2 x 2 normal equations in long double
    y = D.T @ z
    det = G[0, 0] * G[1, 1] - G[0, 1] * G[1, 0]
    c = np.array([G[1, 1] * y[0] - G[0, 1] * y[1], G[0, 0] * y[1] - G[1, 0] * y[0]]) / det
    res = z - D @ c
    return float(np.sqrt(np.sum(res * res) / np.sum(z * z)))


def b6_projection_bound(s):
    """10 x the largest projection residual the float64 oracles get from their own iterates."""
    j, runs = b6_runs(s)
    b = b6_inputs(s)[0]
    return 10 * max(projection_residual(s, r.xs, j, b) for r in runs)
