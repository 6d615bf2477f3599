"""Shapes, inputs and long-double references for the preconditioner-build sweep
(tests/test_gpu_precon_shapes.py; checked on the CPU in tests/test_oracle_precon_longdouble.py).
A plain module: no fixtures, no pytest hooks.

Every build works on S = sigma_K K.  Its reference is oracle/precon.py evaluated in np.longdouble
on the long-double S; the GPU gets the float64 rounding of that S (or the points / descriptors it
is made from).  A GPU result is held by sgdml_shapes.held to

    max|gpu - ref_ld| <= 10 band max|ref_ld|,

band = the largest deviation from ref_ld, relative to max|ref_ld|, of the oracle's own float64
evaluations from the float64 S, floored at 2^-52.  Two evaluations per quantity: as is, and with
the rows and columns of S reversed (every sum over rows runs backwards; the Schur sums of the
pivoted Cholesky run backwards; the Nystrom block S_mm is factored in the opposite order).  The
discrete decisions -- the pivot order and the sign of the 1e-15 shift of cho_factor_stable -- are
taken once, from the long-double data rounded to float64, and handed to every evaluation.

Compared quantities are basis-free (L L^T, the projector T^T T, z = P r, scores, eigenvalues), so
neither a row sign nor an order inside a tie matters.  Everything is computed lazily, once per
session.
"""
from __future__ import annotations

from functools import cached_property

import numpy as np

from oracle import precon as op
from tests import sgdml_shapes as sh
from tests.sgdml_shapes import FLOOR, LD, PIVOT_GAP, SIG, held  # noqa: F401  (held: re-export)

LAMS = (1e-4, 1e-10)          # 1e-10 is the project's own; r - T^T T r cancels there
LENGTH_SCALE = 0.5            # at 0.2 pivots tie exactly between far-apart points
JITTER = 1e-10
MIN_SMM_EIG = 1e-12           # Nystrom variant 0 / lev_scores: the 1e-15 shift's sign is not a rounding matter
EIG_GAP = 1e-3                # (|l_k| - |l_k+1|) / |l_1| where the rank-k subspace is compared
EIG_DECAY = 0.5               # |l_b+1| / |l_k| of the subspace iteration

COLUMN = ("pivL", "wood", "lowrank", "nys0", "nys1", "lev")
PIV = ("pivL", "wood", "lowrank")

# (input, k, builds, sources, note).  input: ("rbf", N) the RBF kernel of rbf_points(N, 3, N) at
# length scale 0.5 + 1e-10 I; ("spd", N) / ("indef", N) a host matrix Q diag(w) Q^T with
# prescribed eigenvalues, condition 1e3; ("sgdml", n_atoms, M, perms) S = -K of sgdml_shapes.
# sources: "host" set_matrix; "points" gen_rbf (columns by launch_rbf_cols); "rows" gen_rbf, then
# get_matrix_rows, which forms the dense rows (columns by the gather); "matfree" sgdml_operator
# (the single-column kernel); "assembled" assemble_sgdml.  The smallest shapes that reach each
# branch of the builds:
TABLE = [
    (("rbf", 1), 1, COLUMN, ("host", "points"), "alloc_panel: 7 pad rows of 8, 63 pad columns of 64"),
    (("rbf", 2), 2, COLUMN, ("host", "points"), "k = N = 2"),
    (("rbf", 63), 7, COLUMN, ("host",), "one row and one column short of the pads"),
    (("rbf", 64), 8, COLUMN, ("host",), "exactly one 64-column pad, one 8-row pad"),
    (("rbf", 65), 9, COLUMN + ("spectrum",), ("host", "points", "rows"),
     "first column / row of a second pad; the three column sources"),
    (("rbf", 129), 63, COLUMN, ("host",), "one row short of a potrf / trsm step; VALU GEMM (k < 64)"),
    (("rbf", 129), 64, COLUMN, ("host",), "one full potrf / trsm step; first matrix-core k x N product"),
    (("rbf", 129), 65, COLUMN + ("spectrum",), ("host", "points"),
     "first row of a second potrf / trsm step; Nystrom index sets"),
    (("rbf", 200), 127, COLUMN, ("host",), "one row short of BM = 128"),
    (("rbf", 200), 128, COLUMN, ("host",), "first BM = 128 workgroup tile"),
    (("rbf", 257), 130, COLUMN, ("host",), "Gram matrix of more than one 128-tile"),
    (("rbf", 1025), 130, COLUMN, ("host", "points"), "three 512-column Gram slabs: the slab sum"),
    (("rbf", 512), 81, PIV, ("host",), "k > 80 but 512 rows: no speculation"),
    (("rbf", 513), 81, COLUMN, ("host", "points"), "first speculative block; Nystrom index sets"),
    (("rbf", 600), 97, PIV, ("host",), "a second speculative block, one step long"),
    (("rbf", 129), 129, PIV, ("host",), "k = N on the RBF kernel: smallest pivot 7e-9"),
    (("spd", 64), 64, COLUMN, ("host",), "k = N: L L^T = S; Nystrom of all columns"),
    (("spd", 129), 129, COLUMN, ("host",), "k = N past one potrf step"),
    (("sgdml", 4, 12, "swap"), 24, COLUMN, ("matfree", "assembled"),
     "sigma_K = -1; the single-column kernel and the gather from the assembled rows"),
    (("sgdml", 4, 12, "swap"), 40, PIV, ("matfree",),
     "pivots down to 1.2e-7 of the first (S_mm of 40 random columns is singular to 1e-12: no Nystrom)"),
]
PERSIST = [(("rbf", 512), 81), (("rbf", 513), 81), (("rbf", 600), 97)]    # MLFF_PIVCHOL_PERSIST = 1 and 0
INDEX_SETS = {(("rbf", 129), 65): ("rand", "first", "ends"),
              (("rbf", 513), 81): ("rand", "first", "ends")}

# Eigen build: (input, k, source, mask_mode, unique, note).  unique: |l_k| - |l_k+1| >= EIG_GAP |l_1|
# (or k = N), so the projector and the row norms of U_k are compared; otherwise evals and z only.
EIG_TABLE = [
    (("rbf", 2), 2, "host", 0, True, "k = N = 2"),
    (("spd", 64), 64, "host", 0, True, "k = N: the full Jacobi path"),
    (("spd", 129), 129, "host", 0, True, "k = N: the full Jacobi path"),
    (("rbf", 65), 9, "host", 0, True, "b = 25, 2 b < N: shifted CholeskyQR3 subspace iteration"),
    (("indef", 129), 40, "host", 0, True,
     "b = 60, 2 b < N; eigenvalues of both signs, a negative one among the k largest |l|"),
    (("indef", 129), 49, "host", 0, True, "2 b = 146 >= N: the full path for k < N"),
    (("sgdml", 3, 20, "id"), 45, "matfree", 0, False,
     "b = 67 > rank K = 60, full off: S Q exactly rank-deficient, the Cholesky retry "
     "(l_45 = 1.3e-10 l_1, gap 2e-11: evals and z only)"),
    (("sgdml", 3, 20, "id"), 45, "assembled", 2, False,
     "mask mode 2, dim_i = 9, against the oracle's masked matrix"),
    # (("rbf", 513), 81): removed.  (l_81 - l_82) / l_1 = 2.0e-7 at length scale 0.5, so neither
    # the projector nor the row norms are defined to rounding, and its long-double
    # eigen-decomposition alone takes 40 s.  W = 3 runs on ("indef", 129) instead.
]

# Sharded runs: (input, k, worlds); builds wood, nys0, lev (and eig where EIG_TABLE has the pair)
SHARDED = [
    (("rbf", 65), 9, (2, 3, 5)),       # ragged row blocks: 33 + 32, 22 + 22 + 21, 13 x 5
    (("rbf", 2), 2, (5,)),             # ranks with no rows
    (("rbf", 513), 81, (3,)),          # k > 80 with 171 local rows: no speculation on any rank
    (("indef", 129), 40, (3,)),        # the eigen build only
]


def label(inp, k):
    return "-".join(str(x) for x in inp) + f"-k{k}"


def lam_id(lam):
    return f"lam{lam:g}"


def _rel(v, ref):
    return sh._rel(v, ref)


def _gram(T):
    """T^T T (N x N) of a k x N panel, the product formed in long double."""
    T = np.asarray(T, dtype=LD)
    return T.T @ T


def flip(a):
    """Reverse every axis of length N (rows and columns of S, entries of a vector)."""
    return a[::-1, ::-1] if a.ndim == 2 else a[::-1]


def prescribed_spectrum(kind, N):
    """Eigenvalues of the host matrices, condition 1e3.  'spd': geometric from 1 to 1e-3.
    'indef' (N = 129): 40 values linear from 1 to 0.5, then geometric from 0.4 to 1e-3, every third
    negative: |l| distinct, l_39 < 0, (|l_40| - |l_41|) / |l_1| = 0.1, |l_61| / |l_40| = 0.2,
    and at k = 49 a gap of 1.5e-2."""
    if kind == "spd":
        return np.geomspace(1.0, 1e-3, N)
    w = np.concatenate([np.linspace(1.0, 0.5, 40), np.geomspace(0.4, 1e-3, N - 40)])
    w[2::3] *= -1.0
    return w


def atomic_mask(K64, dim_i):
    """Entries zeroed by 'eigvec_precon_atomic_interactions' (iterative_solver.py:1238-1253):
    |K| below the largest |K|, outside the same-atom 3 x 3 blocks of every pair of points."""
    a = (np.arange(K64.shape[0]) % dim_i) // 3
    return (np.abs(K64) < np.abs(K64).max()) & (a[:, None] != a[None, :])


class Problem:
    """One (input, k): S in both precisions, the discrete decisions, references and bands."""

    def __init__(self, inp, k, mask_mode=0):
        self.inp, self.k, self.mask_mode = inp, int(k), mask_mode
        self.kind = inp[0]
        self.label = label(inp, k) + ("-mask2" if mask_mode else "")
        self.sigma_K = -1.0 if self.kind == "sgdml" else 1.0
        self._cache = {}

    # ------------------------------------------------------------------ inputs
    @cached_property
    def mol(self):
        return sh.Case(*self.inp[1:])

    @cached_property
    def X(self):
        N = self.inp[1]
        X = np.random.default_rng(N).random((N, 3))      # synthetic.rbf_points(N, 3, N)[0]
        X.setflags(write=False)
        return X

    @cached_property
    def S_ld(self):
        if self.kind == "rbf":
            X = self.X.astype(LD) / LD(LENGTH_SCALE)
            d = np.sum((X[:, None, :] - X[None, :, :]) ** 2, axis=2)
            S = np.exp(LD(-0.5) * d)
            S[np.diag_indices_from(S)] = LD(1) + LD(JITTER)
        elif self.kind in ("spd", "indef"):
            N = self.inp[1]
            Q = np.linalg.qr(np.random.default_rng(7000 + N).standard_normal((N, N)))[0]
            S = (Q * prescribed_spectrum(self.kind, N)) @ Q.T
            S = ((S + S.T) / 2).astype(LD)               # the float64 matrix is the input: exact
        else:
            S = -self.mol.ref("K")
            assert self.mol.group
        if self.mask_mode == 2:
            S = S.copy()
            S[atomic_mask(S.astype(np.float64), self.mol.n3)] = 0
        S.setflags(write=False)
        return S

    @cached_property
    def S64(self):
        S = np.ascontiguousarray(self.S_ld.astype(np.float64))
        S.setflags(write=False)
        return S

    @property
    def N(self):
        return self.S_ld.shape[0]

    @cached_property
    def vectors(self):
        """The residuals z = P r is compared at: one Gaussian, e_0 and e_{N-1}."""
        N = self.N
        r = np.zeros((3, N))
        r[0] = np.random.default_rng(31 * N + self.k).standard_normal(N)
        r[1, 0] = r[2, N - 1] = 1.0
        r.setflags(write=False)
        return r

    def idx(self, which="rand"):
        """Sorted Nystrom column sets: random; the first k columns; one with both 0 and N - 1."""
        N, k = self.N, self.k
        rng = np.random.default_rng(17 * N + k)
        if k == N or which == "first":
            return np.arange(k)
        if which == "ends":
            return np.sort(np.concatenate([[0, N - 1], 1 + rng.choice(N - 2, k - 2, replace=False)]))
        return np.sort(rng.choice(N, k, replace=False))

    # ------------------------------------------------------------------ discrete decisions
    @cached_property
    def pivots(self):
        """(pivots (k,), smallest relative gap to the runner-up, smallest pivot / largest).
        Pivots: the float64 oracle on the float64 S.  Gap and pivots' sizes: the long-double
        run with those pivots; step 0 of an RBF kernel (all diagonal entries equal: the
        first-maximum rule, index 0) and a last step without runner-up are left out of the gap."""
        S64, S, k, N = self.S64, self.S_ld, self.k, self.N
        _, order = op.pivoted_cholesky(lambda i: S64[:, i], np.diag(S64).copy(), k)
        piv = order[:k].copy()
        L, order_ld = op.pivoted_cholesky(lambda i: S[:, i], np.diag(S).copy(), k, dtype=LD, pivots=piv)
        assert np.array_equal(order, order_ld)
        d = np.diag(S)
        gap, sizes = np.inf, []
        for m in range(k):
            rest = order[m:]
            cur = d[rest] - np.sum(L[rest, :m] ** 2, axis=1)
            sizes.append(float(cur[0]))
            if rest.size > 1 and not (m == 0 and self.kind == "rbf"):
                gap = min(gap, float((cur[0] - np.max(cur[1:])) / cur[0]))
        if self.kind == "rbf":
            assert piv[0] == 0 and np.all(d == d[0])
        return piv, gap, min(sizes) / max(sizes)

    @cached_property
    def spectrum_abs(self):
        """|eigenvalues| of the long-double S, descending (float64 roundings)."""
        return np.sort(np.abs(op.eigh_longdouble(self.S_ld)[0]))[::-1].astype(np.float64)

    def smm_min_eig(self, which="rand"):
        idx = self.idx(which)
        return float(op.eigh_longdouble(self.S_ld[np.ix_(idx, idx)])[0][0])

    # ------------------------------------------------------------------ evaluations
    def _factor(self, dtype, rev):
        key = ("L", dtype is LD, rev)
        if key not in self._cache:
            S = self.S_ld if dtype is LD else self.S64
            piv = self.pivots[0]
            if rev:
                S, piv = flip(S), self.N - 1 - piv
            L, _ = op.pivoted_cholesky(lambda i: S[:, i], np.diag(S).copy(), self.k, dtype=dtype,
                                       pivots=piv, reverse=rev)
            self._cache[key] = L                          # in the evaluation's own row order
        return self._cache[key]

    def _panel_out(self, T, sp, lam, dtype, rev):
        r = self.vectors[:, ::-1] if rev else self.vectors
        z = np.stack([op.apply_panel(T, sp, lam, ri, dtype=dtype) for ri in r])
        P = _gram(T)
        return {"proj": flip(P) if rev else P, "z": z[:, ::-1] if rev else z, "T": T}

    def evaluate(self, build, lam, dtype, rev=False, which="rand"):
        """The quantities of one build, {name: array}, in the original row order."""
        S = self.S_ld if dtype is LD else self.S64
        N, k = self.N, self.k
        if rev:
            S = flip(S)
        un = (lambda a: flip(a)) if rev else (lambda a: a)
        if build == "pivL":
            L = self._factor(dtype, rev).astype(LD)
            return {"LLt": un(L @ L.T)}
        if build in ("wood", "lowrank"):
            T, sp = op.woodbury_panel(self._factor(dtype, rev), lam, dtype=dtype)
            return self._panel_out(T, sp, lam, dtype, rev)
        if build in ("nys0", "nys1", "lev"):
            idx = self.idx(which)
            if rev:
                idx = np.sort(N - 1 - idx)
            if build == "lev":
                return {"scores": un(op.lev_scores(S[:, idx], idx, lam, dtype=dtype, signs=(-1, -1)))}
            T, sp = op.nystrom_panel(S[:, idx], idx, lam, int(build[-1]), dtype=dtype, signs=(-1, -1))
            return self._panel_out(T, sp, lam, dtype, rev)
        if build == "eig":
            key = ("svd", dtype is LD, rev)
            if key not in self._cache:
                self._cache[key] = op._svd_symmetric(S, dtype)
            U, s = self._cache[key]
            T, sp = op.woodbury_panel((U * np.sqrt(s))[:, :k], lam, dtype=dtype)
            out = self._panel_out(T, sp, lam, dtype, rev)
            out["evals"] = s[:k].copy()
            out["rowlev"] = un(np.sqrt(np.sum(U[:, :k] ** 2, axis=1)))
            return out
        if build == "spectrum":
            T = self.evaluate("wood", lam, dtype, rev)["T"]
            P = (np.eye(N, dtype=dtype) - np.asarray(T.T @ T, dtype=dtype)) / dtype(lam)
            return {"spectrum_P": op.spectrum(S, lam, P, dtype=dtype),
                    "spectrum_A": op.spectrum(S, lam, None, dtype=dtype)}
        raise KeyError(build)

    def ref(self, build, lam, which="rand"):
        build = "wood" if build == "lowrank" else build     # the same panel, from a given factor
        key = ("ref", build, lam, which)
        if key not in self._cache:
            out = self.evaluate(build, lam, LD, which=which)
            for v in out.values():
                assert v.dtype == LD
                v.setflags(write=False)
            self._cache[key] = out
        return self._cache[key]

    def evals(self, build, lam, which="rand"):
        build = "wood" if build == "lowrank" else build
        key = ("evals", build, lam, which)
        if key not in self._cache:
            self._cache[key] = [self.evaluate(build, lam, np.float64, rev, which) for rev in (False, True)]
        return self._cache[key]

    def band(self, build, lam, name, which="rand", part=None):
        cut = part if part is not None else (lambda a: a)
        ref = cut(self.ref(build, lam, which)[name])
        return max([FLOOR] + [_rel(cut(e[name]), ref) for e in self.evals(build, lam, which)])

    def factor_ref(self):
        """The long-double factor L (N x k) of the reference's pivots: the input of `lowrank`."""
        return self._factor(LD, False)


_CACHE: dict = {}


def problem(inp, k, mask_mode=0):
    key = (inp, k, mask_mode)
    if key not in _CACHE:
        _CACHE[key] = Problem(inp, k, mask_mode)
    return _CACHE[key]


Z_NAMES = ("gauss", "e0", "eN")


def rows(build):
    """[(input, k, source)] of TABLE for one build."""
    return [(inp, k, src) for inp, k, builds, sources, _ in TABLE if build in builds for src in sources]


def check_z(z, p, build, lam, which, tag):
    """Hold the three applies, each against its own maximum; returns the ratios."""
    ref = p.ref(build, lam, which)["z"]
    assert z.shape == ref.shape, (tag, z.shape, ref.shape)
    out = []
    for i, name in enumerate(Z_NAMES):
        b = p.band(build, lam, "z", which, part=lambda a, i=i: a[i])
        out.append(held(z[i], ref[i], b, f"{tag} z/{name}"))
    return out
