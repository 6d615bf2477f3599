"""Molecule shapes, permutation sets and long-double references for the sGDML shape sweep
(tests/test_gpu_sgdml_shapes.py).  A plain module: no fixtures, no pytest hooks.

Every case is (n_atoms, M, kind) from CASES.  Its reference is the CPU oracle (oracle/sgdml.py,
pinned to the reference implementation's outputs in tests/test_oracle_golden.py) evaluated in
np.longdouble (x87, eps = 2^-63) from the long-double descriptors of the geometries; the GPU gets
the float64 roundings of those descriptors.  A GPU result is held to

    max|gpu - ref_ld| <= 10 band max|ref_ld|,

band = the largest deviation of the oracle's own float64 evaluations (from the same float64
inputs the GPU gets) from ref_ld, relative to max|ref_ld|, floored at 2^-52: the rule of
tests/golden/make_predict_golden.py, evaluated at run time.  The factor 10 is the project's
(tests/parity.py, tests/test_gpu_predict.py).  Everything is computed lazily, once per session.
"""
from __future__ import annotations

from functools import cached_property

import numpy as np

from oracle import sgdml as osg

LD = np.longdouble
assert np.finfo(LD).eps <= 2.0 ** -63, "np.longdouble is not an extended-precision type here"
SIG = 10.0
LAM = 1e-10
FLOOR = 2.0 ** -52
MIN_DIST = 0.7
PIVOT_GAP = 1e-9

# (n_atoms, M, kinds): the smallest shapes that reach each size-dependent branch of the kernels
TABLE = [
    (2, 1, ("id",)),                       # smallest legal size; M = 1: the diagonal block only
    (2, 5, ("id",)),
    (3, 4, ("id", "swap", "c3", "s3", "nongroup")),   # smallest with permutations
    (4, 33, ("id", "swap", "s3")),         # MP = 33 / 66 / 198 over the 32-row tile; 2 x 16 + 1 points
    (9, 1, ("id", "c3", "nongroup")),      # D = 36: capacity of pair-tile variant 0
    (9, 17, ("id", "c3", "nongroup")),     # more than one 16-point group
    (10, 3, ("id", "swap")),               # first D of variant 1
    (12, 5, ("id", "c3")),                 # D = 66: just above a 64-wide chunk; last D of variant 1
    (13, 3, ("id", "nongroup")),           # first D of variant 2
    (16, 3, ("id", "swap")),               # first D of variant 3
    (21, 3, ("id", "c3")),                 # 63 rows per point: one column chunk, one row short
    (22, 3, ("id", "c3", "nongroup")),     # 66 rows: two column chunks; first D of variant 4
    (24, 3, ("id", "swap")),               # last pair-tile D, D > 256, last prediction tile D
    (25, 3, ("id", "swap", "nongroup")),   # record-factored default; first prediction stream D
    (43, 2, ("id", "swap", "nongroup")),   # three column chunks; ragged 16-atom block
    (86, 2, ("id", "swap")),               # 3n = 258 > 256: second stride of the t < 3n loops
]
CASES = [(n, M, kind) for n, M, kinds in TABLE for kind in kinds]
GRID_STRIDE_DESC = (190, 2)                # D = 17955 > 64 * 256: the grid-stride step of k_desc

# Geometry seeds.  Default 1000 n + M; an entry here replaces it where the default draw leaves two
# of the first k pivots of the reference's pivoted Cholesky closer than PIVOT_GAP (relative), see
# Case.pivchol (checked on the CPU in tests/test_oracle_longdouble.py::test_sweep_pivots_separated).
SEEDS: dict[tuple[int, int], int] = {(3, 4): 803004}


def case_id(c):
    return f"n{c[0]}-M{c[1]}-{c[2]}"


def molecule(n_atoms, M, seed):
    """M geometries (M x n x 3) of a random compact molecule: a frame in the box of
    test_gpu_matfree._molecule plus 0.08 N(0, 1) displacements per geometry.  The frame is drawn
    atom by atom, an atom redrawn while it lies within 1.1 of an earlier one, and the whole draw
    repeated until no two atoms of any geometry are closer than MIN_DIST (an unfiltered draw has
    distances down to 0.2, and 1 / r^3 then spans four decades for no purpose)."""
    rng = np.random.default_rng(seed)
    half = 2.0 * (n_atoms / 9.0) ** (1.0 / 3.0)
    a, b = np.tril_indices(n_atoms, k=-1)
    while True:
        frame = np.empty((n_atoms, 3))
        for i in range(n_atoms):
            while True:
                p = rng.uniform(-half, half, 3)
                if i == 0 or np.min(np.linalg.norm(frame[:i] - p, axis=1)) >= 1.1:
                    break
            frame[i] = p
        R = frame[None] + 0.08 * rng.standard_normal((M, n_atoms, 3))
        if np.min(np.linalg.norm(R[:, a] - R[:, b], axis=2)) >= MIN_DIST:
            return R


def perm_set(n_atoms, kind):
    """Permutation sets on atoms 0, 1, 2 (n_perms x n_atoms).  `nongroup` = {e, (0 1), (0 1 2)}
    is not closed: the reference's K_op and its mirrored assembly differ there."""
    e = np.arange(n_atoms)
    if kind == "id":
        return e[None, :].copy()
    if n_atoms < 3:
        raise ValueError("permutation sets other than 'id' need n_atoms >= 3")

    def on(first3):
        p = e.copy()
        p[:3] = first3
        return p

    sets = {"swap": [(0, 1, 2), (1, 0, 2)],
            "c3": [(0, 1, 2), (1, 2, 0), (2, 0, 1)],
            "s3": [(0, 1, 2), (1, 0, 2), (0, 2, 1), (2, 1, 0), (1, 2, 0), (2, 0, 1)],
            "nongroup": [(0, 1, 2), (1, 0, 2), (1, 2, 0)]}
    return np.array([on(t) for t in sets[kind]])


def _rel(v, ref):
    top = np.max(np.abs(ref)) if ref.size else LD(0)
    if top == 0:
        return 0.0
    return float(np.max(np.abs(np.asarray(v, dtype=LD) - ref)) / top)


def descriptor_bands(R, desc_ld):
    """((band of R_desc, band of R_d_desc), (their scales)) per entry -- descriptor entries are
    not sums: the float64 oracle from R against the long-double descriptors.  R_desc relative to
    each entry; an entry (r_a - r_b)_c / r^3 of R_d_desc relative to its pair's |r_a - r_b| / r^3
    = R_desc^2 (a component near zero has no relative accuracy in any evaluation)."""
    scales = (np.abs(desc_ld[0]), np.broadcast_to((desc_ld[0] ** 2)[:, :, None], desc_ld[1].shape))
    bands = tuple(max(FLOOR, float(np.max(np.abs(v.astype(LD) - ref) / sc)))
                  for v, ref, sc in zip(osg.descriptors(R), desc_ld, scales))
    return bands, scales


class Case:
    def __init__(self, n_atoms, M, kind):
        self.n, self.M, self.kind = n_atoms, M, kind
        self.D = n_atoms * (n_atoms - 1) // 2
        self.n3 = 3 * n_atoms
        self.N = self.n3 * M
        self.group = kind != "nongroup"
        self.perms = perm_set(n_atoms, kind)
        self.tpl = osg.tril_perms_lin(self.perms)
        self.sig = LD(SIG)
        self.label = case_id((n_atoms, M, kind))
        # the molecule and the vectors do not depend on the permutation set
        self.seed = SEEDS.get((n_atoms, M), 1000 * n_atoms + M)
        xe = np.random.default_rng(self.seed + 7).standard_normal(self.N + M)
        xe.setflags(write=False)
        self.xE = xe                       # [x_F; x_E]
        self.x = xe[:self.N]
        # original index -> index in the system with the training points reversed
        self._idx = np.concatenate([np.arange(self.N).reshape(M, self.n3)[::-1].ravel(),
                                    self.N + np.arange(M)[::-1]])

    # ------------------------------------------------------------------ inputs
    @cached_property
    def R(self):
        R = molecule(self.n, self.M, self.seed)
        R.setflags(write=False)
        return R

    @cached_property
    def desc_ld(self):
        return osg.descriptors(self.R.astype(LD), dtype=LD)

    @cached_property
    def desc(self):
        """float64 roundings of the long-double descriptors: the GPU's inputs."""
        Rd, Rdd = (np.ascontiguousarray(a.astype(np.float64)) for a in self.desc_ld)
        Rd.setflags(write=False)
        Rdd.setflags(write=False)
        return Rd, Rdd

    # ------------------------------------------------------------------ evaluations
    def _eval(self, q, dtype, rev=False):
        """Quantity q from the long-double descriptors (dtype = LD) or from their float64
        roundings (float64); rev: training points in reversed order, the result un-reversed."""
        Rd, Rdd = self.desc_ld if dtype is LD else self.desc
        sig = self.sig if dtype is LD else SIG
        idx, N = self._idx, self.N
        xE = self.xE
        if rev:
            Rd, Rdd, xE = Rd[::-1], Rdd[::-1], xE[idx]
        x = xE[:N]
        if q == "KE":
            out = osg.assemble_kernel(Rd, Rdd, self.tpl, sig, use_E_cstr=True, dtype=dtype)
            return out[np.ix_(idx, idx)] if rev else out
        if q == "Kop":
            out = osg.kernel_matvec_matrix_free(Rd, Rdd, self.perms, sig, x, dtype=dtype)
        elif q == "Kop_factored":
            out = osg.kernel_matvec_factored(Rd, Rdd, self.perms, sig, x, dtype=dtype)
        elif q == "KopE":
            out = osg.kernel_matvec_matrix_free(Rd, Rdd, self.perms, sig, xE, use_E_cstr=True,
                                                dtype=dtype)
        elif q == "diagE":
            out = osg.kernel_diag(Rd, Rdd, self.perms, sig, use_E_cstr=True, dtype=dtype)
        elif q == "E":
            out = osg.energies_matrix_free(Rd, Rdd, self.perms, sig, x, dtype=dtype)
            return out[::-1] if rev else out
        else:
            raise KeyError(q)
        return out[idx[:out.size]] if rev else out

    @cached_property
    def _ref(self):
        return {}

    @cached_property
    def _evals(self):
        return {}

    def ref(self, q):
        """Long-double reference.  K and diag are the force block of KE and diagE (the same
        sums: the border is appended to them); diagK / diagKE are the diagonals of the assembled
        K / KE (what an assembled context returns for a non-group permutation set)."""
        if q not in self._ref:
            N = self.N
            if q == "K":
                v = self.ref("KE")[:N, :N]
            elif q == "diag":
                v = self.ref("diagE")[:N]
            elif q == "diagKE":
                v = np.diag(self.ref("KE")).copy()
            elif q == "diagK":
                v = self.ref("diagKE")[:N]
            else:
                v = self._eval(q, LD)
            assert v.dtype == LD
            v.setflags(write=False)
            self._ref[q] = v
        return self._ref[q]

    def evals(self, q):
        """The oracle's float64 evaluations of q: as is and with the training points reversed;
        for K_op x also the record-factored regrouping (no energy constraints) and, for a
        permutation group, the assembled K times x.  The reference's assembly mirrors the blocks
        i >= j, so for a non-group set the reversed assembly is another matrix: left out."""
        if q not in self._evals:
            N = self.N
            if q in ("K", "diag", "diagK"):
                src = {"K": "KE", "diag": "diagE", "diagK": "diagKE"}[q]
                v = [a[:N, :N] if a.ndim == 2 else a[:N] for a in self.evals(src)]
            elif q == "diagKE":
                v = [np.diag(a).copy() for a in self.evals("KE")]
            elif q == "KE":
                v = [self._eval(q, np.float64)]
                if self.group:
                    v.append(self._eval(q, np.float64, rev=True))
            else:
                v = [self._eval(q, np.float64), self._eval(q, np.float64, rev=True)]
                if q == "Kop":
                    v.append(self._eval("Kop_factored", np.float64))
                    if self.group:
                        v.append(self.evals("K")[0] @ self.x)
                if q == "KopE" and self.group:
                    v.append(self.evals("KE")[0] @ self.xE)
            self._evals[q] = v
        return self._evals[q]

    def band(self, q, part=None):
        """max|v64 - ref_ld| / max|ref_ld| over the float64 evaluations, floored at 2^-52.
        part: a function that cuts the same block out of every array (the energy border's
        blocks are held against their own maxima)."""
        cut = part if part is not None else (lambda a: a)
        ref = cut(self.ref(q))
        return max([FLOOR] + [_rel(cut(v), ref) for v in self.evals(q)])

    # ------------------------------------------------------------------ descriptors
    @cached_property
    def desc_band(self):
        return descriptor_bands(self.R, self.desc_ld)[0]

    # ------------------------------------------------------------------ columns
    @property
    def rank(self):
        """rank K = M (3 n - 6) (3 n - 5 for two atoms: the force is invariant under the rigid
        motions), capped by M D."""
        return self.M * min(self.D, self.n3 - (6 if self.n > 2 else 5))

    @property
    def k_piv(self):
        """Pivoted-Cholesky rank of the column test: 8 where K has that many independent
        columns (pivots past rank K are rounding noise of either sign)."""
        return min(8, self.N, self.rank)

    def column(self, g, dtype):
        Rd, Rdd = self.desc_ld if dtype is LD else self.desc
        sig = self.sig if dtype is LD else SIG
        key = (g, dtype is LD)
        if key not in self._cols:
            self._cols[key] = osg.kernel_column_matrix_free(Rd, Rdd, self.perms, sig, g, dtype=dtype)
        return self._cols[key]

    @cached_property
    def _cols(self):
        return {}

    @cached_property
    def pivchol(self):
        """oracle.precon.pivoted_cholesky of S = -K_op to rank k_piv, in float64, on
        (a) the float64 columns and diagonal and (b) the long-double ones rounded to float64.
        Returns (ref, piv_b, band, gap): (b) is the reference, ref = L_b (N x k) and
        band = max|L_a - L_b| / max|L_b| floored at 2^-52 -- for two and three atoms, where rows
        tie exactly (`tie_class`), the same of the tie-independent L L^T (N x N, long-double
        product).  gap = the smallest relative distance, over the k steps, between the pivot and
        the largest other entry of the running diagonal that is not its exact tie."""
        from oracle.precon import pivoted_cholesky

        k = self.k_piv
        runs = []
        for dtype, dq in ((np.float64, self.evals("diag")[0]), (LD, self.ref("diag"))):
            def get_col(g, dtype=dtype):
                c = -self.column(g, dtype).astype(np.float64)
                c[g] += LAM
                return c

            runs.append(pivoted_cholesky(get_col, -np.asarray(dq, dtype=np.float64), k))
        (La, pa), (Lb, pb) = runs
        assert np.array_equal(self.tie_class(pa[:k]), self.tie_class(pb[:k])), (self.label, pa[:k], pb[:k])
        d = -np.asarray(self.ref("diag"), dtype=np.float64)
        gap = np.inf
        for m in range(k):
            rest = pb[m:]
            cur = d[rest] - np.sum(Lb[rest, :m] ** 2, axis=1)
            tie = ((self.tie_class(rest) == self.tie_class(rest[:1]))
                   & (np.abs(cur - cur[0]) <= 0.1 * PIVOT_GAP * cur[0]))
            if not np.all(tie):
                gap = min(gap, float((cur[0] - np.max(cur[~tie])) / cur[0]))
        if self.ties:
            a, ref = (X.astype(LD) @ X.T.astype(LD) for X in (La, Lb))
        else:
            assert np.array_equal(pa[:k], pb[:k]), (self.label, pa[:k], pb[:k])
            a, ref = La, Lb
        return ref, pb, max(FLOOR, _rel(a, np.asarray(ref, dtype=LD))), gap

    @property
    def ties(self):
        return self.n <= 3

    def tie_class(self, g):
        """Rows that can tie exactly with row g.  The forces of a geometry sum to zero, so the n
        rows (j, a, c) of one point and one coordinate sum to the zero row; once all but two of
        them are pivots, the Schur complements of the last two are each other's negatives, their
        running diagonal entries the same number, and either is a legitimate next pivot that
        gives the same L L^T.  With two or three atoms that happens within the first pivots, so
        there the pivots are compared as (point, coordinate) classes; otherwise row by row."""
        g = np.asarray(g)
        if self.ties:
            return (g // self.n3) * 3 + g % 3
        return g


_CACHE: dict[tuple[int, int, str], Case] = {}


def case(n_atoms, M, kind):
    key = (n_atoms, M, kind)
    if key not in CASES:
        raise KeyError(key)
    if key not in _CACHE:
        _CACHE[key] = Case(*key)
    return _CACHE[key]


def band(c, quantity, part=None):
    return c.band(quantity, part)


def held(gpu, ref_ld, band, label, scale=None):
    """Print `label`, the largest deviation of gpu from ref_ld, the bound 10 band max|ref_ld| and
    their ratio, then assert deviation <= bound.  scale: what the band is relative to instead of
    max|ref_ld| (an array of the result's shape: a bound per entry, figures then relative)."""
    ref_ld = np.asarray(ref_ld, dtype=LD)
    gpu = np.asarray(gpu)
    assert gpu.shape == ref_ld.shape, (label, gpu.shape, ref_ld.shape)
    assert np.all(np.isfinite(gpu)), label
    err = np.abs(gpu.astype(LD) - ref_ld)
    if scale is None:
        top = np.max(np.abs(ref_ld)) if ref_ld.size else LD(0)
        dev, bound = float(np.max(err)) if err.size else 0.0, float(10 * LD(band) * top)
    else:
        dev, bound = float(np.max(err / scale)), 10 * float(band)
    ratio = dev / bound if bound > 0 else (0.0 if dev == 0 else np.inf)
    print(f"shape-sweep {label}: dev={dev:.3e} bound={bound:.3e} band={band:.3e} ratio={ratio:.3f}")
    assert dev <= bound, (label, dev, bound)
    return ratio
