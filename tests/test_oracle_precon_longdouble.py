"""The long-double evaluation of oracle/precon.py and the inputs of the preconditioner sweep
(tests/precon_shapes.py, tests/test_gpu_precon_shapes.py).  CPU only.

* the float64 defaults compute what they computed before the dtype keyword (same bits, on a slice
  of the reference's ethanol fixture; tests/golden/precon_float64_parent.npz holds those outputs);
* dtype=np.longdouble returns long double, agrees with float64 and carries bits below it;
* every input condition the sweep relies on holds for every table row (pivot gaps, pivot sizes,
  the Nystrom block's smallest eigenvalue, the eigenvalue gap and decay of the eigen build);
* sensitivity: with the float64 oracle standing in for the device, four subtly wrong results are
  rejected by `held` at the band of their case.
"""
import numpy as np
import pytest

from oracle import precon as op
from tests import precon_shapes as ps
from tests.conftest import load_golden
from tests.precon_shapes import LAMS, LD, held

TABLE_IDS = [ps.label(r[0], r[1]) for r in ps.TABLE]


def test_float64_default_is_the_parents(golden_dir):
    f = load_golden(golden_dir, "precon_float64_parent")
    S = np.ascontiguousarray(-np.asarray(load_golden(golden_dir, "sgdml_ethanol_n270_perms")["K"])[:81, :81])
    k, lam, idx = int(f["k"]), float(f["lam"]), f["idx"]
    L, order = op.pivoted_cholesky(lambda i: S[:, i], np.diag(S).copy(), k)
    T = op.woodbury_panel(L, lam)[0]
    got = {"L": L, "order": order, "T_wood": T,
           "B0": op.nystrom_panel(S[:, idx], idx, lam, 0)[0],
           "B1": op.nystrom_panel(S[:, idx], idx, lam, 1)[0],
           "cho": op.cho_factor_stable(S[np.ix_(idx, idx)])[0],
           "lev": op.lev_scores(S[:, idx], idx, lam),
           "T_svd": op.svd_panel(S, k, lam)[0],
           "rowlev": op.rank_k_lev_scores(S, k),
           "z": op.apply_panel(T, 1.0, lam, S[:, 3].copy())}
    for name, v in got.items():
        assert v.dtype == f[name].dtype, name
        assert np.array_equal(v, f[name]), name
    # the keyword spelled out is the default
    assert np.array_equal(op.nystrom_panel(S[:, idx], idx, lam, 0, dtype=np.float64)[0], got["B0"])
    assert np.array_equal(op.svd_panel(S, k, lam, dtype=np.float64)[0], got["T_svd"])


def _calls(p, lam):
    """{name: (function of dtype, (build, quantity, how the result becomes that quantity) or None)}.
    None: no band of its own (cho_factor_stable: a factor; it is held through nystrom_panel and
    lev_scores, which call it)."""
    k, N = p.k, p.N
    idx = p.idx()
    piv = p.pivots[0]
    r = p.vectors[0]

    def S(dtype):
        return p.S_ld if dtype is LD else p.S64

    def factor(dtype):
        return op.pivoted_cholesky(lambda i: S(dtype)[:, i], np.diag(S(dtype)).copy(), k, dtype=dtype,
                                   pivots=piv)[0]

    def exact(d):
        return op.precon_exact(S(d), "pivchol", lam, k=k, pivots=piv, dtype=d)

    same = lambda v: v                                                       # noqa: E731
    return {
        "pivoted_cholesky": (factor, ("pivL", "LLt", lambda L: ps._gram(L.T))),
        "woodbury_panel": (lambda d: op.woodbury_panel(factor(d), lam, dtype=d)[0], ("wood", "proj", ps._gram)),
        # (scipy's cho_factor leaves the other triangle as it found it)
        "cho_factor_stable": (lambda d: np.triu(op.cho_factor_stable(S(d)[np.ix_(idx, idx)], dtype=d,
                                                                      sign=-1)[0]), None),
        "nystrom_panel_0": (lambda d: op.nystrom_panel(S(d)[:, idx], idx, lam, 0, dtype=d, signs=(-1, -1))[0],
                            ("nys0", "proj", ps._gram)),
        "nystrom_panel_1": (lambda d: op.nystrom_panel(S(d)[:, idx], idx, lam, 1, dtype=d)[0],
                            ("nys1", "proj", ps._gram)),
        "apply_panel": (lambda d: op.apply_panel(op.woodbury_panel(factor(d), lam, dtype=d)[0], 1.0, lam, r,
                                                 dtype=d), ("wood", "z", same)),
        "lev_scores": (lambda d: op.lev_scores(S(d)[:, idx], idx, lam, dtype=d, signs=(-1, -1)),
                       ("lev", "scores", same)),
        "svd_panel": (lambda d: op.svd_panel(S(d), k, lam, dtype=d)[0], ("eig", "proj", ps._gram)),
        "rank_k_lev_scores": (lambda d: op.rank_k_lev_scores(S(d), k, dtype=d), ("eig", "rowlev", same)),
        # sigma_p (I - T^T T) / lam, sigma_p = 1: back to the projector
        "precon_exact": (exact, ("wood", "proj", lambda P: np.eye(N, dtype=LD) - LD(lam) * P.astype(LD))),
        "spectrum": (lambda d: op.spectrum(S(d), lam, exact(d), dtype=d), ("spectrum", "spectrum_P", same)),
    }


def test_longdouble_type_and_agreement():
    """Every function at both dtypes on the RBF kernel at N = 65, k = 9: the long-double result
    is long double, has the float64 one's shape and carries bits below float64; and the float64
    result, turned into the basis-free quantity the sweep compares, agrees with the sweep's
    long-double reference to the band of that quantity (`held`, as the GPU is)."""
    p = ps.problem(("rbf", 65), 9)
    lam = LAMS[0]
    for name, (f, q) in _calls(p, lam).items():
        v64, vld = f(np.float64), f(LD)
        assert v64.dtype == np.float64, name
        assert vld.dtype == LD, name
        assert vld.shape == v64.shape, name
        # more than a cast of the float64 result: some entry carries bits below float64's
        assert np.any(vld != vld.astype(np.float64)), name
        if q is None:
            continue
        build, quantity, to = q
        ref = p.ref(build, lam)[quantity]
        cut = (lambda a: a[0]) if quantity == "z" else (lambda a: a)
        b = p.band(build, lam, quantity, part=cut)
        held(to(v64), cut(ref), b, f"{p.label} {name} float64")
        held(to(vld), cut(ref), b, f"{p.label} {name} long double")


def test_eigh_longdouble():
    """S = V diag(w) V^T and V^T V = I to the Jacobi's own stop, 2^-60 of the whole per entry
    (n entries to a sum); pairs by |eigenvalue|, as svd orders them, the float64 svd within the
    band of the eigen build's eigenvalues."""
    for inp in (("rbf", 65), ("indef", 129)):
        S = ps.problem(inp, 9).S_ld
        w, V = op.eigh_longdouble(S)
        n = S.shape[0]
        assert w.dtype == LD and V.dtype == LD and np.all(np.diff(w) >= 0)
        top = np.max(np.abs(w))
        assert np.max(np.abs((V * w) @ V.T - S)) <= n * 2.0 ** -60 * top
        assert np.max(np.abs(V.T @ V - np.eye(n, dtype=LD))) <= n * 2.0 ** -60
    p = ps.problem(("indef", 129), 40)
    U, s = op._svd_symmetric(p.S_ld, LD)
    assert np.all(np.diff(s) <= 0) and np.all(s >= 0)
    assert np.array_equal(s[:40], p.ref("eig", LAMS[0])["evals"])
    held(np.linalg.svd(p.S64)[1][:40], s[:40], p.band("eig", LAMS[0], "evals"), f"{p.label} svd float64")


def test_table_has_the_required_shapes():
    have = {(r[0], r[1]) for r in ps.TABLE}
    want = [(1, 1), (2, 2), (63, 7), (64, 8), (65, 9), (129, 63), (129, 64), (129, 65), (200, 127),
            (200, 128), (257, 130), (1025, 130), (512, 81), (513, 81), (600, 97), (129, 129)]
    for N, k in want:
        assert (("rbf", N), k) in have, (N, k)
    assert {(("spd", 64), 64), (("spd", 129), 129)} <= have
    assert any(r[0][0] == "sgdml" and {"matfree", "assembled"} <= set(r[3]) for r in ps.TABLE)
    assert {src for r in ps.TABLE for src in r[3]} == {"host", "points", "rows", "matfree", "assembled"}
    assert set(ps.PERSIST) == {(("rbf", 512), 81), (("rbf", 513), 81), (("rbf", 600), 97)}
    assert set(ps.INDEX_SETS) == {(("rbf", 129), 65), (("rbf", 513), 81)}
    assert all(set(v) == {"rand", "first", "ends"} for v in ps.INDEX_SETS.values())
    eig = {(r[0], r[1], r[3]) for r in ps.EIG_TABLE}
    assert {(("spd", 64), 64, 0), (("spd", 129), 129, 0), (("indef", 129), 40, 0),
            (("indef", 129), 49, 0), (("sgdml", 3, 20, "id"), 45, 0), (("sgdml", 3, 20, "id"), 45, 2)} <= eig
    sharded = {(i, k): w for i, k, w in ps.SHARDED}
    assert sharded[(("rbf", 65), 9)] == (2, 3, 5) and sharded[(("rbf", 2), 2)] == (5,)
    assert sharded[(("rbf", 513), 81)] == (3,)
    assert LAMS == (1e-4, 1e-10)
    for r in ps.TABLE:
        assert r[4], "every row says which branch it reaches"


@pytest.mark.parametrize("row", ps.TABLE, ids=TABLE_IDS)
def test_conditions_of_the_column_builds(row):
    inp, k, builds, _, _ = row
    p = ps.problem(inp, k)
    piv, gap, smallest = p.pivots
    floor = 1e3 * p.N * 2.0 ** -52
    print(f"{p.label}: smallest pivot gap {gap:.3e}, smallest pivot {smallest:.3e} of the largest "
          f"(floor {floor:.1e})")
    assert gap > ps.PIVOT_GAP
    assert smallest > floor
    if p.kind == "rbf":
        assert piv[0] == 0                     # the first maximum of an all-equal diagonal
    if k == p.N:                               # the factorisation reproduces S itself
        assert ps._rel(p.ref("pivL", LAMS[0])["LLt"], p.S_ld) <= p.N * 2.0 ** -60 / smallest
    if "nys0" in builds or "lev" in builds:
        for which in ps.INDEX_SETS.get((inp, k), ("rand",)):
            idx = p.idx(which)
            assert idx.shape == (k,) and np.all(np.diff(idx) > 0) and 0 <= idx[0] and idx[-1] < p.N
            if which == "ends":
                assert idx[0] == 0 and idx[-1] == p.N - 1
            lo = p.smm_min_eig(which)
            print(f"{p.label}: smallest eigenvalue of S_mm[{which}] {lo:.3e}")
            assert lo >= ps.MIN_SMM_EIG
    if p.N <= 257:                             # the larger rows print theirs in the GPU run
        for lam in LAMS:
            for b in builds:
                names = [n for n in p.ref(b, lam) if n != "T"]
                print(f"{p.label} {ps.lam_id(lam)} {b}: " +
                      " ".join(f"band[{n}]={p.band(b, lam, n):.2e}" for n in names))


@pytest.mark.parametrize("row", ps.EIG_TABLE, ids=[ps.label(r[0], r[1]) + f"-mask{r[3]}" for r in ps.EIG_TABLE])
def test_conditions_of_the_eigen_build(row):
    inp, k, _, mask, unique, _ = row
    p = ps.problem(inp, k, mask)
    s = p.spectrum_abs
    b = k + max(16, k // 2)
    full = 2 * b >= p.N
    gap = (s[k - 1] - s[k]) / s[0] if k < p.N else np.inf
    decay = s[b] / s[k - 1] if b < p.N else 0.0
    print(f"{p.label}: full={full} b={b} gap={gap:.3e} decay={decay:.3e} |l_1|={s[0]:.3e} |l_k|={s[k - 1]:.3e}")
    for lam in LAMS:
        print(f"{p.label} {ps.lam_id(lam)}: " + " ".join(
            f"band[{n}]={p.band('eig', lam, n):.2e}" for n in ("evals", "rowlev", "proj", "z")))
    if not full:
        assert decay <= ps.EIG_DECAY
    if unique:
        assert gap >= ps.EIG_GAP
    if inp == ("indef", 129):
        w = op.eigh_longdouble(p.S_ld)[0]
        top = w[np.argsort(-np.abs(w))[:k]]
        assert np.any(top < 0) and np.any(top > 0)
        assert np.min(np.diff(np.sort(np.abs(w)))) > 1e-6
    if inp[0] == "sgdml":
        assert b > p.mol.rank and not full
    if mask == 2:
        # the largest |K| lies inside a same-atom block, so the mask is no rounding matter
        K = np.abs(ps.problem(inp, k).S64)
        i, j = np.unravel_index(np.argmax(K), K.shape)
        assert (i % p.mol.n3) // 3 == (j % p.mol.n3) // 3
        assert np.count_nonzero(p.S64) < np.count_nonzero(K)


def _rejected(*args, **kw):
    with pytest.raises(AssertionError):
        held(*args, **kw)
    return True


@pytest.mark.parametrize("lam", LAMS, ids=[ps.lam_id(x) for x in LAMS])
@pytest.mark.parametrize("row", ps.TABLE, ids=TABLE_IDS)
def test_sensitivity(row, lam):
    """The float64 oracle stands in for the device, on every row of the table.  As it is, it
    passes; with one of four defects it must not:
    * the panel's last row zeroed;
    * one 512-column slab of the Gram matrix added twice (N > 512);
    * the step-0 tie of the RBF diagonal taken by the last maximum (k < N: at k = N, L L^T = S
      whatever the order, and the pivots themselves are compared);
    * z computed with lam (1 + 1e-9), on each r whose own bound 10 x band (the band `held`
      applies, nothing else) lies below the defect.  z = (r - T^T T r) / lam cannot be known
      better than the projector: where float64 leaves T^T T itself uncertain by 5e-10 (lam = 1e-10
      at the rows with pivots down to 1e-6: rbf-200, rbf-257, sgdml) no vector r resolves 1e-9 in z
      -- (I - T^T T) g was tried, its band there is 2e-10 to 1.4e-9 -- and at k = N, z is all
      residue.  Those (row, lam, r) are printed with their band, and every row is resolved at
      lam = 1e-4 for k < N (asserted)."""
    inp, k = row[0], row[1]
    p = ps.problem(inp, k)
    N = p.N
    S = p.S64
    L = p._factor(np.float64, False)
    T, sp = op.woodbury_panel(L, lam)
    ref = p.ref("wood", lam)
    bp, tag = p.band("wood", lam, "proj"), f"{p.label} {ps.lam_id(lam)}"
    held(ps._gram(T), ref["proj"], bp, f"{tag} unperturbed")
    ps.check_z(p.evals("wood", lam)[0]["z"], p, "wood", lam, "rand", f"{tag} unperturbed")

    T0 = T.copy()
    T0[-1] = 0.0
    assert _rejected(ps._gram(T0), ref["proj"], bp, f"{tag} last panel row zeroed")

    if N > 512:
        G = lam * np.eye(k) + L.T @ L + L[:512].T @ L[:512]
        T2 = np.linalg.solve(np.linalg.cholesky(G), L.T)
        assert _rejected(ps._gram(T2), ref["proj"], bp, f"{tag} Gram slab added twice")

    if p.kind == "rbf" and k < N:
        Sr = ps.flip(S)                         # the first maximum of the reversed matrix
        Lr, order = op.pivoted_cholesky(lambda i: Sr[:, i], np.diag(Sr).copy(), k)
        assert N - 1 - order[0] == N - 1
        Lr = Lr[::-1].astype(LD)
        assert _rejected(Lr @ Lr.T, p.ref("pivL", lam)["LLt"], p.band("pivL", lam, "LLt"),
                         f"{tag} step-0 tie to the last maximum")

    defect = 1e-9
    checked = 0
    for i, name in enumerate(ps.Z_NAMES):
        b = p.band("wood", lam, "z", part=lambda a, i=i: a[i])
        if 10 * b < defect:
            z = op.apply_panel(T, sp, lam * (1 + defect), p.vectors[i])
            assert _rejected(z, ref["z"][i], b, f"{tag} z/{name} with lam (1 + 1e-9)")
            checked += 1
        else:
            print(f"{tag} z/{name}: band {b:.2e}, 10 x band >= {defect:g}: the lam defect is below the bound")
    if k < N and lam == LAMS[0]:
        assert checked == len(ps.Z_NAMES), (tag, checked)
