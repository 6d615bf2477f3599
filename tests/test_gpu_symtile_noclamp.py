"""The generating role's entry with and without the clamp of the squared distance
(SymGen::noclamp).

An operator whose scaled points lie in a box of squared diagonal at most 2048 evaluates the
entries of its plain tiles (off the diagonal, no padding) without min(s, 2150); every other
operator, every padded or diagonal tile, and every operator built under MLFF_SYM_GEN_CLAMP=1
keeps it.  Either way a generated entry is the stored bit pattern, so a mat-vec with every
workgroup generating (MLFF_SYM_ROLES=gen) must equal the one with every workgroup streaming
(stream) bit for bit: comparisons are np.array_equal, never a tolerance.  Which form ran is part
of each case (mlff_sym_gen_info): a comparison that cannot tell proves nothing.
"""
import numpy as np
import pytest

from tests.test_gpu_symtile_generate import LAM, N_MID, assert_same

pytestmark = pytest.mark.gpu

ENV = ("MLFF_SYM_GEN", "MLFF_SYM_GEN_TILES", "MLFF_SYM_GEN_QUARTERS", "MLFF_SYM_ROLES",
       "MLFF_SYM_STEAL", "MLFF_SYM_WGS", "MLFF_SYM_GEN_CLAMP")
# 15 tiles, all quarter units: plain, padded and diagonal ones; 512 whole tiles + 83 split
SIZES = (2100, N_MID)
FORMS = ("2", "3")
LS = 0.3     # length scale
SIDE = 5.0   # of a cube of points, in length scales
GAP = 60.0   # between the two clusters, in length scales


def set_env(mp, env):
    for k in ENV:
        mp.delenv(k, raising=False)
    for k, v in env.items():
        mp.setenv(k, v)


def cube(n):
    """(a): uniform in a cube of side 5 length scales; squared distances up to 75."""
    return LS * SIDE * np.random.default_rng(31).random((n, 3))


def clusters(n):
    """(b): the first half of (a) as it is, the second half 60 length scales further along the
    first axis: squared distances of about 3600 across, far past the clamp at 2150."""
    X = cube(n)
    X[n // 2:, 0] += LS * GAP
    return X


def operands(n):
    """A random vector, a unit vector (entry bits, not only sums) and a vector with denormal and
    huge entries (no sum overflows: n * 1e150)."""
    rng = np.random.default_rng(32)
    v = rng.standard_normal(n)
    e = np.zeros(n)
    e[n // 3] = 1.0
    w = rng.standard_normal(n)
    w[::7] = 5e-324
    w[1::7] = 1e-310 * rng.standard_normal(w[1::7].size)
    w[2::7] = 1e150 * rng.standard_normal(w[2::7].size)
    return [v, e, w]


def run(mp, env, X, vecs, rows=None):
    """Each vector applied twice (the second on the counters the first one left), what the
    operator says about its generating role, and on request some stored rows of K."""
    import sgdml_amd

    set_env(mp, env)
    n = X.shape[0]
    s = sgdml_amd.KernelSolver(n, device=0)
    try:
        s.gen_rbf(X, length_scale=LS, jitter=1e-9)
        s.set_operator(1.0, LAM)
        assert s.storage_info()[0] == "sym"
        info = s.sym_gen_info()
        ys = [s.matvec(v) for v in vecs for _ in range(2)]
        K = s.get_matrix_rows(*rows) if rows is not None else None
    finally:
        s.close()
    return ys, info, K


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", SIZES)
def test_small_extent_runs_without_the_clamp(n, form, monkeypatch):
    """(a) and (c): no clamp in the plain tiles of (a), the clamp everywhere under
    MLFF_SYM_GEN_CLAMP=1, the streamed bits both times."""
    X, vecs = cube(n), operands(n)
    ref, info_s, _ = run(monkeypatch, {"MLFF_SYM_WGS": form, "MLFF_SYM_ROLES": "stream"}, X, vecs)
    got, info_g, _ = run(monkeypatch, {"MLFF_SYM_WGS": form, "MLFF_SYM_ROLES": "gen"}, X, vecs)
    forced, info_c, _ = run(monkeypatch, {"MLFF_SYM_WGS": form, "MLFF_SYM_ROLES": "gen",
                                          "MLFF_SYM_GEN_CLAMP": "1"}, X, vecs)
    assert info_s[0] is True and info_g[0] is True and info_c[0] is False
    assert info_s[1] == info_g[1] == info_c[1] and 0.0 < info_g[1] <= 3.0 * SIDE ** 2 * (1 + 1e-12)
    assert all(np.all(np.isfinite(y)) for y in ref)
    assert_same(got, ref)
    assert_same(forced, got)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", SIZES)
def test_large_extent_keeps_the_clamp(n, form, monkeypatch):
    """(b): squared distances past 2150 between the clusters; the clamp stays, the entries
    across are +0 as they are stored, and the bits are the streamed ones."""
    X, vecs = clusters(n), operands(n)
    nr = 64
    ref, info_s, K = run(monkeypatch, {"MLFF_SYM_WGS": form, "MLFF_SYM_ROLES": "stream"}, X, vecs,
                         rows=(0, nr))
    got, info_g, _ = run(monkeypatch, {"MLFF_SYM_WGS": form, "MLFF_SYM_ROLES": "gen"}, X, vecs)
    assert info_s[0] is False and info_g[0] is False
    assert info_g[1] > (GAP - SIDE) ** 2 > 2150.0
    cross = K[:, n // 2:]  # rows of the first cluster, columns of the second
    assert cross.shape == (nr, n - n // 2)
    assert np.all(cross == 0.0) and not np.any(np.signbit(cross))
    assert np.all(K[:, :n // 2] > 0.0)
    assert_same(got, ref)


def two_point_extent(extent_points):
    """64 points in d = 3: two given corner points and 62 on the segment between them."""
    lo, hi = (np.asarray(p, dtype=np.float64) for p in extent_points)
    t = np.random.default_rng(33).random((62, 1))
    return np.ascontiguousarray(np.vstack([lo, hi, lo + t * (hi - lo)]))


@pytest.mark.parametrize("hi,noclamp", [
    ((45.25, 0.0, 0.0), True),                          # 2047.5625
    ((45.26, 0.0, 0.0), False),                         # 2048.4676
    ((32.0, 32.0, 0.0), True),                          # 2048 exactly: the threshold is inside
    ((32.0, float(np.nextafter(32.0, 64.0)), 0.0), False),  # one ulp of 2048 above it
])
def test_threshold_of_the_extent(hi, noclamp, monkeypatch):
    """extent2 just below, at and just above 2048 (length scale 1, so the points are the scaled
    points): the flag follows it, and MLFF_SYM_GEN_CLAMP=1 overrides it."""
    import sgdml_amd

    X = two_point_extent(((0.0, 0.0, 0.0), hi))
    assert np.all(X.min(axis=0) == 0.0) and np.all(X.max(axis=0) == np.asarray(hi))
    want = float(sum(h * h for h in hi))
    assert (want <= 2048.0) == noclamp
    for env, flag in (({}, noclamp), ({"MLFF_SYM_GEN_CLAMP": "1"}, False)):
        set_env(monkeypatch, env)
        s = sgdml_amd.KernelSolver(64, device=0)
        try:
            s.gen_rbf(X, length_scale=1.0, jitter=1e-9)
            s.set_operator(1.0, LAM)
            assert s.storage_info()[0] == "sym"
            got = s.sym_gen_info()
        finally:
            s.close()
        assert got == (flag, want), (env, got)
