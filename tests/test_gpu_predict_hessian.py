"""Analytic Hessians on the GPU (sgdml_amd.GDMLPredict.hessian -> mlff_predict_hessian,
csrc/kernels_predict_hess.hip) against the long-double oracle of tests/hessian_oracle.py (anchored
on the CPU in tests/test_hessian_oracle.py; the reference implementation has no Hessian).

Bound (the project's rule): max|H_gpu - H_ld| <= 10 band max|H_ld|, band = the float64 oracle's
deviation from the long-double one on the same float64 inputs, floored at 2^-52, evaluated at
run time.  Every test prints its figures before it asserts.

Shapes: the smallest that reach each branch of the kernels.  Models of sgdml_shapes.molecule /
perm_set with random alphas_F (hessian_oracle.random_model); five queries per case, training
geometries plus 0.05 N(0, 1), the first one training geometry 0 itself (diff = 0 exactly).
"""
import ctypes
from functools import lru_cache

import numpy as np
import pytest

from tests import hessian_oracle as ho
from tests.sgdml_shapes import FLOOR, LD, held

pytestmark = pytest.mark.gpu

CASES = [
    (2, 1, "id"),          # smallest legal size (D = 1)
    (3, 4, "nongroup"),    # permutations, a set that is not closed
    (4, 33, "swap"),       # MP = 66: two chunks of 33 rows, a 32-row step and a step of one row
    (9, 17, "c3"),         # ethanol's D = 36; staged form, 32 rows per step; 28 blocks in 9 row slots
    (12, 5, "c3"),         # first size of the staged form with 16 rows per step
    (17, 3, "swap"),       # first size of the staged form with 8 rows per step
    (24, 3, "swap"),       # D = 276, 3n = 72: 171 blocks, one row slot; last size of the staged form
    (25, 3, "id"),         # first size whose rows do not fit LDS: the unstaged pair stage, Fd fused
    (30, 2, "id"),         # 3n = 90 > 88: 276 blocks, the first size with a second tile of H
    (33, 2, "id"),         # D = 528 > 512: Fd from the prediction's pair stage, no longer fused
    (86, 2, "swap"),       # 3n = 258 > 256 threads; one row per step
]
ECSTR = [False, True]


def case_id(k):
    return f"n{k[0]}-M{k[1]}-{k[2]}"


@pytest.fixture(scope="module")
def sg():
    import sgdml_amd

    if sgdml_amd.device_count() < 1:
        pytest.fail("no GPU visible to libmlffpcg.so")
    return sgdml_amd


@lru_cache(maxsize=None)
def setup(key, ecstr):
    """(model, queries 5 x n x 3, H_ld, band) of a case; computed once, read-only."""
    from sgdml_amd.predict import load_model_arrays

    n, M, kind = key
    model, Rtr = ho.random_model(n, M, kind, 1000 * n + M, alphas_E=ecstr, std=1.75, c=-3.0)
    rng = np.random.default_rng(2000 * n + M)
    R = Rtr[np.arange(5) % M] + 0.05 * rng.standard_normal((5, n, 3))
    R[0] = Rtr[0]
    ma = load_model_arrays(model, energy_constraints=True)
    H_ld = ho.hessian(ma, R, LD)
    H64 = ho.hessian(ma, R, np.float64)
    assert np.all(np.isfinite(H64))
    band = max(FLOOR, float(np.max(np.abs(H64 - H_ld)) / np.max(np.abs(H_ld))))
    for a in (R, H_ld):
        a.setflags(write=False)
    return model, R, H_ld, band


# ---------------------------------------------------------------- 1. against the oracle
@pytest.mark.parametrize("ecstr", ECSTR, ids=["plain", "ecstr"])
@pytest.mark.parametrize("key", CASES, ids=case_id)
def test_matches_the_long_double_oracle(sg, key, ecstr, monkeypatch):
    monkeypatch.delenv("MLFF_PRED_SLAB", raising=False)
    model, R, H_ld, band = setup(key, ecstr)
    n3 = 3 * key[0]
    with sg.GDMLPredict(model, device=0) as gd:
        assert gd.use_E_cstr == ecstr
        H = gd.hessian(R)
        H1 = [gd.hessian(R[i]) for i in range(5)]
    assert H.shape == (5, n3, n3) and all(h.shape == (1, n3, n3) for h in H1)
    held(H, H_ld, band, f"{case_id(key)} hessian{' ecstr' if ecstr else ''} Q=5")
    held(H1[0], H_ld[:1], band, f"{case_id(key)} hessian{' ecstr' if ecstr else ''} Q=1 (training geometry 0)")
    for q in range(5):
        assert np.array_equal(H[q], H[q].T), (key, q)          # exact symmetry
        assert np.array_equal(H1[q][0], H[q]), (key, q)        # alone = in the batch


# ---------------------------------------------------------------- 2. zero coefficients
@pytest.mark.parametrize("key", CASES, ids=case_id)
def test_zero_coefficients_give_the_unconstrained_bits(sg, key):
    model, R, _, _ = setup(key, False)
    zero = dict(model, alphas_E=np.zeros(key[1]))
    with sg.GDMLPredict(model, device=0) as gd:
        assert not gd.use_E_cstr
        H0 = gd.hessian(R)
    with sg.GDMLPredict(zero, device=0) as gd:
        assert gd.use_E_cstr
        H = gd.hessian(R)
    assert np.array_equal(H, H0)


# ---------------------------------------------------------------- 3. bitwise batch invariance
@pytest.mark.parametrize("ecstr", ECSTR, ids=["plain", "ecstr"])
@pytest.mark.parametrize("key", CASES, ids=case_id)
def test_bits_do_not_depend_on_slab_or_device_split(sg, key, ecstr, monkeypatch):
    """MLFF_PRED_SLAB bounds the Hessian's slab too (it never exceeds the prediction's, whose
    buffers hold the queries' descriptors)."""
    model, R, _, _ = setup(key, ecstr)
    monkeypatch.delenv("MLFF_PRED_SLAB", raising=False)
    with sg.GDMLPredict(model, device=0) as gd:
        H = gd.hessian(R)
        Hr = gd.hessian(R[::-1])
    assert np.array_equal(Hr[::-1], H)
    for slab in ("1", "3"):
        monkeypatch.setenv("MLFF_PRED_SLAB", slab)
        with sg.GDMLPredict(model, device=0) as gd:
            assert gd.slab == int(slab)
            Hs = gd.hessian(R)
            assert np.array_equal(Hs, H), (key, slab)
            for i in (0, 4):
                assert np.array_equal(gd.hessian(R[i])[0], H[i]), (key, slab, i)
    monkeypatch.delenv("MLFF_PRED_SLAB", raising=False)
    with sg.GDMLPredict(model, devices=[0, 0]) as gd:
        H2 = gd.hessian(R)                 # 3 + 2 queries
        H1 = gd.hessian(R[:1])             # one empty block
    assert np.array_equal(H2, H) and np.array_equal(H1, H[:1])


# ---------------------------------------------------------------- 4. against the GPU's own forces
@pytest.mark.parametrize("ecstr", ECSTR, ids=["plain", "ecstr"])
def test_hessian_is_minus_the_derivative_of_the_predicted_forces(sg, ecstr, monkeypatch):
    """-(F(R + h e_i) - F(R - h e_i)) / 2h of GDMLPredict.predict at h = 1e-4 in float64, case
    n9-M17-c3, query 1: a consistency check between the two entry points, not the accuracy test
    (the difference quotient has h^2 truncation and 2^-53 / h rounding).  Measured on an MI355X,
    relative to max|H|: 8.106e-9 without and 1.291e-8 with alphas_E (FD_MEASURED, rounded up); the
    bound is 10 x that, and has to stay below 1e-5."""
    monkeypatch.delenv("MLFF_PRED_SLAB", raising=False)
    model, R, _, _ = setup((9, 17, "c3"), ecstr)
    r0 = R[1].ravel()
    h = 1e-4
    disp = np.repeat(r0[None, :], 54, axis=0)
    disp[np.arange(27), np.arange(27)] += h
    disp[27 + np.arange(27), np.arange(27)] -= h
    with sg.GDMLPredict(model, device=0) as gd:
        H = gd.hessian(r0)[0]
        _, F = gd.predict(disp)
    H_fd = -(F[:27] - F[27:]) / (2 * h)
    d = float(np.max(np.abs(H_fd - H)) / np.max(np.abs(H)))
    bound = 10 * FD_MEASURED[ecstr]
    print(f"n9-M17-c3 ecstr={ecstr}: max|H + dF/2h| / max|H| = {d:.3e} (bound {bound:.3e})")
    assert bound < 1e-5
    assert d <= bound


FD_MEASURED = {False: 8.11e-9, True: 1.29e-8}


# ---------------------------------------------------------------- 5. errors and state
def test_errors(sg):
    from sgdml_amd import _native as nat

    model, R, _, _ = setup((9, 17, "c3"), False)
    dp = ctypes.POINTER(ctypes.c_double)
    with sg.KernelSolver(3 * 9 * 17, device=0) as s:
        Rq = np.ascontiguousarray(R[:1])
        out = np.empty((1, 27, 27))
        rc = s._lib.mlff_predict_hessian(s._ctx, Rq.ctypes.data_as(dp), 1, out.ctypes.data_as(dp))
        assert rc == nat.MLFF_ERR_STATE
        with pytest.raises(RuntimeError):
            s.predict_hessian(Rq)
        with pytest.raises(RuntimeError):
            s.predict_hessian_info()
    with sg.GDMLPredict(model, device=0) as gd:
        H = gd.hessian(np.empty((0, 9, 3)))
        assert H.shape == (0, 27, 27) and H.dtype == np.float64
        for bad in (np.zeros(26), np.zeros((2, 8, 3)), np.zeros((9, 2)), np.zeros((2, 28))):
            with pytest.raises(ValueError):
                gd.hessian(bad)
        for ok in (R[2], R[2].ravel(), R[2:3].reshape(1, 27)):
            assert np.array_equal(gd.hessian(ok), gd.hessian(R[2:3]))
        fl, by = gd._engines[0].predict_hessian_info()
        assert fl > gd.flops_per_query and by == gd.bytes_per_query      # D = 36: one stream, Fd fused
    with pytest.raises(RuntimeError):
        gd.hessian(R)
