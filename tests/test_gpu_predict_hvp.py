"""Hessian-vector products on the GPU (sgdml_amd.GDMLPredict.hessian_vector -> mlff_predict_hvp,
csrc/kernels_predict_hvp.hip) against the long-double oracle of tests/hvp_oracle.py (anchored on
the CPU in tests/test_hvp_oracle.py; the reference implementation has no such product).

Bound (the project's rule): max|HV_gpu - HV_ld| <= 10 band max|HV_ld|, band = the float64 oracle's
deviation from the long-double one on the same float64 inputs, floored at 2^-52, evaluated at
run time.  Every test prints its figures before it asserts.

Shapes: the smallest that reach each branch of the kernels.  Models of sgdml_shapes.molecule /
perm_set with random alphas_F (hessian_oracle.random_model, std 1.75, c -3); five queries per
case, training geometries plus 0.05 N(0, 1), the first one training geometry 0 itself (diff = 0
exactly); N(0, 1) vectors.  K = 1 runs the pair stage's one-vector instantiation, K = KB + 1 = 5 a
full block and a block with three empty slots, K = PASS + 1 = 9 a second pass over the vectors.
"""
import ctypes
from functools import lru_cache

import numpy as np
import pytest

from tests import hessian_oracle as ho
from tests import hvp_oracle as vo
from tests.sgdml_shapes import FLOOR, LD, held

pytestmark = pytest.mark.gpu

KB = 4        # kHvKB: vectors per block of the pair stage
PASS = 8      # kHvPass: vectors of a query per pass
KMAX = PASS + 1

CASES = [
    (2, 1, "id"),          # D = 1
    (3, 4, "nongroup"),    # smallest case with non-trivial permutations
    (4, 33, "swap"),       # MP = 66: two chunks of 33 rows, four rows in flight: a ragged last step
    (9, 17, "c3"),         # ethanol's D = 36
    (10, 3, "swap"),       # D = 45: last D of the register variant <16, 3>
    (11, 3, "id"),         # D = 55: first D of <64, 2>
    (16, 3, "id"),         # D = 120: last D of <64, 2>
    (17, 3, "swap"),       # D = 136: first D of <64, 3>
    (20, 3, "id"),         # D = 190: last D of <64, 3>
    (21, 3, "id"),         # D = 210: first D of <64, 5>
    (24, 3, "swap"),       # D = 276, last D of the register form
    (25, 3, "id"),         # D = 300, first D past the register form: the stream form
    (33, 2, "id"),         # D = 528, more than two entries per lane of 256
    (86, 2, "swap"),       # 3n = 258 > 256
]
TWO_FORMS = [k for k in CASES if k[0] * (k[0] - 1) // 2 <= 288]
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
def setup(key, ecstr, Q=5, K=KMAX, coincide=True):
    """(model, model arrays, queries Q x n x 3, vectors Q x K x 3n, HV_ld, HV_64) of a case;
    computed once, read-only.  coincide: the first query is training geometry 0 itself."""
    from sgdml_amd.predict import load_model_arrays

    n, M, kind = key
    model, Rtr = ho.random_model(n, M, kind, 1000 * n + M, alphas_E=ecstr, std=1.75, c=-3.0)
    rng = np.random.default_rng(2000 * n + M)
    R = Rtr[np.arange(Q) % M] + 0.05 * rng.standard_normal((Q, n, 3))
    if coincide:
        R[0] = Rtr[0]
    V = rng.standard_normal((Q, K, 3 * n))
    ma = load_model_arrays(model, energy_constraints=True)
    HV_ld = vo.hvp(ma, R, V, LD)
    HV_64 = vo.hvp(ma, R, V, np.float64)
    assert np.all(np.isfinite(HV_64))
    for a in (R, V, HV_ld, HV_64):
        a.setflags(write=False)
    return model, ma, R, V, HV_ld, HV_64


def band_of(HV_64, HV_ld):
    return max(FLOOR, float(np.max(np.abs(HV_64 - HV_ld)) / np.max(np.abs(HV_ld))))


def check_case(gd, key, ecstr, label):
    _, _, R, V, HV_ld, HV_64 = setup(key, ecstr)
    n3 = 3 * key[0]
    for K in (1, KB + 1):
        HV = gd.hessian_vector(R, V[:, :K])
        assert HV.shape == (5, K, n3) and HV.dtype == np.float64
        held(HV, HV_ld[:, :K], band_of(HV_64[:, :K], HV_ld[:, :K]),
             f"{case_id(key)} hvp{' ecstr' if ecstr else ''} {label} K={K}")


# ---------------------------------------------------------------- 1. against the oracle
@pytest.mark.parametrize("ecstr", ECSTR, ids=["plain", "ecstr"])
@pytest.mark.parametrize("key", CASES, ids=case_id)
def test_matches_the_long_double_oracle(sg, key, ecstr, monkeypatch):
    monkeypatch.delenv("MLFF_PRED_SLAB", raising=False)
    monkeypatch.delenv("MLFF_PRED_FORM", raising=False)
    model = setup(key, ecstr)[0]
    with sg.GDMLPredict(model, device=0) as gd:
        assert gd.use_E_cstr == ecstr
        assert gd.form == ("tile" if key in TWO_FORMS else "stream")
        check_case(gd, key, ecstr, gd.form)


@pytest.mark.parametrize("form", ["tile", "stream"])
@pytest.mark.parametrize("ecstr", ECSTR, ids=["plain", "ecstr"])
@pytest.mark.parametrize("key", TWO_FORMS, ids=case_id)
def test_both_forms_meet_the_bound(sg, key, ecstr, form, monkeypatch):
    """MLFF_PRED_FORM chooses the pair stage here as it does for the prediction (D <= 288)."""
    monkeypatch.delenv("MLFF_PRED_SLAB", raising=False)
    monkeypatch.setenv("MLFF_PRED_FORM", form)
    model = setup(key, ecstr)[0]
    with sg.GDMLPredict(model, device=0) as gd:
        assert gd.form == form
        check_case(gd, key, ecstr, form)


# ---------------------------------------------------------------- 2. against the GPU's Hessian
@pytest.mark.parametrize("ecstr", ECSTR, ids=["plain", "ecstr"])
@pytest.mark.parametrize("key", [(9, 17, "c3"), (30, 2, "id")], ids=case_id)
def test_matches_the_gpu_hessian_times_the_vector(sg, key, ecstr, monkeypatch):
    """gd.hessian(R) @ V, the product formed in long double on the host, to the bound of test 1."""
    monkeypatch.delenv("MLFF_PRED_SLAB", raising=False)
    monkeypatch.delenv("MLFF_PRED_FORM", raising=False)
    model, _, R, V, HV_ld, HV_64 = setup(key, ecstr)
    K = KB + 1
    with sg.GDMLPredict(model, device=0) as gd:
        H = gd.hessian(R)
        HV = gd.hessian_vector(R, V[:, :K])
    ref = np.einsum("qij,qkj->qki", H.astype(LD), V[:, :K].astype(LD))
    held(HV, ref, band_of(HV_64[:, :K], HV_ld[:, :K]), f"{case_id(key)} hvp{' ecstr' if ecstr else ''} vs hessian @ V")


# ---------------------------------------------------------------- 3. past the Hessian's limit
def test_more_atoms_than_the_hessian_accepts(sg, monkeypatch):
    """683 atoms (D = 232 903): `hessian` refuses, `hessian_vector` has no limit.  One query per
    pass keeps the prediction's slab buffers of this descriptor length small."""
    monkeypatch.setenv("MLFF_PRED_SLAB", "1")
    monkeypatch.delenv("MLFF_PRED_FORM", raising=False)
    key = (683, 1, "id")
    model, _, R, V, HV_ld, HV_64 = setup(key, False, 1, 2, False)
    with sg.GDMLPredict(model, device=0) as gd:
        assert gd.form == "stream"
        HV = gd.hessian_vector(R, V)
        with pytest.raises((ValueError, RuntimeError), match="682 atoms"):
            gd.hessian(R)
    assert HV.shape == (1, 2, 3 * 683)
    held(HV, HV_ld, band_of(HV_64, HV_ld), "n683-M1-id hvp Q=1 K=2")


# ---------------------------------------------------------------- 4. zero coefficients
@pytest.mark.parametrize("key", CASES, ids=case_id)
def test_zero_coefficients_give_the_unconstrained_bits(sg, key, monkeypatch):
    monkeypatch.delenv("MLFF_PRED_SLAB", raising=False)
    monkeypatch.delenv("MLFF_PRED_FORM", raising=False)
    model, _, R, V, _, _ = setup(key, False)
    zero = dict(model, alphas_E=np.zeros(key[1]))
    with sg.GDMLPredict(model, device=0) as gd:
        assert not gd.use_E_cstr
        HV0, HV0_1 = gd.hessian_vector(R, V[:, :KB + 1]), gd.hessian_vector(R, V[:, 0])
    with sg.GDMLPredict(zero, device=0) as gd:
        assert gd.use_E_cstr
        HV, HV_1 = gd.hessian_vector(R, V[:, :KB + 1]), gd.hessian_vector(R, V[:, 0])
    assert np.array_equal(HV, HV0) and np.array_equal(HV_1, HV0_1)


# ---------------------------------------------------------------- 5. bitwise invariance
@pytest.mark.parametrize("ecstr", ECSTR, ids=["plain", "ecstr"])
@pytest.mark.parametrize("key", CASES, ids=case_id)
def test_bits_do_not_depend_on_k_batch_slab_or_device_split(sg, key, ecstr, monkeypatch):
    model, _, R, V, _, _ = setup(key, ecstr)
    K = KB + 1
    monkeypatch.delenv("MLFF_PRED_SLAB", raising=False)
    monkeypatch.delenv("MLFF_PRED_FORM", raising=False)
    with sg.GDMLPredict(model, device=0) as gd:
        HV = gd.hessian_vector(R, V[:, :K])
        # alone (the one-vector instantiation): every position of the block of query 1, and the
        # lone vector of the second block of the first and the last query
        for q, k in [(1, k) for k in range(K)] + [(0, KB), (4, KB)]:
            one = gd.hessian_vector(R[q], V[q:q + 1, k])
            assert one.shape == (1, R.shape[1] * 3)
            assert np.array_equal(one[0], HV[q, k]), (key, q, k)
        # another batch order and other positions in the block
        Hr = gd.hessian_vector(R[::-1], V[::-1, K - 1::-1])
        assert np.array_equal(Hr[::-1, ::-1], HV)
        # a second pass over the vectors (K = 9: eight, then one)
        H9 = gd.hessian_vector(R, V)
        assert np.array_equal(H9[:, :K], HV)
        assert np.array_equal(H9[3, PASS], gd.hessian_vector(R[3], V[3:4, PASS])[0])
    for slab in ("1", "3"):
        monkeypatch.setenv("MLFF_PRED_SLAB", slab)
        with sg.GDMLPredict(model, device=0) as gd:
            assert gd.slab == int(slab)
            assert np.array_equal(gd.hessian_vector(R, V[:, :K]), HV), (key, slab)
            for i in (0, 4):
                assert np.array_equal(gd.hessian_vector(R[i], V[i:i + 1, :K])[0], HV[i]), (key, slab, i)
    monkeypatch.delenv("MLFF_PRED_SLAB", raising=False)
    with sg.GDMLPredict(model, devices=[0, 0]) as gd:
        H2 = gd.hessian_vector(R, V[:, :K])              # 3 + 2 queries
        H1 = gd.hessian_vector(R[:1], V[:1, :K])         # one empty block
    assert np.array_equal(H2, HV) and np.array_equal(H1, HV[:1])


# ---------------------------------------------------------------- 6. structure
@pytest.mark.parametrize("ecstr", ECSTR, ids=["plain", "ecstr"])
@pytest.mark.parametrize("key", CASES, ids=case_id)
def test_translations_vanish_and_scaling_is_exact(sg, key, ecstr, monkeypatch):
    """A rigid translation has y = 0 and every v_a - v_b = 0 exactly: every entry of the result
    is exactly zero (no term is added that does not vanish with them).  Doubling v doubles every
    intermediate exactly."""
    monkeypatch.delenv("MLFF_PRED_SLAB", raising=False)
    monkeypatch.delenv("MLFF_PRED_FORM", raising=False)
    model, _, R, V, _, _ = setup(key, ecstr)
    n = key[0]
    t = np.random.default_rng(7).standard_normal((5, 2, 1, 3))
    T = np.broadcast_to(t, (5, 2, n, 3)).copy()
    with sg.GDMLPredict(model, device=0) as gd:
        Z = gd.hessian_vector(R, T)
        HV = gd.hessian_vector(R, V[:, :KB + 1])
        HV2 = gd.hessian_vector(R, 2.0 * V[:, :KB + 1])
    print(f"{case_id(key)} ecstr={ecstr}: max|H t| = {np.max(np.abs(Z)):.3e} for rigid translations t")
    assert Z.shape == (5, 2, 3 * n) and np.all(Z == 0.0)
    assert np.array_equal(HV2, 2.0 * HV)


@pytest.mark.parametrize("ecstr", ECSTR, ids=["plain", "ecstr"])
@pytest.mark.parametrize("key", [(3, 4, "nongroup"), (9, 17, "c3"), (25, 3, "id")], ids=case_id)
def test_the_operator_is_symmetric(sg, key, ecstr, monkeypatch):
    """u . (H v) against v . (H u): each product is within 10 band max|HV| of the exact one, the
    two dots therefore within 2 x 10 band |u| |v| max|H| (the scale from the Hessian oracle)."""
    monkeypatch.delenv("MLFF_PRED_SLAB", raising=False)
    monkeypatch.delenv("MLFF_PRED_FORM", raising=False)
    model, ma, R, V, HV_ld, HV_64 = setup(key, ecstr)
    band = band_of(HV_64[:, :2], HV_ld[:, :2])
    scale = np.max(np.abs(ho.hessian(ma, R, LD)), axis=(1, 2))
    with sg.GDMLPredict(model, device=0) as gd:
        HV = gd.hessian_vector(R, V[:, :2]).astype(LD)
    u, v = V[:, 0].astype(LD), V[:, 1].astype(LD)
    d = np.abs(np.sum(u * HV[:, 1], axis=1) - np.sum(v * HV[:, 0], axis=1))
    tol = 2 * 10 * LD(band) * np.sqrt(np.sum(u * u, axis=1) * np.sum(v * v, axis=1)) * scale
    print(f"{case_id(key)} ecstr={ecstr}: |u.Hv - v.Hu| = {[f'{float(x):.3e}' for x in d]}, "
          f"tolerance {[f'{float(x):.3e}' for x in tol]} (band {band:.3e})")
    assert np.all(d <= tol)


# ---------------------------------------------------------------- 7. against the GPU's own forces
@pytest.mark.parametrize("ecstr", ECSTR, ids=["plain", "ecstr"])
def test_is_minus_the_directional_derivative_of_the_predicted_forces(sg, ecstr, monkeypatch):
    """(F(R - h v) - F(R + h v)) / 2h of GDMLPredict.predict at h = 1e-4 in float64, case
    n9-M17-c3, query 1: a consistency check between the two entry points, not the accuracy test.
    The bound is 10 x the same difference of the float64 oracles on the CPU (the difference
    quotient's own h^2 truncation and 2^-53 / h rounding), and has to stay below 1e-5."""
    monkeypatch.delenv("MLFF_PRED_SLAB", raising=False)
    monkeypatch.delenv("MLFF_PRED_FORM", raising=False)
    model, ma, R, V, _, HV_64 = setup((9, 17, "c3"), ecstr)
    h = 1e-4
    r0, v = R[1].ravel(), V[1, 0]
    disp = np.stack([r0 - h * v, r0 + h * v])
    _, Fo = ho.energy_forces(ma, disp, np.float64)
    top = np.max(np.abs(HV_64[1, 0]))
    bound = 10 * float(np.max(np.abs((Fo[0] - Fo[1]) / (2 * h) - HV_64[1, 0])) / top)
    with sg.GDMLPredict(model, device=0) as gd:
        HV = gd.hessian_vector(r0, v[None])[0]
        _, F = gd.predict(disp)
    d = float(np.max(np.abs((F[0] - F[1]) / (2 * h) - HV)) / top)
    print(f"n9-M17-c3 ecstr={ecstr}: max|Hv + dF/2h| / max|Hv| = {d:.3e} (bound {bound:.3e})")
    assert bound < 1e-5
    assert d <= bound


# ---------------------------------------------------------------- 8. errors and state
def test_errors(sg, monkeypatch):
    from sgdml_amd import _native as nat

    monkeypatch.delenv("MLFF_PRED_SLAB", raising=False)
    monkeypatch.delenv("MLFF_PRED_FORM", raising=False)
    model, _, R, V, _, _ = setup((9, 17, "c3"), False)
    dp = ctypes.POINTER(ctypes.c_double)
    live0 = nat.live_bytes()
    with sg.KernelSolver(3 * 9 * 17, device=0) as s:
        Rq, Vq = np.ascontiguousarray(R[:1]), np.ascontiguousarray(V[:1, :1])
        out = np.empty((1, 1, 27))
        rc = s._lib.mlff_predict_hvp(s._ctx, Rq.ctypes.data_as(dp), Vq.ctypes.data_as(dp), 1, 1,
                                     out.ctypes.data_as(dp))
        assert rc == nat.MLFF_ERR_ARG
        with pytest.raises((ValueError, RuntimeError), match="no model set"):
            s.predict_hvp(Rq, Vq)
        with pytest.raises((ValueError, RuntimeError), match="no model set"):
            s.predict_hvp_info()
    with sg.GDMLPredict(model, device=0) as gd:
        eng = gd._engines[0]
        for Q, K in ((1, -1), (-1, 1)):
            rc = eng._lib.mlff_predict_hvp(eng._ctx, Rq.ctypes.data_as(dp), Vq.ctypes.data_as(dp), Q, K,
                                           out.ctypes.data_as(dp))
            assert rc == nat.MLFF_ERR_ARG
        e = gd.hessian_vector(np.empty((0, 9, 3)), np.empty((0, 3, 27)))
        assert e.shape == (0, 3, 27) and e.dtype == np.float64
        e = gd.hessian_vector(np.empty((0, 9, 3)), np.empty((0, 27)))
        assert e.shape == (0, 27)
        e = gd.hessian_vector(R, np.empty((5, 0, 27)))
        assert e.shape == (5, 0, 27) and e.dtype == np.float64
        for bad in (np.zeros(27), np.zeros((4, 27)), np.zeros((5, 26)), np.zeros((5, 2, 26)),
                    np.zeros((5, 8, 3)), np.zeros((5, 2, 9, 2)), np.zeros((5, 2, 3, 9, 3))):
            with pytest.raises(ValueError, match="V must be"):
                gd.hessian_vector(R, bad)
        with pytest.raises(ValueError):
            gd.hessian_vector(np.zeros((2, 8, 3)), np.zeros((2, 24)))
        # the four accepted layouts of V
        HV = gd.hessian_vector(R, V[:, :2])
        assert np.array_equal(gd.hessian_vector(R, V[:, :2].reshape(5, 2, 9, 3)), HV)
        assert np.array_equal(gd.hessian_vector(R.reshape(5, 27), V[:, 0]), HV[:, 0])
        assert np.array_equal(gd.hessian_vector(R, V[:, 1].reshape(5, 9, 3)), HV[:, 1])
        assert np.array_equal(gd.hessian_vector(R[2], V[2:3, :2]), HV[2:3])
        fl, by = eng.predict_hvp_info()
        hfl, _ = eng.predict_hessian_info()
        assert gd.flops_per_query < fl < hfl and by == gd.bytes_per_query   # D = 36: one stream of the rows
        assert nat.live_bytes() > live0
    with pytest.raises(RuntimeError):
        gd.hessian_vector(R, V[:, :2])
    assert nat.live_bytes() == live0
