"""The Hessian-vector oracle (tests/hvp_oracle.py) on the CPU.  The GPU tests hold
`GDMLPredict.hessian_vector` against it; here it is anchored on the Hessian oracle
(tests/hessian_oracle.py, itself anchored in tests/test_hessian_oracle.py): its long-double
products equal that oracle's long-double matrix times the vector, and minus the long-double
Richardson central difference of that oracle's forces along the vector.  Every test prints its
figures before it asserts.
"""
import numpy as np
import pytest

from tests import hessian_oracle as ho
from tests import hvp_oracle as vo
from tests.sgdml_shapes import FLOOR, LD

ANCHOR_CASES = [(2, 1, "id"), (3, 4, "nongroup"), (9, 17, "c3"), (25, 3, "id")]
FD_CASES = [(3, 4, "s3"), (4, 33, "swap"), (9, 17, "c3")]
FD_STEPS = (1e-3, 3e-4, 1e-4)
# The bound of tests/test_hessian_oracle.py for the same difference quotient along a coordinate
# axis, 10 x 2.52e-15 of max|H|.  Here the direction is a unit vector, so the step has the same
# length and the truncation (h^4) and rounding (2^-64 / h) terms the same size, relative to max|H|.
FD_BOUND = 10 * 2.52e-15


def arrays(model):
    from sgdml_amd.predict import load_model_arrays

    return load_model_arrays(model, energy_constraints=True)


def case_id(k):
    return f"n{k[0]}-M{k[1]}-{k[2]}"


def case(n, M, kind, ecstr, K=3):
    """(model arrays, five queries: training geometries + 0.05 N(0, 1), the first training geometry
    0 itself; K N(0, 1) vectors per query)."""
    model, Rtr = ho.random_model(n, M, kind, 1000 * n + M, alphas_E=ecstr, std=1.75, c=-3.0)
    rng = np.random.default_rng(3000 * n + M)
    R = Rtr[np.arange(5) % M] + 0.05 * rng.standard_normal((5, n, 3))
    R[0] = Rtr[0]
    return arrays(model), R, rng.standard_normal((5, K, 3 * n))


# ---------------------------------------------------------------- 1. the Hessian oracle's matrix
@pytest.mark.parametrize("ecstr", [False, True], ids=["plain", "ecstr"])
@pytest.mark.parametrize("key", ANCHOR_CASES, ids=case_id)
def test_equals_the_hessian_oracle_times_the_vector(key, ecstr):
    """Long-double hvp against hessian(ma, R, LD) @ v, relative to max|H v|, within 10 x the band
    of that product: the float64 Hessian oracle times v against the long-double one, floored at
    2^-52."""
    ma, R, V = case(*key, ecstr)
    ref = np.einsum("qij,qkj->qki", ho.hessian(ma, R, LD), V.astype(LD))
    p64 = np.einsum("qij,qkj->qki", ho.hessian(ma, R, np.float64).astype(LD), V.astype(LD))
    top = float(np.max(np.abs(ref)))
    band = max(FLOOR, float(np.max(np.abs(p64 - ref))) / top)
    got = vo.hvp(ma, R, V, LD)
    assert got.dtype == LD and got.shape == ref.shape
    dev = float(np.max(np.abs(got - ref))) / top
    dev64 = float(np.max(np.abs(vo.hvp(ma, R, V, np.float64) - ref))) / top
    print(f"{case_id(key)} ecstr={ecstr}: |hvp_ld - H_ld v| / max|H v| = {dev:.3e} (float64 hvp {dev64:.3e}), "
          f"band {band:.3e}, bound {10 * band:.3e}")
    assert dev <= 10 * band


# ---------------------------------------------------------------- 2. differences of the forces
@pytest.mark.parametrize("ecstr", [False, True], ids=["plain", "ecstr"])
@pytest.mark.parametrize("key", FD_CASES, ids=case_id)
def test_is_minus_the_directional_derivative_of_the_forces(key, ecstr):
    """Long-double hvp against -(4 D_h - D_2h) / 3, D_h = (F(r + h v) - F(r - h v)) / 2h with the
    long-double forces of the Hessian oracle and |v| = 1, relative to max|H|."""
    assert FD_BOUND < 1e-10
    ma, R, V = case(*key, ecstr, K=1)
    r = R[1].reshape(-1).astype(LD)
    v = V[1, 0].astype(LD)
    v /= np.sqrt(np.sum(v * v))
    top = float(np.max(np.abs(ho.hessian(ma, r[None], LD))))
    got = vo.hvp(ma, r[None], v[None], LD)[0, 0]

    def central(step):
        _, F = ho.energy_forces(ma, np.stack([r + step * v, r - step * v]), LD)
        return (F[0] - F[1]) / (2 * step)

    devs = []
    for h in FD_STEPS:
        h = LD(h)
        devs.append(float(np.max(np.abs(got + (4 * central(h) - central(2 * h)) / 3))) / top)
    print(f"{case_id(key)} ecstr={ecstr}: |hvp + dF/dv| / max|H| at h = {FD_STEPS}: "
          + " / ".join(f"{d:.3e}" for d in devs) + f"   bound {FD_BOUND:.3e}")
    assert devs[-1] <= FD_BOUND


# ---------------------------------------------------------------- 3. the C entry point
def test_abi_rejects_a_null_context():
    from sgdml_amd import _native

    lib = _native.load_library()
    assert lib.mlff_predict_hvp(None, None, None, 1, 1, None) == _native.MLFF_ERR_ARG
    assert lib.mlff_predict_hvp_info(None, None, None) == _native.MLFF_ERR_ARG
