"""The Hessian oracle (tests/hessian_oracle.py) on the CPU.  The reference implementation has no
Hessian, so the oracle that the GPU tests hold `GDMLPredict.hessian` against is anchored here:
its forces reproduce the reference's golden predictions, and its long-double Hessian is minus the
long-double Richardson central difference of those forces.  Every test prints its figures before
it asserts.
"""
import numpy as np
import pytest

from tests import hessian_oracle as ho
from tests.sgdml_shapes import FLOOR, LD

FD_CASES = [(3, 4, "s3"), (4, 33, "swap"), (9, 17, "c3")]
FD_STEPS = (1e-3, 3e-4, 1e-4)
# 10 x the largest discrepancy measured at the best step (h = 1e-4, see the docstring below)
FD_BOUND = 10 * 2.52e-15


def arrays(model):
    from sgdml_amd.predict import load_model_arrays

    return load_model_arrays(model, energy_constraints=True)


def fd_case(n, M, kind, ecstr):
    model, Rtr = ho.random_model(n, M, kind, 1000 * n + M, alphas_E=ecstr)
    r = Rtr[0] + 0.05 * np.random.default_rng(5).standard_normal((n, 3))
    return arrays(model), Rtr, r


# ---------------------------------------------------------------- 1. forces against the reference
@pytest.mark.parametrize("name", ["d3", "eth"])
def test_forces_match_the_reference(golden_dir, name):
    """float64 energy_forces against the reference's GDMLPredict.predict on the golden cases, under
    the bound of tests/test_gpu_predict.py::check (10 x the reference's own band)."""
    from sgdml_amd.model import r_d_desc_alpha
    from sgdml_amd.solver import host_descriptors

    f = np.load(golden_dir / "sgdml_predict_cases.npz", allow_pickle=False)
    c = {k[len(name) + 2:]: f[k] for k in f.files if k.startswith(name + "__")}
    Rd, Rdd = host_descriptors(c["R_train"])
    model = {"type": "m", "z": c["z"], "perms": c["perms"], "sig": c["sig"], "std": c["std"], "c": c["c"],
             "R_desc": Rd.T, "R_d_desc_alpha": r_d_desc_alpha(Rdd, c["alphas_F"])}
    E, F = ho.energy_forces(arrays(model), c["R"], np.float64)
    E_ref, F_ref, cint = c["E"], c["F"], float(c["c"])
    assert E.shape == E_ref.shape and F.shape == F_ref.shape
    dF, dE = np.max(np.abs(F - F_ref)), np.max(np.abs(E - E_ref))
    bF = 10 * float(c["band_F"]) * np.max(np.abs(F_ref))
    bE = 10 * float(c["band_E"]) * np.max(np.abs(E_ref - cint))
    print(f"{name}: max|dF| = {dF:.3e} (bound {bF:.3e})   max|dE| = {dE:.3e} (bound {bE:.3e})")
    assert dF <= bF and dE <= bE


# ---------------------------------------------------------------- 2. Hessian against differences
@pytest.mark.parametrize("ecstr", [False, True], ids=["plain", "ecstr"])
@pytest.mark.parametrize("key", FD_CASES, ids=lambda k: f"n{k[0]}-M{k[1]}-{k[2]}")
def test_hessian_is_minus_the_derivative_of_the_forces(key, ecstr):
    """Long-double `hessian` against -(4 D_h - D_2h) / 3 of the long-double forces, relative to
    max|H|.  Measured (x87 long double), h = 1e-3 / 3e-4 / 1e-4:
        n3-M4-s3     plain 4.0e-12 / 3.2e-14 / 1.0e-15   ecstr 2.5e-12 / 2.0e-14 / 1.6e-15
        n4-M33-swap  plain 1.7e-12 / 1.4e-14 / 2.0e-15   ecstr 6.4e-12 / 5.1e-14 / 1.6e-15
        n9-M17-c3    plain 1.4e-12 / 1.1e-14 / 2.4e-15   ecstr 2.5e-12 / 2.0e-14 / 2.52e-15
    The truncation error falls as h^4 down to h = 1e-4, where the rounding of the differences
    (2^-64 / h) takes over: h = 1e-4 is the best step, its largest figure 2.52e-15, the bound
    10 x that = 2.52e-14 -- far below the 1e-10 the test needs to stay under to see a missing or
    mis-signed term (1e-3 or more)."""
    assert FD_BOUND < 1e-10
    ma, _, r = fd_case(*key, ecstr)
    H = ho.hessian(ma, r[None], LD)[0]
    top = np.max(np.abs(H))
    devs = [float(np.max(np.abs(H - ho.fd_hessian(ma, r, h, LD))) / top) for h in FD_STEPS]
    print(f"{key} ecstr={ecstr}: |H + dF/dR| / max|H| at h = {FD_STEPS}: "
          + " / ".join(f"{d:.3e}" for d in devs) + f"   bound {FD_BOUND:.3e}")
    assert devs[-1] <= FD_BOUND


# ---------------------------------------------------------------- 3. structure
@pytest.mark.parametrize("ecstr", [False, True], ids=["plain", "ecstr"])
@pytest.mark.parametrize("key", FD_CASES, ids=lambda k: f"n{k[0]}-M{k[1]}-{k[2]}")
def test_symmetric_and_translation_invariant(key, ecstr):
    ma, _, r = fd_case(*key, ecstr)
    n = key[0]
    H = ho.hessian(ma, r[None], LD)[0]
    top = np.max(np.abs(H))
    sym = float(np.max(np.abs(H - H.T)) / top)
    tr = float(np.max(np.abs(H.reshape(3 * n, n, 3).sum(axis=1))) / top)
    print(f"{key} ecstr={ecstr}: asymmetry {sym:.3e}, row sums over the atoms {tr:.3e} (of max|H|)")
    assert sym <= 2.0 ** -60 and tr <= 2.0 ** -60


def test_both_groupings_of_the_descriptor_form_agree():
    """J^T (G J) with the D x D matrix G formed, and with G J formed term by term (the form the
    oracle uses past D = 512): the same sums in another order."""
    ma, _, r = fd_case(9, 17, "c3", True)
    H = ho.hessian(ma, r[None], LD, explicit_G=True)[0]
    H2 = ho.hessian(ma, r[None], LD, explicit_G=False)[0]
    d = float(np.max(np.abs(H - H2)) / np.max(np.abs(H)))
    print(f"explicit G against G J term by term: {d:.3e} of max|H|")
    assert d <= 2.0 ** -58


# ---------------------------------------------------------------- 4. the coincident query
@pytest.mark.parametrize("ecstr", [False, True], ids=["plain", "ecstr"])
@pytest.mark.parametrize("key", FD_CASES, ids=lambda k: f"n{k[0]}-M{k[1]}-{k[2]}")
def test_query_equal_to_a_training_geometry(key, ecstr):
    """diff = 0 exactly for (j, p) = (0, identity) in float64 (the query's descriptor is formed
    like the model's): beta is 0 / 0 without the guard.  The float64 result is finite and within
    10 band of the long-double one, band = the float64 oracle's deviation from the long-double
    one at a generic query of the same model, floored at 2^-52 (the GPU tests' rule)."""
    ma, Rtr, r = fd_case(*key, ecstr)
    ident = np.asarray(ma["perms"])[0]
    assert np.array_equal(ident, np.arange(key[0]))
    r0 = Rtr[0]
    H64 = ho.hessian(ma, r0[None], np.float64)[0]
    assert np.all(np.isfinite(H64))
    Hld = ho.hessian(ma, r0[None], LD)[0]
    top = np.max(np.abs(Hld))
    dev = float(np.max(np.abs(H64 - Hld)) / top)
    # the band of a generic query of this case: the float64 oracle's own deviation, floored
    Hg = ho.hessian(ma, r[None], LD)[0]
    band = max(FLOOR, float(np.max(np.abs(ho.hessian(ma, r[None], np.float64)[0] - Hg)) / np.max(np.abs(Hg))))
    print(f"{key} ecstr={ecstr}: coincident query float64 vs long double {dev:.3e}, band {band:.3e}")
    assert dev <= 10 * band
