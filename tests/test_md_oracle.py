"""The trajectory oracle (tests/md_oracle.py) and the host-side helpers of GDMLPredict.md on the
CPU.  The GPU tests hold `GDMLPredict.md` against the oracle; here the oracle is anchored by what
velocity Verlet must do whatever the force field: its total-energy error is second order in the
step, and it retraces its path when the velocities are reversed.  Every test prints its figures
before it asserts.
"""
import numpy as np
import pytest

from tests import md_oracle as mo
from tests.sgdml_shapes import FLOOR, LD, MIN_DIST

CASES = [(2, 1, "id"), (9, 17, "c3"), (25, 3, "id")]
ACC = 4.184e-4


def case_id(k):
    return f"n{k[0]}-M{k[1]}-{k[2]}"


def total_energy(tr, masses):
    from sgdml_amd.predict import kinetic_energy

    return tr["E"] + kinetic_energy(tr["V"], masses, ACC)


# ---------------------------------------------------------------- 1. second order
@pytest.mark.parametrize("ecstr", [False, True], ids=["plain", "ecstr"])
@pytest.mark.parametrize("key", CASES, ids=case_id)
def test_total_energy_error_is_second_order(key, ecstr):
    """The drift of E + E_kin after 8 fs with dt = 0.5 (16 steps) against dt = 0.25 (32 steps), in
    long double: a ratio of 4 for every replica whose error is above the arithmetic's noise."""
    _, ma, R0, V0, masses = mo.start(*key, ecstr, 3, 4000 * key[0] + key[1])
    err = []
    for dt, steps in ((0.5, 16), (0.25, 32)):
        tr = mo.verlet(ma, R0, V0, masses, dt, steps, steps, ACC, LD)
        assert tr["E"].dtype == LD and tr["R"].shape == (3, 2, key[0], 3)
        Et = total_energy(tr, masses.astype(LD))
        err.append(np.abs(Et[:, 1] - Et[:, 0]))
        if dt == 0.5:
            a, b = np.tril_indices(key[0], k=-1)
            moved = float(np.max(np.linalg.norm((tr["R"][:, 1] - tr["R"][:, 0]).astype(np.float64), axis=2)))
            closest = float(np.min(np.linalg.norm((tr["R"][:, 1][:, a] - tr["R"][:, 1][:, b]).astype(np.float64), axis=2)))
            ekin = kinetic_energy_of(tr, masses)
    ok = err[0] > 1e-12
    ratio = err[0][ok] / err[1][ok]
    print(f"{case_id(key)} ecstr={ecstr}: |dE_tot| at dt 0.5 = {[f'{float(x):.3e}' for x in err[0]]}, at dt 0.25 = "
          f"{[f'{float(x):.3e}' for x in err[1]]}, ratio = {[f'{float(x):.3f}' for x in ratio]}; E_kin = "
          f"{[f'{float(x):.2f}' for x in ekin]}, largest displacement {moved:.3f}, closest pair {closest:.3f}")
    assert closest > MIN_DIST
    assert 2 * int(np.sum(ok)) >= ok.size
    assert np.all((ratio >= 3.5) & (ratio <= 4.5))


def kinetic_energy_of(tr, masses):
    from sgdml_amd.predict import kinetic_energy

    return kinetic_energy(tr["V"][:, 0], masses.astype(LD), ACC)


# ---------------------------------------------------------------- 2. reversibility
@pytest.mark.parametrize("ecstr", [False, True], ids=["plain", "ecstr"])
@pytest.mark.parametrize("key", CASES, ids=case_id)
def test_reversed_velocities_retrace_the_path(key, ecstr):
    """k = 8 steps, V -> -V, 8 steps: the float64 oracle is back at R0 within 10 x the band of that
    run, the largest deviation of its frames from the long-double oracle's (there and back),
    floored at 2^-52 max|R0|; the long-double oracle itself within 2^-52 max|R0|."""
    _, ma, R0, V0, masses = mo.start(*key, ecstr, 3, 4000 * key[0] + key[1])
    k, dt = 8, 0.5
    back, frames = {}, {}
    for dtype in (np.float64, LD):
        fwd = mo.verlet(ma, R0, V0, masses, dt, k, 1, ACC, dtype)
        ret = mo.verlet(ma, fwd["R"][:, -1], -fwd["V"][:, -1], masses, dt, k, 1, ACC, dtype)
        back[dtype] = ret["R"][:, -1]
        frames[dtype] = np.concatenate([fwd["R"], ret["R"]], axis=1)
        assert np.array_equal(fwd["R"][:, 0], R0.astype(dtype))
    top = float(np.max(np.abs(R0)))
    band = max(FLOOR * top, float(np.max(np.abs(frames[np.float64].astype(LD) - frames[LD]))))
    dev = float(np.max(np.abs(back[np.float64] - R0)))
    dev_ld = float(np.max(np.abs(back[LD] - R0.astype(LD))))
    moved = float(np.max(np.abs(frames[LD][:, k] - R0.astype(LD))))
    print(f"{case_id(key)} ecstr={ecstr}: |R_back - R0| = {dev:.3e} (long double {dev_ld:.3e}), band {band:.3e}, "
          f"bound {10 * band:.3e}; largest coordinate change on the way {moved:.3e}")
    assert moved > 1e-3
    assert dev_ld <= FLOOR * top
    assert dev <= 10 * band


def test_frames_are_the_strided_steps():
    _, ma, R0, V0, masses = mo.start(3, 4, "nongroup", True, 2, 5)
    one = mo.verlet(ma, R0, V0, masses, 0.5, 8, 1, ACC)
    four = mo.verlet(ma, R0, V0, masses, 0.5, 8, 4, ACC)
    assert np.array_equal(four["step"], [0, 4, 8]) and np.array_equal(one["step"], np.arange(9))
    for k in ("R", "V", "E", "F"):
        assert np.array_equal(four[k], one[k][:, ::4]), k
    zero = mo.verlet(ma, R0, V0, masses, 0.5, 0, 1, ACC)
    assert np.array_equal(zero["R"][:, 0], R0) and np.array_equal(zero["V"][:, 0], V0)


# ---------------------------------------------------------------- 3. the host-side helpers
def test_normalize_md_inputs_accepts_every_documented_shape():
    from sgdml_amd.predict import normalize_md_inputs

    n = 4
    rng = np.random.default_rng(0)
    R, V, m = rng.standard_normal((3, n, 3)), rng.standard_normal((3, n, 3)), rng.uniform(1, 16, n)
    for r, q in ((R, 3), (R.reshape(3, 12), 3), (R[0], 1), (R[0].reshape(12), 1)):
        vs = (V, V.reshape(3, 12)) if q == 3 else (V[:1], V[:1].reshape(1, 12), V[0], V[0].reshape(12))
        for v in vs:
            Rn, Vn, mn, dt, steps, stride = normalize_md_inputs(r, v, m, 0.5, np.int64(12), 4, n)
            assert Rn.shape == (q, n, 3) and Vn.shape == (q, 12) and mn.shape == (n,)
            assert Rn.flags.c_contiguous and Vn.flags.c_contiguous and Rn.dtype == Vn.dtype == np.float64
            assert np.array_equal(Rn, R[:q]) and np.array_equal(Vn, V[:q].reshape(q, 12)) and np.array_equal(mn, m)
            assert (dt, steps, stride) == (0.5, 12, 4) and type(steps) is int and type(stride) is int
    assert normalize_md_inputs(R, V, list(m), -0.5, 0, 1, n)[3:] == (-0.5, 0, 1)
    e = normalize_md_inputs(np.empty((0, n, 3)), np.empty((0, 12)), m, 0.5, 2, 1, n)
    assert e[0].shape == (0, n, 3) and e[1].shape == (0, 12)


def test_normalize_md_inputs_refuses_bad_inputs():
    from sgdml_amd.predict import normalize_md_inputs

    n = 4
    R, V, m = np.zeros((3, n, 3)), np.zeros((3, n, 3)), np.ones(n)
    bad = [
        (np.zeros((3, n, 2)), V, m, 0.5, 4, 1),              # R: not a geometry
        (R, np.zeros((2, n, 3)), m, 0.5, 4, 1),              # V0: another Q
        (R, np.zeros((3, 11)), m, 0.5, 4, 1),                # V0: not 3n
        (R, np.zeros(12), m, 0.5, 4, 1),                     # one velocity for three geometries
        (R, np.zeros((3, 3, n)), m, 0.5, 4, 1),
        (R, V, np.ones(n + 1), 0.5, 4, 1),                   # masses: another n
        (R, V, np.ones((n, 1)), 0.5, 4, 1),
        (R, V, np.array([1.0, 0.0, 1.0, 1.0]), 0.5, 4, 1),   # masses: not > 0
        (R, V, np.array([1.0, -2.0, 1.0, 1.0]), 0.5, 4, 1),
        (R, V, np.array([1.0, np.inf, 1.0, 1.0]), 0.5, 4, 1),
        (R, V, np.array([1.0, np.nan, 1.0, 1.0]), 0.5, 4, 1),
        (R, V, m, np.inf, 4, 1), (R, V, m, np.nan, 4, 1), (R, V, m, "fast", 4, 1),   # dt
        (R, V, m, 0.5, -1, 1), (R, V, m, 0.5, 4, 0), (R, V, m, 0.5, 4, -2),          # steps, stride
        (R, V, m, 0.5, 5, 2), (R, V, m, 0.5, 4.0, 1), (R, V, m, 0.5, 4, 1.5),
    ]
    for args in bad:
        with pytest.raises(ValueError):
            normalize_md_inputs(*args, n)


def test_kinetic_energy_is_the_direct_sum():
    from sgdml_amd.predict import ACC_KCAL_MOL_A_AMU_FS, kinetic_energy

    assert ACC_KCAL_MOL_A_AMU_FS == ACC
    rng = np.random.default_rng(1)
    n = 5
    V, m = rng.standard_normal((2, 3, n, 3)), rng.uniform(1, 16, n)
    ref = np.zeros((2, 3), dtype=LD)
    for q in range(2):
        for t in range(3):
            for i in range(n):
                ref[q, t] += LD(0.5) * LD(m[i]) * sum(LD(V[q, t, i, c]) ** 2 for c in range(3)) / LD(ACC)
    for got in (kinetic_energy(V, m), kinetic_energy(V.reshape(2, 3, 3 * n), m, ACC)):
        assert got.shape == (2, 3) and got.dtype == np.float64
        dev = float(np.max(np.abs(got - ref) / ref))
        print(f"kinetic_energy: largest relative deviation from the long-double sum {dev:.3e}")
        assert dev <= 3 * n * FLOOR
    assert kinetic_energy(V[0, 0], m).shape == () and kinetic_energy(V[0, 0].ravel(), m, 2 * ACC) * 2 == pytest.approx(
        float(ref[0, 0]), rel=1e-14)
    with pytest.raises(ValueError):
        kinetic_energy(np.zeros((2, 7)), m)


# ---------------------------------------------------------------- 4. the C entry points
def test_abi_rejects_a_null_context():
    from sgdml_amd import _native

    lib = _native.load_library()
    assert lib.mlff_md_run(None, None, None, None, 1, 0.5, 1, 1, 0, None, None, None, None) == _native.MLFF_ERR_ARG
    assert lib.mlff_md_info(None, None, None, None) == _native.MLFF_ERR_ARG
