"""GPU prediction with energy-constrained sGDML models (`alphas_E`, use_E_cstr): the ECSTR
instantiations of k_pr_pair / k_pr_stream (csrc/kernels_predict.hip) through
sgdml_amd.GDMLPredict, against the reference's GDMLPredict.predict (predict.py:206-218).

Fixtures: tests/golden/sgdml_predict_ecstr_cases.npz (make_predict_ecstr_golden.py) -- group 1:
the models of sgdml_predict_cases.npz with random alphas_E, the reference's E, F and its own
spread; group 2: the reference's trained eth_ecstr / ethp_ecstr models of
sgdml_analytic_cases.npz at 12 queries with the spread over its four training variants -- and
the long-double oracle of tests/sgdml_shapes.py.

Bounds (the project's rule): 10 x the reference's own band, floored at 2^-52, relative to
max|F_ref| and max|E_ref - c|.  Every test prints its figures before it asserts.
"""
import numpy as np
import pytest

from tests import sgdml_shapes as sh
from tests.sgdml_shapes import SIG, held

pytestmark = pytest.mark.gpu

CASES = ["d3", "d21", "eth3", "eth3ng", "eth", "tube"]
TRAINED = ["eth_ecstr", "ethp_ecstr"]
TILE_MAX_D = 288
FLOOR = 2.0 ** -52


@pytest.fixture(scope="module")
def sg():
    import sgdml_amd

    if sgdml_amd.device_count() < 1:
        pytest.fail("no GPU visible to libmlffpcg.so")
    return sgdml_amd


@pytest.fixture(scope="module")
def cases(golden_dir):
    """Group 1: the sources of sgdml_predict_cases.npz, the energy coefficients and the
    reference's results of sgdml_predict_ecstr_cases.npz; `model` with alphas_E, `model0`
    without."""
    from sgdml_amd.model import r_d_desc_alpha
    from sgdml_amd.solver import host_descriptors

    src = np.load(golden_dir / "sgdml_predict_cases.npz", allow_pickle=False)
    f = np.load(golden_dir / "sgdml_predict_ecstr_cases.npz", allow_pickle=False)
    assert list(f["cases"]) == CASES
    out = {}
    for name in CASES:
        c = {k: src[f"{name}__{k}"] for k in ("R_train", "z", "perms", "alphas_F", "std", "c", "R", "sig")}
        c.update({k[len(name) + 2:]: f[k] for k in f.files if k.startswith(name + "__")})
        Rd, Rdd = host_descriptors(c["R_train"])
        c["model0"] = {"type": "m", "z": c["z"], "perms": c["perms"], "sig": c["sig"], "std": c["std"],
                       "c": c["c"], "R_desc": Rd.T, "R_d_desc_alpha": r_d_desc_alpha(Rdd, c["alphas_F"])}
        c["model"] = dict(c["model0"], alphas_E=c["alphas_E"])
        for a in c.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        out[name] = c
    return out


def dim_d(case):
    n = case["z"].size
    return n * (n - 1) // 2


def check(tag, E, F, E_ref, F_ref, c, band_F, band_E):
    dF = np.max(np.abs(F - F_ref))
    dE = np.max(np.abs(E - E_ref))
    bF = 10 * max(band_F, FLOOR) * np.max(np.abs(F_ref))
    bE = 10 * max(band_E, FLOOR) * np.max(np.abs(E_ref - c))
    print(f"{tag}: max|dF| = {dF:.3e} (bound {bF:.3e}, {dF / bF:.2f} of it)   "
          f"max|dE| = {dE:.3e} (bound {bE:.3e}, {dE / bE:.2f} of it)")
    assert dF <= bF, (tag, "F", dF, bF)
    assert dE <= bE, (tag, "E", dE, bE)


# ---------------------------------------------------------------- 1. against the reference
@pytest.mark.parametrize("form", ["tile", "stream"])
@pytest.mark.parametrize("name", CASES)
def test_matches_reference(sg, cases, name, form, monkeypatch):
    c = cases[name]
    assert float(np.min(c["share"])) >= 1e-3       # both coefficient sets show in E and in F
    if form == "tile" and dim_d(c) > TILE_MAX_D:
        monkeypatch.setenv("MLFF_PRED_FORM", "tile")
        with pytest.raises(ValueError):
            sg.GDMLPredict(c["model"], device=0)
        return
    monkeypatch.setenv("MLFF_PRED_FORM", form)
    with sg.GDMLPredict(c["model"], device=0) as gd:
        assert gd.form == form and gd.use_E_cstr
        E, F = gd.predict(c["R"])
    assert E.shape == c["E"].shape and F.shape == c["F"].shape
    check(f"{name}/{form}", E, F, c["E"], c["F"], float(c["c"]), float(c["band_F"]), float(c["band_E"]))


def test_work_counts_the_constrained_pair(sg, cases):
    """mlff_predict_info: 9 D + 19 flops per pair with energy coefficients, 9 D + 10 without."""
    c = cases["eth3"]
    D, MP = dim_d(c), c["R_train"].shape[0] * c["perms"].shape[0]
    with sg.GDMLPredict(c["model0"], device=0) as g0, sg.GDMLPredict(c["model"], device=0) as g1:
        assert not g0.use_E_cstr and g1.use_E_cstr
        assert g0.flops_per_query == MP * (9 * D + 10) and g1.flops_per_query == MP * (9 * D + 19)
        assert g0.bytes_per_query == 16 * MP * D and g1.bytes_per_query == 8 * MP * (2 * D + 1)


# ---------------------------------------------------------------- 2. zero coefficients
@pytest.mark.parametrize("name,form", [("eth3", "tile"), ("eth3", "stream"), ("tube", "stream")])
def test_zero_coefficients_give_the_unconstrained_bits(sg, cases, name, form, monkeypatch):
    c = cases[name]
    monkeypatch.setenv("MLFF_PRED_FORM", form)
    zero = dict(c["model0"], alphas_E=np.zeros(c["R_train"].shape[0]))
    with sg.GDMLPredict(c["model0"], device=0) as gd:
        assert gd.form == form and not gd.use_E_cstr
        E0, F0 = gd.predict(c["R"])
    with sg.GDMLPredict(zero, device=0) as gd:
        assert gd.form == form and gd.use_E_cstr
        E, F = gd.predict(c["R"])
    assert np.array_equal(E, E0) and np.array_equal(F, F0)


# ---------------------------------------------------------------- 3. shape sweep
@pytest.mark.parametrize("key", sh.CASES, ids=sh.case_id)
def test_shape_sweep_against_the_long_double_oracle(sg, key, monkeypatch):
    """The constrained operator [x_F; x_E] -> K_c x through the predictor at the training
    geometries (std = 1, c = 0): F = (K_c x)[:N], E = -(K_c x)[N:], each part against its own
    maximum (the rule of test_operator_energy_constraints / test_prediction_at_training_points)."""
    from sgdml_amd.model import r_d_desc_alpha

    c = sh.case(*key)
    Rd, Rdd = c.desc
    N = c.N
    model = {"type": "m", "z": np.ones(c.n, dtype=np.int64), "perms": c.perms, "sig": SIG,
             "std": 1.0, "c": 0.0, "R_desc": Rd.T, "R_d_desc_alpha": r_d_desc_alpha(Rdd, c.xE[:N]),
             "alphas_E": np.ascontiguousarray(c.xE[N:])}
    default = "tile" if c.D <= TILE_MAX_D else "stream"
    cut_F, cut_E = (lambda a: a[:N]), (lambda a: a[N:])
    F_ref, E_ref = cut_F(c.ref("KopE")).reshape(c.M, c.n3), -cut_E(c.ref("KopE"))
    for form in [None] + (["stream"] if default == "tile" else []):
        if form is None:
            monkeypatch.delenv("MLFF_PRED_FORM", raising=False)
        else:
            monkeypatch.setenv("MLFF_PRED_FORM", form)
        with sg.GDMLPredict(model, device=0) as gd:
            assert gd.form == (form or default) and gd.use_E_cstr
            E, F = gd.predict(c.R)
        held(F, F_ref, c.band("KopE", cut_F), f"{c.label} ecstr predict F/{gd.form}")
        held(E, E_ref, c.band("KopE", cut_E), f"{c.label} ecstr predict E/{gd.form}")


# ---------------------------------------------------------------- 4. bitwise batch invariance
@pytest.mark.parametrize("form", ["tile", "stream"])
def test_bitwise_batch_invariance(sg, cases, form, monkeypatch):
    from sgdml_amd import predict as prd

    c = cases["eth3"]
    R = c["R"]
    G = prd.tile_queries_per_workgroup(dim_d(c)) if form == "tile" else prd.STREAM_QUERY_BLOCK
    assert G + 1 <= R.shape[0]
    monkeypatch.setenv("MLFF_PRED_FORM", form)
    monkeypatch.delenv("MLFF_PRED_SLAB", raising=False)
    with sg.GDMLPredict(c["model"], device=0) as gd:
        assert gd.form == form and gd.use_E_cstr
        E, F = gd.predict(R)
        for b in (1, G - 1, G, G + 1):
            for lo in (0, 3, R.shape[0] - b):          # the same queries at other positions
                Eb, Fb = gd.predict(R[lo:lo + b])
                assert np.array_equal(Eb, E[lo:lo + b]), (form, b, lo)
                assert np.array_equal(Fb, F[lo:lo + b]), (form, b, lo)
        Er, Fr = gd.predict(R[::-1])
        assert np.array_equal(Er[::-1], E) and np.array_equal(Fr[::-1], F)
    monkeypatch.setenv("MLFF_PRED_SLAB", "5")
    with sg.GDMLPredict(c["model"], device=0) as gd:
        assert gd.slab == 5
        Es, Fs = gd.predict(R)
    assert np.array_equal(Es, E) and np.array_equal(Fs, F)


def test_devices_split_is_bit_identical(sg, cases):
    c = cases["eth3"]
    with sg.GDMLPredict(c["model"], device=0) as gd:
        E, F = gd.predict(c["R"])
    with sg.GDMLPredict(c["model"], devices=[0, 0, 0]) as gd:
        assert gd.use_E_cstr
        E3, F3 = gd.predict(c["R"])            # 70 queries: 24 + 24 + 22
        E2, F2 = gd.predict(c["R"][:2])        # 2 queries: one empty block
    assert np.array_equal(E3, E) and np.array_equal(F3, F)
    assert np.array_equal(E2, E[:2]) and np.array_equal(F2, F[:2])
    check("eth3 devices", E3, F3, c["E"], c["F"], float(c["c"]), float(c["band_F"]), float(c["band_E"]))


# ---------------------------------------------------------------- 5. forces are the gradient
def test_forces_are_the_gradient_of_the_energy(sg, cases):
    """Central differences of the predicted E at h = 1e-4 on the constrained `eth` model, the 54
    displaced geometries in one batch: max |-dE / 2h - F| <= 1e-6 max|F| (the reference itself
    with constraints: 4.2e-8 on eth, 8.3e-9 on eth3)."""
    c = cases["eth"]
    r0 = c["R"][2].ravel()
    h = 1e-4
    disp = np.repeat(r0[None, :], 54, axis=0)
    disp[np.arange(27), np.arange(27)] += h
    disp[27 + np.arange(27), np.arange(27)] -= h
    with sg.GDMLPredict(c["model"], device=0) as gd:
        assert gd.use_E_cstr
        _, F = gd.predict(r0)
        E, _ = gd.predict(disp)
    F_fd = -(E[:27] - E[27:]) / (2 * h)
    d = np.max(np.abs(F_fd - F[0]))
    print(f"finite differences (ecstr): max|-dE/2h - F| = {d:.3e}, max|F| = {np.max(np.abs(F)):.3e}, "
          f"ratio {d / np.max(np.abs(F)):.3e}")
    assert d <= 1e-6 * np.max(np.abs(F))


# ---------------------------------------------------------------- 6. train, store, predict, score
@pytest.mark.parametrize("case", TRAINED)
def test_train_store_predict_test_errors(sg, golden_dir, case, tmp_path):
    from sgdml_amd import model as mdl
    from tests.test_gpu_analytic import task_of

    an = np.load(golden_dir / "sgdml_analytic_cases.npz", allow_pickle=False)
    f = np.load(golden_dir / "sgdml_predict_ecstr_cases.npz", allow_pickle=False)
    assert sorted(f["trained"]) == sorted(TRAINED)
    g = lambda k: f[f"{case}__{k}"]  # noqa: E731
    task = task_of(an, case)
    assert task["use_E_cstr"]
    m = mdl.train(task)
    M = task["R_train"].shape[0]
    assert m["alphas_E"].shape == (M,) and np.isnan(m["f_err"]["rmse"]) and m["n_test"] == 0
    m.update(hardware="mi355x", n_datapoints=M)
    path = mdl.store_model(m, tmp_path)
    with sg.GDMLPredict(path, device=0) as gd:
        assert gd.use_E_cstr and gd.n_train == M
        E, F = gd.predict(g("Rq"))
    check(case, E, F, g("Eq"), g("Fq"), float(an[f"{case}__c"]), float(g("band_F")), float(g("band_E")))
    R, F_lab, E_lab = an[f"{case}__R"], an[f"{case}__F"], an[f"{case}__E"]
    out = mdl.test_errors(m, R, F_lab, E_lab, device=0, update=True)
    assert out["n_test"] == M and m["n_test"] == M
    for part in (out["f_err"], out["e_err"]):
        assert np.isfinite(part["mae"]) and np.isfinite(part["rmse"])
    with sg.GDMLPredict(m, device=0) as gd:
        _, F_tr = gd.predict(R)
    rmse = np.sqrt(np.mean((F_lab.reshape(M, -1) - F_tr) ** 2))
    print(f"{case}: f_err rmse {out['f_err']['rmse']:.3e}, e_err rmse {out['e_err']['rmse']:.3e}")
    np.testing.assert_allclose(out["f_err"]["rmse"], rmse, rtol=1e-12)
    assert m["f_err"] == out["f_err"] and m["e_err"] == out["e_err"]


# ---------------------------------------------------------------- 7. state
def test_state(sg, cases):
    a, b = cases["eth3"], cases["eth3ng"]          # both 3 n M = 270
    R = a["R"][:4].reshape(4, 9, 3)
    args = lambda m: (m["R_desc"].T, m["R_d_desc_alpha"], m["perms"], float(m["sig"]),  # noqa: E731
                      float(m["std"]), float(m["c"]))
    with sg.GDMLPredict(b["model0"], device=0) as gd:
        Eb0, Fb0 = gd.predict(R)
    with sg.GDMLPredict(a["model"], device=0) as gd:
        Ea, Fa = gd.predict(R)
    with sg.KernelSolver(270, device=0) as s:
        with pytest.raises(RuntimeError):          # MLFF_ERR_STATE: no model yet
            s.predict_set_energy_coefficients(a["alphas_E"])
        with pytest.raises(RuntimeError):
            s.predict_set_energy_coefficients(None)
        s.predict_set_model(*args(a["model"]), alphas_E=a["alphas_E"])
        E, F = s.predict(R)
        assert np.array_equal(E, Ea) and np.array_equal(F, Fa)
        assert not np.array_equal(F, Fb0)
        for bad in (np.zeros(9), np.zeros(11), np.zeros((10, 2))):
            with pytest.raises(ValueError):        # wrong length: the model set before stays
                s.predict_set_model(*args(b["model0"]), alphas_E=bad)
            with pytest.raises(ValueError):
                s.predict_set_energy_coefficients(bad)
        E, F = s.predict(R)
        assert np.array_equal(E, Ea) and np.array_equal(F, Fa)
        s.predict_set_model(*args(b["model0"]))    # an unconstrained model clears the coefficients
        E, F = s.predict(R)
        assert np.array_equal(E, Eb0) and np.array_equal(F, Fb0)
        s.predict_set_energy_coefficients(a["alphas_E"])   # set after the model ...
        E1, _ = s.predict(R)
        assert not np.array_equal(E1, Eb0)
        s.predict_set_energy_coefficients(None)            # ... and cleared again
        E, F = s.predict(R)
        assert np.array_equal(E, Eb0) and np.array_equal(F, Fb0)
