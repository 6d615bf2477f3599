"""GPU prediction of energies and forces (sgdml_amd.GDMLPredict -> mlff_predict,
csrc/kernels_predict.hip) against the reference's GDMLPredict.predict.

Fixture: tests/golden/sgdml_predict_cases.npz (make_predict_golden.py): per case the model's
sources, the queries, the reference's E, F and the reference's own spread (band_F, band_E:
as is / chunk_size = 1 / training points reversed).  The model arrays are rebuilt here with the
project's host code (host_descriptors, r_d_desc_alpha), which the generator asserts to equal the
reference's create_model bit for bit.

Bounds (the tests/parity.py rule, 10 x the measured band):
    |F - F_ref| <= 10 band_F max|F_ref|,   |E - E_ref| <= 10 band_E max|E_ref - c|.
Every test prints its figures before it asserts.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CASES = ["d3", "d21", "eth", "eth3", "eth3ng", "eth_rows", "tube"]
TILE_MAX_D = 288


@pytest.fixture(scope="module")
def sg():
    import sgdml_amd

    if sgdml_amd.device_count() < 1:
        pytest.fail("no GPU visible to libmlffpcg.so")
    return sgdml_amd


@pytest.fixture(scope="module")
def cases(golden_dir):
    from sgdml_amd.model import r_d_desc_alpha
    from sgdml_amd.solver import host_descriptors

    f = np.load(golden_dir / "sgdml_predict_cases.npz", allow_pickle=False)
    assert sorted(f["cases"]) == sorted(CASES)
    out = {}
    for name in CASES:
        c = {k[len(name) + 2:]: f[k] for k in f.files if k.startswith(name + "__")}
        Rd, Rdd = host_descriptors(c["R_train"])
        c["model"] = {"type": "m", "z": c["z"], "perms": c["perms"], "sig": c["sig"], "std": c["std"],
                      "c": c["c"], "R_desc": Rd.T, "R_d_desc_alpha": r_d_desc_alpha(Rdd, c["alphas_F"])}
        for a in c.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        out[name] = c
    return out


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(golden_dir / "sgdml_model_ethanol_n621.npz", allow_pickle=False)


def dim_d(case):
    n = case["z"].size
    return n * (n - 1) // 2


def check(tag, E, F, E_ref, F_ref, c, band_F, band_E):
    dF = np.max(np.abs(F - F_ref))
    dE = np.max(np.abs(E - E_ref))
    bF = 10 * band_F * np.max(np.abs(F_ref))
    bE = 10 * band_E * np.max(np.abs(E_ref - c))
    print(f"{tag}: max|dF| = {dF:.3e} (bound {bF:.3e}, {dF / bF:.2f} of it)   "
          f"max|dE| = {dE:.3e} (bound {bE:.3e}, {dE / bE:.2f} of it)")
    assert dF <= bF, (tag, "F", dF, bF)
    assert dE <= bE, (tag, "E", dE, bE)


# ---------------------------------------------------------------- 1. against the reference
@pytest.mark.parametrize("form", ["tile", "stream"])
@pytest.mark.parametrize("name", CASES)
def test_matches_reference(sg, cases, name, form, monkeypatch):
    c = cases[name]
    if form == "tile" and dim_d(c) > TILE_MAX_D:
        # the tile form does not exist for this D: asking for it is an argument error
        monkeypatch.setenv("MLFF_PRED_FORM", "tile")
        with pytest.raises(ValueError):
            sg.GDMLPredict(c["model"], device=0)
        return
    monkeypatch.setenv("MLFF_PRED_FORM", form)
    with sg.GDMLPredict(c["model"], device=0) as gd:
        assert gd.form == form
        E, F = gd.predict(c["R"])
    assert E.shape == c["E"].shape and F.shape == c["F"].shape
    check(f"{name}/{form}", E, F, c["E"], c["F"], float(c["c"]), float(c["band_F"]), float(c["band_E"]))


def test_default_form_follows_d(sg, cases, monkeypatch):
    monkeypatch.delenv("MLFF_PRED_FORM", raising=False)
    for name, form in (("eth3", "tile"), ("tube", "stream")):
        with sg.GDMLPredict(cases[name]["model"], device=0) as gd:
            assert gd.form == form
            assert gd.flops_per_query > 0 and gd.bytes_per_query > 0 and gd.slab >= 1


# ---------------------------------------------------------------- 2. training points
def test_training_points_of_the_reference_model(sg, cases, fx):
    """The reference's own model arrays (its GDMLTrain.train output) at its training points,
    against its prediction with c = 0 (fixture E_pred_c0, F_pred_c0); the bands of case `eth`
    (the same model)."""
    m = {k[len("model__"):]: fx[k] for k in fx.files if k.startswith("model__")}
    c = float(m["c"])
    with sg.GDMLPredict(m, device=0) as gd:
        E, F = gd.predict(fx["R"])
    eth = cases["eth"]
    check("n621 training points", E, F, fx["E_pred_c0"] + c, fx["F_pred_c0"], c,
          float(eth["band_F"]), float(eth["band_E"]))


def test_forces_equal_the_operator(sg, cases, fx):
    """K_op alphas is the force prediction at the training points with std = 1, c = 0: the new
    kernels against the golden-pinned operator.  (mlff_set_operator wants lam > 0: 1e-300 adds
    nothing to any entry in fp64.)"""
    alphas = np.ascontiguousarray(fx["model__alphas_F"])
    Rd, Rdd = sg.host_descriptors(fx["R"])
    with sg.KernelSolver(alphas.size, device=0) as s:
        s.sgdml_operator(Rd, Rdd, fx["perms"], 10.0)
        s.set_operator(1.0, 1e-300)
        y = s.matvec(alphas)
    m = {"z": fx["z"], "perms": fx["perms"], "sig": 10.0, "std": 1.0, "c": 0.0,
         "R_desc": fx["model__R_desc"], "R_d_desc_alpha": fx["model__R_d_desc_alpha"]}
    with sg.GDMLPredict(m, device=0) as gd:
        _, F = gd.predict(fx["R"])
    bound = 10 * float(cases["eth"]["band_F"]) * np.max(np.abs(y))
    d = np.max(np.abs(F.ravel() - y))
    print(f"predict vs operator: max|dF| = {d:.3e} (bound {bound:.3e}), max|F| = {np.max(np.abs(y)):.3e}")
    assert d <= bound


# ---------------------------------------------------------------- 3. bitwise batch invariance
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
        assert gd.form == form
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


# ---------------------------------------------------------------- 4. several contexts
def test_devices_split_is_bit_identical(sg, cases):
    c = cases["eth3"]
    with sg.GDMLPredict(c["model"], device=0) as gd:
        E, F = gd.predict(c["R"])
    with sg.GDMLPredict(c["model"], devices=[0, 0, 0]) as gd:
        E3, F3 = gd.predict(c["R"])            # 70 queries: 24 + 24 + 22
        E2, F2 = gd.predict(c["R"][:2])        # 2 queries: one empty block
    assert np.array_equal(E3, E) and np.array_equal(F3, F)
    assert np.array_equal(E2, E[:2]) and np.array_equal(F2, F[:2])


# ---------------------------------------------------------------- 5. forces are the gradient
def test_forces_are_the_gradient_of_the_energy(sg, cases):
    """Central differences of the predicted E at h = 1e-4, the 54 displaced geometries in one
    batch: max |-dE / 2h - F| <= 1e-6 max|F| (the reference itself: 3.3e-8; its E rounding of
    ~2e-13 contributes ~2e-9)."""
    c = cases["eth"]
    r0 = c["R"][2].ravel()
    h = 1e-4
    disp = np.repeat(r0[None, :], 54, axis=0)
    disp[np.arange(27), np.arange(27)] += h
    disp[27 + np.arange(27), np.arange(27)] -= h
    with sg.GDMLPredict(c["model"], device=0) as gd:
        _, F = gd.predict(r0)
        E, _ = gd.predict(disp)
    F_fd = -(E[:27] - E[27:]) / (2 * h)
    d = np.max(np.abs(F_fd - F[0]))
    print(f"finite differences: max|-dE/2h - F| = {d:.3e}, max|F| = {np.max(np.abs(F)):.3e}, "
          f"ratio {d / np.max(np.abs(F)):.3e}")
    assert d <= 1e-6 * np.max(np.abs(F))


# ---------------------------------------------------------------- 6. round trip
def test_train_store_predict_round_trip(sg, fx, tmp_path):
    from sgdml_amd import model as mdl
    from tests.test_gpu_model import task_of

    task = task_of(fx)
    n = fx["model__alphas_F"].size
    m = mdl.train(task, break_percentage=int(fx["k_rot"]) / n, str_preconditioner="cholesky")
    assert m["use_E"] and np.isnan(m["f_err"]["rmse"]) and m["n_test"] == 0
    m.update(hardware="mi355x", n_datapoints=int(fx["R"].shape[0]), str_preconditioner="cholesky")
    path = mdl.store_model(m, tmp_path)
    with sg.GDMLPredict(path, device=0) as gd:
        E, F = gd.predict(fx["R"])
    # the training-set energies the integration constant was regressed on
    Rd, Rdd = sg.host_descriptors(fx["R"])
    with sg.KernelSolver(n, device=0) as s:
        s.sgdml_operator(Rd, Rdd, fx["perms"], 10.0)
        _, E_raw = s.sgdml_energies(np.ascontiguousarray(m["alphas_F"]))
    E_exp = E_raw * m["std"] + m["c"]
    dE = np.max(np.abs(E - E_exp))
    print(f"round trip: max|dE| = {dE:.3e}, max|raw std| = {np.max(np.abs(E_raw * m['std'])):.3e}")
    assert dE <= 1e-12 * np.max(np.abs(E_raw * m["std"]))
    out = mdl.test_errors(m, fx["R"], fx["F"], fx["E"], device=0, update=True)
    assert out["n_test"] == 23 and m["n_test"] == 23
    for part in (out["f_err"], out["e_err"]):
        assert np.isfinite(part["mae"]) and np.isfinite(part["rmse"])
    rmse = np.sqrt(np.mean((fx["F"].reshape(23, -1) - F) ** 2))
    np.testing.assert_allclose(out["f_err"]["rmse"], rmse, rtol=1e-12)
    assert m["f_err"] == out["f_err"] and m["e_err"] == out["e_err"]


# ---------------------------------------------------------------- 7. state and errors
def test_state_and_errors(sg, cases):
    a, b = cases["eth3"], cases["eth3ng"]          # both 3 n M = 270
    R = a["R"][:4].reshape(4, 9, 3)
    with sg.GDMLPredict(b["model"], device=0) as gd:
        Eb, Fb = gd.predict(R)
    with sg.KernelSolver(270, device=0) as s:
        with pytest.raises(RuntimeError):          # MLFF_ERR_STATE: no model yet
            s.predict(R)
        with pytest.raises(RuntimeError):
            s.predict_info()
        for case in (a, b):                        # the second model replaces the first
            m = case["model"]
            s.predict_set_model(m["R_desc"].T, m["R_d_desc_alpha"], m["perms"], float(m["sig"]),
                                float(m["std"]), float(m["c"]))
        E, F = s.predict(R)
        assert np.array_equal(E, Eb) and np.array_equal(F, Fb)
        E0, F0 = s.predict(np.empty((0, 9, 3)))    # Q = 0
        assert E0.shape == (0,) and F0.shape == (0, 27)
        with pytest.raises(ValueError):            # a model of another size: N != 3 n M
            m = cases["d3"]["model"]
            s.predict_set_model(m["R_desc"].T, m["R_d_desc_alpha"], m["perms"], 10.0)
        E, F = s.predict(R)                        # the model set before stays
        assert np.array_equal(E, Eb) and np.array_equal(F, Fb)
