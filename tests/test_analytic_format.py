"""Host side of the closed-form ('analytic') training path: the label vector with energy
constraints against the reference's (tests/golden/sgdml_ethanol_n270_ecstr, make_golden.py
fx_ecstr), the refusals of sgdml_amd.model.train, and create_model's keys against the
reference's GDMLTrain.train(solver 'analytic') model (tests/golden/sgdml_analytic_cases,
make_analytic_golden.py).  CPU only; the GPU runs are tests/test_gpu_analytic.py."""
import numpy as np
import pytest

from sgdml_amd import model as mdl
from sgdml_amd.solver import host_descriptors


def task_of(R, F, E, z, perms, solver_name, use_E_cstr=False, lam=1e-15):
    M = R.shape[0]
    return {"type": "t", "dataset_name": np.array("ethanol"),
            "dataset_theory": np.array("synthetic"), "z": z, "R_train": R, "F_train": F,
            "E_train": E, "idxs_train": np.arange(M), "md5_train": "0",
            "idxs_valid": np.arange(0), "md5_valid": "0", "sig": 10, "lam": lam, "use_E": True,
            "use_E_cstr": use_E_cstr, "use_sym": np.atleast_2d(perms).shape[0] > 1,
            "use_cprsn": False, "solver_name": solver_name, "solver_tol": 1e-4,
            "n_inducing_pts_init": 25, "interact_cut_off": None, "perms": np.atleast_2d(perms)}


def test_label_vector_with_energy_constraints(golden_dir):
    f = np.load(golden_dir / "sgdml_ethanol_n270_ecstr.npz", allow_pickle=False)
    task = task_of(f["R"], f["F"], f["E"], f["z"], f["perms"], "analytic", use_E_cstr=True)
    y, y_std, E_mean = mdl.label_vector(task)
    np.testing.assert_array_equal(y, f["y"])
    assert y_std == float(f["y_std"])
    assert E_mean == np.mean(f["E"])
    # without the constraints: the forces alone
    y0, s0, m0 = mdl.label_vector(dict(task, use_E_cstr=False))
    assert m0 is None and s0 == np.std(f["F"].ravel())
    np.testing.assert_array_equal(y0, f["F"].ravel() / s0)


def test_train_refusals(golden_dir):
    f = np.load(golden_dir / "sgdml_ethanol_n270_ecstr.npz", allow_pickle=False)
    args = (f["R"], f["F"], f["E"], f["z"], f["perms"])
    with pytest.raises(ValueError, match="use_E_cstr"):
        mdl.train(task_of(*args, "cg", use_E_cstr=True))
    for name in ("analytic", "cg"):
        with pytest.raises(NotImplementedError, match="lattice"):
            mdl.train(dict(task_of(*args, name), lattice=np.eye(3)))
        with pytest.raises(NotImplementedError, match="compression"):
            mdl.train(dict(task_of(*args, name), use_cprsn=True))
    for name in ("cg_cholesky", "fk"):
        with pytest.raises(NotImplementedError, match=name):
            mdl.train(task_of(*args, name))


@pytest.mark.parametrize("case", ["eth", "ethp", "eth_ecstr", "ethp_ecstr"])
def test_create_model_keys(golden_dir, case):
    f = np.load(golden_dir / "sgdml_analytic_cases.npz", allow_pickle=False)
    g = lambda k: f[f"{case}__{k}"]  # noqa: E731
    ecstr = bool(g("use_E_cstr"))
    task = task_of(g("R"), g("F"), g("E"), g("z"), g("perms"), "analytic", use_E_cstr=ecstr,
                   lam=float(g("lam")))
    Rd, Rdd = host_descriptors(g("R"))
    y, y_std, _ = mdl.label_vector(task)
    assert y_std == float(g("std"))
    m = mdl.create_model(task, "analytic", Rd, Rdd, mdl.tril_perms_lin(g("perms")), y_std,
                         g("alphas_F"), alphas_E=g("alphas_E") if ecstr else None,
                         norm_y_train=np.linalg.norm(y))
    assert sorted(m) == list(g("model_keys"))
    assert m["solver_name"] == "analytic" and m["lam"] == float(g("lam"))
    assert ("alphas_E" in m) == ecstr
