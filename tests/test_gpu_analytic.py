"""Closed-form ('analytic') sGDML training on the GPU: the two-level blocked Cholesky
(mlff_test_potrf), the dense solve (mlff_dense_cho_solve) and the training entry points
against the reference's GDMLTrain.train(solver 'analytic') models
(tests/golden/sgdml_analytic_cases.npz, make_analytic_golden.py).

Criteria.  Factorisation: |A - L L^T| <= gamma_{n+1} |L| |L|^T entrywise, gamma_k = k u /
(1 - k u), u = 2^-53 (Higham, Accuracy and Stability of Numerical Algorithms, Theorem 10.3; it
holds for any order of the sums, and fused multiply-adds only lower it), the upper triangle
exactly zero.  Solve: ||A x - b||_2 <= n gamma_{3n+1} ||A||_2 ||x||_2 (Theorem 10.4 with
|| |L| |L^T| ||_2 <= n ||A||_2).  Both residuals are formed in extended precision (x87 long
double, 2^-64), so that the check's own rounding stays 2^-11 of the bound.  End to end:
ten times the reference's own spread over four variants of its run (the bands of the fixture).
"""
import os
import subprocess
import sys
from datetime import datetime
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
SIZES = [1, 63, 64, 65, 255, 256, 257, 300, 621, 777]
SGDML = ["sgdml_ethanol_n270", "sgdml_ethanol_n270_perms", "sgdml_ethanol_n621",
         "sgdml_ethanol_n270_ecstr", "sgdml_ethanol_n270_perms_ecstr"]
REPO = Path(__file__).resolve().parent.parent


def gamma(k):
    return k * U / (1.0 - k * U)


def spd(n, seed=0):
    """Seeded B B^T + I, exactly symmetric."""
    B = np.random.default_rng(1000 * seed + n).standard_normal((n, n))
    A = B @ B.T + np.eye(n)
    return np.tril(A) + np.tril(A, -1).T


def check_factor(A, L):
    n = A.shape[0]
    assert np.array_equal(np.triu(L, 1), np.zeros_like(L)), "upper triangle not zero"
    Lx = L.astype(np.longdouble)
    resid = np.abs(A.astype(np.longdouble) - Lx @ Lx.T)
    bound = gamma(n + 1) * (np.abs(Lx) @ np.abs(Lx).T)
    ratio = float(np.max(resid / bound))
    print(f"n={n}: max |A - L L^T| / (gamma_(n+1) |L||L|^T) = {ratio:.3e}")
    assert np.all(resid <= bound), ratio


def solve_eta(A, x, b):
    """(||A x - b||_2, ||A||_2 ||x||_2), the residual in extended precision."""
    r = A.astype(np.longdouble) @ x.astype(np.longdouble) - b.astype(np.longdouble)
    return float(np.linalg.norm(r.astype(np.float64))), np.linalg.norm(A, 2) * np.linalg.norm(x)


def check_solve(A, x, b, label):
    n = A.shape[0]
    r, scale = solve_eta(A, x, b)
    print(f"{label} n={n}: eta = ||A x - b|| / (||A|| ||x||) = {r / scale:.3e}, "
          f"bound n gamma_(3n+1) = {n * gamma(3 * n + 1):.3e}")
    assert r <= n * gamma(3 * n + 1) * scale
    return r / scale


@pytest.fixture(scope="module")
def solver_of():
    """One context per size for the whole module."""
    import sgdml_amd

    made = {}

    def get(n):
        if n not in made:
            made[n] = sgdml_amd.KernelSolver(n, device=0)
        return made[n]

    yield get
    for s in made.values():
        s.close()


# ------------------------------------------------------------------ factorisation
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_potrf(solver_of, n, variant):
    A = spd(n)
    check_factor(A, solver_of(n).test_potrf(A, variant=variant))


def test_potrf_not_positive_definite(solver_of):
    A = spd(300)
    A[170, 170] = -1.0
    for variant in (0, 1):
        with pytest.raises(np.linalg.LinAlgError):
            solver_of(300).test_potrf(A, variant=variant)


CHILD = """
import sys
import numpy as np
sys.path[:0] = [{repo!r}, {pkg!r}]
import sgdml_amd
from tests.test_gpu_analytic import spd
out = {{}}
for n in (257, 621):
    with sgdml_amd.KernelSolver(n, device=0) as s:
        for v in (0, 1):
            out[f"L{{v}}_{{n}}"] = s.test_potrf(spd(n), variant=v)
np.savez(sys.argv[1], **out)
"""


def factors_with_outer(outer, tmp_path):
    """Variants 0 and 1 at n = 257, 621 from a fresh process with MLFF_POTRF_OUTER set (the
    knob is read once per process)."""
    path = tmp_path / f"outer{outer}.npz"
    env = dict(os.environ, MLFF_POTRF_OUTER=str(outer))
    code = CHILD.format(repo=str(REPO), pkg=str(REPO / "mlff-preconditioner_amd"))
    res = subprocess.run([sys.executable, "-c", code, str(path)], env=env, capture_output=True,
                         text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    return np.load(path)


def test_potrf_outer_128(solver_of, tmp_path):
    f = factors_with_outer(128, tmp_path)
    for n in (257, 621):
        check_factor(spd(n), f[f"L1_{n}"])
    # the knob was read: another trailing depth groups the sums of the last panels otherwise
    assert not np.array_equal(f["L1_621"], solver_of(621).test_potrf(spd(621), variant=1))


def test_potrf_outer_64_is_the_one_level_order(tmp_path):
    f = factors_with_outer(64, tmp_path)
    for n in (257, 621):
        assert np.array_equal(f[f"L1_{n}"], f[f"L0_{n}"])


# ------------------------------------------------------------------ solve, host matrices
@pytest.mark.parametrize("n", SIZES)
def test_solve_host_matrix(solver_of, n):
    A = spd(n, seed=1)
    b = np.random.default_rng(n).standard_normal(n)
    s = solver_of(n)
    s.set_matrix(A)
    s.set_operator(1.0, 1e-3)
    v = np.random.default_rng(n + 1).standard_normal(n)
    rows0, y0 = s.get_matrix_rows(), s.matvec(v)
    x, sec = s.dense_cho_solve(b, sigma_K=1.0, shift=0.0, want_seconds=True)
    check_solve(A, x, b, "host")
    assert sec.shape == (3,) and np.all(sec >= 0) and sec[1] > 0
    # K and the operator are as before
    assert np.array_equal(s.get_matrix_rows(), rows0) and np.array_equal(rows0, A)
    assert np.array_equal(s.matvec(v), y0)


def test_solve_shift_and_sign(solver_of):
    n = 300
    A = spd(n, seed=2)
    b = np.random.default_rng(5).standard_normal(n)
    s = solver_of(n)
    s.set_matrix(-A)
    x = s.dense_cho_solve(b, sigma_K=-1.0, shift=0.5)
    check_solve(A + 0.5 * np.eye(n), x, b, "shifted")


def test_solve_not_positive_definite(solver_of):
    n = 65
    s = solver_of(n)
    s.set_matrix(-np.eye(n))
    with pytest.raises(np.linalg.LinAlgError):
        s.dense_cho_solve(np.ones(n), sigma_K=1.0, shift=0.0)
    x = s.dense_cho_solve(np.ones(n), sigma_K=-1.0, shift=0.0)  # the context still works
    assert np.array_equal(x, np.ones(n))


# ------------------------------------------------------------------ solve, sGDML systems
@pytest.mark.parametrize("name", SGDML)
def test_solve_sgdml(golden_dir, name):
    import scipy.linalg

    import sgdml_amd

    f = np.load(golden_dir / f"{name}.npz", allow_pickle=False)
    y = f["y"]
    n = y.size
    with sgdml_amd.KernelSolver(n, device=0) as s:
        s.assemble_sgdml(f["R_desc"], f["R_d_desc"], f["perms"], float(f["sig"]),
                         use_E_cstr=name.endswith("ecstr"))
        x = s.dense_cho_solve(y)  # the reference's call: sigma_K = -1, shift = 1e-10
        K = s.get_matrix_rows()
    A = -K
    A[np.diag_indices(n)] += 1e-10
    eta = check_solve(A, x, y, name)
    x_ref = scipy.linalg.cho_solve(scipy.linalg.cho_factor(A, lower=True), y)
    r, scale = solve_eta(A, x_ref, y)
    print(f"{name}: eta device {eta:.3e}, eta scipy cho_solve {r / scale:.3e}")


# ------------------------------------------------------------------ state
def test_matrix_free_only_is_a_state_error(golden_dir):
    import sgdml_amd

    f = np.load(golden_dir / "sgdml_ethanol_n270.npz", allow_pickle=False)
    with sgdml_amd.KernelSolver(270, device=0) as s:
        s.sgdml_operator(f["R_desc"], f["R_d_desc"], f["perms"], 10.0)
        with pytest.raises(RuntimeError, match=r"error -5"):
            s.dense_cho_solve(f["y"])


# ------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def cases(golden_dir):
    return np.load(golden_dir / "sgdml_analytic_cases.npz", allow_pickle=False)


def task_of(f, case):
    from tests.test_analytic_format import task_of as make

    g = lambda k: f[f"{case}__{k}"]  # noqa: E731
    return make(g("R"), g("F"), g("E"), g("z"), g("perms"), "analytic",
                use_E_cstr=bool(g("use_E_cstr")), lam=float(g("lam")))


@pytest.fixture(scope="module")
def trained(cases):
    """Every case trained once."""
    from sgdml_amd import model as mdl

    return {c: mdl.train(task_of(cases, c)) for c in cases["cases"]}


@pytest.mark.parametrize("case", ["eth", "ethp"])
def test_train_analytic_predicts_as_the_reference(cases, trained, case):
    import sgdml_amd

    g = lambda k: cases[f"{case}__{k}"]  # noqa: E731
    m = trained[case]
    assert sorted(m) == list(g("model_keys"))
    assert m["solver_name"] == "analytic" and m["use_E"] and "alphas_E" not in m
    assert m["lam"] == float(g("lam")) and m["std"] == float(g("std"))
    with sgdml_amd.GDMLPredict(m, device=0) as gd:
        E, F = gd.predict(g("Rq"))
    E_ref, F_ref, c_ref = g("Eq"), g("Fq"), float(g("c"))
    dF = np.max(np.abs(F - F_ref)) / np.max(np.abs(F_ref))
    dE = np.max(np.abs(E - E_ref)) / np.max(np.abs(E_ref - c_ref))
    dc = abs(m["c"] - c_ref) / abs(c_ref)
    da = np.linalg.norm(m["alphas_F"] - g("alphas_F")) / np.linalg.norm(g("alphas_F"))
    print(f"{case}: dF {dF:.3e} (band {float(g('band_F')):.3e}), dE {dE:.3e} (band "
          f"{float(g('band_E')):.3e}), dc {dc:.3e} (band {float(g('band_c')):.3e}), dalpha "
          f"{da:.3e} (band {float(g('band_rel_dalpha')):.3e})")
    assert dF <= 10 * float(g("band_F"))
    assert dE <= 10 * float(g("band_E"))
    assert dc <= 10 * float(g("band_c"))


@pytest.mark.parametrize("case", ["eth_ecstr", "ethp_ecstr"])
def test_train_analytic_energy_constraints(cases, trained, case):
    import sgdml_amd
    from sgdml_amd import model as mdl
    from sgdml_amd.solver import host_descriptors

    g = lambda k: cases[f"{case}__{k}"]  # noqa: E731
    m = trained[case]
    assert sorted(m) == list(g("model_keys"))
    assert m["solver_name"] == "analytic" and m["use_E"]
    assert m["c"] == np.mean(g("E")) and m["std"] == float(g("std"))
    M = g("R").shape[0]
    assert m["alphas_E"].shape == (M,) and m["alphas_F"].shape == (27 * M,)
    a = np.concatenate([m["alphas_F"], m["alphas_E"]])
    a_ref = np.concatenate([g("alphas_F"), g("alphas_E")])
    da = np.linalg.norm(a - a_ref) / np.linalg.norm(a_ref)
    print(f"{case}: dalpha {da:.3e} (band {float(g('band_rel_dalpha')):.3e})")
    assert da <= 10 * float(g("band_rel_dalpha"))
    # the residual of the (N + M) system the coefficients solve: (-K + 1e-10 I) (-alphas) = y
    task = task_of(cases, case)
    y, _, _ = mdl.label_vector(task)
    Rd, Rdd = host_descriptors(g("R"))
    with sgdml_amd.KernelSolver(y.size, device=0) as s:
        s.assemble_sgdml(Rd, Rdd, g("perms"), 10.0, use_E_cstr=True)
        K = s.get_matrix_rows()
    A = -K
    A[np.diag_indices(y.size)] += 1e-10
    check_solve(A, -a, y, case)


# ------------------------------------------------------------------ entry points
def test_analytic_solver_class_equals_train(cases, trained):
    from sgdml_amd import model as mdl
    from sgdml_amd.solver import host_descriptors
    from sgdml_amd.solvers import Analytic

    for case in ("ethp", "ethp_ecstr"):
        task = task_of(cases, case)
        Rd, Rdd = host_descriptors(task["R_train"])
        y, _, _ = mdl.label_vector(task)
        msgs = []
        with Analytic(None, None, callback=lambda *a, **k: msgs.append(k.get("disp_str"))) as an:
            alphas = an.solve(task, Rd, Rdd, mdl.tril_perms_lin(task["perms"]), y)
        m = trained[case]
        both = np.concatenate([m["alphas_F"], m.get("alphas_E", np.zeros(0))])
        assert np.array_equal(alphas, both)
        for want in ("Assembling kernel matrix", "Solving linear system (Cholesky factorization)",
                     "Training on 23 points"):
            assert want in msgs, msgs
    with pytest.raises(NotImplementedError):
        Analytic(None, None).solve(dict(task, cprsn_keep_atoms_idxs=np.arange(3)), Rd, Rdd,
                                   mdl.tril_perms_lin(task["perms"]), y)


def test_train_model_stores_under_analytic(cases, tmp_path):
    from sgdml_amd import model as mdl

    m = mdl.train_model(dict(task_of(cases, "eth"), solver_name="cg"), "ethanol", 23, "cholesky",
                        solver="analytic")
    assert m["solver_name"] == "analytic" and m["kernel_size"] == 621 and m["use_E"]
    out = mdl.store_model(m, tmp_path, now=datetime(2024, 1, 2, 3, 4))
    assert out == tmp_path / "data_new/models/mi355x/ethanol/analytic/n=23/2024-01-02_0304.npz"
    back = np.load(out, allow_pickle=True)
    np.testing.assert_array_equal(back["alphas_F"], m["alphas_F"])
