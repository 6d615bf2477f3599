"""The two forms of the two-role tile mat-vec (k_symv_dyn<true>).

MLFF_SYM_WGS=3: three resident workgroups per CU, one streaming the stored tiles in 4-row half
batches and two generating; MLFF_SYM_WGS=2: two per CU, 8-row batches, one of each role (unset:
three where the operator has enough units per workgroup, which these sizes have not).  Both run the same unit set through the same tile body, and the generated entries are the
stored bits (the select-free exp, tests/test_gpu_rbf_exp_lean.py; no select at all on a plain
tile), so under every role rule either form must give the all-streamed bits (MLFF_SYM_GEN=0):
comparisons are np.array_equal, never a tolerance.  Of the launch only the occupancy and the
grid are asserted; where the workgroups sit is hardware behaviour.
"""
import numpy as np
import pytest

from tests.test_gpu_symtile_generate import LAM, N_MID, OFF, assert_same, points, probe_vectors

pytestmark = pytest.mark.gpu

ENV = ("MLFF_SYM_GEN", "MLFF_SYM_GEN_TILES", "MLFF_SYM_GEN_QUARTERS", "MLFF_SYM_ROLES",
       "MLFF_SYM_STEAL", "MLFF_SYM_WGS")
FORMS = ("2", "3")
ROLES = ("cu", "stream", "gen")
# 15 tiles, all quarters, the last block padded: the generating role's non-plain path only;
# 512 whole tiles (plain ones, diagonal ones and the padded last row block's) + 83 split
SIZES = (2100, N_MID)


def set_env(mp, env):
    for k in ENV:
        mp.delenv(k, raising=False)
    for k, v in env.items():
        mp.setenv(k, v)


def operator_outputs(mp, env, n, vecs):
    """Each vector applied twice (the second application runs on the counters the first one
    left), and the launch the operator reports."""
    import sgdml_amd

    set_env(mp, env)
    X, _ = points(n, 3)
    s = sgdml_amd.KernelSolver(n, device=0)
    try:
        s.gen_rbf(X, length_scale=0.3, jitter=1e-9)
        s.set_operator(1.0, LAM)
        assert s.storage_info()[0] == "sym"
        launch = s.sym_launch_info()
        ys = [s.matvec(v) for v in vecs for _ in range(2)]
    finally:
        s.close()
    return ys, launch


@pytest.fixture(scope="module")
def references():
    """The all-streamed mat-vecs of both sizes: a random vector and two unit vectors each."""
    mp = pytest.MonkeyPatch()
    out = {}
    try:
        for n in SIZES:
            vecs = probe_vectors(n, [0, n - 1])
            ref, _ = operator_outputs(mp, OFF, n, vecs)
            for r in ref:
                r.setflags(write=False)
            out[n] = (vecs, ref)
    finally:
        mp.undo()
    return out


@pytest.mark.parametrize("roles", ROLES)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", SIZES)
def test_forms_matvec(n, form, roles, references, monkeypatch):
    vecs, ref = references[n]
    got, _ = operator_outputs(monkeypatch, {"MLFF_SYM_WGS": form, "MLFF_SYM_ROLES": roles}, n, vecs)
    assert_same(got, ref)


def test_launch_of_each_form(references, monkeypatch):
    """Three resident workgroups per CU and a grid of three times the CUs with the 3-workgroup
    form, two with the other one and without a generating role; one of the two when the library
    chooses."""
    import torch

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    vecs, _ = references[N_MID]
    for env, wgs in (({"MLFF_SYM_WGS": "3"}, 3), ({"MLFF_SYM_WGS": "2"}, 2), (OFF, 2)):
        _, launch = operator_outputs(monkeypatch, env, N_MID, vecs[:1])
        assert launch == (wgs, wgs * cus), (env, launch)
    _, launch = operator_outputs(monkeypatch, {}, N_MID, vecs[:1])
    assert launch in ((2, 2 * cus), (3, 3 * cus)), launch


def pcg_outputs(mp, env):
    import sgdml_amd

    set_env(mp, env)
    n = N_MID
    X, b = points(n, 3, seed=5)
    idx = np.sort(np.random.default_rng(7).choice(n, 64, replace=False))
    s = sgdml_amd.KernelSolver(n, device=0)
    try:
        s.gen_rbf(X, length_scale=0.3, jitter=1e-9)
        s.set_operator(1.0, LAM)
        s.precon_nystrom(idx, variant=0)
        res = s.pcg(b, tol=0.0, maxiter=30)
    finally:
        s.close()
    assert res.iters == 30
    return res.trace, res.x


@pytest.fixture(scope="module")
def pcg_reference():
    mp = pytest.MonkeyPatch()
    try:
        trace, x = pcg_outputs(mp, OFF)
    finally:
        mp.undo()
    trace.setflags(write=False)
    x.setflags(write=False)
    return trace, x


@pytest.mark.parametrize("form", FORMS)
def test_pcg_bitwise(form, pcg_reference, monkeypatch):
    """30 fused-p iterations, rank-64 Nystrom, the default share and role rule: the all-streamed
    trace and iterate, and a second run equal to the first."""
    env = {"MLFF_SYM_WGS": form}
    first = pcg_outputs(monkeypatch, env)
    again = pcg_outputs(monkeypatch, env)
    for a, b in ((pcg_reference, first), (first, again)):
        assert np.array_equal(a[0], b[0])
        assert np.array_equal(a[1], b[1])
