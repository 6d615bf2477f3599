"""Role assignment and unit stealing of the tile mat-vec (k_symv_dyn<true>).

A workgroup's role (streaming or generating) comes from its arrival count on its CU
(MLFF_SYM_ROLES=cu), from the parity of its index (index), or is forced (stream, gen), and a
workgroup whose own range is exhausted goes on with the other role's.  So how many workgroups
hold either role is not known at launch, and every split -- all of them in one role included --
must finish every range and give the all-streamed bits (MLFF_SYM_GEN=0): comparisons are
np.array_equal, never a tolerance.  Where the workgroups sit is hardware behaviour and is not
asserted here (profiles/symroles/ has the traces).
"""
import numpy as np
import pytest

from tests.test_gpu_symtile_generate import (LAM, N_MID, OFF, assert_same, forced, points,
                                             probe_vectors, streamed_bytes, tile_counts)

pytestmark = pytest.mark.gpu

ENV = ("MLFF_SYM_GEN", "MLFF_SYM_GEN_TILES", "MLFF_SYM_GEN_QUARTERS", "MLFF_SYM_ROLES",
       "MLFF_SYM_STEAL")
ROLES = ("cu", "index", "stream", "gen")
N_SMALL = 2100  # 15 tiles, all quarters


def set_env(mp, env):
    for k in ENV:
        mp.delenv(k, raising=False)
    for k, v in env.items():
        mp.setenv(k, v)


def operator_outputs(mp, env, n, vecs):
    """Each vector applied twice (the second application runs on the counters the first one
    left: the work counters reset, the arrival counts not), and the bytes the operator reports."""
    import sgdml_amd

    set_env(mp, env)
    X, _ = points(n, 3)
    s = sgdml_amd.KernelSolver(n, device=0)
    try:
        s.gen_rbf(X, length_scale=0.3, jitter=1e-9)
        s.set_operator(1.0, LAM)
        mode, nbytes = s.storage_info()
        assert mode == "sym"
        ys = [s.matvec(v) for v in vecs for _ in range(2)]
    finally:
        s.close()
    return ys, nbytes


@pytest.fixture(scope="module")
def references():
    """The all-streamed mat-vecs of both sizes: a random vector and two unit vectors each."""
    mp = pytest.MonkeyPatch()
    out = {}
    try:
        for n in (N_SMALL, N_MID):
            vecs = probe_vectors(n, [0, n - 1])
            ref, nbytes = operator_outputs(mp, OFF, n, vecs)
            nt, _ = tile_counts(n)
            assert nbytes == 8.0 * 512 * 512 * nt + 16.0 * n
            for r in ref:
                r.setflags(write=False)
            out[n] = (vecs, ref)
    finally:
        mp.undo()
    return out


@pytest.mark.parametrize("quarters", [0, 1, 2])
@pytest.mark.parametrize("tiles", [0, 256, 512])
@pytest.mark.parametrize("roles", ROLES)
@pytest.mark.parametrize("n", [N_SMALL, N_MID])
def test_roles_matvec(n, roles, tiles, quarters, references, monkeypatch):
    vecs, ref = references[n]
    env = forced(tiles, quarters)
    env["MLFF_SYM_ROLES"] = roles
    got, nbytes = operator_outputs(monkeypatch, env, n, vecs)
    assert_same(got, ref)
    assert nbytes == streamed_bytes(n, env)  # the plan's bytes, whoever took the units


@pytest.mark.parametrize("steal", ["other", "pool"])
def test_steal_order(steal, references, monkeypatch):
    """Both orders in which a finished workgroup turns to the remaining ranges."""
    vecs, ref = references[N_MID]
    for roles in ("cu", "gen"):
        env = dict(forced(256, 0), MLFF_SYM_ROLES=roles, MLFF_SYM_STEAL=steal)
        got, _ = operator_outputs(monkeypatch, env, N_MID, vecs)
        assert_same(got, ref)


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


@pytest.mark.parametrize("roles", ["cu", "stream", "gen"])
def test_pcg_bitwise(roles, pcg_reference, monkeypatch):
    """30 fused-p iterations, rank-64 Nystrom, the default share: the all-streamed trace and
    iterate, and a second run equal to the first."""
    env = {"MLFF_SYM_ROLES": roles}
    first = pcg_outputs(monkeypatch, env)
    again = pcg_outputs(monkeypatch, env)
    for a, b in ((pcg_reference, first), (first, again)):
        assert np.array_equal(a[0], b[0])
        assert np.array_equal(a[1], b[1])


def test_sharded_bitwise(monkeypatch):
    """3 ranks in one process (about 392 tiles each, all quarters, all the generating role's):
    with every workgroup streaming the quarter range is finished by stealing alone, and the list
    reduction's counter reset serves that as well."""
    from tests.test_gpu_multirank import run_ranks
    from tests.test_gpu_symtile_generate import sharded_case

    n = 3 * 8192
    out = {}
    for name, env in (("off", OFF),
                      ("stream", dict(forced(quarters=2), MLFF_SYM_ROLES="stream")),
                      ("gen", dict(forced(quarters=2), MLFF_SYM_ROLES="gen"))):
        set_env(monkeypatch, env)
        out[name] = run_ranks(3, lambda r, w, key: sharded_case(r, w, key, n))
    for name in ("stream", "gen"):
        for a, b in zip(out["off"], out[name]):
            assert len(a[0]) == 11
            assert np.array_equal(a[0], b[0])
            assert np.array_equal(a[1], b[1])
            assert b[2] < a[2]
