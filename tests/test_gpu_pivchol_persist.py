"""The persistent pivoted Cholesky (k_piv_persist, csrc/kernels_pivchol.hip; round 6) against the
launch sequence it replaces (MLFF_PIVCHOL_PERSIST=0: finaliser, column, split-K Schur GEMV and
finisher per step).  Both restate incomplete_cholesky.py:24-93 with the same operations in the
same order, so the pivot sequence, the factor L and everything built from it are bit-identical.

* the sGDML single-column path (the configs[1] / configs[4] geometry, matrix-free operator) and
  the dense rows (a host matrix), both through the speculative blocks (hits and misses);
* configs[1] at its full size (N = 15540, k = 2701), with the build times of both forms;
* a workgroup that stops publishing (test hook MLFF_PIV_MUTE): every workgroup times out, the
  build falls back to the launch sequence and still returns the same factor.
"""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIG, LAM = 10.0, 1e-10


@pytest.fixture(scope="module")
def sg():
    import sgdml_amd

    if sgdml_amd.device_count() < 1:
        pytest.fail("no GPU visible to libmlffpcg.so")
    return sgdml_amd


def _nanotube(sg, M):
    from sgdml_amd import synthetic

    ds = synthetic.nanotube_like(M, seed=0)
    Rd, Rdd = sg.sgdml_descriptors(ds["R"])
    y, _ = synthetic.labels(ds["F"])
    return Rd, Rdd, np.arange(370)[None, :], y


def _build(sg, monkeypatch, persist, setup, n, k, woodbury=False):
    monkeypatch.setenv("MLFF_PIVCHOL_PERSIST", "1" if persist else "0")
    with sg.KernelSolver(n) as s:
        setup(s)
        t0 = time.perf_counter()
        piv, sec = s.precon_pivchol(k, build_woodbury=woodbury)
        wall = time.perf_counter() - t0
        Lt = s.precon_panel()
        cols, _ = s.pivchol_times(k)
    return piv, Lt, sec, wall, cols


def _compare(a, b, k):
    np.testing.assert_array_equal(a[0], b[0])          # the whole permutation
    np.testing.assert_array_equal(a[1][:k], b[1][:k])  # L, bit for bit


@pytest.mark.timeout(300)
@pytest.mark.parametrize("M,k", [(3, 150), (4, 700)])
def test_persistent_matches_launch_sequence_sgdml(sg, monkeypatch, M, k):
    Rd, Rdd, perms, y = _nanotube(sg, M)
    n = y.size

    def setup(s):
        s.sgdml_operator(Rd, Rdd, perms, SIG)
        s.set_operator(-1.0, LAM)

    a = _build(sg, monkeypatch, True, setup, n, k)
    b = _build(sg, monkeypatch, False, setup, n, k)
    print(f"M={M} N={n} k={k}: persistent {a[2]:.4f} s, launch sequence {b[2]:.4f} s")
    _compare(a, b, k)
    assert np.all(a[4] > 0) and abs(a[4].sum() - a[2]) <= 0.5 * a[2] + 1e-3


@pytest.mark.timeout(300)
@pytest.mark.parametrize("n,k", [(1000, 40), (3000, 400)])
def test_persistent_matches_launch_sequence_dense(sg, monkeypatch, n, k):
    rng = np.random.default_rng(3)
    X = rng.uniform(size=(n, 3))
    d2 = ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)
    K = np.exp(-d2 / (2 * 0.3 ** 2)) + 1e-6 * np.eye(n)

    def setup(s):
        s.set_matrix(K)
        s.set_operator(1.0, 1e-6)

    a = _build(sg, monkeypatch, True, setup, n, k)
    b = _build(sg, monkeypatch, False, setup, n, k)
    _compare(a, b, k)
    # and the factor is the oracle's (incomplete_cholesky.py:24-93 restated)
    from oracle.precon import pivoted_cholesky

    kk = 10  # (random points: later candidates can tie to rounding)
    L_ref, piv_ref = pivoted_cholesky(lambda i: K[:, i].copy(), np.diag(K).copy(), kk)
    np.testing.assert_array_equal(a[0][:kk], piv_ref[:kk])
    np.testing.assert_allclose(a[1][:kk].T[:n], L_ref, rtol=0, atol=1e-10)


@pytest.fixture(scope="module")
def dense513():
    n = 513  # the smallest size with speculation: nrows > kSpecGroups * kSpecPer = 512
    X = np.random.default_rng(3).uniform(size=(n, 3))
    d2 = ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)
    K = np.exp(-d2 / (2 * 0.3 ** 2)) + 1e-6 * np.eye(n)
    K.setflags(write=False)
    return K


@pytest.mark.parametrize("k", [80, 81, 96, 97])
def test_block_loop_edges_dense(sg, monkeypatch, dense513, k):
    """The block loop both forms share (piv_spec_block and its callers), at the panel sizes where
    the blocks' ends move: speculation needs k > kSpecMin + kSpecB = 80, so k = 80 has no block;
    81 one full block [64, 80) and a one-step block; 96 blocks that end exactly at k; 97 a
    one-step tail again.  The two forms agree bit for bit and both report every column's time."""
    K = dense513
    n = K.shape[0]

    def setup(s):
        s.set_matrix(K)
        s.set_operator(1.0, 1e-6)

    a = _build(sg, monkeypatch, True, setup, n, k)
    b = _build(sg, monkeypatch, False, setup, n, k)
    _compare(a, b, k)
    assert a[4].shape == (k,) and np.all(a[4] > 0)
    assert b[4].shape == (k,) and np.all(b[4] > 0)
    from oracle.precon import pivoted_cholesky

    kk = 10  # (random points: later candidates can tie to rounding)
    L_ref, piv_ref = pivoted_cholesky(lambda i: K[:, i].copy(), np.diag(K).copy(), kk)
    np.testing.assert_array_equal(a[0][:kk], piv_ref[:kk])
    np.testing.assert_allclose(a[1][:kk].T[:n], L_ref, rtol=0, atol=1e-10)


@pytest.mark.timeout(600)
def test_persistent_configs1_full_size(sg, monkeypatch):
    """configs[1]: N = 15540, the rule-of-thumb k = 2701 -- the factor bit-identical to the launch
    sequence's, the build faster."""
    Rd, Rdd, perms, y = _nanotube(sg, 14)
    n, k = y.size, 2701

    def setup(s):
        s.sgdml_operator(Rd, Rdd, perms, SIG)
        s.set_operator(-1.0, LAM)

    _build(sg, monkeypatch, True, setup, n, 200)   # warm-up (module load, allocations)
    a = _build(sg, monkeypatch, True, setup, n, k)
    b = _build(sg, monkeypatch, False, setup, n, k)
    print(f"configs[1] k={k}: pivoted Cholesky persistent {a[2]:.4f} s (wall {a[3]:.4f}), "
          f"launch sequence {b[2]:.4f} s (wall {b[3]:.4f})")
    _compare(a, b, k)
    assert a[2] < b[2]


@pytest.mark.timeout(300)
def test_persistent_timeout_falls_back(sg, monkeypatch):
    """A workgroup that never publishes (MLFF_PIV_MUTE): the others give up after ~1 s, the
    build restarts with the launch sequence, the factor is the same."""
    Rd, Rdd, perms, y = _nanotube(sg, 3)
    n, k = y.size, 150

    def setup(s):
        s.sgdml_operator(Rd, Rdd, perms, SIG)
        s.set_operator(-1.0, LAM)

    b = _build(sg, monkeypatch, False, setup, n, k)
    monkeypatch.setenv("MLFF_PIV_MUTE", "5")
    a = _build(sg, monkeypatch, True, setup, n, k)
    monkeypatch.delenv("MLFF_PIV_MUTE")
    assert a[3] >= 0.9, a[3]  # it did wait for the muted workgroup
    _compare(a, b, k)
