"""Every device and pinned buffer has one owner that frees it (csrc/common.h DevBuf).

The library counts the bytes its owners hold (`_native.live_bytes()`, mlff_live_bytes); every
assertion here is on a difference of that count, read at the start of the test after
gc.collect() because solvers of other tests may still be alive in the process.  The equalities
are exact: they are conditions (a context returns every byte, replacing a model does not grow),
not measurements.
"""
import gc

import numpy as np
import pytest

from tests import sgdml_shapes as shp
from tests.test_gpu_multirank import run_ranks

pytestmark = pytest.mark.gpu

MIB = 1 << 20


def live():
    from sgdml_amd import _native

    return _native.live_bytes()


@pytest.fixture
def base():
    gc.collect()
    return live()


def rbf_lifecycle(n, rank=0, world=1, key=None):
    """gen_rbf, both storages, the three low-rank builds, a solve and the leverage scores."""
    import sgdml_amd
    from sgdml_amd import synthetic

    X, b = synthetic.rbf_points(n, 3, n)
    idx = np.sort(np.random.default_rng(5).choice(n, 40, replace=False))
    s = sgdml_amd.KernelSolver(n, device=0, rank=rank, world=world, comm_id=key if world > 1 else None)
    try:
        r0, r1 = s.row_range()
        b_loc = np.ascontiguousarray(b[r0:r1])
        s.gen_rbf(X, 0.2)
        s.set_operator(1.0, 0.5)
        s.set_storage("sym")
        s.matvec(b)
        assert s.storage_info()[0] == "sym"
        s.precon_pivchol(40)
        s.pcg(b_loc, tol=1e-8, maxiter=5 * n)
        s.precon_nystrom(idx)
        s.precon_eig(8)
        s.lev_scores(idx, 1e-8)
        s.set_storage("dense")
        s.matvec(b)
        assert s.storage_info()[0] == "dense"
        s.gen_rbf(X, 0.2)
        held = live()
    finally:
        s.close()
    return held


def test_lifecycle_returns_every_byte_one_rank(base):
    """N = 513 is the smallest size with two tiles: the sym path allocates its full set of slot
    and split tables."""
    held = rbf_lifecycle(513)
    assert held > base  # the counter sees the context
    assert live() - base == 0


def test_lifecycle_returns_every_byte_two_ranks(base):
    """Two in-process ranks: the reduce-scatter operands yg / yr, the flat load list and the
    gather buffer of world ranks."""
    run_ranks(2, lambda r, w, key: rbf_lifecycle(1100, r, w, key))
    assert live() - base == 0


@pytest.mark.parametrize("shape", [(9, 17, "c3"), (25, 3, "swap")], ids=shp.case_id)
def test_sgdml_operator_returns_every_byte(base, shape):
    """(9, 17, c3) runs the pair-tile form, (25, 3, swap) the record-factored one; each assembled
    and matrix-free, plain and with energy constraints."""
    import sgdml_amd

    c = shp.case(*shape)
    Rd, Rdd = c.desc
    for E in (False, True):
        N = c.N + (c.M if E else 0)
        x = c.xE[:N]
        with sgdml_amd.KernelSolver(N) as s:
            s.assemble_sgdml(Rd, Rdd, c.perms, shp.SIG, use_E_cstr=E)
            s.set_operator(-1.0, shp.LAM)
            s.matvec(x)
            s.diag()
            s.sgdml_operator(Rd, Rdd, c.perms, shp.SIG, use_E_cstr=E)
            s.set_operator(-1.0, shp.LAM)
            s.matvec(x)
            s.diag()
            if not E:
                s.sgdml_energies(c.x)
            assert live() > base
        assert live() - base == 0, ("use_E_cstr", E)


def test_replacing_a_model_does_not_grow(base):
    import sgdml_amd
    from sgdml_amd import synthetic

    c = shp.case(9, 17, "c3")
    Rd, _ = c.desc
    Rda = np.random.default_rng(2).standard_normal(Rd.shape)
    a_E = np.random.default_rng(3).standard_normal(c.M)
    MP = c.M * c.perms.shape[0]
    R = np.ascontiguousarray(c.R[:3])
    with sgdml_amd.KernelSolver(c.N) as s:
        def model():
            s.predict_set_model(Rd, Rda, c.perms, shp.SIG)
            s.predict(R)
            s.predict_hessian(R)
            return live()

        first = model()
        assert model() == first
        s.predict_set_energy_coefficients(a_E)
        s.predict_hessian(R)
        assert live() - first == 8 * MP  # Et: MP doubles
        s.predict_set_energy_coefficients(None)
        assert live() == first
    assert live() - base == 0

    n = 513
    X, b = synthetic.rbf_points(n, 3, n)
    with sgdml_amd.KernelSolver(n) as s:
        s.gen_rbf(X, 0.2)
        s.set_operator(1.0, 0.5)
        s.matvec(b)  # the storage is resolved (tiles built) before the first reading
        s.precon_pivchol(40)
        once = live()
        s.precon_pivchol(40)
        assert live() == once
        # the residual trace holds maxiter + 1 doubles: it grows once and is kept
        s.pcg(b, tol=1e-8, maxiter=10)
        t10 = live()
        s.pcg(b, tol=1e-8, maxiter=2000)
        t2000 = live()
        assert t2000 - t10 == 8 * (2001 - 11)
        s.pcg(b, tol=1e-8, maxiter=10)
        assert live() == t2000
    assert live() - base == 0


def test_build_scratch_is_returned(base):
    """A build keeps the arena's one standing 64 MiB chunk (api.hip kScratchChunk) and the panel
    buffers of alloc_panel, nothing else.  The panel buffers for k rows of blk = n rounded up to 64
    columns, in doubles: the panel round_up(k, 8) x blk; kVecGrid = 512 partials + k x tsplit,
    tsplit <= 64 (choose_tsplit's cap); zsplit x blk, zsplit <= ceil(k / 16) (choose_zsplit's cap);
    and, the rows being short enough for the one-pass apply, lr_rows_groups(k) x blk with at least
    7 rows per group."""
    import sgdml_amd
    from sgdml_amd import synthetic

    n, k = 513, 40
    X, b = synthetic.rbf_points(n, 3, n)
    idx = np.sort(np.random.default_rng(5).choice(n, k, replace=False))
    with sgdml_amd.KernelSolver(n) as s:
        s.gen_rbf(X, 0.2)
        s.set_operator(1.0, 0.5)
        s.matvec(b)  # the tiles are the operator's, not the build's: built before the reading
        before = live()
        s.precon_nystrom(idx)
        after = live()
        kk = s.precon_info()[1]
        assert kk == k
        blk = -(-n // 64) * 64
        panel = 8 * (-(-kk // 8) * 8 * blk + (512 + 64 * kk) + -(-kk // 16) * blk + -(-kk // 7) * blk)
        print(f"build scratch: held {after - before} bytes, bound {64 * MIB} + {panel}")
        assert 0 < after - before <= 64 * MIB + panel
    assert live() - base == 0
