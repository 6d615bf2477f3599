"""The oracle's long-double evaluation (oracle/sgdml.py, dtype=np.longdouble): the
high-precision reference of tests/test_gpu_sgdml_shapes.py.  CPU only."""
import numpy as np
import pytest

from oracle import sgdml as osg
from tests import sgdml_shapes as sh

LD = np.longdouble
SMALL = [(3, 4, "nongroup"), (9, 1, "c3")]


def test_longdouble_is_extended_precision():
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63


def _calls(c):
    Rd, Rdd = c.desc
    g = c.N - 2
    return {
        "descriptors_0": lambda **k: osg.descriptors(c.R, **k)[0],
        "descriptors_1": lambda **k: osg.descriptors(c.R, **k)[1],
        "assemble_kernel": lambda **k: osg.assemble_kernel(Rd, Rdd, c.tpl, sh.SIG, **k),
        "assemble_kernel_E": lambda **k: osg.assemble_kernel(Rd, Rdd, c.tpl, sh.SIG,
                                                             use_E_cstr=True, **k),
        "kernel_matvec_matrix_free": lambda **k: osg.kernel_matvec_matrix_free(
            Rd, Rdd, c.perms, sh.SIG, c.x, **k),
        "kernel_matvec_matrix_free_E": lambda **k: osg.kernel_matvec_matrix_free(
            Rd, Rdd, c.perms, sh.SIG, c.xE, use_E_cstr=True, **k),
        "kernel_matvec_factored": lambda **k: osg.kernel_matvec_factored(
            Rd, Rdd, c.perms, sh.SIG, c.x, **k),
        "pair_records_U": lambda **k: osg.pair_records(Rd, Rdd, c.perms, sh.SIG, **k)[0],
        "pair_records_w": lambda **k: osg.pair_records(Rd, Rdd, c.perms, sh.SIG, **k)[3],
        "kernel_column_matrix_free": lambda **k: osg.kernel_column_matrix_free(
            Rd, Rdd, c.perms, sh.SIG, g, **k),
        "kernel_diag": lambda **k: osg.kernel_diag(Rd, Rdd, c.perms, sh.SIG, **k),
        "kernel_diag_E": lambda **k: osg.kernel_diag(Rd, Rdd, c.perms, sh.SIG, use_E_cstr=True, **k),
        "kernel_diag_identity": lambda **k: osg.kernel_diag(Rd, Rdd, np.arange(c.n)[None], sh.SIG, **k),
        "energies_matrix_free": lambda **k: osg.energies_matrix_free(
            Rd, Rdd, c.perms, sh.SIG, c.x, **k),
    }


@pytest.mark.parametrize("key", SMALL, ids=sh.case_id)
def test_longdouble_type_and_agreement(key):
    c = sh.case(*key)
    for name, f in _calls(c).items():
        v64, vld = f(), f(dtype=LD)
        assert v64.dtype == np.float64, name
        assert vld.dtype == LD, name
        assert vld.shape == v64.shape, name
        d = float(np.max(np.abs(vld - v64)) / np.max(np.abs(vld)))
        print(f"{c.label} {name}: float64 vs long double {d:.2e} of the largest entry")
        assert d <= 1e-13, (name, d)
        # more than a cast of the float64 result: some entry carries bits below float64's
        if name != "kernel_diag_identity" or c.n > 2:
            assert np.any(vld != vld.astype(np.float64)), name


def test_default_dtype_is_float64(golden_dir):
    """The default is the float64 evaluation (same bits as dtype=np.float64 passed explicitly),
    within the reference fixture's 1e-13 as tests/test_oracle_golden.py pins it."""
    from tests.conftest import load_golden

    f = load_golden(golden_dir, "sgdml_ethanol_n270_perms")
    Rd, Rdd = f["R_desc"][:3], f["R_d_desc"][:3]
    tpl = osg.tril_perms_lin(f["perms"])
    a = osg.assemble_kernel(Rd, Rdd, tpl, float(f["sig"]))
    b = osg.assemble_kernel(Rd, Rdd, tpl, float(f["sig"]), dtype=np.float64)
    assert np.array_equal(a, b)
    assert np.max(np.abs(a - f["K"][:81, :81])) <= 1e-13 * np.max(np.abs(a))


def test_molecule_and_perm_sets():
    for n, M, kinds in sh.TABLE:
        R = sh.molecule(n, M, sh.SEEDS.get((n, M), 1000 * n + M))
        assert R.shape == (M, n, 3)
        a, b = np.tril_indices(n, k=-1)
        assert np.min(np.linalg.norm(R[:, a] - R[:, b], axis=2)) >= sh.MIN_DIST
        assert np.array_equal(R, sh.molecule(n, M, sh.SEEDS.get((n, M), 1000 * n + M)))
        for kind in kinds:
            p = sh.perm_set(n, kind)
            assert np.array_equal(np.sort(p, axis=1), np.broadcast_to(np.arange(n), p.shape))
            closed = {tuple(x[y]) for x in p for y in p} == {tuple(x) for x in p}
            assert closed == (kind != "nongroup")
    with pytest.raises(ValueError):
        sh.perm_set(2, "swap")


@pytest.mark.parametrize("key", [k for k in sh.CASES if k[0] <= 25], ids=sh.case_id)
def test_sweep_pivots_separated(key):
    """The seeds of the sweep (1000 n + M, sgdml_shapes.SEEDS): the first k pivots of the
    reference's pivoted Cholesky are separated by more than 1e-9 (relative) from the runner-up,
    so that test_columns may ask for the same pivots."""
    c = sh.case(*key)
    _, piv, band, gap = c.pivchol
    print(f"{c.label}: seed {c.seed} k {c.k_piv} smallest gap {gap:.3e} panel band {band:.2e}")
    assert gap > sh.PIVOT_GAP
