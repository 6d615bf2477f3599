"""The PCG oracle in long double (oracle/pcg.py, dtype = np.longdouble) and every condition that
tests/pcg_shapes.py sets on its cases: the bands and the residual floor of Table A, the 5 % margins
of the stop decisions of Table B in long double and in both float64 orders, and the agreement of
the three evaluations on every decision (B6 / B7: of the two float64 ones, see there).  CPU only.
"""
import numpy as np
import pytest

from oracle.pcg import cg_legacy
from tests import pcg_shapes as pc
from tests.conftest import load_golden
from tests.pcg_shapes import LD, MARGIN

F64 = np.float64


def test_default_arguments_keep_the_bits(golden_dir):
    """dtype = float64 and a record dict change no bit of a golden solve; the record's last
    iterate is the returned x."""
    f = load_golden(golden_dir, "sgdml_ethanol_n270")
    K, y, lam = f["K"], f["y"], float(f["lam"])
    ref = f["dense_none__trace"]
    rec = {}
    for kw in ({}, {"dtype": F64, "record": rec}):
        x, info, tr, it = cg_legacy(lambda v: -(K @ v) + lam * v, y, tol=1e-4, maxiter=len(ref), **kw)
        assert info == int(f["dense_none__info"]) and x.dtype == tr.dtype == F64
        np.testing.assert_array_equal(tr[1:], ref)
        np.testing.assert_array_equal(x, f["dense_none__x"])
    assert len(rec["x"]) == it + 1 and np.array_equal(rec["x"][-1], x)
    assert not np.any(rec["x"][0])


def test_long_double_stays_long_double():
    s = pc.system(("spd", 65), 9, pc.HOST_LAM)
    seen = []

    def matvec(v):
        seen.append(v.dtype)
        return s.operators(LD)[0](v)

    rec = {}
    x, info, tr, it = cg_legacy(matvec, s.b, tol=1e-12, psolve=s.operators(LD)[1], dtype=LD, record=rec)
    assert info == 0 and x.dtype == tr.dtype == LD and all(d == LD for d in seen)
    assert all(v.dtype == LD for v in rec["x"]) and len(rec["x"]) == it + 1
    # the last stop test is the true residual, below anything float64 reaches
    it_c, rec_r, true_r, passed = rec["recheck"][-1]
    assert it_c == it and passed and tr[-1] == true_r
    r = s.residual_ld(x)
    assert abs(np.sqrt(r @ r) - true_r) <= 1e-15 * true_r + 1e-19 * np.sqrt(s.b @ s.b)


# ---------------------------------------------------------------- Table A
def _a_rows():
    rows = [(inp, k, lam, J) for inp, k, lam, J in pc.TABLE_A]
    for case, k, J0, Jk, *_ in pc.SGDML_A:
        rows += [(("sgdml",) + case, 0, None, J0), (("sgdml",) + case, k, None, Jk)]
    case, k, J0, Jk = pc.ECSTR_A
    rows += [(("sgdmlE",) + case, 0, None, J0), (("sgdmlE",) + case, k, None, Jk)]
    return rows


A_ROWS = _a_rows()


@pytest.mark.parametrize("inp,k,lam,J", A_ROWS, ids=[f"{pc.sys_id(i, k)}-J{J}" for i, k, _, J in A_ROWS])
def test_table_a_conditions(inp, k, lam, J):
    s = pc.system(inp, k, lam)
    ref, evals = s.smooth(J)
    bx, bt = s.smooth_bands(J)
    floor = float(ref.trace[J] / ref.trace[0])
    print(f"pcg-sweep {s.label} J={J} lam={s.lam:g}: band x={bx:.2e} trace={bt:.2e} "
          f"trace[J]/trace[0]={floor:.2e}")
    assert J >= 1 and (J <= s.N - 1 or s.N == 1)
    if s.N == 1:
        # x_1 = b / a; whether r_1 is exactly zero (info 0) is a rounding matter with a
        # preconditioner (alpha q != b in float64): decided per case by converges_at_1
        assert ref.iters == 1 and bx <= pc.BAND_X
        assert pc.converges_at_1(s) == (k == 0)
        return
    for r in [ref] + evals:
        assert r.iters == r.info == J and r.trace.size == J + 1 and len(r.xs) == J + 1
    assert bx <= pc.BAND_X
    assert bt <= pc.BAND_TRACE
    assert floor >= pc.TRACE_FLOOR


@pytest.mark.parametrize("case", [c for c, *_ in pc.SGDML_A], ids=[str(c) for c, *_ in pc.SGDML_A])
def test_sgdml_condition_number(case):
    s = pc.sgdml_system(case, 0)
    w = np.linalg.eigvalsh(s.p.S64)
    cond = (w[-1] + s.lam) / (w[0] + s.lam)
    print(f"pcg-sweep {s.label}: lam={s.lam:g} cond(A)={cond:.2f}")
    assert w[0] > -1e-10 * w[-1] and cond <= pc.SGDML_COND


# ---------------------------------------------------------------- Table B
def _three(s, **kw):
    return [s.solve(LD, **kw), s.solve(F64, **kw), s.solve(F64, True, **kw)]


B_NAMES = list(pc.B_SYSTEMS)


@pytest.mark.parametrize("name", B_NAMES)
def test_b1_legacy_early_exit(name):
    s, _ = pc.b_system(name)
    x0 = np.linalg.solve(s.A_ld().astype(F64), s.b)
    for r in _three(s, x0=x0, tol=1e-6):
        assert r.iters == 0 and r.info == 0 and r.callbacks == 0 and r.trace.size == 1
        assert r.trace[0] <= (1 - MARGIN) * 1e-6
        assert np.array_equal(r.x.astype(F64), x0)
    for tol in (0.0, 1e-8):
        for r in _three(s, b=np.zeros(s.N), tol=tol):
            assert r.iters == 0 and r.info == 0 and r.callbacks == 0 and not np.any(r.x)


@pytest.mark.parametrize("name", B_NAMES)
def test_b2_small_r0_without_early_exit(name):
    s, _ = pc.b_system(name)
    b, x0, tol = pc.b2_inputs(s)
    bn = float(np.linalg.norm(b))
    assert abs(bn - 100) <= 1e-12
    for r in _three(s, b=b, x0=x0, tol=tol):
        assert r.iters == 0 and r.info == 0 and r.callbacks == 1 and r.trace.size == 1
        assert r.trace[0] >= (1 + MARGIN) * tol and r.trace[0] <= (1 - MARGIN) * tol * bn
        assert np.array_equal(r.x.astype(F64), x0)


@pytest.mark.parametrize("name", B_NAMES)
def test_b3_converges_at_iteration_1(name):
    s, _ = pc.b_system(name)
    b, tol = pc.b3_inputs(s)
    for r in _three(s, b=b, tol=tol):
        atol = tol * float(np.linalg.norm(b))
        assert r.iters == 1 and r.info == 0 and r.callbacks == 1 and not r.recheck
        assert r.trace[0] >= (1 + MARGIN) * atol and r.trace[1] <= 1e-3 * atol


def _assert_margins(trace, m, atol, tag):
    assert np.all(trace[:m] >= (1 + MARGIN) * atol), (tag, [float(t / atol) for t in trace[:m]])
    assert trace[m] <= (1 - MARGIN) * atol, (tag, float(trace[m] / atol))


@pytest.mark.parametrize("name", B_NAMES)
def test_b4_b5_convergence_and_maxiter(name):
    s, m = pc.b_system(name)
    assert 6 <= m <= 12
    tol = s.tol_for(m)
    atol = tol * float(np.linalg.norm(s.b))
    for r in _three(s, tol=tol, maxiter=10 * s.N):
        assert r.iters == m and r.info == 0 and r.callbacks == m
        assert len(r.recheck) == 1 and r.recheck[0][0] == m and r.recheck[0][3]
        _assert_margins(r.trace, m, atol, name)
        assert r.recheck[0][1] <= (1 - MARGIN) * atol      # the recurrence residual passed first
    for r in _three(s, tol=tol, maxiter=1):
        assert r.iters == r.info == 1
    for r in _three(s, tol=tol, maxiter=m - 1):
        assert r.iters == r.info == m - 1 and not r.recheck
    for r in _three(s, tol=tol, maxiter=m):
        assert r.iters == m and r.info == 0                # convergence at maxiter: info 0 wins


@pytest.mark.parametrize("name", list(pc.B6_CASES))
def test_b6_b7_failing_recheck(name):
    """The float64 oracles agree on j*, with the margins, and their true residual there is
    >= 100 atol; the long-double oracle does not take this path (its r0 is clean)."""
    s = pc.b6_system(name)
    k = s.label
    b, x0, tol = pc.b6_inputs(s)
    atol = tol * float(np.linalg.norm(b))
    j, runs = pc.b6_runs(s)
    for r in runs:
        assert r.recheck and r.recheck[0][0] == j and not r.recheck[0][3]
        _assert_margins(np.concatenate([r.trace[:j], [r.recheck[0][1]]]), j, atol, k)
        assert r.recheck[0][2] >= 100 * atol and r.trace[j] == r.recheck[0][2]
        assert r.iters == r.info == j + pc.B6_MORE and all(not c[3] for c in r.recheck)
    # the 1 % the device's recurrence residuals are held to: on the compared entries the oracle's
    # own orders are ten times closer; on the others they are not within 1 % themselves
    d = np.abs(runs[0].trace[:j] / runs[1].trace[:j] - 1)
    sure = pc.b6_compared(s)
    assert sure.sum() >= j // 2 and np.all(d[sure] <= 1e-3) and np.max(d[~sure]) > 1e-2
    print(f"pcg-sweep b6 k={k}: j*={j} recurrence {[float(r.recheck[0][1]) for r in runs]} "
          f"true {[float(r.recheck[0][2]) for r in runs]}; {int(sure.sum())} entries compared, orders "
          f"differ by {np.max(d[sure]):.2e} there and by {np.max(d[~sure]):.2e} elsewhere; "
          f"projection residuals {[pc.projection_residual(s, r.xs, j, b) for r in runs]} "
          f"bound {pc.b6_projection_bound(s):.3e}")
    assert pc.b6_projection_bound(s) < 0.5                 # a z from another residual gives ~ 1
    ld = s.solve(LD, b=b, x0=x0, tol=tol, maxiter=j + pc.B6_MORE)
    assert ld.info == 0 or ld.recheck[0][0] != j or ld.recheck[0][3]
    for r in (s.solve(F64, rev, b=b, x0=x0, tol=tol, maxiter=j) for rev in (False, True)):   # B7
        assert r.iters == r.info == j and r.trace[j] >= 100 * atol and len(r.recheck) == 1
