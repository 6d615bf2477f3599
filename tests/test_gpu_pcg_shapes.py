"""The PCG iteration and its stop rules against the long-double oracle (tests/pcg_shapes.py: the
tables, the systems, the references, the bands; its conditions are checked on the CPU in
tests/test_oracle_pcg_longdouble.py).

Table A: J iterations at tol = 0 on every form the storage admits; x_J and every trace entry are
held (sgdml_shapes.held: 10 x the spread of the oracle's own float64 evaluations around its
long-double run, no tolerance written here).  Table B: the discrete stop decisions of scipy 1.7.3,
posed with a 5 % margin so that they are compared exactly.  Table C: solver state across solves on
one context.  Every comparison prints its deviation, bound, band and ratio before it asserts;
profiles/pcg_shapes/README.txt holds the measured ratios.  The environment switches used here are
all read when a context, a preconditioner or an operator is built (std::getenv at those calls, no
static), so monkeypatch.setenv before KernelSolver(...) is enough.
"""
import numpy as np
import pytest

from tests import pcg_shapes as pc
from tests import precon_shapes as ps
from tests.pcg_shapes import LD, held

pytestmark = pytest.mark.gpu

RUNNING, CONVERGED, MAXITER = 0, 2, 3        # sgdml_amd._native.PCG_*
SWITCHES = ("MLFF_LR_ROWS", "MLFF_FUSE_P", "MLFF_FUSE_XR", "MLFF_EXACT_SUMS", "MLFF_SYM_SCHED",
            "MLFF_MF_FORM")


@pytest.fixture(scope="module")
def sg():
    import sgdml_amd

    if sgdml_amd.device_count() < 1:
        pytest.fail("no GPU visible to libmlffpcg.so")
    return sgdml_amd


class Form:
    """storage: dense | sym | sym-static | matfree; lr: None (no preconditioner), "0" two-pass,
    "1" one-pass rows; env: further switches; mf: the matrix-free operator form expected."""

    def __init__(self, storage, lr=None, env=None, world=1, mf=None):
        self.storage, self.lr, self.env, self.world, self.mf = storage, lr, dict(env or {}), world, mf
        if storage == "sym-static":
            self.env["MLFF_SYM_SCHED"] = "static"
        parts = [storage, {None: "none", "0": "twopass", "1": "rows"}[lr]]
        parts += [f"{k[5:].lower()}{v}" for k, v in (env or {}).items()]
        parts += [f"W{world}"] if world > 1 else []
        self.id = "-".join(parts)

    def setenv(self, monkeypatch):
        for name in SWITCHES:
            monkeypatch.delenv(name, raising=False)
        for k, v in self.env.items():
            monkeypatch.setenv(k, v)
        if self.lr is not None:
            monkeypatch.setenv("MLFF_LR_ROWS", self.lr)


def _open(sg, s, form, rank=0, world=1, key=None):
    """A context with the system's operator and preconditioner in the given form; asserts that
    the form is the one that runs."""
    p = s.p
    c = sg.KernelSolver(s.N, device=0, rank=rank, world=world, comm_id=key if world > 1 else None)
    try:
        r0, r1 = c.row_range()
        if p.kind == "rbf":
            c.gen_rbf(p.X, ps.LENGTH_SCALE, ps.JITTER)
        elif p.kind in ("sgdml", "sgdmlE"):
            Rd, Rdd = p.mol.desc
            c.sgdml_operator(Rd, Rdd, p.mol.perms, pc.SIG, use_E_cstr=p.kind == "sgdmlE")
        else:
            c.set_matrix(np.ascontiguousarray(s.sigma_K * p.S64[r0:r1]))
        c.set_operator(s.sigma_K, s.lam)
        c.set_storage(form.storage.split("-")[0])
        if s.k:
            assert form.lr is not None
            c.precon_lowrank(np.ascontiguousarray(s.Lt64[:, r0:r1]))
            assert c.precon_info() == (4, s.k)
            # the one-pass apply exists on one rank only
            assert c.precon_apply_traffic()[0] == (int(form.lr) if world == 1 else 0)
        else:
            assert form.lr is None
            c.precon_none()
        assert c.storage_info()[0] == form.storage.split("-")[0]
        if form.storage == "sym-static":
            assert c.sym_launch_info() == (0, 0)
        elif form.storage == "sym":
            assert c.sym_launch_info()[1] > 0
        if form.mf is not None:
            assert c.operator_form() == form.mf
    except BaseException:
        c.close()
        raise
    return c


class Out:
    """One device solve, the ranks' blocks of x concatenated; every rank holds the same iteration
    count, status and trace, bit for bit."""

    def __init__(self, parts, N):
        parts = sorted(parts, key=lambda o: (o["r"], o["rank"]))
        assert parts[0]["r"][0] == 0 and parts[-1]["r"][1] == N
        assert all(a["r"][1] == b["r"][0] for a, b in zip(parts, parts[1:]))
        first = parts[0]
        for o in parts[1:]:
            for key in ("iters", "info", "early", "callbacks", "status"):
                assert o[key] == first[key], key
            assert np.array_equal(o["trace"], first["trace"])
            assert len(o["xs"]) == len(first["xs"]) and o["statuses"] == first["statuses"]
            assert all(np.array_equal(a, b) for a, b in zip(o["traces"], first["traces"]))
        self.x = np.concatenate([o["x"] for o in parts])
        self.xs = [np.concatenate([o["xs"][i] for o in parts]) for i in range(len(first["xs"]))]
        self.iters, self.info, self.trace = first["iters"], first["info"], first["trace"]
        self.early, self.callbacks, self.status = first["early"], first["callbacks"], first["status"]
        self.statuses, self.traces = first["statuses"], first["traces"]


def _on_ranks(sg, s, form, fn):
    """fn(context, r0, r1) on every rank of the form; the list of its results."""
    def body(rank, world, key):
        with _open(sg, s, form, rank, world, key) as c:
            r0, r1 = c.row_range()
            out = fn(c, r0, r1)
            if isinstance(out, dict):
                out.update(r=(r0, r1), rank=rank)
            return out

    if form.world == 1:
        return [body(0, 1, None)]
    from tests.test_gpu_multirank import run_ranks

    return run_ranks(form.world, body, timeout=120)


def _cut(v, r0, r1):
    return None if v is None else np.ascontiguousarray(v[r0:r1])


def _result(c, early=False, xs=(), statuses=(), traces=()):
    it, status, _, info = c.pcg_result()
    return {"x": c.pcg_x(), "iters": it, "info": info, "status": status, "trace": c.pcg_trace(),
            "early": early, "callbacks": 0 if early else max(it, 1), "xs": list(xs),
            "statuses": list(statuses), "traces": list(traces)}


def _solve(sg, s, form, b=None, x0=None, tol=0.0, maxiter=None, chunk=0, stepped=False, run=None):
    """One solve through KernelSolver.pcg; stepped: pcg_start, then pcg_run(1, chunk = 1) while
    running, x and the trace read after every iteration; run: pcg_start + pcg_run(run) only."""
    b = s.b if b is None else b

    def fn(c, r0, r1):
        if not stepped and run is None:
            res = c.pcg(_cut(b, r0, r1), _cut(x0, r0, r1), tol=tol, maxiter=maxiter, chunk=chunk)
            out = _result(c, res.early_exit)
            assert np.array_equal(out["x"], res.x) and np.array_equal(out["trace"], res.trace)
            assert (out["iters"], out["info"], out["callbacks"]) == (res.iters, res.info, res.callbacks)
            return out
        early = c.pcg_start(_cut(b, r0, r1), _cut(x0, r0, r1), tol=tol, maxiter=maxiter)
        if run is not None:
            c.pcg_run(run, chunk)
            return _result(c, early)
        xs, statuses, traces = [c.pcg_x()], [c.pcg_result()[1]], [c.pcg_trace()]
        while statuses[-1] == RUNNING:
            statuses.append(c.pcg_run(1, 1))
            xs.append(c.pcg_x())
            traces.append(c.pcg_trace())
        return _result(c, early, xs, statuses, traces)

    return Out(_on_ranks(sg, s, form, fn), s.N)


# ---------------------------------------------------------------- Table A
def _forms_stored(k, rbf=False):
    """Forms of a host-matrix or RBF system: three storages x the applies, MLFF_FUSE_P = 0 where
    the tile workgroups would form p (symmetric tiles, dynamic schedule, low-rank apply)."""
    lrs = ("0", "1") if k else (None,)
    forms = [Form(st, lr) for st in ("dense", "sym", "sym-static") for lr in lrs]
    if k:
        forms += [Form("sym", lr, {"MLFF_FUSE_P": "0"}) for lr in lrs]
    return forms


def _table_a():
    rows = []
    for inp, k, lam, J in pc.TABLE_A:
        rows += [(inp, k, lam, J, f) for f in _forms_stored(k)]
    # the exact-sum anchor is a dense-row operator on one rank (every other storage is refused)
    exact = {"MLFF_EXACT_SUMS": "1"}
    rows += [(("spd", 257), 0, pc.HOST_LAM, 8, Form("dense", None, exact)),
             (("spd", 257), 33, pc.HOST_LAM, 8, Form("dense", "0", exact)),
             (("rbf", 65), 9, 1e-2, 8, Form("dense", "0", exact))]
    for case, k, J0, Jk, mf_env, mf, fused in pc.SGDML_A:
        inp = ("sgdml",) + case
        env = {"MLFF_MF_FORM": mf_env} if mf_env else {}
        rows += [(inp, 0, None, J0, Form("matfree", None, env, mf=mf)),
                 (inp, k, None, Jk, Form("matfree", "0", env, mf=mf)),
                 (inp, k, None, Jk, Form("matfree", "1", env, mf=mf))]
        if fused:       # the folds: p formed inside the operator, x / r moved into the next apply
            rows += [(inp, 0, None, J0, Form("matfree", None, {**env, "MLFF_FUSE_P": "0"}, mf=mf)),
                     (inp, k, None, Jk, Form("matfree", "1", {**env, "MLFF_FUSE_P": "0"}, mf=mf)),
                     (inp, k, None, Jk, Form("matfree", "1", {**env, "MLFF_FUSE_XR": "0"}, mf=mf))]
    case, k, J0, Jk = pc.ECSTR_A       # energy constraints: N = 3 n M + M, the pair sums
    inp = ("sgdmlE",) + case
    rows += [(inp, 0, None, J0, Form("matfree", None, mf="pair")),
             (inp, k, None, Jk, Form("matfree", "0", mf="pair")),
             (inp, k, None, Jk, Form("matfree", "1", mf="pair"))]
    return rows


def _ranks_a():
    rows = []
    for inp, k, worlds in pc.RANKS_A:
        lam, J = next((lam, J) for i, kk, lam, J in pc.TABLE_A if (i, kk) == (inp, k))
        for w in worlds:
            for st in ("dense", "sym"):
                rows += [(inp, 0, lam, J, Form(st, None, world=w)), (inp, k, lam, J, Form(st, "0", world=w))]
    case, k, w = pc.RANKS_SGDML
    J0, Jk = next((J0, Jk) for c, _, J0, Jk, *_ in pc.SGDML_A if c == case)
    rows += [(("sgdml",) + case, 0, None, J0, Form("matfree", None, world=w, mf="pt")),
             (("sgdml",) + case, k, None, Jk, Form("matfree", "0", world=w, mf="pt"))]
    return rows


A_ROWS = _table_a() + _ranks_a()


@pytest.mark.parametrize("inp,k,lam,J,form", A_ROWS, ids=[f"{pc.sys_id(i, k)}-{f.id}" for i, k, _, _, f in A_ROWS])
def test_iterates_after_J_iterations(sg, monkeypatch, inp, k, lam, J, form):
    """tol = 0, maxiter = J: iters == info == J, x_J and trace[0..J] held to the long-double run
    (the ranks' blocks concatenated: held to the reference, not to the one-rank run)."""
    s = pc.system(inp, k, lam)
    ref, _ = s.smooth(J)
    bx, bt = s.smooth_bands(J)
    form.setenv(monkeypatch)
    got = _solve(sg, s, form, tol=0.0, maxiter=J)
    tag = f"{s.label} {form.id} J={J}"
    assert not got.early and got.trace.size == got.iters + 1
    if s.N == 1:
        # x_1 = b / a and r_1 = b - alpha q is the rounding error of alpha, at most 3 x 2^-53 |b|
        # to first order (rho, p.q and the division: one rounding each).  Whether it is exactly
        # zero, so that 0 <= atol = 0 converges at ITER 1, is a rounding matter: the oracle
        # rounds alpha q to b (zero, info 0; with a preconditioner not even that, see
        # pcg_shapes.converges_at_1), the device's fma(-alpha, q, r) keeps the remainder
        # (MI355X: 3.3e-17 |b|, info 1).  So: the stop rule applied to the device's own residual.
        print(f"pcg-sweep {tag}: trace[1] / trace[0] = {got.trace[1] / got.trace[0]:.3e} info={got.info}")
        assert got.iters == 1 and got.trace[1] <= 4 * 2.0 ** -53 * got.trace[0]
        assert (got.info, got.status) == ((0, CONVERGED) if got.trace[1] == 0 else (1, MAXITER))
        held(got.x, ref.x, bx, f"{tag} x")
        held(got.trace[:1], ref.trace[:1], bt, f"{tag} trace[0]", scale=ref.trace[:1])
        return
    assert got.iters == got.info == J and got.status == MAXITER
    held(got.x, ref.x, bx, f"{tag} x")
    held(got.trace, ref.trace, bt, f"{tag} trace", scale=ref.trace)


# ---------------------------------------------------------------- Table B
B_FORMS = [("host", Form("dense")), ("host", Form("dense", world=3)),
           ("host-lr", Form("sym", "1")), ("host-lr", Form("sym", "0", world=3)),
           ("sgdml-pt", Form("matfree", "1", mf="pt"))]
B_IDS = [f"{n}-{f.id}" for n, f in B_FORMS]


@pytest.mark.parametrize("name,form", B_FORMS, ids=B_IDS)
def test_b1_legacy_early_exit(sg, monkeypatch, name, form):
    s, _ = pc.b_system(name)
    form.setenv(monkeypatch)
    x0 = np.linalg.solve(s.A_ld().astype(np.float64), s.b)
    got = _solve(sg, s, form, x0=x0, tol=1e-6, maxiter=10 * s.N)
    assert got.early and got.iters == 0 and got.info == 0 and got.callbacks == 0
    assert np.array_equal(got.x, x0) and got.trace.size == 1
    for tol in (0.0, 1e-8):
        got = _solve(sg, s, form, b=np.zeros(s.N), tol=tol, maxiter=10 * s.N)
        assert got.early and got.iters == 0 and got.info == 0 and got.callbacks == 0
        assert not np.any(got.x)


@pytest.mark.parametrize("name,form", B_FORMS, ids=B_IDS)
def test_b2_small_r0_without_early_exit(sg, monkeypatch, name, form):
    s, _ = pc.b_system(name)
    form.setenv(monkeypatch)
    b, x0, tol = pc.b2_inputs(s)
    ref, evals = s.solve(LD, b=b, x0=x0, tol=tol), [s.solve(np.float64, rev, b=b, x0=x0, tol=tol) for rev in (0, 1)]
    band = max([pc.FLOOR] + [float(abs(e.trace[0] - ref.trace[0]) / ref.trace[0]) for e in evals])
    got = _solve(sg, s, form, b=b, x0=x0, tol=tol, maxiter=10 * s.N)
    assert not got.early and got.iters == 0 and got.info == 0 and got.callbacks == 1
    assert got.status == CONVERGED and np.array_equal(got.x, x0)
    held(got.trace, ref.trace, band, f"{name} {form.id} B2 trace", scale=ref.trace)


@pytest.mark.parametrize("name,form", B_FORMS, ids=B_IDS)
def test_b3_converges_at_iteration_1(sg, monkeypatch, name, form):
    s, _ = pc.b_system(name)
    form.setenv(monkeypatch)
    b, tol = pc.b3_inputs(s)
    got = _solve(sg, s, form, b=b, tol=tol, maxiter=10 * s.N)
    atol = tol * float(np.linalg.norm(b))
    print(f"pcg-sweep {name} {form.id} B3: trace[1] / atol = {got.trace[1] / atol:.3e}")
    assert got.iters == 1 and got.info == 0 and got.status == CONVERGED and got.callbacks == 1
    assert got.trace[1] <= atol


@pytest.mark.parametrize("name,form", B_FORMS, ids=B_IDS)
def test_b4_b5_convergence_chunks_and_maxiter(sg, monkeypatch, name, form):
    """The stop at the first, a middle and the last iteration of a chunk; then maxiter = 1,
    m - 1 (against pcg_start + pcg_run(m - 1) of the converging solve) and m."""
    s, m = pc.b_system(name)
    form.setenv(monkeypatch)
    tol = s.tol_for(m)
    big = 10 * s.N
    ref, _ = s.runs(("B4", m), tol=tol, maxiter=big)
    bx, bt = s.bands(("B4", m), tol=tol, maxiter=big)
    tag = f"{name} {form.id} B4"
    outs = {chunk: _solve(sg, s, form, tol=tol, maxiter=big, chunk=chunk) for chunk in (1, m - 1, m, m + 1, 0)}
    # with the x, r update of an iteration moved into the next apply (matrix-free + rows apply)
    # the rr partials inside a chunk are summed by k_lr_fin, at a chunk's end by k_update_xr:
    # the same r, another order, so there the trace is held per chunking, not compared bitwise
    moved = form.storage == "matfree" and form.lr == "1"
    for chunk, got in outs.items():
        assert got.iters == m and got.info == 0 and got.callbacks == m and got.status == CONVERGED, chunk
        assert np.array_equal(got.x, outs[1].x), f"x differs between chunk 1 and chunk {chunk}"
        if moved:
            d = np.max(np.abs(got.trace / outs[1].trace - 1))
            print(f"pcg-sweep {tag} chunk {chunk}: trace differs from chunk 1 by {d:.2e}")
        else:
            assert np.array_equal(got.trace, outs[1].trace), chunk
        held(got.trace, ref.trace, bt, f"{tag} chunk {chunk} trace", scale=ref.trace)
    got = outs[0]
    held(got.x, ref.x, bx, f"{tag} x")
    r = s.residual_ld(got.x)
    true = np.sqrt(r @ r)
    held(got.trace[m:], np.array([true]), bt, f"{tag} trace[m] against ||b - A x_m||", scale=np.array([true]))
    # B5
    one = _solve(sg, s, form, tol=tol, maxiter=1)
    assert one.iters == one.info == 1 and one.status == MAXITER
    short = _solve(sg, s, form, tol=tol, maxiter=m - 1)
    part = _solve(sg, s, form, tol=tol, maxiter=big, run=m - 1)
    assert short.iters == short.info == m - 1 and short.status == MAXITER
    assert part.iters == m - 1 and part.status == RUNNING
    assert np.array_equal(short.x, part.x) and np.array_equal(short.trace, part.trace)
    exact = _solve(sg, s, form, tol=tol, maxiter=m)
    assert exact.iters == m and exact.info == 0 and exact.status == CONVERGED
    assert np.array_equal(exact.x, got.x)


B6_FORMS = [("none", Form("dense")), ("lr", Form("dense", "0", world=3)), ("lr", Form("sym", "1")),
            ("sgdml-pt", Form("matfree", "1", mf="pt"))]


@pytest.mark.parametrize("name,form", B6_FORMS, ids=[f"{n}-{f.id}" for n, f in B6_FORMS])
def test_b6_b7_failing_recheck(sg, monkeypatch, name, form):
    """x0 of size 1e8 puts 1e-8 of rounding into r0: the recurrence residual falls through atol
    at j*, the true residual cannot, the recheck fails and the solve goes on from the true r
    (ST_RECHECK -> ST_RUNNING, rho1 = rho, no stale T r or z).  B7: the same at maxiter = j*."""
    s = pc.b6_system(name)
    form.setenv(monkeypatch)
    b, x0, tol = pc.b6_inputs(s)
    atol = tol * float(np.linalg.norm(b))
    j, runs = pc.b6_runs(s)
    last = j + pc.B6_MORE
    tag = f"b6 {s.label} {form.id}"
    got = _solve(sg, s, form, b=b, x0=x0, tol=tol, maxiter=last, stepped=True)
    assert got.iters == got.info == last and got.status == MAXITER
    assert got.statuses == [RUNNING] * last + [MAXITER]
    assert [t.size for t in got.traces] == list(range(1, last + 2))
    # before j*: the recurrence residuals, within 1 % of the float64 oracle's up to the entry at
    # which the oracle's own two orders part (pcg_shapes.b6_compared: they differ by up to 80 %
    # from there on); every entry stays above atol by the margin, which is what decides j*
    sure = pc.b6_compared(s)
    dev = np.abs(got.trace[:j] / runs[0].trace[:j] - 1)
    print(f"pcg-sweep {tag}: j*={j}; {int(sure.sum())} of {j} entries compared to 1 %, largest "
          f"deviation there {np.max(dev[sure]):.2e}, elsewhere {np.max(dev[~sure], initial=0):.2e}")
    assert np.all(dev[sure] <= 1e-2)
    assert np.all(got.trace[:j] >= (1 + pc.MARGIN) * atol)
    # at j*: the entry is the true residual of the device's own x_j*, far above atol
    r = s.residual_ld(got.xs[j], b)
    true = float(np.sqrt(r @ r))
    print(f"pcg-sweep {tag}: trace[j*]={got.trace[j]:.6e} ||b - A x_j*||={true:.6e} atol={atol:.1e}")
    assert abs(got.trace[j] - true) <= 1e-6 * true and got.trace[j] >= 100 * atol
    assert np.array_equal(got.traces[j][:j], got.trace[:j]) and got.traces[j][j] == got.trace[j]
    # the step after the failed recheck: z = P (b - A x_j*) lies in span{d_j*+1, d_j*}
    res = pc.projection_residual(s, got.xs, j, b)
    bound = pc.b6_projection_bound(s)
    print(f"pcg-sweep {tag}: projection residual {res:.3e} bound {bound:.3e} ratio {res / bound:.3f}")
    assert res <= bound
    # unstepped: the stop tests folded into the next iteration; matrix-free + rows apply also moves
    # the x, r update there, and its rr partials are then summed in another order (k_lr_fin, not
    # k_update_xr: the same r, so within N roundings of the sum)
    moved = form.storage == "matfree" and form.lr == "1"
    if form.world == 1 and form.storage in ("dense", "matfree"):
        for chunk in (0, 3):
            whole = _solve(sg, s, form, b=b, x0=x0, tol=tol, maxiter=last, chunk=chunk)
            assert whole.iters == got.iters and whole.info == got.info
            assert np.array_equal(whole.x, got.x), chunk
            if moved:
                d = np.max(np.abs(whole.trace / got.trace - 1))
                print(f"pcg-sweep {tag} chunk {chunk}: trace differs from the stepped run by {d:.2e}")
                assert d <= s.N * 2.0 ** -53
            else:
                assert np.array_equal(whole.trace, got.trace), chunk
    # B7
    end = _solve(sg, s, form, b=b, x0=x0, tol=tol, maxiter=j)
    assert end.iters == end.info == j and end.status == MAXITER
    assert np.array_equal(end.x, got.xs[j])
    if moved:
        assert np.max(np.abs(end.trace / got.trace[:j + 1] - 1)) <= s.N * 2.0 ** -53
    else:
        assert np.array_equal(end.trace, got.trace[:j + 1])


# ---------------------------------------------------------------- Table C
C_FORMS = [Form("dense", "1"), Form("dense", "0", world=3)]


def _grab(c):
    it, status, _, info = c.pcg_result()
    return c.pcg_x(), c.pcg_trace(), it, status, info


def _same(a, b, what):
    assert a[2:] == b[2:], what
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), what


@pytest.mark.parametrize("form", C_FORMS, ids=[f.id for f in C_FORMS])
def test_state_across_solves(sg, monkeypatch, form):
    """One context: the converging solve, the same with maxiter 10 x larger (the trace buffer
    regrows), then a tol = 0 run of 8 iterations: each bit-identical to the same solve on a
    fresh context.  pcg_run in pieces (3, 0, 2) equals pcg_run(5); pcg_run after convergence is
    a no-op."""
    s, m = pc.b_system("host-lr")
    form.setenv(monkeypatch)
    tol = s.tol_for(m)
    solves = [dict(tol=tol, maxiter=2 * m), dict(tol=tol, maxiter=20 * m), dict(tol=0.0, maxiter=8)]

    def one(c, r0, r1, kw, pieces=None):
        c.pcg_start(_cut(s.b, r0, r1), None, **kw)
        for n in pieces or (kw["maxiter"],):
            c.pcg_run(n)
        return _grab(c)

    def fn(c, r0, r1):
        seq = [one(c, r0, r1, kw) for kw in solves]
        again = one(c, r0, r1, solves[0])
        status = c.pcg_run(5)                      # after convergence: nothing moves
        still = _grab(c)
        pieces = one(c, r0, r1, solves[2], (3, 0, 2))
        whole = one(c, r0, r1, solves[2], (5,))
        return {"seq": seq, "again": again, "status": status, "still": still, "pieces": pieces, "whole": whole}

    used = _on_ranks(sg, s, form, fn)
    fresh = [_on_ranks(sg, s, form, lambda c, r0, r1, kw=kw: {"one": one(c, r0, r1, kw)}) for kw in solves]
    for rank, u in enumerate(used):
        for i in range(3):
            _same(u["seq"][i], fresh[i][rank]["one"], f"solve {i} on a used context, rank {rank}")
        assert u["seq"][0][2:] == (m, CONVERGED, 0) and u["seq"][1][2:] == (m, CONVERGED, 0)
        assert u["seq"][2][2:] == (8, MAXITER, 8)
        _same(u["again"], u["seq"][0], "the first solve repeated")
        assert u["status"] == CONVERGED
        _same(u["still"], u["again"], "pcg_run after convergence")
        assert u["pieces"][2:] == (5, RUNNING, 5)
        _same(u["pieces"], u["whole"], "pcg_run(3), (0), (2) against pcg_run(5)")


def test_result_before_start_raises(sg, monkeypatch):
    s, _ = pc.b_system("host-lr")
    form = Form("dense", "1")
    form.setenv(monkeypatch)
    with _open(sg, s, form) as c:
        with pytest.raises(RuntimeError):
            c.pcg_result()
        with pytest.raises(RuntimeError):
            c.pcg_trace()
        with pytest.raises(RuntimeError):
            c.pcg_run(1)
