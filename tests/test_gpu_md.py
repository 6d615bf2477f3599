"""Molecular dynamics on the GPU (sgdml_amd.GDMLPredict.md -> mlff_md_run, csrc/kernels_md.hip).

Two yardsticks.  The frames of a run equal, bit for bit, those of the numpy loop
    v += h F;  R += dt v;  E, F = predict(R);  v += h F        (h = (0.5 dt acc_unit) / m per row)
over the same object's `predict`: the device run shares the prediction's kernels and reduction
orders and rounds each product before its sum, as numpy does.  And the last frame is held against
the long-double oracle of tests/md_oracle.py (anchored on the CPU in tests/test_md_oracle.py) by
the project's rule: max|gpu - ref_ld| <= 10 band max|ref_ld|, band = the float64 oracle's deviation
from the long-double one on the same inputs, floored at 2^-52, evaluated at run time.  Every test
prints its figures before it asserts.

Shapes from tests/sgdml_shapes.TABLE, the smallest that reach each branch; models of
hessian_oracle.random_model (std 1.75, c -3), plain and with alphas_E; five replicas from training
geometries plus 0.05 N(0, 1), velocities 0.01 N(0, 1) Angstrom / fs, masses uniform in [1, 16];
at most 16 steps of 0.5 fs.  Tile models (D <= 288) have both forms of the step (two and four
launches) and also run under MLFF_PRED_FORM=stream.
"""
import ctypes
from functools import lru_cache

import numpy as np
import pytest

from tests import md_oracle as mo
from tests.sgdml_shapes import FLOOR, LD, held

pytestmark = pytest.mark.gpu

CASES = [
    (2, 1, "id"),          # D = 1
    (3, 4, "nongroup"),    # smallest with non-trivial permutations
    (9, 17, "c3"),         # ethanol's D = 36
    (22, 3, "id"),         # 3n = 66: a second 64-row block of the J^T stage; D = 231
    (24, 3, "swap"),       # last tile D
    (25, 3, "id"),         # first stream D: four launches only
    (86, 2, "swap"),       # 3n = 258 > 256
]
TILE = [k for k in CASES if k[0] * (k[0] - 1) // 2 <= 288]
# (case, MLFF_PRED_FORM): the default form of every case, and the stream form where it is not
RUNS = [(k, None) for k in CASES] + [(k, "stream") for k in TILE]
ECSTR = [False, True]
Q, STEPS, DT = 5, 12, 0.5
ACC = 4.184e-4


def case_id(k):
    return f"n{k[0]}-M{k[1]}-{k[2]}"


def run_id(r):
    return case_id(r[0]) + ("" if r[1] is None else "-" + r[1])


@pytest.fixture(scope="module")
def sg():
    import sgdml_amd

    if sgdml_amd.device_count() < 1:
        pytest.fail("no GPU visible to libmlffpcg.so")
    return sgdml_amd


@lru_cache(maxsize=None)
def setup(key, ecstr):
    """(model, model arrays, R0, V0, masses) of a case; computed once, read-only."""
    return mo.start(*key, ecstr, Q, 5000 * key[0] + key[1])


@lru_cache(maxsize=None)
def last_frames(key, ecstr):
    """The oracle's last frame (R, V) after STEPS steps in long double and in float64."""
    _, ma, R0, V0, masses = setup(key, ecstr)
    out = []
    for dtype in (LD, np.float64):
        tr = mo.verlet(ma, R0, V0, masses, DT, STEPS, STEPS, ACC, dtype)
        out.append((tr["R"][:, -1], tr["V"][:, -1]))
    return out


def env(monkeypatch, form=None, slab=None, frames=None):
    for name, v in (("MLFF_PRED_FORM", form), ("MLFF_PRED_SLAB", slab), ("MLFF_MD_FRAMES", frames)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


def forms_of(gd):
    """The forms of the step this model has: launches per step."""
    return (2, 4) if gd.form == "tile" else (4,)


def host_loop(gd, R0, V0, masses, dt, steps):
    """Every frame (R, V, E, F) of the numpy loop over gd.predict."""
    n3 = R0.shape[1] * 3
    h = np.repeat((0.5 * dt * ACC) / masses, 3)
    R, V = R0.reshape(-1, n3).copy(), V0.reshape(-1, n3).copy()
    E, F = gd.predict(R)
    fr = [(R, V, E, F)]
    for _ in range(steps):
        V = V + h * F
        R = R + dt * V
        E, F = gd.predict(R)
        V = V + h * F
        fr.append((R, V, E, F))
    return [np.stack([f[i] for f in fr], axis=1) for i in range(4)]


def same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("R", "V", "E", "F", "step")) and set(a) == set(b)


# ---------------------------------------------------------------- 1. the host loop's bits
@pytest.mark.parametrize("ecstr", ECSTR, ids=["plain", "ecstr"])
@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_same_bits_as_the_host_loop(sg, run, ecstr, monkeypatch):
    key, form = run
    env(monkeypatch, form)
    model, _, R0, V0, masses = setup(key, ecstr)
    n = key[0]
    with sg.GDMLPredict(model, device=0) as gd:
        assert gd.form == (form or ("tile" if key in TILE else "stream")) and gd.use_E_cstr == ecstr
        Rl, Vl, El, Fl = host_loop(gd, R0, V0, masses, DT, STEPS)
        for launches in forms_of(gd):
            tr = gd.md(R0, V0, masses, DT, STEPS, stride=1, forces=True, launches=launches)
            assert gd.md_info()[0] == launches
            assert tr["R"].shape == (Q, STEPS + 1, n, 3) and tr["V"].shape == (Q, STEPS + 1, n, 3)
            assert tr["E"].shape == (Q, STEPS + 1) and tr["F"].shape == (Q, STEPS + 1, 3 * n)
            assert np.array_equal(tr["step"], np.arange(STEPS + 1)) and tr["step"].dtype == np.int64
            diff = [int(np.sum(a.reshape(b.shape) != b)) for a, b in
                    ((tr["R"], Rl), (tr["V"], Vl), (tr["E"], El), (tr["F"], Fl))]
            moved = float(np.max(np.abs(tr["R"][:, -1] - R0)))
            print(f"{run_id(run)} ecstr={ecstr} {launches} launches: entries that differ from the host loop "
                  f"R {diff[0]} V {diff[1]} E {diff[2]} F {diff[3]}; largest coordinate change {moved:.3e}")
            assert np.all(np.isfinite(tr["R"])) and moved > 1e-3
            assert diff == [0, 0, 0, 0]


# ---------------------------------------------------------------- 2. the long-double oracle
def check_oracle(label, tr, ref_ld, ref_64):
    for name, i in (("R", 0), ("V", 1)):
        band = max(FLOOR, float(np.max(np.abs(ref_64[i].astype(LD) - ref_ld[i])) / np.max(np.abs(ref_ld[i]))))
        held(tr[name][:, -1], ref_ld[i], band, f"{label} md {name} after {tr['step'][-1]} steps")


@pytest.mark.parametrize("ecstr", ECSTR, ids=["plain", "ecstr"])
@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_matches_the_long_double_oracle(sg, run, ecstr, monkeypatch):
    key, form = run
    env(monkeypatch, form)
    model, _, R0, V0, masses = setup(key, ecstr)
    ref_ld, ref_64 = last_frames(key, ecstr)
    with sg.GDMLPredict(model, device=0) as gd:
        tr = gd.md(R0, V0, masses, DT, STEPS, stride=STEPS)
    assert "F" not in tr and tr["R"].shape[1] == 2
    check_oracle(f"{run_id(run)}{' ecstr' if ecstr else ''}", tr, ref_ld, ref_64)


def test_golden_ethanol_matches_the_long_double_oracle(sg, golden_dir, monkeypatch):
    """The 23-point ethanol model of tests/golden/sgdml_predict_cases.npz: masses from z, 16 steps
    of 0.5 fs from five of its stored query geometries, 0.01 N(0, 1) Angstrom / fs velocities."""
    from sgdml_amd.model import r_d_desc_alpha
    from sgdml_amd.predict import load_model_arrays
    from sgdml_amd.solver import host_descriptors

    env(monkeypatch)
    f = np.load(golden_dir / "sgdml_predict_cases.npz", allow_pickle=False)
    Rd, Rdd = host_descriptors(f["eth__R_train"])
    model = {"type": "m", "z": f["eth__z"], "perms": f["eth__perms"], "sig": f["eth__sig"], "std": f["eth__std"],
             "c": f["eth__c"], "R_desc": Rd.T, "R_d_desc_alpha": r_d_desc_alpha(Rdd, f["eth__alphas_F"])}
    assert f["eth__R_train"].shape[0] == 23
    masses = np.array([mo.MASS_OF_Z[int(z)] for z in f["eth__z"]])
    R0 = f["eth__R"][:Q]
    V0 = 0.01 * np.random.default_rng(23).standard_normal(R0.shape)
    ma = load_model_arrays(model, energy_constraints=True)
    refs = []
    for dtype in (LD, np.float64):
        tr = mo.verlet(ma, R0, V0, masses, 0.5, 16, 16, ACC, dtype)
        refs.append((tr["R"][:, -1], tr["V"][:, -1]))
    with sg.GDMLPredict(model, device=0) as gd:
        for launches in forms_of(gd):
            check_oracle(f"golden ethanol, {launches} launches",
                         gd.md(R0, V0, masses, 0.5, 16, stride=16, launches=launches), *refs)


# ---------------------------------------------------------------- 3. invariances, bit for bit
@pytest.mark.parametrize("ecstr", ECSTR, ids=["plain", "ecstr"])
@pytest.mark.parametrize("run", RUNS, ids=run_id)
def test_bits_do_not_depend_on_batch_stride_restart_buffers_or_form(sg, run, ecstr, monkeypatch):
    key, form = run
    env(monkeypatch, form)
    model, _, R0, V0, masses = setup(key, ecstr)
    args = (masses, DT, STEPS)
    with sg.GDMLPredict(model, device=0) as gd:
        full = gd.md(R0, V0, *args, forces=True)
        cap = gd.md_info()[1]
        # the other form of the step
        for launches in forms_of(gd):
            assert same(gd.md(R0, V0, *args, forces=True, launches=launches), full), (run, launches)
        # a replica alone, and at the positions 0, 2 and 4 of the batch
        alone = gd.md(R0[1], V0[1], *args, forces=True)
        assert all(np.array_equal(alone[k][0], full[k][1]) for k in ("R", "V", "E", "F"))
        for pos in (0, 2, 4):
            order = np.arange(Q)
            order[[1, pos]] = order[[pos, 1]]
            tr = gd.md(R0[order], V0[order], *args, forces=True)
            assert all(np.array_equal(tr[k][pos], alone[k][0]) for k in ("R", "V", "E", "F")), (run, pos)
        # every fourth frame
        s4 = gd.md(R0, V0, *args, stride=4, forces=True)
        assert np.array_equal(s4["step"], [0, 4, 8, 12])
        assert all(np.array_equal(s4[k], full[k][:, ::4]) for k in ("R", "V", "E", "F"))
        # restart from a frame
        a = gd.md(R0, V0, masses, DT, 6, forces=True)
        b = gd.md(a["R"][:, -1], a["V"][:, -1], masses, DT, 6, forces=True)
        for k in ("R", "V", "E", "F"):
            assert np.array_equal(a[k], full[k][:, :7]) and np.array_equal(b[k], full[k][:, 6:]), (run, k)
    assert cap >= 2           # the budget's capacity above; two frames, so seven flushes, here
    env(monkeypatch, form, frames=2)
    with sg.GDMLPredict(model, device=0) as gd:
        assert same(gd.md(R0, V0, *args, forces=True), full)
        assert gd.md_info()[1:] == (2, 7)
    env(monkeypatch, form, slab=2)
    with sg.GDMLPredict(model, device=0) as gd:
        assert gd.slab == 2     # slabs of 2, 2 and 1 replicas
        for launches in forms_of(gd):
            assert same(gd.md(R0, V0, *args, forces=True, launches=launches), full), (run, "slab", launches)
    env(monkeypatch, form)
    with sg.GDMLPredict(model, devices=[0, 0]) as gd:
        assert same(gd.md(R0, V0, *args, forces=True), full)           # 3 + 2 replicas
        one = gd.md(R0[:1], V0[:1], *args, forces=True)                # one empty block
        assert all(np.array_equal(one[k], full[k][:1]) for k in ("R", "V", "E", "F"))


# ---------------------------------------------------------------- 4. no step
@pytest.mark.parametrize("run", [((9, 17, "c3"), None), ((25, 3, "id"), None)], ids=run_id)
def test_zero_steps_give_the_start(sg, run, monkeypatch):
    key, form = run
    env(monkeypatch, form)
    model, _, R0, V0, masses = setup(key, True)
    with sg.GDMLPredict(model, device=0) as gd:
        E, F = gd.predict(R0)
        for launches in forms_of(gd):
            tr = gd.md(R0, V0, masses, DT, 0, forces=True, launches=launches)
            assert tr["R"].shape == (Q, 1, key[0], 3) and np.array_equal(tr["step"], [0])
            assert np.array_equal(tr["R"][:, 0], R0) and np.array_equal(tr["V"][:, 0], V0)
            assert np.array_equal(tr["E"][:, 0], E) and np.array_equal(tr["F"][:, 0], F)
            assert gd.md_info()[2] == 1
        e = gd.md(np.empty((0, key[0], 3)), np.empty((0, 3 * key[0])), masses, DT, 4, stride=2, forces=True)
        assert e["R"].shape == (0, 3, key[0], 3) and e["E"].shape == (0, 3) and e["F"].shape == (0, 3, 3 * key[0])
        assert gd.md_info()[2] == 0


# ---------------------------------------------------------------- 5. launches and synchronisations
@pytest.mark.parametrize("run", [((9, 17, "c3"), None), ((9, 17, "c3"), "stream"), ((25, 3, "id"), None)], ids=run_id)
def test_md_info_counts_flushes_not_steps(sg, run, monkeypatch):
    key, form = run
    env(monkeypatch, form, frames=4)
    model, _, R0, V0, masses = setup(key, False)
    with sg.GDMLPredict(model, device=0) as gd:
        launches, cap, syncs = gd.md_info()
        assert launches == (2 if gd.form == "tile" else 4) and cap == 4 and syncs == 0
        for stride, frames in ((1, 13), (4, 4), (12, 2), (3, 5)):
            gd.md(R0, V0, masses, DT, STEPS, stride=stride)
            got = gd.md_info()
            print(f"{run_id(run)}: {STEPS} steps, stride {stride}: {frames} frames, capacity 4, "
                  f"{got[2]} synchronisations, {got[0]} launches per step")
            assert got == (launches, 4, -(-frames // 4))
        gd.md(R0, V0, masses, DT, STEPS, launches=4)
        assert gd.md_info() == (4, 4, 4)
    env(monkeypatch, form, slab=2, frames=4)
    with sg.GDMLPredict(model, device=0) as gd:
        gd.md(R0, V0, masses, DT, STEPS)
        assert gd.md_info()[2] == 3 * 4     # three slabs, four flushes each


# ---------------------------------------------------------------- 6. errors and state
def test_errors(sg, monkeypatch):
    from sgdml_amd import _native as nat

    env(monkeypatch)
    key = (9, 17, "c3")
    model, _, R0, V0, masses = setup(key, False)
    dp = ctypes.POINTER(ctypes.c_double)
    R1, V1 = np.ascontiguousarray(R0[:1]), np.ascontiguousarray(V0[:1]).reshape(1, 27)
    h = np.ascontiguousarray((0.5 * DT * ACC) / masses)
    out = [np.empty((1, 2, 27)), np.empty((1, 2, 27)), np.empty((1, 2)), np.empty((1, 2, 27))]

    def raw(eng, steps, stride, want_f=1, dt=DT, Q=1, null=None):
        ptr = [a.ctypes.data_as(dp) for a in (R1, V1, h, *out)]
        if null is not None:
            ptr[null] = None
        return eng._lib.mlff_md_run(eng._ctx, ptr[0], ptr[1], ptr[2], Q, dt, steps, stride, want_f, *ptr[3:])

    live0 = nat.live_bytes()
    with sg.KernelSolver(3 * 9 * 17, device=0) as s:
        assert raw(s, 1, 1) == nat.MLFF_ERR_STATE
        assert s._lib.mlff_md_info(s._ctx, None, None, None) == nat.MLFF_ERR_STATE
        with pytest.raises(RuntimeError, match="no model set"):
            s.md_run(R1, V1, h, DT, 1)
    with sg.GDMLPredict(model, device=0) as gd:
        eng = gd._engines[0]
        live1 = nat.live_bytes()
        assert raw(eng, 1, 0) == nat.MLFF_ERR_ARG          # stride = 0
        assert raw(eng, 3, 2) == nat.MLFF_ERR_ARG          # not a multiple
        assert raw(eng, -1, 1) == nat.MLFF_ERR_ARG
        assert raw(eng, 1, 1, Q=-1) == nat.MLFF_ERR_ARG
        assert raw(eng, 1, 1, dt=float("inf")) == nat.MLFF_ERR_ARG
        assert raw(eng, 1, 1, dt=float("nan")) == nat.MLFF_ERR_ARG
        for null in range(7):                              # F_out may be null only without forces
            assert raw(eng, 1, 1, null=null) == nat.MLFF_ERR_ARG
        with pytest.raises(ValueError):
            eng.md_set_form(3)
        bad = [
            (R0, V0[:4], masses, DT, STEPS), (R0, V0, masses[:-1], DT, STEPS), (R0, V0, -masses, DT, STEPS),
            (R0, V0, masses * np.inf, DT, STEPS), (R0, V0, masses, np.nan, STEPS), (R0, V0, masses, DT, -1),
            (R0, V0, masses, DT, STEPS, 0), (R0, V0, masses, DT, STEPS, 5), (R0[:, :8], V0, masses, DT, STEPS),
        ]
        for a in bad:
            with pytest.raises(ValueError):
                gd.md(*a)
        with pytest.raises(ValueError):
            gd.md(R0, V0, masses, DT, STEPS, launches=3)
        # none of these reached the device: no buffer was allocated, no run was counted
        assert nat.live_bytes() == live1 and gd.md_info()[2] == 0
        assert raw(eng, 1, 1, want_f=0, null=6) == nat.MLFF_OK
        ref = gd.md(R1, V1, masses, DT, 1, forces=True)
        assert raw(eng, 1, 1) == nat.MLFF_OK
        for a, k in zip(out, ("R", "V", "E", "F")):
            assert np.array_equal(a.reshape(ref[k].shape), ref[k])
        assert nat.live_bytes() > live1
    with pytest.raises(RuntimeError):
        gd.md(R0, V0, masses, DT, STEPS)
    with pytest.raises(RuntimeError):
        gd.md_info()
    assert nat.live_bytes() == live0
    env(monkeypatch, "stream")
    with sg.GDMLPredict(model, device=0) as gd:
        with pytest.raises(ValueError, match="tile model"):
            gd.md(R0, V0, masses, DT, STEPS, launches=2)
    env(monkeypatch, frames=0)
    with sg.GDMLPredict(model, device=0) as gd:
        with pytest.raises(ValueError, match="MLFF_MD_FRAMES"):
            gd.md(R0, V0, masses, DT, STEPS)


# ---------------------------------------------------------------- 7. a replica that blows up
@pytest.mark.parametrize("run", [((9, 17, "c3"), None), ((9, 17, "c3"), "stream"), ((25, 3, "id"), None)], ids=run_id)
def test_coinciding_atoms_stay_in_their_replica(sg, run, monkeypatch):
    """Replica 2 starts with atom 1 on atom 0: its descriptor has an infinite entry, its frames
    are not finite from the first E and F on, and the other four replicas keep their bits (the
    kernels have no data-dependent addressing and no sum across replicas)."""
    key, form = run
    env(monkeypatch, form)
    model, _, R0, V0, masses = setup(key, True)
    Rb = R0.copy()
    Rb[2, 1] = Rb[2, 0]
    others = [0, 1, 3, 4]
    with sg.GDMLPredict(model, device=0) as gd:
        for launches in forms_of(gd):
            good = gd.md(R0, V0, masses, DT, 4, forces=True, launches=launches)
            tr = gd.md(Rb, V0, masses, DT, 4, forces=True, launches=launches)
            assert np.array_equal(tr["R"][2, 0], Rb[2]) and np.array_equal(tr["V"][2, 0], V0[2])
            assert not np.any(np.isfinite(tr["E"][2])) and not np.all(np.isfinite(tr["F"][2, 0]))
            assert not np.any(np.isfinite(tr["R"][2, 1:, :2])) and not np.any(np.isfinite(tr["V"][2, 1:, :2]))
            for k in ("R", "V", "E", "F"):
                assert np.array_equal(tr[k][others], good[k][others]), (run, launches, k)
            assert same(gd.md(R0, V0, masses, DT, 4, forces=True, launches=launches), good)
