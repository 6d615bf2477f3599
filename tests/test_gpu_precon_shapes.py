"""Every preconditioner build against the long-double oracle, over the sizes at which the builds
change branch (tests/precon_shapes.py: the tables, the inputs, the references, the bands).

Bound everywhere: 10 x the spread of the oracle's own float64 evaluations around its long-double
run, floored at 2^-52 (sgdml_shapes.held); no tolerance is written here.  Every comparison prints
its deviation, bound, band and ratio before it asserts; profiles/precon_shapes/README.txt holds
the measured ratios.  Each case runs at lam = 1e-4 and at the project's 1e-10, and every apply in
the two-pass and in the one-pass form (MLFF_LR_ROWS = 0 / 1).
"""
import numpy as np
import pytest

from tests import precon_shapes as ps
from tests.precon_shapes import LAMS, LD, held

pytestmark = pytest.mark.gpu

KIND = {"wood": 1, "nys0": 2, "nys1": 3, "lowrank": 4, "eig": 5}      # MLFF_PRECON_*
LAM_IDS = [ps.lam_id(x) for x in LAMS]


@pytest.fixture(scope="module")
def sg():
    import sgdml_amd

    if sgdml_amd.device_count() < 1:
        pytest.fail("no GPU visible to libmlffpcg.so")
    return sgdml_amd


def _solver(sg, p, source, lam, rank=0, world=1, key=None):
    """A context with the case's K (S = sigma_K K) from the given column source."""
    s = sg.KernelSolver(p.N, device=0, rank=rank, world=world, comm_id=key if world > 1 else None)
    try:
        r0, r1 = s.row_range()
        if source == "host":
            s.set_matrix(np.ascontiguousarray(p.sigma_K * p.S64[r0:r1]))
        elif source in ("points", "rows"):
            s.gen_rbf(p.X, ps.LENGTH_SCALE, ps.JITTER)
            if source == "rows":       # forms the dense rows: the column source becomes the gather
                s.get_matrix_rows()
        elif source in ("matfree", "assembled"):
            Rd, Rdd = p.mol.desc
            (s.sgdml_operator if source == "matfree" else s.assemble_sgdml)(Rd, Rdd, p.mol.perms, ps.SIG)
        else:
            raise KeyError(source)
        s.set_operator(p.sigma_K, lam)
    except BaseException:
        s.close()
        raise
    return s


def _built(s, build):
    """`build(s)` on an open solver; the context is closed if the build raises."""
    try:
        build(s)
    except BaseException:
        s.close()
        raise
    return s


def _ids(rows):
    return [f"{ps.label(inp, k)}-{src}" for inp, k, src in rows]


def _persist_rows(build):
    """TABLE rows of a build x MLFF_PIVCHOL_PERSIST: unset, and 1 / 0 where the speculation
    threshold lies (precon_shapes.PERSIST)."""
    out = []
    for inp, k, src in ps.rows(build):
        for persist in ((None, "1", "0") if (inp, k) in ps.PERSIST and src == "host" else (None,)):
            out.append((inp, k, src, persist))
    return out


def _persist_ids(rows):
    return [f"{ps.label(inp, k)}-{src}" + ("" if e is None else f"-persist{e}") for inp, k, src, e in rows]


def _set_persist(monkeypatch, persist):
    if persist is None:
        monkeypatch.delenv("MLFF_PIVCHOL_PERSIST", raising=False)
    else:
        monkeypatch.setenv("MLFF_PIVCHOL_PERSIST", persist)


def _apply_forms(monkeypatch, make, build, p, lam, tag, which="rand"):
    """Build with `make(s)` under MLFF_LR_ROWS = 0 and 1: kind, k and the apply form, the
    projector T^T T (the panel does not depend on the apply form: same bits), z for three r."""
    panels = []
    for form in (0, 1):
        monkeypatch.setenv("MLFF_LR_ROWS", str(form))
        with make() as s:
            assert s.precon_info() == (KIND[build], p.k)
            assert s.precon_apply_traffic()[0] == form
            panels.append(s.precon_panel())
            z = np.stack([s.precon_apply(r) for r in p.vectors])
        assert panels[-1].shape == (p.k, p.N)
        ps.check_z(z, p, build, lam, which, f"{tag} form {form}")
    assert np.array_equal(panels[0], panels[1])
    held(ps._gram(panels[0]), p.ref(build, lam, which)["proj"], p.band(build, lam, "proj", which),
         f"{tag} T^T T")


# ---------------------------------------------------------------- pivoted Cholesky
PIVL = _persist_rows("pivL")


@pytest.mark.parametrize("inp,k,source,persist", PIVL, ids=_persist_ids(PIVL))
def test_pivoted_cholesky_factor(sg, monkeypatch, inp, k, source, persist):
    """build_woodbury = False: the pivots (first maximum: index 0 on the RBF kernel's all-equal
    diagonal) and L L^T.  At k = N that is S itself."""
    p = ps.problem(inp, k)
    piv_ref, gap, smallest = p.pivots
    print(f"precon-sweep {p.label} pivots: smallest gap={gap:.3e} smallest pivot={smallest:.3e}")
    _set_persist(monkeypatch, persist)
    with _solver(sg, p, source, LAMS[1]) as s:
        piv, _ = s.precon_pivchol(k, build_woodbury=False)
        Lt = s.precon_panel()
    assert Lt.shape == (k, p.N)
    assert sorted(piv) == list(range(p.N))
    assert np.array_equal(piv[:k], piv_ref), (piv[:k], piv_ref)
    if p.kind == "rbf":
        assert piv[0] == 0
    Lt = Lt.astype(LD)
    held(Lt.T @ Lt, p.ref("pivL", LAMS[1])["LLt"], p.band("pivL", LAMS[1], "LLt"), f"{p.label}/{source} L L^T")


WOOD = _persist_rows("wood")


@pytest.mark.parametrize("lam", LAMS, ids=LAM_IDS)
@pytest.mark.parametrize("inp,k,source,persist", WOOD, ids=_persist_ids(WOOD))
def test_pivchol_woodbury(sg, monkeypatch, inp, k, source, persist, lam):
    p = ps.problem(inp, k)
    _set_persist(monkeypatch, persist)

    def build(s):
        piv, _ = s.precon_pivchol(k)
        assert np.array_equal(piv[:k], p.pivots[0])

    def make():
        return _built(_solver(sg, p, source, lam), build)

    _apply_forms(monkeypatch, make, "wood", p, lam, f"{p.label}/{source} {ps.lam_id(lam)} woodbury")


LOWRANK = [r for r in ps.rows("lowrank") if r[2] in ("host", "matfree")]


@pytest.mark.parametrize("lam", LAMS, ids=LAM_IDS)
@pytest.mark.parametrize("inp,k,source", LOWRANK, ids=_ids(LOWRANK))
def test_precon_lowrank(sg, monkeypatch, inp, k, source, lam):
    """Woodbury on a given factor: the float64 rounding of the reference's long-double L."""
    p = ps.problem(inp, k)
    Lt = np.ascontiguousarray(p.factor_ref().astype(np.float64).T)

    def make():
        return _built(_solver(sg, p, source, lam), lambda s: s.precon_lowrank(Lt))

    _apply_forms(monkeypatch, make, "lowrank", p, lam, f"{p.label}/{source} {ps.lam_id(lam)} lowrank")


# ---------------------------------------------------------------- Nystrom, leverage scores
def _index_rows(build):
    return [(inp, k, src, w) for inp, k, src in ps.rows(build)
            for w in (ps.INDEX_SETS.get((inp, k), ("rand",)) if src == "host" else ("rand",))]


NYS = [r + (v,) for v in (0, 1) for r in _index_rows(f"nys{v}")]
NYS_IDS = [f"{ps.label(inp, k)}-{src}-{w}-variant{v}" for inp, k, src, w, v in NYS]


@pytest.mark.parametrize("lam", LAMS, ids=LAM_IDS)
@pytest.mark.parametrize("inp,k,source,which,variant", NYS, ids=NYS_IDS)
def test_nystrom(sg, monkeypatch, inp, k, source, which, variant, lam):
    build = f"nys{variant}"
    p = ps.problem(inp, k)
    idx = p.idx(which)

    def make():
        return _built(_solver(sg, p, source, lam), lambda s: s.precon_nystrom(idx, variant=variant))

    _apply_forms(monkeypatch, make, build, p, lam,
                 f"{p.label}/{source}/{which} {ps.lam_id(lam)} nystrom{variant}", which)


LEV = _index_rows("lev")


@pytest.mark.parametrize("lam", LAMS, ids=LAM_IDS)
@pytest.mark.parametrize("inp,k,source,which", LEV,
                         ids=[f"{ps.label(inp, k)}-{src}-{w}" for inp, k, src, w in LEV])
def test_lev_scores(sg, inp, k, source, which, lam):
    p = ps.problem(inp, k)
    with _solver(sg, p, source, lam) as s:
        got = s.lev_scores(p.idx(which), lam)
    held(got, p.ref("lev", lam, which)["scores"], p.band("lev", lam, "scores", which),
         f"{p.label}/{source}/{which} {ps.lam_id(lam)} lev_scores")


# ---------------------------------------------------------------- eigen build
def _check_eig(p, unique, lam, ev, rl, T, z, tag):
    ref = p.ref("eig", lam)
    # relative to |l_1|: the trailing eigenvalues are held absolutely
    held(ev, ref["evals"], p.band("eig", lam, "evals"), f"{tag} evals")
    if unique:
        held(rl, ref["rowlev"], p.band("eig", lam, "rowlev"), f"{tag} rowlev")
        held(ps._gram(T), ref["proj"], p.band("eig", lam, "proj"), f"{tag} T^T T")
    ps.check_z(z, p, "eig", lam, "rand", tag)


@pytest.mark.parametrize("lam", LAMS, ids=LAM_IDS)
@pytest.mark.parametrize("inp,k,source,mask,unique", [r[:5] for r in ps.EIG_TABLE],
                         ids=[f"{ps.label(r[0], r[1])}-{r[2]}-mask{r[3]}" for r in ps.EIG_TABLE])
def test_eig(sg, monkeypatch, inp, k, source, mask, unique, lam):
    p = ps.problem(inp, k, mask)
    tag = f"{p.label}/{source} {ps.lam_id(lam)} eig"
    b = k + max(16, k // 2)
    sp = p.spectrum_abs
    print(f"precon-sweep {tag}: full={2 * b >= p.N} b={b} |l_k|/|l_1|={sp[k - 1] / sp[0]:.3e}")
    for form in (0, 1):
        monkeypatch.setenv("MLFF_LR_ROWS", str(form))
        with _solver(sg, p, source, lam) as s:
            ev, rl = s.precon_eig(k, mask_mode=mask, dim_i=p.mol.n3 if mask == 2 else 0,
                                  want_evals=True, want_rowlev=True)
            assert s.eig_info()[0] is True, s.eig_info()
            assert s.precon_info() == (KIND["eig"], k)
            assert s.precon_apply_traffic()[0] == form
            T = s.precon_panel()
            z = np.stack([s.precon_apply(r) for r in p.vectors])
        _check_eig(p, unique and form == 0, lam, ev, rl, T, z, f"{tag} form {form}")


# ---------------------------------------------------------------- spectrum
SPEC = [r for r in ps.rows("spectrum") if r[2] == "host"]


@pytest.mark.parametrize("lam", LAMS, ids=LAM_IDS)
@pytest.mark.parametrize("inp,k,source", SPEC, ids=_ids(SPEC))
def test_spectrum(sg, inp, k, source, lam):
    """All N eigenvalues of P A (pivoted Cholesky + Woodbury) and of A itself."""
    p = ps.problem(inp, k)
    with _solver(sg, p, source, lam) as s:
        s.precon_pivchol(k)
        with_p = s.spectrum(True)
        without = s.spectrum(False)
    tag = f"{p.label}/{source} {ps.lam_id(lam)} spectrum"
    held(with_p, p.ref("spectrum", lam)["spectrum_P"], p.band("spectrum", lam, "spectrum_P"), f"{tag} P A")
    held(without, p.ref("spectrum", lam)["spectrum_A"], p.band("spectrum", lam, "spectrum_A"), f"{tag} A")


# ---------------------------------------------------------------- ranks
def _sharded_params():
    eig = {(r[0], r[1]): r[4] for r in ps.EIG_TABLE if r[3] == 0}
    out = []
    for inp, k, worlds in ps.SHARDED:
        builds = [b for i, kk, bs, _, _ in ps.TABLE if (i, kk) == (inp, k)
                  for b in ("wood", "nys0", "lev") if b in bs]
        builds += ["eig"] if (inp, k) in eig else []
        out += [(inp, k, w, b) for w in worlds for b in builds]
    return out


SHARDED = _sharded_params()


@pytest.mark.parametrize("lam", LAMS, ids=LAM_IDS)
@pytest.mark.parametrize("inp,k,world,build", SHARDED,
                         ids=[f"{ps.label(i, k)}-W{w}-{b}" for i, k, w, b in SHARDED])
def test_sharded(sg, inp, k, world, build, lam):
    """Row blocks of ceil(N / W) rows (ragged, and ranks without rows): the panel columns and z
    gathered by row_range() and held to the long-double reference, not to the one-rank run."""
    from tests.test_gpu_multirank import run_ranks

    p = ps.problem(inp, k)
    source = "points" if p.kind == "rbf" and world % 2 else "host"
    unique = {(r[0], r[1]): r[4] for r in ps.EIG_TABLE}.get((inp, k), False)
    idx = p.idx()

    def body(rank, w, key):
        with _solver(sg, p, source, lam, rank, w, key) as s:
            r0, r1 = s.row_range()
            if build == "lev":
                return r0, r1, s.lev_scores(idx, lam)
            extra = None
            if build == "wood":
                piv, _ = s.precon_pivchol(k)
                extra = piv[:k]
            elif build == "nys0":
                s.precon_nystrom(idx, variant=0)
            else:
                extra = s.precon_eig(k, want_evals=True, want_rowlev=True) + (s.eig_info()[0],)
            assert s.precon_info() == (KIND[build], k)
            T = s.precon_panel()
            z = np.stack([s.precon_apply(np.ascontiguousarray(r[r0:r1])) for r in p.vectors])
            return r0, r1, T, z, extra

    outs = run_ranks(world, body, timeout=120)
    tag = f"{p.label}/{source} {ps.lam_id(lam)} {build} world={world}"
    assert [o[0] for o in outs[1:]] == [o[1] for o in outs[:-1]] and outs[-1][1] == p.N
    if build == "lev":
        for o in outs:
            held(o[2], p.ref("lev", lam)["scores"], p.band("lev", lam, "scores"), tag)
        return
    T = np.concatenate([o[2] for o in outs], axis=1)
    z = np.concatenate([o[3] for o in outs], axis=1)
    if build == "eig":
        for o in outs:
            ev, rl, conv = o[4]
            assert conv is True
            held(ev, p.ref("eig", lam)["evals"], p.band("eig", lam, "evals"), f"{tag} evals")
            if unique:
                held(rl, p.ref("eig", lam)["rowlev"], p.band("eig", lam, "rowlev"), f"{tag} rowlev")
    if build == "wood":
        for o in outs:
            assert np.array_equal(o[4], p.pivots[0])
    if build != "eig" or unique:
        held(ps._gram(T), p.ref(build, lam)["proj"], p.band(build, lam, "proj"), f"{tag} T^T T")
    ps.check_z(z, p, build, lam, "rand", tag)
