"""Every sGDML kernel against the long-double oracle, over the molecule sizes at which the
kernels change branch (tests/sgdml_shapes.py: the table, the references, the bands, `held`).

Inputs to the GPU are the float64 roundings of the long-double descriptors (for the descriptor
and the prediction tests: the geometries).  Bound everywhere: 10 x the spread of the oracle's own
float64 evaluations around its long-double run, floored at 2^-52.  Every test prints the deviation,
the bound and their ratio before it asserts; profiles/shape_sweep/README.txt holds the measured
ratios.
"""
import numpy as np
import pytest

from tests import sgdml_shapes as sh
from tests.sgdml_shapes import LAM, LD, SIG, held

pytestmark = pytest.mark.gpu

CASE_IDS = [sh.case_id(c) for c in sh.CASES]
PT_MAX_ATOMS = 24          # csrc/kernels_pt.hip kPtVariants: D <= 288
PT_CAPACITY = [36, 72, 112, 224, 288]  # L x DL
PRED_TILE_MAX_D = 288


@pytest.fixture(scope="module")
def sg():
    import sgdml_amd

    if sgdml_amd.device_count() < 1:
        pytest.fail("no GPU visible to libmlffpcg.so")
    return sgdml_amd


@pytest.fixture(params=sh.CASES, ids=CASE_IDS)
def c(request):
    return sh.case(*request.param)


def _operator_ref(c, E=False):
    """(-K_op + lam I) x in long double."""
    x = (c.xE if E else c.x).astype(LD)
    return -c.ref("KopE" if E else "Kop") + LD(LAM) * x


# ---------------------------------------------------------------- descriptors
def _check_descriptors(sg, R, ref_ld, label):
    bands, scales = sh.descriptor_bands(R, ref_ld)
    for got, ref, b, sc, name in zip(sg.sgdml_descriptors(R), ref_ld, bands, scales,
                                     ("R_desc", "R_d_desc")):
        held(got, ref, b, f"{label} {name}", scale=sc)


def test_descriptors(sg, c):
    _check_descriptors(sg, c.R, c.desc_ld, c.label)


def test_descriptors_grid_stride(sg):
    """n = 190, M = 2: D = 17955 > 64 * 256, the grid-stride step of k_desc."""
    from oracle.sgdml import descriptors

    n, M = sh.GRID_STRIDE_DESC
    R = sh.molecule(n, M, 1000 * n + M)
    _check_descriptors(sg, R, descriptors(R.astype(LD), dtype=LD), f"n{n}-M{M}")


# ---------------------------------------------------------------- assembly
@pytest.mark.parametrize("E", [False, True], ids=["noE", "E"])
def test_assembly(sg, c, E):
    Rd, Rdd = c.desc
    N = c.N + (c.M if E else 0)
    with sg.KernelSolver(N) as s:
        s.assemble_sgdml(Rd, Rdd, c.perms, SIG, use_E_cstr=E)
        K = s.get_matrix_rows()
    q = "KE" if E else "K"
    held(K, c.ref(q), c.band(q), f"{c.label} {q}")
    # exactly symmetric -- where the reference's K is symmetric at all: for the set that is not
    # closed under inversion its diagonal blocks (stored transposed, train.py:172-210) differ
    # from their transposes by 5 % of max|K|, and the assembly follows them (held above)
    Ks = K.copy()
    if not c.group:
        assert not np.allclose(c.ref(q), c.ref(q).T, rtol=0, atol=1e-3 * float(np.max(np.abs(c.ref("K")))))
        for i in range(c.M):
            Ks[i * c.n3:(i + 1) * c.n3, i * c.n3:(i + 1) * c.n3] = 0.0
    assert np.array_equal(Ks, Ks.T), "assembled K is not exactly symmetric"
    if E:
        n = c.N
        # the energy-energy entries are O(1), the force block O(1 / sig^2): each block against
        # its own maximum
        for name, cut in (("K_ff", lambda a: a[:n, :n]), ("K_fe", lambda a: a[:n, n:]),
                          ("K_ee", lambda a: a[n:, n:])):
            held(cut(K), cut(c.ref(q)), c.band(q, cut), f"{c.label} {name}")


# ---------------------------------------------------------------- operator
def _matvec(sg, c, want_form, E=False):
    Rd, Rdd = c.desc
    N = c.N + (c.M if E else 0)
    with sg.KernelSolver(N) as s:
        s.sgdml_operator(Rd, Rdd, c.perms, SIG, use_E_cstr=E)
        s.set_operator(-1.0, LAM)
        assert s.storage_info()[0] == "matfree"
        assert s.operator_form() == want_form, (s.operator_form(), want_form)
        return s.matvec(c.xE if E else c.x)


@pytest.mark.parametrize("form", ["pair", "rec", "pt"])
def test_operator(sg, c, form, monkeypatch):
    monkeypatch.setenv("MLFF_MF_FORM", form)
    for v in ("MLFF_PT_VARIANT", "MLFF_PT_CHUNKS", "MLFF_REC_RG", "MLFF_MF_REC"):
        monkeypatch.delenv(v, raising=False)
    # the one exception: no pair-tile form past 24 atoms, the request falls to the record form
    want = "rec" if form == "pt" and c.n > PT_MAX_ATOMS else form
    ref, b = _operator_ref(c), c.band("Kop")
    held(_matvec(sg, c, want), ref, b, f"{c.label} Kop/{form}")
    if want == "pt":
        for i, cap in enumerate(PT_CAPACITY):
            if c.D <= cap:
                monkeypatch.setenv("MLFF_PT_VARIANT", str(i))
                held(_matvec(sg, c, want), ref, b, f"{c.label} Kop/pt variant {i}")
        monkeypatch.delenv("MLFF_PT_VARIANT")
        monkeypatch.setenv("MLFF_PT_CHUNKS", "1")
        held(_matvec(sg, c, want), ref, b, f"{c.label} Kop/pt one chunk")
    if form == "rec":
        for rg in ("4", "8", "16"):
            monkeypatch.setenv("MLFF_REC_RG", rg)
            held(_matvec(sg, c, want), ref, b, f"{c.label} Kop/rec RG={rg}")


def test_operator_energy_constraints(sg, c, monkeypatch):
    """Only the pair form exists with the energy border."""
    monkeypatch.delenv("MLFF_MF_FORM", raising=False)
    y = _matvec(sg, c, "pair", E=True)
    ref, n = _operator_ref(c, E=True), c.N
    held(y, ref, c.band("KopE"), f"{c.label} KopE")
    # the energy rows are O(1), the force rows O(1 / sig^2): each against its own maximum
    for name, cut in (("force rows", lambda a: a[:n]), ("energy rows", lambda a: a[n:])):
        held(cut(y), cut(ref), c.band("KopE", cut), f"{c.label} KopE {name}")


@pytest.mark.parametrize("world", [4, 7])
@pytest.mark.parametrize("key", [(4, 33, "s3"), (22, 3, "c3"), (43, 2, "nongroup")],
                         ids=sh.case_id)
def test_operator_sharded(sg, key, world, monkeypatch):
    """Row blocks that end inside a point and inside an atom's three rows."""
    from tests.test_gpu_multirank import run_ranks

    c = sh.case(*key)
    Rd, Rdd = c.desc
    assert (-(-c.N // world)) % c.n3 != 0                   # a block ends inside a point
    if world == 7 and c.n > 4:
        assert (-(-c.N // world)) % 3 != 0                  # and inside an atom's three rows
    default = "pt" if c.n <= PT_MAX_ATOMS else "rec"
    ref, b = _operator_ref(c), c.band("Kop")
    for form in [None] + (["rec"] if default == "pt" else []):
        if form is None:
            monkeypatch.delenv("MLFF_MF_FORM", raising=False)
        else:
            monkeypatch.setenv("MLFF_MF_FORM", form)
        want = form or default

        def body(rank, w, comm):
            with sg.KernelSolver(c.N, device=0, rank=rank, world=w, comm_id=comm) as s:
                s.sgdml_operator(Rd, Rdd, c.perms, SIG)
                s.set_operator(-1.0, LAM)
                if s.nrows > 0:
                    assert s.operator_form() == want, (s.operator_form(), want)
                return s.matvec(c.x)

        y = np.concatenate(run_ranks(world, body, timeout=120))
        held(y, ref, b, f"{c.label} Kop/{want} world={world}")


# ---------------------------------------------------------------- diagonal, energies
@pytest.mark.parametrize("E", [False, True], ids=["noE", "E"])
def test_diag(sg, c, E):
    Rd, Rdd = c.desc
    N = c.N + (c.M if E else 0)
    q = "diagE" if E else "diag"
    with sg.KernelSolver(N) as s:
        s.sgdml_operator(Rd, Rdd, c.perms, SIG, use_E_cstr=E)
        s.set_operator(-1.0, LAM)
        d_mf = s.diag()
    with sg.KernelSolver(N) as s:
        s.assemble_sgdml(Rd, Rdd, c.perms, SIG, use_E_cstr=E)
        s.set_operator(-1.0, LAM)
        d_asm = s.diag()
    held(d_mf, -c.ref(q), c.band(q), f"{c.label} {q}/matfree")
    qa = q if c.group else ("diagKE" if E else "diagK")
    held(d_asm, -c.ref(qa), c.band(qa), f"{c.label} {qa}/assembled")


def test_energies(sg, c):
    Rd, Rdd = c.desc
    with sg.KernelSolver(c.N) as s:
        s.sgdml_operator(Rd, Rdd, c.perms, SIG)
        i0, E = s.sgdml_energies(c.x)
    assert i0 == 0
    held(E, c.ref("E"), c.band("E"), f"{c.label} E")


# ---------------------------------------------------------------- single columns
def test_columns(sg, c):
    """Pivoted Cholesky with columns K_op e_g from the single-column kernel.  Geometry seed:
    1000 n + M (sgdml_shapes.SEEDS lists the exceptions); with it the pivot of each of the k steps
    is more than 1e-9 (relative) above the runner-up, so the pivot order is not a rounding matter.
    Two and three atoms: rows of one point and coordinate tie exactly (Case.tie_class), so the
    pivots are compared as classes and the panel through T^T T = L L^T, the same for either."""
    Rd, Rdd = c.desc
    k = c.k_piv
    L, piv_ref, b, gap = c.pivchol
    print(f"shape-sweep {c.label} pivots: k={k} seed={c.seed} smallest gap={gap:.3e}")
    assert gap > sh.PIVOT_GAP
    with sg.KernelSolver(c.N) as s:
        s.sgdml_operator(Rd, Rdd, c.perms, SIG)
        s.set_operator(-1.0, LAM)
        piv, _ = s.precon_pivchol(k, build_woodbury=False)
        T = s.precon_panel()
    assert T.shape == (k, c.N)
    assert np.array_equal(c.tie_class(piv[:k]), c.tie_class(piv_ref[:k])), (piv[:k], piv_ref[:k])
    if c.ties:
        held(T.T.astype(LD) @ T.astype(LD), L, b, f"{c.label} panel T^T T")
    else:
        held(T, L.T, b, f"{c.label} panel")
    # first panel row x sqrt(pivot) is the pivot column of -K_op (lam e_g goes to the column's
    # own entry g, which the factorisation replaces by the diagonal's: without lam)
    g = int(piv[0])
    col = -c.column(g, LD)
    bcol = max(sh.FLOOR, sh._rel(-c.column(g, np.float64), col))
    held(T[0] * T[0, g], col, bcol, f"{c.label} pivot column {g}")


# ---------------------------------------------------------------- prediction
def test_prediction_at_training_points(sg, c, monkeypatch):
    """K_op alphas and the training-set energies through GDMLPredict (std = 1, c = 0) at the
    training geometries, alphas = the case's x."""
    from sgdml_amd.model import r_d_desc_alpha

    Rd, Rdd = c.desc
    model = {"type": "m", "z": np.ones(c.n, dtype=np.int64), "perms": c.perms, "sig": SIG,
             "std": 1.0, "c": 0.0, "R_desc": Rd.T, "R_d_desc_alpha": r_d_desc_alpha(Rdd, c.x)}
    default = "tile" if c.D <= PRED_TILE_MAX_D else "stream"
    F_ref, E_ref = c.ref("Kop").reshape(c.M, c.n3), c.ref("E")
    for form in [None] + (["stream"] if default == "tile" else []):
        if form is None:
            monkeypatch.delenv("MLFF_PRED_FORM", raising=False)
        else:
            monkeypatch.setenv("MLFF_PRED_FORM", form)
        with sg.GDMLPredict(model, device=0) as gd:
            assert gd.form == (form or default)
            E, F = gd.predict(c.R)
        held(F, F_ref, c.band("Kop"), f"{c.label} predict F/{gd.form}")
        if np.max(np.abs(E_ref)) > 0:
            held(E, E_ref, c.band("E"), f"{c.label} predict E/{gd.form}")
        else:
            # one training point, identity: diff = 0 and E = 0 exactly in the oracle, whose
            # query descriptors are the model's.  The predictor forms them from R, up to
            # 10 desc_band from R_desc per entry (test_descriptors), so
            # |E| = |sum_d diff_d z_d| 5 / (3 sig^2) <= 10 desc_band sum_d |R_desc_d z_d| 5 / (3 sig^2)
            z = model["R_d_desc_alpha"]
            scale = float(np.sum(np.abs(Rd * z))) * 5.0 / (3.0 * SIG ** 2)
            held(E, E_ref, c.desc_band[0], f"{c.label} predict E/{gd.form} (zero reference)",
                 scale=scale)
