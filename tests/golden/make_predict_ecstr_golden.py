"""Generate tests/golden/sgdml_predict_ecstr_cases.npz by running the REFERENCE's predictor on
energy-constrained models (alphas_E: predict.py:206-218, 364-368).

Run where the reference checkout is available (never on the GPU box):

    python tests/golden/make_predict_ecstr_golden.py --ref /path/to/reference   (or MLFF_REFERENCE)

The reference (bluecher31/mlff-preconditioner) is imported at run time, as make_predict_golden.py
and make_analytic_golden.py do (np.int / np.float / np.bool aliases, GDMLPredict.prepare_parallel
stubbed).  Only arrays are written (npz, allow_pickle=False); nothing of the reference is copied.

Group 1 (`cases`): the models d3, d21, eth3, eth3ng, eth and tube of
make_predict_golden.cases() -- the same geometries, alphas_F, std, c and queries, which the
consumer reads from sgdml_predict_cases.npz (this script asserts that file holds exactly them)
-- each with alphas_E = s * N(0, 1) (seed 1618 + index), through create_model(...,
alphas_E=...) with use_E_cstr.  Per case <c>:
  <c>__alphas_E, <c>__s        the energy coefficients and their scale
  <c>__E, <c>__F               GDMLPredict.predict(R) of the reference
  <c>__band_F, <c>__band_E     the reference's own spread: as is / chunk_size = 1 / training
                               points (and alphas_E) reversed, as make_predict_golden.py
  <c>__share                   the four shares below
0 < band < 1e-9 is asserted.  Both coefficient sets have to show in both outputs, or a predictor
that drops a term would pass: with (E0, F0) the prediction of the same model without alphas_E,
  share = [max|F - F0| / max|F|, max|F0| / max|F|, max|E - E0| / max|E - c|, max|E0 - c| / max|E - c|]
and s is the power of ten in 1e0 .. 1e6 with the largest min(share); min(share) >= 1e-3 is
asserted.

Group 2 (`trained`): eth_ecstr and ethp_ecstr of make_analytic_golden.py (its make_task,
variants and queries; synthetic.ethanol_harmonic(23, seed=13)), trained by the reference's
closed-form solver.  Per case <c>:
  <c>__Rq                      12 query geometries (seed 400 + the case's index there), the first
                               two undisplaced training geometries
  <c>__Eq, <c>__Fq             GDMLPredict.predict(Rq) with the reference's model
  <c>__band_F, <c>__band_E     spread over the four training variants (reversed order, LU path,
                               two perturbed K), as that generator's unconstrained cases
0 < band < 1e-5 is asserted (that generator's condition).
"""
from __future__ import annotations

import argparse
import os
import sys
from pathlib import Path

sys.dont_write_bytecode = True
HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent
sys.path[:0] = [str(REPO / "mlff-preconditioner_amd"), str(HERE)]

import numpy as np  # noqa: E402

import make_analytic_golden as mag  # noqa: E402  (also sets the np.int / np.float / np.bool aliases)
import make_predict_golden as mpg  # noqa: E402

from sgdml_amd import synthetic  # noqa: E402  (input generation only)

RANDOM_CASES = ["d3", "d21", "eth3", "eth3ng", "eth", "tube"]
TRAINED_CASES = {"eth_ecstr": (np.arange(9)[None, :], 402), "ethp_ecstr": (mag.PERMS_P, 403)}
SCALES = [10.0 ** k for k in range(7)]


def reference_model(train, Desc, case, alphas_E):
    """create_model of the reference for a case of make_predict_golden.cases(); alphas_E None:
    the unconstrained model."""
    R_train, perms = case["R_train"], case["perms"]
    M, n = R_train.shape[:2]
    desc = Desc(n, interact_cut_off=None, max_processes=1)
    tril = np.array([desc.perm(p) for p in perms])
    tpl = (tril + np.arange(perms.shape[0])[:, None] * desc.dim).flatten("F")
    R_desc, R_d_desc = desc.from_R(R_train.reshape(M, -1), lat_and_inv=None, callback=None)
    task = {
        "dataset_name": np.array("synthetic"), "dataset_theory": np.array("synthetic"),
        "z": case["z"], "idxs_train": np.arange(M), "md5_train": "0", "idxs_valid": np.arange(0),
        "md5_valid": "0", "sig": mpg.SIG, "lam": 1e-10, "use_E": True,
        "use_E_cstr": alphas_E is not None, "use_sym": perms.shape[0] > 1, "use_cprsn": False,
        "solver_tol": 1e-4, "n_inducing_pts_init": 25, "interact_cut_off": None, "perms": perms,
    }
    model = train.create_model(task, "analytic", R_desc, R_d_desc, tpl, float(case["std"]),
                               case["alphas_F"], alphas_E=alphas_E)
    model["c"] = float(case["c"])
    assert ("alphas_E" in model) == (alphas_E is not None)
    return model


def reference_predict(GDMLPredict, train, Desc, case, alphas_E):
    """E, F of the reference, its spread over the three runs, and the shares of the two
    coefficient sets."""
    model = reference_model(train, Desc, case, alphas_E)
    R = case["R"].reshape(case["R"].shape[0], -1)
    runs = []
    gd = GDMLPredict(model, max_processes=1)
    runs.append(gd.predict(R))
    gd._set_chunk_size(1)
    runs.append(gd.predict(R))
    rev = dict(model, R_desc=np.ascontiguousarray(model["R_desc"][:, ::-1]),
               R_d_desc_alpha=np.ascontiguousarray(model["R_d_desc_alpha"][::-1]),
               alphas_E=np.ascontiguousarray(alphas_E[::-1]))
    runs.append(GDMLPredict(rev, max_processes=1).predict(R))
    E, F = (np.array(a) for a in runs[0])
    c = float(case["c"])
    mF, mE = np.max(np.abs(F)), np.max(np.abs(E - c))
    band_F = max(np.max(np.abs(np.asarray(f) - F)) for _, f in runs[1:]) / mF
    band_E = max(np.max(np.abs(np.asarray(e) - E)) for e, _ in runs[1:]) / mE
    E0, F0 = GDMLPredict(reference_model(train, Desc, case, None), max_processes=1).predict(R)
    share = np.array([np.max(np.abs(F - F0)) / mF, np.max(np.abs(F0)) / mF,
                      np.max(np.abs(E - E0)) / mE, np.max(np.abs(E0 - c)) / mE])
    return E, F, band_F, band_E, share


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("MLFF_REFERENCE"),
                    help="checkout of the reference (bluecher31/mlff-preconditioner)")
    a = ap.parse_args()
    if not a.ref:
        ap.error("--ref (or MLFF_REFERENCE) is required")
    GDMLPredict, GDMLTrain, analytic = mag.import_reference(Path(a.ref))
    from sgdml.utils.desc import Desc

    train = mag.trainer(GDMLTrain)
    out = {"cases": np.array(RANDOM_CASES), "trained": np.array(sorted(TRAINED_CASES))}

    # group 1: the models of sgdml_predict_cases.npz with random energy coefficients
    stored = np.load(HERE / "sgdml_predict_cases.npz", allow_pickle=False)
    all_cases = mpg.cases()
    for idx, name in enumerate(RANDOM_CASES):
        case = all_cases[name]
        for key, val in case.items():
            assert np.array_equal(stored[f"{name}__{key}"], val), (name, key)
        M = case["R_train"].shape[0]
        unit = np.random.default_rng(1618 + idx).standard_normal(M)
        best = None
        for s in SCALES:
            res = reference_predict(GDMLPredict, train, Desc, case, s * unit)
            print(f"  {name} s={s:g} share F: aE {res[4][0]:.2e} aF {res[4][1]:.2e}   "
                  f"E: aE {res[4][2]:.2e} aF {res[4][3]:.2e}", flush=True)
            if best is None or res[4].min() > best[1][4].min():
                best = (s, res)
        s, (E, F, band_F, band_E, share) = best
        print(f"{name}: M={M} s={s:g} band_F={band_F:.3e} band_E={band_E:.3e} "
              f"min share={share.min():.3e} max|F|={np.max(np.abs(F)):.3e} "
              f"max|E-c|={np.max(np.abs(E - case['c'])):.3e}", flush=True)
        assert 0 < band_F < 1e-9 and 0 < band_E < 1e-9, (name, band_F, band_E)
        assert share.min() >= 1e-3, (name, share)
        pre = f"{name}__"
        out.update({pre + "alphas_E": s * unit, pre + "s": np.float64(s), pre + "E": E, pre + "F": F,
                    pre + "band_F": np.float64(band_F), pre + "band_E": np.float64(band_E),
                    pre + "share": share})

    # group 2: the reference's own energy-constrained models
    ds = synthetic.ethanol_harmonic(23, seed=13)
    for name, (perms, seed) in TRAINED_CASES.items():
        task = mag.make_task(ds, perms, True)
        runs = mag.variants(GDMLTrain, analytic, task)
        assert all("alphas_E" in m for m, _ in runs)
        c = float(runs[0][0]["c"])
        Rq = mag.queries(ds["R"], 12, seed, 2)
        pred = [GDMLPredict(m, max_processes=1).predict(Rq.reshape(12, -1)) for m, _ in runs]
        E, F = (np.array(x) for x in pred[0])
        band_F = max(np.max(np.abs(np.asarray(f) - F)) for _, f in pred[1:]) / np.max(np.abs(F))
        band_E = max(np.max(np.abs(np.asarray(e) - E)) for e, _ in pred[1:]) / np.max(np.abs(E - c))
        print(f"{name}: band_F={band_F:.3e} band_E={band_E:.3e} max|F|={np.max(np.abs(F)):.3e} "
              f"max|E-c|={np.max(np.abs(E - c)):.3e}", flush=True)
        assert 0 < band_F < 1e-5 and 0 < band_E < 1e-5, (name, band_F, band_E)
        pre = f"{name}__"
        out.update({pre + "Rq": Rq, pre + "Eq": E, pre + "Fq": F,
                    pre + "band_F": np.float64(band_F), pre + "band_E": np.float64(band_E)})
    path = HERE / "sgdml_predict_ecstr_cases.npz"
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({path.stat().st_size / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
