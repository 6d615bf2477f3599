"""Generate tests/golden/sgdml_analytic_cases.npz by running the REFERENCE's closed-form trainer.

Run where the reference checkout is available (never on the GPU box):

    python tests/golden/make_analytic_golden.py --ref /path/to/reference   (or MLFF_REFERENCE)

The reference (bluecher31/mlff-preconditioner) is imported at run time, as make_golden.py and
make_predict_golden.py do (np.int / np.float / np.bool aliases, GDMLPredict.prepare_parallel
stubbed).  Only arrays are written (npz, allow_pickle=False); nothing of the reference is copied.

Source data: synthetic.ethanol_harmonic(23, seed=13), sig 10, task['lam'] = 1e-15 (the
closed-form solver shifts by 1e-10 whatever it says, analytic.py:136).  Cases

  eth          N = 621   no symmetries            no constraints
  ethp         N = 621   identity + (3 4)          no constraints
  eth_ecstr    N = 644   no symmetries            use_E_cstr
  ethp_ecstr   N = 644   identity + (3 4)          use_E_cstr

Per case <c> the file holds
  <c>__R, __F, __E, __z, __perms, __sig, __lam, __use_E_cstr   the task's arrays
  <c>__model_keys                      sorted keys of GDMLTrain.train(task), solver 'analytic'
  <c>__alphas_F, (__alphas_E), __c, __std                       its coefficients and constants
  <c>__band_rel_dalpha (, __band_c)    the reference's own spread (below)
and for the two unconstrained cases
  <c>__Rq          12 query geometries: the training geometries displaced by N(0, 0.03^2), the
                   first two undisplaced
  <c>__Eq, __Fq    GDMLPredict.predict(Rq) with the reference's model
  <c>__band_F, __band_E
(the reference's and this project's predictors are not run on use_E_cstr models here: this
project's GDMLPredict refuses alphas_E, so no prediction is compared for them).

Bands: the reference is trained again in four variants -- the training points in reversed order;
the LU path (cho_factor made to raise, analytic.py:154-167); the assembled K multiplied
entrywise by 1 + 16 * 2^-53 * S, S symmetric uniform in [-1, 1], seeds 0 and 1 --
  band_F = max |dF| / max |F|,   band_E = max |dE| / max |E - c|,   band_c = max |dc| / |c|,
  band_rel_dalpha = max ||d alpha|| / ||alpha||   over [alphas_F; alphas_E]
(the reversed run's coefficients put back into the original order).  0 < band < 1e-5 is
asserted for every band, so that a bound built on it is neither vacuous nor absurd.
"""
from __future__ import annotations

import argparse
import os
import sys
from pathlib import Path

sys.dont_write_bytecode = True
HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent
sys.path[:0] = [str(REPO / "mlff-preconditioner_amd")]

import numpy as np  # noqa: E402

for _alias, _t in (("int", int), ("float", float), ("bool", bool)):
    if not hasattr(np, _alias):
        setattr(np, _alias, _t)

from sgdml_amd import synthetic  # noqa: E402  (input generation only)

SIG = 10
LAM = 1e-15
PERMS_P = np.array([np.arange(9), [0, 1, 2, 4, 3, 5, 6, 7, 8]])


def noop(*a, **k):
    pass


def import_reference(ref: Path):
    sys.path += [str(ref / "src" / "sGDML"), str(ref / "src")]
    import sgdml.predict
    import sgdml.solvers.analytic as analytic
    import sgdml.train

    sgdml.predict.GDMLPredict.prepare_parallel = lambda self, *a, **k: None
    return sgdml.predict.GDMLPredict, sgdml.train.GDMLTrain, analytic


_TRAIN = None


def trainer(GDMLTrain):
    """The one GDMLTrain instance (the reference refuses a second one)."""
    global _TRAIN
    if _TRAIN is None:
        _TRAIN = GDMLTrain(max_processes=1)
    return _TRAIN


def make_task(ds, perms, use_E_cstr):
    M, n = ds["R"].shape[:2]
    return {
        "type": "t", "dataset_name": np.array("ethanol"), "dataset_theory": np.array("synthetic"),
        "z": ds["z"], "R_train": ds["R"], "F_train": ds["F"], "E_train": ds["E"],
        "idxs_train": np.arange(M), "md5_train": "0", "idxs_valid": np.arange(0),
        "md5_valid": "0", "sig": SIG, "lam": LAM, "use_E": True, "use_E_cstr": use_E_cstr,
        "use_sym": perms.shape[0] > 1, "use_cprsn": False, "solver_name": "analytic",
        "solver_tol": 1e-4, "n_inducing_pts_init": 25, "interact_cut_off": None, "perms": perms,
    }


def queries(R_train, Q, seed, n_exact):
    rng = np.random.default_rng(seed)
    M = R_train.shape[0]
    R = R_train[np.arange(Q) % M] + 0.03 * rng.standard_normal((Q,) + R_train.shape[1:])
    R[:n_exact] = R_train[:n_exact]
    return R


def coefficients(model, reverse=False):
    """[alphas_F; alphas_E] of a model, a reversed-order model's put back in order."""
    M = model["R_desc"].shape[1]
    aF = np.asarray(model["alphas_F"]).reshape(M, -1)
    aE = np.asarray(model["alphas_E"]) if model.get("alphas_E") is not None else np.zeros(0)
    if reverse:
        aF, aE = aF[::-1], aE[::-1]
    return np.concatenate([aF.ravel(), aE.ravel()])


def variants(GDMLTrain, analytic, task):
    """The reference's model and its four variants: (model, reversed?) pairs."""
    out = [(trainer(GDMLTrain).train(task, callback=noop), False)]
    rev = dict(task, R_train=task["R_train"][::-1].copy(), F_train=task["F_train"][::-1].copy(),
               E_train=task["E_train"][::-1].copy())
    out.append((trainer(GDMLTrain).train(rev, callback=noop), True))

    cho = analytic.sp.linalg.cho_factor

    def raising(*a, **k):
        raise np.linalg.LinAlgError("forced: the LU path")

    analytic.sp.linalg.cho_factor = raising
    try:
        out.append((trainer(GDMLTrain).train(task, callback=noop), False))
    finally:
        analytic.sp.linalg.cho_factor = cho
    for seed in (0, 1):
        tr = trainer(GDMLTrain)
        assemble = tr._assemble_kernel_mat

        def perturbed(*a, _assemble=assemble, _seed=seed, **k):
            K = np.array(_assemble(*a, **k))
            S = np.random.default_rng(_seed).uniform(-1.0, 1.0, K.shape)
            S = np.tril(S) + np.tril(S, -1).T
            return K * (1.0 + 16.0 * 2.0 ** -53 * S)

        tr._assemble_kernel_mat = perturbed
        try:
            out.append((tr.train(task, callback=noop), False))
        finally:
            del tr._assemble_kernel_mat  # the instance attribute: the class's method is back
    return out


def check_cholesky_path(GDMLTrain, analytic, task):
    """The plain run factors without the LU fallback: cho_factor returns."""
    calls = []
    cho = analytic.sp.linalg.cho_factor

    def spy(*a, **k):
        r = cho(*a, **k)
        calls.append(1)
        return r

    analytic.sp.linalg.cho_factor = spy
    try:
        trainer(GDMLTrain).train(task, callback=noop)
    finally:
        analytic.sp.linalg.cho_factor = cho
    assert calls == [1], "the reference fell back to LU"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("MLFF_REFERENCE"),
                    help="checkout of the reference (bluecher31/mlff-preconditioner)")
    a = ap.parse_args()
    if not a.ref:
        ap.error("--ref (or MLFF_REFERENCE) is required")
    GDMLPredict, GDMLTrain, analytic = import_reference(Path(a.ref))
    ds = synthetic.ethanol_harmonic(23, seed=13)
    ident = np.arange(9)[None, :]
    cases = {"eth": (ident, False), "ethp": (PERMS_P, False), "eth_ecstr": (ident, True),
             "ethp_ecstr": (PERMS_P, True)}
    out = {"cases": np.array(sorted(cases))}
    for qi, (name, (perms, ecstr)) in enumerate(cases.items()):
        task = make_task(ds, perms, ecstr)
        check_cholesky_path(GDMLTrain, analytic, task)
        runs = variants(GDMLTrain, analytic, task)
        model = runs[0][0]
        assert model["solver_name"] == "analytic" and model["use_E"]
        al = coefficients(model)
        band_da = max(np.linalg.norm(coefficients(m, r) - al) for m, r in runs[1:]) / np.linalg.norm(al)
        bands = {"band_rel_dalpha": band_da}
        pre = f"{name}__"
        out.update({pre + "R": ds["R"], pre + "F": ds["F"], pre + "E": ds["E"], pre + "z": ds["z"],
                    pre + "perms": perms.astype(np.int64), pre + "sig": np.float64(SIG),
                    pre + "lam": np.float64(LAM), pre + "use_E_cstr": np.bool_(ecstr),
                    pre + "model_keys": np.array(sorted(model.keys())),
                    pre + "alphas_F": np.asarray(model["alphas_F"]),
                    pre + "c": np.float64(model["c"]), pre + "std": np.float64(model["std"])})
        if ecstr:
            out[pre + "alphas_E"] = np.asarray(model["alphas_E"])
            assert model["c"] == np.mean(ds["E"])
        else:
            c = float(model["c"])
            bands["band_c"] = max(abs(float(m["c"]) - c) for m, _ in runs[1:]) / abs(c)
            Rq = queries(ds["R"], 12, 400 + qi, 2)
            pred = [GDMLPredict(m, max_processes=1).predict(Rq.reshape(12, -1)) for m, _ in runs]
            E, F = (np.array(x) for x in pred[0])
            bands["band_F"] = max(np.max(np.abs(np.asarray(f) - F)) for _, f in pred[1:]) / np.max(np.abs(F))
            bands["band_E"] = max(np.max(np.abs(np.asarray(e) - E)) for e, _ in pred[1:]) / np.max(np.abs(E - c))
            out.update({pre + "Rq": Rq, pre + "Eq": E, pre + "Fq": F})
        print(name, f"N={al.size}", " ".join(f"{k}={v:.3e}" for k, v in bands.items()), flush=True)
        for k, v in bands.items():
            assert 0 < v < 1e-5, (name, k, v)
            out[pre + k] = np.float64(v)
    path = HERE / "sgdml_analytic_cases.npz"
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({path.stat().st_size / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
