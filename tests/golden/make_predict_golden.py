"""Generate tests/golden/sgdml_predict_cases.npz by running the REFERENCE's predictor.

Run where the reference checkout is available (never on the GPU box):

    python tests/golden/make_predict_golden.py --ref /path/to/reference   (or MLFF_REFERENCE)

The reference (bluecher31/mlff-preconditioner) is imported at run time, with the shims its
older NumPy idioms need (np.int / np.float / np.bool aliases) and
GDMLPredict.prepare_parallel stubbed (it writes a cache file into the package directory,
predict.py:895-925).  Only arrays are written (npz, allow_pickle=False); nothing of the
reference is copied here.

Per case <c> the file holds
  <c>__R_train, <c>__perms, <c>__z, <c>__sig, <c>__alphas_F, <c>__std, <c>__c   the model's sources
  <c>__R                                  the query geometries
  <c>__E, <c>__F                          GDMLPredict.predict(R) of the reference
  <c>__band_F, <c>__band_E                the reference's own spread (below)
The model arrays (R_desc, R_d_desc_alpha) are rebuilt by the consumer from R_train and alphas_F
with the project's host code (host_descriptors, r_d_desc_alpha); this script asserts that they
equal the reference's create_model output bit for bit.

Band: the reference is run three ways -- as is, with chunk_size = 1, and on the same model
with its training points in reversed order (a permutation of the model's data) --
  band_F = max |dF| / max |F|,   band_E = max |dE| / max |E - c|
(the energy band relative to the raw sum: c cancels most of E).  0 < band < 1e-9 is asserted
for every case, so that a bound built on it is neither vacuous nor absurd.
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
from sgdml_amd.model import r_d_desc_alpha, tril_perms_lin  # noqa: E402
from sgdml_amd.solver import host_descriptors  # noqa: E402

SIG = 10


def import_reference(ref: Path):
    sys.path += [str(ref / "src" / "sGDML"), str(ref / "src")]
    import sgdml.predict
    import sgdml.train
    from sgdml.utils.desc import Desc

    sgdml.predict.GDMLPredict.prepare_parallel = lambda self, *a, **k: None
    return sgdml.predict.GDMLPredict, sgdml.train.GDMLTrain(max_processes=1), Desc


def queries(R_train, Q, seed, n_exact=0):
    """Training geometries (cycled) displaced by N(0, 0.03^2); the first n_exact undisplaced."""
    rng = np.random.default_rng(seed)
    M = R_train.shape[0]
    R = R_train[np.arange(Q) % M] + 0.03 * rng.standard_normal((Q,) + R_train.shape[1:])
    R[:n_exact] = R_train[:n_exact]
    return R


def cases():
    g = lambda name: np.load(HERE / f"{name}.npz", allow_pickle=False)  # noqa: E731
    rng = np.random.default_rng(2718)
    out = {}

    def add(name, R_train, z, perms, Q, seed, n_exact=0, alphas=None, std=None, c=None):
        M, n = R_train.shape[:2]
        out[name] = {
            "R_train": np.ascontiguousarray(R_train), "z": np.asarray(z),
            "perms": np.atleast_2d(np.asarray(perms)).astype(np.int64),
            "alphas_F": rng.standard_normal(3 * n * M) if alphas is None else np.asarray(alphas),
            "std": np.float64(rng.uniform(0.5, 2.0) if std is None else std),
            # of the raw sums' size (1e-2 .. 1e-1 for these models), so that the rounding of
            # E = raw std + c does not hide the raw sum's own spread from band_E
            "c": np.float64(rng.uniform(-0.1, 0.1) if c is None else c),
            "R": queries(R_train, Q, seed, n_exact),
        }

    eth = synthetic.ethanol_like
    add("d3", eth(9, seed=31)["R"][:, :3], synthetic.ETHANOL_Z[:3], np.arange(3), 5, 101)
    add("d21", eth(12, seed=32)["R"][:, :7], synthetic.ETHANOL_Z[:7],
        [np.arange(7), [0, 1, 2, 4, 3, 5, 6]], 5, 102)
    m = g("sgdml_model_ethanol_n621")
    add("eth", m["R"], m["z"], m["model__perms"], 70, 103, n_exact=2, alphas=m["model__alphas_F"],
        std=m["model__std"], c=m["model__c"])
    p3 = g("sgdml_ethanol_n270_perms")
    add("eth3", p3["R"], p3["z"], p3["perms"], 70, 104, n_exact=2)
    ng = g("sgdml_ethanol_n270_nongroup")
    add("eth3ng", ng["R"], ng["z"], ng["perms"], 5, 105)
    add("eth_rows", eth(150, seed=33)["R"], synthetic.ETHANOL_Z, np.arange(9), 3, 106)
    tube = synthetic.nanotube_like(3, seed=4)
    add("tube", tube["R"], tube["z"], np.arange(370), 2, 107)
    return out


def reference_predict(GDMLPredict, train, Desc, case):
    R_train, perms = case["R_train"], case["perms"]
    M, n = R_train.shape[:2]
    desc = Desc(n, interact_cut_off=None, max_processes=1)
    tril = np.array([desc.perm(p) for p in perms])
    tpl = (tril + np.arange(perms.shape[0])[:, None] * desc.dim).flatten("F")
    R_desc, R_d_desc = desc.from_R(R_train.reshape(M, -1), lat_and_inv=None, callback=None)
    task = {
        "dataset_name": np.array("synthetic"), "dataset_theory": np.array("synthetic"),
        "z": case["z"], "idxs_train": np.arange(M), "md5_train": "0", "idxs_valid": np.arange(0),
        "md5_valid": "0", "sig": SIG, "lam": 1e-10, "use_E": True, "use_E_cstr": False,
        "use_sym": perms.shape[0] > 1, "use_cprsn": False, "solver_tol": 1e-4,
        "n_inducing_pts_init": 25, "interact_cut_off": None, "perms": perms,
    }
    model = train.create_model(task, "cg", R_desc, R_d_desc, tpl, float(case["std"]),
                               case["alphas_F"])
    model["c"] = float(case["c"])
    # the consumer's rebuild of the model arrays, with the project's host code
    Rd_own, Rdd_own = host_descriptors(R_train)
    assert np.array_equal(Rd_own.T, model["R_desc"]), "host_descriptors != Desc.from_R"
    assert np.array_equal(r_d_desc_alpha(Rdd_own, case["alphas_F"]), model["R_d_desc_alpha"]), \
        "r_d_desc_alpha != create_model"
    assert np.array_equal(tril_perms_lin(perms), tpl)
    R = case["R"].reshape(case["R"].shape[0], -1)
    runs = []
    gd = GDMLPredict(model, max_processes=1)
    runs.append(gd.predict(R))
    gd._set_chunk_size(1)
    runs.append(gd.predict(R))
    rev = dict(model, R_desc=np.ascontiguousarray(model["R_desc"][:, ::-1]),
               R_d_desc_alpha=np.ascontiguousarray(model["R_d_desc_alpha"][::-1]))
    runs.append(GDMLPredict(rev, max_processes=1).predict(R))
    E, F = (np.array(a) for a in runs[0])
    dF = max(np.max(np.abs(np.asarray(f) - F)) for _, f in runs[1:])
    dE = max(np.max(np.abs(np.asarray(e) - E)) for e, _ in runs[1:])
    band_F = dF / np.max(np.abs(F))
    band_E = dE / np.max(np.abs(E - case["c"]))
    return E, F, band_F, band_E


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("MLFF_REFERENCE"),
                    help="checkout of the reference (bluecher31/mlff-preconditioner)")
    a = ap.parse_args()
    if not a.ref:
        ap.error("--ref (or MLFF_REFERENCE) is required")
    GDMLPredict, train, Desc = import_reference(Path(a.ref))
    out = {"cases": np.array(sorted(cases()))}
    for name, case in cases().items():
        E, F, band_F, band_E = reference_predict(GDMLPredict, train, Desc, case)
        print(f"{name}: M={case['R_train'].shape[0]} n={case['R_train'].shape[1]} "
              f"Q={case['R'].shape[0]} band_F={band_F:.3e} band_E={band_E:.3e} "
              f"max|F|={np.max(np.abs(F)):.3e} max|E-c|={np.max(np.abs(E - case['c'])):.3e}", flush=True)
        assert 0 < band_F < 1e-9 and 0 < band_E < 1e-9, (name, band_F, band_E)
        for key, val in case.items():
            out[f"{name}__{key}"] = val
        out[f"{name}__sig"] = np.float64(SIG)
        out[f"{name}__E"], out[f"{name}__F"] = E, F
        out[f"{name}__band_F"], out[f"{name}__band_E"] = np.float64(band_F), np.float64(band_E)
    path = HERE / "sgdml_predict_cases.npz"
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({path.stat().st_size / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
