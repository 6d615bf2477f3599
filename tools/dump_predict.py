"""Dump the predictor's E, F (and Hessians) for cases of tests/golden/sgdml_predict_cases.npz, so
that two builds can be compared bit for bit:

    python tools/dump_predict.py --out a.npz [--tree /path/to/another/checkout] [--cases eth3 eth tube]
                                 [--hessian] [--energy-constraints]
    python tools/dump_predict.py --compare a.npz b.npz

--hessian also stores gd.hessian(R) of every case.  --energy-constraints gives every model a
deterministic alphas_E (M standard normal draws, seed 20240), so that the ECSTR kernels run.

--tree: import sgdml_amd (and its libmlffpcg.so) from that checkout instead of this one; the
cases are always read from this one.  Default forms (tile for D <= 288, stream otherwise).
--compare prints one line per array and exits 1 unless every array is np.array_equal.
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent


ALPHAS_E_SEED = 20240


def dump(tree: Path, names, out: Path, hessian: bool = False, energy_constraints: bool = False):
    sys.path[:0] = [str(tree / "mlff-preconditioner_amd")]
    import sgdml_amd
    from sgdml_amd import _native
    from sgdml_amd.model import r_d_desc_alpha
    from sgdml_amd.solver import host_descriptors

    assert Path(sgdml_amd.__file__).resolve().is_relative_to(tree.resolve()), sgdml_amd.__file__
    f = np.load(REPO / "tests" / "golden" / "sgdml_predict_cases.npz", allow_pickle=False)
    res = {"build_hash": np.array(_native.build_hash())}
    for name in names:
        g = lambda k: f[f"{name}__{k}"]  # noqa: E731
        Rd, Rdd = host_descriptors(g("R_train"))
        model = {"type": "m", "z": g("z"), "perms": g("perms"), "sig": g("sig"), "std": g("std"),
                 "c": g("c"), "R_desc": Rd.T, "R_d_desc_alpha": r_d_desc_alpha(Rdd, g("alphas_F"))}
        if energy_constraints:
            M = g("R_train").shape[0]
            model["alphas_E"] = np.random.default_rng(ALPHAS_E_SEED).standard_normal(M)
        with sgdml_amd.GDMLPredict(model, device=0) as gd:
            E, F = gd.predict(g("R"))
            print(f"{name}: form {gd.form}, Q = {E.size}, use_E_cstr {gd.use_E_cstr}, "
                  f"build {_native.build_hash()}", flush=True)
            if hessian:
                res[f"{name}__H"] = gd.hessian(g("R"))
        res[f"{name}__E"], res[f"{name}__F"] = E, F
    out.parent.mkdir(parents=True, exist_ok=True)
    np.savez(out, **res)


def compare(a: Path, b: Path) -> int:
    fa, fb = np.load(a, allow_pickle=False), np.load(b, allow_pickle=False)
    print(f"builds {fa['build_hash']} / {fb['build_hash']}")
    keys = sorted(k for k in fa.files if k != "build_hash")
    assert keys == sorted(k for k in fb.files if k != "build_hash")
    bad = 0
    for k in keys:
        same = np.array_equal(fa[k], fb[k])
        print(f"{k} {fa[k].shape}: array_equal = {same}")
        bad += not same
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", type=Path)
    ap.add_argument("--tree", type=Path, default=REPO)
    ap.add_argument("--cases", nargs="*", default=["eth3", "eth", "tube"])
    ap.add_argument("--hessian", action="store_true")
    ap.add_argument("--energy-constraints", action="store_true")
    ap.add_argument("--compare", nargs=2, type=Path)
    a = ap.parse_args()
    if a.compare:
        raise SystemExit(compare(*a.compare))
    if a.out is None:
        ap.error("--out or --compare is required")
    dump(a.tree, a.cases, a.out, a.hessian, a.energy_constraints)


if __name__ == "__main__":
    main()
