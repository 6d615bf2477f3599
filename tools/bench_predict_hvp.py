"""Time Hessian-vector products (mlff_predict_hvp) against the full Hessian and the prediction at
the same queries on one MI355X.

    python tools/bench_predict_hvp.py [--rounds 5] [--reps 15] [--warmup 5] [--energy-constraints]
                                      [--legs ethanol nanotube] [--leg-timeout 240]

Legs (models):
  ethanol    the reference's trained ethanol model tests/golden/sgdml_model_ethanol_n621.npz
             (621 unknowns: M = 23, n = 9, D = 36: the register form of the pair stage), Q = 1 and Q = 64
             ethanol-like geometries
  nanotube   synthetic.nanotube_like, M = 141, n = 370, D = 68 265 (the stream form), random
             coefficients, Q = 1 and Q = 4

Per leg and batch size Q, through the same plain binding and bracketed by HIP events on the
context's stream (copies in and out included):
  hvp_K1, hvp_K8   one mlff_predict_hvp call with K = 1 and K = 8 vectors per query
  hessian          one mlff_predict_hessian call on the same Q queries: the only route to H v
                   before mlff_predict_hvp existed (the product with v on the host is not timed)
  predict          one mlff_predict call on the same Q queries
A round times the four in that order (median of --reps calls after --warmup each); the figures
are the medians over --rounds rounds, the spread over the rounds is reported with them.

Each leg runs in a child process of its own under a time limit (--leg-timeout seconds); a leg
that fails or runs out of time ends the run, and no further leg is started.  One JSON line: per
leg and Q the four times, hessian / hvp_K1, hvp_K8 / hvp_K1, hvp_K1 / predict, the largest
deviation of the K = 1 product from hessian @ v, and the modelled flops of mlff_predict_hvp_info.
"""
from __future__ import annotations

import argparse
import json
import subprocess
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO / "mlff-preconditioner_amd"), str(Path(__file__).resolve().parent)]

import numpy as np  # noqa: E402

LEGS = {"ethanol": [1, 64], "nanotube": [1, 4]}


def leg_inputs(name, energy_constraints):
    """(model, a function Q -> queries Q x n x 3) of a leg."""
    from bench_predict import build_model, queries
    from sgdml_amd import synthetic

    if name == "ethanol":
        f = np.load(REPO / "tests" / "golden" / "sgdml_model_ethanol_n621.npz", allow_pickle=False)
        model = {k: f["model__" + k] for k in ("type", "z", "perms", "sig", "std", "c", "R_desc", "R_d_desc_alpha")}
        if energy_constraints:
            model["alphas_E"] = np.random.default_rng(101).standard_normal(model["R_desc"].shape[1])
        ds = synthetic.ethanol_like(64, seed=0)
    else:
        ds = synthetic.nanotube_like(141, seed=0)
        model = build_model(ds, 2, energy_constraints)[0]
    return model, lambda Q: np.ascontiguousarray(queries(ds, Q, 1000 + Q))


def run_leg(name, a):
    """The record of one leg (this process opens the GPU)."""
    import sgdml_amd
    from bench_predict import Events, median_ms
    from sgdml_amd import _native as nat

    if sgdml_amd.device_count() < 1:
        raise SystemExit("no GPU visible to libmlffpcg.so")
    model, make_queries = leg_inputs(name, a.energy_constraints)
    ev = Events()
    rec = {"leg": name, "use_E_cstr": bool(a.energy_constraints), "batches": {}}
    with sgdml_amd.GDMLPredict(model, device=0) as gd:
        eng = gd._engines[0]
        stream = eng.stream_handle()
        n3 = 3 * gd.n_atoms
        fl, _ = eng.predict_hvp_info()
        hfl, _ = eng.predict_hessian_info()
        rec.update(M=int(gd.n_train), n_atoms=int(gd.n_atoms), n_perms=int(gd.n_perms), form=gd.form,
                   flops_per_product=fl, flops_per_hessian=hfl, flops_per_prediction=gd.flops_per_query)
        for Q in LEGS[name]:
            R = make_queries(Q)
            V = np.random.default_rng(77 + Q).standard_normal((Q, 8, n3))
            V1 = np.ascontiguousarray(V[:, :1])
            HV1, HV8 = np.empty((Q, 1, n3)), np.empty((Q, 8, n3))
            H, E, F = np.empty((Q, n3, n3)), np.empty(Q), np.empty((Q, n3))
            calls = {
                "hvp_K1": lambda: eng._call("mlff_predict_hvp", nat.dptr(R), nat.dptr(V1), Q, 1, nat.dptr(HV1)),
                "hvp_K8": lambda: eng._call("mlff_predict_hvp", nat.dptr(R), nat.dptr(V), Q, 8, nat.dptr(HV8)),
                "hessian": lambda: eng._call("mlff_predict_hessian", nat.dptr(R), Q, nat.dptr(H)),
                "predict": lambda: eng._call("mlff_predict", nat.dptr(R), Q, nat.dptr(E), nat.dptr(F)),
            }
            t = {k: [] for k in calls}
            for _ in range(a.rounds):
                for k, fn in calls.items():
                    t[k].append(median_ms(ev, stream, fn, a.reps, a.warmup) * 1e3)
            med = {k: float(np.median(v)) for k, v in t.items()}
            ref = np.einsum("qij,qj->qi", H, V[:, 0])
            b = {"queries": int(Q)}
            for k in calls:
                b[k + "_us"] = med[k]
                b[k + "_us_min_max"] = [min(t[k]), max(t[k])]
            b.update(hessian_over_hvp_K1=med["hessian"] / med["hvp_K1"],
                     hvp_K8_over_hvp_K1=med["hvp_K8"] / med["hvp_K1"],
                     hvp_K1_over_predict=med["hvp_K1"] / med["predict"],
                     K8_equals_K1_bits=bool(np.array_equal(HV8[:, 0], HV1[:, 0])),
                     max_abs_dHv_over_max_abs_Hv=float(np.max(np.abs(HV1[:, 0] - ref)) / np.max(np.abs(ref))))
            rec["batches"][f"Q{Q}"] = b
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", nargs="*", default=list(LEGS), choices=list(LEGS))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--energy-constraints", action="store_true")
    ap.add_argument("--leg-timeout", type=float, default=240.0)
    ap.add_argument("--child-leg", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child_leg is not None:
        print(json.dumps(run_leg(a.child_leg, a)), flush=True)
        return
    from sgdml_amd import _native

    out = {"tool": "bench_predict_hvp", "rounds": a.rounds, "reps": a.reps, "warmup": a.warmup,
           "build_hash": _native.build_hash(), "legs": {}}
    for name in a.legs:
        cmd = [sys.executable, str(Path(__file__).resolve()), "--child-leg", name, "--rounds", str(a.rounds),
               "--reps", str(a.reps), "--warmup", str(a.warmup)] + (["--energy-constraints"] if a.energy_constraints else [])
        try:
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=a.leg_timeout)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"leg {name}: no result within {a.leg_timeout:.0f} s; nothing further is started")
        if res.returncode != 0:
            sys.stderr.write(res.stderr)
            raise SystemExit(f"leg {name} failed with {res.returncode}; nothing further is started")
        out["legs"][name] = json.loads(res.stdout.strip().splitlines()[-1])
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
