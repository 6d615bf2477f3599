#!/usr/bin/env python3
"""Share sweep of the two-role tile mat-vec (k_symv_dyn<true>) on one GPU.

    python tools/sweep_symgen.py [--n 65536] [--tiles 2048,2730,...] [--roles cu] [--wgs 2|3]
                                 --out FILE.json

For each configuration a fresh operator is built from the same RBF points and timed over
three runs of 10 unpreconditioned PCG steps (after 5 warm-up steps); x and the residual trace
after the 35 steps are compared bit for bit with the first configuration's ("off": every unit
streamed, MLFF_SYM_GEN=0).

Configurations: "off"; "0:2" no whole tile generated, the quarters the generating role's;
"8192:2" (every whole tile : 2) every unit the generating role's; "<t>:0" t generated whole
tiles, the quarters to either role.  Since a workgroup that is done takes units of the other
role's range, "0:2" and "8192:2" isolate a role only under MLFF_SYM_ROLES=index with the old
library; --pure adds "0:2/stream" and "8192:2/gen", the same plans with all 512 workgroups in
the one role (the role's rate with the chip to itself, an upper bound of its rate beside the
other role).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "mlff-preconditioner_amd"))

KEYS = ("MLFF_SYM_GEN", "MLFF_SYM_GEN_TILES", "MLFF_SYM_GEN_QUARTERS", "MLFF_SYM_ROLES",
        "MLFF_SYM_WGS")


def config_env(cfg: str, roles: str | None, wgs: str | None = None) -> dict:
    if cfg == "off":
        return {"MLFF_SYM_GEN": "0"}
    cfg, _, forced = cfg.partition("/")
    t, q = cfg.split(":")
    env = {"MLFF_SYM_GEN_TILES": t, "MLFF_SYM_GEN_QUARTERS": q}
    if wgs:
        env["MLFF_SYM_WGS"] = wgs
    if forced or roles:
        env["MLFF_SYM_ROLES"] = forced or roles
    return env


def run(cfg_env: dict, n: int, lam: float, ell: float):
    import sgdml_amd
    from sgdml_amd import synthetic

    for k in KEYS:
        os.environ.pop(k, None)
    os.environ.update(cfg_env)
    X, b = synthetic.rbf_points(n, 3, 0)
    s = sgdml_amd.KernelSolver(n, device=0)
    try:
        s.gen_rbf(X, ell)
        s.set_operator(1.0, lam)
        s.precon_none()
        _, nbytes = s.storage_info()
        s.pcg_start(b, tol=0.0, maxiter=36)
        s.pcg_run(5, 5)
        ms = []
        for _ in range(3):
            s.synchronize()
            t0 = time.perf_counter()
            s.pcg_run(10, 10)
            s.synchronize()
            ms.append(round((time.perf_counter() - t0) / 10 * 1e3, 4))
        x = np.asarray(s.pcg_x(), dtype=np.float64).copy()
        trace = np.asarray(s.pcg_trace(), dtype=np.float64).copy()
    finally:
        s.close()
    return ms, float(nbytes), x, trace


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--lam", type=float, default=1e-6)
    ap.add_argument("--ell", type=float, default=0.2)
    ap.add_argument("--tiles", default="2048,2730,3072,3500,4096",
                    help="generated whole tiles of the <t>:0 configurations")
    ap.add_argument("--whole", type=int, default=8192,
                    help="generated whole tiles of the all-generated configuration")
    ap.add_argument("--roles", default=None, help="MLFF_SYM_ROLES of the run (default: the library's)")
    ap.add_argument("--wgs", choices=["2", "3"], default=None,
                    help="MLFF_SYM_WGS of the run: workgroups per CU (default: the library's choice)")
    ap.add_argument("--pure", action="store_true", help="add the one-role configurations")
    ap.add_argument("--out", type=Path, required=True)
    a = ap.parse_args()
    cfgs = ["off", "0:2", f"{a.whole}:2"] + [f"{t}:0" for t in a.tiles.split(",") if t]
    if a.pure:
        cfgs += ["0:2/stream", f"{a.whole}:2/gen"]
    rows, first = [], None
    for cfg in cfgs:
        env = config_env(cfg, a.roles, a.wgs)
        ms, nbytes, x, trace = run(env, a.n, a.lam, a.ell)
        if first is None:
            first = (x, trace)
        same = bool(np.array_equal(x, first[0]) and np.array_equal(trace, first[1]))
        rows.append({"cfg": cfg, "env": env, "ms_per_iter": ms, "bytes": nbytes,
                     "same_as_first": same})
        print(json.dumps(rows[-1]), flush=True)
        a.out.parent.mkdir(parents=True, exist_ok=True)
        a.out.write_text(json.dumps(rows, indent=1))
    return 0 if all(r["same_as_first"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
