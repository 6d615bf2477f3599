"""Time on-device molecular dynamics (GDMLPredict.md -> mlff_md_run) against the host loop over
GDMLPredict.predict, one predict call per step, on one MI355X.

    python tools/bench_md.py [--rounds 7] [--steps 256] [--stride 8] [--warmup 1]
                             [--legs golden m5833] [--leg-timeout 240]

Legs (models, both of ethanol's shape: n = 9, D = 36, the tile form):
  golden   the reference's trained ethanol model tests/golden/sgdml_model_ethanol_n621.npz (M = 23)
  m5833    synthetic.ethanol_like(5833) with random coefficients (scaled by 1e-3, so that the
           replicas stay near their start for the steps timed), M = 5833

Per leg and batch size Q (1 and 64 replicas), by the host clock around calls that end in a
stream synchronisation:
  md_2, md_4   one md() call of --steps steps, a frame every --stride steps, with two and with
               four launches per step (the forms the model has)
  loop         the numpy loop  v += h F; R += dt v; E, F = predict(R); v += h F  over the same
               object's predict(), --steps steps: what a user ran before md() existed
A round times md_2, md_4 and loop one after the other (after --warmup untimed rounds), so every
md time has a loop time taken next to it; the figures are the medians over --rounds rounds of the
times and of the per-round ratios, with the spread over the rounds.  The last frame of every
md() run is compared with the loop's, bit for bit.

Each leg runs in a child process of its own under a time limit (--leg-timeout seconds); a leg
that fails or runs out of time ends the run, and no further leg is started.  One JSON line.
"""
from __future__ import annotations

import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO / "mlff-preconditioner_amd"), str(Path(__file__).resolve().parent)]

import numpy as np  # noqa: E402

LEGS = ("golden", "m5833")
BATCHES = (1, 64)
DT = 0.5
MASS_OF_Z = {1: 1.008, 6: 12.011, 8: 15.999}


def leg_model(name):
    from sgdml_amd import synthetic
    from sgdml_amd.model import r_d_desc_alpha
    from sgdml_amd.solver import host_descriptors

    if name == "golden":
        f = np.load(REPO / "tests" / "golden" / "sgdml_model_ethanol_n621.npz", allow_pickle=False)
        return {k: f["model__" + k] for k in ("type", "z", "perms", "sig", "std", "c", "R_desc", "R_d_desc_alpha")}
    ds = synthetic.ethanol_like(5833, seed=0)
    Rd, Rdd = host_descriptors(ds["R"])
    alphas = 1e-3 * np.random.default_rng(2).standard_normal(3 * 9 * 5833)
    return {"type": "m", "z": ds["z"], "perms": np.arange(9)[None, :], "sig": 10.0, "std": 1.0, "c": 0.0,
            "R_desc": Rd.T, "R_d_desc_alpha": r_d_desc_alpha(Rdd, alphas)}


def host_loop(gd, R0, V0, h3, dt, steps):
    """The last frame (R, V, E, F) of the loop over predict."""
    R, V = R0.copy(), V0.copy()
    E, F = gd.predict(R)
    for _ in range(steps):
        V = V + h3 * F
        R = R + dt * V
        E, F = gd.predict(R)
        V = V + h3 * F
    return R, V, E, F


def run_leg(name, a):
    """The record of one leg (this process opens the GPU)."""
    import sgdml_amd
    from sgdml_amd import synthetic
    from sgdml_amd.predict import ACC_KCAL_MOL_A_AMU_FS

    if sgdml_amd.device_count() < 1:
        raise SystemExit("no GPU visible to libmlffpcg.so")
    model = leg_model(name)
    masses = np.array([MASS_OF_Z[int(z)] for z in np.asarray(model["z"]).reshape(-1)])
    h3 = np.repeat((0.5 * DT * ACC_KCAL_MOL_A_AMU_FS) / masses, 3)
    rec = {"leg": name, "steps": a.steps, "stride": a.stride, "dt": DT, "batches": {}}
    with sgdml_amd.GDMLPredict(model, device=0) as gd:
        forms = (2, 4) if gd.form == "tile" else (4,)
        rec.update(M=int(gd.n_train), n_atoms=int(gd.n_atoms), form=gd.form, frame_capacity=gd.md_info()[1])
        for Q in BATCHES:
            R0 = np.ascontiguousarray(synthetic.ethanol_like(Q, seed=1000 + Q)["R"].reshape(Q, 27))
            V0 = 0.01 * np.random.default_rng(Q).standard_normal((Q, 27))
            t = {f"md_{f}": [] for f in forms}
            t["loop"] = []
            last = {}
            for rnd in range(a.warmup + a.rounds):
                for f in forms:
                    t0 = time.perf_counter()
                    last[f] = gd.md(R0, V0, masses, DT, a.steps, stride=a.stride, forces=True, launches=f)
                    dt_s = time.perf_counter() - t0
                    if rnd >= a.warmup:
                        t[f"md_{f}"].append(dt_s)
                t0 = time.perf_counter()
                ref = host_loop(gd, R0, V0, h3, DT, a.steps)
                dt_s = time.perf_counter() - t0
                if rnd >= a.warmup:
                    t["loop"].append(dt_s)
            b = {"replicas": int(Q), "finite": bool(np.all(np.isfinite(ref[0])))}
            loop = np.array(t["loop"])
            b["loop_steps_per_s"] = a.steps / float(np.median(loop))
            b["loop_us_per_step"] = 1e6 * float(np.median(loop)) / a.steps
            b["loop_us_per_step_min_max"] = [1e6 * float(loop.min()) / a.steps, 1e6 * float(loop.max()) / a.steps]
            for f in forms:
                m = np.array(t[f"md_{f}"])
                k = f"md_{f}"
                b[k + "_steps_per_s"] = a.steps / float(np.median(m))
                b[k + "_us_per_step"] = 1e6 * float(np.median(m)) / a.steps
                b[k + "_us_per_step_min_max"] = [1e6 * float(m.min()) / a.steps, 1e6 * float(m.max()) / a.steps]
                ratio = loop / m
                b["loop_over_" + k] = float(np.median(ratio))
                b["loop_over_" + k + "_min_max"] = [float(ratio.min()), float(ratio.max())]
                tr = last[f]
                b[k + "_same_bits_as_loop"] = bool(
                    np.array_equal(tr["R"][:, -1].reshape(Q, 27), ref[0]) and np.array_equal(tr["V"][:, -1].reshape(Q, 27), ref[1])
                    and np.array_equal(tr["E"][:, -1], ref[2]) and np.array_equal(tr["F"][:, -1], ref[3]))
            if len(forms) == 2:
                r24 = np.array(t["md_4"]) / np.array(t["md_2"])
                b["md_4_over_md_2"] = float(np.median(r24))
                b["md_4_over_md_2_min_max"] = [float(r24.min()), float(r24.max())]
            rec["batches"][f"Q{Q}"] = b
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", nargs="*", default=list(LEGS), choices=list(LEGS))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--stride", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--leg-timeout", type=float, default=240.0)
    ap.add_argument("--child-leg", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child_leg is not None:
        print(json.dumps(run_leg(a.child_leg, a)), flush=True)
        return
    from sgdml_amd import _native

    out = {"tool": "bench_md", "rounds": a.rounds, "warmup": a.warmup, "build_hash": _native.build_hash(), "legs": {}}
    for name in a.legs:
        cmd = [sys.executable, str(Path(__file__).resolve()), "--child-leg", name, "--rounds", str(a.rounds),
               "--steps", str(a.steps), "--stride", str(a.stride), "--warmup", str(a.warmup)]
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
