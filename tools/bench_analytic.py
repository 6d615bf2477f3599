"""Measure the closed-form ('analytic') sGDML solve (mlff_dense_cho_solve) on one MI355X.

    python tools/bench_analytic.py [--large] [--reps 3] [--M points] [--skip-potrf]

One JSON line: an ethanol_like system (synthetic provides no symmetries: n_perms = 1) of
M = 600 training points, N = 27 M = 16200 (--large: M = 1200, N = 32400):
  assemble_s            wall seconds of mlff_assemble_sgdml (dense K and the operator tables)
  copy_s / factor_s / solves_s   device seconds of mlff_dense_cho_solve's phases (stream events),
                        every repetition and the median; factor_tflops = N^3 / 3 / factor_s,
                        solves_bytes_per_s = 8 N^2 / solves_s (L's lower triangle once per sweep)
  rel_resid             ||(-K + shift I) x - y|| / ||y|| through the context's own mat-vec
  potrf_v0_s / potrf_v1_s        mlff_test_potrf on the same matrix -K + shift I (host copy),
                        variant 0 the one-level factorisation, 1 the two-level one
                        (MLFF_POTRF_OUTER, default 256), every repetition and the median
The labels are Gaussian (synthetic.ethanol_like); where -K + 1e-10 I is not numerically positive
definite the shift is raised by factors of 100 until the factorisation succeeds and the shift
used is reported (the timings do not depend on the values).
"""
from __future__ import annotations

import argparse
import json
import sys
import timeit
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO / "mlff-preconditioner_amd")]

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--large", action="store_true", help="N = 32400 instead of 16200")
    ap.add_argument("--M", type=int, default=None, help="training points (N = 27 M)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-potrf", action="store_true",
                    help="only the solve (no host copy of the matrix)")
    a = ap.parse_args()
    import sgdml_amd
    from sgdml_amd import _native, synthetic
    from sgdml_amd.solver import host_descriptors

    if sgdml_amd.device_count() < 1:
        raise SystemExit("no GPU visible to libmlffpcg.so")
    M = a.M or (1200 if a.large else 600)
    ds = synthetic.ethanol_like(M, seed=0)
    y, _ = synthetic.labels(ds["F"])
    n = y.size
    Rd, Rdd = host_descriptors(ds["R"])
    rec = {"leg": "analytic_ethanol_like", "M": M, "N": n, "reps": a.reps,
           "build_hash": _native.build_hash()}
    med = lambda v: float(np.median(v))  # noqa: E731
    with sgdml_amd.KernelSolver(n, device=0) as s:
        t0 = timeit.default_timer()
        s.assemble_sgdml(Rd, Rdd, np.arange(9)[None, :], 10.0)
        s.synchronize()
        rec["assemble_s"] = timeit.default_timer() - t0
        shift, failed = 1e-10, []
        while True:
            try:
                x, sec = s.dense_cho_solve(y, sigma_K=-1.0, shift=shift, want_seconds=True)
                break
            except np.linalg.LinAlgError:
                failed.append(shift)
                shift *= 100.0
                if shift > 1.0:
                    raise
        rec.update(shift=shift, shifts_not_positive_definite=failed)
        runs = [sec] + [s.dense_cho_solve(y, sigma_K=-1.0, shift=shift, want_seconds=True)[1]
                        for _ in range(a.reps - 1)]
        runs = np.array(runs)
        for i, name in enumerate(("copy_s", "factor_s", "solves_s")):
            rec[name] = med(runs[:, i])
            rec[name + "_all"] = [float(v) for v in runs[:, i]]
        rec["factor_tflops"] = n ** 3 / 3.0 / rec["factor_s"] / 1e12
        rec["solves_bytes_per_s"] = 8.0 * n * n / rec["solves_s"]
        s.set_operator(-1.0, shift)
        rec["rel_resid"] = float(np.linalg.norm(s.matvec(x) - y) / np.linalg.norm(y))
        total = rec["assemble_s"] + rec["copy_s"] + rec["factor_s"] + rec["solves_s"]
        rec["split"] = {k: rec[k] / total for k in ("assemble_s", "copy_s", "factor_s", "solves_s")}
        if not a.skip_potrf:
            A = s.get_matrix_rows()
            np.negative(A, out=A)
            A[np.diag_indices(n)] += shift
            L = None
            for v in (0, 1):
                times = []
                for _ in range(a.reps):
                    L, t = s.test_potrf(A, variant=v, want_seconds=True)
                    times.append(t)
                rec[f"potrf_v{v}_s"] = med(times)
                rec[f"potrf_v{v}_s_all"] = times
                rec[f"potrf_v{v}_tflops"] = n ** 3 / 3.0 / med(times) / 1e12
            rec["potrf_v1_over_v0"] = rec["potrf_v1_s"] / rec["potrf_v0_s"]
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
