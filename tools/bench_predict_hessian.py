"""Time analytic Hessians (mlff_predict_hessian) against central differences of predicted forces
on one MI355X.

    python tools/bench_predict_hessian.py [--baseline-lib /path/to/parent/libmlffpcg.so]
                                          [--rounds 5] [--reps 15] [--warmup 5] [--energy-constraints]

Model: the ethanol-sized synthetic model of tools/bench_predict.py (M = 5833, n = 9, n_perms = 1).
Batches: Q = 1 and Q = 64 Hessians.

  analytic    one mlff_predict_hessian call on the Q geometries (this build)
  baseline    one mlff_predict call on the 6 n Q central-difference displacements (h = 1e-4) of
              the same geometries, in one batch: the only route to a Hessian before this entry
              point existed.  --baseline-lib times the mlff_predict of another build of the library
              (the parent commit's), through a plain binding, in the same process; without it this
              build's mlff_predict is timed.  Forming the displacements and the difference quotient
              on the host is not timed.

Both are called through the same plain ctypes binding and bracketed by HIP events on their
context's stream (copies in and out included).  A round times the analytic call and then the
baseline (median of --reps calls after --warmup each); the figures are the medians over --rounds
alternating rounds, the spread over the rounds is reported with them.  One JSON line: per batch
size both times, their ratio (baseline / analytic), the largest deviation between the two
Hessians, and the achieved fraction of the fp64 vector peak (78.6 TFLOP/s) of the flops of
mlff_predict_hessian_info over the whole call.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO / "mlff-preconditioner_amd"), str(Path(__file__).resolve().parent)]

import numpy as np  # noqa: E402

H_STEP = 1e-4
DP, IP, VP = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32), ctypes.c_void_p


def dptr(a):
    return a.ctypes.data_as(DP)


class Lib:
    """A plain binding of the prediction entry points of one build of the library."""

    def __init__(self, path, hessian):
        self.lib = lib = ctypes.CDLL(str(path))
        lib.mlff_ctx_create.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_char_p,
                                        ctypes.c_int64, ctypes.POINTER(VP)]
        lib.mlff_predict_set_model.argtypes = [VP, DP, DP, ctypes.c_int64, ctypes.c_int, IP, ctypes.c_int,
                                               ctypes.c_double, ctypes.c_double, ctypes.c_double]
        lib.mlff_predict_set_energy_coefficients.argtypes = [VP, DP]
        lib.mlff_predict.argtypes = [VP, DP, ctypes.c_int64, DP, DP]
        lib.mlff_stream.argtypes = [VP, ctypes.POINTER(VP)]
        lib.mlff_ctx_destroy.argtypes = [VP]
        lib.mlff_build_hash.restype = ctypes.c_char_p
        if hessian:
            lib.mlff_predict_hessian.argtypes = [VP, DP, ctypes.c_int64, DP]
            lib.mlff_predict_hessian_info.argtypes = [VP, DP, DP]
        self.ctx = VP()
        self.hash = lib.mlff_build_hash().decode()

    def ok(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed with {rc}")

    def open(self, model):
        Rd = np.ascontiguousarray(np.asarray(model["R_desc"]).T)
        Rda = np.ascontiguousarray(model["R_d_desc_alpha"])
        perms = np.ascontiguousarray(model["perms"], dtype=np.int32)
        M, n = Rd.shape[0], perms.shape[1]
        self.ok(self.lib.mlff_ctx_create(0, 0, 1, None, 3 * n * M, ctypes.byref(self.ctx)), "mlff_ctx_create")
        self.ok(self.lib.mlff_predict_set_model(self.ctx, dptr(Rd), dptr(Rda), M, n, perms.ctypes.data_as(IP),
                                                perms.shape[0], float(model["sig"]), float(model["std"]),
                                                float(model["c"])), "mlff_predict_set_model")
        if "alphas_E" in model:
            aE = np.ascontiguousarray(model["alphas_E"], dtype=np.float64)
            self.ok(self.lib.mlff_predict_set_energy_coefficients(self.ctx, dptr(aE)),
                    "mlff_predict_set_energy_coefficients")
        self.stream = VP()
        self.ok(self.lib.mlff_stream(self.ctx, ctypes.byref(self.stream)), "mlff_stream")
        return self

    def close(self):
        if self.ctx:
            self.lib.mlff_ctx_destroy(self.ctx)
            self.ctx = VP()


def displacements(R, h):
    """(6 n Q) x n x 3: for every geometry the 3n forward, then the 3n backward displacements."""
    Q, n = R.shape[:2]
    n3 = 3 * n
    out = np.repeat(R.reshape(Q, 1, n3), 2 * n3, axis=1)
    out[:, np.arange(n3), np.arange(n3)] += h
    out[:, n3 + np.arange(n3), np.arange(n3)] -= h
    return np.ascontiguousarray(out.reshape(Q * 2 * n3, n, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 64])
    ap.add_argument("--train", type=int, default=5833)
    ap.add_argument("--energy-constraints", action="store_true")
    a = ap.parse_args()
    import sgdml_amd
    from bench_predict import FP64_VECTOR_PEAK, Events, build_model, median_ms, queries
    from sgdml_amd import _native, synthetic

    if sgdml_amd.device_count() < 1:
        raise SystemExit("no GPU visible to libmlffpcg.so")
    ds = synthetic.ethanol_like(a.train, seed=0)
    model = build_model(ds, 1, a.energy_constraints)[0]
    n = ds["R"].shape[1]
    n3 = 3 * n
    ev = Events()
    new = Lib(_native.LIB_PATH, True).open(model)
    base = Lib(a.baseline_lib or _native.LIB_PATH, False).open(model)
    try:
        fl, by = ctypes.c_double(), ctypes.c_double()
        new.ok(new.lib.mlff_predict_hessian_info(new.ctx, ctypes.byref(fl), ctypes.byref(by)),
               "mlff_predict_hessian_info")
        rec = {"tool": "bench_predict_hessian", "M": int(a.train), "n_atoms": int(n),
               "use_E_cstr": bool(a.energy_constraints), "fd_step": H_STEP,
               "rounds": a.rounds, "reps": a.reps, "warmup": a.warmup,
               "flops_per_hessian": fl.value, "build_hash": new.hash, "baseline_build_hash": base.hash,
               "baseline_is_parent_build": a.baseline_lib is not None, "batches": {}}
        for Q in a.batches:
            R = np.ascontiguousarray(queries(ds, Q, 1000 + Q))
            disp = displacements(R, H_STEP)
            H = np.empty((Q, n3, n3))
            E, F = np.empty(disp.shape[0]), np.empty((disp.shape[0], n3))
            run_new = lambda: new.ok(new.lib.mlff_predict_hessian(new.ctx, dptr(R), Q, dptr(H)),  # noqa: E731
                                     "mlff_predict_hessian")
            run_base = lambda: base.ok(base.lib.mlff_predict(base.ctx, dptr(disp), disp.shape[0], dptr(E),  # noqa: E731
                                                             dptr(F)), "mlff_predict")
            t_new, t_base = [], []
            for _ in range(a.rounds):
                t_new.append(median_ms(ev, new.stream, run_new, a.reps, a.warmup))
                t_base.append(median_ms(ev, base.stream, run_base, a.reps, a.warmup))
            Ff = F.reshape(Q, 2, n3, n3)
            H_fd = -(Ff[:, 0] - Ff[:, 1]) / (2 * H_STEP)
            ms_new, ms_base = float(np.median(t_new)), float(np.median(t_base))
            rate = fl.value * Q / (ms_new * 1e-3)
            rec["batches"][f"Q{Q}"] = {
                "hessians": int(Q), "baseline_geometries": int(disp.shape[0]),
                "analytic_us": ms_new * 1e3, "analytic_us_min_max": [min(t_new) * 1e3, max(t_new) * 1e3],
                "baseline_us": ms_base * 1e3, "baseline_us_min_max": [min(t_base) * 1e3, max(t_base) * 1e3],
                "baseline_over_analytic": ms_base / ms_new,
                "max_abs_dH_over_max_abs_H": float(np.max(np.abs(H - H_fd)) / np.max(np.abs(H))),
                "fp64_flops_per_s": rate, "frac_of_fp64_vector_peak": rate / FP64_VECTOR_PEAK}
        print(json.dumps(rec), flush=True)
    finally:
        new.close()
        base.close()


if __name__ == "__main__":
    main()
