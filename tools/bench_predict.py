"""Measure the GPU predictor (sgdml_amd.GDMLPredict -> mlff_predict) on one MI355X.

    python tools/bench_predict.py [--legs ethanol nanotube ratio] [--reps 15] [--warmup 3]
                                  [--operator-lib /path/to/another/libmlffpcg.so]
                                  [--energy-constraints]

One JSON line per measurement:
  ethanol_like   M = 5833 (synthetic provides no symmetries: n_perms = 1), tile form,
                 Q = 1, 64, 4096: geometries/s, us per call, achieved fp64 FLOP/s of the pair
                 stage's algorithmic work (mlff_predict_info) as a fraction of the fp64 vector
                 peak (78.6 TFLOP/s)
  nanotube_like  M = 141, D = 68265, stream form, Q = 1, 16: achieved bytes/s of the
                 Rt / Zt stream (per query block of 4) against the measured copy rate (6.29 TB/s)
  ratio          prediction at Q = M on the ethanol model against one mlff_matvec of the
                 matrix-free pair-tile operator on the same geometries (the same pairs, minus the
                 energy fma); --operator-lib times the operator of another build of the library
                 (the parent commit's) in the same session
--energy-constraints gives the models of the ethanol and nanotube legs random energy
coefficients (alphas_E ~ N(0, 1), as a model trained with use_E_cstr carries), so that the
constrained pair kernels are the ones timed; the records then say "use_E_cstr": true.  The ratio
leg keeps the unconstrained model: the operator it is compared with has no energy rows.
Every figure is the median of --reps calls after --warmup calls, each call bracketed by HIP
events on the context's stream (the call's copies in and out included, for the prediction and
for the mat-vec alike).
"""
from __future__ import annotations

import argparse
import ctypes
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO / "mlff-preconditioner_amd")]

import numpy as np  # noqa: E402

FP64_VECTOR_PEAK = 78.6e12   # FLOP/s
COPY_RATE = 6.29e12          # bytes/s, measured float4 copy


class Events:
    """hipEvent pairs through the HIP runtime the library itself is linked against."""

    def __init__(self):
        self.hip = ctypes.CDLL("libamdhip64.so")
        self.hip.hipEventCreate.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
        self.hip.hipEventRecord.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        self.hip.hipEventSynchronize.argtypes = [ctypes.c_void_p]
        self.hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_void_p,
                                                 ctypes.c_void_p]
        self.a, self.b = ctypes.c_void_p(), ctypes.c_void_p()
        for e in (self.a, self.b):
            if self.hip.hipEventCreate(ctypes.byref(e)) != 0:
                raise RuntimeError("hipEventCreate failed")

    def time_ms(self, stream, fn) -> float:
        self.hip.hipEventRecord(self.a, stream)
        fn()
        self.hip.hipEventRecord(self.b, stream)
        self.hip.hipEventSynchronize(self.b)
        ms = ctypes.c_float()
        if self.hip.hipEventElapsedTime(ctypes.byref(ms), self.a, self.b) != 0:
            raise RuntimeError("hipEventElapsedTime failed")
        return float(ms.value)


def median_ms(ev, stream, fn, reps, warmup):
    for _ in range(warmup):
        fn()
    return float(np.median([ev.time_ms(stream, fn) for _ in range(reps)]))


def build_model(ds, seed, energy_constraints=False):
    from sgdml_amd.model import r_d_desc_alpha
    from sgdml_amd.solver import host_descriptors

    M, n = ds["R"].shape[:2]
    Rd, Rdd = host_descriptors(ds["R"])
    alphas = np.random.default_rng(seed).standard_normal(3 * n * M)
    model = {"type": "m", "z": ds["z"], "perms": np.arange(n)[None, :], "sig": 10.0, "std": 1.0,
             "c": 0.0, "R_desc": Rd.T, "R_d_desc_alpha": r_d_desc_alpha(Rdd, alphas)}
    if energy_constraints:
        model["alphas_E"] = np.random.default_rng(seed + 100).standard_normal(M)
    return model, Rd, Rdd, alphas


def queries(ds, Q, seed):
    rng = np.random.default_rng(seed)
    M = ds["R"].shape[0]
    return ds["R"][np.arange(Q) % M] + 0.03 * rng.standard_normal((Q,) + ds["R"].shape[1:])


def predict_leg(name, ds, model, Qs, form, ev, reps, warmup):
    import sgdml_amd

    out = []
    with sgdml_amd.GDMLPredict(model, device=0) as gd:
        if gd.form != form:
            raise RuntimeError(f"{name}: expected the {form} form, got {gd.form}")
        eng = gd._engines[0]
        stream = eng.stream_handle()
        for Q in Qs:
            R = queries(ds, Q, 1000 + Q)
            ms = median_ms(ev, stream, lambda: eng.predict(R), reps, warmup)
            rec = {"leg": name, "form": gd.form, "use_E_cstr": bool(gd.use_E_cstr),
                   "M": int(ds["R"].shape[0]), "Q": int(Q),
                   "slab": int(gd.slab), "us_per_call": ms * 1e3, "geometries_per_s": Q / (ms * 1e-3)}
            if form == "tile":
                fl = gd.flops_per_query * Q / (ms * 1e-3)
                rec.update(fp64_flops_per_s=fl, frac_of_fp64_vector_peak=fl / FP64_VECTOR_PEAK)
            else:
                blocks = -(-Q // 4)  # every query block of 4 streams Rt / Zt once
                by = gd.bytes_per_query * blocks / (ms * 1e-3)
                rec.update(stream_bytes_per_s=by, frac_of_copy_rate=by / COPY_RATE)
            print(json.dumps(rec), flush=True)
            out.append(rec)
    return out


def operator_ms(lib_path, Rd, Rdd, alphas, n_atoms, ev, reps, warmup):
    """One mlff_matvec of the matrix-free operator (pair-tile form) through a plain binding of
    the library at lib_path (which may be an older build without the prediction entry points)."""
    lib = ctypes.CDLL(str(lib_path))
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    vp = ctypes.c_void_p
    lib.mlff_ctx_create.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_char_p,
                                    ctypes.c_int64, ctypes.POINTER(vp)]
    lib.mlff_sgdml_operator.argtypes = [vp, dp, dp, ctypes.c_int64, ctypes.c_int, ip, ctypes.c_int,
                                        ctypes.c_double]
    lib.mlff_set_operator.argtypes = [vp, ctypes.c_double, ctypes.c_double]
    lib.mlff_set_storage.argtypes = [vp, ctypes.c_int]
    lib.mlff_operator_form.argtypes = [vp, ctypes.POINTER(ctypes.c_int)]
    lib.mlff_matvec.argtypes = [vp, dp, dp]
    lib.mlff_stream.argtypes = [vp, ctypes.POINTER(vp)]
    lib.mlff_ctx_destroy.argtypes = [vp]
    lib.mlff_build_hash.restype = ctypes.c_char_p
    M = Rd.shape[0]
    N = alphas.size
    ctx = vp()

    def ok(rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed with {rc}")

    ok(lib.mlff_ctx_create(0, 0, 1, None, N, ctypes.byref(ctx)), "mlff_ctx_create")
    try:
        perms = np.arange(n_atoms, dtype=np.int32)[None, :].copy()
        Rd = np.ascontiguousarray(Rd)
        Rdd = np.ascontiguousarray(Rdd)
        ok(lib.mlff_sgdml_operator(ctx, Rd.ctypes.data_as(dp), Rdd.ctypes.data_as(dp), M, n_atoms,
                                   perms.ctypes.data_as(ip), 1, 10.0), "mlff_sgdml_operator")
        ok(lib.mlff_set_operator(ctx, 1.0, 1e-300), "mlff_set_operator")
        ok(lib.mlff_set_storage(ctx, 3), "mlff_set_storage")  # MLFF_STORAGE_MATFREE
        form = ctypes.c_int(-1)
        ok(lib.mlff_operator_form(ctx, ctypes.byref(form)), "mlff_operator_form")
        stream = vp()
        ok(lib.mlff_stream(ctx, ctypes.byref(stream)), "mlff_stream")
        y = np.empty(N)
        v = np.ascontiguousarray(alphas)
        run = lambda: ok(lib.mlff_matvec(ctx, v.ctypes.data_as(dp), y.ctypes.data_as(dp)), "mlff_matvec")  # noqa: E731
        ms = median_ms(ev, stream, run, reps, warmup)
        return ms, {0: "pair", 1: "rec", 2: "pt"}.get(form.value), lib.mlff_build_hash().decode(), y
    finally:
        lib.mlff_ctx_destroy(ctx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", nargs="*", default=["ethanol", "nanotube", "ratio"])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--operator-lib", default=None)
    ap.add_argument("--energy-constraints", action="store_true")
    a = ap.parse_args()
    import sgdml_amd
    from sgdml_amd import _native, synthetic

    if sgdml_amd.device_count() < 1:
        raise SystemExit("no GPU visible to libmlffpcg.so")
    ev = Events()
    if "ethanol" in a.legs or "ratio" in a.legs:
        ds = synthetic.ethanol_like(5833, seed=0)
        model, Rd, Rdd, alphas = build_model(ds, 1)
        if "ethanol" in a.legs:
            leg_model = model
            if a.energy_constraints:
                leg_model = build_model(ds, 1, True)[0]
            predict_leg("ethanol_like", ds, leg_model, [1, 64, 4096], "tile", ev, a.reps, a.warmup)
        if "ratio" in a.legs:
            M = ds["R"].shape[0]
            with sgdml_amd.GDMLPredict(model, device=0) as gd:
                eng = gd._engines[0]
                p_ms = median_ms(ev, eng.stream_handle(), lambda: eng.predict(ds["R"]), a.reps, a.warmup)
                _, F = eng.predict(ds["R"])
            lib_path = a.operator_lib or _native.LIB_PATH
            o_ms, form, bhash, y = operator_ms(lib_path, Rd, Rdd, alphas, 9, ev, a.reps, a.warmup)
            print(json.dumps({
                "leg": "ratio_predict_Q_eq_M_over_matvec", "M": int(M), "predict_us": p_ms * 1e3,
                "matvec_us": o_ms * 1e3, "ratio": p_ms / o_ms, "operator_form": form,
                "operator_lib_build_hash": bhash, "predict_lib_build_hash": _native.build_hash(),
                "max_abs_dF_over_max_abs_F": float(np.max(np.abs(F.ravel() - y)) / np.max(np.abs(y)))}),
                flush=True)
    if "nanotube" in a.legs:
        ds = synthetic.nanotube_like(141, seed=0)
        model, _, _, _ = build_model(ds, 2, a.energy_constraints)
        predict_leg("nanotube_like", ds, model, [1, 16], "stream", ev, a.reps, a.warmup)


if __name__ == "__main__":
    main()
