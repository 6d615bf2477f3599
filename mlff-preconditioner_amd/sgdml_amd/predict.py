"""GDMLPredict: energies and forces of a trained sGDML model at new geometries, on the MI355X.

Drop-in for the reference's `sgdml.predict.GDMLPredict` (src/sGDML/sgdml/predict.py:237-384,
997-1110) for models without lattice or cut-off, with or without energy constraints (`alphas_E`
of a model trained with `use_E_cstr`, predict.py:206-218):

    with GDMLPredict("model.npz") as gdml:      # or a model dict / an open np.load result
        E, F = gdml.predict(R)                  # R: Q x 3n, Q x n x 3, 3n or n x 3

The model arrays go to the device once (`mlff_predict_set_model`,
`mlff_predict_set_energy_coefficients`); every `predict` call sends
the geometries and gets E (Q,) and F (Q, 3n) back (`mlff_predict`, csrc/kernels_predict.hip).
A query's result has the same bits whatever batch it is part of, so splitting a batch over
`devices=[...]` (contiguous blocks, one context and one thread per entry) changes nothing.

`gdml.hessian(R)` returns the analytic second derivative d2E / dR2, (Q, 3n, 3n), with the same
guarantees (`mlff_predict_hessian`, csrc/kernels_predict_hess.hip); the reference has none.
`gdml.hessian_vector(R, V)` returns the products of that matrix with one or K vectors per
geometry without forming it (`mlff_predict_hvp`, csrc/kernels_predict_hvp.hip), for any number of
atoms.

`gdml.md(R0, V0, masses, dt, steps)` runs velocity-Verlet trajectories of Q independent replicas
with positions, velocities and forces kept on the device for the whole run (`mlff_md_run`,
csrc/kernels_md.hip); the recorded frames equal, bit for bit, those of a host loop over `predict`.
"""
from __future__ import annotations

import operator
import os
import threading

import numpy as np

from .sharded import _Worker
from .solver import KernelSolver

# queries per workgroup of the pair stage (csrc/kernels_predict.hip: kPrThreads / L of the
# variant that covers D; kPrQB of the stream form)
STREAM_QUERY_BLOCK = 4
TILE_MAX_D = 288


def tile_queries_per_workgroup(D: int) -> int:
    """G of the tile form for descriptor length D (k_pr_pair<L, DL>: 128 / L queries)."""
    for L, DL in ((2, 18), (4, 18), (4, 28), (8, 28), (8, 36)):
        if D <= L * DL:
            return 128 // L
    raise ValueError(f"the tile form covers D <= {TILE_MAX_D}, got {D}")


def _scalar(v, name):
    a = np.asarray(v)
    if a.size != 1:
        raise ValueError(f"model['{name}'] must be a scalar, got shape {a.shape}")
    return float(a.reshape(()))


def _has(model, key):
    files = getattr(model, "files", None)
    return key in files if files is not None else key in model


def load_model_arrays(model, energy_constraints: bool = False) -> dict:
    """The arrays the predictor needs from a model dict, an open `np.load` result or the path
    of a `.npz` (written by `store_model` or by the reference): sig, std, c, R_desc (stored
    D x M, returned M x D), R_d_desc_alpha (M x D), perms (n_perms x n), z.  Scalars may be
    0-d arrays.  Only these keys are read, so pickled entries of the file are never loaded.
    A model with `alphas_E` is refused unless `energy_constraints` is set; then the result also
    has "alphas_E": a contiguous float64 (M,) array, or None for a model without the key."""
    opened = None
    if isinstance(model, (str, os.PathLike)):
        opened = model = np.load(model, allow_pickle=False)
    try:
        if _has(model, "type"):
            t = np.asarray(model["type"]).reshape(-1)[0]
            if t not in ("m", b"m"):
                raise ValueError("the provided data structure is not a model (type != 'm')")
        if _has(model, "lattice"):
            raise NotImplementedError("models with a periodic lattice are not supported")
        if not energy_constraints and _has(model, "alphas_E"):
            raise NotImplementedError("models with energy constraints (alphas_E) are not supported")
        if _has(model, "interact_cut_off"):
            try:
                cut = model["interact_cut_off"]
            except ValueError:  # a pickled None in a .npz opened without pickle support
                cut = None
            if cut is not None and np.asarray(cut).dtype != object:
                raise NotImplementedError("models with an interaction cut-off are not supported")
        for key in ("sig", "c", "R_desc", "R_d_desc_alpha", "perms", "z"):
            if not _has(model, key):
                raise ValueError(f"model has no '{key}'")
        z = np.asarray(model["z"]).reshape(-1)
        n = z.size
        D = n * (n - 1) // 2
        perms = np.ascontiguousarray(np.atleast_2d(np.asarray(model["perms"])), dtype=np.int32)
        R_desc = np.asarray(model["R_desc"], dtype=np.float64)
        Rda = np.asarray(model["R_d_desc_alpha"], dtype=np.float64)
        if n < 2:
            raise ValueError("model['z'] must list at least two atoms")
        if perms.ndim != 2 or perms.shape[1] != n:
            raise ValueError(f"model['perms'] must be n_perms x {n}, got {perms.shape}")
        if R_desc.ndim != 2 or R_desc.shape[0] != D:
            raise ValueError(f"model['R_desc'] must be {D} x M (D = n (n - 1) / 2), got {R_desc.shape}")
        M = R_desc.shape[1]
        if M < 1 or Rda.shape != (M, D):
            raise ValueError(f"model['R_d_desc_alpha'] must be {M} x {D}, got {Rda.shape}")
        if not np.array_equal(np.sort(perms, axis=1), np.broadcast_to(np.arange(n), perms.shape)):
            raise ValueError("model['perms']: every row must be a permutation of the atoms")
        out = {}
        if energy_constraints:
            out["alphas_E"] = None
            if _has(model, "alphas_E"):
                aE = np.asarray(model["alphas_E"])
                if aE.shape != (M,):
                    raise ValueError(f"model['alphas_E'] must have shape ({M},), got {aE.shape}")
                out["alphas_E"] = np.ascontiguousarray(aE, dtype=np.float64)
        out.update({
            "sig": _scalar(model["sig"], "sig"),
            "std": _scalar(model["std"], "std") if _has(model, "std") else 1.0,
            "c": _scalar(model["c"], "c"),
            "R_desc": np.ascontiguousarray(R_desc.T),
            "R_d_desc_alpha": np.ascontiguousarray(Rda),
            "perms": perms,
            "z": z.copy(),
        })
        return out
    finally:
        if opened is not None:
            opened.close()


def normalize_geometries(R, n_atoms: int) -> np.ndarray:
    """R as Q x 3n, Q x n x 3, or one geometry 3n / n x 3  ->  contiguous Q x n x 3."""
    R = np.asarray(R, dtype=np.float64)
    n3 = 3 * n_atoms
    if R.ndim == 1 and R.size == n3:
        R = R.reshape(1, n_atoms, 3)
    elif R.ndim == 2 and R.shape == (n_atoms, 3):
        R = R.reshape(1, n_atoms, 3)
    elif R.ndim == 2 and R.shape[1] == n3:
        R = R.reshape(R.shape[0], n_atoms, 3)
    elif R.ndim == 3 and R.shape[1:] == (n_atoms, 3):
        pass
    else:
        raise ValueError(f"R must be Q x {n3}, Q x {n_atoms} x 3, {n3} or {n_atoms} x 3; got {R.shape}")
    return np.ascontiguousarray(R)


# Angstrom fs^-2 per kcal mol^-1 Angstrom^-1 amu^-1: 4184 J/mol over 1e-10 m over 1e-3 kg/mol is
# 4.184e16 m s^-2 = 4.184e-4 Angstrom fs^-2
ACC_KCAL_MOL_A_AMU_FS = 4.184e-4


def normalize_md_inputs(R0, V0, masses, dt, steps, stride, n_atoms: int):
    """The inputs of `GDMLPredict.md`, checked on the host: (R0 as Q x n x 3, V0 as Q x 3n, masses
    (n,), dt, steps, stride).  R0: the shapes `predict` accepts; V0: Q x 3n, Q x n x 3 or, for one
    geometry, 3n / n x 3; masses finite and > 0; dt finite; steps >= 0 a multiple of stride >= 1.
    ValueError otherwise."""
    R = normalize_geometries(R0, n_atoms)
    Q, n3 = R.shape[0], 3 * n_atoms
    V = np.asarray(V0, dtype=np.float64)
    if V.shape in ((Q, n3), (Q, n_atoms, 3)) or (Q == 1 and V.shape in ((n3,), (n_atoms, 3))):
        V = np.ascontiguousarray(V.reshape(Q, n3))
    else:
        raise ValueError(f"V0 must be {Q} x {n3} or {Q} x {n_atoms} x 3 for these {Q} geometries "
                         f"(or {n3} / {n_atoms} x 3 for one); got {V.shape}")
    m = np.asarray(masses, dtype=np.float64)
    if m.shape != (n_atoms,):
        raise ValueError(f"masses must have shape ({n_atoms},), got {m.shape}")
    if not (np.all(np.isfinite(m)) and np.all(m > 0)):
        raise ValueError("masses must be finite and > 0")
    try:
        dt = float(dt)
    except (TypeError, ValueError):
        raise ValueError(f"dt must be a number, got {dt!r}") from None
    if not np.isfinite(dt):
        raise ValueError(f"dt must be finite, got {dt}")
    try:
        steps, stride = operator.index(steps), operator.index(stride)
    except TypeError:
        raise ValueError(f"steps and stride must be integers, got {steps!r}, {stride!r}") from None
    if steps < 0:
        raise ValueError(f"steps must be >= 0, got {steps}")
    if stride < 1:
        raise ValueError(f"stride must be >= 1, got {stride}")
    if steps % stride != 0:
        raise ValueError(f"steps must be a multiple of stride, got {steps} and {stride}")
    return R, V, np.ascontiguousarray(m), dt, steps, stride


def kinetic_energy(V, masses, acc_unit: float = ACC_KCAL_MOL_A_AMU_FS) -> np.ndarray:
    """0.5 sum_i m_i |v_i|^2 / acc_unit of every frame, in the model's energy unit, on the host.
    V: (..., n, 3) or (..., 3n), as `md` returns it; the result has the leading shape (float64;
    long double where V or the masses are)."""
    wide = any(np.asarray(a).dtype == np.longdouble for a in (V, masses))  # an oracle's frames
    m = np.asarray(masses, dtype=np.longdouble if wide else np.float64)
    V = np.asarray(V, dtype=m.dtype)
    n = m.size
    if V.ndim >= 2 and V.shape[-2:] == (n, 3):
        V = V.reshape(V.shape[:-2] + (3 * n,))
    elif V.ndim < 1 or V.shape[-1] != 3 * n:
        raise ValueError(f"V must end in {n} x 3 or {3 * n}, got {V.shape}")
    return 0.5 * np.sum(np.repeat(m, 3) * V * V, axis=-1) / acc_unit


def split_blocks(Q: int, parts: int) -> list[tuple[int, int]]:
    """Contiguous blocks [a, b) of Q queries for `parts` workers (blocks may be empty)."""
    per = -(-Q // parts) if Q > 0 else 0
    return [(min(r * per, Q), min((r + 1) * per, Q)) for r in range(parts)]


class GDMLPredict:
    def __init__(self, model, device: int | None = None, devices=None):
        arrs = load_model_arrays(model, energy_constraints=True)
        self.n_atoms = arrs["z"].size
        self.n_train = arrs["R_desc"].shape[0]
        self.n_perms = arrs["perms"].shape[0]
        self.sig, self.std, self.c = arrs["sig"], arrs["std"], arrs["c"]
        self.use_E_cstr = arrs["alphas_E"] is not None
        self._lock = threading.Lock()
        self._workers = None
        self._engines: list[KernelSolver] = []
        n_global = 3 * self.n_atoms * self.n_train

        def make(dev):
            s = KernelSolver(n_global, device=dev)
            try:
                s.predict_set_model(arrs["R_desc"], arrs["R_d_desc_alpha"], arrs["perms"],
                                    self.sig, self.std, self.c, alphas_E=arrs["alphas_E"])
            except BaseException:
                s.close()
                raise
            return s

        if devices is None:
            self._engines = [make(device)]
        else:
            devices = [int(d) for d in devices]
            if not devices:
                raise ValueError("devices must name at least one device")
            self._workers = [_Worker(f"mlff-predict{r}-dev{d}") for r, d in enumerate(devices)]
            created: list[KernelSolver] = []

            def make_on(r):
                s = make(devices[r])
                created.append(s)
                return s

            try:
                self._engines = self._all(make_on)
            except BaseException:
                self._engines = created  # those that were set up: released by close()
                self.close()
                raise
        form, slab, flops, nbytes = self._engines[0].predict_info()
        self.form, self.slab = form, slab
        self.flops_per_query, self.bytes_per_query = flops, nbytes

    def _all(self, fn):
        boxes, events = [], []
        for r, w in enumerate(self._workers):
            box, done = {}, threading.Event()
            w.q.put((lambda r=r: fn(r), box, done))
            boxes.append(box)
            events.append(done)
        for e in events:
            e.wait()
        for b in boxes:
            if "error" in b:
                raise b["error"]
        return [b.get("value") for b in boxes]

    def predict(self, R) -> tuple[np.ndarray, np.ndarray]:
        """GDMLPredict.predict (predict.py:997-1110): E (Q,), F (Q, 3 n_atoms)."""
        if not self._engines:
            raise RuntimeError("GDMLPredict is closed")
        R = normalize_geometries(R, self.n_atoms)
        Q = R.shape[0]
        if self._workers is None:
            return self._engines[0].predict(R)
        blocks = split_blocks(Q, len(self._engines))
        parts = self._all(lambda r: self._engines[r].predict(R[blocks[r][0]:blocks[r][1]]))
        return (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]))

    def hessian(self, R) -> np.ndarray:
        """The analytic Hessian d2E / dR2 at the geometries R (the shapes `predict` accepts):
        (Q, 3 n_atoms, 3 n_atoms) in the model's [E] / [R]^2, each H[q] exactly symmetric
        (`mlff_predict_hessian`, csrc/kernels_predict_hess.hip).  The reference has no Hessian;
        the bits of a query's result do not depend on the batch or on the device split."""
        if not self._engines:
            raise RuntimeError("GDMLPredict is closed")
        R = normalize_geometries(R, self.n_atoms)
        if self._workers is None:
            return self._engines[0].predict_hessian(R)
        blocks = split_blocks(R.shape[0], len(self._engines))
        parts = self._all(lambda r: self._engines[r].predict_hessian(R[blocks[r][0]:blocks[r][1]]))
        return np.concatenate(parts)

    def hessian_vector(self, R, V) -> np.ndarray:
        """Hessian-vector products H(R_q) V[q] without forming H (`mlff_predict_hvp`,
        csrc/kernels_predict_hvp.hip): what `hessian(R) @ v` gives, at about a quarter of the
        arithmetic per vector and with no limit on the number of atoms.  R: the shapes `predict`
        accepts.  V: one vector per geometry, (Q, 3n) or (Q, n, 3), giving (Q, 3n); or K vectors
        per geometry, (Q, K, 3n) or (Q, K, n, 3), giving (Q, K, 3n).  The K vectors of a geometry
        share the pass over the training set.  The bits of a product do not depend on the batch,
        on K, on the vector's position or on the device split."""
        if not self._engines:
            raise RuntimeError("GDMLPredict is closed")
        R = normalize_geometries(R, self.n_atoms)
        Q, n, n3 = R.shape[0], self.n_atoms, 3 * self.n_atoms
        V = np.asarray(V, dtype=np.float64)
        if V.shape in ((Q, n3), (Q, n, 3)):
            single, V = True, V.reshape(Q, 1, n3)
        elif V.ndim >= 3 and V.shape[0] == Q and V.shape[2:] in ((n3,), (n, 3)):
            single, V = False, V.reshape(Q, V.shape[1], n3)
        else:
            raise ValueError(f"V must be {Q} x {n3}, {Q} x {n} x 3, {Q} x K x {n3} or {Q} x K x {n} x 3 "
                             f"for these {Q} geometries; got {V.shape}")
        V = np.ascontiguousarray(V)
        if self._workers is None:
            HV = self._engines[0].predict_hvp(R, V)
        else:
            blocks = split_blocks(Q, len(self._engines))
            HV = np.concatenate(self._all(
                lambda r: self._engines[r].predict_hvp(R[blocks[r][0]:blocks[r][1]], V[blocks[r][0]:blocks[r][1]])))
        return HV[:, 0] if single else HV

    def md(self, R0, V0, masses, dt, steps, stride=1, acc_unit=ACC_KCAL_MOL_A_AMU_FS, forces=False,
           launches=None) -> dict:
        """Velocity-Verlet trajectories of Q independent replicas on the device (`mlff_md_run`,
        csrc/kernels_md.hip): positions R0 (the shapes `predict` accepts), velocities V0 ((Q, 3n),
        (Q, n, 3), or one geometry's (3n,) / (n, 3)) in [R] per time unit, masses (n,), `steps`
        steps of dt.  `acc_unit` converts [E] / [R] / mass into [R] / time^2 (the default: kcal/mol,
        Angstrom, amu, fs).  With h_i = (0.5 dt acc_unit) / m_i a step is
            v += h_i F;  R += dt v;  E, F = predict(R);  v += h_i F,
        every product rounded before its sum, so the frames equal those of that loop over
        `predict` bit for bit; a replica's bits do not depend on the batch, the stride, a restart
        from a frame, or the device split.  Returns the frames of the steps 0, stride, ..., steps
        (T = steps / stride + 1): {"R": (Q, T, n, 3), "V": (Q, T, n, 3), "E": (Q, T), "step": (T,)}
        and "F": (Q, T, 3n) with `forces`; a frame holds R, V, E(R) and F(R) of one instant.
        Between flushes of the device's frame buffer nothing is copied and nothing waits.
        launches: 2 or 4 kernel launches per step instead of the model's default (2 needs a tile
        model); the same bits."""
        if not self._engines:
            raise RuntimeError("GDMLPredict is closed")
        R, V, m, dt, steps, stride = normalize_md_inputs(R0, V0, masses, dt, steps, stride, self.n_atoms)
        if launches not in (None, 0, 2, 4):
            raise ValueError(f"launches must be 2 or 4, got {launches!r}")
        h = (0.5 * dt * acc_unit) / m
        Q, n = R.shape[0], self.n_atoms
        T = steps // stride + 1

        def run(eng, a, b):
            eng.md_set_form(launches or 0)
            return eng.md_run(R[a:b], V[a:b], h, dt, steps, stride, forces)

        if self._workers is None:
            parts = [run(self._engines[0], 0, Q)]
        else:
            blocks = split_blocks(Q, len(self._engines))
            parts = self._all(lambda r: run(self._engines[r], *blocks[r]))
        out = {"R": np.concatenate([p[0] for p in parts]).reshape(Q, T, n, 3),
               "V": np.concatenate([p[1] for p in parts]).reshape(Q, T, n, 3),
               "E": np.concatenate([p[2] for p in parts]),
               "step": np.arange(T, dtype=np.int64) * stride}
        if forces:
            out["F"] = np.concatenate([p[3] for p in parts])
        return out

    def md_info(self) -> tuple[int, int, int]:
        """(kernel launches per step, frames the device's frame buffer holds, stream
        synchronisations of the last `md` on the first device: one per flush of that buffer)."""
        if not self._engines:
            raise RuntimeError("GDMLPredict is closed")
        if self._workers is None:
            return self._engines[0].md_info()
        return self._all(lambda r: self._engines[r].md_info())[0]

    def close(self):
        """Release the device contexts and stop the workers (idempotent)."""
        with self._lock:
            engines, self._engines = self._engines, []
            workers, self._workers = self._workers, None
        for s in engines:
            if s is not None:
                s.close()
        for w in workers or []:
            w.q.put(None)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass
