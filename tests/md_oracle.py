"""NumPy oracle for velocity-Verlet trajectories of a trained sGDML model (csrc/kernels_md.hip,
GDMLPredict.md).  A plain module: no fixtures, no pytest hooks.  The reference implementation has
no trajectory runner; the forces are those of tests/hessian_oracle.energy_forces (anchored in
tests/test_hessian_oracle.py), the integrator is anchored in tests/test_md_oracle.py by its order
and its reversibility.

With h_i = (0.5 dt acc_unit) / m_i a step is
    v += h_i F;  R += dt v;  E, F = the model at R;  v += h_i F,
and the frames of the steps 0, stride, ..., steps hold R, V, E(R) and F(R) of one instant.
Everything is evaluated in `dtype` (float64 or np.longdouble), the operands widened first.
"""
from __future__ import annotations

import numpy as np

from tests import hessian_oracle as ho

# standard atomic weights of the elements the golden models contain
MASS_OF_Z = {1: 1.008, 6: 12.011, 7: 14.007, 8: 15.999}


def verlet(model_arrays, R0, V0, masses, dt, steps, stride, acc_unit, dtype=np.float64):
    """{"R": (Q, T, n, 3), "V": (Q, T, n, 3), "E": (Q, T), "F": (Q, T, 3n), "step": (T,)} of the Q
    replicas R0 (Q x n x 3 or Q x 3n) with velocities V0 (the same shapes), T = steps / stride + 1."""
    masses = np.asarray(masses, dtype=dtype)
    n = masses.size
    R = np.array(R0, dtype=dtype).reshape(-1, 3 * n)
    V = np.array(V0, dtype=dtype).reshape(-1, 3 * n)
    assert R.shape == V.shape and steps >= 0 and stride >= 1 and steps % stride == 0
    h = np.repeat((dtype(0.5) * dtype(dt) * dtype(acc_unit)) / masses, 3)
    dt = dtype(dt)
    Q, T = R.shape[0], steps // stride + 1
    out = {"R": np.empty((Q, T, n, 3), dtype=dtype), "V": np.empty((Q, T, n, 3), dtype=dtype),
           "E": np.empty((Q, T), dtype=dtype), "F": np.empty((Q, T, 3 * n), dtype=dtype),
           "step": np.arange(T, dtype=np.int64) * stride}
    E, F = ho.energy_forces(model_arrays, R, dtype)
    for k in range(steps + 1):
        if k > 0:
            V = V + h * F
            R = R + dt * V
            E, F = ho.energy_forces(model_arrays, R, dtype)
            V = V + h * F
        if k % stride == 0:
            t = k // stride
            out["R"][:, t] = R.reshape(Q, n, 3)
            out["V"][:, t] = V.reshape(Q, n, 3)
            out["E"][:, t] = E
            out["F"][:, t] = F
    return out


def start(n, M, kind, ecstr, Q, seed):
    """(model, model arrays, R0 Q x n x 3, V0 Q x n x 3, masses) of a shape of sgdml_shapes.TABLE:
    the model of hessian_oracle.random_model(n, M, kind, 1000 n + M, std 1.75, c -3), training
    geometries plus 0.05 N(0, 1), velocities 0.01 N(0, 1) Angstrom / fs, masses uniform in [1, 16]."""
    from sgdml_amd.predict import load_model_arrays

    model, Rtr = ho.random_model(n, M, kind, 1000 * n + M, alphas_E=ecstr, std=1.75, c=-3.0)
    rng = np.random.default_rng(seed)
    R0 = Rtr[np.arange(Q) % M] + 0.05 * rng.standard_normal((Q, n, 3))
    V0 = 0.01 * rng.standard_normal((Q, n, 3))
    masses = rng.uniform(1.0, 16.0, n)
    for a in (R0, V0, masses):
        a.setflags(write=False)
    return model, load_model_arrays(model, energy_constraints=True), R0, V0, masses
