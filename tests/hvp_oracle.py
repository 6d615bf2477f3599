"""NumPy oracle for Hessian-vector products of a trained sGDML model (csrc/kernels_predict_hvp.hip,
GDMLPredict.hessian_vector).  A plain module: no fixtures, no pytest hooks.  It evaluates the
matrix-free formulas, never the Hessian, and is anchored on the CPU in tests/test_hvp_oracle.py:
its long-double result equals the Hessian oracle's (tests/hessian_oracle.py) matrix times the
vector, and minus the Richardson central difference of that oracle's forces along the vector.

Notation of tests/hessian_oracle.py.  For a query with descriptor rd, compact Jacobian
Rdd_d = (R_a - R_b) / r^3 of the pair d = (a, b), a > b, and a vector v (3n):
    y = J v,  y_d = Rdd_d . (v_b - v_a)
and over the permuted training rows jp (diff, z = Zt[jp], e, m, w, a, beta as in the Hessian oracle):
    bb = diff . y,  cc = z . y
    Gy = sum_jp ((beta + 5 m e) bb - 5 m cc) diff - (5 m bb) z  -  (sum_jp 5 m a + e w) y
    Fd = sum_jp (5 m a + e w) diff - w z,  g = -Fd
    H v = std [J^T Gy + sum_d g_d (+B_d (v_a - v_b) at atom a, -B_d (v_a - v_b) at atom b)],
    B_d u = 3 Rdd_d (Rdd_d . u) / rd_d - rd_d^3 u.
"""
from __future__ import annotations

import numpy as np

from tests.hessian_oracle import _jacobian, _model, _pair_scalars, random_model  # noqa: F401


def hvp(model_arrays, R, V, dtype=np.float64):
    """HV (Q, K, 3n) = H(R_q) V[q, k] of the geometries R (Q x n x 3 or Q x 3n) and the vectors
    V (Q x K x 3n or Q x 3n), evaluated in dtype without forming H or the D x D matrix G."""
    n, Rt, Zt, Et, sig, std, _ = _model(model_arrays, dtype)
    R = np.asarray(R, dtype=dtype).reshape(-1, n, 3)
    Q = R.shape[0]
    V = np.asarray(V, dtype=dtype).reshape(Q, -1, 3 * n)
    HV = np.empty(V.shape, dtype=dtype)
    for q, r in enumerate(R):
        _, pa, pb, vec, dist = _jacobian(r, dtype)
        rd = 1 / dist
        rdd = vec / (dist ** 3)[:, None]                      # D x 3
        diff, nrm, m, w, a, e, _ = _pair_scalars(rd, Rt, Zt, Et, sig, dtype)
        pos = nrm > 0
        beta = np.zeros_like(nrm)
        beta[pos] = 25 * m[pos] * a[pos] / (sig * nrm[pos])
        cdd = beta + 5 * m * e
        ci = 5 * m * a + e * w
        g = -(ci @ diff - w @ Zt)
        for k in range(V.shape[1]):
            v = V[q, k].reshape(n, 3)
            y = np.sum(rdd * (v[pb] - v[pa]), axis=1)
            bb, cc = diff @ y, Zt @ y
            Gy = (cdd * bb - 5 * m * cc) @ diff - (5 * m * bb) @ Zt - np.sum(ci) * y
            out = np.zeros((n, 3), dtype=dtype)
            np.add.at(out, pb, rdd * Gy[:, None])             # J^T Gy: -Rdd at atom a, +Rdd at atom b
            np.add.at(out, pa, -rdd * Gy[:, None])
            u = v[pa] - v[pb]
            Bu = 3 * rdd * (np.sum(rdd * u, axis=1) / rd)[:, None] - (rd ** 3)[:, None] * u
            np.add.at(out, pa, g[:, None] * Bu)
            np.add.at(out, pb, -g[:, None] * Bu)
            HV[q, k] = std * out.reshape(-1)
    return HV
