"""NumPy oracle for the analytic Hessian of a trained sGDML model (csrc/kernels_predict_hess.hip,
GDMLPredict.hessian).  A plain module: no fixtures, no pytest hooks.  The reference
implementation has no Hessian, so this oracle stands on two anchors
(tests/test_hessian_oracle.py): its forces reproduce the reference's golden predictions, and its
long-double Hessian equals minus the Richardson central difference of its long-double forces.

Notation of csrc/kernels_predict.hip.  For a query with descriptor rd (D = n (n - 1) / 2 inverse
distances, pairs in np.tril_indices order) and every permuted training row jp:
    diff = rd - Rt[jp],  z = Zt[jp],  e = alphas_E[j] (0 without energy constraints)
    nrm = sqrt5 |diff|,  x = nrm / sig,  a = diff . z
    m = exp(-x) 5 / (3 sig^4),  w = (sig^2 + sig nrm) m
    E_q = sum a w + e K_ee,  K_ee = (1 + x (1 + nrm / (3 sig))) exp(-x)
    Fd  = sum (5 m a + e w) diff - w z = -dE_q / drd
    G   = d2E_q / drd2 = sum -5 m (z diff^T + diff z^T) - (5 m a + e w) I + (beta + 5 m e) diff diff^T
    beta = 25 m a / (sig nrm) for nrm > 0, 0 for nrm = 0 (the limit: a = O(nrm))
With J = drd / dR (row (a, b), a > b, v = R_a - R_b, r = |v|: -v / r^3 in the columns of a,
+v / r^3 in those of b) and g = -Fd:
    E = std E_q + c,  F = std J^T Fd
    H = std [J^T G J + sum_d g_d d2rd_d / dR2],
d2(1 / r) / dR2 = +B at the blocks (a, a), (b, b) and -B at (a, b), (b, a), B = (3 v v^T / r^2 - I) / r^3.

`model_arrays` is what sgdml_amd.predict.load_model_arrays returns (R_desc M x D, R_d_desc_alpha
M x D, perms, sig, std, c, optionally alphas_E); every function evaluates in `dtype` (float64 or
np.longdouble) with the operands widened before the first operation.
"""
from __future__ import annotations

import numpy as np

from oracle import sgdml as osg

EXPLICIT_G_MAX_D = 512


def _model(ma, dtype):
    """(Rt, Zt, Et: MP x D, MP x D, MP or None; sig, std, c) in dtype."""
    Rd = np.asarray(ma["R_desc"], dtype=dtype)
    Z = np.asarray(ma["R_d_desc_alpha"], dtype=dtype)
    M, D = Rd.shape
    n = int((1 + np.sqrt(8 * D + 1)) / 2)
    perms = np.atleast_2d(np.asarray(ma["perms"]))
    P = np.array([osg.desc_perm(p) for p in perms]).reshape(perms.shape[0], D)
    Rt = Rd[:, P].reshape(-1, D)           # row jp = j n_perms + p: Rd_j[P_p]
    Zt = Z[:, P].reshape(-1, D)
    aE = ma.get("alphas_E")
    Et = None if aE is None else np.repeat(np.asarray(aE, dtype=dtype), perms.shape[0])
    return n, Rt, Zt, Et, dtype(ma["sig"]), dtype(ma.get("std", 1.0)), dtype(ma["c"])


def _geometries(R, n, dtype):
    R = np.asarray(R, dtype=dtype)
    return R.reshape(-1, n, 3)


def _pair_scalars(rd, Rt, Zt, Et, sig, dtype):
    diff = rd[None, :] - Rt
    nrm = np.sqrt(dtype(5)) * np.sqrt(np.sum(diff * diff, axis=1))
    x = nrm / sig
    ex = np.exp(-x)
    m = ex * 5 / (3 * sig ** 4)
    w = (sig ** 2 + sig * nrm) * m
    a = np.sum(diff * Zt, axis=1)
    e = np.zeros_like(a) if Et is None else Et
    kee = (1 + x * (1 + nrm / (3 * sig))) * ex
    return diff, nrm, m, w, a, e, kee


def _jacobian(r, dtype):
    """J = drd / dR (D x 3n) of one geometry r (n x 3) and the pair data (a, b, v, dist)."""
    n = r.shape[0]
    a, b = np.tril_indices(n, k=-1)
    v = r[a] - r[b]
    dist = np.sqrt(np.sum(v * v, axis=1))
    J = osg.d_desc_from_comp(v / (dist ** 3)[:, None], n)
    return J, a, b, v, dist


def energy_forces(model_arrays, R, dtype=np.float64):
    """E (Q,), F (Q, 3n) of the geometries R (Q x n x 3 or Q x 3n)."""
    n, Rt, Zt, Et, sig, std, c = _model(model_arrays, dtype)
    R = _geometries(R, n, dtype)
    E = np.empty(R.shape[0], dtype=dtype)
    F = np.empty((R.shape[0], 3 * n), dtype=dtype)
    for q, r in enumerate(R):
        J, _, _, _, dist = _jacobian(r, dtype)
        diff, nrm, m, w, a, e, kee = _pair_scalars(1 / dist, Rt, Zt, Et, sig, dtype)
        Fd = (5 * m * a + e * w) @ diff - w @ Zt
        E[q] = std * (np.sum(a * w) + np.sum(e * kee)) + c
        F[q] = std * (J.T @ Fd)
    return E, F


def hessian(model_arrays, R, dtype=np.float64, explicit_G=None):
    """H (Q, 3n, 3n) = d2E / dR2.  explicit_G: form the D x D matrix G and J^T G J as written
    (default for D <= EXPLICIT_G_MAX_D); otherwise G J is formed term by term from the same
    formula without storing G (D = 3655 at 86 atoms makes G 13 M entries)."""
    n, Rt, Zt, Et, sig, std, c = _model(model_arrays, dtype)
    R = _geometries(R, n, dtype)
    D = Rt.shape[1]
    if explicit_G is None:
        explicit_G = D <= EXPLICIT_G_MAX_D
    H = np.empty((R.shape[0], 3 * n, 3 * n), dtype=dtype)
    eye3 = np.eye(3, dtype=dtype)
    for q, r in enumerate(R):
        J, pa, pb, v, dist = _jacobian(r, dtype)
        diff, nrm, m, w, a, e, _ = _pair_scalars(1 / dist, Rt, Zt, Et, sig, dtype)
        pos = nrm > 0
        beta = np.zeros_like(nrm)
        beta[pos] = 25 * m[pos] * a[pos] / (sig * nrm[pos])
        cdd = beta + 5 * m * e                     # coefficient of diff diff^T
        cI = np.sum(5 * m * a + e * w)             # coefficient of -I
        zm = (5 * m)[:, None] * Zt
        if explicit_G:
            G = -(zm.T @ diff) - (diff.T @ zm) + (diff * cdd[:, None]).T @ diff
            G[np.diag_indices(D)] -= cI
            GJ = G @ J
            Hq = J.T @ GJ
        else:
            def jt(X):                             # J^T X from the 6 non-zeros of every row of J
                c3 = (v / (dist ** 3)[:, None])[:, :, None] * X[:, None, :]
                out = np.zeros((n, 3, X.shape[1]), dtype=dtype)
                np.add.at(out, pb, c3)
                np.add.at(out, pa, -c3)
                return out.reshape(3 * n, X.shape[1])

            dJ, zJ = jt(diff.T).T, jt(zm.T).T      # MP x 3n
            GJ = -(zm.T @ dJ) - (diff.T @ zJ) + (diff * cdd[:, None]).T @ dJ - cI * J
            Hq = jt(GJ)
        # sum_d g_d d2rd_d / dR2, g = -Fd
        g = -((5 * m * a + e * w) @ diff - w @ Zt)
        B = (3 * v[:, :, None] * v[:, None, :] / (dist ** 2)[:, None, None] - eye3) / (dist ** 3)[:, None, None]
        B = B * g[:, None, None]
        Hb = np.zeros((n, n, 3, 3), dtype=dtype)
        np.add.at(Hb, (pa, pa), B)
        np.add.at(Hb, (pb, pb), B)
        np.add.at(Hb, (pa, pb), -B)
        np.add.at(Hb, (pb, pa), -B)
        H[q] = std * (Hq + Hb.transpose(0, 2, 1, 3).reshape(3 * n, 3 * n))
    return H


def fd_hessian(model_arrays, r, h, dtype):
    """-(Richardson central difference of the forces), (4 D_h - D_2h) / 3, of one geometry r."""
    n3 = np.asarray(r).size
    r = np.asarray(r, dtype=dtype).reshape(-1)

    def central(step):
        disp = np.repeat(r[None, :], 2 * n3, axis=0)
        disp[np.arange(n3), np.arange(n3)] += step
        disp[n3 + np.arange(n3), np.arange(n3)] -= step
        _, F = energy_forces(model_arrays, disp, dtype)
        return (F[:n3] - F[n3:]) / (2 * step)      # [i, k] = dF_k / dR_i

    h = dtype(h)
    return -(4 * central(h) - central(2 * h)) / 3


def random_model(n, M, kind, seed, alphas_E=False, sig=10.0, std=1.0, c=0.0):
    """A model of sgdml_shapes.molecule / perm_set with random alphas_F through the project's host
    code, as the GPU tests build it: (model dict with the reference's keys, training geometries)."""
    from sgdml_amd.model import r_d_desc_alpha
    from sgdml_amd.solver import host_descriptors
    from tests import sgdml_shapes as sh

    Rtr = sh.molecule(n, M, seed)
    rng = np.random.default_rng(seed + 11)
    Rd, Rdd = host_descriptors(Rtr)
    model = {"type": "m", "z": np.ones(n, dtype=np.int64), "perms": sh.perm_set(n, kind), "sig": sig,
             "std": std, "c": c, "R_desc": Rd.T,
             "R_d_desc_alpha": r_d_desc_alpha(Rdd, rng.standard_normal(3 * n * M))}
    if alphas_E:
        model["alphas_E"] = rng.standard_normal(M)
    return model, Rtr
