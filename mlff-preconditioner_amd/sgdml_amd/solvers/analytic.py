"""Drop-in for the reference's closed-form solver, `sgdml.solvers.analytic.Analytic`
(src/sGDML/sgdml/solvers/analytic.py:47-208), with assembly, factorisation and solve on the
MI355X:

    K = _assemble_kernel_mat(..., use_E_cstr)      -> KernelSolver.assemble_sgdml
    K[diag] -= 1e-10                               (whatever task['lam'] says, :136)
    alphas = -cho_solve(cho_factor(-K), y)         -> KernelSolver.dense_cho_solve(y, -1, 1e-10)

The reference's three progress messages go through `callback` as it sends them.  Not covered:
symmetry compression (`cprsn_keep_atoms_idxs`, the least-squares path of a non-square K), the LU
fallback after a failed Cholesky factorisation, `return_K`, several devices.
"""
from __future__ import annotations

import timeit
from functools import partial

import numpy as np

from ..solver import KernelSolver
from .iterative_solver import DONE, NOT_DONE

SHIFT = 1e-10  # analytic.py:136


class Analytic(object):
    def __init__(self, gdml_train, desc, callback=None, device=None):
        self.gdml_train = gdml_train
        self.desc = desc
        self.callback = callback
        self.device = device
        self.solver = None   # KernelSolver of the last solve (kept for the training-set energies)
        self.seconds = None  # device seconds of its copy / factorisation / triangular solves

    def close(self):
        """Release the device context of the last solve (a new solve does so too)."""
        solver, self.solver = self.solver, None
        if solver is not None:
            solver.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def solve(self, task, R_desc, R_d_desc, tril_perms_lin, y):
        if "cprsn_keep_atoms_idxs" in task:
            raise NotImplementedError("symmetry compression (cprsn_keep_atoms_idxs) is not "
                                      "supported by the closed-form solve on the device")
        sig = float(task["sig"])
        use_E_cstr = bool(task["use_E_cstr"])
        R_desc, R_d_desc = np.asarray(R_desc), np.asarray(R_d_desc)
        n_train, dim_d = R_d_desc.shape[:2]
        n_atoms = int((1 + np.sqrt(8 * dim_d + 1)) / 2)
        n = 3 * n_atoms * n_train + (n_train if use_E_cstr else 0)
        y = np.ascontiguousarray(y, dtype=np.float64)
        if y.shape != (n,):
            raise ValueError(f"y has {y.size} entries, the system {n}")
        perms = np.atleast_2d(np.asarray(task["perms"]))
        if len(tril_perms_lin) != perms.shape[0] * dim_d:
            raise ValueError("tril_perms_lin does not match task['perms']")

        self.close()
        self.solver = s = KernelSolver(n, device=self.device)
        cb = self.callback
        if cb is not None:  # :78-93, the messages of _assemble_kernel_mat (train.py:1265, 1301)
            cb = partial(cb, disp_str="Assembling kernel matrix")
            cb(0, 100)
        t0 = timeit.default_timer()
        s.assemble_sgdml(R_desc, R_d_desc, perms, sig, use_E_cstr=use_E_cstr)
        s.synchronize()
        if cb is not None:
            dur_s = timeit.default_timer() - t0
            cb(DONE, sec_disp_str="took {:.1f} s".format(dur_s) if dur_s >= 0.1 else "")

        start = timeit.default_timer()
        if cb is not None:  # :138-143
            cb = partial(cb, disp_str="Solving linear system (Cholesky factorization)")
            cb(NOT_DONE)
        try:
            x, self.seconds = s.dense_cho_solve(y, sigma_K=-1.0, shift=SHIFT, want_seconds=True)
        except np.linalg.LinAlgError as e:
            raise np.linalg.LinAlgError(
                f"{e} -- the reference falls back to an LU factorisation here "
                "(analytic.py:154-167); the device path has no such fallback") from e
        alphas = -x  # :151
        if cb is not None:  # :197-204
            dur_s = (timeit.default_timer() - start) / 2
            cb(DONE, disp_str="Training on {:,} points".format(n_train),
               sec_disp_str="took {:.1f} s".format(dur_s) if dur_s >= 0.1 else "")
        return alphas
