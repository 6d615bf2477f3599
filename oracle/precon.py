"""Low-rank preconditioners of the reference, restated in NumPy/SciPy.

TEST INFRASTRUCTURE (see oracle/__init__.py).

All functions work on S = sigma_K * K, the PSD matrix whose columns the
reference's pivoted Cholesky fetches (get_col of -K_op, iterative_cholesky.py:152-156)
and whose K_mm block it factors (`_cho_factor_stable(-K_mm)`, iterative_solver.py:218).
Preconditioner panels are returned "wide" (k x N) together with the sign
sigma_p of the apply z = sigma_p * lam^-1 * (r - T^T T r).
"""
from __future__ import annotations

import numpy as np
import scipy.linalg

# Every function takes dtype = np.float64 (the default: the reference's own arithmetic, bit for
# bit) or np.longdouble: the same formulas in extended precision, the high-precision reference of
# tests/precon_shapes.py.  SciPy takes no long double, so that path has its own Cholesky, forward
# substitution and Jacobi eigensolver below.  The discrete decisions (pivot order, sign of the
# 1e-15 shift) can be handed in, so that two evaluations of one case take the same.


def _is_f64(dtype):
    return np.dtype(dtype) == np.float64


def _cholesky_lower(A):
    """Lower Cholesky factor in A's own dtype, column by column."""
    A = np.array(A, copy=True)
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        if not d > 0:
            raise np.linalg.LinAlgError(f"{j + 1}-th leading minor is not positive definite")
        L[j, j] = np.sqrt(d)
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def _forward(L, B):
    """X with L X = B, L lower triangular, row by row."""
    X = np.array(B, dtype=L.dtype, copy=True)
    for i in range(L.shape[0]):
        X[i] = (X[i] - L[i, :i] @ X[:i]) / L[i, i]
    return X


def eigh_longdouble(S):
    """(w, V), S = V diag(w) V^T in long double, w ascending: float64 eigh, its V orthonormalised
    in long double (one Newton-Schulz step: 1e-16 -> 1e-32), V^T S V formed in long double, and
    cyclic Jacobi sweeps until the off-diagonal Frobenius norm is <= 2^-60 of the whole.  A sweep
    visits every pair once in round-robin order, the n / 2 disjoint rotations of a round at once."""
    LD = np.longdouble
    S = np.asarray(S, dtype=LD)
    n = S.shape[0]
    Vt = np.linalg.eigh(S.astype(np.float64))[1].astype(LD).T.copy()
    Vt = (LD(1.5) * np.eye(n, dtype=LD) - LD(0.5) * (Vt @ Vt.T)) @ Vt
    A = Vt @ S @ Vt.T
    A = (A + A.T) / 2
    whole = np.sqrt(np.sum(A * A))
    m = n + (n & 1)
    for _ in range(30):
        low = np.tril(A, -1)
        off = np.sqrt(2 * np.sum(low * low))
        if not off > LD(2.0) ** -60 * whole:
            break
        tiny = LD(2.0) ** -80 * whole
        ring = np.arange(m)
        for _round in range(m - 1):
            P, Q = ring[:m // 2], ring[m // 2:][::-1]
            keep = (P < n) & (Q < n)
            p, q = np.minimum(P, Q)[keep], np.maximum(P, Q)[keep]
            ring = np.concatenate([ring[:1], ring[-1:], ring[1:-1]])
            apq = A[p, q]
            turn = np.abs(apq) > tiny
            if not np.any(turn):
                continue
            p, q, apq = p[turn], q[turn], apq[turn]
            theta = (A[q, q] - A[p, p]) / (2 * apq)
            t = np.where(theta >= 0, LD(1), LD(-1)) / (np.abs(theta) + np.sqrt(theta * theta + 1))
            c = 1 / np.sqrt(t * t + 1)
            s = t * c
            for X in (A, A.T, Vt):           # rows, then columns of A; the eigenvectors
                Xp, Xq = X[p], X[q]
                X[p], X[q] = c[:, None] * Xp - s[:, None] * Xq, s[:, None] * Xp + c[:, None] * Xq
    else:
        raise np.linalg.LinAlgError("Jacobi sweeps did not converge")
    w = np.diag(A).copy()
    order = np.argsort(w, kind="stable")
    return w[order], Vt[order].T.copy()


def _svd_symmetric(S, dtype):
    """(U, s) of scipy.linalg.svd(S) for symmetric S: pairs ordered by |eigenvalue|, descending."""
    if _is_f64(dtype):
        U, s, _ = scipy.linalg.svd(S)
        return U, s
    w, V = eigh_longdouble(S)
    order = np.argsort(-np.abs(w), kind="stable")
    return V[:, order], np.abs(w[order])


def pivoted_cholesky(get_col, diagonal, max_rank, dtype=np.float64, pivots=None, reverse=False):
    """incomplete_cholesky.py:24-93.  Returns (L (N x k), index_columns (N,)).
    pivots: the pivot of every step, instead of the first maximum of the running diagonal;
    reverse: the Schur sum of every entry taken from the last column to the first."""
    diag = np.array(diagonal, dtype=dtype, copy=True)
    n = diag.size
    index_columns = np.arange(n)
    L = np.zeros((n, max_rank), dtype=dtype)
    for m in range(max_rank):
        i_argmax = int(np.argmax(diag[index_columns][m:]) + m)           # :53
        if pivots is not None:
            i_argmax = int(np.nonzero(index_columns[m:] == pivots[m])[0][0] + m)
        index_columns[m], index_columns[i_argmax] = index_columns[i_argmax], index_columns[m]
        m_pi = index_columns[m]
        i_pi = index_columns[m + 1:]
        pivot_element = diag[m_pi]
        assert pivot_element > 0, "given matrix is not PSD"              # :62
        L[m_pi, m] = np.sqrt(pivot_element)
        k = get_col(m_pi)
        schur = 0
        if m > 0 and reverse:
            schur = np.einsum("c, rc->r", L[m_pi, :m][::-1], L[i_pi, :m][:, ::-1])
        elif m > 0:
            schur = np.einsum("c, rc->r", L[m_pi, :m], L[i_pi, :m])      # :72
        L[i_pi, m] = (k[i_pi] - schur) / L[m_pi, m]                       # :75
        diag[i_pi] -= L[i_pi, m] ** 2                                     # :78
    return L, index_columns


def woodbury_panel(L, lam, dtype=np.float64):
    """iterative_cholesky.py:141-148: T = chol(lam I + L^T L)^-1 L^T, apply (r - T^T T r)/lam."""
    k = L.shape[1]
    if not _is_f64(dtype):
        L = np.asarray(L, dtype=dtype)
        kernel = dtype(lam) * np.eye(k, dtype=dtype) + (L.T @ L)
        return _forward(_cholesky_lower(kernel), L.T), 1.0
    kernel = lam * np.eye(k) + (L.T @ L)
    L2 = scipy.linalg.cholesky(kernel, lower=True)
    T = scipy.linalg.solve_triangular(L2, L.T, lower=True)
    return T, 1.0


def cho_factor_stable(M, dtype=np.float64, sign=None):
    """iterative_solver.py:576-583 (the code after :583 is unreachable).
    sign: the sign of the 1e-15 shift, instead of deciding it from the smallest eigenvalue (in
    long double that eigenvalue is the float64 eigh of M rounded to float64)."""
    M = np.array(M, dtype=dtype, copy=True)
    if sign is None:
        lo_eig = scipy.linalg.eigh(M.astype(np.float64, copy=False), eigvals_only=True,
                                   subset_by_index=[0, 0])
        sgn = 1 if lo_eig <= 0 else -1
    else:
        sgn = int(sign)
    M[np.diag_indices_from(M)] += sgn * 1.0e-15
    if not _is_f64(dtype):
        return _cholesky_lower(M).T, False
    return scipy.linalg.cho_factor(M, overwrite_a=False, check_finite=False)


def _solve_factor_T(c, lower, B):
    """solve_triangular(c, B, lower=lower, trans="T") for the upper factor c of cho_factor."""
    if _is_f64(c.dtype):
        return scipy.linalg.solve_triangular(c, B, lower=lower, trans="T")
    assert not lower
    return _forward(c.T, B)


def nystrom_panel(S_nm, idx, lam, variant=0, dtype=np.float64, signs=(None, None)):
    """Nystrom preconditioner panel from the column panel S[:, idx] (N x k).

    variant 0: Iterative._init_precon_operator (iterative_solver.py:112-322):
      U = chol_stable(S_mm); C = S_nm U^-1; V = chol_stable(C^T C + lam I);
      B = V^-T C^T; apply (B^T B v - v)/lam  -> sigma_p = -1.
    variant 1: _init_precon_operator_sb (iterative_solver.py:343-381):
      L_m = chol(S_mm + 1e-16 I); Kb = S_nm L_m^-T; L_in = chol(lam I + Kb^T Kb);
      P = L_in^-1 Kb^T; apply -(v - P^T P v)/lam -> sigma_p = -1.
    signs: the signs of the two 1e-15 shifts of variant 0 (cho_factor_stable).
    """
    S_nm = np.array(S_nm, dtype=dtype, copy=True)
    k = S_nm.shape[1]
    S_mm = S_nm[idx, :]
    if variant == 0:
        U, lower = cho_factor_stable(S_mm, dtype=dtype, sign=signs[0])
        C = _solve_factor_T(U, lower, S_nm.T).T
        inner = C.T.dot(C)
        inner[np.diag_indices_from(inner)] += lam
        V, lower = cho_factor_stable(inner, dtype=dtype, sign=signs[1])
        B = _solve_factor_T(V, lower, C.T)
        return B, -1.0
    if not _is_f64(dtype):
        L_m = _cholesky_lower(S_mm + dtype(1e-16) * np.eye(k, dtype=dtype))
        Kbar = _forward(L_m, S_nm.T).T
        inner = dtype(lam) * np.eye(k, dtype=dtype) + Kbar.T @ Kbar
        return _forward(_cholesky_lower(inner), Kbar.T), -1.0
    L_m = scipy.linalg.cholesky(S_mm + 1e-16 * np.eye(k), lower=True)
    Kbar = scipy.linalg.solve_triangular(L_m, S_nm.T, lower=True).T
    inner = lam * np.eye(k) + Kbar.T @ Kbar
    L_in = scipy.linalg.cholesky(inner, lower=True)
    P = scipy.linalg.solve_triangular(L_in, Kbar.T, lower=True)
    return P, -1.0


def apply_panel(T, sigma_p, lam, r, dtype=np.float64):
    """z = sigma_p * lam^-1 * (r - T^T (T r))."""
    if not _is_f64(dtype):
        T, r = np.asarray(T, dtype=dtype), np.asarray(r, dtype=dtype)
        return dtype(sigma_p) * ((r - T.T @ (T @ r)) / dtype(lam))
    lam_inv = 1.0 / lam
    return sigma_p * (lam_inv * (r - T.T @ (T @ r)))


def lev_scores(S_nm, idx, lam, dtype=np.float64, signs=(None, None)):
    """Numeric part of _lev_scores (iterative_solver.py:489-552)."""
    S_nm = np.array(S_nm, dtype=dtype, copy=True)
    S_mm = S_nm[idx, :]
    L, lower = cho_factor_stable(S_mm, dtype=dtype, sign=signs[0])
    B = _solve_factor_T(L, lower, S_nm.T)
    B_BT_lam = B.dot(B.T)
    B_BT_lam[np.diag_indices_from(B_BT_lam)] += lam
    C, C_lower = cho_factor_stable(B_BT_lam, dtype=dtype, sign=signs[1])
    C_B = _solve_factor_T(C, C_lower, B)
    return np.einsum("i...,i...->...", C_B, C_B)


def svd_panel(S, k, lam, dtype=np.float64):
    """svd_preconditioner (iterative_solver.py:1297-1329): L = U sqrt(s)[:, :k], Woodbury."""
    U, s = _svd_symmetric(S, dtype)
    L = (U * np.sqrt(s))[:, :k]
    return woodbury_panel(L, lam, dtype=dtype)


def rank_k_lev_scores(S, k, dtype=np.float64):
    """_rank_k_leverage_scores (iterative_solver.py:1110-1175): ||U_k row|| (not squared)."""
    U, _ = _svd_symmetric(S, dtype)
    if not _is_f64(dtype):
        return np.sqrt(np.sum(U[:, :k] ** 2, axis=1))
    return np.linalg.norm(U[:, :k], axis=1)


def precon_exact(S, kind, lam, k=None, idx=None, variant=0, pivots=None, signs=(None, None),
                 dtype=np.float64):
    """The dense N x N preconditioner a panel stands for, sigma_p (I - T^T T) / lam, for
    kind 'pivchol' (rank k, + Woodbury), 'nystrom' (columns idx) or 'eig' (rank k)."""
    S = np.asarray(S, dtype=dtype)
    n = S.shape[0]
    if kind == "pivchol":
        L, _ = pivoted_cholesky(lambda i: S[:, i], np.diag(S).copy(), k, dtype=dtype, pivots=pivots)
        T, sp = woodbury_panel(L, lam, dtype=dtype)
    elif kind == "nystrom":
        T, sp = nystrom_panel(S[:, idx], idx, lam, variant, dtype=dtype, signs=signs)
    elif kind == "eig":
        T, sp = svd_panel(S, k, lam, dtype=dtype)
    else:
        raise KeyError(kind)
    return dtype(sp) * ((np.eye(n, dtype=dtype) - T.T @ T) / dtype(lam))


def spectrum(S, lam, P=None, dtype=np.float64):
    """Iterative.solve(flag_eigvals=True) (iterative_solver.py:978-989; dev_utils.get_eigvals,
    dev_utils.py:8-25), as mlff_spectrum returns it: the eigenvalues, descending and real, of
    P A (P: the dense preconditioner, precon_exact) or of A = S + lam I itself.  float64:
    scipy.linalg.eigvals as the reference calls it, the real parts; long double: P A is similar
    to the symmetric R^T P R, A = R R^T, whose eigenvalues come from eigh_longdouble."""
    S = np.asarray(S, dtype=dtype)
    A = S + dtype(lam) * np.eye(S.shape[0], dtype=dtype)
    if _is_f64(dtype):
        ev = scipy.linalg.eigvals(A if P is None else P @ A)
        return np.sort(np.real(ev))[::-1]
    if P is None:
        return eigh_longdouble(A)[0][::-1]
    R = _cholesky_lower(A)
    return eigh_longdouble(R.T @ np.asarray(P, dtype=dtype) @ R)[0][::-1]
