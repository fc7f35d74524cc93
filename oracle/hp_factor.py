"""Extended-precision truth of the GP factorisations (mgpr.py:81-89, smgpr.py:24-45), plain NumPy.

TEST INFRASTRUCTURE ONLY.  The Gram matrices are formed from the float64 inputs in x87 extended precision (np.longdouble,
64-bit significand: asserted below, never skipped).  Solves run as float64 Cholesky plus iterative refinement with the residual
in extended precision: the refined solution is accurate to about cond * 2^-64 (about 1e-10 at cond 1e9), three orders of
magnitude closer to the truth than a float64 solve (cond * 2^-53).  iK is represented by its action on fixed probe vectors,
so N = 4160 stays cheap; mp_truth.py (40 digits) pins this module on small cases (tests/test_factorisations_cpu.py).

Each case also gets the float64 forward error of oracle.tf_path (LAPACK through SciPy, the reference's own formulas) on the same
inputs: the GPU kernels are judged against that state of the art where the problem is ill-conditioned.
"""
from __future__ import annotations

import numpy as np
import scipy.linalg as sla

from oracle import tf_path as tp

LD = np.longdouble
if np.finfo(LD).nmant < 63:
    raise ImportError("oracle.hp_factor needs an 80-bit np.longdouble (64-bit significand); this platform has "
                      f"{np.finfo(LD).nmant + 1} bits")

JITTER = 1e-6   # smgpr.py:27
_ROWS = 256     # rows per chunk when forming Gram matrices (bounds the extended-precision temporaries)


def gram(X1, X2, ls, var):
    """var * exp(-|x1 - x2|^2_ls / 2) of one output in extended precision, (N1, N2) longdouble."""
    X1 = np.asarray(X1, np.float64).astype(LD)
    X2 = np.asarray(X2, np.float64).astype(LD)
    il = 1 / np.asarray(ls, np.float64).astype(LD)
    out = np.empty((X1.shape[0], X2.shape[0]), LD)
    for r0 in range(0, X1.shape[0], _ROWS):
        a = X1[r0:r0 + _ROWS]
        r2 = np.zeros((a.shape[0], X2.shape[0]), LD)
        for d in range(X1.shape[1]):
            t = (a[:, d, None] - X2[None, :, d]) * il[d]
            r2 += t * t
        out[r0:r0 + _ROWS] = LD(var) * np.exp(-r2 / 2)
    return out


def refine(A, c, B, its=12):
    """A^{-1} B for the longdouble matrix A, float64 Cholesky factor c of A: refined until the correction stops mattering."""
    B = np.asarray(B).astype(LD)
    X = sla.cho_solve(c, B.astype(np.float64)).astype(LD)
    for _ in range(its):
        R = B - A @ X
        dX = sla.cho_solve(c, R.astype(np.float64))
        X += dX
        if np.linalg.norm(dX) <= 1e-19 * np.linalg.norm(X.astype(np.float64)):
            break
    return X


def cond_estimate(A64, c, its=40):
    """cond_2 of the SPD float64 matrix: power iteration for the largest eigenvalue, inverse iteration for the smallest."""
    n = A64.shape[0]
    if n <= 512:
        w = np.linalg.eigvalsh(A64)
        return float(w[-1] / w[0])
    v = np.random.RandomState(1).randn(n)
    u = v.copy()
    for _ in range(its):
        v = A64 @ v
        v /= np.linalg.norm(v)
        u = sla.cho_solve(c, u)
        u /= np.linalg.norm(u)
    lmax = v @ (A64 @ v)
    lmin = 1.0 / (u @ sla.cho_solve(c, u))
    return float(lmax / lmin)


def _rel(a, b):
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))


def exact(X, Y, ls, var, noise, P, lapack=True, full_iK=False):
    """Per output a: beta = (K + s2 I)^{-1} y and iK P (the probes), their float64 roundings of the refined truth, nlml
    (mgpr's objective, the log-determinant from the float64 factor), cond estimate and -- lapack=True -- the forward errors of
    oracle.tf_path (beta, iK P) on the same inputs.  full_iK: also the whole inverse, from the float64 Cholesky factor of the
    extended-precision matrix rounded once (accurate to about cond * 1e-16: a truth at 1e-10 for well-conditioned cases only)."""
    X = np.asarray(X, np.float64)
    Y = np.asarray(Y, np.float64)
    N, E = X.shape[0], Y.shape[1]
    out = dict(beta=np.empty((E, N)), iKP=np.empty((E, N, P.shape[1])), nlml=np.empty(E), cond=np.empty(E),
               lapack_beta=np.full(E, np.nan), lapack_iKP=np.full(E, np.nan))
    if full_iK:
        out["iK"] = np.empty((E, N, N))
    if lapack:
        iK_tf, beta_tf = tp.calculate_factorizations(X, Y, ls, var, noise)
    for a in range(E):
        A = gram(X, X, ls[a], var[a])
        A[np.diag_indices(N)] += LD(noise[a])
        A64 = A.astype(np.float64)
        c = sla.cho_factor(A64, lower=True)
        b = refine(A, c, Y[:, a])
        out["beta"][a] = b.astype(np.float64)
        out["iKP"][a] = refine(A, c, P).astype(np.float64)
        logdet = 2 * np.sum(np.log(np.diag(c[0]).astype(LD)))
        out["nlml"][a] = float(b @ Y[:, a].astype(LD) / 2 + logdet / 2 + LD(N) * np.log(2 * LD(np.pi)) / 2)
        out["cond"][a] = cond_estimate(A64, c)
        if full_iK:
            out["iK"][a] = sla.cho_solve(c, np.eye(N))
        if lapack:
            out["lapack_beta"][a] = _rel(beta_tf[a], out["beta"][a])
            out["lapack_iKP"][a] = _rel(iK_tf[a] @ P, out["iKP"][a])
    return out


def fitc(X, Y, Z, ls, var, noise, P, lapack=True):
    """The FITC factorisation of smgpr.py:24-45 per output, in its closed form: with Kmm = K(Z) + 1e-6 I, Kmn = K(Z, X),
    Lam = s2 + var - diag(Knm Kmm^{-1} Kmn) and B = Kmm + Kmn Lam^{-1} Knm,
        iK = Kmm^{-1} - B^{-1},      beta = B^{-1} Kmn Lam^{-1} y
    (smgpr's iAt^T iAt s2 = (L Am Am^T L^T / s2)^{-1} = B^{-1}).  Returns beta, iK P, cond(B) estimate, cond(Kmm) estimate and
    the forward errors of oracle.tf_path.fitc_factorizations."""
    X = np.asarray(X, np.float64)
    Y = np.asarray(Y, np.float64)
    Z = np.asarray(Z, np.float64)
    M, E = Z.shape[0], Y.shape[1]
    out = dict(beta=np.empty((E, M)), iKP=np.empty((E, M, P.shape[1])), cond=np.empty(E), cond_kmm=np.empty(E),
               lapack_beta=np.full(E, np.nan), lapack_iKP=np.full(E, np.nan))
    if lapack:
        iK_tf, beta_tf = tp.fitc_factorizations(X, Y, Z, ls, var, noise)
    for a in range(E):
        Kmm = gram(Z, Z, ls[a], var[a])
        Kmm[np.diag_indices(M)] += LD(JITTER)
        Kmn = gram(Z, X, ls[a], var[a])
        cm = sla.cho_factor(Kmm.astype(np.float64), lower=True)
        W = refine(Kmm, cm, Kmn)
        lam = LD(noise[a]) + LD(var[a]) - np.sum(Kmn * W, axis=0)
        B = Kmm + (Kmn / lam) @ Kmn.T
        B64 = B.astype(np.float64)
        cb = sla.cho_factor(B64, lower=True)
        b = refine(B, cb, Kmn @ (Y[:, a].astype(LD) / lam))
        out["beta"][a] = b.astype(np.float64)
        out["iKP"][a] = (refine(Kmm, cm, P) - refine(B, cb, P)).astype(np.float64)
        out["cond"][a] = cond_estimate(B64, cb)
        out["cond_kmm"][a] = cond_estimate(Kmm.astype(np.float64), cm)
        if lapack:
            out["lapack_beta"][a] = _rel(beta_tf[a], out["beta"][a])
            out["lapack_iKP"][a] = _rel(iK_tf[a] @ P, out["iKP"][a])
    return out


def residual(X, y, ls, var, noise, beta):
    """Normwise backward error of a solution: |(K + s2 I) beta - y| / (|K + s2 I| |beta| + |y|), Frobenius norm of the
    matrix, the residual in extended precision."""
    A = gram(X, X, ls, var)
    A[np.diag_indices(A.shape[0])] += LD(noise)
    r = y.astype(LD) - A @ np.asarray(beta, np.float64).astype(LD)
    nA = float(np.sqrt(np.sum(A * A)))
    return float(np.linalg.norm(r.astype(np.float64)) / (nA * np.linalg.norm(beta) + np.linalg.norm(y)))
