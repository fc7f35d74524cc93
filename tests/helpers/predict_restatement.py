"""NumPy / SciPy float64 restatement of GPflow's GPR.predict_f and GPRFITC.predict_f (full_cov=False), written with
Cholesky factors and triangular solves the way GPflow evaluates them -- the yardstick of pilco_gp_predict_points
(tests/test_gpu_predict_points.py), itself pinned to the executed reference in tests/test_predict_points_cpu.py."""
import numpy as np
from scipy.linalg import cho_factor, solve_triangular

JITTER = 1e-6   # gpflow default_jitter: Kuu + jitter I (the reference's smgpr.py uses the same)


def se_ard(A, B, ls, var):
    """SquaredExponential K(A, B) with lengthscales ls (D,) and variance var."""
    d = (A[:, None, :] - B[None, :, :]) / np.asarray(ls, np.float64)
    return float(var) * np.exp(-0.5 * np.sum(d * d, axis=-1))


def _chol(A):
    return np.tril(cho_factor(A, lower=True)[0])


def gpr_predict_f(X, Y, lengthscales, variance, noise, Xs):
    """GPR.predict_f: mean = K*^T (K + sn2 I)^{-1} y, var = sf2 - ||L^{-1} K*||^2; (E, Nt) each."""
    X, Y, Xs = (np.asarray(a, np.float64) for a in (X, Y, Xs))
    E = Y.shape[1]
    mean, var = np.empty((E, Xs.shape[0])), np.empty((E, Xs.shape[0]))
    for e in range(E):
        K = se_ard(X, X, lengthscales[e], variance[e]) + noise[e] * np.eye(X.shape[0])
        L = _chol(K)
        A = solve_triangular(L, se_ard(X, Xs, lengthscales[e], variance[e]), lower=True)
        mean[e] = A.T @ solve_triangular(L, Y[:, e], lower=True)
        var[e] = variance[e] - np.sum(A * A, axis=0)
    return mean, var


def fitc_predict_f(X, Y, Z, lengthscales, variance, noise, Xs, jitter=JITTER):
    """GPRFITC.predict_f.  Z: (M, D) shared by every output, or (E, M, D): output e's own inducing inputs.
    Luu = chol(Kuu + jitter I), V = Luu^{-1} Kuf, nu = diag(Kff - V^T V) + sn2, LB = chol(I + V nu^{-1} V^T),
    gamma = LB^{-1} V (y / nu); w = Luu^{-1} Ku*, tmp = LB^{-1} w: mean = tmp^T gamma, var = sf2 - ||w||^2 + ||tmp||^2."""
    X, Y, Xs = (np.asarray(a, np.float64) for a in (X, Y, Xs))
    Z = np.asarray(Z, np.float64)
    E = Y.shape[1]
    mean, var = np.empty((E, Xs.shape[0])), np.empty((E, Xs.shape[0]))
    for e in range(E):
        Ze = Z[e] if Z.ndim == 3 else Z
        ls, sf2, sn2 = lengthscales[e], variance[e], noise[e]
        Luu = _chol(se_ard(Ze, Ze, ls, sf2) + jitter * np.eye(Ze.shape[0]))
        V = solve_triangular(Luu, se_ard(Ze, X, ls, sf2), lower=True)
        nu = sf2 - np.sum(V * V, axis=0) + sn2
        LB = _chol(np.eye(Ze.shape[0]) + (V / nu) @ V.T)
        gamma = solve_triangular(LB, V @ (Y[:, e] / nu), lower=True)
        w = solve_triangular(Luu, se_ard(Ze, Xs, ls, sf2), lower=True)
        tmp = solve_triangular(LB, w, lower=True)
        mean[e] = tmp.T @ gamma
        var[e] = sf2 - np.sum(w * w, axis=0) + np.sum(tmp * tmp, axis=0)
    return mean, var
