"""NumPy / SciPy float64 restatement of the input Jacobians of GPR.predict_f and GPRFITC.predict_f (full_cov=False), written
with Cholesky factors and triangular solves -- the yardstick of pilco_gp_predict_points_jac (tests/test_gpu_predict_jac.py),
in NumPy / LAPACK, sharing no code with the kernels.  tests/test_predict_jac_cpu.py pins it to
torch autograd through the value restatement, to the executed reference and to a 40-digit evaluation.

With dk[i, t, d] = d k(X_i, x_t) / d x_td = k_it (X_id - x_td) / l_d^2:
  GPR:   A = L^{-1} K*:   d mean = (L^{-T} L^{-1} y)^T dk,   d var = -2 A^T L^{-1} dk
  FITC:  w = Luu^{-1} Ku*, tmp = LB^{-1} w:   d mean = (Luu^{-T} LB^{-T} gamma)^T dk,
         d var = -2 w^T Luu^{-1} dk + 2 tmp^T LB^{-1} Luu^{-1} dk
SIGN, LS_POWER and VAR_FACTOR exist for the mutant guard of tests/test_predict_jac_cpu.py only."""
import numpy as np
from scipy.linalg import solve_triangular

from helpers.predict_restatement import JITTER, _chol, se_ard

SIGN = 1.0         # (X - x): a mutant flips it
LS_POWER = 2       # / l^2: a mutant divides by l
VAR_FACTOR = 2.0   # the 2 of d (a^T a): a mutant drops it


def dk_dx(P, Xs, ls, var):
    """K (n, Nt) and dK (n, Nt, D): k(P_i, x_t) and its derivative with respect to x_t."""
    ls = np.asarray(ls, np.float64)
    K = se_ard(P, Xs, ls, var)
    diff = SIGN * (P[:, None, :] - Xs[None, :, :]) / ls ** LS_POWER
    return K, K[:, :, None] * diff


def _tri(L, B):
    """L^{-1} B for B (n, Nt, D)."""
    n = B.shape[0]
    return solve_triangular(L, B.reshape(n, -1), lower=True).reshape(B.shape)


def gpr_predict_f_jac(X, Y, lengthscales, variance, noise, Xs):
    """(mean, var, dmean, dvar): (E, Nt), (E, Nt), (E, Nt, D), (E, Nt, D)."""
    X, Y, Xs = (np.asarray(a, np.float64) for a in (X, Y, Xs))
    E, Nt, D = Y.shape[1], Xs.shape[0], X.shape[1]
    mean, var = np.empty((E, Nt)), np.empty((E, Nt))
    dmean, dvar = np.empty((E, Nt, D)), np.empty((E, Nt, D))
    for e in range(E):
        L = _chol(se_ard(X, X, lengthscales[e], variance[e]) + noise[e] * np.eye(X.shape[0]))
        K, dK = dk_dx(X, Xs, lengthscales[e], variance[e])
        A = solve_triangular(L, K, lower=True)
        Liy = solve_triangular(L, Y[:, e], lower=True)
        alpha = solve_triangular(L.T, Liy, lower=False)
        mean[e] = A.T @ Liy
        var[e] = variance[e] - np.sum(A * A, axis=0)
        dmean[e] = np.einsum("i,itd->td", alpha, dK)
        dvar[e] = -VAR_FACTOR * np.einsum("it,itd->td", A, _tri(L, dK))
    return mean, var, dmean, dvar


def fitc_predict_f_jac(X, Y, Z, lengthscales, variance, noise, Xs, jitter=JITTER):
    """Z: (M, D) shared by every output, or (E, M, D): output e's own inducing inputs.  Shapes as gpr_predict_f_jac."""
    X, Y, Xs = (np.asarray(a, np.float64) for a in (X, Y, Xs))
    Z = np.asarray(Z, np.float64)
    E, Nt, D = Y.shape[1], Xs.shape[0], X.shape[1]
    mean, var = np.empty((E, Nt)), np.empty((E, Nt))
    dmean, dvar = np.empty((E, Nt, D)), np.empty((E, Nt, D))
    for e in range(E):
        Ze = Z[e] if Z.ndim == 3 else Z
        ls, sf2, sn2 = lengthscales[e], variance[e], noise[e]
        Luu = _chol(se_ard(Ze, Ze, ls, sf2) + jitter * np.eye(Ze.shape[0]))
        V = solve_triangular(Luu, se_ard(Ze, X, ls, sf2), lower=True)
        nu = sf2 - np.sum(V * V, axis=0) + sn2
        LB = _chol(np.eye(Ze.shape[0]) + (V / nu) @ V.T)
        gamma = solve_triangular(LB, V @ (Y[:, e] / nu), lower=True)
        K, dK = dk_dx(Ze, Xs, ls, sf2)
        w = solve_triangular(Luu, K, lower=True)
        tmp = solve_triangular(LB, w, lower=True)
        dw = _tri(Luu, dK)
        dtmp = _tri(LB, dw)
        mean[e] = tmp.T @ gamma
        var[e] = sf2 - np.sum(w * w, axis=0) + np.sum(tmp * tmp, axis=0)
        dmean[e] = np.einsum("i,itd->td", gamma, dtmp)
        dvar[e] = -VAR_FACTOR * np.einsum("it,itd->td", w, dw) + VAR_FACTOR * np.einsum("it,itd->td", tmp, dtmp)
    return mean, var, dmean, dvar


def mp_jacobians(cfg, xs, dps=40):
    """(dmean, dvar) (E, Nt, D) of the exact GP evaluated with dps digits: beta and iK from oracle.mp_truth.factorize."""
    import mpmath as mp
    from oracle.mp_truth import factorize
    X, ls, sf2 = cfg["X"], cfg["lengthscales"], cfg["variance"]
    iKs, betas = factorize(X, cfg["Y"], ls, sf2, cfg["noise"], dps=dps)
    f = mp.mpf
    N, D = X.shape
    E = len(sf2)
    dm, dv = np.empty((E, len(xs), D)), np.empty((E, len(xs), D))
    for e in range(E):
        for t, x in enumerate(xs):
            k = mp.matrix([f(sf2[e]) * mp.exp(-sum(((f(X[i, d]) - f(x[d])) / f(ls[e, d])) ** 2 for d in range(D)) / 2) for i in range(N)])
            a = iKs[e] * k
            for d in range(D):
                wgt = [k[i] * (f(X[i, d]) - f(x[d])) / f(ls[e, d]) ** 2 for i in range(N)]
                dm[e, t, d] = float(sum(betas[e][i] * wgt[i] for i in range(N)))
                dv[e, t, d] = float(-2 * sum(a[i] * wgt[i] for i in range(N)))
    return dm, dv
