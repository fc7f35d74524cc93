"""40-digit truth (mpmath) of the full posterior covariance between test points and its per-entry unit, written with the
primitives of oracle/mp_predict.py (kern, chol, tri_inv: Gram matrices, Cholesky factors and triangular inverses on object
arrays of mpf).  TEST INFRASTRUCTURE ONLY: tools/gen_golden_predict_cov.py writes it into tests/golden/predict_cov.npz and
tests/test_predict_cov_cpu.py holds it to oracle.mp_predict's variance and to K** - K*^T iK K*; the GPU tests read the fixture.

  exact GP:  cov = K** - W^T W,  W = L^-1 K*                       unit_ab = 2^-53 (|k(x_a, x_b)| + g_a . g_b),  g = |L^-1| |k*|
  FITC:      cov = K** - W0^T W0 + W1^T W1,  W0 = Luu^-1 Ku*, W1 = LB^-1 Luu^-1 Ku*   (sn2 ||iAt k*||^2 of the device: Am Am^T = sn2 LB LB^T)
                                                                   unit: both walks summed
No unit goes below 2^-1022; on the diagonal the unit is uvar of oracle.mp_predict."""
import mpmath as mp
import numpy as np

from oracle.mp_predict import DPS, EPS, TINY, _abs, _f, _o, chol, kern, tri_inv


def _walks(ops, k):
    """sum over the operators of W^T W with signs, and of g^T g: ops = [(Op, sign)]."""
    ak = _abs(k)
    s = u = 0
    for op, sign in ops:
        W, g = np.dot(op, k), np.dot(_abs(op), ak)
        s = s + sign * np.dot(W.T, W)
        u = u + np.dot(g.T, g)
    return s, u


def _finish(kss, s, u):
    return _f(kss + s), np.maximum(EPS * _f(_abs(kss) + u), TINY)


def gpr_cov(X, ls, sf2, sn2, xs, dps=DPS):
    """One output of the exact GP: (cov, unit), float64 (Nt, Nt) each."""
    mp.mp.dps = dps
    X, ls, xs = _o(X), _o(ls), _o(xs)
    sf2, sn2 = mp.mpf(float(sf2)), mp.mpf(float(sn2))
    K = kern(X, X, ls, sf2)
    for i in range(X.shape[0]):
        K[i, i] += sn2
    s, u = _walks([(tri_inv(chol(K)), -1)], kern(X, xs, ls, sf2))
    return _finish(kern(xs, xs, ls, sf2), s, u)


def fitc_cov(X, Z, ls, sf2, sn2, xs, jitter=1e-6, dps=DPS):
    """One output of GPRFITC on the inducing inputs Z (M, D): (cov, unit)."""
    mp.mp.dps = dps
    X, Z, ls, xs = _o(X), _o(Z), _o(ls), _o(xs)
    sf2, sn2, jit = mp.mpf(float(sf2)), mp.mpf(float(sn2)), mp.mpf(float(jitter))
    M = Z.shape[0]
    Kuu = kern(Z, Z, ls, sf2)
    for i in range(M):
        Kuu[i, i] += jit
    Lui = tri_inv(chol(Kuu))
    V = np.dot(Lui, kern(Z, X, ls, sf2))
    nu = sf2 - np.sum(V * V, axis=0) + sn2
    Bm = np.dot(V / nu, V.T)
    for i in range(M):
        Bm[i, i] += 1
    T = np.dot(tri_inv(chol(Bm)), Lui)
    s, u = _walks([(Lui, -1), (T, 1)], kern(Z, xs, ls, sf2))
    return _finish(kern(xs, xs, ls, sf2), s, u)


def gpr_cov_direct(X, ls, sf2, sn2, xs, dps=DPS):
    """K** - K*^T (K + sn2 I)^-1 K* with the inverse formed by mpmath's own LU: another route to the same numbers."""
    mp.mp.dps = dps
    Xo, lo, xo = _o(X), _o(ls), _o(xs)
    sf2, sn2 = mp.mpf(float(sf2)), mp.mpf(float(sn2))
    n = Xo.shape[0]
    K = mp.matrix(kern(Xo, Xo, lo, sf2).tolist()) + sn2 * mp.eye(n)
    ks = mp.matrix(kern(Xo, xo, lo, sf2).tolist())
    kss = mp.matrix(kern(xo, xo, lo, sf2).tolist())
    C = kss - ks.T * (mp.inverse(K) * ks)
    return np.array([[float(C[i, j]) for j in range(C.cols)] for i in range(C.rows)])
