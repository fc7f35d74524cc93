"""Extended-precision (mpmath, 40 digits) evaluation of GPflow's GPR.predict_f and GPRFITC.predict_f (full_cov=False) and of
their derivatives with respect to the test input, with a unit per entry.

TEST INFRASTRUCTURE ONLY: the truth of tests/golden/predict_edges.npz (oracle/gen_golden_predict.py, docs/predict_edges.md).
Every operation (Gram matrices, Cholesky factors, inverses, exponentials, sums) runs in DPS-digit arithmetic from the float64
inputs; only the results are rounded.  The matrices are numpy object arrays of mpf, so the O(n^3) loops run in numpy's C loops.

  exact GP:  L L^T = K + sn2 I,  beta = L^-T L^-1 y,   mean = k*^T beta,   var = sf2 - ||L^-1 k*||^2
  FITC:      Luu Luu^T = Kuu + jitter I,  V = Luu^-1 Kuf,  nu = sf2 - sum V^2 + sn2,  LB LB^T = I + V nu^-1 V^T,
             B = Kuu + jitter I + Kuf nu^-1 Kfu = Luu LB LB^T Luu^T,  beta = B^-1 Kuf nu^-1 y,
             mean = k*^T beta,   var = sf2 - k*^T (Kuu^-1 - B^-1) k* = sf2 - ||Luu^-1 k*||^2 + ||LB^-1 Luu^-1 k*||^2
  (the device's iAt = Am^-1 Luu^-1 has Am Am^T = sn2 LB LB^T: sn2 ||iAt k*||^2 is the last term)
  d mean / d x_d = sum_i beta_i k_i w_id,   d var / d x_d = -2 sum_i a_i k_i w_id,   w_id = (X_id - x_d) / l_d^2,
  a = L^-T L^-1 k*  (FITC: Luu^-T Luu^-1 k* - T^T T k*, T = LB^-1 Luu^-1)

Units: 2^-53 times the sum of the absolute terms of the quantity as csrc/predict.hip and csrc/predict_jac.hip sum it, through
the factors -- the plain |k|^T |iK| |k| undercounts a flat kernel, whose L^-1 cancels heavily.  With g = |L^-1| |k*|:
  mean  g^T |L^-1 y|   (FITC: sum_i |k_i| |beta_i|)          var  sf2 + ||g||^2   (FITC: sf2 + || |Luu^-1||k*| ||^2 + || |T||k*| ||^2)
  dmean sum_i |beta_i k_i w_id|                              dvar 2 sum_i (|L^-T| g)_i |k_i w_id|   (FITC: both walks)
No unit goes below 2^-1022."""
from __future__ import annotations

import mpmath as mp
import numpy as np

DPS = 40
EPS = 2.0 ** -53
TINY = 2.0 ** -1022


def _o(a):
    """float64 array -> object array of mpf."""
    a = np.asarray(a, np.float64)
    out = np.empty(a.shape, dtype=object)
    for idx in np.ndindex(a.shape):
        out[idx] = mp.mpf(float(a[idx]))
    return out


def _f(a):
    a = np.asarray(a, dtype=object)
    return np.array([float(x) for x in a.ravel()], np.float64).reshape(a.shape)


def _abs(a):
    out = np.empty(a.shape, dtype=object)
    for idx in np.ndindex(a.shape):
        out[idx] = abs(a[idx])
    return out


def kern(P, Q, ls, sf2):
    """k(P_i, Q_j) (n, m) from object arrays P (n, D), Q (m, D), ls (D), sf2."""
    n, m = P.shape[0], Q.shape[0]
    out = np.empty((n, m), dtype=object)
    for i in range(n):
        for j in range(m):
            r2 = mp.mpf(0)
            for d in range(P.shape[1]):
                t = (P[i, d] - Q[j, d]) / ls[d]
                r2 += t * t
            out[i, j] = sf2 * mp.exp(-r2 / 2)
    return out


def chol(A):
    """Lower Cholesky factor of an object matrix."""
    n = A.shape[0]
    L = np.empty((n, n), dtype=object)
    L[:] = mp.mpf(0)
    for j in range(n):
        s = A[j, j] - (np.dot(L[j, :j], L[j, :j]) if j else 0)
        if s <= 0:
            raise ArithmeticError("not positive definite at %d" % j)
        L[j, j] = mp.sqrt(s)
        if j + 1 < n:
            col = A[j + 1:, j] - (np.dot(L[j + 1:, :j], L[j, :j]) if j else 0)
            L[j + 1:, j] = col / L[j, j]
    return L


def tri_inv(L):
    """L^-1 of a lower-triangular object matrix."""
    n = L.shape[0]
    X = np.empty((n, n), dtype=object)
    X[:] = mp.mpf(0)
    for i in range(n):
        if i:
            X[i, :i] = -np.dot(L[i, :i], X[:i, :i]) / L[i, i]
        X[i, i] = 1 / L[i, i]
    return X


def _finish(k, beta, a, abs_a, X, xs, ls, sf2, mean, var, umean, uvar):
    """The Jacobians and their units from k (n, Nt), beta (n), a = iK k (n, Nt), abs_a the absolute sum of a's walks."""
    n, Nt = k.shape
    D = X.shape[1]
    dm = np.empty((Nt, D), dtype=object)
    dv = np.empty((Nt, D), dtype=object)
    udm = np.empty((Nt, D), dtype=object)
    udv = np.empty((Nt, D), dtype=object)
    ak, bk = _abs(k), _abs(beta)
    for t in range(Nt):
        for d in range(D):
            w = (X[:, d] - xs[t, d]) / (ls[d] * ls[d])
            kw = k[:, t] * w
            akw = ak[:, t] * _abs(w)
            dm[t, d] = np.dot(beta, kw)
            dv[t, d] = -2 * np.dot(a[:, t], kw)
            udm[t, d] = np.dot(bk, akw)
            udv[t, d] = 2 * np.dot(abs_a[:, t], akw)
    unit = lambda u: np.maximum(EPS * _f(u), TINY)
    return dict(mean=_f(mean), var=_f(var), dmean=_f(dm), dvar=_f(dv), umean=unit(umean), uvar=unit(uvar), udmean=unit(udm),
                udvar=unit(udv))


def gpr(X, y, ls, sf2, sn2, xs, dps=DPS):
    """One output of the exact GP at the test points xs (Nt, D): dict of float64 mean, var (Nt), dmean, dvar (Nt, D) and the units
    umean, uvar, udmean, udvar of the same shapes."""
    mp.mp.dps = dps
    X, y, ls, xs = _o(X), _o(y), _o(ls), _o(xs)
    sf2, sn2 = mp.mpf(float(sf2)), mp.mpf(float(sn2))
    n = X.shape[0]
    K = kern(X, X, ls, sf2)
    for i in range(n):
        K[i, i] += sn2
    Li = tri_inv(chol(K))
    Liy = np.dot(Li, y)
    beta = np.dot(Li.T, Liy)
    k = kern(X, xs, ls, sf2)
    W = np.dot(Li, k)
    aLi = _abs(Li)
    g = np.dot(aLi, _abs(k))
    mean = np.dot(W.T, Liy)
    var = sf2 - np.sum(W * W, axis=0)
    umean = np.dot(g.T, _abs(Liy))
    uvar = sf2 + np.sum(g * g, axis=0)
    return _finish(k, beta, np.dot(Li.T, W), np.dot(aLi.T, g), X, xs, ls, sf2, mean, var, umean, uvar)


def fitc(X, y, Z, ls, sf2, sn2, xs, jitter=1e-6, dps=DPS):
    """One output of GPRFITC on the inducing inputs Z (M, D); results as gpr()."""
    mp.mp.dps = dps
    X, y, Z, ls, xs = _o(X), _o(y), _o(Z), _o(ls), _o(xs)
    sf2, sn2, jit = mp.mpf(float(sf2)), mp.mpf(float(sn2)), mp.mpf(float(jitter))
    M = Z.shape[0]
    Kuu = kern(Z, Z, ls, sf2)
    for i in range(M):
        Kuu[i, i] += jit
    Luu = chol(Kuu)
    Lui = tri_inv(Luu)
    V = np.dot(Lui, kern(Z, X, ls, sf2))
    nu = sf2 - np.sum(V * V, axis=0) + sn2
    Vn = V / nu
    Bm = np.dot(Vn, V.T)
    for i in range(M):
        Bm[i, i] += 1
    T = np.dot(tri_inv(chol(Bm)), Lui)            # B^-1 = T^T T
    beta = np.dot(T.T, np.dot(T, np.dot(np.dot(Luu, Vn), y)))   # Kuf nu^-1 y = Luu V nu^-1 y
    k = kern(Z, xs, ls, sf2)
    W0, W1 = np.dot(Lui, k), np.dot(T, k)
    aL, aT, ak = _abs(Lui), _abs(T), _abs(k)
    g0, g1 = np.dot(aL, ak), np.dot(aT, ak)
    mean = np.dot(k.T, beta)
    var = sf2 - np.sum(W0 * W0, axis=0) + np.sum(W1 * W1, axis=0)
    umean = np.dot(ak.T, _abs(beta))
    uvar = sf2 + np.sum(g0 * g0, axis=0) + np.sum(g1 * g1, axis=0)
    a = np.dot(Lui.T, W0) - np.dot(T.T, W1)
    abs_a = np.dot(aL.T, g0) + np.dot(aT.T, g1)
    return _finish(k, beta, a, abs_a, Z, xs, ls, sf2, mean, var, umean, uvar)
