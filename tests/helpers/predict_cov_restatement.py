"""Two float64 restatements of the full posterior covariance between test points (GPR.predict_f / GPRFITC.predict_f with
full_cov=True) -- the yardsticks of pilco_gp_predict_points_cov, following the rule of docs/predict_edges.md --, the sampling map
of predict_f_samples and a NumPy restatement of Philox domain 5 (csrc/philox_normal.h).

  (a) GPflow's order: Cholesky factors and triangular solves (an extension of helpers/predict_restatement.py)
        exact  L = chol(K + sn2 I),  A = L \\ K*,  cov = K** - A^T A
        FITC   Luu = chol(Kuu + jitter I), V = Luu \\ Kuf, nu = diag(Kff - V^T V) + sn2, LB = chol(I + V nu^-1 V^T),
               A = Luu \\ Ku*,  B = LB \\ A,  cov = K** - A^T A + B^T B
  (b) the device's order: the kernel's scaled differences (x - y) fl(1 / l) as k_gram forms them, L^-1 by launch_trtri's
      recursive doubling on 64-blocks (helpers/trtri_doubling.py), plain products: W0 = L^-1 K*, FITC W1 = iAt K*,
      cov = K** - W0^T W0 + sn2 W1^T W1.  (b) takes mutants for the sensitivity test.
K of a result: max |result - truth| / unit; the cap of a case is 8 x the larger K of the two restatements, at least 4."""
import numpy as np
from scipy.linalg import solve_triangular

from helpers import predict_cov_cases as cc
from helpers.predict_restatement import _chol, se_ard
from helpers.trtri_doubling import padded_inverse

MUTANTS = ("fitc_sign", "no_sn2", "kss_ls", "n_minus_1", "waa", "jitter_added")
FITC_ONLY = ("fitc_sign", "no_sn2")


def se_device(A, B, ls, var):
    """k_gram's order: the difference times the rounded reciprocal lengthscale."""
    dd = (A[:, None, :] - B[None, :, :]) * (1.0 / np.asarray(ls, np.float64))
    return float(var) * np.exp(-0.5 * np.sum(dd * dd, axis=-1))


def restate_a(c, d):
    """cov (E, Nt, Nt) in GPflow's order."""
    X, xs = d["X"], d["xs"]
    out = np.empty((c["E"], len(xs), len(xs)))
    for e in range(c["E"]):
        ls, sf2, sn2 = d["ls"][e], d["var"][e], d["noise"][e]
        Kss = se_ard(xs, xs, ls, sf2)
        if not c["M"]:
            L = _chol(se_ard(X, X, ls, sf2) + sn2 * np.eye(len(X)))
            A = solve_triangular(L, se_ard(X, xs, ls, sf2), lower=True)
            out[e] = Kss - A.T @ A
        else:
            Z = cc.points_of(c, d, e)
            Luu = _chol(se_ard(Z, Z, ls, sf2) + cc.JITTER * np.eye(len(Z)))
            V = solve_triangular(Luu, se_ard(Z, X, ls, sf2), lower=True)
            nu = sf2 - np.sum(V * V, axis=0) + sn2
            LB = _chol(np.eye(len(Z)) + (V / nu) @ V.T)
            A = solve_triangular(Luu, se_ard(Z, xs, ls, sf2), lower=True)
            B = solve_triangular(LB, A, lower=True)
            out[e] = Kss - A.T @ A + B.T @ B
    return out


def restate_b(c, d, mutant=None):
    """The same in the device's order; mutant: one of MUTANTS."""
    X, xs = d["X"], d["xs"]
    E, Nt = c["E"], len(xs)
    out = np.empty((E, Nt, Nt))
    for e in range(E):
        ls, sf2, sn2 = d["ls"][e], d["var"][e], d["noise"][e]
        if not c["M"]:
            P = X[:-1] if mutant == "n_minus_1" else X
            L = np.linalg.cholesky(se_device(P, P, ls, sf2) + sn2 * np.eye(len(P)))
            ops = [(padded_inverse(L), -1.0)]
        else:
            Z = cc.points_of(c, d, e)
            P = Z[:-1] if mutant == "n_minus_1" else Z
            M = len(P)
            Lui = padded_inverse(np.linalg.cholesky(se_device(P, P, ls, sf2) + cc.JITTER * np.eye(M)))
            V = Lui @ se_device(P, X, ls, sf2)
            G = np.sqrt(1.0 + (sf2 - np.sum(V * V, axis=0)) / sn2)
            V = V / G
            Ami = padded_inverse(np.linalg.cholesky(V @ V.T + sn2 * np.eye(M)))
            ops = [(Lui, -1.0), (Ami @ Lui, 1.0 if mutant == "no_sn2" else -sn2 if mutant == "fitc_sign" else sn2)]
        k = se_device(P, xs, ls, sf2)
        cov = se_device(xs, xs, d["ls"][(e + 1) % E] * (1.5 if E == 1 else 1.0) if mutant == "kss_ls" else ls, sf2)
        for op, sc in ops:
            W = op @ k
            cov = cov + sc * (np.sum(W * W, axis=0)[:, None] * np.ones((1, Nt)) if mutant == "waa" else W.T @ W)
        if mutant == "jitter_added":
            cov = cov + 1e-6 * np.eye(Nt)
        out[e] = cov
    return out


def k_of(cov, d):
    """K of a covariance (E, Nt, Nt) against the truth of a loaded case: the largest error in the truth's units."""
    return float(np.max(np.abs(cov - d["cov"]) / d["unit"]))


def k_ref(c, d):
    return max(k_of(restate_a(c, d), d), k_of(restate_b(c, d), d))


def cap_from(kref):
    return max(cc.CAP_FLOOR, cc.CAP_FACTOR * kref)


def sample_map(mean, cov, z, jitter=1e-6):
    """predict_f_samples: mean (Nt, E), cov (E, Nt, Nt), z (S, Nt, E) -> (S, Nt, E) = mean + chol(cov + jitter I) z."""
    out = np.empty_like(z)
    for e in range(cov.shape[0]):
        C = np.linalg.cholesky(cov[e] + jitter * np.eye(cov.shape[1]))
        out[:, :, e] = mean[None, :, e] + z[:, :, e] @ C.T
    return out


COV_Z = 5   # the domain of pilco_gp_sample_points' normals: counter {s, a, j, 5} -> outputs 2j, 2j + 1 of sample s at test point a


def cov_normals(seed, S, Nt, outputs):
    """(z, r), (S, Nt, len(outputs)) each, of Philox domain 5: the normals and the Box-Muller radius behind each, from the
    vectorised streams of helpers/particle_fn_restatement.py."""
    from helpers import particle_fn_restatement as fr
    outputs = np.asarray(list(outputs))
    s, a, e = np.meshgrid(np.arange(S), np.arange(Nt), outputs, indexing="ij")
    z0, z1, r = fr.normal_pairs_np(s, a, e >> 1, COV_Z, seed)
    return np.where(e & 1, z1, z0), r
