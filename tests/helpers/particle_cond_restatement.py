"""NumPy restatement of the path-conditioned particle rollout (pilco_rollout_particles_cond, csrc/particles_cond.hip;
docs/particle_conditioned.md) -- the yardstick of tests/test_gpu_particle_cond.py, itself held to the sampling map of
helpers/predict_cov_restatement.py in tests/test_particle_cond_cpu.py.

  path covariance   c_ts = k_e(xt_t, xt_s) - w_t . w_s  (FITC: - w0_t . w0_s + w1_t . w1_s), between the visited points of ONE
                    particle: the two float64 restatements of helpers/predict_cov_restatement.py (restate_a, restate_b), and a
                    np.longdouble evaluation (64-bit significand) that serves as their and the device's truth, with the units
                    of docs/predict_cov.md, 2^-53 (|k| + g_t . g_s), g = |L^-1| |k*|
  one row           row t of the factor of C + j I from the rows above it, the draw and the increment, in np.longdouble
  the whole path    the rows one after the other
  Philox domain 6   the observation-noise draws, from the vectorised streams of helpers/particle_fn_restatement.py"""
import numpy as np

from helpers import predict_cov_cases as cc
from helpers import predict_cov_restatement as rc

LD = np.longdouble
U53 = 2.0 ** -53
COND_OBS = 6   # counter {p, t, j, 6} -> the observation draws of outputs 2j, 2j + 1 of particle p at step t


# ------------------------------------------------------------------ linear algebra in np.longdouble
def chol_ld(A):
    """Lower Cholesky factor of A (n, n) in np.longdouble, column by column."""
    A = np.array(A, LD)
    n = A.shape[0]
    L = np.zeros((n, n), LD)
    for j in range(n):
        d = A[j, j] - np.dot(L[j, :j], L[j, :j])
        L[j, j] = np.sqrt(d)
        if j + 1 < n:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def tri_inv_ld(L):
    """L^-1 of a lower triangular L in np.longdouble, by forward substitution on the identity."""
    n = L.shape[0]
    X = np.zeros((n, n), LD)
    for i in range(n):
        r = -(L[i, :i] @ X[:i]) if i else np.zeros(n, LD)
        r[i] += 1
        X[i] = r / L[i, i]
    return X


def se_ld(A, B, ls, var):
    d = (np.asarray(A, LD)[:, None, :] - np.asarray(B, LD)[None, :, :]) / np.asarray(ls, LD)
    return LD(var) * np.exp(-0.5 * np.sum(d * d, axis=-1))


def operators_ld(model):
    """Per output the operators of the covariance's walks, [(Op, sign)], in np.longdouble, and the points they act on:
    exact GP [(L^-1, -1)] on X; FITC [(Luu^-1, -1), (LB^-1 Luu^-1, +1)] on Z (helpers/predict_cov_truth.py's formulas)."""
    X, Z = np.asarray(model["X"], np.float64), model.get("Z")
    out = []
    for e in range(len(model["variance"])):
        ls, sf2, sn2 = model["lengthscales"][e], model["variance"][e], model["noise"][e]
        if Z is None:
            K = se_ld(X, X, ls, sf2) + LD(sn2) * np.eye(len(X), dtype=LD)
            out.append(([(tri_inv_ld(chol_ld(K)), -1)], X))
        else:
            M = len(Z)
            Lui = tri_inv_ld(chol_ld(se_ld(Z, Z, ls, sf2) + LD(cc.JITTER) * np.eye(M, dtype=LD)))
            V = Lui @ se_ld(Z, X, ls, sf2)
            nu = LD(sf2) - np.sum(V * V, axis=0) + LD(sn2)
            T = tri_inv_ld(chol_ld((V / nu) @ V.T + np.eye(M, dtype=LD))) @ Lui
            out.append(([(Lui, -1), (T, 1)], np.asarray(Z, np.float64)))
    return out


def path_cov_truth(model, ops, xs):
    """xs (H, P, D): the visited points.  -> (cov, unit) (P, E, H, H) float64: the np.longdouble path covariances of every
    particle and output, rounded, and their units 2^-53 (|k| + sum over the walks of g_t . g_s), never below 2^-1022."""
    H, P, D = xs.shape
    E = len(ops)
    cov, unit = np.zeros((P, E, H, H)), np.zeros((P, E, H, H))
    flat = xs.reshape(H * P, D)
    for e, (walks, pts) in enumerate(ops):
        ls, sf2 = model["lengthscales"][e], model["variance"][e]
        k = se_ld(pts, flat, ls, sf2)                      # (n, H P)
        Ws = [((op @ k).reshape(-1, H, P), sign, (np.abs(op) @ np.abs(k)).reshape(-1, H, P)) for op, sign in walks]
        for p in range(P):
            kss = se_ld(xs[:, p], xs[:, p], ls, sf2)
            c, u = kss.copy(), np.abs(kss)
            for W, sign, g in Ws:
                c = c + sign * (W[:, :, p].T @ W[:, :, p])
                u = u + g[:, :, p].T @ g[:, :, p]
            cov[p, e], unit[p, e] = c.astype(np.float64), np.maximum(U53 * u.astype(np.float64), cc.TINY)
    return cov, unit


def path_cov_f64(model, xs, which):
    """The float64 restatement (a: GPflow's order, b: the device's) of predict_cov_restatement on every particle's own
    points: (P, E, H, H)."""
    H, P, _ = xs.shape
    E = len(model["variance"])
    Z = model.get("Z")
    c = dict(E=E, M=0 if Z is None else len(Z), own=False)
    out = np.zeros((P, E, H, H))
    fn = rc.restate_a if which == "a" else rc.restate_b
    for p in range(P):
        d = dict(X=model["X"], xs=xs[:, p], ls=model["lengthscales"], var=model["variance"], noise=model["noise"],
                 Z=None if Z is None else Z[None])
        out[p] = fn(c, d)
    return out


def k_of(cov, truth, unit):
    """The largest error of the lower triangles in the truth's units."""
    i, j = np.tril_indices(cov.shape[-1])
    return float(np.max(np.abs(cov - truth)[..., i, j] / unit[..., i, j])) if cov.shape[-1] else 0.0


# ------------------------------------------------------------------ the factor row, the draw, the path
def row(c_row, lam_above, j, mu, z):
    """One teacher-forced row in np.longdouble: c_row (t + 1,) = c_t0 .. c_tt, lam_above (t, t) the factor rows above,
    j the jitter j_e, mu the posterior mean, z (t + 1,) the draws z_0 .. z_t.
    -> (l (t + 1,) with l_t = Lam_tt, d the pivot, f the increment), np.longdouble."""
    t = len(c_row) - 1
    c_row, lam_above, z = np.asarray(c_row, LD), np.asarray(lam_above, LD), np.asarray(z, LD)
    l = np.zeros(t + 1, LD)
    for s in range(t):
        l[s] = (c_row[s] - np.dot(l[:s], lam_above[s, :s])) / lam_above[s, s]
    d = (c_row[t] + LD(j)) - np.dot(l[:t], l[:t])
    l[t] = np.sqrt(d) if d > 0 else LD(np.nan)
    return l, d, LD(mu) + np.dot(l, z)


def path(C, j, mu, z):
    """The whole path of one particle and output: C (H, H) the path covariance (lower triangle read), mu, z (H,).
    -> (Lam (H, H), pivots d (H,), increments f (H,)), np.longdouble."""
    H = len(mu)
    lam, ds, fs = np.zeros((H, H), LD), np.zeros(H, LD), np.zeros(H, LD)
    for t in range(H):
        l, ds[t], fs[t] = row(C[t, :t + 1], lam[:t, :t], j, mu[t], z[:t + 1])
        lam[t, :t + 1] = l
    return lam, ds, fs


def backward_error(lam, A):
    """max |Lam Lam^T - A| / (2^-53 |Lam| |Lam|^T) over the lower triangle (docs/predict_cov.md's measure); stacked matrices."""
    lam, A = np.asarray(lam, LD), np.asarray(A, LD)
    if lam.shape[-1] == 0:
        return 0.0
    num = np.abs(lam @ np.swapaxes(lam, -1, -2) - A)
    den = LD(U53) * (np.abs(lam) @ np.swapaxes(np.abs(lam), -1, -2))
    i, k = np.tril_indices(lam.shape[-1])
    return float(np.max(num[..., i, k] / den[..., i, k]))


# ------------------------------------------------------------------ the observation stream
def obs_normals(seed, H, P, E):
    """(zeta, r) (H, P, E): the normals of Philox domain 6 and the Box-Muller radius behind each."""
    from helpers import particle_fn_restatement as fr
    t, p, e = np.meshgrid(np.arange(H), np.arange(P), np.arange(E), indexing="ij")
    z0, z1, r = fr.normal_pairs_np(p, t, e >> 1, COND_OBS, seed)
    return np.where(e & 1, z1, z0), r


# ------------------------------------------------------------------ the group plan (csrc/particles_cond_plan.h)
def tri(H):
    return H * (H + 1) // 2


def per_particle(H, nops, E, D, npad, want_cov):
    return H * nops * E * npad + (2 if want_cov else 1) * E * tri(H) + H * D + E * npad + 2 * E


def chunk_cap(E, npad):
    return max(64, (2 ** 24 // (E * npad)) // 64 * 64)


def plan(P, H, nops, E, D, npad, want_cov, budget, cap):
    """-> (G, ngroups, per_particle, footprint, H_fit): the mirror of cond_plan."""
    per = per_particle(H, nops, E, D, npad, want_cov)
    fit = budget // per // 64 * 64
    if fit < 64:
        hs = [h for h in range(H) if per_particle(h, nops, E, D, npad, want_cov) * 64 <= budget]
        return 0, 0, per, per * 64, (hs[-1] if hs else -1)
    G = min(fit, (P + 63) // 64 * 64, cap)
    return G, (P + G - 1) // G, per, per * G, H
