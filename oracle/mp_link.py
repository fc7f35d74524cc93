"""Extended-precision (mpmath, 50 digits) evaluation of the serial link of a horizon step.

TEST INFRASTRUCTURE ONLY.  The link is controller -> squash_sin -> joint Gaussian -> reward (controllers.py:13-36,46-58,
108-121; pilco.py:138-153; rewards.py:19-81).  At its edge inputs (action variance 1e-16 .. 1e3, means up to 1e6, rank
deficient or indefinite reward weights, far targets) every float64 evaluation of these formulas cancels or underflows the
same way, so oracle.tf_path cannot judge a kernel there.  Here every operation runs in `DPS`-digit arithmetic from the
float64 inputs and is rounded to float64 once, at the very end.  All functions take and return mpmath values (lists /
mp.matrix), so that a parameter can be moved by 1e-15 for a central difference in the same arithmetic (`gradient`).

The RbfController does not go through mp_truth.factorize / moments_mp: those take float64 arrays, and the gradient truth has
to move centres, targets and lengthscales by 1e-15 IN mp arithmetic.  rbf_factor / mean_only_moments restate the same lines
(mgpr.py:81-149 with iK = 0, kernel variance 1) on mp values; the dynamics GP, which is never differentiated, uses mp_truth.

Used by oracle/gen_golden_link.py (tests/golden/link_edges.npz) and tests/test_link_edges_cpu.py.
"""
from __future__ import annotations

import mpmath as mp
import numpy as np

from oracle import mp_truth

DPS = 50


def f(x):
    return x if isinstance(x, mp.mpf) else mp.mpf(float(x))


def vec(a):
    return [f(x) for x in (a if isinstance(a, list) else np.ravel(a))]


def mat(a, r=None, c=None):
    if isinstance(a, mp.matrix):
        return a
    a = np.asarray(a, np.float64)
    if r is not None:
        a = a.reshape(r, c)
    m = mp.matrix(a.shape[0], a.shape[1]) if a.size else mp.matrix(a.shape[0], max(a.shape[1], 0))
    for i in range(a.shape[0]):
        for j in range(a.shape[1]):
            m[i, j] = f(a[i, j])
    return m


def to_np(m, r, c):
    return np.array([[float(m[i, j]) for j in range(c)] for i in range(r)], dtype=np.float64).reshape(r, c)


# --------------------------------------------------------------------------- controllers
def squash_sin(m, s, e=None):
    """controllers.py:13-36: moments of e sin(x), x ~ N(m, s).  m [U], s (U,U), e [U] or None -> M [U], S (U,U), C [U] (diag)."""
    mp.mp.dps = DPS
    U = len(m)
    e = [f(1)] * U if e is None else e
    M = [e[u] * mp.exp(-s[u, u] / 2) * mp.sin(m[u]) for u in range(U)]
    S = mp.matrix(U, U)
    for u in range(U):
        for v in range(U):
            lq = -(s[u, u] + s[v, v]) / 2
            q = mp.exp(lq)
            S[u, v] = e[u] * e[v] * ((mp.exp(lq + s[u, v]) - q) * mp.cos(m[u] - m[v]) - (mp.exp(lq - s[u, v]) - q) * mp.cos(m[u] + m[v])) / 2
    C = [e[u] * mp.exp(-s[u, u] / 2) * mp.cos(m[u]) for u in range(U)]
    return M, S, C


def linear_controller(m, s, W, b, e=None, squash=True):
    """controllers.py:46-58.  m [E], s (E,E), W (U,E), b [U] -> M [U], S (U,U), V (E,U); also the pre-squash mean."""
    mp.mp.dps = DPS
    U, E = W.rows, W.cols
    M = [sum(W[u, k] * m[k] for k in range(E)) + b[u] for u in range(U)]
    S = W * s * W.T
    V = W.T.copy()
    pre = list(M)
    if squash:
        M, S, C = squash_sin(M, S, e)
        for k in range(E):
            for u in range(U):
                V[k, u] *= C[u]
    return M, S, V, pre


def rbf_factor(cX, cY, ls, noise):
    """beta of the policy GP (controllers.py:76,92: kernel variance 1, likelihood variance `noise`): mp values throughout."""
    mp.mp.dps = DPS
    bf, E, U = cX.rows, cX.cols, cY.cols
    betas = []
    for a in range(U):
        K = mp.matrix(bf, bf)
        for i in range(bf):
            for j in range(i, bf):
                r2 = sum(((cX[i, d] - cX[j, d]) / ls[a, d]) ** 2 for d in range(E))
                K[i, j] = K[j, i] = mp.exp(-r2 / 2)
            K[i, i] += noise[a]
        betas.append(mp.lu_solve(K, mp.matrix([cY[i, a] for i in range(bf)])))
    return betas


def mean_only_moments(X, ls, betas, m, s):
    """mgpr.py:91-149 with iK = 0 and kernel variance 1, every input an mp value: M [U], S (U,U), V (E,U)."""
    mp.mp.dps = DPS
    n, D, U = X.rows, X.cols, ls.rows
    zeta = [[X[i, d] - m[d] for d in range(D)] for i in range(n)]
    M, V = [f(0)] * U, mp.matrix(D, U)
    for a in range(U):
        iL = mp.diag([1 / ls[a, d] for d in range(D)])
        B = iL * s * iL + mp.eye(D)
        iB = mp.inverse(B)
        c = 1 / mp.sqrt(mp.det(B))
        for i in range(n):
            iN = mp.matrix([zeta[i][d] / ls[a, d] for d in range(D)])
            t = iB.T * iN
            lb = mp.exp(-(iN.T * t)[0] / 2) * betas[a][i]
            M[a] += lb * c
            for d in range(D):
                V[d, a] += t[d] / ls[a, d] * lb * c
    S = mp.matrix(U, U)
    for a in range(U):
        for b in range(a + 1):
            Lam = mp.diag([1 / ls[a, d] ** 2 + 1 / ls[b, d] ** 2 for d in range(D)])
            Rm = s * Lam + mp.eye(D)
            Q = mp.inverse(Rm) * s / 2
            za = [mp.matrix([zeta[i][d] / ls[a, d] ** 2 for d in range(D)]) for i in range(n)]
            wb = [mp.matrix([zeta[i][d] / ls[b, d] ** 2 for d in range(D)]) for i in range(n)]
            ka = [-sum((zeta[i][d] / ls[a, d]) ** 2 for d in range(D)) / 2 for i in range(n)]
            kb = [-sum((zeta[i][d] / ls[b, d]) ** 2 for d in range(D)) / 2 for i in range(n)]
            acc = f(0)
            for i in range(n):
                for j in range(n):
                    zw = za[i] + wb[j]
                    acc += betas[a][i] * betas[b][j] * mp.exp(ka[i] + kb[j] + (zw.T * Q * zw)[0])
            S[a, b] = S[b, a] = acc / mp.sqrt(mp.det(Rm)) - M[a] * M[b] + (1 if a == b else 0)
    return M, S, V


def rbf_controller(m, s, cX, cY, ls, e=None, squash=True, noise=None):
    """controllers.py:108-121: the policy GP's mean function only (iK zeroed), S -= diag(var - 1e-6), then squash_sin."""
    mp.mp.dps = DPS
    U, E = ls.rows, ls.cols
    noise = [f(1e-4)] * U if noise is None else noise
    M, S, V = mean_only_moments(cX, ls, rbf_factor(cX, cY, ls, noise), m, s)
    for u in range(U):
        S[u, u] -= f(1) - f(1e-6)
    pre = list(M)
    if squash:
        M, S, C = squash_sin(M, S, e)
        for k in range(E):
            for u in range(U):
                V[k, u] *= C[u]
    return M, S, V, pre


# --------------------------------------------------------------------------- rewards
def exponential_reward(m, s, W, t=None):
    """rewards.py:32-48 for a general (E,E) weight and target: mean, variance, and what the units need: the mean's
    quadratic form q = d W (I + S W)^-1 d^T, the second moment r2, and the two determinants."""
    mp.mp.dps = DPS
    E = len(m)
    d = mp.matrix([m[k] - (t[k] if t is not None else 0) for k in range(E)])
    SW = s * W
    A1, A2 = mp.eye(E) + SW, mp.eye(E) + 2 * SW
    q1 = (d.T * W * mp.inverse(A1) * d)[0]
    q2 = (d.T * W * mp.inverse(A2) * d)[0]
    det1, det2 = mp.det(A1), mp.det(A2)
    mu = mp.exp(-q1 / 2) / mp.sqrt(det1)
    r2 = mp.exp(-q2) / mp.sqrt(det2)
    return mu, r2 - mu * mu, dict(q=q1, q2=q2, r2=r2, det1=det1, det2=det2)


def linear_reward(m, s, w):
    """rewards.py:58-61."""
    mp.mp.dps = DPS
    E = len(m)
    return sum(m[k] * w[k] for k in range(E)), sum(w[i] * s[i, j] * w[j] for i in range(E) for j in range(E))


def combined_rewards(m, s, terms):
    """rewards.py:73-81.  terms: list of dict(kind 'exp' | 'lin', coef, W, t) with mp values -> mean, variance, per-term list."""
    mu, var, per = f(0), f(0), []
    for tm in terms:
        if tm["kind"] == "exp":
            a, b, info = exponential_reward(m, s, tm["W"], tm.get("t"))
        else:
            a, b = linear_reward(m, s, tm["W"])
            info = dict(q=f(0), q2=f(0), r2=a * a + b, det1=f(1), det2=f(1))
        per.append((a, b, info))
        mu += tm["coef"] * a
        var += tm["coef"] ** 2 * b
    return mu, var, per


def mp_terms(terms, E):
    """float64 reward terms (dict(kind, coef, W, t)) -> mp values."""
    out = []
    for tm in terms:
        if tm["kind"] == "exp":
            out.append(dict(kind="exp", coef=f(tm["coef"]), W=mat(tm["W"], E, E), t=None if tm.get("t") is None else vec(tm["t"])))
        else:
            out.append(dict(kind="lin", coef=f(tm["coef"]), W=vec(tm["W"])))
    return out


# --------------------------------------------------------------------------- cascade
def joint_gaussian(m, s, Mu, Su, V):
    """pilco.py:141-144: mean [D], covariance (D,D) of (x, u) and the cross block s V (E,U)."""
    E, U = len(m), len(Mu)
    sc = s * V if U else mp.matrix(E, 0)
    js = mp.matrix(E + U, E + U)
    for i in range(E):
        for j in range(E):
            js[i, j] = s[i, j]
        for u in range(U):
            js[i, E + u] = js[E + u, i] = sc[i, u]
    for u in range(U):
        for v in range(U):
            js[E + u, E + v] = Su[u, v]
    return list(m) + list(Mu), js, sc


def make_policy(kind, d, squash=True):
    """A callable (m, s) -> (M, S, V, pre-squash mean) from float64 / mp parameters in d: 'none', 'linear' (W, b, maxact),
    'rbf' (cX, cY, cl, maxact).  d['maxact'] None: no scaling (max_action=None)."""
    if kind == "none":
        return lambda m, s: ([], mp.matrix(0, 0), mp.matrix(len(m), 0), [])
    e = None if d.get("maxact") is None else vec(d["maxact"])
    if kind == "linear":
        W, b = mat(d["W"]), vec(d["b"])
        return lambda m, s: linear_controller(m, s, W, b, e, squash)
    cX, cY, cl = mat(d["cX"]), mat(d["cY"]), mat(d["cl"])
    return lambda m, s: rbf_controller(m, s, cX, cY, cl, e, squash)


def cascade(gp, policy, terms, m0, S0, H, fact=None):
    """The H-step rollout of pilco.py:118-153 in DPS-digit arithmetic.  gp: dict(X, Y, ls, var, noise) float64; policy: a
    callable from make_policy; terms: mp reward terms.  Returns mp values: states [(m, s)] (H+1), running reward [H+1],
    per step the action (M, S, s V, V) and the joint (mean, covariance)."""
    mp.mp.dps = DPS
    E = len(m0) if isinstance(m0, list) else np.size(m0)
    D = np.asarray(gp["X"]).shape[1]
    fact = fact or mp_truth.factorize(gp["X"], gp["Y"], gp["ls"], gp["var"], gp["noise"], DPS)
    mx, sx = vec(m0), mat(S0, E, E)
    states, rews, acts, total = [(mx, sx)], [f(0)], [], f(0)
    for _ in range(H):
        total += combined_rewards(mx, sx, terms)[0]
        Mu, Su, V, pre = policy(mx, sx)
        jm, js, sc = joint_gaussian(mx, sx, Mu, Su, V)
        acts.append((Mu, Su, sc, V, pre))
        Mg, Sg, Vg = mp_truth.moments_mp(gp["X"], gp["ls"], gp["var"], fact, jm, js, DPS)
        Cdx = mp.matrix(D, E)
        for a in range(E):
            for dd in range(D):
                Cdx[dd, a] = Vg[a][dd]
        s1 = js[0:E, 0:D]
        t1 = s1 * Cdx
        sx = Sg + sx + t1 + t1.T
        mx = [Mg[a] + mx[a] for a in range(E)]
        states.append((mx, sx))
        rews.append(total)
    return states, rews, acts


def round_cascade(states, rews, acts, E, U):
    """A cascade rounded to float64: traj (H+1, E + E*E), running reward (H+1), act (H, U + U*U + E*U) = [M | S | s V]."""
    H = len(acts)
    traj = np.array([[float(x) for x in m] + [float(s[i, j]) for i in range(E) for j in range(E)] for m, s in states])
    act = np.array([[float(x) for x in a[0]] + [float(a[1][u, v]) for u in range(U) for v in range(U)] +
                    [float(a[2][i, u]) for i in range(E) for u in range(U)] for a in acts]).reshape(H, U + U * U + E * U)
    return traj, np.array([float(r) for r in rews]), act


def cascade_np(gp, kind, d, terms, m0, S0, H, squash=True, fact=None):
    E = np.size(m0)
    U = np.asarray(gp["X"]).shape[1] - E
    return round_cascade(*cascade(gp, make_policy(kind, d, squash), mp_terms(terms, E), m0, S0, H, fact), E, U)


def gradient(gp, kind, d, terms, m0, S0, H, names, h=1e-15, fact=None):
    """d (total reward) / d d[name] for every name, by central differences of the DPS-digit cascade in the same arithmetic
    (step h: truncation error ~ h^2, rounding ~ 10^-DPS / h).  Returns float64 arrays shaped like d[name]."""
    mp.mp.dps = DPS
    E = np.size(m0)
    fact = fact or mp_truth.factorize(gp["X"], gp["Y"], gp["ls"], gp["var"], gp["noise"], DPS)
    tm = mp_terms(terms, E)
    pk = [k for k in ("W", "b", "cX", "cY", "cl", "maxact") if k in d]
    base = {k: (None if d[k] is None else (mat(d[k]) if np.ndim(d[k]) == 2 else vec(d[k]))) for k in pk}
    hh = f(h)

    def total(p):
        return cascade(gp, make_policy(kind, p), tm, m0, S0, H, fact)[1][H]

    out = []
    for name in names:
        shape = np.shape(d[name])
        g = np.empty(int(np.prod(shape)))
        for idx in range(g.size):
            vals = []
            for sgn in (1, -1):
                p = dict(base)
                if len(shape) == 2:
                    p[name] = base[name].copy()
                    p[name][idx // shape[1], idx % shape[1]] += sgn * hh
                else:
                    p[name] = list(base[name])
                    p[name][idx] += sgn * hh
                vals.append(total(p))
            g[idx] = float((vals[0] - vals[1]) / (2 * hh))
        out.append(g.reshape(shape))
    return out
