"""NumPy float64 restatement of the pathwise gradient of the particle return (pilco_rollout_particles_grad / _grad_rbf,
csrc/particles_grad.hip; docs/particle_gradients.md) -- the yardstick of tests/test_gpu_particle_grad.py, itself pinned to
torch autograd in tests/test_particle_grad_cpu.py.  Built from helpers/particles_restatement.py (the forward step, the
rewards) and helpers/predict_jac_restatement.py (the kernel derivative dk_dx, the Cholesky factors); it shares no code with the
kernels and covers the exact GP and FITC on shared inducing inputs.

With z = [x, u], u = action(x), v~ = v [+ noise], sd = sqrt(max(v~, 0)) and x' = x + mu + sd eps:
  A[e, d] = [e == d] + d mu_e / d z_d + g_e d v_e / d z_d,   g_e = eps_e / (2 sd_e) where v~_e > 0, 0 elsewhere
  lam_H = 0;  t = H-1 .. 0:  g_u = A[:, E:]^T lam,  ds_k = g_u[k] scale_k cos(s_k),
                             lam <- A[:, :E]^T lam + (ds / dx)^T ds + grad r(x_t)
(the matrix of step H-1 meets lam_H = 0 and is not formed).  The parameter sums are divided by P once; dx0 is lam_0, the
gradient of every particle's own return.  HALF, DVAR_SIGN, SYM and RBF_SCALE exist for the mutant guard of
tests/test_particle_grad_cpu.py only."""
import math

import numpy as np
from scipy.linalg import solve_triangular

from helpers import particles_restatement as pr
from helpers.predict_jac_restatement import dk_dx
from helpers.predict_restatement import JITTER, _chol, se_ard

HALF = 0.5          # g = eps / (2 sd): a mutant drops the 1/2
DVAR_SIGN = 1.0     # + g dv: a mutant flips it
SYM = True          # grad r = -r/2 (W + W^T)(x - t): a mutant uses W alone
RBF_SCALE = math.exp(-0.5 * pr.RBF_SQUASH_VARIANCE)   # the RbfController's squash of a 1e-6 variance: a mutant drops it


# ------------------------------------------------------------------ the posterior and its input Jacobians
_LAST = []      # the last Jacobian call: (model, xu, result)
_FACTORS = {}   # id(model) -> (model, per-output factors): a model is factorised once


def _factors(model):
    hit = _FACTORS.get(id(model))
    if hit is not None and hit[0] is model:
        return hit[1]
    X, Y = np.asarray(model["X"], np.float64), np.asarray(model["Y"], np.float64)
    Z = model.get("Z")
    out = []
    for e in range(Y.shape[1]):
        ls, sf2, sn2 = model["lengthscales"][e], model["variance"][e], model["noise"][e]
        if Z is None:
            L = _chol(se_ard(X, X, ls, sf2) + sn2 * np.eye(X.shape[0]))
            alpha = solve_triangular(L.T, solve_triangular(L, Y[:, e], lower=True), lower=False)
            out.append((X, L, None, alpha))
        else:
            Zf = np.asarray(Z, np.float64)
            Luu = _chol(se_ard(Zf, Zf, ls, sf2) + JITTER * np.eye(Zf.shape[0]))
            V = solve_triangular(Luu, se_ard(Zf, X, ls, sf2), lower=True)
            nu = sf2 - np.sum(V * V, axis=0) + sn2
            LB = _chol(np.eye(Zf.shape[0]) + (V / nu) @ V.T)
            gamma = solve_triangular(LB, V @ (Y[:, e] / nu), lower=True)
            alpha = solve_triangular(Luu.T, solve_triangular(LB.T, gamma, lower=False), lower=False)
            out.append((Zf, Luu, LB, alpha))
    _FACTORS.clear()
    _FACTORS[id(model)] = (model, out)
    return out


def posterior_jac(model, xu, jac=True):
    """(mu, v, dmu, dv): (P, E), (P, E), (P, E, D), (P, E, D) at xu (P, D) (jac=False: (mu, v)).  The formulas of
    predict_jac_restatement with the variance's weights solved once per point, c = -2 L^{-T} L^{-1} k* (FITC: -2 Luu^{-T} (w -
    LB^{-T} tmp)), so that the cost is that of the values, and with the factors of a model kept between calls
    (tests/test_particle_grad_cpu.py holds it against gpr_predict_f_jac / fitc_predict_f_jac and particles_restatement.step)."""
    xu = np.asarray(xu, np.float64)
    if jac and _LAST and _LAST[0] is model and np.array_equal(_LAST[1], xu):   # (the sweep and its bound ask for the same points)
        return _LAST[2]
    E, D, Pn = np.asarray(model["Y"]).shape[1], xu.shape[1], xu.shape[0]
    mu, v = np.empty((Pn, E)), np.empty((Pn, E))
    dmu, dv = np.empty((Pn, E, D)), np.empty((Pn, E, D))
    for e, (pts, L, LB, alpha) in enumerate(_factors(model)):
        ls, sf2 = model["lengthscales"][e], model["variance"][e]
        for i in range(0, Pn, 512):
            K, dK = dk_dx(pts, xu[i:i + 512], ls, sf2) if jac else (se_ard(pts, xu[i:i + 512], ls, sf2), None)
            w = solve_triangular(L, K, lower=True)
            if LB is None:
                var = sf2 - np.sum(w * w, axis=0)
                c = -2.0 * solve_triangular(L.T, w, lower=False) if jac else None
            else:
                tmp = solve_triangular(LB, w, lower=True)
                var = sf2 - np.sum(w * w, axis=0) + np.sum(tmp * tmp, axis=0)
                c = -2.0 * solve_triangular(L.T, w - solve_triangular(LB.T, tmp, lower=False), lower=False) if jac else None
            mu[i:i + 512, e] = alpha @ K
            v[i:i + 512, e] = var
            if jac:
                dmu[i:i + 512, e] = np.einsum("i,itd->td", alpha, dK)
                dv[i:i + 512, e] = np.einsum("it,itd->td", c, dK)
    if jac:
        _LAST[:] = [model, xu.copy(), (mu, v, dmu, dv)]
    return (mu, v, dmu, dv) if jac else (mu, v)


# ------------------------------------------------------------------ the policy: sines' arguments, their derivatives
def _rbf_parts(policy, x):
    C, Y = np.asarray(policy["X"], np.float64), np.asarray(policy["Y"], np.float64)
    ls = np.asarray(policy["lengthscales"], np.float64)
    U = Y.shape[1]
    noise = np.broadcast_to(np.asarray(policy["noise"], np.float64).reshape(-1), (U,))
    Kc = np.stack([se_ard(C, C, ls[k], 1.0) for k in range(U)])                                   # (U, bf, bf)
    Ainv = np.stack([np.linalg.inv(Kc[k] + noise[k] * np.eye(C.shape[0])) for k in range(U)])
    beta = np.stack([Ainv[k] @ Y[:, k] for k in range(U)])                                        # (U, bf)
    kk = np.stack([se_ard(x, C, ls[k], 1.0) for k in range(U)], axis=1)                            # (P, U, bf)
    return C, ls, Kc, Ainv, beta, kk


def policy_scale(policy):
    if policy is None:
        return np.empty(0)
    U = np.asarray(policy["W"]).shape[0] if policy["kind"] == "linear" else np.asarray(policy["Y"]).shape[1]
    sc = np.broadcast_to(np.asarray(policy.get("max_action", 1.0), np.float64).reshape(-1), (U,)).copy()
    return sc * RBF_SCALE if policy["kind"] == "rbf" else sc


def sine_arguments(policy, x):
    """s (P, U): u = scale sin(s)."""
    x = np.asarray(x, np.float64)
    if policy is None:
        return np.empty((x.shape[0], 0))
    if policy["kind"] == "linear":
        return x @ np.asarray(policy["W"], np.float64).T + np.asarray(policy["b"], np.float64).reshape(1, -1)
    _, _, _, _, beta, kk = _rbf_parts(policy, x)
    return np.einsum("pkc,kc->pk", kk, beta)


class _PolicyAdj:
    """Accumulates the parameter cotangents of one reverse sweep; absolute=True: the first-order error bound of the same
    sums for cotangent bounds ds >= 0 (every factor in absolute value)."""

    def __init__(self, policy, absolute=False):
        self.p, self.abs = policy, absolute
        if policy is None:
            return
        if policy["kind"] == "linear":
            W = np.asarray(policy["W"], np.float64)
            self.dW, self.db = np.zeros_like(W), np.zeros(W.shape[0])
        else:
            C, Y = np.asarray(policy["X"]), np.asarray(policy["Y"])
            self.dbeta, self.dC = np.zeros((Y.shape[1], C.shape[0])), np.zeros(C.shape)
            self.dl = np.zeros((Y.shape[1], C.shape[1]))

    def step(self, x, ds):
        """x (P, E), ds (P, U) -> (ds / dx)^T ds (P, E); adds the step's parameter sums."""
        a = np.abs if self.abs else (lambda q: q)
        p = self.p
        if p is None:
            return np.zeros_like(x)
        if p["kind"] == "linear":
            W = np.asarray(p["W"], np.float64)
            self.dW += np.einsum("pk,pe->ke", ds, a(x))
            self.db += ds.sum(axis=0)
            return ds @ a(W)
        C, ls, _, _, beta, kk = _rbf_parts(p, x)
        w = ds[:, :, None] * a(beta)[None] * kk                                   # (P, U, bf)
        diff = a(x[:, None, :] - C[None, :, :])                                   # (P, bf, E)
        self.dbeta += np.einsum("pk,pkc->kc", ds, kk)
        self.dC += np.einsum("pkc,pce,ke->ce", w, diff, 1.0 / ls ** 2)
        self.dl += np.einsum("pkc,pce,ke->ke", w, diff ** 2, 1.0 / ls ** 3)
        return (1.0 if self.abs else -1.0) * np.einsum("pkc,pce,ke->pe", w, diff, 1.0 / ls ** 2)

    def finish(self, P):
        """The sums over P; RbfController: dbeta through beta_k = (K_k + noise_k I)^-1 Y_k into (dX, dY, dls)."""
        a = np.abs if self.abs else (lambda q: q)
        p = self.p
        if p is None:
            return ()
        if p["kind"] == "linear":
            return self.dW / P, self.db / P
        C, ls, Kc, Ainv, beta, _ = _rbf_parts(p, np.zeros((1, np.asarray(p["X"]).shape[1])))
        dX, dl, dbeta = self.dC / P, self.dl / P, self.dbeta / P
        U = ls.shape[0]
        dY = np.empty((C.shape[0], U))
        diff = a(C[:, None, :] - C[None, :, :])                                   # (bf, bf, E)
        for k in range(U):
            g = a(Ainv[k]) @ dbeta[k]
            dY[:, k] = g
            Wk = (1.0 if self.abs else -1.0) * np.outer(g, a(beta[k])) * Kc[k]
            ws = Wk + Wk.T
            s = 1.0 if self.abs else -1.0
            dX = dX + s * np.einsum("ij,ije->ie", ws, diff) / ls[k] ** 2
            dl[k] = dl[k] + 0.5 * np.einsum("ij,ije->e", ws, diff ** 2) / ls[k] ** 3
        return dX, dY, dl


# ------------------------------------------------------------------ rewards
def reward_grad(terms, x):
    """(P, E): the gradient of particles_restatement.reward."""
    x = np.asarray(x, np.float64)
    g = np.zeros_like(x)
    for t in terms:
        W = np.asarray(t["W"], np.float64)
        if t["kind"] == "exponential":
            d = x - (np.zeros(x.shape[1]) if t.get("t") is None else np.asarray(t["t"], np.float64).reshape(1, -1))
            r = np.exp(-0.5 * np.einsum("pi,ij,pj->p", d, W, d))
            g += float(t.get("coef", 1.0)) * (-0.5 * r)[:, None] * (d @ ((W + W.T) if SYM else W).T)
        else:
            g += float(t.get("coef", 1.0)) * W.reshape(1, -1)
    return g


# ------------------------------------------------------------------ the step matrix, the sweep
def step_matrix(model, policy, x, eps, observation_noise=False, variance=None):
    """A (P, E, D) at the states x (P, E) with the draws eps (P, E), and (x', v~).  variance (P, E): in place of the
    posterior's (the clamp case: v~ <= 0 cannot be reached through a positive definite model)."""
    x, eps = np.asarray(x, np.float64), np.asarray(eps, np.float64)
    E = x.shape[1]
    u = pr.action(policy, x)
    mu, v, dmu, dv = posterior_jac(model, np.concatenate([x, u], axis=1))
    if variance is not None:
        v = np.asarray(variance, np.float64)
    if observation_noise:
        v = v + np.asarray(model["noise"], np.float64).reshape(1, -1)
    pos = v > 0.0
    sd = np.sqrt(np.maximum(v, 0.0))
    g = np.where(pos, (2.0 * HALF) * eps / (2.0 * np.where(pos, sd, 1.0)), 0.0)
    A = dmu + DVAR_SIGN * g[:, :, None] * dv
    A[:, np.arange(E), np.arange(E)] += 1.0
    return A, x + mu + sd * eps, v


def reverse(model, policy, terms, xs, eps, observation_noise=False, variance=None):
    """The reverse sweep on GIVEN states xs (H or H+1, P, E) and draws eps (H, P, E): -> (grads, dx0 (P, E)); grads as
    PILCO.value_and_gradient: (dW, db), (dX, dY, dls) or ().  variance: {t: (P, E)} for step_matrix."""
    xs, eps = np.asarray(xs, np.float64), np.asarray(eps, np.float64)
    H, P, E = eps.shape
    adj = _PolicyAdj(policy)
    scale = policy_scale(policy)
    lam = np.zeros((P, E))
    for t in range(H - 1, -1, -1):
        x = xs[t]
        if t < H - 1:
            A, _, _ = step_matrix(model, policy, x, eps[t], observation_noise, None if variance is None else variance.get(t))
            gu = np.einsum("ped,pe->pd", A[:, :, E:], lam)
            ds = gu * scale * np.cos(sine_arguments(policy, x))
            lam = np.einsum("ped,pe->pd", A[:, :, :E], lam) + adj.step(x, ds)
        lam = lam + reward_grad(terms, x)
    return adj.finish(P), lam


def forward(model, policy, terms, x0, eps, observation_noise=False):
    """xs (H+1, P, E) and J = sum_t mean_p r(x_t^p) over the pre-step states: the step of particles_restatement.step."""
    xs = [np.asarray(x0, np.float64)]
    J = 0.0
    for t in range(eps.shape[0]):
        x = xs[-1]
        J += pr.reward(terms, x).mean()
        mu, v = posterior_jac(model, np.concatenate([x, pr.action(policy, x)], axis=1), jac=False)
        if observation_noise:
            v = v + np.asarray(model["noise"], np.float64).reshape(1, -1)
        xs.append(x + mu + np.sqrt(np.maximum(v, 0.0)) * np.asarray(eps[t], np.float64))
    return np.stack(xs), J


def value_and_grad(model, policy, terms, x0, eps, observation_noise=False):
    xs, J = forward(model, policy, terms, x0, eps, observation_noise)
    grads, dx0 = reverse(model, policy, terms, xs, eps, observation_noise)
    return J, grads, dx0


# ------------------------------------------------------------------ first-order error bound of the device's sweep
def reverse_bound(model, policy, terms, xs, eps, observation_noise=False):
    """Bounds (same structure as reverse's results) on |device - restatement| for a sweep on the SAME states and draws, from the
    project's per-entry bounds on the posterior (tests/test_gpu_predict_points.py, tests/test_gpu_predict_jac.py):
      |d v_e| <= 1e-8 sf2_e,   |d dmean_e| <= 1e-8 max |dmean_e|,   |d dvar_e| <= 1e-8 sf2_e / min_d l_ed
    carried to first order, every factor in absolute value, into g_e = eps_e / (2 sqrt(v~_e)) (|d g_e| = |g_e| |d v_e| / (2 v~_e)),
    into A, and through the recursion: d lam <- |A_x|^T d lam + dA_x^T |lam| + |ds/dx|^T d ds,  d ds = |scale cos s| (|A_u|^T d lam
    + dA_u^T |lam|), and the same parameter sums with d ds in place of ds and absolute factors.  (The mean's bound does not
    enter: the states are given.)  Also returns the absolute-sum scale of every quantity: the same sums with every term in
    absolute value, what a relative error of the terms is measured against."""
    xs, eps = np.asarray(xs, np.float64), np.asarray(eps, np.float64)
    H, P, E = eps.shape
    sf2 = np.asarray(model["variance"], np.float64)
    lmin = np.asarray(model["lengthscales"], np.float64).min(axis=1)
    bnd, scl = _PolicyAdj(policy, absolute=True), _PolicyAdj(policy, absolute=True)
    scale = np.abs(policy_scale(policy))
    lam, dlam, slam = np.zeros((P, E)), np.zeros((P, E)), np.zeros((P, E))
    for t in range(H - 1, -1, -1):
        x = xs[t]
        if t < H - 1:
            u = pr.action(policy, x)
            _, v, dmu, dv = posterior_jac(model, np.concatenate([x, u], axis=1))
            if observation_noise:
                v = v + np.asarray(model["noise"], np.float64).reshape(1, -1)
            assert np.all(v > 0.0)
            g = eps[t] / (2.0 * np.sqrt(v))
            A = dmu + g[:, :, None] * dv
            A[:, np.arange(E), np.arange(E)] += 1.0
            dg = np.abs(g) * (1e-8 * sf2)[None, :] / (2.0 * v)
            dA = (1e-8 * np.abs(dmu).max(axis=(0, 2)))[None, :, None] + np.abs(g)[:, :, None] * (1e-8 * sf2 / lmin)[None, :, None] \
                + dg[:, :, None] * np.abs(dv)
            c = np.abs(scale * np.cos(sine_arguments(policy, x)))
            aA = np.abs(A)
            dds = c * (np.einsum("ped,pe->pd", aA[:, :, E:], dlam) + np.einsum("ped,pe->pd", dA[:, :, E:], np.abs(lam)))
            sds = c * np.einsum("ped,pe->pd", aA[:, :, E:], slam)
            ds = scale * np.cos(sine_arguments(policy, x)) * np.einsum("ped,pe->pd", A[:, :, E:], lam)
            dlam = np.einsum("ped,pe->pd", aA[:, :, :E], dlam) + np.einsum("ped,pe->pd", dA[:, :, :E], np.abs(lam)) + bnd.step(x, dds)
            slam = np.einsum("ped,pe->pd", aA[:, :, :E], slam) + scl.step(x, sds)
            lam = np.einsum("ped,pe->pd", A[:, :, :E], lam) + _PolicyAdj(policy).step(x, ds)
        lam = lam + reward_grad(terms, x)
        slam = slam + np.abs(reward_grad(terms, x))
    return (bnd.finish(P), dlam), (scl.finish(P), slam)
