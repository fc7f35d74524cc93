"""The yardstick of the particle gradients (tests/helpers/particle_grad_restatement.py) against torch autograd through a torch
restatement of the particle rollout, on the CPU; its clamp contract; its mutants; the input condition of the device tests; and
the declarations / exports of the two entry points.  docs/particle_gradients.md records the figures printed here (-s)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from helpers import particle_grad_cases as pgc
from helpers import particle_grad_restatement as pg
from helpers import particles_restatement as pr
from helpers.predict_jac_restatement import fitc_predict_f_jac, gpr_predict_f_jac
from helpers.predict_restatement import JITTER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=torch.float64)   # noqa: E731
# both sides evaluate the same smooth function in float64; the sweep's terms (step matrices of norm O(1), H = 5) amplify a
# rounding error of 2^-53 by far less than 1e5: 1e-10 of the largest entry leaves four digits to spare over the 3e-14 measured
K_REF_BOUND = 1e-10


# ------------------------------------------------------------------ the rollout in torch
def _se(a, b, ls, sf2):
    d = (a[:, None, :] - b[None, :, :]) / ls
    return sf2 * torch.exp(-0.5 * (d * d).sum(-1))


def _posterior_t(model, xu):
    X, Y = T(model["X"]), T(model["Y"])
    mus, vs = [], []
    for e in range(Y.shape[1]):
        ls, sf2, sn2 = T(model["lengthscales"][e]), float(model["variance"][e]), float(model["noise"][e])
        if model.get("Z") is None:
            L = torch.linalg.cholesky(_se(X, X, ls, sf2) + sn2 * torch.eye(X.shape[0], dtype=torch.float64))
            A = torch.linalg.solve_triangular(L, _se(X, xu, ls, sf2), upper=False)
            mus.append(A.T @ torch.linalg.solve_triangular(L, Y[:, e:e + 1], upper=False)[:, 0])
            vs.append(sf2 - (A * A).sum(0))
        else:
            Z = T(model["Z"])
            M = Z.shape[0]
            Luu = torch.linalg.cholesky(_se(Z, Z, ls, sf2) + JITTER * torch.eye(M, dtype=torch.float64))
            V = torch.linalg.solve_triangular(Luu, _se(Z, X, ls, sf2), upper=False)
            nu = sf2 - (V * V).sum(0) + sn2
            LB = torch.linalg.cholesky(torch.eye(M, dtype=torch.float64) + (V / nu) @ V.T)
            gamma = torch.linalg.solve_triangular(LB, (V @ (Y[:, e] / nu))[:, None], upper=False)[:, 0]
            w = torch.linalg.solve_triangular(Luu, _se(Z, xu, ls, sf2), upper=False)
            tmp = torch.linalg.solve_triangular(LB, w, upper=False)
            mus.append(tmp.T @ gamma)
            vs.append(sf2 - (w * w).sum(0) + (tmp * tmp).sum(0))
    return torch.stack(mus, 1), torch.stack(vs, 1)


def _action_t(policy, par, x):
    if policy is None:
        return x[:, :0]
    ma = T(np.broadcast_to(np.asarray(policy.get("max_action", 1.0), np.float64).reshape(-1), (par[1].shape[-1] if policy["kind"] == "rbf" else par[0].shape[0],)))
    if policy["kind"] == "linear":
        W, b = par
        return ma * torch.sin(x @ W.T + b.reshape(1, -1))
    C, Y, ls = par
    U = Y.shape[1]
    noise = np.broadcast_to(np.asarray(policy["noise"], np.float64).reshape(-1), (U,))
    cols = []
    for k in range(U):
        K = _se(C, C, ls[k], 1.0) + float(noise[k]) * torch.eye(C.shape[0], dtype=torch.float64)
        cols.append(_se(x, C, ls[k], 1.0) @ torch.linalg.solve(K, Y[:, k]))
    return ma * math.exp(-0.5 * pr.RBF_SQUASH_VARIANCE) * torch.sin(torch.stack(cols, 1))


def _reward_t(terms, x):
    tot = torch.zeros(x.shape[0], dtype=torch.float64)
    for t in terms:
        if t["kind"] == "exponential":
            d = x - (T(t["t"]).reshape(1, -1) if t.get("t") is not None else 0.0)
            tot = tot + float(t.get("coef", 1.0)) * torch.exp(-0.5 * torch.einsum("pi,ij,pj->p", d, T(t["W"]), d))
        else:
            tot = tot + float(t.get("coef", 1.0)) * (x @ T(t["W"]).reshape(-1))
    return tot


def autograd(model, policy, terms, x0, eps, obs):
    """(J, grads, dx0) by torch autograd; dx0: the gradient of P J, every particle's own return."""
    if policy is None:
        par = []
    elif policy["kind"] == "linear":
        par = [T(policy["W"]).requires_grad_(), T(policy["b"]).reshape(-1).requires_grad_()]
    else:
        par = [T(policy["X"]).requires_grad_(), T(policy["Y"]).requires_grad_(), T(policy["lengthscales"]).requires_grad_()]
    x = T(x0).requires_grad_()
    xs, J = x, 0.0
    for t in range(eps.shape[0]):
        J = J + _reward_t(terms, xs).mean()
        mu, v = _posterior_t(model, torch.cat([xs, _action_t(policy, par, xs)], 1))
        if obs:
            v = v + T(model["noise"]).reshape(1, -1)
        assert bool((v > 0).all())
        xs = xs + mu + torch.sqrt(v) * T(eps[t])
    if eps.shape[0] == 0:
        return 0.0, tuple(np.zeros(p.shape) for p in par), np.zeros(x0.shape)
    g = torch.autograd.grad(J, par + [x], allow_unused=True)
    g = [np.zeros(p.shape) if gi is None else gi.numpy() for gi, p in zip(g, par + [x])]
    return float(J.detach()), tuple(g[:-1]), g[-1] * x0.shape[0]


# ------------------------------------------------------------------ small random cases
def small_case(kind, fitc=False, reward="combined", seed=0, N=60, E=3, U=2, H=5, P=7):
    r = np.random.RandomState(seed)
    if kind == "none":
        U = 0
    D = E + U
    X = r.randn(N, D)
    Y = np.stack([np.sin(X @ r.randn(D)) * 0.3 + 0.05 * r.randn(N) for _ in range(E)], 1)
    model = dict(X=X, Y=Y, lengthscales=1.5 + r.rand(E, D), variance=0.5 + r.rand(E), noise=0.01 + 0.02 * r.rand(E),
                 Z=X[r.permutation(N)[:20]] + 0.01 * r.randn(20, D) if fitc else None)
    if kind == "linear":
        policy = dict(kind="linear", W=0.5 * r.randn(U, E), b=0.1 * r.randn(U), max_action=np.array([1.3, 0.7])[:U])
    elif kind == "rbf":
        policy = dict(kind="rbf", X=r.randn(8, E), Y=0.5 * r.randn(8, U), lengthscales=1.0 + r.rand(U, E), noise=np.full(U, 1e-2),
                      max_action=np.array([1.3, 0.7])[:U])
    else:
        policy = None
    expo = dict(kind="exponential", W=np.eye(E) + 0.4 * r.randn(E, E), t=0.3 * r.randn(E), coef=1.2)   # asymmetric W
    lin = dict(kind="linear", W=r.randn(E), coef=-0.3)
    terms = dict(exponential=[expo], linear=[lin], combined=[expo, lin])[reward]
    return model, policy, terms, 0.3 * r.randn(P, E), r.randn(H, P, E)


def _rel_diff(case, obs):
    model, policy, terms, x0, eps = case
    J, grads, dx0 = pg.value_and_grad(model, policy, terms, x0, eps, obs)
    Ja, ga, dxa = autograd(model, policy, terms, x0, eps, obs)
    worst = abs(J - Ja) / max(abs(Ja), 1e-300)
    assert len(grads) == len(ga)
    for a, b in zip(list(grads) + [dx0], list(ga) + [dxa]):
        worst = max(worst, np.abs(np.asarray(a).reshape(b.shape) - b).max() / max(np.abs(b).max(), 1e-300))
    return worst


AUTOGRAD_CASES = [(k, f, rw, obs) for k in ("linear", "rbf", "none") for f in (False, True) for rw, obs in
                  (("combined", False), ("exponential", True), ("linear", False))]


@pytest.mark.parametrize("kind,fitc,reward,obs", AUTOGRAD_CASES, ids=["%s-fitc%d-%s-obs%d" % c for c in AUTOGRAD_CASES])
def test_restatement_matches_autograd(kind, fitc, reward, obs):
    k_ref = _rel_diff(small_case(kind, fitc, reward, seed=3), obs)
    print("K_ref %s fitc=%d %s obs=%d: %.3g" % (kind, fitc, reward, obs, k_ref))
    assert k_ref <= K_REF_BOUND


def test_short_horizons():
    for H in (0, 1, 2):
        model, policy, terms, x0, eps = small_case("linear", seed=5, H=H)
        assert _rel_diff((model, policy, terms, x0, eps), False) <= K_REF_BOUND
        _, grads, dx0 = pg.value_and_grad(model, policy, terms, x0, eps)
        if H <= 1:
            assert not any(np.any(g) for g in grads)
            assert np.array_equal(dx0, pg.reward_grad(terms, x0) if H else np.zeros_like(x0))


@pytest.mark.parametrize("name,value", [("DVAR_SIGN", -1.0), ("HALF", 1.0), ("SYM", False), ("RBF_SCALE", 1.0)])
def test_mutants_fail_the_autograd_check(monkeypatch, name, value):
    case = small_case("rbf", False, "combined", seed=3)
    assert _rel_diff(case, False) <= K_REF_BOUND
    monkeypatch.setattr(pg, name, value)
    diff = _rel_diff(case, False)
    print("mutant %s: %.3g" % (name, diff))
    assert diff > K_REF_BOUND


def test_posterior_jacobians_are_those_of_the_predict_restatement():
    for fitc in (False, True):
        model, _, _, _, _ = small_case("linear", fitc, seed=7)
        xu = np.random.RandomState(1).randn(9, 5)
        args = (model["lengthscales"], model["variance"], model["noise"], xu)
        ref = fitc_predict_f_jac(model["X"], model["Y"], model["Z"], *args) if fitc else gpr_predict_f_jac(model["X"], model["Y"], *args)
        got = pg.posterior_jac(model, xu)
        for a, b in zip(got, ref):
            b = np.moveaxis(b, 0, 1)
            assert np.abs(a - b).max() <= 1e-11 * max(np.abs(b).max(), 1.0)
        _, policy, terms, x0, eps = small_case("linear", fitc, seed=7)
        xs, _ = pg.forward(model, policy, terms, x0, eps[:1], True)
        assert np.abs(xs[1] - pr.step(model, policy, x0, eps[0], True)[0]).max() <= 1e-12


def test_the_clamp_has_no_derivative():
    """v~ <= 0 for output 1 (a caller-supplied variance: zero, and negative): the derivative through that draw is exactly 0."""
    model, policy, terms, x0, eps = small_case("linear", seed=9, H=3)
    xs, _ = pg.forward(model, policy, terms, x0, eps)
    _, _, dmu, _ = pg.posterior_jac(model, np.concatenate([xs[0], pr.action(policy, xs[0])], 1))
    for bad in (0.0, -1e-3):
        var = np.full(x0.shape, 0.02)
        var[:, 1] = bad
        A, _, _ = pg.step_matrix(model, policy, xs[0], eps[0], variance=var)
        want = dmu[:, 1, :].copy()
        want[:, 1] += 1.0
        assert np.array_equal(A[:, 1, :], want)
        eps2 = eps.copy()
        eps2[:, :, 1] = 7.0 * eps[:, :, 1] + 1.0                 # other draws for that output: nothing may change
        a = pg.reverse(model, policy, terms, xs, eps, variance={0: var, 1: var})
        b = pg.reverse(model, policy, terms, xs, eps2, variance={0: var, 1: var})
        assert all(np.array_equal(p, q) for p, q in zip(list(a[0]) + [a[1]], list(b[0]) + [b[1]]))
    # ... and it is there where v~ > 0
    var = np.full(x0.shape, 0.02)
    eps2 = eps.copy()
    eps2[:, :, 1] += 1.0
    a = pg.reverse(model, policy, terms, xs, eps, variance={0: var, 1: var})
    b = pg.reverse(model, policy, terms, xs, eps2, variance={0: var, 1: var})
    assert not np.array_equal(a[1], b[1])


@pytest.mark.parametrize("name,P,H,obs", pgc.CASES, ids=pgc.CASE_IDS)
def test_device_cases_meet_the_input_condition(name, P, H, obs):
    """Under the restatement alone: the bound the device test asserts against is at most 1e-5 of every quantity's
    absolute-sum scale, so that a vanishing sd cannot blow it up until it passes anything -- and at most 1e-5 of the quantity's
    own largest entry, so that it cannot pass a wrong gradient either (the absolute-sum scale of a cancelling sum can be many
    times the sum)."""
    if H < 2:
        return   # no step matrix enters: the propagated bound is zero
    s = pgc.setup(name)
    x0 = pgc.x0_of(name, P, 100 + P)
    eps = np.random.RandomState(200 + P + H).randn(H, P, s["E"])
    xs, _ = pg.forward(s["model"], s["policy"], s["terms"], x0, eps, obs)
    ref_g, ref_x = pg.reverse(s["model"], s["policy"], s["terms"], xs, eps, obs)
    (bg, bx), (sg, sx) = pg.reverse_bound(s["model"], s["policy"], s["terms"], xs, eps, obs)
    worst = tight = 0.0
    for b, sc, ref in zip(list(bg) + [bx], list(sg) + [sx], list(ref_g) + [ref_x]):
        worst = max(worst, float((b / np.maximum(sc, 1e-300)).max()))
        tight = max(tight, float(np.max(b) / np.abs(ref).max()))
    print("%s P=%d H=%d obs=%d: bound / scale %.3g, largest bound / largest entry %.3g" % (name, P, H, obs, worst, tight))
    assert worst <= 1e-5 and tight <= 1e-5


def test_both_entry_points_are_declared_and_exported():
    from pilco_amd import _lib
    header = open(os.path.join(ROOT, "include", "pilco_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("pilco_rollout_particles_grad", "pilco_rollout_particles_grad_rbf"):
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.SIGNATURES
        assert getattr(lib, name) is not None
    assert "#define PILCO_ABI_VERSION 2" in header or _lib.load_library().pilco_abi_version() == 2
