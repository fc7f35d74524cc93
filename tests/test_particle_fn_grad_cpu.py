"""The yardstick of the function-sample particle gradients (tests/helpers/particle_fn_grad_restatement.py) against torch
autograd through a torch restatement of the function-sample rollout, on the CPU; its mutants; the input conditions of the
device tests' tolerance; the declarations, exports and ctypes signatures of the two entry points; and the Python arguments
that are refused before any device call.  docs/particle_fn_gradients.md records the figures printed here (-s)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from helpers import particle_fn_grad_cases as fgc
from helpers import particle_fn_grad_restatement as fg
from helpers import particle_fn_restatement as rf
from helpers import particles_restatement as pr
from helpers.predict_restatement import se_ard

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=torch.float64)   # noqa: E731
# the project's bound for the marginal restatement (tests/test_particle_grad_cpu.py): both sides evaluate the same smooth
# function, the restatement's sums in np.longdouble and its sweep in float64
K_REF_BOUND = 1e-10
U53 = 2.0 ** -53


# ------------------------------------------------------------------ the function-sample rollout in torch
def _se(a, b, ls):
    d = (a[:, None, :] - b[None, :, :]) / ls
    return torch.exp(-0.5 * (d * d).sum(-1))


def _action_t(policy, par, x):
    if policy is None:
        return x[:, :0]
    U = par[1].shape[-1] if policy["kind"] == "rbf" else par[0].shape[0]
    ma = T(np.broadcast_to(np.asarray(policy.get("max_action", 1.0), np.float64).reshape(-1), (U,)))
    if policy["kind"] == "linear":
        W, b = par
        return ma * torch.sin(x @ W.T + b.reshape(1, -1))
    C, Y, ls = par
    noise = np.broadcast_to(np.asarray(policy["noise"], np.float64).reshape(-1), (U,))
    cols = []
    for k in range(U):
        K = _se(C, C, ls[k]) + float(noise[k]) * torch.eye(C.shape[0], dtype=torch.float64)
        cols.append(_se(x, C, ls[k]) @ torch.linalg.solve(K, Y[:, k]))
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


def _f_t(model, dr, v, z):
    """f (P, E) of every particle's own function at its own point z (P, D)"""
    X = T(model["X"])
    cols = []
    for e in range(np.asarray(model["Y"]).shape[1]):
        om, ph, w, ve = T(dr["omega"][e]), T(dr["phase"][e]), T(dr["w"][:, e, :]), T(v[:, e, :])
        amp = math.sqrt(2.0 * float(model["variance"][e]) / om.shape[0])
        k = float(model["variance"][e]) * _se(z, X, T(model["lengthscales"][e]))
        cols.append(amp * (w * torch.cos(z @ om.T + ph[None, :])).sum(1) + (k * ve).sum(1))
    return torch.stack(cols, 1)


def autograd(model, policy, terms, dr, v, x0, H, eps):
    """(J, grads, dx0) by torch autograd; dx0: the gradient of P J, every particle's own return."""
    if policy is None:
        par = []
    elif policy["kind"] == "linear":
        par = [T(policy["W"]).requires_grad_(), T(policy["b"]).reshape(-1).requires_grad_()]
    else:
        par = [T(policy["X"]).requires_grad_(), T(policy["Y"]).requires_grad_(), T(policy["lengthscales"]).requires_grad_()]
    x = T(x0).requires_grad_()
    xs, J = x, 0.0
    for t in range(H):
        J = J + _reward_t(terms, xs).mean()
        xs = xs + _f_t(model, dr, v, torch.cat([xs, _action_t(policy, par, xs)], 1))
        if eps is not None:
            xs = xs + T(np.sqrt(model["noise"])).reshape(1, -1) * T(eps[t])
    if H == 0:
        return 0.0, tuple(np.zeros(p.shape) for p in par), np.zeros(x0.shape)
    g = torch.autograd.grad(J, par + [x], allow_unused=True)
    g = [np.zeros(p.shape) if gi is None else gi.numpy() for gi, p in zip(g, par + [x])]
    return float(J.detach()), tuple(g[:-1]), g[-1] * x0.shape[0]


# ------------------------------------------------------------------ small random cases
def host_v(model, dr):
    """v (P, E, N) = (K_e + noise_e I)^-1 R_e in float64"""
    X = np.asarray(model["X"], np.float64)
    iK = [np.linalg.inv(se_ard(X, X, model["lengthscales"][e], model["variance"][e]) + model["noise"][e] * np.eye(X.shape[0]))
          for e in range(np.asarray(model["Y"]).shape[1])]
    return rf.v_of(model, dr, iK)[0].astype(np.float64)


def small_case(kind, reward="combined", seed=0, N=60, E=3, U=2, H=5, P=7, L=33):
    r = np.random.RandomState(seed)
    if kind == "none":
        U = 0
    D = E + U
    X = r.randn(N, D)
    Y = np.stack([np.sin(X @ r.randn(D)) * 0.3 + 0.05 * r.randn(N) for _ in range(E)], 1)
    model = dict(X=X, Y=Y, lengthscales=1.5 + r.rand(E, D), variance=0.5 + r.rand(E), noise=0.01 + 0.02 * r.rand(E))
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
    dr = rf.draws(seed + 100, model, P, L)
    return dict(model=model, policy=policy, terms=terms, dr=dr, v=host_v(model, dr), x0=0.3 * r.randn(P, E), H=H,
                eps=r.randn(H, P, E))


def _rel_diff(c, obs):
    eps = c["eps"] if obs else None
    xs, J = fg.forward_fn(c["model"], c["policy"], c["terms"], c["dr"], c["v"], c["x0"], c["H"], eps)
    grads, dx0 = fg.reverse_on(c["model"], c["policy"], c["terms"], c["dr"], c["v"], xs, c["H"])
    Ja, ga, dxa = autograd(c["model"], c["policy"], c["terms"], c["dr"], c["v"], c["x0"], c["H"], eps)
    worst = abs(J - Ja) / max(abs(Ja), 1e-300)
    assert len(grads) == len(ga)
    for a, b in zip(list(grads) + [dx0], list(ga) + [dxa]):
        worst = max(worst, np.abs(np.asarray(a).reshape(b.shape) - b).max() / max(np.abs(b).max(), 1e-300))
    return worst


AUTOGRAD_CASES = [(k, rw, obs) for k in ("linear", "rbf", "none") for rw in ("combined", "exponential", "linear") for obs in (False, True)]


@pytest.mark.parametrize("kind,reward,obs", AUTOGRAD_CASES, ids=["%s-%s-obs%d" % c for c in AUTOGRAD_CASES])
def test_restatement_matches_autograd(kind, reward, obs):
    k_ref = _rel_diff(small_case(kind, reward, seed=3), obs)
    print("K_ref %s %s obs=%d: %.3g" % (kind, reward, obs, k_ref))
    assert k_ref <= K_REF_BOUND


def test_short_horizons():
    for H in (0, 1, 2):
        c = small_case("linear", seed=5, H=H)
        assert _rel_diff(c, False) <= K_REF_BOUND
        xs, _ = fg.forward_fn(c["model"], c["policy"], c["terms"], c["dr"], c["v"], c["x0"], H)
        grads, dx0 = fg.reverse_on(c["model"], c["policy"], c["terms"], c["dr"], c["v"], xs, H)
        if H <= 1:
            assert not any(np.any(g) for g in grads)
            assert np.array_equal(dx0, fg.reward_grad(c["terms"], c["x0"]) if H else np.zeros_like(c["x0"]))


@pytest.mark.parametrize("name,value", [("SINE_SIGN", 1.0), ("USE_OMEGA", False), ("LS_POWER", 1), ("USE_AMP", False),
                                        ("USE_DELTA", False)])
def test_mutants_fail_the_autograd_check(monkeypatch, name, value):
    c = small_case("rbf", "combined", seed=3)
    assert _rel_diff(c, False) <= K_REF_BOUND
    monkeypatch.setattr(fg, name, value)
    diff = _rel_diff(c, False)
    print("mutant %s: %.3g" % (name, diff))
    assert diff > K_REF_BOUND


def test_reverse_fn_on_supplied_matrices_is_the_marginal_recursion():
    """reverse_fn is particle_grad_restatement.reverse with the matrices handed in: on the identity it carries lam through."""
    c = small_case("linear", seed=7, H=3)
    xs, _ = fg.forward_fn(c["model"], c["policy"], c["terms"], c["dr"], c["v"], c["x0"], 3)
    P, E = c["x0"].shape
    D = c["model"]["X"].shape[1]
    eye = np.zeros((P, E, D))
    eye[:, np.arange(E), np.arange(E)] = 1.0
    grads, dx0 = fg.reverse_fn(c["policy"], c["terms"], xs[:3], [eye, eye])
    assert not any(np.any(g) for g in grads)          # no dependence on u: no policy gradient
    want = sum(fg.reward_grad(c["terms"], xs[t]) for t in (2, 1, 0))
    assert np.allclose(dx0, want, rtol=0, atol=1e-15 * np.abs(want).max())


# ------------------------------------------------------------------ the input conditions of the device tests' tolerance
@pytest.mark.parametrize("kind", ["linear", "rbf", "none"])
def test_tolerance_conditions_under_the_restatement(kind):
    """The device tests hold every gradient to reverse_bound_fn plus the float64 floor and require that tolerance to be at
    most 1e-6 of the quantity's absolute-sum scale and of its largest entry: conditions on the model, asserted here on the
    restatement's own particles."""
    c = small_case(kind, "combined", seed=3, P=65)
    H, P = c["H"], 65
    xs, _ = fg.forward_fn(c["model"], c["policy"], c["terms"], c["dr"], c["v"], c["x0"], H)
    ref_g, ref_x = fg.reverse_on(c["model"], c["policy"], c["terms"], c["dr"], c["v"], xs, H)
    (bg, bx), (sg, sx) = fg.reverse_bound_fn(c["model"], c["policy"], c["terms"], c["dr"], c["v"], xs, H)
    for ref, b, sc, params in zip(list(ref_g) + [ref_x], list(bg) + [bx], list(sg) + [sx], [True] * len(ref_g) + [False]):
        b, sc = np.asarray(b).reshape(np.shape(ref)), np.asarray(sc).reshape(np.shape(ref))
        tol = b + ((4 * P if params else 0) + 4096) * U53 * sc
        cond, tight = float((tol / np.maximum(sc, 1e-300)).max()), float(tol.max() / np.abs(ref).max())
        print("tolerance %s: tolerance / scale = %.3g, largest tolerance / largest entry = %.3g" % (kind, cond, tight))
        assert cond <= 1e-6 and tight <= 1e-6
        assert np.all(np.abs(ref) <= sc * (1 + 1e-12))


def tolerance_of(b, sc, P, params):
    """The device tests' tolerance: the propagated bound plus the float64 floor of tests/test_gpu_particle_grad.py (4096 * 2^-53
    of the absolute-sum scale for a particle's chain, 4 P 2^-53 more for a sum over the particles)."""
    return b + ((4 * P if params else 0) + 4096) * U53 * sc


DEVICE_CASES = [c for c in fgc.CASES if c[3] >= 2]


@pytest.mark.parametrize("name,P,L,H,obs", DEVICE_CASES, ids=["%s-P%d-L%d-H%d-obs%d" % c for c in DEVICE_CASES])
def test_tolerance_conditions_of_the_device_cases(name, P, L, H, obs):
    """The same two conditions on the models the device tests run (helpers/particle_fn_grad_cases.py), on the restatement's
    own particles and draws: a model that misses them is replaced, the cap is not."""
    s = fgc.setup(name)
    x0 = fgc.x0_of(name, P, 100 + P)
    dr = rf.draws(300 + P + H, s["model"], P, L)
    v = host_v(s["model"], dr)
    eps = np.random.RandomState(1).randn(H, P, s["E"]) if obs else None
    xs, _ = fg.forward_fn(s["model"], s["policy"], s["terms"], dr, v, x0, H, eps)
    ref_g, ref_x = fg.reverse_on(s["model"], s["policy"], s["terms"], dr, v, xs, H)
    (bg, bx), (sg, sx) = fg.reverse_bound_fn(s["model"], s["policy"], s["terms"], dr, v, xs, H)
    cond = tight = 0.0
    for ref, b, sc, params in zip(list(ref_g) + [ref_x], list(bg) + [bx], list(sg) + [sx], [True] * len(ref_g) + [False]):
        b, sc = np.asarray(b).reshape(np.shape(ref)), np.asarray(sc).reshape(np.shape(ref))
        tol = tolerance_of(b, sc, P, params)
        cond = max(cond, float((tol / np.maximum(sc, 1e-300)).max()))
        tight = max(tight, float(tol.max() / np.abs(ref).max()))
    print("tolerance %s P=%d L=%d H=%d: tolerance / scale = %.3g, largest tolerance / largest entry = %.3g" % (name, P, L, H, cond, tight))
    assert cond <= 1e-6 and tight <= 1e-6


def test_the_count_of_rounding_steps():
    assert fg.c_prime(300, 100, 5) == 300 + 3 + 15 + 16 + 6 and fg.c_prime(1, 64, 3) == 64 + 3 + 9 + 16 + 6


# ------------------------------------------------------------------ declarations, exports, ctypes
NAMES = ("pilco_rollout_particles_fn_grad", "pilco_rollout_particles_fn_grad_rbf")


def test_entry_points_are_declared_exported_and_bound():
    from pilco_amd import _lib
    header = open(os.path.join(ROOT, "include", "pilco_hip.h")).read()
    assert re.search(r"#define PILCO_HIP_ABI_VERSION 2\b", header)
    for name in NAMES:
        assert re.search(r"\bint %s\(pilco_ctx\* ctx, const pilco_policy\* policy," % name, header), name
        assert name in _lib.SIGNATURES
    lin, rbf = (_lib.SIGNATURES[n][1] for n in NAMES)
    assert len(lin) == 17 and len(rbf) == 23
    for sig in (lin, rbf):
        assert sig[10] == ctypes.POINTER(_lib.FunctionDraws) and sig[11] == ctypes.POINTER(_lib.FunctionDrawsOut)
    assert rbf[16] == ctypes.c_int
    so = os.path.join(ROOT, "pilco_amd", "libpilco_hip.so")
    assert os.path.exists(so), "libpilco_hip.so is not built"
    lib = ctypes.CDLL(so)
    assert lib.pilco_abi_version() == 2
    for name in NAMES:
        assert hasattr(lib, name)


# ------------------------------------------------------------------ Python arguments refused before any device call
class _NoDevice:
    """stands where the context would: any use is a device call"""

    def __getattr__(self, name):
        raise AssertionError("device call: " + name)


def _pilco(sparse=False):
    from pilco_amd import controllers
    from pilco_amd.models import PILCO
    r = np.random.RandomState(0)
    X, Y = r.randn(20, 3), r.randn(20, 2)
    ctx = _NoDevice()
    ctl = controllers.LinearController(2, 1, ctx=ctx)
    return PILCO((X, Y), num_induced_points=5 if sparse else None, controller=ctl, ctx=ctx)


def test_dynamics_argument_is_checked_before_any_device_call():
    p = _pilco()
    with pytest.raises(ValueError, match="dynamics"):
        p.particle_value_and_gradient(dynamics="functions")
    with pytest.raises(ValueError, match="dynamics"):
        p.particle_value_and_gradient(dynamics=None)
    with pytest.raises(NotImplementedError, match="exact GP"):
        _pilco(sparse=True).particle_value_and_gradient(dynamics="function")


def test_particle_options_keys():
    p = _pilco()
    with pytest.raises(ValueError, match="unknown particle_options"):
        p.optimize_policy(objective="particles", particle_options=dict(dynamic="function"))
    with pytest.raises(ValueError, match="dynamics"):
        p.optimize_policy(objective="particles", particle_options=dict(dynamics="sampled", num_features=64))
    with pytest.raises(NotImplementedError, match="exact GP"):
        _pilco(sparse=True).optimize_policy(objective="particles", particle_options=dict(dynamics="function"))
    with pytest.raises(ValueError, match="go with objective"):
        p.optimize_policy(particle_options=dict(dynamics="function"))
