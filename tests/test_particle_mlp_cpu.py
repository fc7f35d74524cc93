"""The yardstick of the MLP-policy particle paths (tests/helpers/particle_mlp_restatement.py) against torch autograd through a
torch restatement of the same rollouts, on the CPU; the boundary (header, ABI, ctypes, exports); the Python surface of
MlpController and of PILCO with one, on a context that raises on any use; the count of rounding steps; and the input conditions
of the device tests' tolerance.  docs/particle_mlp.md records the figures printed here (-s)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from helpers import particle_fn_restatement as rf
from helpers import particle_mlp_cases as mc
from helpers import particle_mlp_restatement as pm
from helpers import particles_restatement as pr
from helpers.predict_restatement import se_ard

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=torch.float64)   # noqa: E731
K_REF_BOUND = 1e-10   # the project's bound for restatements (tests/test_particle_grad_cpu.py)
U53 = 2.0 ** -53
KEYS = ("W1", "b1", "W2", "b2")


# ------------------------------------------------------------------ the two rollouts in torch
def _se(a, b, ls):
    d = (a[:, None, :] - b[None, :, :]) / ls
    return torch.exp(-0.5 * (d * d).sum(-1))


def _action_t(policy, par, x):
    W1, b1, W2, b2 = par
    s = torch.tanh(x @ W1.T + b1.reshape(1, -1)) @ W2.T + b2.reshape(1, -1)
    if not policy["squash"]:
        return s
    return T(np.broadcast_to(np.asarray(policy["max_action"], np.float64).reshape(-1), (W2.shape[0],))) * torch.sin(s)


def _reward_t(terms, x):
    tot = torch.zeros(x.shape[0], dtype=torch.float64)
    for t in terms:
        if t["kind"] == "exponential":
            d = x - (T(t["t"]).reshape(1, -1) if t.get("t") is not None else 0.0)
            tot = tot + float(t.get("coef", 1.0)) * torch.exp(-0.5 * torch.einsum("pi,ij,pj->p", d, T(t["W"]), d))
        else:
            tot = tot + float(t.get("coef", 1.0)) * (x @ T(t["W"]).reshape(-1))
    return tot


def _marginal_t(model, z, eps, obs):
    """the increment mu + sqrt(v) eps of the exact GP posterior at z (P, D)"""
    X = T(model["X"])
    cols = []
    for e in range(np.asarray(model["Y"]).shape[1]):
        ls, sf2, sn2 = T(model["lengthscales"][e]), float(model["variance"][e]), float(model["noise"][e])
        K = sf2 * _se(X, X, ls) + sn2 * torch.eye(X.shape[0], dtype=torch.float64)
        ks = sf2 * _se(z, X, ls)
        mu = ks @ torch.linalg.solve(K, T(model["Y"][:, e]))
        v = sf2 - (ks * torch.linalg.solve(K, ks.T).T).sum(1) + (sn2 if obs else 0.0)
        cols.append(mu + torch.sqrt(v) * eps[:, e])
    return torch.stack(cols, 1)


def _fn_t(model, dr, v, z):
    X = T(model["X"])
    cols = []
    for e in range(np.asarray(model["Y"]).shape[1]):
        om, ph, w, ve = T(dr["omega"][e]), T(dr["phase"][e]), T(dr["w"][:, e, :]), T(v[:, e, :])
        amp = float(np.sqrt(2.0 * float(model["variance"][e]) / om.shape[0]))
        k = float(model["variance"][e]) * _se(z, X, T(model["lengthscales"][e]))
        cols.append(amp * (w * torch.cos(z @ om.T + ph[None, :])).sum(1) + (k * ve).sum(1))
    return torch.stack(cols, 1)


def autograd(c, dynamics, obs):
    """(J, (dW1, db1, dW2, db2), dx0) by torch autograd; dx0: the gradient of P J, every particle's own return."""
    policy, model = c["policy"], c["model"]
    par = [T(np.asarray(policy[k]).reshape(-1) if k[0] == "b" else policy[k]).requires_grad_() for k in KEYS]
    x = T(c["x0"]).requires_grad_()
    xs, J = x, 0.0
    for t in range(c["H"]):
        J = J + _reward_t(c["terms"], xs).mean()
        z = torch.cat([xs, _action_t(policy, par, xs)], 1)
        if dynamics == "marginal":
            xs = xs + _marginal_t(model, z, T(c["eps"][t]), obs)
        else:
            xs = xs + _fn_t(model, c["dr"], c["v"], z)
            if obs:
                xs = xs + T(np.sqrt(model["noise"])).reshape(1, -1) * T(c["eps"][t])
    g = torch.autograd.grad(J, par + [x], allow_unused=True)
    g = [np.zeros(p.shape) if gi is None else gi.numpy() for gi, p in zip(g, par + [x])]
    return float(J.detach()), tuple(g[:-1]), g[-1] * c["x0"].shape[0]


# ------------------------------------------------------------------ the restatement's own rollouts
def host_v(model, dr):
    X = np.asarray(model["X"], np.float64)
    iK = [np.linalg.inv(se_ard(X, X, model["lengthscales"][e], model["variance"][e]) + model["noise"][e] * np.eye(X.shape[0]))
          for e in range(np.asarray(model["Y"]).shape[1])]
    return rf.v_of(model, dr, iK)[0].astype(np.float64)


def rollout(c, dynamics, obs, bound=False):
    """The restatement's states xs (H+1, P, E), J, the step matrices of t < H - 1 and (bound) their per-entry bounds."""
    model, policy, H = c["model"], c["policy"], c["H"]
    xs, J = [np.asarray(c["x0"], np.float64)], 0.0
    for t in range(H):
        J += pr.reward(c["terms"], xs[-1]).mean()
        if dynamics == "marginal":
            xn = pm.step_marginal(model, policy, xs[-1], c["eps"][t], obs)[0]
        else:
            xn = pm.step_fn(model, policy, c["dr"], c["v"], xs[-1])[0]
            if obs:
                xn = xn + np.sqrt(np.asarray(model["noise"], np.float64))[None, :] * c["eps"][t]
        xs.append(xn)
    return np.stack(xs), J, matrices(c, dynamics, obs, xs, bound)


def matrices(c, dynamics, obs, xs, bound=False):
    out = []
    for t in range(c["H"] - 1):
        if dynamics == "marginal":
            out.append(pm.step_matrix_marginal(c["model"], c["policy"], xs[t], c["eps"][t], obs, bound=bound))
        else:
            out.append(pm.step_matrix_fn(c["model"], c["policy"], c["dr"], c["v"], xs[t], bound=bound))
    return out


def small_case(seed=3, N=60, E=3, U=2, H=5, P=7, Hn=5, L=33, squash=True):
    r = np.random.RandomState(seed)
    D = E + U
    X = r.randn(N, D)
    Y = np.stack([np.sin(X @ r.randn(D)) * 0.3 + 0.05 * r.randn(N) for _ in range(E)], 1)
    model = dict(X=X, Y=Y, lengthscales=1.5 + r.rand(E, D), variance=0.5 + r.rand(E), noise=0.01 + 0.02 * r.rand(E), Z=None)
    policy = dict(W1=0.8 * r.randn(Hn, E), b1=0.3 * r.randn(Hn), W2=0.7 * r.randn(U, Hn), b2=0.2 * r.randn(U),
                  max_action=np.array([1.3, 0.7])[:U], squash=squash)
    expo = dict(kind="exponential", W=np.eye(E) + 0.4 * r.randn(E, E), t=0.3 * r.randn(E), coef=1.2)   # asymmetric W
    terms = [expo, dict(kind="linear", W=r.randn(E), coef=-0.3)]
    dr = rf.draws(seed + 100, model, P, L)
    return dict(model=model, policy=policy, terms=terms, dr=dr, v=host_v(model, dr), x0=0.3 * r.randn(P, E), H=H,
                eps=r.randn(H, P, E))


def _rel_diff(c, dynamics, obs):
    xs, J, mats = rollout(c, dynamics, obs)
    grads, dx0 = pm.reverse(c["policy"], c["terms"], xs[:c["H"]], mats)
    Ja, ga, dxa = autograd(c, dynamics, obs)
    worst = abs(J - Ja) / max(abs(Ja), 1e-300)
    for a, b in zip(list(grads) + [dx0], list(ga) + [dxa]):
        worst = max(worst, np.abs(np.asarray(a).reshape(b.shape) - b).max() / max(np.abs(b).max(), 1e-300))
    return worst


# ------------------------------------------------------------------ 1. the restatement against autograd
@pytest.mark.parametrize("squash", [True, False])
@pytest.mark.parametrize("obs", [False, True])
@pytest.mark.parametrize("dynamics", ["marginal", "function"])
def test_restatement_matches_autograd(dynamics, obs, squash):
    k_ref = _rel_diff(small_case(squash=squash), dynamics, obs)
    print("K_ref %s obs=%d squash=%d: %.3g" % (dynamics, obs, squash, k_ref))
    assert k_ref <= K_REF_BOUND


def test_action_and_jacobian_against_autograd():
    c = small_case()
    par = [T(np.asarray(c["policy"][k])) for k in KEYS]
    x = T(c["x0"]).requires_grad_()
    u = _action_t(c["policy"], par, x)
    assert np.abs(pm.action(c["policy"], c["x0"]) - u.detach().numpy()).max() <= K_REF_BOUND * np.abs(u.detach().numpy()).max()
    J = pm.action_jacobian(c["policy"], c["x0"])
    for k in range(u.shape[1]):
        g = torch.autograd.grad(u[:, k].sum(), x, retain_graph=True)[0].numpy()
        assert np.abs(J[:, k, :] - g).max() <= K_REF_BOUND * np.abs(g).max()


@pytest.mark.parametrize("name,value", [("ds_factor", lambda p, x: np.ones((np.shape(x)[0], np.shape(p["W2"])[0]))),
                                        ("action", lambda p, x: pr.linear_action(x, np.asarray(p["W2"]) @ np.asarray(p["W1"]), p["b2"]))])
def test_mutants_fail_the_autograd_check(monkeypatch, name, value):
    c = small_case()
    assert _rel_diff(c, "function", False) <= K_REF_BOUND
    monkeypatch.setattr(pm, name, value)
    assert _rel_diff(c, "function", False) > K_REF_BOUND


def test_short_horizons_and_constant_action():
    from helpers.particle_grad_restatement import reward_grad
    for H in (1, 2):
        c = small_case(H=H)
        assert _rel_diff(c, "marginal", False) <= K_REF_BOUND
    c = small_case(H=1)
    xs, _, mats = rollout(c, "function", False)
    grads, dx0 = pm.reverse(c["policy"], c["terms"], xs[:1], mats)
    assert not any(np.any(g) for g in grads) and np.array_equal(dx0, reward_grad(c["terms"], c["x0"]))
    c = small_case(H=4)
    c["policy"]["W2"] = np.zeros_like(c["policy"]["W2"])          # a constant action: nothing reaches the hidden layer
    xs, _, mats = rollout(c, "function", False)
    (dW1, db1, dW2, db2), _ = pm.reverse(c["policy"], c["terms"], xs[:4], mats)
    assert not np.any(dW1) and not np.any(db1) and np.any(dW2) and np.any(db2)


# ------------------------------------------------------------------ 2. the boundary
NAMES = ("pilco_set_policy_mlp", "pilco_rollout_particles_grad_mlp", "pilco_rollout_particles_fn_grad_mlp")


def test_entry_points_are_declared_exported_and_bound():
    from pilco_amd import _lib
    header = open(os.path.join(ROOT, "include", "pilco_hip.h")).read()
    assert re.search(r"#define PILCO_HIP_ABI_VERSION 2\b", header)
    assert re.search(r"#define PILCO_MAX_MLP_HIDDEN 256\b", header) and re.search(r"PILCO_POLICY_MLP = 3\b", header)
    assert _lib.POLICY_MLP == 3 and _lib.MAX_MLP_HIDDEN == 256
    for name in NAMES:
        assert re.search(r"\bint %s\(pilco_ctx\* ctx," % name, header), name
        assert name in _lib.SIGNATURES
    # pilco_policy keeps its layout
    body = re.search(r"typedef struct pilco_policy \{(.*?)\} pilco_policy;", header, re.S).group(1)
    assert re.findall(r"(?:const double\*|int) (\w+);", body) == ["kind", "state_dim", "control_dim", "W", "b", "max_action", "squash"]
    assert [f[0] for f in _lib.PolicyStruct._fields_] == ["kind", "state_dim", "control_dim", "W", "b", "max_action", "squash"]
    dp = ctypes.POINTER(ctypes.c_double)
    assert _lib.SIGNATURES[NAMES[0]][1][1:] == [ctypes.c_int] * 3 + [dp] * 4
    lin, mlp = _lib.SIGNATURES["pilco_rollout_particles_grad"][1], _lib.SIGNATURES[NAMES[1]][1]
    assert mlp[:12] == lin[:12] and mlp[12:] == [dp] * 5 and len(mlp) == len(lin) + 2
    lin, mlp = _lib.SIGNATURES["pilco_rollout_particles_fn_grad"][1], _lib.SIGNATURES[NAMES[2]][1]
    assert mlp[:14] == lin[:14] and mlp[14:] == [dp] * 5 and len(mlp) == len(lin) + 2
    so = os.path.join(ROOT, "pilco_amd", "libpilco_hip.so")
    assert os.path.exists(so), "libpilco_hip.so is not built"
    lib = ctypes.CDLL(so)
    assert lib.pilco_abi_version() == 2
    for name in NAMES:
        assert hasattr(lib, name)
    n_decl = len(re.findall(r"^(?:int|const char\*) pilco_\w+\(", header, re.M))
    for doc in ("README.md", "INTEGRATION.md"):
        assert int(re.search(r"(\d+) entry points", open(os.path.join(ROOT, doc)).read()).group(1)) == n_decl == 64


# ------------------------------------------------------------------ 3. the Python surface, without a device
class _NoDevice:
    """stands where the context would: any use is a device call"""

    def __getattr__(self, name):
        raise AssertionError("device call: " + name)


def _controller(E=3, U=2, Hn=5, seed=0):
    from pilco_amd.controllers import MlpController
    np.random.seed(seed)
    ctl = MlpController(E, U, num_hidden=Hn, max_action=np.array([1.3, 0.7])[:U], ctx=_NoDevice())
    ctl.b1.assign(0.3 * np.random.randn(Hn))
    return ctl


def test_controller_parameters_and_actions():
    ctl = _controller()
    assert [p.shape for p in ctl.trainable_parameters] == [(5, 3), (5,), (2, 5), (1, 2)]
    assert [p.name for p in ctl.trainable_parameters] == list(KEYS)
    x = np.random.RandomState(1).randn(4, 3)
    for squash in (True, False):
        want = pm.action(pm.policy_of(ctl, squash), x)
        for p in range(4):
            M, S, V = ctl.compute_action(x[p:p + 1], np.zeros((3, 3)), squash=squash)
            assert M.shape == (1, 2) and S.shape == (2, 2) and V.shape == (3, 2) and not np.any(S) and not np.any(V)
            assert np.abs(M[0] - want[p]).max() <= 8 * U53 * (1.0 + np.abs(want[p]).max())
    with pytest.raises(NotImplementedError, match='objective="particles"'):
        ctl.compute_action(x[:1], 1e-300 * np.eye(3))
    with pytest.raises(ValueError):
        from pilco_amd.controllers import MlpController
        MlpController(3, 2, num_hidden=257)


def test_action_jacobian_against_central_differences():
    ctl = _controller()
    LD = np.longdouble
    x = np.random.RandomState(2).randn(3)
    J = ctl.action_jacobian(x)
    pol = pm.policy_of(ctl)
    W1, b1, W2, b2 = (np.asarray(pol[k], LD) for k in KEYS)

    def act(xq):
        return np.asarray(pol["max_action"], LD) * np.sin(W2 @ np.tanh(W1 @ xq + b1) + b2.reshape(-1))

    h = LD(2.0) ** -21          # longdouble central differences: truncation h^2 ~ 2e-13, rounding 2^-64 / h ~ 1e-13
    for e in range(3):
        d = np.zeros(3, LD)
        d[e] = h
        fd = (act(np.asarray(x, LD) + d) - act(np.asarray(x, LD) - d)) / (2 * h)
        assert np.abs(J[:, e] - fd.astype(np.float64)).max() <= 1e-10 * np.abs(J).max()
    assert np.abs(J - pm.action_jacobian(pol, x[None])[0]).max() <= 64 * U53 * np.abs(J).max()


def test_randomize_draws_in_the_stated_order():
    ctl = _controller(E=3, U=2, Hn=4)
    np.random.seed(12)
    ctl.randomize()
    np.random.seed(12)
    W1 = np.random.normal(size=(4, 3)) / np.sqrt(3)
    W2 = np.random.normal(size=(2, 4)) / np.sqrt(4)
    b2 = np.random.normal(size=(1, 2))
    after = np.random.normal()
    assert np.array_equal(ctl.W1.numpy(), W1) and np.array_equal(ctl.W2.numpy(), W2) and np.array_equal(ctl.b2.numpy(), b2)
    assert not np.any(ctl.b1.numpy())
    np.random.seed(12)
    ctl.randomize()
    assert np.random.normal() == after          # nothing else was drawn


def _pilco(sparse=False):
    from pilco_amd.models import PILCO
    r = np.random.RandomState(0)
    X = r.randn(20, 5)
    Y = r.randn(20, 3)
    p = PILCO((X, Y), controller=_controller(), horizon=3, **(dict(num_induced_points=5) if sparse else {}))
    p._ctx = _NoDevice()
    p.mgpr._ctx = _NoDevice()
    return p


def test_moment_matching_refuses_a_network_before_any_device_call():
    p = _pilco()
    m, S = p.m_init, p.S_init
    for call in (lambda: p.predict(m, S, 2), lambda: p.predict_trajectory(m, S, 2), lambda: p.propagate(m, S), p.compute_reward,
                 p.training_loss, p.value_and_gradient, lambda: p.optimize_policy(maxiter=1, verbose=False),
                 lambda: p.optimize_policy(maxiter=1, verbose=False, objective="moment_matching")):
        with pytest.raises(NotImplementedError, match="MlpController"):
            call()
    with pytest.raises(NotImplementedError, match="conditioned"):
        p.particle_value_and_gradient(m, S, 2, num_particles=4, dynamics="conditioned")
    assert p.compute_action(m).shape == (1, 2)          # the host action: drives an environment, feeds linearize
    assert [q.name for q in p.trainable_parameters[-4:]] == list(KEYS)


def test_policy_params_round_trip():
    from pilco_amd.training import _policy_params
    ctl = _controller()
    get, put = _policy_params(ctl)
    u = get()
    assert u.shape == (5 * 3 + 5 + 2 * 5 + 2,)
    assert np.array_equal(u, np.concatenate([np.asarray(getattr(ctl, k).numpy()).ravel() for k in KEYS]))
    v = np.arange(u.size, dtype=np.float64) * 0.01 - 0.1
    put(v)
    assert np.array_equal(get(), v) and np.array_equal(ctl.b2.numpy(), v[-2:].reshape(1, 2))
    assert np.array_equal(ctl.W2.numpy(), v[20:30].reshape(2, 5))


# ------------------------------------------------------------------ 4. the count, and the tolerance's input conditions
def test_the_count_of_rounding_steps():
    assert pm.c_mlp(3, 64) == (64 + 9, 4) and pm.c_mlp(10, 256) == (265, 11) and pm.c_mlp(1, 1) == (10, 2)


def tolerance_of(b, sc, P, params):
    """The device tests' tolerance: the propagated bound plus the float64 floor of tests/test_gpu_particle_grad.py (4096 * 2^-53
    of the absolute-sum scale for a particle's chain, 4 P 2^-53 more for a sum over the particles)."""
    return b + ((4 * P if params else 0) + 4096) * U53 * sc


def device_case(dynamics, name, Hn, P, H, obs, squash):
    """A case of helpers/particle_mlp_cases.py under the restatement alone (its own particles and draws)."""
    s = mc.setup(name)
    c = dict(model=s["model"], policy=mc.network(name, Hn, squash=squash), terms=s["terms"], x0=mc.x0_of(name, P, 100 + P), H=H,
             eps=np.random.RandomState(1).randn(H, P, s["E"]))
    if dynamics == "function":
        c["dr"] = rf.draws(300 + P + H, s["model"], P, mc.L)
        c["v"] = host_v(s["model"], c["dr"])
    return c


def conditions(c, dynamics, obs, xs, P):
    """(tolerance / scale, largest tolerance / largest entry) over the five quantities, on the states xs"""
    pairs = matrices(c, dynamics, obs, xs, bound=True)
    mats, dmats = [a for a, _ in pairs], [d for _, d in pairs]
    ref_g, ref_x = pm.reverse(c["policy"], c["terms"], xs[:c["H"]], mats)
    (bg, bx), (sg, sx) = pm.reverse_bound(c["policy"], c["terms"], xs[:c["H"]], mats, dmats)
    cond = tight = 0.0
    for ref, b, sc, params in zip(list(ref_g) + [ref_x], list(bg) + [bx], list(sg) + [sx], [True] * 4 + [False]):
        b, sc = np.asarray(b).reshape(np.shape(ref)), np.asarray(sc).reshape(np.shape(ref))
        assert np.all(np.abs(ref) <= sc * (1 + 1e-12))
        tol = tolerance_of(b, sc, P, params)
        cond = max(cond, float((tol / np.maximum(sc, 1e-300)).max()))
        tight = max(tight, float(tol.max() / np.abs(ref).max()))
    return cond, tight


DEVICE_CASES = [c for c in mc.CASES if c[4] >= 2]


@pytest.mark.parametrize("dynamics,name,Hn,P,H,obs,squash", DEVICE_CASES, ids=["%s-%s-Hn%d-P%d-H%d-obs%d-sq%d" % c for c in DEVICE_CASES])
def test_tolerance_conditions_of_the_device_cases(dynamics, name, Hn, P, H, obs, squash):
    """The device tests' tolerance is at most 1e-6 of every quantity's absolute-sum scale and of its largest entry: conditions
    on the models and networks, asserted on the restatement's own particles.  A model that misses them is replaced, the cap
    is not."""
    c = device_case(dynamics, name, Hn, P, H, obs, squash)
    xs, _, _ = rollout(c, dynamics, obs)
    cond, tight = conditions(c, dynamics, obs, xs, P)
    print("tolerance %s %s Hn=%d P=%d H=%d: tolerance / scale = %.3g, largest tolerance / largest entry = %.3g"
          % (dynamics, name, Hn, P, H, cond, tight))
    assert cond <= 1e-6 and tight <= 1e-6


@pytest.mark.parametrize("name,Hn", [("n300", 64), ("syn5a", 1), ("syn65b", 256), ("predictions", 65)])
def test_action_bound_is_small_against_its_scale(name, Hn):
    pol = mc.network(name, Hn)
    b, sc = pm.action_bound(pol, mc.x0_of(name, 65, 3))
    assert np.all(b <= 1e-6 * sc) and np.all(b > 0)
