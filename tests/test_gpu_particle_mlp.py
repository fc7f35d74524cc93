"""Neural-network policies on the particle paths on the MI355X: PILCO_POLICY_MLP in pilco_rollout_particles[_events], _fn,
_cond and pilco_debug_particle_actions, pilco_rollout_particles_grad_mlp / _fn_grad_mlp (csrc/particles.hip,
csrc/particles_grad.hip; docs/particle_mlp.md), controllers.MlpController, PILCO.particle_value_and_gradient and
optimize_policy(objective="particles") with one.  The yardstick is tests/helpers/particle_mlp_restatement.py, which
tests/test_particle_mlp_cpu.py pins to torch autograd.  Every figure a bound is held against is printed before the
assertion (-s)."""
import ctypes as C

import numpy as np
import pytest

from helpers import particle_fn_restatement as rf
from helpers import particle_mlp_cases as mc
from helpers import particle_mlp_restatement as pm
from helpers import particles_restatement as pr
from helpers.particle_grad_restatement import reward_grad

pytestmark = pytest.mark.gpu
E_SHAPE, E_STATE = 1, 5
U53 = 2.0 ** -53
LD = np.longdouble
BUDGET = "PILCO_PARTICLE_GRAD_BUDGET"
KEYS = ("omega", "phase", "w", "xi")
PS = (1, 63, 64, 65, 129, 257)
_CTX = None
_OBJ = {}


@pytest.fixture(scope="module", autouse=True)
def own_ctx():
    """The models of this module live on a context of their own (closed at the end), not on the process-wide default."""
    from pilco_amd import _lib
    global _CTX
    _CTX = _lib.Context(device=0)
    yield _CTX
    _OBJ.clear()
    _CTX.close()


def _obj(name):
    """The PILCO object of a model of helpers/particle_mlp_cases.py on this module's context, with its rewards and an
    MlpController whose parameters _net assigns."""
    if name in _OBJ:
        return _OBJ[name]
    from pilco_amd import controllers, rewards
    from pilco_amd.models import PILCO
    s = mc.setup(name)
    cfg, Z, E, U = s["cfg"], s["Z"], s["E"], s["U"]
    ex, li = s["terms"]
    rw = rewards.CombinedRewards(E, [rewards.ExponentialReward(E, W=ex["W"], t=ex["t"].reshape(1, E)), rewards.LinearReward(E, li["W"])],
                                 coefs=[ex["coef"], li["coef"]])
    ctl = controllers.MlpController(E, U, num_hidden=1, max_action=s["maxact"], ctx=_CTX)
    p = PILCO((cfg["X"], cfg["Y"]), num_induced_points=None if Z is None else Z.shape[0], controller=ctl, reward=rw, ctx=_CTX)
    for i, mdl in enumerate(p.mgpr.models):
        mdl.kernel.lengthscales.assign(cfg["lengthscales"][i])
        mdl.kernel.variance.assign(cfg["variance"][i])
        mdl.likelihood.variance.assign(cfg["noise"][i])
    if Z is not None:
        for mdl in p.mgpr.models:
            mdl.inducing_variable.Z.assign(Z)
    _OBJ[name] = p
    return p


def _net(p, pol):
    """Give p's controller the network of the restatement's policy dict pol (any number of hidden units)."""
    from pilco_amd import controllers
    from pilco_amd.params import Parameter
    ctl = p.controller
    Hn = np.asarray(pol["W1"]).shape[0]
    if ctl.num_hidden != Hn:
        ctl.num_hidden = Hn
        ctl.W1, ctl.b1 = Parameter(np.zeros((Hn, ctl.state_dim)), name="W1"), Parameter(np.zeros(Hn), name="b1")
        ctl.W2 = Parameter(np.zeros((ctl.control_dim, Hn)), name="W2")
    for k in ("W1", "b1", "W2", "b2"):
        getattr(ctl, k).assign(np.asarray(pol[k]))
    ctl.max_action = pol["max_action"]
    assert isinstance(ctl, controllers.MlpController)
    return p


def _spec(p, pol):
    return _net(p, pol).controller.policy_spec(bool(pol["squash"]))


def _ready(p):
    p.mgpr._user_factors = None
    p.mgpr._ensure_factorized()


def _actions(p, pol, x):
    _ready(p)
    return _CTX.particle_actions(_spec(p, pol), x)


def _grad(p, pol, dynamics, x0, H, draws=None, eps=None, seed=0, obs=False, want_draws=False):
    """-> (J, reward_steps, (dW1, db1, dW2, db2), dx0, draws or None)"""
    _ready(p)
    spec = _spec(p, pol)
    if dynamics == "function":
        out = _CTX.rollout_particles_fn_grad_mlp(spec, p._reward_terms(), x0, H, num_features=mc.L,
                                                 function_draws=None if draws is None else {k: draws[k] for k in KEYS}, eps=eps,
                                                 seed=seed, observation_noise=obs, want_dx0=True, want_draws=want_draws)
        return out[0], out[1], tuple(out[2:6]), out[6], out[7]
    out = _CTX.rollout_particles_grad_mlp(spec, p._reward_terms(), x0, H, eps=eps, seed=seed, observation_noise=obs, want_dx0=True)
    return out[0], out[1], tuple(out[2:6]), out[6], None


def _fwd(p, pol, dynamics, x0, H, draws=None, eps=None, seed=0, obs=False, want_draws=False, events=None):
    """-> (mean, cov, reward_steps, particles, eps, counts, first_hit, draws)"""
    _ready(p)
    spec = _spec(p, pol)
    if dynamics == "function":
        return _CTX.rollout_particles_fn(spec, p._reward_terms(), x0, H, num_features=mc.L,
                                         function_draws=None if draws is None else {k: draws[k] for k in KEYS}, eps=eps, seed=seed,
                                         observation_noise=obs, want_particles=True, want_draws=want_draws, events=events)
    if dynamics == "conditioned":
        out = _CTX.rollout_particles_cond(spec, p._reward_terms(), x0, H, eps=eps, seed=seed, observation_noise=obs,
                                          want_particles=True, events=events, want_path=True)
        return tuple(out[:7]) + (out[9],)          # the last: path_factor
    out = _CTX.rollout_particles(spec, p._reward_terms(), x0, H, eps=eps, seed=seed, observation_noise=obs, want_particles=True,
                                 events=events)
    return tuple(out) + (None,) * (8 - len(out))


def _flat(res):
    return [np.atleast_1d(res[0]), res[1]] + [np.asarray(g) for g in res[2]] + [res[3]]


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(_flat(a), _flat(b)))


# ------------------------------------------------------------------ 1. actions
@pytest.mark.parametrize("Hn", mc.HIDDEN)
@pytest.mark.parametrize("name", ["n300", "syn5a", "syn65a", "w8"])
def test_actions_against_the_restatement(name, Hn):
    p = _obj(name)
    worst = 0.0
    for squash in (True, False):
        pol = mc.network(name, Hn, squash=squash)
        for P in PS:
            x = mc.x0_of(name, P, 10 + P)
            u = _actions(p, pol, x)
            b, sc = pm.action_bound(pol, x)
            err = np.abs(u - pm.action(pol, x))
            worst = max(worst, float((err / b).max()))
            assert u.shape == (P, mc.setup(name)["U"]) and np.all(err <= b), (squash, P, float((err / b).max()))
            assert np.all(b <= 1e-6 * sc)
    print("actions %s Hn=%d: largest error / bound = %.3g" % (name, Hn, worst))


def test_actions_at_the_edges_of_tanh():
    name = "n300"
    p, s = _obj(name), mc.setup(name)
    E, U = s["E"], s["U"]
    x = mc.x0_of(name, 65, 4)
    pol = mc.network(name, 64)
    # saturated units: pre-activations of +-40, h = +-1 exactly, the action the sine of the signed row sums of W2
    sat = dict(pol, W1=np.zeros((64, E)), b1=40.0 * np.where(np.arange(64) % 2, -1.0, 1.0))
    u = _actions(p, sat, x)
    h = np.where(np.arange(64) % 2, -1.0, 1.0)
    want = pm.action(sat, x)
    assert np.all(np.abs(u - want) <= pm.action_bound(sat, x)[0])
    assert np.all(np.abs(want - s["maxact"] * np.sin(sat["W2"] @ h + sat["b2"])) <= 1e-14)
    assert np.all(u == u[0])                                           # no dependence on the state is left
    # tiny pre-activations: tanh(a) = a to the last bit's neighbourhood
    tiny = dict(pol, W1=1e-9 * pol["W1"], b1=1e-9 * pol["b1"])
    assert np.all(np.abs(_actions(p, tiny, x) - pm.action(tiny, x)) <= pm.action_bound(tiny, x)[0])
    # W2 = 0: the constant action max_action sin(b2), bitwise the same for every particle
    const = mc.network(name, 64, W2_zero=True)
    u = _actions(p, const, x)
    assert np.all(u == u[0]) and np.all(np.abs(u[0] - s["maxact"] * np.sin(const["b2"])) <= 8 * U53 * np.abs(s["maxact"]))
    lin = dict(const, squash=False)
    assert np.array_equal(_actions(p, lin, x), np.broadcast_to(lin["b2"], (65, U)))


# ------------------------------------------------------------------ 2. forward rollouts
def _marginal_bound(model, mu, v, eps, xn):
    """the step bound of tests/test_gpu_particles.py"""
    d = 1e-8 * np.asarray(model["variance"]).reshape(1, -1)
    return (1e-8 * np.abs(mu).max(axis=0, keepdims=True) + np.abs(eps) * (np.sqrt(v + d) - np.sqrt(np.maximum(v - d, 0.0)))
            + 4 * U53 * np.abs(xn))


@pytest.mark.parametrize("name,Hn,P,H", [("n300", 64, 129, 4), ("fitc", 65, 65, 2), ("syn5b", 1, 257, 4), ("syn65a", 256, 63, 1),
                                         ("syn65b", 5, 64, 0)])
def test_marginal_rollout_teacher_forced_on_the_devices_own_actions(name, Hn, P, H):
    p, s = _obj(name), mc.setup(name)
    pol = mc.network(name, Hn)
    x0 = mc.x0_of(name, P, 20 + P)
    for obs in (False, True):
        mean, cov, rew, parts, eps = _fwd(p, pol, "marginal", x0, H, seed=31 + H, obs=obs)[:5]
        assert parts.shape == (H + 1, P, s["E"]) and np.array_equal(parts[0], x0)
        if H == 0:
            continue
        X = parts[:-1].reshape(H * P, -1)
        u = _actions(p, pol, X)
        assert np.all(np.abs(u - pm.action(pol, X)) <= pm.action_bound(pol, X)[0])
        mu, v = pr.posterior(s["model"], np.concatenate([X, u], axis=1))
        if obs:
            v = v + np.asarray(s["model"]["noise"]).reshape(1, -1)
        e = eps.reshape(H * P, -1)
        xn = X + mu + np.sqrt(np.maximum(v, 0.0)) * e
        err, bound = np.abs(parts[1:].reshape(H * P, -1) - xn), _marginal_bound(s["model"], mu, v, e, xn)
        print("teacher-forced marginal %s Hn=%d P=%d H=%d obs=%d: largest |dx'| / bound = %.3g" % (name, Hn, P, H, obs, (err / bound).max()))
        assert np.all(err <= bound)
        r_np = np.array([pr.reward(s["terms"], parts[t]).mean() for t in range(H)])
        assert np.all(np.abs(rew - r_np) <= (4 * P * U53 + 1e-12) * max(np.abs(r_np).max(), 1e-300))


@pytest.mark.parametrize("name,Hn,P,H", [("n300", 64, 129, 4), ("syn5a", 2, 65, 2), ("syn65b", 63, 257, 1), ("w8", 256, 63, 4)])
def test_function_rollout_teacher_forced_on_the_devices_own_actions(name, Hn, P, H):
    p, s = _obj(name), mc.setup(name)
    pol = mc.network(name, Hn)
    x0 = mc.x0_of(name, P, 30 + P)
    out = _fwd(p, pol, "function", x0, H, seed=41, want_draws=True)
    parts, dr = out[3], out[7]
    X = parts[:-1].reshape(H * P, -1)
    u = _actions(p, pol, X)
    worst = 0.0
    for t in range(H):
        z = np.concatenate([parts[t], u[t * P:(t + 1) * P]], axis=1)
        f, m1, m2 = rf.f_of(s["model"], dr, dr["v"], z)
        xn = (np.asarray(parts[t], LD) + f).astype(np.float64)
        err, bound = np.abs(parts[t + 1] - xn), rf.step_bound(s["model"], mc.L, m1, m2, xn)
        worst = max(worst, float((err / bound).max()))
        assert np.all(err <= bound), (t, float((err / bound).max()))
    print("teacher-forced function %s Hn=%d P=%d H=%d: largest |dx'| / bound = %.3g" % (name, Hn, P, H, worst))


@pytest.mark.parametrize("name,Hn,P,H", [("fitc", 64, 65, 4), ("syn65b", 65, 129, 3)])
def test_conditioned_rollout_update_on_the_devices_own_actions(name, Hn, P, H):
    """the update check of tests/test_gpu_particle_cond.py: x' - x = mu + Lam z with the device's own mean at the visited points
    and its own path factor"""
    from pilco_amd import _lib
    p, s = _obj(name), mc.setup(name)
    pol = mc.network(name, Hn)
    E = s["E"]
    x0 = mc.x0_of(name, P, 40 + P)
    out = _fwd(p, pol, "conditioned", x0, H, seed=51)
    parts, eps, pf = out[3], out[4], out[7]
    X = parts[:-1].reshape(H * P, E)
    u = _actions(p, pol, X)
    assert np.all(np.abs(u - pm.action(pol, X)) <= pm.action_bound(pol, X)[0])
    xs = np.concatenate([X, u], axis=1)
    mu = np.asarray(_CTX.gp_predict_points(_lib.SLOT_DYNAMICS, xs, xs.shape[1], E)[0]).T.reshape(H, P, E)
    z, lam = np.asarray(eps, LD), np.asarray(pf, LD)
    dot = np.einsum("pets,spe->tpe", lam, z)
    mag = np.einsum("pets,spe->tpe", np.abs(lam), np.abs(z)) + np.abs(mu)
    err = np.abs((np.asarray(parts[1:], LD) - np.asarray(parts[:-1], LD)) - (np.asarray(mu, LD) + dot)).astype(np.float64)
    bound = (np.arange(H).reshape(H, 1, 1) + 4) * U53 * mag.astype(np.float64) + 2.0 ** -52 * np.abs(parts[1:])
    print("conditioned update %s Hn=%d P=%d H=%d: |dx'| / bound = %.3g" % (name, Hn, P, H, (err / bound).max()))
    assert np.all(err <= bound)


@pytest.mark.parametrize("dynamics,name", [("marginal", "n300"), ("marginal", "fitc"), ("function", "n300"), ("conditioned", "syn65b")])
def test_a_trajectory_has_the_same_bits_alone_in_a_batch_permuted_and_repeated(dynamics, name):
    p = _obj(name)
    pol = mc.network(name, 65)
    P, H = 129, 3
    x0 = mc.x0_of(name, P, 3)
    eps = np.random.RandomState(4).randn(H, P, x0.shape[1])
    kw = dict(eps=eps, seed=9, obs=dynamics != "conditioned")
    full = _fwd(p, pol, dynamics, x0, H, want_draws=dynamics == "function", **kw) if dynamics == "function" else _fwd(p, pol, dynamics, x0, H, **kw)
    dr = full[7] if dynamics == "function" else None
    again = _fwd(p, pol, dynamics, x0, H, draws=dr, **kw)
    assert all(np.array_equal(a, b) for a, b in zip(full[:5], again[:5]))
    for q in (0, 63, 64, 128):
        one_dr = None if dr is None else dict(dr, w=dr["w"][q:q + 1], xi=dr["xi"][q:q + 1])
        one = _fwd(p, pol, dynamics, x0[q:q + 1], H, draws=one_dr, eps=eps[:, q:q + 1], seed=9, obs=kw["obs"])
        assert np.array_equal(one[3][:, 0], full[3][:, q]), q
    perm = np.random.RandomState(5).permutation(P)
    perm_dr = None if dr is None else dict(dr, w=dr["w"][perm], xi=dr["xi"][perm])
    pmd = _fwd(p, pol, dynamics, x0[perm], H, draws=perm_dr, eps=eps[:, perm], seed=9, obs=kw["obs"])
    assert np.array_equal(pmd[3], full[3][:, perm])


def test_events_sample_trajectories_and_sample_risk_run():
    from pilco_amd import controllers
    from pilco_amd.safe import SafePILCO, SingleConstraint
    name = "syn65b"
    p, s = _net(_obj(name), mc.network(name, 8)), mc.setup(name)
    ev = [dict(clauses=[(0, None, 0.0)], complement=False)]
    for dynamics in ("marginal", "function", "conditioned"):
        res = p.sample_trajectories(s["m0"], s["S0"], 3, num_particles=129, seed=2, events=ev, dynamics=dynamics, return_particles=True)
        assert res.particles.shape == (4, 129, s["E"]) and np.all(np.isfinite(res.particles))
        want = (res.particles[:, :, 0] <= 0.0).sum(axis=1)
        assert np.array_equal(res.event_counts[:, 0], want)
    ctl = controllers.MlpController(s["E"], s["U"], num_hidden=8, max_action=s["maxact"], ctx=_CTX)
    sp = SafePILCO((s["cfg"]["X"], s["cfg"]["Y"]), controller=ctl, reward_mult=SingleConstraint(0, high=0.0, inside=True), horizon=3, ctx=_CTX)
    for i, mdl in enumerate(sp.mgpr.models):
        mdl.kernel.lengthscales.assign(s["cfg"]["lengthscales"][i])
        mdl.kernel.variance.assign(s["cfg"]["variance"][i])
        mdl.likelihood.variance.assign(s["cfg"]["noise"][i])
    for dynamics in ("marginal", "function", "conditioned"):
        risk = sp.sample_risk(s["m0"], s["S0"], 3, num_particles=65, seed=1, dynamics=dynamics)
        assert risk.risk_particles.shape == (3,) and np.all((risk.risk_particles >= 0) & (risk.risk_particles <= 1))
        assert risk.risk_moment_matched is None and risk.objective_moment_matched is None and "None" in repr(risk)
    _OBJ.pop(name, None)            # (the SafePILCO object took the dynamics slot: the module's object is rebuilt on next use)


# ------------------------------------------------------------------ 3. gradients
def _tolerance(b, sc, P, params):
    """the propagated bound plus the float64 floor of tests/test_gpu_particle_grad.py: a particle's chain within 4096 * 2^-53 of
    its absolute-sum scale, the sum over the particles within 4 P 2^-53 more"""
    return b + ((4 * P if params else 0) + 4096) * U53 * sc


def _matrices(s, pol, dynamics, parts, eps, dr, H, obs):
    out = []
    for t in range(H - 1):
        if dynamics == "marginal":
            out.append(pm.step_matrix_marginal(s["model"], pol, parts[t], eps[t], obs, bound=True))
        else:
            out.append(pm.step_matrix_fn(s["model"], pol, dr, dr["v"], parts[t], bound=True))
    return [a for a, _ in out], [d for _, d in out]


@pytest.mark.parametrize("dynamics,name,Hn,P,H,obs,squash", mc.CASES, ids=mc.CASE_IDS)
def test_gradient_against_the_restatement_on_the_devices_own_particles(dynamics, name, Hn, P, H, obs, squash):
    p, s = _obj(name), mc.setup(name)
    pol = mc.network(name, Hn, squash=squash)
    x0 = mc.x0_of(name, P, 100 + P)
    seed = 300 + P + H
    fwd = _fwd(p, pol, dynamics, x0, H, seed=seed, obs=obs, want_draws=True)
    rew, parts, eps, dr = fwd[2], fwd[3], fwd[4], fwd[7]
    # the draws fed back for even P, generated from the seed for odd P: the same stream either way
    J, steps, grads, dx0, _ = _grad(p, pol, dynamics, x0, H, draws=dr if P % 2 == 0 else None,
                                    eps=eps if (P % 2 == 0 and eps is not None) else None, seed=seed, obs=obs)
    assert np.array_equal(steps, rew)
    total = 0.0
    for r in rew:
        total += r
    assert J == total
    if H == 0:
        assert not any(np.any(g) for g in grads) and not np.any(dx0)
        return
    mats, dmats = _matrices(s, pol, dynamics, parts, eps, dr, H, obs)
    ref_g, ref_x = pm.reverse(pol, s["terms"], parts[:H], mats)
    (bg, bx), (sg, sx) = pm.reverse_bound(pol, s["terms"], parts[:H], mats, dmats)
    if H == 1:
        assert not any(np.any(g) for g in grads)
        assert np.all(np.abs(dx0 - reward_grad(s["terms"], x0)) <= 4096 * U53 * sx)
    worst = share = cond = tight = 0.0
    for got, ref, b, sc, params in zip(list(grads) + [dx0], list(ref_g) + [ref_x], list(bg) + [bx], list(sg) + [sx], [True] * 4 + [False]):
        got, ref, b, sc = (np.asarray(a, np.float64).reshape(np.shape(ref)) for a in (got, ref, b, sc))
        err = np.abs(got - ref)
        tol = _tolerance(b, sc, P, params)
        if H >= 2 and np.abs(ref).max() > 0:
            cond = max(cond, float((tol / np.maximum(sc, 1e-300)).max()))
            tight = max(tight, float(tol.max() / np.abs(ref).max()))
        worst = max(worst, float((err / np.maximum(tol, 1e-300)).max()))
        assert np.all(err <= tol), (dynamics, name, Hn, P, H, float((err / np.maximum(tol, 1e-300)).max()))
    print("teacher-forced gradient %s %s Hn=%d P=%d H=%d obs=%d squash=%d: largest error / tolerance = %.3g, tolerance / scale = "
          "%.3g, largest tolerance / largest entry = %.3g" % (dynamics, name, Hn, P, H, obs, squash, worst, cond, tight))
    assert cond <= 1e-6 and tight <= 1e-6


@pytest.mark.parametrize("dynamics", ["marginal", "function"])
def test_gradient_bits_alone_batched_permuted_grouped_and_fed_back(dynamics, monkeypatch):
    name, P, H = "n300", 257, 3
    p = _obj(name)
    pol = mc.network(name, 65)
    x0 = mc.x0_of(name, P, 6)
    eps = np.random.RandomState(7).randn(H, P, x0.shape[1])
    kw = dict(eps=eps, seed=12, obs=True)
    full = _grad(p, pol, dynamics, x0, H, want_draws=True, **kw)
    dr = full[4]
    fwd = _fwd(p, pol, dynamics, x0, H, draws=dr, **kw)
    assert np.array_equal(full[1], fwd[2])                              # reward_steps: the bits of the forward entry point
    assert _same(full, _grad(p, pol, dynamics, x0, H, draws=dr, **kw))   # the draws fed back reproduce everything
    for q in (0, 64, 128, 256):
        one_dr = None if dr is None else dict(dr, w=dr["w"][q:q + 1], xi=dr["xi"][q:q + 1])
        one = _grad(p, pol, dynamics, x0[q:q + 1], H, draws=one_dr, eps=eps[:, q:q + 1], seed=12, obs=True)
        assert np.array_equal(one[3][0], full[3][q]), q
    perm = np.random.RandomState(8).permutation(P)
    perm_dr = None if dr is None else dict(dr, w=dr["w"][perm], xi=dr["xi"][perm])
    pmd = _grad(p, pol, dynamics, x0[perm], H, draws=perm_dr, eps=eps[:, perm], seed=12, obs=True)
    assert np.array_equal(pmd[3], full[3][perm])
    # groups of 128 particles: (H - 1) E D doubles per particle
    E, D = x0.shape[1], x0.shape[1] + mc.setup(name)["U"]
    monkeypatch.setenv(BUDGET, str(128 * (H - 1) * E * D))
    assert _same(full, _grad(p, pol, dynamics, x0, H, draws=dr, **kw))
    monkeypatch.delenv(BUDGET)


def test_constant_action_gives_exact_zeros_in_the_first_layer():
    name = "syn65b"
    p = _obj(name)
    pol = mc.network(name, 64, W2_zero=True)
    x0 = mc.x0_of(name, 129, 9)
    for dynamics in ("marginal", "function"):
        J, steps, (dW1, db1, dW2, db2), dx0, _ = _grad(p, pol, dynamics, x0, 4, seed=3)
        assert not np.any(dW1) and not np.any(db1) and np.any(dW2) and np.any(db2)
    sat = dict(mc.network(name, 64), W1=np.zeros((64, 3)), b1=np.full(64, 40.0))   # h = 1 exactly: its derivative is exactly 0
    J, steps, (dW1, db1, dW2, db2), dx0, _ = _grad(p, sat, "function", x0, 4, seed=3)
    assert not np.any(dW1) and not np.any(db1) and np.any(dW2)
    assert np.array_equal(dW2, np.repeat(db2.reshape(-1, 1), 64, axis=1))           # d W2_kj = sum ds_k * 1


# ------------------------------------------------------------------ 4. refusals
def _raw_grad(lib, h, which, spec_struct, terms, x0, H, outs, draws=None):
    dp = C.POINTER(C.c_double)
    ptr = lambda a: None if a is None else a.ctypes.data_as(dp)   # noqa: E731
    P = x0.shape[0]
    head = (h, C.byref(spec_struct), terms[0], terms[1], ptr(x0), P, H, None, C.c_ulonglong(1), 0)
    if which.startswith("pilco_rollout_particles_fn"):
        head = head + (C.byref(draws), None)
    return getattr(lib, which)(*head, *[ptr(a) for a in outs])


def test_refusals_leave_the_outputs_untouched_and_a_valid_call_follows():
    from pilco_amd import _lib
    name = "syn65b"
    s = mc.setup(name)
    E, U = s["E"], s["U"]
    pol = mc.network(name, 8)
    x0 = mc.x0_of(name, 5, 1)
    cx = _lib.Context(device=0)
    try:
        cfg = s["cfg"]
        cx.gp_set_data(0, cfg["X"], cfg["Y"])
        cx.gp_set_hyp(0, cfg["lengthscales"], cfg["variance"], cfg["noise"])
        cx.gp_factorize(0)
        spec = dict(kind=_lib.POLICY_MLP, state_dim=E, control_dim=U, max_action=s["maxact"], squash=True)
        terms = [dict(kind=_lib.REWARD_LINEAR, coef=1.0, W=np.ones(E))]

        def refused(code, call):
            with pytest.raises(_lib.PilcoError) as ei:
                call()
            assert ei.value.code == code, str(ei.value)

        # kind 3 with no network set
        refused(E_STATE, lambda: cx.rollout_particles(spec, terms, x0, 2))
        refused(E_STATE, lambda: cx.particle_actions(spec, x0))
        refused(E_STATE, lambda: cx.rollout_particles_grad_mlp(spec, terms, x0, 2))
        # hidden outside 1..256, null parameters
        dp = C.POINTER(C.c_double)
        W1, b1, W2, b2 = (np.ascontiguousarray(pol[k], dtype=np.float64) for k in ("W1", "b1", "W2", "b2"))
        ptr = lambda a: a.ctypes.data_as(dp)   # noqa: E731
        for hidden in (0, 257, -1):
            assert cx.lib.pilco_set_policy_mlp(cx.h, E, U, hidden, ptr(W1), ptr(b1), ptr(W2), ptr(b2)) == E_SHAPE
        for k in range(4):
            args = [ptr(W1), ptr(b1), ptr(W2), ptr(b2)]
            args[k] = None
            assert cx.lib.pilco_set_policy_mlp(cx.h, E, U, 8, *args) == E_SHAPE
        refused(E_STATE, lambda: cx.rollout_particles(spec, terms, x0, 2))          # the refused calls set nothing
        # a network of other dimensions than the dynamics slot's
        cx.set_policy_mlp(np.zeros((8, E + 1)), b1, W2, b2)
        refused(E_SHAPE, lambda: cx.rollout_particles(spec, terms, x0, 2))
        cx.set_policy_mlp(W1, b1, np.zeros((U + 1, 8)), np.zeros(U + 1))
        refused(E_SHAPE, lambda: cx.rollout_particles_fn(spec, terms, x0, 2, num_features=8))
        cx.set_policy_mlp(W1, b1, W2, b2)
        # the policy kind against the entry point
        refused(E_SHAPE, lambda: cx.rollout_particles_grad(spec, terms, x0, 2))
        refused(E_SHAPE, lambda: cx.rollout_particles_fn_grad(spec, terms, x0, 2, num_features=8))
        refused(E_SHAPE, lambda: cx.rollout_particles_grad_rbf(spec, terms, x0, 2, np.zeros((3, E)), np.zeros((3, U)), np.ones((U, E)), np.ones(U)))
        lin = dict(kind=_lib.POLICY_LINEAR, state_dim=E, control_dim=U, W=np.zeros((U, E)), b=np.zeros(U), max_action=s["maxact"])
        refused(E_SHAPE, lambda: cx.rollout_particles_grad_mlp(lin, terms, x0, 2))
        refused(E_SHAPE, lambda: cx.rollout_particles_fn_grad_mlp(lin, terms, x0, 2, num_features=8))
        # null gradient pointers: nothing is written
        ps, keep = cx._policy(spec)
        rw = cx._rewards(terms, E)
        draws = _lib.FunctionDraws()
        draws.L = 8
        for which in ("pilco_rollout_particles_grad_mlp", "pilco_rollout_particles_fn_grad_mlp"):
            for k in range(2, 6):
                outs = [np.full(1, 7.0), np.full(2, 7.0), np.full((8, E), 7.0), np.full(8, 7.0), np.full((U, 8), 7.0), np.full(U, 7.0),
                        np.full((5, E), 7.0)]
                kept = list(outs)
                outs[k] = None
                assert _raw_grad(cx.lib, cx.h, which, ps, (rw[0], 1), x0, 2, outs, draws) == E_SHAPE, (which, k)
                assert all(np.all(a == 7.0) for a in kept)
        # the moment-matching entry points refuse kind 3
        m0, S0 = np.zeros(E), 0.1 * np.eye(E)
        refused(E_SHAPE, lambda: cx.rollout(spec, terms, m0, S0, 2))
        refused(E_SHAPE, lambda: cx.propagate(spec, m0, S0))
        refused(E_SHAPE, lambda: cx.policy_action(spec, m0, S0))
        refused(E_SHAPE, lambda: cx.rollout_grad(spec, terms, m0, S0, 2))
        # a valid call after them is correct
        u = cx.particle_actions(spec, x0)
        assert np.all(np.abs(u - pm.action(pol, x0)) <= pm.action_bound(pol, x0)[0])
        out = cx.rollout_particles_grad_mlp(spec, terms, x0, 2, seed=4, want_dx0=True)
        assert np.array_equal(out[1], cx.rollout_particles(spec, terms, x0, 2, seed=4)[2]) and np.any(out[4])
    finally:
        cx.close()


# ------------------------------------------------------------------ 5. end to end
@pytest.mark.parametrize("dynamics", ["function", "marginal"])
def test_optimize_policy_on_particles_with_a_network(dynamics):
    from pilco_amd import controllers
    name = "syn65b"
    s = mc.setup(name)
    p = _obj(name)
    np.random.seed(5)
    p.controller = controllers.MlpController(s["E"], s["U"], num_hidden=8, max_action=s["maxact"], ctx=_CTX)
    p.horizon = 4
    p.m_init, p.S_init = s["m0"], s["S0"]
    opts = dict(num_particles=129, seed=3, dynamics=dynamics, num_features=mc.L)
    x0 = p._initial_particles(p.m_init, p.S_init, 129, 3)
    kw = dict(x0=x0, seed=3, dynamics=dynamics, num_features=mc.L)
    start, g0 = p.particle_value_and_gradient(**kw)
    assert [g.shape for g in g0] == [(8, s["E"]), (8,), (s["U"], 8), (1, s["U"])]
    best = p.optimize_policy(maxiter=5, verbose=False, objective="particles", particle_options=opts)
    fresh = p.particle_value_and_gradient(**kw)[0]
    print("optimize_policy(particles, %s) with an MlpController: %.6g -> %.6g" % (dynamics, start, best))
    assert best >= start and best == fresh
    with pytest.raises(NotImplementedError):
        p.optimize_policy(maxiter=1, verbose=False)
    lin = p.linearize(s["m0"][0])
    assert lin.K.shape == (s["U"], s["E"]) and np.all(np.isfinite(lin.A_cl))
    _OBJ.pop(name, None)            # (the controller was replaced: the module's object is rebuilt on next use)
