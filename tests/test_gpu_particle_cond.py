"""Particle rollouts conditioned on their own path on the MI355X: pilco_rollout_particles_cond (csrc/particles_cond.hip),
Context.rollout_particles_cond and PILCO.sample_trajectories(dynamics="conditioned"), held to the NumPy restatement
(tests/helpers/particle_cond_restatement.py; tests/test_particle_cond_cpu.py pins it without a device).  Every test prints
its figures before it asserts (run with -s; docs/particle_conditioned.md records them)."""
import os

import numpy as np
import pytest

from helpers import particle_cond_restatement as rq
from helpers import particle_events_restatement as er
from helpers import particles_restatement as pr
from helpers import predict_cov_cases as cc
from pilco_amd import synthetic

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U53 = 2.0 ** -53
LD = np.longdouble
E_SHAPE, E_NOT_PD = 1, 2
JITTER = 1e-8
_CTX = None
_SETUPS = {}
_OPS = {}
_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def own_ctx():
    from pilco_amd import _lib
    global _CTX
    _CTX = _lib.Context(device=0)
    yield _CTX
    for k, v in sorted(_WORST.items()):
        print("largest figure, %s: %.3g" % (k, v))
    _SETUPS.clear()
    _OPS.clear()
    _CTX.close()


def _g(name):
    return np.load(os.path.join(GOLDEN, name))


def _setup(name):
    """-> (PILCO on this module's context, restatement model, restatement policy, m0, S0)."""
    if name in _SETUPS:
        return _SETUPS[name]
    from pilco_amd import controllers
    from pilco_amd.models import PILCO
    policy = ctl = Z = None
    if name in ("predictions", "sparse"):     # tests/golden/(sparse_)predictions.npz: state 2 + 1 control, linear policy
        g = _g("predictions.npz" if name == "predictions" else "sparse_predictions.npz")
        cfg = {k: g[k] for k in ("X", "Y", "lengthscales", "variance", "noise")}
        Z = g["Z"] if name == "sparse" else None
        W, b, maxact = np.array([[0.7, -0.4]]), np.array([[0.15]]), 1.3
        ctl = controllers.LinearController(2, 1, max_action=maxact, ctx=_CTX)
        ctl.W.assign(W)
        ctl.b.assign(b)
        policy = dict(kind="linear", W=W, b=b, max_action=maxact)
        m0 = cfg["X"][:1, :2]
    elif name == "rbf":                # N = 300, state 3 (odd: the Box-Muller pairs) + 2 controls, an RbfController
        cfg = synthetic.config_c2(N=300, D=5, E=3, control_dim=2, seed=21)
        g = _g("rbf_controller.npz")
        ctl = controllers.RbfController(3, 2, g["X"].shape[0], max_action=2.0, ctx=_CTX)
        ctl.set_data((g["X"], g["Y"]))
        for i, mdl in enumerate(ctl.models):
            mdl.kernel.lengthscales.assign(g["lengthscales"][i])
        policy = dict(kind="rbf", X=g["X"], Y=g["Y"], lengthscales=g["lengthscales"], noise=np.full(2, 1e-4), max_action=2.0)
        m0 = cfg["m0"]
    elif name.startswith("syn"):       # synthetic, N in {1, 63, 64, 65, 130}, state 3, no policy
        cfg = synthetic.config_c2(N=int(name[3:]), D=3, E=3, seed=33)
        m0 = cfg["m0"]
    else:
        raise KeyError(name)
    E = cfg["Y"].shape[1]
    p = PILCO((cfg["X"], cfg["Y"]), num_induced_points=None if Z is None else Z.shape[0], controller=ctl, ctx=_CTX)
    for i, mdl in enumerate(p.mgpr.models):
        mdl.kernel.lengthscales.assign(cfg["lengthscales"][i])
        mdl.kernel.variance.assign(cfg["variance"][i])
        mdl.likelihood.variance.assign(cfg["noise"][i])
        if Z is not None:
            mdl.inducing_variable.Z.assign(Z)
    model = dict(X=np.asarray(cfg["X"], np.float64), Y=np.asarray(cfg["Y"], np.float64), lengthscales=np.asarray(cfg["lengthscales"]),
                 variance=np.asarray(cfg["variance"]), noise=np.asarray(cfg["noise"]), Z=Z)
    _SETUPS[name] = (p, model, policy, m0, 0.05 * np.eye(E))
    return _SETUPS[name]


def _ops(name):
    if name not in _OPS:
        _OPS[name] = rq.operators_ld(_setup(name)[1])
    return _OPS[name]


SETUPS = ["predictions", "rbf", "syn1", "syn63", "syn64", "syn65", "syn130", "sparse"]


def _note(key, v):
    _WORST[key] = max(_WORST.get(key, 0.0), float(v))


def _visited(p, parts):
    """the points [x, u] the device visited: particles (H + 1, P, E) -> (H, P, D), the actions from the device's own kernel"""
    H, P, E = parts.shape[0] - 1, parts.shape[1], parts.shape[2]
    spec = p._policy_spec()
    if spec["control_dim"] == 0:
        return parts[:H].copy()
    u = p.ctx.particle_actions(spec, parts[:H].reshape(H * P, E)).reshape(H, P, -1)
    return np.concatenate([parts[:H], u], axis=2)


def _device_mean(p, xs):
    """pilco_gp_predict_points at the visited points: (H, P, E)"""
    from pilco_amd import _lib
    H, P, D = xs.shape
    E = p.state_dim
    mean, _ = p.ctx.gp_predict_points(_lib.SLOT_DYNAMICS, xs.reshape(H * P, D), D, E)
    return np.asarray(mean).T.reshape(H, P, E)


def _check_path(name, res, H, P, obs, jitter=JITTER, tag=""):
    """c_ts, the factor and the update of every step of a run, against the restatement on the device's own visited points."""
    p, model, policy, m0, S0 = _setup(name)
    E = p.state_dim
    parts, eps, pc, pf = res.particles, res.eps, res.path_cov, res.path_factor
    assert parts.shape == (H + 1, P, E) and eps.shape == (H, P, E) and pc.shape == (P, E, H, H) and pf.shape == (P, E, H, H)
    assert (res.eps_obs is None) == (not obs)
    if H == 0:
        return
    iu = np.triu_indices(H, 1)
    assert not pc[..., iu[0], iu[1]].any() and not pf[..., iu[0], iu[1]].any()      # the upper triangles are zero
    xs = _visited(p, parts)
    # c_ts: a few particles against the np.longdouble truth, in its units; the cap from the two float64 restatements
    sel = sorted({0, 1 % P, 62 % P, 63 % P, 64 % P, P - 1})
    truth, unit = rq.path_cov_truth(model, _ops(name), xs[:, sel])
    ka = rq.k_of(rq.path_cov_f64(model, xs[:, sel], "a"), truth, unit)
    kb = rq.k_of(rq.path_cov_f64(model, xs[:, sel], "b"), truth, unit)
    cap = max(cc.CAP_FLOOR, cc.CAP_FACTOR * max(ka, kb))
    kd = rq.k_of(pc[sel], truth, unit)
    # the factor: backward error on the device's own matrix against NumPy's Cholesky of the same matrix
    je = jitter * np.asarray(model["variance"]).reshape(1, E, 1, 1)
    A = np.tril(pc) + np.swapaxes(np.tril(pc, -1), -1, -2) + je * np.eye(H)
    be_dev = rq.backward_error(pf, A)
    be_np = rq.backward_error(np.linalg.cholesky(A), A)
    # the update
    mu = _device_mean(p, xs)
    z = np.asarray(eps, LD)
    lam = np.asarray(pf, LD)
    dot = np.einsum("pets,spe->tpe", lam, z)
    mag = np.einsum("pets,spe->tpe", np.abs(lam), np.abs(z)) + np.abs(mu)
    if obs:
        sn = np.sqrt(np.asarray(model["noise"], np.float64)).reshape(1, 1, E)
        dot = dot + np.asarray(sn * res.eps_obs, LD)
        mag = mag + np.abs(sn * res.eps_obs)
    err = np.abs((np.asarray(parts[1:], LD) - np.asarray(parts[:-1], LD)) - (np.asarray(mu, LD) + dot)).astype(np.float64)
    steps = np.arange(H).reshape(H, 1, 1)
    bound = (steps + 4) * U53 * mag.astype(np.float64) + 2.0 ** -52 * np.abs(parts[1:])
    ru = float((err / bound).max())
    print("%s%s P=%d H=%d obs=%d: c_ts K = %.3g (K_ref a %.3g, b %.3g, cap %.3g); factor backward error %.3g (NumPy %.3g); "
          "update |dx'| / bound = %.3g" % (name, tag, P, H, obs, kd, ka, kb, cap, be_dev, be_np, ru))
    _note("c_ts K, " + name, kd)
    _note("factor backward error / NumPy's, " + name, be_dev / be_np if be_np > 0 else 0.0)
    _note("update, " + name, ru)
    assert kd <= cap
    assert be_dev <= 8 * be_np
    assert np.all(err <= bound)


def _check_stats(res, P, E, H, terms=None):
    parts = res.particles
    xmax = np.abs(parts).max()
    mean_np = parts.mean(axis=1)
    c = parts - mean_np[:, None, :]
    cov_np = np.einsum("tpa,tpb->tab", c, c) / P
    assert res.mean.shape == (H + 1, E) and res.cov.shape == (H + 1, E, E) and res.reward_steps.shape == (H,)
    assert np.abs(res.mean - mean_np).max() <= 4 * P * U53 * xmax and np.abs(res.cov - cov_np).max() <= 4 * P * U53 * xmax ** 2
    if P == 1:
        assert not res.cov.any()
    if H > 0:
        terms = terms or [dict(kind="exponential", W=np.eye(E), t=None, coef=1.0)]   # PILCO's default reward
        r_np = np.array([pr.reward(terms, parts[t]) for t in range(H)])
        assert np.abs(res.reward_steps - r_np.mean(axis=1)).max() <= (4 * P * U53 + 1e-12) * max(np.abs(r_np).max(), 1e-300)
        assert res.reward[0, 0] == res.reward_steps.sum()


# ------------------------------------------------------------------ the grid: every setup, P and H
CASES = [(n, P, H) for n in SETUPS for P in (1, 63, 65, 129) for H in (0, 1, 2, 6)]


@pytest.mark.parametrize("name,P,H", CASES, ids=["%s-P%d-H%d" % c for c in CASES])
def test_path_covariance_factor_update_and_statistics(name, P, H):
    p, model, policy, m0, S0 = _setup(name)
    obs = P in (63, 129)
    seed = 7 + P + H
    res = p.sample_trajectories(m0, S0, H, num_particles=P, seed=seed, return_particles=True, dynamics="conditioned",
                                observation_noise=obs)
    assert np.array_equal(res.particles[0], p._initial_particles(m0, S0, P, seed))
    _check_path(name, res, H, P, obs)
    _check_stats(res, P, p.state_dim, H)
    if H > 0:    # the generated draws are the streams: domain 0 for the steps, domain 6 for the observation noise
        z, r = pr.normals(seed, H, P, p.state_dim, particles=[0, P - 1])
        for q in (0, P - 1):
            assert np.all(np.abs(res.eps[:, q] - z[:, q]) <= 16 * U53 * np.maximum(1.0, r[:, q]))
        if obs:
            zo, ro = rq.obs_normals(seed, H, P, p.state_dim)
            assert np.all(np.abs(res.eps_obs - zo) <= 16 * U53 * np.maximum(1.0, ro))


def _tiny(N=5, ls_scale=1.0, zero_y=False):
    """synthetic N = 5, E = 1, no policy, on its own PILCO"""
    from pilco_amd.models import PILCO
    rs = np.random.RandomState(17)
    X = rs.uniform(-1.0, 1.0, (N, 1))
    Y = np.zeros((N, 1)) if zero_y else 0.3 * np.sin(2.0 * X) + 0.01 * rs.randn(N, 1)
    p = PILCO((X, Y), ctx=_CTX)
    spread = float(X.max() - X.min())
    ls, var, noise = np.array([[ls_scale * spread]]), np.array([0.8]), np.array([1e-2])
    p.mgpr.models[0].kernel.lengthscales.assign(ls[0])
    p.mgpr.models[0].kernel.variance.assign(var[0])
    p.mgpr.models[0].likelihood.variance.assign(noise[0])
    return p, dict(X=X, Y=Y, lengthscales=ls, variance=var, noise=noise, Z=None)


@pytest.mark.parametrize("H", [65, 128])
def test_long_paths_cross_the_64_row_edge_of_the_factor(H):
    p, model = _tiny()
    name = "tiny%d" % H
    _SETUPS[name] = (p, model, None, None, None)
    x0 = np.array([[0.1], [-0.4], [0.7]])
    res = p.sample_trajectories(None, None, H, x0=x0, seed=3, return_particles=True, dynamics="conditioned")
    _check_path(name, res, H, 3, False)
    _check_stats(res, 3, 1, H)
    del _SETUPS[name], _OPS[name]


# ------------------------------------------------------------------ the first step against the marginal rollout
@pytest.mark.parametrize("name", ["predictions", "rbf", "syn65", "sparse"])
def test_first_step_is_the_marginal_draw_up_to_the_jitter(name):
    """Step 0 of the conditioned rollout is mu + sqrt(c_00 + j) z, the marginal rollout's mu + sqrt(v) z on the same z: c_00
    and v are the same variance summed in two orders, each within K_v / 2 = 4 units 2^-53 (sf2 + g . g) of the truth (the floor
    of the project's caps), so |dx_1| <= |z| (sqrt(v_hi + j) - sqrt(v_lo)) + 4 * 2^-53 (|x_1| + |mu| + sd |z|),
    v_hi / v_lo = truth +- 4 units (v_lo clamped at 0)."""
    p, model, policy, m0, S0 = _setup(name)
    P, seed = 129, 41
    a = p.sample_trajectories(m0, S0, 1, num_particles=P, seed=seed, return_particles=True, dynamics="conditioned")
    b = p.sample_trajectories(m0, S0, 1, num_particles=P, seed=seed, return_particles=True)
    assert np.array_equal(a.eps, b.eps) and np.array_equal(a.particles[0], b.particles[0])
    xs = _visited(p, a.particles)
    truth, unit = rq.path_cov_truth(model, _ops(name), xs)
    v, un = truth[:, :, 0, 0], unit[:, :, 0, 0]           # (P, E)
    j = JITTER * np.asarray(model["variance"]).reshape(1, -1)
    z = np.abs(a.eps[0])
    mu = np.abs(_device_mean(p, xs)[0])
    hi, lo = np.sqrt(v + 4 * un + j), np.sqrt(np.maximum(v - 4 * un, 0.0))
    bound = z * (hi - lo) + 4 * U53 * (np.abs(a.particles[1]) + mu + hi * z)
    err = np.abs(a.particles[1] - b.particles[1])
    print("%s: first step against the marginal rollout: largest |dx_1| = %.3g, largest |dx_1| / bound = %.3g" %
          (name, err.max(), (err / bound).max()))
    _note("first step against marginal, " + name, (err / bound).max())
    assert np.all(err <= bound)


# ------------------------------------------------------------------ bits
FIELDS = ("mean", "cov", "reward_steps", "particles", "eps", "path_cov", "path_factor", "reward")


def _same(a, b, fields=FIELDS):
    return all(np.array_equal(getattr(a, f), getattr(b, f)) for f in fields)


@pytest.mark.parametrize("name,obs", [("predictions", True), ("rbf", False), ("sparse", True)])
def test_a_trajectory_has_the_same_bits_alone_in_a_batch_permuted_repeated_and_fed_back(name, obs):
    p, model, policy, m0, S0 = _setup(name)
    P, H, seed = 129, 6, 19
    x0 = p._initial_particles(m0, S0, P, seed)
    kw = dict(return_particles=True, dynamics="conditioned", observation_noise=obs)
    full = p.sample_trajectories(m0, S0, H, x0=x0, seed=seed, **kw)
    again = p.sample_trajectories(m0, S0, H, x0=x0, seed=seed, **kw)
    assert _same(full, again) and (not obs or np.array_equal(full.eps_obs, again.eps_obs))
    fed = p.sample_trajectories(m0, S0, H, x0=x0, seed=seed + 1, eps=full.eps, eps_obs=full.eps_obs if obs else None, **kw)
    assert _same(full, fed) and (not obs or np.array_equal(full.eps_obs, fed.eps_obs))
    for q in (0, 64, 128):                                  # alone (P = 1), on its own draws
        one = p.sample_trajectories(m0, S0, H, x0=x0[q:q + 1], seed=0, eps=full.eps[:, q:q + 1],
                                    eps_obs=full.eps_obs[:, q:q + 1] if obs else None, **kw)
        assert np.array_equal(one.particles[:, 0], full.particles[:, q])
        assert np.array_equal(one.path_cov[0], full.path_cov[q]) and np.array_equal(one.path_factor[0], full.path_factor[q])
    perm = np.random.RandomState(2).permutation(P)
    pm = p.sample_trajectories(m0, S0, H, x0=x0[perm], seed=0, eps=full.eps[:, perm], eps_obs=full.eps_obs[:, perm] if obs else None, **kw)
    assert np.array_equal(pm.particles, full.particles[:, perm]) and np.array_equal(pm.path_factor, full.path_factor[perm])
    assert np.array_equal(pm.path_cov, full.path_cov[perm])
    if not obs:   # without observation noise eps_obs is never read: two different ones give identical bits
        rs = np.random.RandomState(4)
        o1 = p.ctx.rollout_particles_cond(p._policy_spec(), p._reward_terms(), x0, H, eps=full.eps, want_particles=True, want_path=True,
                                          eps_obs=rs.randn(H, P, p.state_dim))
        o2 = p.ctx.rollout_particles_cond(p._policy_spec(), p._reward_terms(), x0, H, eps=full.eps, want_particles=True, want_path=True,
                                          eps_obs=rs.randn(H, P, p.state_dim))
        assert all(np.array_equal(u, v) for u, v in zip(o1[:5] + o1[8:], o2[:5] + o2[8:])) and o1[7] is None
        assert np.array_equal(o1[3], full.particles)


@pytest.mark.parametrize("name", ["predictions", "sparse"])
def test_groups_change_no_bit(name, monkeypatch):
    p, model, policy, m0, S0 = _setup(name)
    P, H, seed = 129, 6, 23
    E, D = p.state_dim, model["X"].shape[1]
    nops = 2 if model["Z"] is not None else 1
    npad = -(-len(model["Z"] if model["Z"] is not None else model["X"]) // 64) * 64
    ev = [dict(clauses=[(0, None, float(m0[0, 0]))], complement=False)]
    kw = dict(return_particles=True, dynamics="conditioned", observation_noise=True, events=ev)
    whole = p.sample_trajectories(m0, S0, H, num_particles=P, seed=seed, **kw)
    budget = 64 * rq.per_particle(H, nops, E, D, npad, True) + 7
    G, ng, _, _, _ = rq.plan(P, H, nops, E, D, npad, True, budget, rq.chunk_cap(E, npad))
    assert (G, ng) == (64, 3)
    monkeypatch.setenv("PILCO_PARTICLE_COND_BUDGET", str(budget))
    grouped = p.sample_trajectories(m0, S0, H, num_particles=P, seed=seed, **kw)
    monkeypatch.setenv("PILCO_PARTICLE_COND_BUDGET", str(64 * rq.per_particle(H, nops, E, D, npad, True) - 1))
    from pilco_amd import _lib
    with pytest.raises(_lib.PilcoError, match="largest H that fits is %d" % (H - 1)) as ei:
        p.sample_trajectories(m0, S0, H, num_particles=P, seed=seed, **kw)
    assert ei.value.code == E_SHAPE
    monkeypatch.delenv("PILCO_PARTICLE_COND_BUDGET")
    print("%s: %d groups of %d against the ungrouped call: every output bitwise" % (name, ng, G))
    assert _same(whole, grouped) and np.array_equal(whole.eps_obs, grouped.eps_obs)
    assert np.array_equal(whole.event_counts, grouped.event_counts) and np.array_equal(whole.first_hit, grouped.first_hit)


def test_marginal_and_function_rollouts_keep_their_bits_around_a_conditioned_call():
    p, model, policy, m0, S0 = _setup("predictions")
    kw = dict(num_particles=129, seed=5, return_particles=True)
    m1 = p.sample_trajectories(m0, S0, 6, **kw)
    f1 = p.sample_trajectories(m0, S0, 6, dynamics="function", num_features=64, **kw)
    p.sample_trajectories(m0, S0, 6, dynamics="conditioned", observation_noise=True, **kw)
    m2 = p.sample_trajectories(m0, S0, 6, **kw)
    f2 = p.sample_trajectories(m0, S0, 6, dynamics="function", num_features=64, **kw)
    base = ("mean", "cov", "reward_steps", "particles", "eps")
    assert _same(m1, m2, base) and _same(f1, f2, base[:4])
    assert all(np.array_equal(f1.function_draws[k], f2.function_draws[k]) for k in f1.function_draws)


# ------------------------------------------------------------------ the point of the feature
def test_two_visits_of_one_region_are_correlated_as_the_posterior_says():
    """Lengthscale 1e3 x the data spread, all particles at one x0, H = 2: the two increments are almost the same function
    value.  Conditioned: their empirical correlation over the particles is the exact rho of the path covariance within
    5 (1 - rho^2) / sqrt(P), the standard error of a sample correlation; marginal, same eps: within 5 / sqrt(P) of 0."""
    p, model = _tiny(ls_scale=1e3)
    P, H = 4096, 2
    x0 = np.full((P, 1), 0.2)
    c = p.sample_trajectories(None, None, H, x0=x0, seed=9, return_particles=True, dynamics="conditioned")
    m = p.sample_trajectories(None, None, H, x0=x0, eps=c.eps, return_particles=True)
    inc_c, inc_m = np.diff(c.particles[:, :, 0], axis=0), np.diff(m.particles[:, :, 0], axis=0)
    # the exact rho: every particle has its own second point; the restatement's path covariance at each
    ops = rq.operators_ld(model)
    truth, _ = rq.path_cov_truth(model, ops, c.particles[:H])
    C = truth[:, 0] + JITTER * model["variance"][0] * np.eye(H)
    rho = float(np.mean(C[:, 1, 0] / np.sqrt(C[:, 0, 0] * C[:, 1, 1])))
    # the means of the two increments differ from particle to particle by the posterior mean at the visited points: remove them
    mu = _device_mean(p, c.particles[:H])[:, :, 0]
    rc_ = float(np.corrcoef(inc_c[0] - mu[0], inc_c[1] - mu[1])[0, 1])
    mum = _device_mean(p, m.particles[:H])[:, :, 0]
    rm_ = float(np.corrcoef(inc_m[0] - mum[0], inc_m[1] - mum[1])[0, 1])
    print("correlation of the two increments over %d particles: conditioned %.6f (exact rho %.6f, bound %.3g), marginal %.4f (bound %.3g)"
          % (P, rc_, rho, 5 * (1 - rho ** 2) / np.sqrt(P), rm_, 5 / np.sqrt(P)))
    assert abs(rc_ - rho) <= 5 * (1 - rho ** 2) / np.sqrt(P)
    assert abs(rm_) <= 5 / np.sqrt(P)


# ------------------------------------------------------------------ events, rewards, risk
def test_events_rewards_and_host_event_terms():
    from pilco_amd import rewards
    p, model, policy, m0, S0 = _setup("predictions")
    P, H = 129, 6
    evs = [dict(clauses=[(0, None, float(m0[0, 0]))], complement=False), dict(clauses=[(0, -0.5, 0.5), (1, -0.5, 0.5)], complement=True)]
    res = p.sample_trajectories(m0, S0, H, num_particles=P, seed=13, return_particles=True, dynamics="conditioned", events=evs)
    assert np.array_equal(res.event_counts, er.counts(evs, res.particles)) and np.array_equal(res.first_hit, er.first_hit(evs, res.particles))
    assert np.array_equal(res.event_prob, res.event_counts / float(P))
    print("events: counts %s" % res.event_counts.T.tolist())
    old = p.reward
    try:
        t = np.array([[0.3, -0.2]])
        Wr = np.array([[1.5, 0.2], [0.2, 0.7]])
        p.reward = rewards.CombinedRewards(2, [rewards.ExponentialReward(2, W=Wr, t=t), rewards.LinearReward(2, np.array([0.4, -1.0]))],
                                           coefs=[0.7, -0.3])
        r2 = p.sample_trajectories(m0, S0, H, num_particles=P, seed=13, return_particles=True, dynamics="conditioned")
        assert np.array_equal(r2.particles, res.particles)
        terms = [dict(kind="exponential", W=Wr, t=t, coef=0.7), dict(kind="linear", W=np.array([0.4, -1.0]), coef=-0.3)]
        _check_stats(r2, P, 2, H, terms)
    finally:
        p.reward = old


def test_sample_risk_passes_conditioned_through():
    from pilco_amd import rewards
    from pilco_amd.safe import SafePILCO, SingleConstraint
    p, model, policy, m0, S0 = _setup("predictions")
    n, P, mu = 4, 129, 0.7
    con = SingleConstraint(0, high=float(m0[0, 0]), inside=True)
    sp = SafePILCO((model["X"], model["Y"]), controller=p.controller, reward_add=rewards.ExponentialReward(2), reward_mult=con, mu=mu,
                   horizon=n, ctx=_CTX)
    for i, mdl in enumerate(sp.mgpr.models):
        mdl.kernel.lengthscales.assign(model["lengthscales"][i])
        mdl.kernel.variance.assign(model["variance"][i])
        mdl.likelihood.variance.assign(model["noise"][i])
    rk = sp.sample_risk(m0, S0, n, num_particles=P, seed=3, dynamics="conditioned", return_particles=True)
    res = rk.trajectories
    spec = [con.event_spec()]
    assert res.path_factor is not None and res.path_factor.shape == (P, 2, n, n)
    same = p.sample_trajectories(m0, S0, n, num_particles=P, seed=3, dynamics="conditioned", return_particles=True)
    assert np.array_equal(res.particles, same.particles)
    assert np.array_equal(res.event_counts, er.counts(spec, res.particles))
    assert np.array_equal(rk.risk_particles, res.event_counts[:n, 0] / float(P))
    first = er.first_hit(spec, res.particles)[:, 0]
    any_p = np.count_nonzero((first >= 0) & (first < n)) / P
    print("sample_risk(conditioned): risk per step %s, any hit %.4f" % (rk.risk_particles.tolist(), rk.any_hit_particles))
    assert rk.any_hit_particles == any_p
    assert rk.objective_particles == float(res.reward_steps.sum()) + sp._mu() * any_p
    with pytest.raises(ValueError, match="num_features"):
        sp.sample_risk(m0, S0, n, num_particles=P, dynamics="conditioned", num_features=64)


# ------------------------------------------------------------------ refusals
def test_refusals_leave_the_outputs_untouched_and_a_valid_call_follows():
    import ctypes as C
    from pilco_amd import _lib
    p, model, policy, m0, S0 = _setup("predictions")
    P, H, E = 5, 3, 2
    x0 = p._initial_particles(m0, S0, P, 1)
    good = p.sample_trajectories(m0, S0, H, x0=x0, seed=2, return_particles=True, dynamics="conditioned", observation_noise=True)
    ctx = p.ctx
    pol, k1 = ctx._policy(p._policy_spec())
    rw, k2 = ctx._rewards(p._reward_terms(), E)
    dp = _lib._ptr

    def call(H=H, P=P, jitter=JITTER, n_events=0, events=None, counts=None, x0=x0):
        Hs = min(max(H, 0), 128)
        outs = [np.full(s, 777.0) for s in ((Hs + 1, E), (Hs + 1, E, E), (max(Hs, 1),), (Hs + 1, max(P, 1), E), (Hs, max(P, 1), E),
                                             (max(P, 1), E, Hs, Hs), (max(P, 1), E, Hs, Hs), (Hs, max(P, 1), E))]
        co = _lib.CondOut(dp(outs[7]), dp(outs[5]), dp(outs[6]))
        rc_ = ctx.lib.pilco_rollout_particles_cond(ctx.h, C.byref(pol), rw, len(p._reward_terms()), dp(x0), P, H, None, C.c_ulonglong(2),
                                                   1, dp(outs[0]), dp(outs[1]), dp(outs[2]), dp(outs[3]), dp(outs[4]), events, n_events,
                                                   counts, None, C.c_double(jitter), None, C.byref(co))
        return rc_, outs

    bad_ev = (_lib.Event * 1)()
    bad_ev[0].n_clauses = 9
    cnt = np.zeros((H + 1, 1), np.int64)
    for what, kw in (("H > 128", dict(H=129)), ("negative jitter", dict(jitter=-1e-8)), ("NaN jitter", dict(jitter=float("nan"))),
                     ("infinite jitter", dict(jitter=float("inf"))), ("P = 0", dict(P=0)), ("H < 0", dict(H=-1)),
                     ("a bad event", dict(n_events=1, events=bad_ev, counts=cnt.ctypes.data_as(C.POINTER(C.c_longlong))))):
        rc_, outs = call(**kw)
        msg = ctx.lib.pilco_last_error(ctx.h).decode()
        print("refusal, %s: status %d, %s" % (what, rc_, msg))
        assert rc_ == E_SHAPE and all(np.all(o == 777.0) for o in outs), what
    rc_, outs = call()
    assert rc_ == 0 and np.array_equal(outs[3], good.particles) and np.array_equal(outs[6], good.path_factor)
    assert np.array_equal(outs[7], good.eps_obs) and np.array_equal(outs[0], good.mean) and not np.any(outs[1] == 777.0)


def test_a_revisited_point_without_jitter_is_not_positive_definite():
    """Y = 0, so mu = 0; eps = 0, so x_1 = x_0 and the two points coincide to the bit: c_10 = c_00 = c_11 = c.  Without jitter
    Lam_00 = fl(sqrt(c)), l_0 = fl(c / Lam_00) and the pivot is d = fl(c - l_0^2), whose sign is that of the exact
    c - l_0^2: about as often negative as positive.  The restatement evaluates it on the CPU, in exact rational arithmetic on
    the c the device reports for every particle, before the call without jitter is made; the call must fail exactly where
    that pivot is not positive (16 particles: at the lowest such particle), and succeed if it is positive everywhere."""
    from fractions import Fraction
    from pilco_amd import _lib
    p, model = _tiny(zero_y=True)
    P, H = 16, 2
    x0 = np.linspace(-0.9, 0.9, P).reshape(P, 1)
    zero = np.zeros((H, P, 1))
    keep = p.sample_trajectories(None, None, H, x0=x0, eps=zero, return_particles=True, dynamics="conditioned")
    assert np.array_equal(keep.particles[1], x0) and np.array_equal(keep.particles[2], x0)      # with the default jitter: fine
    c = keep.path_cov[:, 0]
    assert np.array_equal(c[:, 1, 0], c[:, 0, 0]) and np.array_equal(c[:, 1, 1], c[:, 0, 0])    # a bit-identical revisit
    ds = []
    for q in range(P):
        c00 = float(c[q, 0, 0])
        l0 = c00 / float(np.sqrt(np.float64(c00)))
        ds.append(Fraction(c00) - Fraction(l0) ** 2)
    bad = [q for q in range(P) if ds[q] <= 0]
    print("revisit without jitter: the restatement's second pivots d / c = %s; not positive at particles %s" %
          (["%.2g" % float(d / Fraction(float(c[q, 0, 0]))) for q, d in enumerate(ds)], bad))
    kw = dict(x0=x0, eps=zero, return_particles=True, dynamics="conditioned", jitter=0.0)
    if bad:
        with pytest.raises(_lib.NotPositiveDefiniteError, match=r"particle %d, output 0 .* step 1$" % bad[0]) as ei:
            p.sample_trajectories(None, None, H, **kw)
        assert ei.value.code == E_NOT_PD and ei.value.output == 0
    else:
        p.sample_trajectories(None, None, H, **kw)
    after = p.sample_trajectories(None, None, H, x0=x0, eps=zero, return_particles=True, dynamics="conditioned")
    assert _same(keep, after)
