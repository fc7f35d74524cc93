"""Particle rollouts on posterior function samples on the MI355X: pilco_rollout_particles_fn (csrc/particles_fn.hip),
Context.rollout_particles_fn and PILCO.sample_trajectories(dynamics="function"), held to the NumPy restatement
(tests/helpers/particle_fn_restatement.py, sums in np.longdouble; tests/test_particle_fn_cpu.py pins its streams to the
header's host probe and its mathematics to the closed forms).  Every test prints its figures before it asserts (run with -s;
docs/particle_functions.md records them)."""
import ctypes as C
import os

import numpy as np
import pytest

from helpers import particle_events_restatement as er
from helpers import particle_fn_restatement as rf
from helpers import particles_restatement as pr
from pilco_amd import synthetic

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U53 = 2.0 ** -53
E_SHAPE, E_STATE = 1, 5
_CTX = None
_SETUPS = {}
_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def own_ctx():
    from pilco_amd import _lib
    global _CTX
    _CTX = _lib.Context(device=0)
    yield _CTX
    for k, v in sorted(_WORST.items()):
        print("largest ratio to the bound, %s: %.3g" % (k, v))
    _SETUPS.clear()
    _CTX.close()


def _g(name):
    return np.load(os.path.join(GOLDEN, name))


def _setup(name):
    """-> (PILCO on this module's context, restatement model, restatement policy, m0, S0)."""
    if name in _SETUPS:
        return _SETUPS[name]
    from pilco_amd import controllers
    from pilco_amd.models import PILCO
    policy = ctl = None
    if name == "predictions":          # tests/golden/predictions.npz: state 2 + 1 control, linear policy
        g = _g("predictions.npz")
        cfg = {k: g[k] for k in ("X", "Y", "lengthscales", "variance", "noise")}
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
    elif name.startswith("syn"):       # synthetic, N in {1, 65, 100}, state 3, no policy
        cfg = synthetic.config_c2(N=int(name[3:]), D=3, E=3, seed=33)
        m0 = cfg["m0"]
    else:
        raise KeyError(name)
    E = cfg["Y"].shape[1]
    p = PILCO((cfg["X"], cfg["Y"]), controller=ctl, ctx=_CTX)
    for i, mdl in enumerate(p.mgpr.models):
        mdl.kernel.lengthscales.assign(cfg["lengthscales"][i])
        mdl.kernel.variance.assign(cfg["variance"][i])
        mdl.likelihood.variance.assign(cfg["noise"][i])
    model = dict(X=cfg["X"], Y=cfg["Y"], lengthscales=cfg["lengthscales"], variance=cfg["variance"], noise=cfg["noise"])
    _SETUPS[name] = (p, model, policy, m0, 0.05 * np.eye(E))
    return _SETUPS[name]


SETUPS = ["predictions", "rbf", "syn1", "syn65", "syn100"]


def _x0(name, P, seed):
    p, _, _, m0, S0 = _setup(name)
    return p._initial_particles(m0, S0, P, seed)


def _note(key, ratio):
    _WORST[key] = max(_WORST.get(key, 0.0), float(ratio))


def _same(a, b, fields=("mean", "cov", "reward_steps", "particles", "reward")):
    return all(np.array_equal(getattr(a, f), getattr(b, f)) for f in fields)


def _same_draws(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("omega", "phase", "w", "xi", "v"))


# ------------------------------------------------------------------ the teacher-forced step, every step of every case
CASES = [(n, P, L, H) for n in SETUPS for P in (1, 63, 129) for L in (1, 63, 64, 100) for H in (0, 1, 6)]


@pytest.mark.parametrize("name,P,L,H", CASES, ids=["%s-P%d-L%d-H%d" % c for c in CASES])
def test_teacher_forced_steps_and_statistics(name, P, L, H):
    p, model, policy, m0, S0 = _setup(name)
    res = p.sample_trajectories(m0, S0, H, num_particles=P, seed=7 + P + L + H, return_particles=True, dynamics="function",
                                num_features=L)
    parts, dr = res.particles, res.function_draws
    E, (N, D) = m0.shape[1], model["X"].shape
    assert parts.shape == (H + 1, P, E) and res.mean.shape == (H + 1, E) and res.cov.shape == (H + 1, E, E)
    assert res.reward_steps.shape == (H,) and res.eps is None
    assert dr["omega"].shape == (E, L, D) and dr["phase"].shape == (E, L) and dr["w"].shape == (P, E, L)
    assert dr["xi"].shape == (P, E, N) and dr["v"].shape == (P, E, N)
    assert np.array_equal(parts[0], p._initial_particles(m0, S0, P, 7 + P + L + H))
    for t in range(H):
        xn, f, m1, m2, _ = rf.step(model, policy, dr, dr["v"], parts[t])
        bound = rf.step_bound(model, L, m1, m2, xn)
        err = np.abs(parts[t + 1] - xn)
        ratio = (err / bound).max()
        print("teacher-forced %s P=%d L=%d H=%d t=%d: largest |dx'| / bound = %.3g (largest |dx'| = %.3g)" % (name, P, L, H, t, ratio, err.max()))
        _note("teacher-forced step, " + name, ratio)
        assert np.all(err <= bound)
    xmax = np.abs(parts).max()
    mean_np = parts.mean(axis=1)
    c = parts - mean_np[:, None, :]
    cov_np = np.einsum("tpa,tpb->tab", c, c) / P
    assert np.abs(res.mean - mean_np).max() <= 4 * P * U53 * xmax and np.abs(res.cov - cov_np).max() <= 4 * P * U53 * xmax ** 2
    if P == 1:
        assert not res.cov.any()
    if H > 0:
        terms = [dict(kind="exponential", W=np.eye(E), t=None, coef=1.0)]   # PILCO's default reward
        r_np = np.array([pr.reward(terms, parts[t]) for t in range(H)])
        assert np.abs(res.reward_steps - r_np.mean(axis=1)).max() <= (4 * P * U53 + 1e-12) * max(np.abs(r_np).max(), 1e-300)
        assert res.reward[0, 0] == res.reward_steps.sum()


# ------------------------------------------------------------------ the generated draws and V
@pytest.mark.parametrize("name", ["predictions", "rbf", "syn65"])
def test_generated_draws_are_the_streams(name):
    p, model, _, m0, S0 = _setup(name)
    P, L, seed = 129, 100, 2 ** 33 + 5
    dr = p.sample_trajectories(m0, S0, 0, num_particles=P, seed=seed, return_particles=True, dynamics="function", num_features=L).function_draws
    ls = np.asarray(model["lengthscales"])
    E, (N, D) = ls.shape[0], model["X"].shape
    z, r = rf.freq_normals(seed, E, L, D)
    b_om = (16 * np.maximum(1.0, r) + np.abs(z)) * U53 / ls[:, None, :]     # the normal's bound and the rounding of the division
    rat = [(np.abs(dr["omega"] - z / ls[:, None, :]) / b_om).max(),
           (np.abs(dr["phase"] - rf.phases(seed, E, L)) / (4 * U53 * 2 * np.pi)).max()]
    for key, (want, rr) in (("w", rf.weights(seed, np.arange(P), E, L)), ("xi", rf.xis(seed, np.arange(P), E, N))):
        rat.append((np.abs(dr[key] - want) / (16 * U53 * np.maximum(1.0, rr))).max())
    print("generated draws %s: largest error / bound: omega %.3g, phase %.3g, w %.3g, xi %.3g" % (name, *rat))
    for k, v in zip(("omega", "phase", "w", "xi"), rat):
        _note("generated " + k, v)
    assert max(rat) <= 1.0
    assert np.all((dr["phase"] >= 0) & (dr["phase"] < 2 * np.pi))


@pytest.mark.parametrize("name,P,L", [(n, P, L) for n in SETUPS for (P, L) in ((129, 100), (1, 1), (63, 64))])
def test_v_is_iK_times_the_residual(name, P, L):
    p, model, _, m0, S0 = _setup(name)
    dr = p.sample_trajectories(m0, S0, 0, num_particles=P, seed=3, return_particles=True, dynamics="function", num_features=L).function_draws
    E, N = model["Y"].shape[1], model["X"].shape[0]
    iK, _ = _CTX.gp_get_factors(0, E)
    V, mag = rf.v_of(model, dr, iK)
    npad, Lpad = (N + 63) // 64 * 64, (L + 63) // 64 * 64
    bound = ((npad + Lpad + 8) * U53 * mag).astype(np.float64)
    err = np.abs(dr["v"] - V.astype(np.float64))
    ratio = (err / bound).max()
    print("V %s P=%d L=%d: largest error / bound = %.3g (largest |v| = %.3g)" % (name, P, L, ratio, np.abs(dr["v"]).max()))
    _note("V, " + name, ratio)
    assert np.all(err <= bound)


# ------------------------------------------------------------------ bits
@pytest.mark.parametrize("name", ["predictions", "rbf", "syn65"])
def test_a_particle_has_the_same_bits_alone_permuted_fed_back_and_run_to_run(name):
    p, model, _, m0, S0 = _setup(name)
    P, L, H, seed = 129, 63, 4, 12
    x0 = _x0(name, P, 2)
    ev = [dict(clauses=[(0, float(m0[0, 0]), None)], complement=False)]
    kw = dict(x0=x0, seed=seed, return_particles=True, dynamics="function", num_features=L, events=ev)
    a = p.sample_trajectories(m0, S0, H, **kw)
    b = p.sample_trajectories(m0, S0, H, **kw)
    ef = ("event_counts", "first_hit")
    assert _same(a, b) and _same(a, b, ef) and _same_draws(a.function_draws, b.function_draws)
    # fed back: every output bitwise (the seed no longer matters)
    c = p.sample_trajectories(m0, S0, H, **dict(kw, seed=999, function_draws=a.function_draws))
    assert _same(a, c) and _same(a, c, ef) and _same_draws(a.function_draws, c.function_draws)
    # alone: particle 0 with the generated draws, particle 77 with its own draws fed back
    one = p.sample_trajectories(m0, S0, H, **dict(kw, x0=x0[:1]))
    assert np.array_equal(one.particles[:, 0], a.particles[:, 0]) and np.array_equal(one.function_draws["v"][0], a.function_draws["v"][0])
    q = 77
    d77 = dict(a.function_draws, w=a.function_draws["w"][q:q + 1], xi=a.function_draws["xi"][q:q + 1])
    alone = p.sample_trajectories(m0, S0, H, **dict(kw, x0=x0[q:q + 1], function_draws=d77))
    assert np.array_equal(alone.particles[:, 0], a.particles[:, q]) and np.array_equal(alone.function_draws["v"][0], a.function_draws["v"][q])
    assert np.array_equal(alone.first_hit[0], a.first_hit[q])
    # permuted
    perm = np.random.RandomState(1).permutation(P)
    dp = dict(a.function_draws, w=a.function_draws["w"][perm], xi=a.function_draws["xi"][perm])
    pm = p.sample_trajectories(m0, S0, H, **dict(kw, x0=x0[perm], function_draws=dp))
    assert np.array_equal(pm.particles, a.particles[:, perm]) and np.array_equal(pm.first_hit, a.first_hit[perm])
    assert np.array_equal(pm.event_counts, a.event_counts)
    # without observation_noise the step draws are not read: two different eps arrays, identical bits
    e1, e2 = np.random.RandomState(2).randn(H, P, x0.shape[1]), np.random.RandomState(3).randn(H, P, x0.shape[1])
    r1 = p.sample_trajectories(m0, S0, H, **dict(kw, eps=e1))
    r2 = p.sample_trajectories(m0, S0, H, **dict(kw, eps=e2))
    assert _same(a, r1) and _same(a, r2) and r1.eps is None


def test_one_function_per_particle_is_consistent_where_marginal_draws_are_not():
    """The property the feature exists for: two particles with the same x0 row and the same (w, xi) ARE the same function --
    identical trajectories over H = 6; the marginal path on the same x0 with its different draws separates them."""
    p, model, _, m0, S0 = _setup("rbf")
    P, L, H = 8, 64, 6
    x0 = np.tile(_x0("rbf", 1, 4), (P, 1))
    first = p.sample_trajectories(m0, S0, H, x0=x0, seed=1, return_particles=True, dynamics="function", num_features=L)
    d = first.function_draws
    assert not np.array_equal(first.particles[-1, 0], first.particles[-1, 1])          # different functions: different paths
    same = dict(d, w=np.tile(d["w"][:1], (P, 1, 1)), xi=np.tile(d["xi"][:1], (P, 1, 1)))
    twin = p.sample_trajectories(m0, S0, H, x0=x0, return_particles=True, dynamics="function", function_draws=same)
    for q in range(1, P):
        assert np.array_equal(twin.particles[:, q], twin.particles[:, 0])
    assert np.array_equal(twin.particles[:, 0], first.particles[:, 0]) and not twin.cov[-1].any()
    marg = p.sample_trajectories(m0, S0, H, x0=x0, seed=1, return_particles=True)
    assert not np.array_equal(marg.particles[1, 0], marg.particles[1, 1])
    print("consistency: spread of dim 0 after %d steps: one function %.3g, marginal draws %.3g"
          % (H, np.ptp(twin.particles[-1, :, 0]), np.ptp(marg.particles[-1, :, 0])))


def test_the_marginal_path_is_untouched():
    p, _, _, m0, S0 = _setup("rbf")
    kw = dict(num_particles=129, seed=5, return_particles=True)
    a = p.sample_trajectories(m0, S0, 3, **kw)
    b = p.sample_trajectories(m0, S0, 3, dynamics="marginal", **kw)
    assert _same(a, b, ("mean", "cov", "reward_steps", "particles", "eps", "reward")) and a.function_draws is None and b.function_draws is None
    with pytest.raises(ValueError):
        p.sample_trajectories(m0, S0, 3, dynamics="exact", **kw)


# ------------------------------------------------------------------ events, rewards, observation noise
def test_events_are_exact_on_the_returned_particles():
    p, _, _, m0, S0 = _setup("rbf")
    P, H, L = 129, 6, 100
    kw = dict(num_particles=P, seed=8, return_particles=True, dynamics="function", num_features=L)
    base = p.sample_trajectories(m0, S0, H, **kw)
    parts = base.particles
    last = parts[-1]
    q = int(np.argsort(last[:, 0], kind="stable")[P // 2])
    med, top = float(last[q, 0]), float(last[:, 0].max())
    q10, q90 = (float(v) for v in np.quantile(parts[..., 0], [0.1, 0.9]))
    r10, r90 = (float(v) for v in np.quantile(parts[..., 2], [0.1, 0.9]))
    events = [dict(clauses=[(0, med, top), (2, float(parts[..., 2].min()), float(parts[..., 2].max()))], complement=False),
              dict(clauses=[(0, med, None)], complement=False),
              dict(clauses=[(2, r10, r90)], complement=True),
              dict(clauses=[(0, q10, q90), (2, r10, r90), (0, None, top), (2, None, None)], complement=False),
              dict(clauses=[(2, float(last[q, 2]), float(last[q, 2]))], complement=False),
              dict(clauses=[(2, None, float(np.median(parts[H // 2][:, 2])))], complement=True),
              dict(clauses=[(0, None, None)], complement=False),
              dict(clauses=[(0, q90, q90 + 1e-3), (2, None, r10)], complement=False)]
    res = p.sample_trajectories(m0, S0, H, events=events, **kw)
    assert _same(base, res)
    print("events on function samples: counts at the last state %s, ever %s"
          % (res.event_counts[-1].tolist(), (res.first_hit >= 0).sum(axis=0).tolist()))
    assert np.array_equal(res.event_counts, er.counts(events, parts)) and np.array_equal(res.first_hit, er.first_hit(events, parts))
    assert res.event_counts[-1, 0] >= 1 and res.event_counts[-1, 6] == P


def test_sample_risk_on_function_samples():
    """SafePILCO.sample_risk(dynamics="function"): the fields are their definitions on the function-sample particles, and the
    moment-matched column does not depend on the dynamics argument."""
    from pilco_amd import rewards
    from pilco_amd.safe import RiskOfCollision, SafePILCO
    p, model, _, m0, S0 = _setup("rbf")
    P, n, mu, E, L = 300, 5, -3.0, 3, 64
    probe = p.sample_trajectories(m0, S0, n, num_particles=P, seed=9, return_particles=True, dynamics="function", num_features=L)
    lo = np.quantile(probe.particles[..., [0, 2]].reshape(-1, 2), 0.3, axis=0)
    hi = np.quantile(probe.particles[..., [0, 2]].reshape(-1, 2), 0.8, axis=0)
    risk = RiskOfCollision(E, lo, hi)
    sp = SafePILCO((model["X"], model["Y"]), controller=p.controller, reward_add=rewards.ExponentialReward(E), reward_mult=risk,
                   mu=mu, horizon=n, ctx=_CTX)
    for i, mdl in enumerate(sp.mgpr.models):
        mdl.kernel.lengthscales.assign(model["lengthscales"][i])
        mdl.kernel.variance.assign(model["variance"][i])
        mdl.likelihood.variance.assign(model["noise"][i])
    r = sp.sample_risk(m0, S0, n, num_particles=P, seed=9, return_particles=True, dynamics="function", num_features=L)
    marg = sp.sample_risk(m0, S0, n, num_particles=P, seed=9)
    tr = r.trajectories
    spec = risk.event_spec()
    hits = er.hit(spec, tr.particles)
    first = er.first_hit([spec], tr.particles)[:, 0]
    any_p = float(np.mean((first >= 0) & (first < n)))
    print("sample_risk on function samples: risk_particles %s (marginal draws %s), any hit %.4g (marginal draws %.4g, moment matched %.4g)"
          % (r.risk_particles.tolist(), marg.risk_particles.tolist(), r.any_hit_particles, marg.any_hit_particles, r.any_hit_moment_matched))
    assert np.array_equal(tr.particles, probe.particles) and tr.function_draws is not None
    assert np.array_equal(r.risk_particles, hits[:n].sum(axis=1) / P) and np.array_equal(tr.first_hit[:, 0], first)
    assert 0 < any_p < 1 and abs(r.any_hit_particles - any_p) <= 4 * U53
    assert abs(r.objective_particles - (tr.reward_steps.sum() + mu * any_p)) <= 4 * U53 * abs(r.objective_particles)
    assert np.array_equal(r.risk_moment_matched, marg.risk_moment_matched) and r.objective_moment_matched == marg.objective_moment_matched
    assert marg.trajectories.function_draws is None


def test_reward_of_particles_at_one_point_and_the_observation_noise():
    from pilco_amd import _lib
    p, model, _, m0, S0 = _setup("predictions")
    p.mgpr._ensure_factorized()
    g = _g("reward.npz")
    E = 2
    expo = dict(kind=_lib.REWARD_EXPONENTIAL, coef=1.0, W=g["W2"], t=g["t2"].ravel())
    lin = dict(kind=_lib.REWARD_LINEAR, coef=1.0, W=g["W_lin"])
    comb = [dict(expo, coef=float(g["coefs"][0])), dict(lin, coef=float(g["coefs"][1]))]
    worst = 0.0
    for m in (g["m"], m0, np.array([[0.3, -1.1]])):
        x0 = np.tile(np.asarray(m, np.float64).reshape(1, E), (65, 1))
        for terms in ([expo], [lin], comb):
            rew = _CTX.rollout_particles_fn(p._policy_spec(), terms, x0, 1, num_features=8, seed=1)[2]
            want = float(np.ravel(_CTX.reward_eval(terms, E, m, np.zeros((E, E)))[0])[0])
            worst = max(worst, abs(rew[0] - want) / abs(want))
            assert abs(rew[0] - want) <= 1e-12 * abs(want)
    print("reward parity on function samples: largest relative difference %.3g (bound 1e-12)" % worst)
    # observation noise: x' = the noiseless x' + sqrt(noise) eps_out, one step from the same states
    P, L = 129, 64
    kw = dict(x0=_x0("predictions", P, 6), seed=6, return_particles=True, dynamics="function", num_features=L)
    quiet = p.sample_trajectories(m0, S0, 1, **kw)
    noisy = p.sample_trajectories(m0, S0, 1, observation_noise=True, **kw)
    assert quiet.eps is None and noisy.eps.shape == (1, P, E) and _same_draws(quiet.function_draws, noisy.function_draws)
    z, r = pr.normals(6, 1, P, E)
    assert np.all(np.abs(noisy.eps - z) <= 16 * U53 * np.maximum(1.0, r))             # the step stream {p, t, j, 0}
    want = quiet.particles[1] + np.sqrt(model["noise"])[None, :] * noisy.eps[0]
    err = np.abs(noisy.particles[1] - want)
    print("observation noise: largest |dx'| / (4 2^-53 |x'|) = %.3g" % (err / (4 * U53 * np.abs(want))).max())
    assert np.all(err <= 4 * U53 * np.abs(want))
    fed = p.sample_trajectories(m0, S0, 1, observation_noise=True, eps=noisy.eps, **dict(kw, seed=77, function_draws=noisy.function_draws))
    assert _same(noisy, fed) and np.array_equal(fed.eps, noisy.eps)


@pytest.mark.parametrize("name", ["predictions", "rbf"])
def test_statistics_against_moment_matching_where_it_is_exact(name):
    """s_x = 0, one step: the mean against propagate(m, 0) within 5 sqrt(S / P); the variance against the closed form of the
    L-feature prior (NOT against S: the feature bias is a property of the method, docs/particle_functions.md)."""
    p, model, policy, m0, _ = _setup(name)
    E, P, L = m0.shape[1], 4096, 256
    M, S = p.propagate(m0, np.zeros((E, E)))
    res = p.sample_trajectories(m0, np.zeros((E, E)), 1, num_particles=P, seed=0, return_particles=True, dynamics="function", num_features=L)
    assert np.array_equal(res.mean[0], m0.ravel()) and not res.cov[0].any()
    d = res.function_draws
    xu = np.concatenate([m0, pr.action(policy, m0)], axis=1)
    _, var = rf.closed_form(model, d["omega"], d["phase"], xu)
    Sd, var = np.diag(S), var[0]
    dm, dv = np.abs(res.mean[1] - np.ravel(M)), np.abs(np.diag(res.cov[1]) - var)
    rm, rv = (dm / (5 * np.sqrt(Sd / P))).max(), (dv / (5 * var * np.sqrt(2 / P))).max()
    print("moment matching %s: |dmean| / (5 sqrt(S/P)) = %.3g, |dvar| / (5 var_closed sqrt(2/P)) = %.3g, var_closed / S = %s"
          % (name, rm, rv, np.array2string(var / Sd, precision=3)))
    _note("moment matching mean, " + name, rm)
    _note("moment matching variance, " + name, rv)
    assert np.all(dm <= 5 * np.sqrt(Sd / P)) and np.all(dv <= 5 * var * np.sqrt(2 / P))


# ------------------------------------------------------------------ refusals
def test_refusals(monkeypatch):
    from pilco_amd import _lib
    g = _g("predictions.npz")
    E, U, D, N, P, H, L = 2, 1, 3, 100, 10, 2, 16
    x0 = np.random.RandomState(0).randn(P, E)
    spec = dict(kind=_lib.POLICY_LINEAR, state_dim=E, control_dim=U, W=np.ones((U, E)), b=np.zeros(U), max_action=1.0)
    rw = [dict(kind=_lib.REWARD_EXPONENTIAL, coef=1.0, W=np.eye(E), t=None)]
    cx = _lib.Context(device=0)
    try:
        cx.gp_set_data(0, g["X"], g["Y"])
        cx.gp_set_hyp(0, g["lengthscales"], g["variance"], g["noise"])
        pol, k1 = cx._policy(spec)
        terms, k2 = cx._rewards(rw, E)
        q = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
        mean, cov, parts = np.full((H + 1, E), -7.0), np.full((H + 1, E, E), -7.0), np.full((H + 1, P, E), -7.0)
        vout = np.full((P, E, N), -7.0)
        om, ph, w, xi = np.ones((E, L, D)), np.ones((E, L)), np.ones((P, E, L)), np.ones((P, E, N))

        def raw(draws, P_=P, n_events=0):
            do = _lib.FunctionDrawsOut(None, None, None, None, q(vout))
            return cx.lib.pilco_rollout_particles_fn(cx.h, C.byref(pol), terms, 1, q(x0), P_, H, None, C.c_ulonglong(0), 0, q(mean), q(cov),
                                                     None, q(parts), None, None, n_events, None, None,
                                                     None if draws is None else C.byref(draws), C.byref(do))
        F = _lib.FunctionDraws
        bad = [("null draws", None, {}, E_SHAPE), ("L = 0", F(0, None, None, None, None), {}, E_SHAPE),
               ("L = 4097", F(4097, None, None, None, None), {}, E_SHAPE),
               ("omega alone", F(L, q(om), None, None, None), {}, E_SHAPE),
               ("three of four", F(L, q(om), q(ph), q(w), None), {}, E_SHAPE),
               ("P = 0: an existing refusal", F(L, None, None, None, None), dict(P_=0), E_SHAPE),
               ("events without a table: an existing refusal", F(L, None, None, None, None), dict(n_events=1), E_SHAPE)]
        for what, dr, kw, code in bad:
            rc = raw(dr, **kw)
            print("refusal %-45s -> %d  %s" % (what, rc, cx.lib.pilco_last_error(cx.h).decode()))
            assert rc == code, what
            assert all(np.all(a == -7.0) for a in (mean, cov, parts, vout))
        # the budget: E Ppad (Lpad + 2 npad) = 2 * 64 * (64 + 256) doubles
        monkeypatch.setenv("PILCO_PARTICLE_FN_BUDGET", str(2 * 64 * (64 + 256) - 1))
        assert raw(F(L, None, None, None, None)) == E_SHAPE and b"largest P that fits is 0" in cx.lib.pilco_last_error(cx.h)
        monkeypatch.setenv("PILCO_PARTICLE_FN_BUDGET", str(2 * 128 * (64 + 256)))
        assert raw(F(L, None, None, None, None), P_=P) == 0
        monkeypatch.delenv("PILCO_PARTICLE_FN_BUDGET")
        # a sparse slot
        cs = _lib.Context(device=0)
        try:
            cs.gp_set_data(0, g["X"], g["Y"])
            cs.gp_set_hyp(0, g["lengthscales"], g["variance"], g["noise"])
            cs.gp_set_inducing(0, g["X"][:20])
            mean[:] = -7.0
            rc = cs.lib.pilco_rollout_particles_fn(cs.h, C.byref(pol), terms, 1, q(x0), P, H, None, C.c_ulonglong(0), 0, q(mean), q(cov),
                                                   None, None, None, None, 0, None, None, C.byref(F(L, None, None, None, None)), None)
            print("refusal sparse slot -> %d  %s" % (rc, cs.lib.pilco_last_error(cs.h).decode()))
            assert rc == E_STATE and b"sparse" in cs.lib.pilco_last_error(cs.h) and np.all(mean == -7.0)
        finally:
            cs.close()
        # a valid call after them is correct: the binding on the same context gives the same particles
        mean[:], parts[:] = -7.0, -7.0
        assert raw(F(L, None, None, None, None)) == 0
        ref = cx.rollout_particles_fn(spec, rw, x0, H, num_features=L, seed=0, want_particles=True, want_draws=True)
        assert np.array_equal(parts, ref[3]) and np.array_equal(mean, ref[0]) and np.array_equal(vout, ref[7]["v"])
        assert np.all(np.isfinite(parts)) and np.array_equal(parts[0], x0)
    finally:
        cx.close()
