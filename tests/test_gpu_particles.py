"""Particle rollouts through the learned dynamics on the MI355X: PILCO.sample_trajectories, Context.rollout_particles and the C
entry point under them, pilco_rollout_particles (csrc/particles.hip, DESIGN.md section 13, docs/particles.md).  The yardstick
is the NumPy float64 restatement of one particle step in tests/helpers/particles_restatement.py, which
tests/test_particles_cpu.py pins to the executed reference.  Every figure a bound is held against is printed before the
assertion (run with -s to see them; docs/particles.md records them)."""
import ctypes as C
import os

import numpy as np
import pytest

from helpers import particles_restatement as pr
from pilco_amd import synthetic

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
E_SHAPE, E_STATE = 1, 5
U53 = 2.0 ** -53
_CTX = None
_SETUPS = {}


@pytest.fixture(scope="module", autouse=True)
def own_ctx():
    """The models of this module live on a context of their own (closed at the end), not on the process-wide default."""
    from pilco_amd import _lib
    global _CTX
    _CTX = _lib.Context(device=0)
    yield _CTX
    _SETUPS.clear()
    _CTX.close()


def _g(name):
    return np.load(os.path.join(GOLDEN, name))


def _set_hyp(model, cfg):
    for i, mdl in enumerate(model.models):
        mdl.kernel.lengthscales.assign(cfg["lengthscales"][i])
        mdl.kernel.variance.assign(cfg["variance"][i])
        mdl.likelihood.variance.assign(cfg["noise"][i])


def _setup(name):
    """-> (PILCO object on this module's context, restatement model, restatement policy, restatement reward terms, m0, S0)."""
    if name in _SETUPS:
        return _SETUPS[name]
    from pilco_amd import controllers
    from pilco_amd.models import PILCO
    Z = None
    if name == "predictions":          # tests/golden/predictions.npz: 3 inputs, 2 outputs -> state 2 + 1 control, linear
        g = _g("predictions.npz")
        cfg = {k: g[k] for k in ("X", "Y", "lengthscales", "variance", "noise")}
        W, b, maxact = np.array([[0.7, -0.4]]), np.array([[0.15]]), 1.3
        m0, S0 = cfg["X"][:1, :2], 0.05 * np.eye(2)
    elif name == "c2":                 # N = 1000, D = E = 10, no policy
        cfg = synthetic.config_c2(N=1000, D=10, E=10)
        W = b = maxact = None
        m0, S0 = cfg["m0"], 0.05 * np.eye(10)
    elif name == "c2u":                # the C2u shape: state 10 + 1 control, linear
        cfg = synthetic.config_c2(N=1000, D=11, E=10, control_dim=1)
        W, b, maxact = cfg["W"] * 5.0, cfg["b"] + 0.2, 1.5
        m0, S0 = cfg["m0"], 0.05 * np.eye(10)
    elif name == "rbf":                # an RbfController on the rbf_controller.npz policy (state 3 -> 2 controls)
        cfg = synthetic.config_c2(N=300, D=5, E=3, control_dim=2, seed=21)
        W = b = None
        maxact = 2.0
        m0, S0 = cfg["m0"], 0.05 * np.eye(3)
    elif name == "c4":                 # SMGPR, N = 5000, M = 200
        cfg = synthetic.config_c4(N=5000, M=200)
        Z = cfg["Z"]
        W = b = maxact = None
        m0, S0 = cfg["m0"], 0.05 * np.eye(10)
    else:
        raise KeyError(name)
    E = cfg["Y"].shape[1]
    U = cfg["X"].shape[1] - E
    policy, ctl = None, None
    if name == "rbf":
        g = _g("rbf_controller.npz")
        ctl = controllers.RbfController(E, U, g["X"].shape[0], max_action=maxact, ctx=_CTX)
        ctl.set_data((g["X"], g["Y"]))
        for i, mdl in enumerate(ctl.models):
            mdl.kernel.lengthscales.assign(g["lengthscales"][i])
        policy = dict(kind="rbf", X=g["X"], Y=g["Y"], lengthscales=g["lengthscales"], noise=np.full(U, 1e-4), max_action=maxact)
    elif U > 0:
        ctl = controllers.LinearController(E, U, max_action=maxact, ctx=_CTX)
        ctl.W.assign(W)
        ctl.b.assign(b)
        policy = dict(kind="linear", W=W, b=b, max_action=maxact)
    p = PILCO((cfg["X"], cfg["Y"]), num_induced_points=None if Z is None else Z.shape[0], controller=ctl, ctx=_CTX)
    _set_hyp(p.mgpr, cfg)
    if Z is not None:
        for mdl in p.mgpr.models:
            mdl.inducing_variable.Z.assign(Z)
    model = dict(X=cfg["X"], Y=cfg["Y"], lengthscales=cfg["lengthscales"], variance=cfg["variance"], noise=cfg["noise"], Z=Z)
    terms = [dict(kind="exponential", W=np.eye(E), t=None, coef=1.0)]   # PILCO's default reward
    _SETUPS[name] = (p, model, policy, terms, m0, S0)
    return _SETUPS[name]


def _step_bound(model, mu, v, eps, xn, observation_noise):
    """1e-8 max|mu_e| + |eps| (sqrt(v + d) - sqrt(max(v - d, 0))) + 4 * 2^-53 |x'_e|,  d = 1e-8 sf2_e: the tolerance of the
    predict_f tests (mean within 1e-8 max|mu_e|, variance within 1e-8 sf2_e) carried through the update."""
    d = 1e-8 * np.asarray(model["variance"]).reshape(1, -1)
    return (1e-8 * np.abs(mu).max(axis=0, keepdims=True) + np.abs(eps) * (np.sqrt(v + d) - np.sqrt(np.maximum(v - d, 0.0)))
            + 4 * U53 * np.abs(xn))


def _check_run(name, res, x0, P, H, obs):
    """Teacher-forced step check over every step of the run, and the statistics against NumPy on the returned particles."""
    p, model, policy, terms, _, _ = _setup(name)
    E = x0.shape[1]
    parts, eps = res.particles, res.eps
    assert parts.shape == (H + 1, P, E) and eps.shape == (H, P, E) and res.mean.shape == (H + 1, E)
    assert res.cov.shape == (H + 1, E, E) and res.reward_steps.shape == (H,) and res.reward.shape == (1, 1)
    assert np.array_equal(parts[0], x0)
    if H > 0:
        X = parts[:-1].reshape(H * P, E)
        xn, mu, v, _ = pr.step(model, policy, X, eps.reshape(H * P, E), obs)
        bound = _step_bound(model, mu, v, eps.reshape(H * P, E), xn, obs)
        err = np.abs(parts[1:].reshape(H * P, E) - xn)
        print("teacher-forced %s P=%d H=%d obs=%d: largest |dx'| / bound = %.3g (largest |dx'| = %.3g)"
              % (name, P, H, obs, (err / bound).max(), err.max()))
        assert np.all(err <= bound)
    # statistics: summation-error bounds
    xmax = np.abs(parts).max()
    mean_np = parts.mean(axis=1)
    c = parts - mean_np[:, None, :]
    cov_np = np.einsum("tpa,tpb->tab", c, c) / P
    e_mean, e_cov = np.abs(res.mean - mean_np).max(), np.abs(res.cov - cov_np).max()
    print("statistics %s P=%d H=%d: |dmean| = %.3g (bound %.3g), |dcov| = %.3g (bound %.3g)"
          % (name, P, H, e_mean, 4 * P * U53 * xmax, e_cov, 4 * P * U53 * xmax ** 2))
    assert e_mean <= 4 * P * U53 * xmax and e_cov <= 4 * P * U53 * xmax ** 2
    assert np.array_equal(res.cov, np.swapaxes(res.cov, 1, 2))
    if P == 1:
        assert not res.cov.any()
    if H > 0:
        r_np = np.array([pr.reward(terms, parts[t]) for t in range(H)])
        rmax = max(np.abs(r_np).max(), 1e-300)
        e_rew = np.abs(res.reward_steps - r_np.mean(axis=1)).max()
        # the sum's bound, and 1e-12 relative for the evaluation of a particle's reward (the bound of the reward-parity test)
        assert e_rew <= (4 * P * U53 + 1e-12) * rmax, (e_rew, rmax)
        assert res.reward[0, 0] == res.reward_steps.sum()
    else:
        assert res.reward[0, 0] == 0.0


CASES = [(n, P, H) for n in ("predictions", "c2", "c2u", "rbf") for P in (1, 63, 1000, 4097) for H in (0, 1, 10)]
CASES += [("c4", P, 3) for P in (1, 63, 1000, 4097)]


@pytest.mark.parametrize("obs", [False, True])
@pytest.mark.parametrize("name,P,H", CASES, ids=["%s-P%d-H%d" % c for c in CASES])
def test_teacher_forced_steps_and_statistics(name, P, H, obs):
    p, _, _, _, m0, S0 = _setup(name)
    res = p.sample_trajectories(m0, S0, H, num_particles=P, seed=5 + P + H, observation_noise=obs, return_particles=True)
    _check_run(name, res, res.particles[0], P, H, obs)
    assert type(res).__name__ == "ParticleTrajectories" and res.mean.dtype == np.float64


def _raw_run(name, x0, H, eps=None, seed=0, obs=False, want_particles=True):
    p, _, _, _, _, _ = _setup(name)
    p.mgpr._user_factors = None
    p.mgpr._ensure_factorized()
    return _CTX.rollout_particles(p._policy_spec(), p._reward_terms(), x0, H, eps=eps, seed=seed, observation_noise=obs,
                                  want_particles=want_particles)


def _x0(name, P, seed):
    _, _, _, _, m0, S0 = _setup(name)
    return m0 + np.random.RandomState(seed).randn(P, m0.shape[1]) * np.sqrt(np.diag(S0))


def _same(a, b):
    return all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", ["c2u", "rbf"])
def test_a_particle_has_the_same_bits_alone_permuted_and_run_to_run(name):
    P, H = 4097, 4
    x0 = _x0(name, P, 3)
    eps = np.random.RandomState(4).randn(H, P, x0.shape[1])
    full = _raw_run(name, x0, H, eps=eps)
    assert _same(full, _raw_run(name, x0, H, eps=eps))          # run to run: particles, mean, cov, rewards
    for q in (0, 1, 1599, 1600, 3199, 3200, 4096):              # alone = row q of the batch, at the chunk boundaries too
        one = _raw_run(name, x0[q:q + 1], H, eps=eps[:, q:q + 1])
        assert np.array_equal(one[3][:, 0], full[3][:, q]), q
    perm = np.random.RandomState(5).permutation(P)
    pm = _raw_run(name, x0[perm], H, eps=eps[:, perm])
    assert np.array_equal(pm[3], full[3][:, perm])
    assert np.array_equal(pm[4], eps[:, perm])                  # the draws used = the draws given


@pytest.mark.parametrize("name", ["predictions", "c2u"])
def test_seed_path(name):
    H = 3
    x63, x4097 = _x0(name, 63, 1), _x0(name, 4097, 1)
    E = x63.shape[1]
    a = _raw_run(name, x4097, H, seed=1234)
    assert _same(a, _raw_run(name, x4097, H, seed=1234))        # the same seed: the same bits
    b = _raw_run(name, x4097, H, seed=1235)
    assert not np.array_equal(a[4], b[4]) and np.abs(a[4] - b[4]).max() > 1.0
    assert _same(a, _raw_run(name, x4097, H, eps=a[4]))         # the draws fed back: every output bitwise
    s = _raw_run(name, x63, H, seed=1234)
    assert np.array_equal(s[4], a[4][:, :63])                   # a draw depends on (seed, t, p, e), not on P
    # the draws against the Python restatement of the stream
    sel = list(range(63)) + [1599, 1600, 3200, 4096]
    z, r = pr.normals(1234, H, 4097, E, particles=sel)
    dz = np.abs(a[4][:, sel] - z[:, sel])
    bound = 16 * U53 * np.maximum(1.0, r[:, sel])
    print("seed path %s: largest |dz| / bound = %.3g (largest |dz| = %.3g) over %d draws" % (name, (dz / bound).max(), dz.max(), dz.size))
    assert np.all(dz <= bound)
    big = 2 ** 64 - 3                                           # both key words in use
    zb, rb = pr.normals(big, 1, 2, E)
    eb = _raw_run(name, x63[:2], 1, seed=big)[4]
    assert np.all(np.abs(eb - zb) <= 16 * U53 * np.maximum(1.0, rb))
    # the standard normal it claims to be
    assert abs(a[4].mean()) < 5 / np.sqrt(a[4].size) and abs(a[4].var() - 1) < 5 * np.sqrt(2 / a[4].size)


def test_reward_of_particles_at_one_point_is_the_device_reward_at_zero_covariance():
    from pilco_amd import _lib
    p, _, _, _, m0, _ = _setup("predictions")
    p.mgpr._ensure_factorized()
    g = _g("reward.npz")
    E = 2
    expo = dict(kind=_lib.REWARD_EXPONENTIAL, coef=1.0, W=g["W2"], t=g["t2"].ravel())
    lin = dict(kind=_lib.REWARD_LINEAR, coef=1.0, W=g["W_lin"])
    comb = [dict(expo, coef=float(g["coefs"][0])), dict(lin, coef=float(g["coefs"][1]))]
    for m in (g["m"], m0, np.array([[0.3, -1.1]])):
        x0 = np.tile(np.asarray(m, np.float64).reshape(1, E), (64, 1))
        for terms in ([expo], [lin], comb, [dict(expo, t=None, W=np.eye(E))]):
            _, _, rew, _, _ = _CTX.rollout_particles(p._policy_spec(), terms, x0, 1, seed=1)
            want = float(np.ravel(_CTX.reward_eval(terms, E, m, np.zeros((E, E)))[0])[0])
            print("reward parity: %.17g vs %.17g" % (rew[0], want))
            assert abs(rew[0] - want) <= 1e-12 * abs(want)


@pytest.mark.parametrize("name", ["predictions", "c2u", "c4"])
def test_agreement_with_moment_matching_where_it_is_exact(name):
    """s_x = 0, one step: the particles are exact draws from the Gaussian propagate(m, 0) returns."""
    p, _, _, _, m0, _ = _setup(name)
    E, P = m0.shape[1], 4096
    M, S = p.propagate(m0, np.zeros((E, E)))
    res = p.sample_trajectories(m0, np.zeros((E, E)), 1, num_particles=P, seed=0)
    assert np.array_equal(res.mean[0], m0.ravel()) and not res.cov[0].any()
    Sd = np.diag(S)
    dm, dv = np.abs(res.mean[1] - np.ravel(M)), np.abs(np.diag(res.cov[1]) - Sd)
    print("moment matching %s: |dmean| / (5 sqrt(S/P)) = %.3g, |dvar| / (5 S sqrt(2/P)) = %.3g"
          % (name, (dm / (5 * np.sqrt(Sd / P))).max(), (dv / (5 * Sd * np.sqrt(2 / P))).max()))
    assert np.all(dm <= 5 * np.sqrt(Sd / P))
    assert np.all(dv <= 5 * Sd * np.sqrt(2 / P))


@pytest.mark.parametrize("name", ["predictions", "c2u", "rbf"])
def test_action_is_the_device_policy_action_at_zero_covariance(name):
    """The action kernel alone (pilco_debug_particle_actions) against pilco_policy_action(x, s = 0)[0], and against the
    restatement the teacher-forced check steps with."""
    p, _, policy, _, _, _ = _setup(name)
    x = _x0(name, 6, 8)
    E = x.shape[1]
    p.mgpr._ensure_factorized()
    u = _CTX.particle_actions(p._policy_spec(), x)
    for i in range(6):
        want = np.ravel(p.compute_action(x[i:i + 1]))
        rel = np.abs(u[i] - want) / np.abs(want)
        print("action parity %s: largest relative difference %.3g" % (name, rel.max()))
        assert np.all(rel <= 1e-12)
    np.testing.assert_allclose(u, pr.action(policy, x), rtol=1e-11)


def _raw(cx, pol, terms, n_rw, x0, P, H, eps, mean, cov, rew=None, parts=None, used=None, obs=0):
    q = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    return cx.lib.pilco_rollout_particles(cx.h, None if pol is None else C.byref(pol), terms, n_rw, q(x0), P, H, q(eps),
                                          C.c_ulonglong(0), obs, q(mean), q(cov), q(rew), q(parts), q(used))


def test_refusals():
    from pilco_amd import _lib
    g = _g("predictions.npz")
    cfg = {k: g[k] for k in ("X", "Y", "lengthscales", "variance", "noise")}
    E, U, P, H = 2, 1, 10, 2
    x0 = np.random.RandomState(0).randn(P, E)
    mean, cov = np.empty((H + 1, E)), np.empty((H + 1, E, E))
    spec = dict(kind=_lib.POLICY_LINEAR, state_dim=E, control_dim=U, W=np.ones((U, E)), b=np.zeros(U), max_action=1.0)
    rw = [dict(kind=_lib.REWARD_EXPONENTIAL, coef=1.0, W=np.eye(E), t=None)]
    cx = _lib.Context(device=0)
    try:
        pol, k1 = cx._policy(spec)
        terms, k2 = cx._rewards(rw, E)
        assert _raw(cx, pol, terms, 1, x0, P, H, None, mean, cov) == E_STATE            # no data yet
        cx.gp_set_data(0, cfg["X"], cfg["Y"])
        cx.gp_set_hyp(0, cfg["lengthscales"], cfg["variance"], cfg["noise"])
        assert _raw(cx, pol, terms, 1, x0, P, H, None, mean, cov) == 0                  # factorises by itself
        for args in ((x0, 0, H), (x0, -3, H), (x0, P, -1), (None, P, H)):
            assert _raw(cx, pol, terms, 1, args[0], args[1], args[2], None, mean, cov) == E_SHAPE
            assert b"rollout_particles" in cx.lib.pilco_last_error(cx.h)
        assert _raw(cx, pol, terms, 1, x0, P, H, None, None, cov) == E_SHAPE
        assert _raw(cx, pol, terms, 1, x0, P, H, None, mean, None) == E_SHAPE
        assert _raw(cx, None, terms, 1, x0, P, H, None, mean, cov) == E_SHAPE
        for bad in (dict(spec, state_dim=3, W=np.ones((U, 3))), dict(spec, control_dim=2, W=np.ones((2, E)), b=np.zeros(2)),
                    dict(kind=_lib.POLICY_NONE, state_dim=E, control_dim=0)):
            bp, kb = cx._policy(bad)
            assert _raw(cx, bp, terms, 1, x0, P, H, None, mean, cov) == E_SHAPE         # dims do not match the slot
            assert b"polic" in cx.lib.pilco_last_error(cx.h)
        rp, kr = cx._policy(dict(kind=_lib.POLICY_RBF, state_dim=E, control_dim=U, max_action=1.0))
        assert _raw(cx, rp, terms, 1, x0, P, H, None, mean, cov) == E_STATE             # no policy GP in the policy slot
        cx.gp_set_data(1, np.random.RandomState(1).randn(8, 3), np.zeros((8, U)))        # a policy GP of the wrong input width
        cx.gp_set_hyp(1, np.ones((U, 3)), np.ones(U), 1e-4 * np.ones(U))
        cx.gp_factorize(1)
        assert _raw(cx, rp, terms, 1, x0, P, H, None, mean, cov) == E_SHAPE
        iK, beta = cx.gp_get_factors(0, E)
        cx.gp_set_factors(0, iK, beta)
        assert _raw(cx, pol, terms, 1, x0, P, H, None, mean, cov) == E_STATE            # factors of pilco_gp_set_factors
        cx.gp_factorize(0)
        assert _raw(cx, pol, terms, 1, x0, P, H, None, mean, cov) == 0
        assert _raw(cx, pol, terms, 1, x0, P, 0, None, mean, cov) == 0                  # H = 0: the moments of x0
        np.testing.assert_allclose(mean[0], x0.mean(0), rtol=0, atol=4 * P * U53 * np.abs(x0).max())
    finally:
        cx.close()
    sh = _lib.Context(device=0)
    try:
        sh.shard_set(0, 2)
        sh.gp_set_data(0, cfg["X"], cfg["Y"])
        sh.gp_set_hyp(0, cfg["lengthscales"], cfg["variance"], cfg["noise"])
        pol, k1 = sh._policy(spec)
        terms, k2 = sh._rewards(rw, E)
        assert _raw(sh, pol, terms, 1, x0, P, H, None, mean, cov) == E_STATE            # sharded context
        assert b"single rank" in sh.lib.pilco_last_error(sh.h)
    finally:
        sh.close()


def test_python_layer_shapes_types_and_host_reward_terms():
    from pilco_amd import rewards
    from pilco_amd.models import PILCO
    p, model, policy, _, m0, S0 = _setup("predictions")
    res = p.sample_trajectories(m0, S0, 4, num_particles=50, seed=2)
    assert res.particles is None and res.eps.shape == (4, 50, 2) and res.mean.shape == (5, 2) and res.cov.shape == (5, 2, 2)
    assert res.reward.shape == (1, 1) and res.reward_steps.shape == (4,)
    assert all(isinstance(a, np.ndarray) and a.dtype == np.float64 for a in (res.mean, res.cov, res.reward, res.reward_steps, res.eps))
    # x0 drawn on the host: m + z sqrt(s), z from default_rng(seed); the same call twice gives the same bits
    res2 = p.sample_trajectories(m0, S0, 4, num_particles=50, seed=2, return_particles=True)
    assert np.array_equal(res.mean, res2.mean) and np.array_equal(res.eps, res2.eps)
    z = np.random.default_rng(2).standard_normal((50, 2))
    np.testing.assert_allclose(res2.particles[0], m0 + z * np.sqrt(0.05), rtol=1e-14)
    # the caller's own x0 and draws
    x0 = _x0("predictions", 7, 9)
    eps = np.random.RandomState(1).randn(3, 7, 2)
    res3 = p.sample_trajectories(None, None, 3, x0=x0, eps=eps, return_particles=True)
    assert np.array_equal(res3.particles[0], x0) and np.array_equal(res3.eps, eps)
    xn, _, _, _ = pr.step(model, policy, x0, eps[0])
    np.testing.assert_allclose(res3.particles[1], xn, rtol=1e-7)
    # comparable with predict(): a tight initial state, a few steps
    Mp, Sp, Rp = p.predict(m0, 1e-4 * np.eye(2), 2)
    res4 = p.sample_trajectories(m0, 1e-4 * np.eye(2), 2, num_particles=4096, seed=3)
    assert np.abs(res4.mean[2] - np.ravel(Mp)).max() < 0.1 and abs(res4.reward[0, 0] - np.ravel(Rp)[0]) < 0.1
    with pytest.raises(ValueError):
        p.sample_trajectories(None, None, 3, x0=x0, eps=eps[:2])

    class Mine:   # a reward object of the caller's own: evaluated on the host along predict()'s trajectory
        def compute_reward(self, m, s):
            return np.array([[1.0]]), np.array([[0.0]])
    q = PILCO((model["X"], model["Y"]), controller=p.controller, reward=rewards.CombinedRewards(2, [rewards.ExponentialReward(2), Mine()]),
              ctx=_CTX)
    with pytest.raises(NotImplementedError, match="return_particles"):
        q.sample_trajectories(m0, S0, 2, num_particles=8)
