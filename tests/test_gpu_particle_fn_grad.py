"""Policy gradients through function-sample particle rollouts on the MI355X: pilco_rollout_particles_fn_grad / _grad_rbf
(csrc/particles_fn_grad.hip, docs/particle_fn_gradients.md), Context.rollout_particles_fn_grad[_rbf],
PILCO.particle_value_and_gradient(dynamics="function") and optimize_policy(objective="particles", dynamics="function").  The
yardstick is the NumPy restatement tests/helpers/particle_fn_grad_restatement.py, which tests/test_particle_fn_grad_cpu.py pins
to torch autograd; the independent check is a central difference of the device's own pilco_rollout_particles_fn value on
fed-back draws.  Every figure a bound is held against is printed before the assertion (-s)."""
import ctypes as C

import numpy as np
import pytest

from helpers import particle_fn_grad_cases as fgc
from helpers import particle_fn_grad_restatement as fg

pytestmark = pytest.mark.gpu
E_SHAPE, E_NOT_PD, E_STATE = 1, 2, 5
U53 = 2.0 ** -53
BUDGET, FN_BUDGET = "PILCO_PARTICLE_GRAD_BUDGET", "PILCO_PARTICLE_FN_BUDGET"
KEYS = ("omega", "phase", "w", "xi")
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


def _rbf_controller(E, U, X, Y, ls, maxact):
    from pilco_amd import controllers
    ctl = controllers.RbfController(E, U, X.shape[0], max_action=maxact, ctx=_CTX)
    ctl.set_data((X, Y))
    for i, mdl in enumerate(ctl.models):
        mdl.kernel.lengthscales.assign(ls[i])
    return ctl


def _obj(name, small_rbf=False):
    """The PILCO object of a model of helpers/particle_fn_grad_cases.py on this module's context, with its rewards."""
    key = (name, small_rbf)
    if key in _OBJ:
        return _OBJ[key]
    from pilco_amd import controllers, rewards
    from pilco_amd.models import PILCO
    s = fgc.setup(name)
    cfg, E, U = s["cfg"], s["E"], s["U"]
    ctl = None
    if small_rbf:       # five basis functions, centres 1.5 apart: every parameter gets a difference (tests/test_gpu_particle_grad.py)
        r = np.random.RandomState(31)
        ctl = _rbf_controller(E, U, s["m0"] + 1.5 * r.randn(5, E), 0.5 * r.randn(5, U), 1.0 + r.rand(U, E), s["maxact"])
    elif s["rbf"] is not None:
        ctl = _rbf_controller(E, U, s["rbf"]["X"], s["rbf"]["Y"], s["rbf"]["lengthscales"], s["maxact"])
    elif U > 0:
        ctl = controllers.LinearController(E, U, max_action=s["maxact"], ctx=_CTX)
        ctl.W.assign(s["W"])
        ctl.b.assign(s["b"])
    ex, li = s["terms"]
    rw = rewards.CombinedRewards(E, [rewards.ExponentialReward(E, W=ex["W"], t=ex["t"].reshape(1, E)), rewards.LinearReward(E, li["W"])],
                                 coefs=[ex["coef"], li["coef"]])
    p = PILCO((cfg["X"], cfg["Y"]), controller=ctl, reward=rw, ctx=_CTX)
    for i, mdl in enumerate(p.mgpr.models):
        mdl.kernel.lengthscales.assign(cfg["lengthscales"][i])
        mdl.kernel.variance.assign(cfg["variance"][i])
        mdl.likelihood.variance.assign(cfg["noise"][i])
    _OBJ[key] = p
    return p


def _ready(p):
    p.mgpr._user_factors = None
    p.mgpr._ensure_factorized()


def _feed(dr):
    return None if dr is None else {k: dr[k] for k in KEYS}


def _fwd(p, x0, H, L=64, draws=None, eps=None, seed=0, obs=False, want_particles=False, want_draws=False):
    """Context.rollout_particles_fn: (mean, cov, reward_steps, particles, eps, counts, first_hit, draws)"""
    _ready(p)
    return _CTX.rollout_particles_fn(p._policy_spec(), p._reward_terms(), x0, H, num_features=L, function_draws=_feed(draws), eps=eps,
                                     seed=seed, observation_noise=obs, want_particles=want_particles, want_draws=want_draws)


def _grad(p, x0, H, L=64, draws=None, eps=None, seed=0, obs=False, want_draws=False):
    """-> (J, reward_steps, grads (tuple), dx0, draws)"""
    from pilco_amd import controllers
    _ready(p)
    kw = dict(num_features=L, function_draws=_feed(draws), eps=eps, seed=seed, observation_noise=obs, want_dx0=True, want_draws=want_draws)
    ctl = p.controller
    if isinstance(ctl, controllers.RbfController):
        out = _CTX.rollout_particles_fn_grad_rbf(p._policy_spec(), p._reward_terms(), x0, H, ctl.X, ctl.Y, ctl.lengthscales, ctl.noise, **kw)
        return out[0], out[1], tuple(out[2:5]), out[5], out[6]
    out = _CTX.rollout_particles_fn_grad(p._policy_spec(), p._reward_terms(), x0, H, **kw)
    return out[0], out[1], (tuple(out[2:4]) if p.control_dim > 0 else ()), out[4], out[5]


def _flat(res):
    return [np.atleast_1d(res[0]), res[1]] + [np.asarray(g) for g in res[2]] + [res[3]]


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(_flat(a), _flat(b)))


def _step_order_sum(steps):
    total = 0.0
    for r in steps:
        total += r
    return total


# ------------------------------------------------------------------ 1. forward bits
@pytest.mark.parametrize("L", [1, 63, 64, 100])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 129, 257])
def test_rewards_have_the_bits_of_the_function_sample_rollout(P, L):
    p = _obj("rbf")
    x0 = fgc.x0_of("rbf", P, 7)
    for H in (0, 1, 2, 6):
        for obs in (False, True):
            seed = 77 + H
            fwd = _fwd(p, x0, H, L, seed=seed, obs=obs, want_draws=True)
            J, steps, _, _, dr = _grad(p, x0, H, L, seed=seed, obs=obs, want_draws=True)          # generated draws
            assert np.array_equal(steps, fwd[2]) and J == _step_order_sum(fwd[2]), (H, obs)
            assert all(np.array_equal(dr[k], fwd[7][k]) for k in KEYS + ("v",))
            J2, steps2, _, _, _ = _grad(p, x0, H, L, draws=dr, seed=seed, obs=obs)                 # fed back
            assert np.array_equal(steps2, fwd[2]) and J2 == J, (H, obs)
            assert np.array_equal(_fwd(p, x0, H, L, seed=seed, obs=obs)[2], fwd[2])               # the forward call after a gradient call


@pytest.mark.parametrize("name", ["predictions", "syn1", "syn65", "syn100", "w16", "w32"])
def test_rewards_have_the_forward_bits_on_every_setup(name):
    p = _obj(name)
    x0 = fgc.x0_of(name, 129, 8)
    eps = np.random.RandomState(9).randn(6, 129, x0.shape[1])
    for obs, e in ((False, None), (True, None), (True, eps)):
        fwd = _fwd(p, x0, 6, 100, eps=e, seed=5, obs=obs)
        J, steps, _, _, _ = _grad(p, x0, 6, 100, eps=e, seed=5, obs=obs)
        assert np.array_equal(steps, fwd[2]) and J == _step_order_sum(fwd[2])


# ------------------------------------------------------------------ 2. the gradient against the restatement, teacher-forced
def _tolerance(b, sc, P, params):
    """reverse_bound_fn plus the float64 floor of tests/test_gpu_particle_grad.py: a particle's chain within 4096 * 2^-53 of its
    absolute-sum scale, the sum over the particles within 4 P 2^-53 more."""
    return b + ((4 * P if params else 0) + 4096) * U53 * sc


@pytest.mark.parametrize("name,P,L,H,obs", fgc.CASES, ids=fgc.CASE_IDS)
def test_gradient_against_the_restatement_on_the_devices_own_particles(name, P, L, H, obs):
    p, s = _obj(name), fgc.setup(name)
    x0 = fgc.x0_of(name, P, 100 + P)
    seed = 300 + P + H
    fwd = _fwd(p, x0, H, L, seed=seed, obs=obs, want_particles=True, want_draws=True)
    rew, parts, dr = fwd[2], fwd[3], fwd[7]
    # the draws fed back for even P, generated from the seed for odd P: the same functions either way
    J, steps, grads, dx0, _ = _grad(p, x0, H, L, draws=dr if P % 2 == 0 else None, seed=seed, obs=obs)
    assert np.array_equal(steps, rew)
    ref_g, ref_x = fg.reverse_on(s["model"], s["policy"], s["terms"], dr, dr["v"], parts, H)
    (bg, bx), (sg, sx) = fg.reverse_bound_fn(s["model"], s["policy"], s["terms"], dr, dr["v"], parts, H)
    assert len(grads) == len(ref_g)
    worst = cond = tight = 0.0
    for got, ref, b, sc, params in zip(list(grads) + [dx0], list(ref_g) + [ref_x], list(bg) + [bx], list(sg) + [sx],
                                      [True] * len(grads) + [False]):
        got, ref, b, sc = (np.asarray(a, np.float64).reshape(np.shape(ref)) for a in (got, ref, b, sc))
        err = np.abs(got - ref)
        tol = _tolerance(b, sc, P, params)
        if H >= 1 and np.abs(ref).max() > 0:
            cond = max(cond, float((tol / np.maximum(sc, 1e-300)).max()))
            tight = max(tight, float(tol.max() / np.abs(ref).max()))
        worst = max(worst, float((err / np.maximum(tol, 1e-300)).max()) if err.size else 0.0)
        assert np.all(err <= tol), (name, P, H, float(err.max()))
    print("teacher-forced gradient %s P=%d L=%d H=%d obs=%d: largest error / tolerance = %.3g, tolerance / scale = %.3g, largest "
          "tolerance / largest entry = %.3g" % (name, P, L, H, obs, worst, cond, tight))
    # the input conditions, on the device's own particles
    assert cond <= 1e-6 and tight <= 1e-6


# ------------------------------------------------------------------ 3. the independent check: central differences
def _central_differences(p, get, put, x0, H, dr, h=1e-5):
    u0 = get()
    g = np.empty_like(u0)
    for i in range(u0.size):
        vals = []
        for sgn in (1.0, -1.0):
            u = u0.copy()
            u[i] += sgn * h
            put(u)
            vals.append(_fwd(p, x0, H, draws=dr)[2].sum())
        g[i] = (vals[0] - vals[1]) / (2 * h)
    put(u0)
    return g


def test_linear_policy_gradient_against_central_differences():
    p = _obj("predictions")
    ctl = p.controller
    P, H, L = 64, 3, 64
    x0 = fgc.x0_of("predictions", P, 1)
    nW = ctl.W.numpy().size

    def get():
        return np.concatenate([ctl.W.numpy().ravel(), ctl.b.numpy().ravel()])

    def put(u):
        ctl.W.assign(u[:nW].reshape(ctl.W.shape))
        ctl.b.assign(u[nW:].reshape(ctl.b.shape))

    _, _, (dW, db), _, dr = _grad(p, x0, H, L, seed=2, want_draws=True)
    g = np.concatenate([dW.ravel(), db.ravel()])
    fd = _central_differences(p, get, put, x0, H, dr)
    print("central differences, linear: largest |g - fd| = %.3g (max |g| = %.3g)" % (np.abs(g - fd).max(), np.abs(g).max()))
    assert np.abs(g - fd).max() <= 1e-6 * max(1.0, np.abs(g).max())


def test_rbf_policy_gradient_against_central_differences():
    p = _obj("rbf", small_rbf=True)
    ctl = p.controller
    gp = ctl._gp
    P, H, L = 64, 3, 64
    x0 = fgc.x0_of("rbf", P, 1)
    bf, E, U = 5, 3, 2

    def get():
        return np.concatenate([np.asarray(ctl.X).ravel(), np.asarray(ctl.Y).ravel(), np.asarray(ctl.lengthscales).ravel()])

    def put(u):
        gp.set_data((u[:bf * E].reshape(bf, E), u[bf * E:bf * E + bf * U].reshape(bf, U)))
        ls = u[bf * E + bf * U:].reshape(U, E)
        for i, m in enumerate(gp.models):
            m.kernel.lengthscales.assign(ls[i])

    _, _, (dX, dY, dl), _, dr = _grad(p, x0, H, L, seed=2, want_draws=True)
    g = np.concatenate([dX.ravel(), dY.ravel(), dl.ravel()])
    fd = _central_differences(p, get, put, x0, H, dr)
    print("central differences, rbf: largest |g - fd| = %.3g (max |g| = %.3g)" % (np.abs(g - fd).max(), np.abs(g).max()))
    assert np.abs(g - fd).max() <= 1e-6 * max(1.0, np.abs(g).max())


# ------------------------------------------------------------------ 4. bits
@pytest.mark.parametrize("name", ["rbf", "predictions", "w24"])
def test_same_bits_run_to_run_alone_in_a_batch_and_permuted(name):
    p = _obj(name)
    P, H, L = 129, 4, 100
    x0 = fgc.x0_of(name, P, 5)
    full = _grad(p, x0, H, L, seed=6, want_draws=True)
    dr = full[4]
    assert _same(full, _grad(p, x0, H, L, seed=6))                       # run to run
    assert _same(full, _grad(p, x0, H, L, draws=dr, seed=99))            # the generated draws and their fed-back copy
    for q in (0, 63, 64, 127, 128):
        one = _grad(p, x0[q:q + 1], H, L, draws={k: (dr[k][q:q + 1] if k in ("w", "xi") else dr[k]) for k in KEYS})
        assert np.array_equal(one[3][0], full[3][q]), q
    perm = np.random.RandomState(7).permutation(P)
    drp = {k: (dr[k][perm] if k in ("w", "xi") else dr[k]) for k in KEYS}
    assert np.array_equal(_grad(p, x0[perm], H, L, draws=drp)[3], full[3][perm])


@pytest.mark.parametrize("name,obs", [("rbf", False), ("predictions", True), ("syn65", False)])
def test_groups_do_not_change_a_bit(monkeypatch, name, obs):
    p, s = _obj(name), fgc.setup(name)
    P, H, L = 257, 3, 64
    x0 = fgc.x0_of(name, P, 9)
    per_particle = (H - 1) * s["E"] * (s["E"] + s["U"])
    one = _grad(p, x0, H, L, seed=11, obs=obs)
    monkeypatch.setenv(BUDGET, str(per_particle * 128))                   # three groups: 128 + 128 + 1
    assert _same(one, _grad(p, x0, H, L, seed=11, obs=obs))
    monkeypatch.setenv(BUDGET, str(per_particle * 256))                   # two: 256 + 1
    assert _same(one, _grad(p, x0, H, L, seed=11, obs=obs))
    monkeypatch.setenv(BUDGET, "1")                                       # below one block: groups of one block
    assert _same(one, _grad(p, x0, H, L, seed=11, obs=obs))
    monkeypatch.delenv(BUDGET)
    assert _same(one, _grad(p, x0, H, L, seed=11, obs=obs))


# ------------------------------------------------------------------ 5. horizons 0 and 1, refusals
@pytest.mark.parametrize("name", ["rbf", "predictions", "syn65"])
def test_horizons_zero_and_one(name):
    p, s = _obj(name), fgc.setup(name)
    x0 = fgc.x0_of(name, 65, 4)
    J, steps, grads, dx0, dr = _grad(p, x0, 0, want_draws=True)
    assert J == 0.0 and steps.shape == (0,) and not dx0.any() and not any(np.any(g) for g in grads)
    assert all(np.array_equal(dr[k], _fwd(p, x0, 0, want_draws=True)[7][k]) for k in KEYS + ("v",))
    J, steps, grads, dx0, _ = _grad(p, x0, 1, seed=3)
    assert not any(np.any(g) for g in grads)
    want = fg.reward_grad(s["terms"], x0)
    assert np.all(np.abs(dx0 - want) <= 4096 * U53 * (np.abs(want) + 1.0))
    assert J == _fwd(p, x0, 1, seed=3)[2][0]


def _raw_call(p, rbf, name, **over):
    """The C entry point with every output prefilled; over: replacements of single arguments.  -> (code, outputs)"""
    from pilco_amd import _lib
    _ready(p)          # (the models of this module take turns in the context's dynamics slot)
    ctl = p.controller
    E, U = p.state_dim, p.control_dim
    pol, k1 = _CTX._policy(over.pop("policy_spec", p._policy_spec()))
    terms = over.pop("terms", p._reward_terms())
    rw, k2 = _CTX._rewards(terms, E)
    x0 = np.ascontiguousarray(fgc.x0_of(name, 5, 1))
    N, D = fgc.setup(name)["model"]["X"].shape
    dp = _lib._dp
    ptr = lambda a: a.ctypes.data_as(dp)   # noqa: E731
    L = over.pop("L", 8)
    r = np.random.RandomState(3)
    own = dict(omega=r.randn(E, L if L > 0 else 1, D), phase=r.rand(E, L if L > 0 else 1), w=r.randn(5, E, L if L > 0 else 1),
               xi=r.randn(5, E, N))
    given = over.pop("given", ())
    draws = _lib.FunctionDraws()
    draws.L = L
    for k in given:
        setattr(draws, k, ptr(own[k]))
    outs = dict(reward=np.full(1, 7.0), steps=np.full(2, 7.0), dx0=np.full((5, E), 7.0), v=np.full((5, E, N), 7.0))
    dout = _lib.FunctionDrawsOut(None, None, None, None, ptr(outs["v"]))
    a = dict(policy=C.byref(pol), rewards=rw, n_rewards=len(terms), x0=ptr(x0), P=5, H=2, eps=None, seed=C.c_ulonglong(1), obs=0,
             draws=C.byref(draws), draws_out=C.byref(dout))
    if rbf:
        bf = np.asarray(ctl.X).shape[0]
        Xp, Yp, lsp, nz = (np.ascontiguousarray(np.asarray(q, np.float64)) for q in (ctl.X, ctl.Y, ctl.lengthscales, np.asarray(ctl.noise).reshape(-1)))
        outs.update(dX=np.full((bf, E), 7.0), dY=np.full((bf, U), 7.0), dls=np.full((U, E), 7.0))
        a.update(Xp=ptr(Xp), Yp=ptr(Yp), lsp=ptr(lsp), noisep=ptr(nz), bf=bf, reward=ptr(outs["reward"]), steps=ptr(outs["steps"]),
                 dX=ptr(outs["dX"]), dY=ptr(outs["dY"]), dls=ptr(outs["dls"]), dx0=ptr(outs["dx0"]))
        fn = _CTX.lib.pilco_rollout_particles_fn_grad_rbf
    else:
        outs.update(dW=np.full((U, E), 7.0), db=np.full(U, 7.0))
        a.update(reward=ptr(outs["reward"]), steps=ptr(outs["steps"]), dW=ptr(outs["dW"]), db=ptr(outs["db"]), dx0=ptr(outs["dx0"]))
        fn = _CTX.lib.pilco_rollout_particles_fn_grad
    for k, v in over.items():
        assert k in a, k
        a[k] = v
    return fn(_CTX.h, *a.values()), outs


def test_refusals_leave_the_outputs_untouched_and_a_valid_call_follows(monkeypatch):
    from pilco_amd import _lib
    lin, rbf = _obj("predictions"), _obj("rbf")
    x0 = fgc.x0_of("predictions", 5, 1)
    good = _grad(lin, x0, 2, 8, seed=1)
    untouched = lambda outs: all(np.all(v == 7.0) for v in outs.values())   # noqa: E731
    bad_kind = [dict(kind=7, coef=1.0, W=np.zeros(2))]
    # what pilco_rollout_particles_grad refuses ...
    linear_cases = [dict(P=0), dict(P=-3), dict(H=-1), dict(x0=None), dict(reward=None), dict(dW=None), dict(db=None),
                    dict(policy=None), dict(n_rewards=5), dict(n_rewards=-1), dict(rewards=None), dict(terms=bad_kind),
                    dict(policy_spec=dict(kind=_lib.POLICY_NONE, state_dim=2, control_dim=0)),
                    dict(policy_spec=dict(kind=_lib.POLICY_LINEAR, state_dim=3, control_dim=1, W=np.zeros((1, 3)), b=np.zeros(1))),
                    dict(policy_spec=dict(kind=_lib.POLICY_RBF, state_dim=2, control_dim=1, max_action=1.0)),
                    # ... and what pilco_rollout_particles_fn refuses about the draws
                    dict(draws=None), dict(L=0), dict(L=4097), dict(given=("omega",)), dict(given=("omega", "phase", "w"))]
    for over in linear_cases:
        code, outs = _raw_call(lin, False, "predictions", **dict(over))
        assert code in (E_SHAPE, E_STATE), (over, code)
        assert untouched(outs), over
    monkeypatch.setenv(FN_BUDGET, "64")                     # E Ppad (Lpad + 2 npad) doubles do not fit
    code, outs = _raw_call(lin, False, "predictions")
    assert code == E_SHAPE and untouched(outs) and b"PILCO_PARTICLE_FN_BUDGET" in _CTX.lib.pilco_last_error(_CTX.h)
    monkeypatch.delenv(FN_BUDGET)
    rbf_cases = [dict(P=0), dict(H=-1), dict(x0=None), dict(reward=None), dict(Xp=None), dict(Yp=None), dict(lsp=None),
                 dict(noisep=None), dict(dX=None), dict(dY=None), dict(dls=None), dict(bf=99), dict(bf=0), dict(draws=None), dict(L=0),
                 dict(given=("w", "xi")),
                 dict(policy_spec=dict(kind=_lib.POLICY_LINEAR, state_dim=3, control_dim=2, W=np.zeros((2, 3)), b=np.zeros(2)))]
    code, outs = _raw_call(rbf, True, "rbf")                 # the call itself is sound, with generated ...
    assert code == 0 and not np.any(outs["dX"] == 7.0) and not np.any(outs["v"] == 7.0), (code, _CTX.lib.pilco_last_error(_CTX.h))
    code, outs = _raw_call(rbf, True, "rbf", given=KEYS)    # ... and with given draws
    assert code == 0 and not np.any(outs["dX"] == 7.0), (code, _CTX.lib.pilco_last_error(_CTX.h))
    for over in rbf_cases:
        code, outs = _raw_call(rbf, True, "rbf", **dict(over))
        assert code == E_SHAPE, (over, code)
        assert untouched(outs), over
    bf = np.asarray(rbf.controller.X).shape[0]
    same, none = np.zeros((bf, 3)), np.zeros(2)
    code, outs = _raw_call(rbf, True, "rbf", Xp=same.ctypes.data_as(_lib._dp), noisep=none.ctypes.data_as(_lib._dp))
    assert code == E_NOT_PD and untouched(outs), (code, _CTX.lib.pilco_last_error(_CTX.h))
    # a sparse slot: function samples need an exact GP
    cfg = fgc.setup("predictions")["cfg"]
    cx = _lib.Context(device=0)
    try:
        cx.gp_set_data(0, cfg["X"], cfg["Y"])
        cx.gp_set_hyp(0, cfg["lengthscales"], cfg["variance"], cfg["noise"])
        cx.gp_set_inducing(0, cfg["X"][:10])
        pol, k1 = cx._policy(lin._policy_spec())
        rw, k2 = cx._rewards(lin._reward_terms(), 2)
        x5 = np.ascontiguousarray(x0)
        ptr = lambda a: a.ctypes.data_as(_lib._dp)   # noqa: E731
        outs = dict(reward=np.full(1, 7.0), steps=np.full(2, 7.0), dW=np.full((1, 2), 7.0), db=np.full(1, 7.0), dx0=np.full((5, 2), 7.0))
        draws = _lib.FunctionDraws()
        draws.L = 8
        code = cx.lib.pilco_rollout_particles_fn_grad(cx.h, C.byref(pol), rw, 2, ptr(x5), 5, 2, None, C.c_ulonglong(1), 0, C.byref(draws),
                                                      None, ptr(outs["reward"]), ptr(outs["steps"]), ptr(outs["dW"]), ptr(outs["db"]),
                                                      ptr(outs["dx0"]))
        assert code == E_STATE and untouched(outs), (code, cx.lib.pilco_last_error(cx.h))
    finally:
        cx.close()
    code, outs = _raw_call(lin, False, "predictions")        # the call itself is sound
    assert code == 0 and not np.any(outs["dW"] == 7.0)
    assert _same(good, _grad(lin, x0, 2, 8, seed=1))


# ------------------------------------------------------------------ 6. routing
def test_default_arguments_are_the_marginal_path_and_function_routes_to_the_new_entry_points():
    p = _obj("rbf")
    ctl = p.controller
    x0 = fgc.x0_of("rbf", 64, 3)
    r, grads, dx0 = p.particle_value_and_gradient(n=3, x0=x0, seed=4, return_dx0=True)
    _ready(p)
    raw = _CTX.rollout_particles_grad_rbf(p._policy_spec(), p._reward_terms(), x0, 3, ctl.X, ctl.Y, ctl.lengthscales, ctl.noise, seed=4,
                                          want_dx0=True)
    assert r == raw[0] and all(np.array_equal(a, b) for a, b in zip(grads, raw[2:5])) and np.array_equal(dx0, raw[5])
    r2, g2 = p.particle_value_and_gradient(n=3, x0=x0, seed=4, dynamics="marginal")
    assert r2 == r and all(np.array_equal(a, b) for a, b in zip(g2, grads))
    traj = p.sample_trajectories(p.m_init, p.S_init, 3, x0=x0, seed=4, return_particles=True, dynamics="function", num_features=100)
    rf_, gf, dxf = p.particle_value_and_gradient(n=3, x0=x0, seed=4, return_dx0=True, dynamics="function",
                                                 function_draws=traj.function_draws)
    assert rf_ == _step_order_sum(traj.reward_steps) and len(gf) == 3
    fed = _grad(p, x0, 3, draws=traj.function_draws, seed=4)
    assert rf_ == fed[0] and all(np.array_equal(a, b) for a, b in zip(gf, fed[2])) and np.array_equal(dxf, fed[3])
    rg, gg = p.particle_value_and_gradient(n=3, x0=x0, seed=4, dynamics="function", num_features=100)   # the draws of the seed
    assert rg == rf_ and all(np.array_equal(a, b) for a, b in zip(gg, gf))
    for name in ("predictions", "syn65"):          # LinearController and no controller
        q = _obj(name)
        xq = fgc.x0_of(name, 65, 3)
        rq, gq = q.particle_value_and_gradient(n=2, x0=xq, seed=5, dynamics="function", num_features=63)
        fed = _grad(q, xq, 2, 63, seed=5)
        assert rq == fed[0] and len(gq) == len(fed[2]) and all(np.array_equal(a.reshape(b.shape), b) for a, b in zip(gq, fed[2]))


# ------------------------------------------------------------------ 7. the optimiser
def test_optimize_policy_on_function_samples_does_not_lose_value_and_repeats_bit_for_bit():
    p = _obj("rbf")
    get, put = __import__("pilco_amd.training", fromlist=["_policy_params"])._policy_params(p.controller)
    u0 = get().copy()
    horizon = p.horizon
    try:
        p.horizon = 4
        put(u0)          # (both runs start from the parameters put(get()) leaves: the softplus round trip is not the identity)
        opts = dict(dynamics="function", num_features=64, num_particles=128)
        x0 = p._initial_particles(p.m_init, p.S_init, 128, 0)
        before = p.particle_value_and_gradient(x0=x0, seed=0, dynamics="function", num_features=64)[0]
        best = p.optimize_policy(maxiter=5, verbose=False, objective="particles", particle_options=opts)
        after = p.particle_value_and_gradient(x0=x0, seed=0, dynamics="function", num_features=64)[0]
        u1 = get().copy()
        print("optimize_policy(objective='particles', dynamics='function'): particle value %.6f -> %.6f" % (before, after))
        assert after >= before and best == after
        put(u0)
        best2 = p.optimize_policy(maxiter=5, verbose=False, objective="particles", particle_options=opts)
        assert best2 == best and np.array_equal(u1, get())
    finally:
        p.horizon = horizon
        put(u0)
