"""Policy gradients through particle rollouts on the MI355X: pilco_rollout_particles_grad / _grad_rbf (csrc/particles_grad.hip,
docs/particle_gradients.md), Context.rollout_particles_grad[_rbf], PILCO.particle_value_and_gradient and
optimize_policy(objective="particles").  The yardstick is the NumPy restatement tests/helpers/particle_grad_restatement.py,
which tests/test_particle_grad_cpu.py pins to torch autograd; the independent check is a central difference of the device's
own pilco_rollout_particles value.  Every figure a bound is held against is printed before the assertion (-s)."""
import ctypes as C
import os

import numpy as np
import pytest

from helpers import particle_grad_cases as pgc
from helpers import particle_grad_restatement as pg

pytestmark = pytest.mark.gpu
E_SHAPE, E_NOT_PD, E_STATE = 1, 2, 5
U53 = 2.0 ** -53
BUDGET = "PILCO_PARTICLE_GRAD_BUDGET"
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
    """The PILCO object of a model of helpers/particle_grad_cases.py on this module's context, with its rewards."""
    key = (name, small_rbf)
    if key in _OBJ:
        return _OBJ[key]
    from pilco_amd import controllers, rewards
    from pilco_amd.models import PILCO
    s = pgc.setup(name)
    cfg, Z, E, U = s["cfg"], s["Z"], s["E"], s["U"]
    ctl = None
    if small_rbf:       # five basis functions in place of the hundred of rbf_controller.npz: every parameter gets a difference.
        # Centres 1.5 apart: K + noise I is well conditioned (|beta| < 5), so that the central difference's own truncation
        # error, h^2 / 6 times the third derivative (1e-10 under the restatement on the CPU; 5.6e-7 with centres 0.5 apart,
        # where |beta| reaches 287), stays far below the tolerance it is held to
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
    p = PILCO((cfg["X"], cfg["Y"]), num_induced_points=None if Z is None else Z.shape[0], controller=ctl, reward=rw, ctx=_CTX)
    for i, mdl in enumerate(p.mgpr.models):
        mdl.kernel.lengthscales.assign(cfg["lengthscales"][i])
        mdl.kernel.variance.assign(cfg["variance"][i])
        mdl.likelihood.variance.assign(cfg["noise"][i])
    if Z is not None:
        for mdl in p.mgpr.models:
            mdl.inducing_variable.Z.assign(Z)
    _OBJ[key] = p
    return p


def _ready(p):
    p.mgpr._user_factors = None
    p.mgpr._ensure_factorized()


def _fwd(p, x0, H, eps=None, seed=0, obs=False, want_particles=False):
    _ready(p)
    return _CTX.rollout_particles(p._policy_spec(), p._reward_terms(), x0, H, eps=eps, seed=seed, observation_noise=obs,
                                  want_particles=want_particles)


def _grad(p, x0, H, eps=None, seed=0, obs=False):
    """-> (J, reward_steps, grads (tuple), dx0)"""
    from pilco_amd import controllers
    _ready(p)
    kw = dict(eps=eps, seed=seed, observation_noise=obs, want_dx0=True)
    ctl = p.controller
    if isinstance(ctl, controllers.RbfController):
        out = _CTX.rollout_particles_grad_rbf(p._policy_spec(), p._reward_terms(), x0, H, ctl.X, ctl.Y, ctl.lengthscales, ctl.noise, **kw)
        return out[0], out[1], tuple(out[2:5]), out[5]
    out = _CTX.rollout_particles_grad(p._policy_spec(), p._reward_terms(), x0, H, **kw)
    return out[0], out[1], (tuple(out[2:4]) if p.control_dim > 0 else ()), out[4]


def _flat(res):
    return [np.atleast_1d(res[0]), res[1]] + [np.asarray(g) for g in res[2]] + [res[3]]


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(_flat(a), _flat(b)))


# ------------------------------------------------------------------ forward bits
@pytest.mark.parametrize("given", [False, True], ids=["generated", "given"])
@pytest.mark.parametrize("name,P,H,obs", [("rbf", 129, 4, False), ("c2u", 1601, 2, True), ("fitc", 65, 3, False), ("c2", 63, 2, False)])
def test_rewards_have_the_bits_of_the_particle_rollout(name, P, H, obs, given):
    p = _obj(name)
    x0 = pgc.x0_of(name, P, 7)
    eps = np.random.RandomState(8).randn(H, P, x0.shape[1]) if given else None
    fwd = _fwd(p, x0, H, eps=eps, seed=77, obs=obs)
    J, steps, _, _ = _grad(p, x0, H, eps=eps, seed=77, obs=obs)
    assert np.array_equal(steps, fwd[2])
    total = 0.0
    for r in fwd[2]:
        total += r                       # J: the steps' rewards added in step order
    assert J == total


# ------------------------------------------------------------------ the gradient against the restatement, teacher-forced
def _floor(scale, P, params):
    """Where no step matrix enters (H <= 1) the propagated bound is exactly zero and only the float64 floor of the
    quantity's own arithmetic is left: a particle's chain (a few thousand operations of a few ulp each) within 4096 * 2^-53
    of its absolute-sum scale, and for a parameter the sum over the particles within 4 P 2^-53 more (the bound of the
    particle statistics, tests/test_gpu_particles.py).  At H >= 2 the propagated bound stands alone."""
    return ((4 * P if params else 0) + 4096) * U53 * scale


@pytest.mark.parametrize("name,P,H,obs", pgc.CASES, ids=pgc.CASE_IDS)
def test_gradient_against_the_restatement_on_the_devices_own_particles(name, P, H, obs):
    p, s = _obj(name), pgc.setup(name)
    x0 = pgc.x0_of(name, P, 100 + P)
    seed = 300 + P + H
    mean, cov, rew, parts, eps = _fwd(p, x0, H, seed=seed, obs=obs, want_particles=True)
    # the draws given for even P, generated from the seed for odd P: the same stream either way
    J, steps, grads, dx0 = _grad(p, x0, H, eps=eps if P % 2 == 0 else None, seed=seed, obs=obs)
    assert np.array_equal(steps, rew)
    ref_g, ref_x = pg.reverse(s["model"], s["policy"], s["terms"], parts, eps, obs)
    (bg, bx), (sg, sx) = pg.reverse_bound(s["model"], s["policy"], s["terms"], parts, eps, obs)
    assert len(grads) == len(ref_g)
    worst = cond = tight = 0.0
    for got, ref, b, sc, params in zip(list(grads) + [dx0], list(ref_g) + [ref_x], list(bg) + [bx], list(sg) + [sx],
                                      [True] * len(grads) + [False]):
        got, ref, b, sc = (np.asarray(a, np.float64).reshape(np.shape(ref)) for a in (got, ref, b, sc))
        err = np.abs(got - ref)
        tol = b if H >= 2 else _floor(sc, P, params)
        if H >= 2:
            cond = max(cond, float((b / np.maximum(sc, 1e-300)).max()))
            tight = max(tight, float(b.max() / np.abs(ref).max()))
        worst = max(worst, float((err / np.maximum(tol, 1e-300)).max()) if err.size else 0.0)
        assert np.all(err <= tol), (name, P, H, float(err.max()))
    print("teacher-forced gradient %s P=%d H=%d obs=%d: largest error / %s = %.3g, bound / scale = %.3g, largest bound / largest "
          "entry = %.3g" % (name, P, H, obs, "propagated bound" if H >= 2 else "float64 floor", worst, cond, tight))
    # the input conditions: a vanishing sd cannot blow the bound up, and it is small beside the gradient it checks
    assert cond <= 1e-5 and tight <= 1e-5


# ------------------------------------------------------------------ the independent check: central differences
def _central_differences(p, get, put, x0, H, eps, h=1e-5):
    u0 = get()
    g = np.empty_like(u0)
    for i in range(u0.size):
        vals = []
        for sgn in (1.0, -1.0):
            u = u0.copy()
            u[i] += sgn * h
            put(u)
            vals.append(_fwd(p, x0, H, eps=eps)[2].sum())
        g[i] = (vals[0] - vals[1]) / (2 * h)
    put(u0)
    return g


def test_linear_policy_gradient_against_central_differences():
    p = _obj("predictions")
    ctl = p.controller
    P, H = 64, 3
    x0 = pgc.x0_of("predictions", P, 1)
    eps = np.random.RandomState(2).randn(H, P, 2)
    nW = ctl.W.numpy().size

    def get():
        return np.concatenate([ctl.W.numpy().ravel(), ctl.b.numpy().ravel()])

    def put(u):
        ctl.W.assign(u[:nW].reshape(ctl.W.shape))
        ctl.b.assign(u[nW:].reshape(ctl.b.shape))

    _, _, (dW, db), _ = _grad(p, x0, H, eps=eps)
    g = np.concatenate([dW.ravel(), db.ravel()])
    fd = _central_differences(p, get, put, x0, H, eps)
    print("central differences, linear: largest |g - fd| = %.3g (max |g| = %.3g)" % (np.abs(g - fd).max(), np.abs(g).max()))
    assert np.abs(g - fd).max() <= 1e-6 * max(1.0, np.abs(g).max())


def test_rbf_policy_gradient_against_central_differences():
    p = _obj("rbf", small_rbf=True)
    ctl = p.controller
    gp = ctl._gp
    P, H = 64, 3
    x0 = pgc.x0_of("rbf", P, 1)
    eps = np.random.RandomState(2).randn(H, P, 3)
    bf, E, U = 5, 3, 2

    def get():
        return np.concatenate([np.asarray(ctl.X).ravel(), np.asarray(ctl.Y).ravel(), np.asarray(ctl.lengthscales).ravel()])

    def put(u):
        gp.set_data((u[:bf * E].reshape(bf, E), u[bf * E:bf * E + bf * U].reshape(bf, U)))
        ls = u[bf * E + bf * U:].reshape(U, E)
        for i, m in enumerate(gp.models):
            m.kernel.lengthscales.assign(ls[i])

    _, _, (dX, dY, dl), _ = _grad(p, x0, H, eps=eps)
    g = np.concatenate([dX.ravel(), dY.ravel(), dl.ravel()])
    fd = _central_differences(p, get, put, x0, H, eps)
    print("central differences, rbf: largest |g - fd| = %.3g (max |g| = %.3g)" % (np.abs(g - fd).max(), np.abs(g).max()))
    assert np.abs(g - fd).max() <= 1e-6 * max(1.0, np.abs(g).max())


# ------------------------------------------------------------------ edges
@pytest.mark.parametrize("name", ["rbf", "predictions", "c2"])
def test_horizons_zero_and_one(name):
    p, s = _obj(name), pgc.setup(name)
    x0 = pgc.x0_of(name, 65, 4)
    J, steps, grads, dx0 = _grad(p, x0, 0)
    assert J == 0.0 and steps.shape == (0,) and not dx0.any() and not any(np.any(g) for g in grads)
    J, steps, grads, dx0 = _grad(p, x0, 1, seed=3)
    assert not any(np.any(g) for g in grads)
    want = pg.reward_grad(s["terms"], x0)
    scale = np.abs(want) + 1.0
    assert np.all(np.abs(dx0 - want) <= 4096 * U53 * scale)
    assert J == _fwd(p, x0, 1, seed=3)[2][0]


# ------------------------------------------------------------------ bits
@pytest.mark.parametrize("name", ["rbf", "c2u"])
def test_same_bits_run_to_run_alone_in_a_batch_and_permuted(name):
    p = _obj(name)
    P, H = 257, 4
    x0 = pgc.x0_of(name, P, 5)
    eps = np.random.RandomState(6).randn(H, P, x0.shape[1])
    full = _grad(p, x0, H, eps=eps)
    assert _same(full, _grad(p, x0, H, eps=eps))
    for q in (0, 63, 64, 127, 128, 256):
        one = _grad(p, x0[q:q + 1], H, eps=eps[:, q:q + 1])
        assert np.array_equal(one[3][0], full[3][q]), q
    perm = np.random.RandomState(7).permutation(P)
    assert np.array_equal(_grad(p, x0[perm], H, eps=eps[:, perm])[3], full[3][perm])


def _with_budget(doubles, fn):
    old = os.environ.get(BUDGET)
    os.environ[BUDGET] = str(int(doubles))
    try:
        return fn()
    finally:
        if old is None:
            del os.environ[BUDGET]
        else:
            os.environ[BUDGET] = old


@pytest.mark.parametrize("name", ["rbf", "predictions", "c2"])
def test_groups_do_not_change_a_bit(name):
    p, s = _obj(name), pgc.setup(name)
    P, H = 385, 3
    x0 = pgc.x0_of(name, P, 9)
    per_particle = (H - 1) * s["E"] * (s["E"] + s["U"])
    one = _grad(p, x0, H, seed=11)
    for blocks in (2, 1):            # groups of 256 + 129 particles, and of 128 + 128 + 128 + 1
        assert _same(one, _with_budget(per_particle * 128 * blocks, lambda: _grad(p, x0, H, seed=11))), blocks
    assert _same(one, _with_budget(1, lambda: _grad(p, x0, H, seed=11)))      # (a budget below one block: groups of one block)


def test_chunk_boundary_does_not_change_a_bit():
    """C2u: 1600 particles per chunk.  P = 1601 runs as chunks of 1600 + 1; in groups of 1024 + 577 the chunks fall elsewhere."""
    p, s = _obj("c2u"), pgc.setup("c2u")
    P, H = 1601, 2
    x0 = pgc.x0_of("c2u", P, 12)
    one = _grad(p, x0, H, seed=13)
    assert _same(one, _with_budget((H - 1) * 10 * 11 * 1024, lambda: _grad(p, x0, H, seed=13)))
    eps = _fwd(p, x0, H, seed=13)[4]
    for q in (1599, 1600):
        assert np.array_equal(_grad(p, x0[q:q + 1], H, eps=eps[:, q:q + 1])[3][0], one[3][q]), q


# ------------------------------------------------------------------ refusals
def _raw_call(p, rbf, cx=None, **over):
    """The C entry point with every output prefilled; over: replacements of single arguments; cx: another context than this
    module's.  -> (code, outputs)"""
    from pilco_amd import _lib
    if cx is None:
        _ready(p)          # (the models of this module take turns in the context's dynamics slot)
    cx = _CTX if cx is None else cx
    ctl = p.controller
    E, U = p.state_dim, p.control_dim
    pol, k1 = cx._policy(over.pop("policy_spec", p._policy_spec()))
    terms = over.pop("terms", p._reward_terms())
    rw, k2 = cx._rewards(terms, E)
    P, H = over.pop("P", 5), over.pop("H", 2)
    x0 = np.ascontiguousarray(pgc.x0_of("rbf" if rbf else "predictions", 5, 1))
    dp = _lib._dp
    ptr = lambda a: a.ctypes.data_as(dp)   # noqa: E731
    outs = dict(reward=np.full(1, 7.0), steps=np.full(2, 7.0), dx0=np.full((5, E), 7.0))
    if rbf:
        bf = np.asarray(ctl.X).shape[0]
        Xp, Yp, lsp, nz = (np.ascontiguousarray(np.asarray(a, np.float64)) for a in (ctl.X, ctl.Y, ctl.lengthscales, np.asarray(ctl.noise).reshape(-1)))
        outs.update(dX=np.full((bf, E), 7.0), dY=np.full((bf, U), 7.0), dls=np.full((U, E), 7.0))
        a = dict(policy=C.byref(pol), rewards=rw, n_rewards=len(terms), x0=ptr(x0), P=P, H=H, eps=None, seed=C.c_ulonglong(1), obs=0,
                 Xp=ptr(Xp), Yp=ptr(Yp), lsp=ptr(lsp), noisep=ptr(nz), bf=bf, reward=ptr(outs["reward"]), steps=ptr(outs["steps"]),
                 dX=ptr(outs["dX"]), dY=ptr(outs["dY"]), dls=ptr(outs["dls"]), dx0=ptr(outs["dx0"]))
        fn = cx.lib.pilco_rollout_particles_grad_rbf
    else:
        outs.update(dW=np.full((U, E), 7.0), db=np.full(U, 7.0))
        a = dict(policy=C.byref(pol), rewards=rw, n_rewards=len(terms), x0=ptr(x0), P=P, H=H, eps=None, seed=C.c_ulonglong(1), obs=0,
                 reward=ptr(outs["reward"]), steps=ptr(outs["steps"]), dW=ptr(outs["dW"]), db=ptr(outs["db"]), dx0=ptr(outs["dx0"]))
        fn = cx.lib.pilco_rollout_particles_grad
    for k, v in over.items():
        assert k in a, k
        a[k] = v
    return fn(cx.h, *a.values()), outs


def test_refusals_leave_the_outputs_untouched_and_a_valid_call_follows():
    from pilco_amd import _lib
    lin, rbf = _obj("predictions"), _obj("rbf")
    _ready(lin)
    _ready(rbf)
    x0 = pgc.x0_of("predictions", 5, 1)
    good = _grad(lin, x0, 2, seed=1)
    bad_kind = [dict(kind=7, coef=1.0, W=np.zeros(2))]
    linear_cases = [dict(P=0), dict(P=-3), dict(H=-1), dict(x0=None), dict(reward=None), dict(dW=None), dict(db=None),
                    dict(policy=None), dict(n_rewards=5), dict(n_rewards=-1), dict(rewards=None), dict(terms=bad_kind),
                    dict(policy_spec=dict(kind=_lib.POLICY_NONE, state_dim=2, control_dim=0)),          # the model has a control input
                    dict(policy_spec=dict(kind=_lib.POLICY_LINEAR, state_dim=3, control_dim=1, W=np.zeros((1, 3)), b=np.zeros(1))),
                    dict(policy_spec=dict(kind=_lib.POLICY_RBF, state_dim=2, control_dim=1, max_action=1.0))]
    for over in linear_cases:
        code, outs = _raw_call(lin, False, **dict(over))
        assert code in (E_SHAPE, E_STATE), (over, code)
        assert all(np.all(v == 7.0) for v in outs.values()), over
    rbf_cases = [dict(P=0), dict(H=-1), dict(x0=None), dict(reward=None), dict(Xp=None), dict(Yp=None), dict(lsp=None),
                 dict(noisep=None), dict(dX=None), dict(dY=None), dict(dls=None), dict(bf=99), dict(bf=0),
                 dict(policy_spec=dict(kind=_lib.POLICY_LINEAR, state_dim=3, control_dim=2, W=np.zeros((2, 3)), b=np.zeros(2)))]
    code, outs = _raw_call(rbf, True)                        # the call itself is sound
    assert code == 0 and not np.any(outs["dX"] == 7.0), (code, _CTX.lib.pilco_last_error(_CTX.h))
    for over in rbf_cases:
        code, outs = _raw_call(rbf, True, **dict(over))
        assert code == E_SHAPE, (over, code)
        assert all(np.all(v == 7.0) for v in outs.values()), over
    # a singular K + noise I of the policy the caller describes (every centre the same, no noise): refused on the host
    bf = np.asarray(rbf.controller.X).shape[0]
    dp = _lib._dp
    same, none = np.zeros((bf, 3)), np.zeros(2)
    code, outs = _raw_call(rbf, True, Xp=same.ctypes.data_as(dp), noisep=none.ctypes.data_as(dp))
    assert code == E_NOT_PD and all(np.all(v == 7.0) for v in outs.values()), (code, _CTX.lib.pilco_last_error(_CTX.h))
    # the states pilco_rollout_particles refuses, on contexts of their own
    cfg = pgc.setup("predictions")["cfg"]
    rbf_spec = dict(kind=_lib.POLICY_RBF, state_dim=2, control_dim=1, max_action=1.0)
    cx = _lib.Context(device=0)
    try:
        code, outs = _raw_call(lin, False, cx=cx)                                         # no data yet
        assert code == E_STATE and all(np.all(v == 7.0) for v in outs.values())
        cx.gp_set_data(0, cfg["X"], cfg["Y"])
        cx.gp_set_hyp(0, cfg["lengthscales"], cfg["variance"], cfg["noise"])
        code, outs = _raw_call(lin, False, cx=cx, policy_spec=rbf_spec)                   # an RbfController, no policy GP in its slot
        assert code in (E_STATE, E_SHAPE) and all(np.all(v == 7.0) for v in outs.values())
        cx.gp_set_data(1, np.random.RandomState(1).randn(8, 2), np.zeros((8, 1)))         # ... and one that is not factorised
        cx.gp_set_hyp(1, np.ones((1, 2)), np.ones(1), 1e-4 * np.ones(1))
        one = (np.zeros((8, 2)), np.zeros((8, 1)), np.ones((1, 2)), np.ones(1))
        outs = dict(reward=np.full(1, 7.0), steps=np.full(2, 7.0), dX=np.full((8, 2), 7.0), dY=np.full((8, 1), 7.0),
                    dls=np.full((1, 2), 7.0), dx0=np.full((5, 2), 7.0))
        pol, k1 = cx._policy(rbf_spec)
        rw, k2 = cx._rewards(lin._reward_terms(), 2)
        x5 = np.ascontiguousarray(pgc.x0_of("predictions", 5, 1))
        ptr = lambda a: a.ctypes.data_as(dp)   # noqa: E731
        code = cx.lib.pilco_rollout_particles_grad_rbf(cx.h, C.byref(pol), rw, 2, ptr(x5), 5, 2, None, C.c_ulonglong(1), 0,
                                                       ptr(one[0]), ptr(one[1]), ptr(one[2]), ptr(one[3]), 8, ptr(outs["reward"]),
                                                       ptr(outs["steps"]), ptr(outs["dX"]), ptr(outs["dY"]), ptr(outs["dls"]),
                                                       ptr(outs["dx0"]))
        assert code == E_STATE and all(np.all(v == 7.0) for v in outs.values())
        code, outs = _raw_call(lin, False, cx=cx)                                         # factorises by itself
        assert code == 0
        iK, beta = cx.gp_get_factors(0, 2)
        cx.gp_set_factors(0, iK, beta)
        code, outs = _raw_call(lin, False, cx=cx)                                         # factors of pilco_gp_set_factors
        assert code == E_STATE and all(np.all(v == 7.0) for v in outs.values())
    finally:
        cx.close()
    sh = _lib.Context(device=0)
    try:
        sh.shard_set(0, 2)
        sh.gp_set_data(0, cfg["X"], cfg["Y"])
        sh.gp_set_hyp(0, cfg["lengthscales"], cfg["variance"], cfg["noise"])
        code, outs = _raw_call(lin, False, cx=sh)                                         # sharded context
        assert code == E_STATE and all(np.all(v == 7.0) for v in outs.values())
        assert b"single rank" in sh.lib.pilco_last_error(sh.h)
    finally:
        sh.close()
    code, outs = _raw_call(lin, False)                       # the call itself is sound
    assert code == 0 and not np.any(outs["dW"] == 7.0)
    assert _same(good, _grad(lin, x0, 2, seed=1))


# ------------------------------------------------------------------ PILCO and optimize_policy
def test_particle_value_and_gradient_is_the_context_call_and_refuses_host_terms():
    from pilco_amd import safe
    p = _obj("rbf")
    x0 = pgc.x0_of("rbf", 64, 3)
    r, grads, dx0 = p.particle_value_and_gradient(n=3, x0=x0, seed=4, return_dx0=True)
    raw = _grad(p, x0, 3, seed=4)
    assert r == raw[0] and all(np.array_equal(a, b) for a, b in zip(grads, raw[2])) and np.array_equal(dx0, raw[3])
    r2, g2 = p.particle_value_and_gradient(n=3, num_particles=64, seed=4)
    traj = p.sample_trajectories(p.m_init, p.S_init, 3, num_particles=64, seed=4)
    total = 0.0
    for v in traj.reward_steps:
        total += v
    assert r2 == total and len(g2) == 3
    keep = p.reward
    try:
        from pilco_amd import rewards
        p.reward = rewards.CombinedRewards(3, list(keep.base_rewards) + [safe.SingleConstraint(0, high=0.5, inside=False)])
        with pytest.raises(NotImplementedError):
            p.particle_value_and_gradient(n=2, num_particles=8)
    finally:
        p.reward = keep


def test_optimize_policy_on_the_particle_objective_does_not_lose_value():
    p = _obj("rbf")
    get, put = __import__("pilco_amd.training", fromlist=["_policy_params"])._policy_params(p.controller)
    u0 = get().copy()
    horizon = p.horizon
    try:
        p.horizon = 4
        opts = dict(num_particles=128, seed=5)
        x0 = p._initial_particles(p.m_init, p.S_init, 128, 5)
        before = p.particle_value_and_gradient(x0=x0, seed=5)[0]
        best = p.optimize_policy(maxiter=5, verbose=False, objective="particles", particle_options=opts)
        after = p.particle_value_and_gradient(x0=x0, seed=5)[0]
        print("optimize_policy(objective='particles'): particle value %.6f -> %.6f" % (before, after))
        assert after >= before and best == after
        # the default objective is untouched: with and without the argument, bit for bit
        put(u0)
        r1 = p.optimize_policy(maxiter=5, verbose=False)
        u1 = get().copy()
        put(u0)
        r2 = p.optimize_policy(maxiter=5, verbose=False, objective="moment_matching")
        assert r1 == r2 and np.array_equal(u1, get())
    finally:
        p.horizon = horizon
        put(u0)
