"""GP posterior prediction at deterministic test inputs on the MI355X: GPModelView.predict_f / predict_y (gpflow's
GPR / GPRFITC calls the reference's troubleshooting notebook makes by hand), MGPR / SMGPR.predict_f / predict_y, and the C
entry point under them, pilco_gp_predict_points (csrc/predict.hip).  The yardstick is the NumPy
float64 restatement of GPflow's predict_f in tests/helpers/predict_restatement.py, which tests/test_predict_points_cpu.py
pins to the executed reference."""
import ctypes as C
import os

import numpy as np
import pytest

from helpers.predict_restatement import fitc_predict_f, gpr_predict_f
from pilco_amd import synthetic

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
E_SHAPE, E_STATE = 1, 5
_CTX = None


def _g(name):
    return np.load(os.path.join(GOLDEN, name))


def _set_hyp(model, cfg):
    for i, mdl in enumerate(model.models):
        mdl.kernel.lengthscales.assign(cfg["lengthscales"][i])
        mdl.kernel.variance.assign(cfg["variance"][i])
        mdl.likelihood.variance.assign(cfg["noise"][i])
    return model


@pytest.fixture(scope="module", autouse=True)
def own_ctx():
    """The models of this module live on a context of their own (closed at the end), not on the process-wide default."""
    from pilco_amd import _lib
    global _CTX
    _CTX = _lib.Context(device=0)
    yield _CTX
    _CTX.close()


def _mgpr(cfg):
    from pilco_amd.models import MGPR
    return _set_hyp(MGPR((cfg["X"], cfg["Y"]), ctx=_CTX), cfg)


def _smgpr(cfg, Zs):
    from pilco_amd.models import SMGPR
    m = _set_hyp(SMGPR((cfg["X"], cfg["Y"]), num_induced_points=Zs[0].shape[0], ctx=_CTX), cfg)
    for mdl, Z in zip(m.models, Zs):
        mdl.inducing_variable.Z.assign(Z)
    return m


def _inputs(X, n, seed):
    rs = np.random.RandomState(seed)
    lo, hi = X.min(0), X.max(0)
    return lo + (hi - lo) * rs.rand(n, X.shape[1])


def _check(mean, var, ref_mean, ref_var, sf2):
    """mean, var (Nt, E) against the restatement's (E, Nt): mean within 1e-8 of max|mean|, variance within 1e-8 sf2."""
    mean, var = np.asarray(mean).T, np.asarray(var).T
    assert mean.shape == ref_mean.shape and var.shape == ref_var.shape
    for e in range(ref_mean.shape[0]):
        assert np.abs(mean[e] - ref_mean[e]).max() <= 1e-8 * np.abs(ref_mean[e]).max(), e
        assert np.abs(var[e] - ref_var[e]).max() <= 1e-8 * sf2[e], e


def _cfg_golden(name):
    g = _g(name)
    return {k: g[k] for k in ("X", "Y", "lengthscales", "variance", "noise")}


C2 = dict(N=1000, D=10, E=10)


@pytest.mark.parametrize("which", ["predictions", "c2"])
@pytest.mark.parametrize("Nt", [1, 63, 1000, 4097])
def test_exact_gp_predict_f_matches_the_restatement(which, Nt):
    cfg = _cfg_golden("predictions.npz") if which == "predictions" else synthetic.config_c2(**C2)
    m = _mgpr(cfg)
    xs = _inputs(cfg["X"], Nt, 7 + Nt)
    rm, rv = gpr_predict_f(cfg["X"], cfg["Y"], cfg["lengthscales"], cfg["variance"], cfg["noise"], xs)
    mean, var = m.predict_f(xs)
    assert mean.shape == (Nt, cfg["Y"].shape[1]) and hasattr(mean, "numpy")
    _check(mean, var, rm, rv, cfg["variance"])
    for i, mdl in enumerate(m.models):   # GPModelView.predict_f: output i alone, (Nt, 1)
        mi, vi = mdl.predict_f(xs)
        assert mi.shape == (Nt, 1) and vi.shape == (Nt, 1)
        _check(mi, vi, rm[i:i + 1], rv[i:i + 1], cfg["variance"][i:i + 1])


def _own_z(M, D, E, seed, first=None):
    rs = np.random.RandomState(seed)
    Zs = [rs.rand(M, D) for _ in range(E)]
    if first is not None:
        Zs[0] = first
    return Zs


@pytest.mark.parametrize("which", ["sparse_predictions", "c4"])
def test_fitc_predict_f_with_every_outputs_own_z(which):
    if which == "c4":
        cfg = synthetic.config_c4(N=5000, M=200)
        Zs = _own_z(200, 10, 10, 3, cfg["Z"])
    else:
        g = _g("sparse_predictions.npz")
        cfg = _cfg_golden("sparse_predictions.npz")
        Zs = _own_z(g["Z"].shape[0], 3, 2, 4, g["Z"])
    m = _smgpr(cfg, Zs)
    for Nt in (1, 63, 1000):
        xs = _inputs(cfg["X"], Nt, 11 + Nt)
        rm, rv = fitc_predict_f(cfg["X"], cfg["Y"], np.stack(Zs), cfg["lengthscales"], cfg["variance"], cfg["noise"], xs)
        mean, var = m.predict_f(xs)
        _check(mean, var, rm, rv, cfg["variance"])
        for i, mdl in enumerate(m.models):   # each with its OWN Z, not model 0's
            mi, vi = mdl.predict_f(xs)
            _check(mi, vi, rm[i:i + 1], rv[i:i + 1], cfg["variance"][i:i + 1])
    # ... and not what model 0's Z gives (the slot's factorisation, used by the rollout)
    xs = _inputs(cfg["X"], 50, 1)
    shared_m, _ = fitc_predict_f(cfg["X"], cfg["Y"], Zs[0], cfg["lengthscales"], cfg["variance"], cfg["noise"], xs)
    mean1, _ = m.models[1].predict_f(xs)
    assert np.abs(np.asarray(mean1)[:, 0] - shared_m[1]).max() > 1e-6 * np.abs(shared_m[1]).max()


@pytest.mark.parametrize("kind", ["exact", "sparse"])
def test_single_points_agree_with_predict_on_noisy_inputs_at_zero_variance(kind):
    if kind == "exact":
        cfg = _cfg_golden("predictions.npz")
        m = _mgpr(cfg)
    else:
        g = _g("sparse_predictions.npz")
        cfg = _cfg_golden("sparse_predictions.npz")
        m = _smgpr(cfg, [g["Z"]] * 2)   # every model on model 0's Z: the moment matching's model
    D = cfg["X"].shape[1]
    for x in _inputs(cfg["X"], 5, 2):
        M, S, _ = m.predict_on_noisy_inputs(x.reshape(1, D), np.zeros((D, D)))
        mean, var = m.predict_f(x.reshape(1, D))
        scale = np.maximum(cfg["variance"], np.asarray(M).ravel() ** 2)
        assert np.all(np.abs(np.asarray(mean).ravel() - np.asarray(M).ravel()) <= 1e-8 * scale)
        assert np.all(np.abs(np.asarray(var).ravel() - np.diag(S)) <= 1e-8 * scale)


def test_low_noise_variance_against_40_digit_truth():
    import mpmath as mp
    from oracle.mp_truth import factorize
    cfg = _cfg_golden("predictions_lownoise.npz")
    X, ls, sf2 = cfg["X"], cfg["lengthscales"], cfg["variance"]
    xs = _inputs(X, 8, 9)
    iKs, _ = factorize(X, cfg["Y"], ls, sf2, cfg["noise"])
    truth = np.empty((len(sf2), len(xs)))
    f = mp.mpf
    for e in range(len(sf2)):
        for t, x in enumerate(xs):
            k = mp.matrix([f(sf2[e]) * mp.exp(-sum(((f(X[i, d]) - f(x[d])) / f(ls[e, d])) ** 2 for d in range(X.shape[1])) / 2)
                           for i in range(X.shape[0])])
            truth[e, t] = float(f(sf2[e]) - (k.T * iKs[e] * k)[0])
    _, v_np = gpr_predict_f(X, cfg["Y"], ls, sf2, cfg["noise"], xs)
    _, v_gpu = _mgpr(cfg).predict_f(xs)
    v_gpu = np.asarray(v_gpu).T           # (no clamping of negative variances: GPflow does none)
    for e in range(len(sf2)):
        err_np = np.abs(v_np[e] - truth[e]).max()
        err_gpu = np.abs(v_gpu[e] - truth[e]).max()
        assert err_gpu <= 10 * err_np + 1e-14 * sf2[e], (e, err_gpu, err_np)


def test_troubleshooting_notebook_cell_predict_y_after_optimize_models():
    """examples/Hyperparameter setting and troubleshooting tips.ipynb, 'Check the one-step predictions manually'."""
    from pilco_amd.models import PILCO
    c = synthetic.config_cascade()
    pilco = PILCO((c["X"], c["Y"]), horizon=5)
    pilco.optimize_models(verbose=False)
    X_new = _inputs(c["X"], 25, 4)
    for i, m in enumerate(pilco.mgpr.models):
        y_pred_test, var_pred_test = m.predict_y(X_new)
        f_mean, f_var = m.predict_f(X_new)
        assert y_pred_test.shape == (25, 1) and var_pred_test.shape == (25, 1)
        np.testing.assert_array_equal(y_pred_test, f_mean)
        np.testing.assert_allclose(np.asarray(var_pred_test) - np.asarray(f_var), float(m.likelihood.variance.numpy()), rtol=1e-9)
    with pytest.raises(NotImplementedError):
        pilco.mgpr.models[0].predict_f(X_new, full_cov=True)
    mean, var = pilco.mgpr.predict_y(X_new)
    assert mean.shape == (25, 2) and var.shape == (25, 2)


def _ctx_model(cfg, Z=None):
    from pilco_amd import _lib
    cx = _lib.Context(device=0)
    cx.gp_set_data(0, cfg["X"], cfg["Y"])
    cx.gp_set_hyp(0, cfg["lengthscales"], cfg["variance"], cfg["noise"])
    if Z is not None:
        cx.gp_set_inducing(0, Z)
    cx.gp_factorize(0)
    return cx


def test_bit_identity_alone_batched_run_to_run_and_large_nt():
    cfg = synthetic.config_c2(**C2)
    D, E = 10, 10
    cx = _ctx_model(cfg)
    try:
        xs = _inputs(cfg["X"], 5000, 21)
        mean, var = cx.gp_predict_points(0, xs, D, E)
        m2, v2 = cx.gp_predict_points(0, xs, D, E)
        assert np.array_equal(mean, m2) and np.array_equal(var, v2)                       # run to run
        for t in (0, 1, 1599, 1600, 3199, 3200, 4999):                                    # alone = in the batch, at chunk boundaries
            ma, va = cx.gp_predict_points(0, xs[t:t + 1], D, E)
            assert np.array_equal(ma[:, 0], mean[:, t]) and np.array_equal(va[:, 0], var[:, t]), t
        for e in (0, 7):                                                                  # one output: other chunking, same bits
            me, ve = cx.gp_predict_points(0, xs, D, E, output=e)
            assert np.array_equal(me[0], mean[e]) and np.array_equal(ve[0], var[e])
        big = np.concatenate([_inputs(cfg["X"], 95000, 22), xs])                         # Nt = 100 000 at N = 1000
        mb, vb = cx.gp_predict_points(0, big, D, E)
        assert np.array_equal(mb[:, 95000:], mean) and np.array_equal(vb[:, 95000:], var)
    finally:
        cx.close()


def test_bit_identity_of_rollouts_and_objectives_around_predictions():
    from pilco_amd import _lib
    E, U = 4, 1
    c = synthetic.config_c2(N=300, D=E + U, E=E, noise=1e-2, seed=11, control_dim=U)
    D = E + U
    pol = dict(kind=_lib.POLICY_LINEAR, state_dim=E, control_dim=U, W=c["W"], b=c["b"].ravel(), max_action=1.3, squash=True)
    rw = [dict(kind=_lib.REWARD_EXPONENTIAL, coef=1.0, W=np.eye(E), t=np.zeros(E))]
    m0, S0 = c["m0"], 0.05 * np.eye(E)
    xs = _inputs(c["X"], 300, 5)
    same = lambda a, b: all(np.array_equal(x, y) for x, y in zip(a, b))
    # exact GP: rollout, predictions, rollout; nlml -> predictions give the same bits
    cx = _ctx_model(c)
    try:
        r0 = cx.rollout(pol, rw, m0, S0, 5)
        p0 = cx.gp_predict_points(0, xs, D, E)
        assert same(r0, cx.rollout(pol, rw, m0, S0, 5))
        cx.gp_nlml(0, D, E)
        assert same(p0, cx.gp_predict_points(0, xs, D, E))
        assert same(r0, cx.rollout(pol, rw, m0, S0, 5))
    finally:
        cx.close()
    # sparse, per-output Z: predictions leave the slot's factorisation alone; fitc_nlml -> predict -> rollout as before
    Z = np.random.RandomState(2).rand(40, D)
    Z_all = np.stack([Z] + _own_z(40, D, E - 1, 6))
    cx = _ctx_model(c, Z)
    try:
        r0 = cx.rollout(pol, rw, m0, S0, 5)
        ps = cx.gp_predict_points(0, xs, D, E)
        pz = cx.gp_predict_points(0, xs, D, E, Z_all=Z_all)
        assert same(r0, cx.rollout(pol, rw, m0, S0, 5))
        assert same(ps, cx.gp_predict_points(0, xs, D, E))
        cx.gp_fitc_nlml(0, Z_all, D, E)
        assert same(pz, cx.gp_predict_points(0, xs, D, E, Z_all=Z_all))
        assert same(r0, cx.rollout(pol, rw, m0, S0, 5))
        assert same(ps, cx.gp_predict_points(0, xs, D, E))
    finally:
        cx.close()


def _raw(cx, slot, Xs, Nt, output, Z_all, mean, var):
    p = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    return cx.lib.pilco_gp_predict_points(cx.h, slot, p(Xs), Nt, output, p(Z_all), p(mean), p(var))


def test_contract_errors_and_stale_models():
    from pilco_amd import _lib
    cfg = _cfg_golden("predictions.npz")
    D, E = 3, 2
    xs = _inputs(cfg["X"], 10, 3)
    out = np.empty((E, 10))
    cx = _ctx_model(cfg)
    try:
        assert _raw(cx, 0, xs, 10, -1, None, out, out.copy()) == 0
        assert _raw(cx, 0, xs, 0, -1, None, out, out.copy()) == E_SHAPE
        assert _raw(cx, 0, None, 10, -1, None, out, out.copy()) == E_SHAPE
        assert _raw(cx, 0, xs, 10, -1, None, None, out) == E_SHAPE
        assert _raw(cx, 0, xs, 10, E, None, out, out.copy()) == E_SHAPE
        assert _raw(cx, 0, xs, 10, -2, None, out, out.copy()) == E_SHAPE
        assert _raw(cx, 0, xs, 10, -1, np.zeros((E, 5, D)), out, out.copy()) == E_SHAPE   # Z_all on an exact slot
        iK, beta = cx.gp_get_factors(0, E)
        cx.gp_set_factors(0, iK, beta)
        assert _raw(cx, 0, xs, 10, -1, None, out, out.copy()) == E_STATE                 # factors of pilco_gp_set_factors
        cx.gp_factorize(0)
        assert _raw(cx, 0, xs, 10, -1, None, out, out.copy()) == 0
    finally:
        cx.close()
    sh = _lib.Context(device=0)
    try:
        sh.shard_set(0, 2)
        sh.gp_set_data(0, cfg["X"], cfg["Y"])
        sh.gp_set_hyp(0, cfg["lengthscales"], cfg["variance"], cfg["noise"])
        assert _raw(sh, 0, xs, 10, -1, None, out, out.copy()) == E_STATE                 # sharded context
    finally:
        sh.close()
    # a stale model: set_data / a hyper-parameter assign between predictions give the new model's answer
    m = _mgpr(cfg)
    m.predict_f(xs)
    X2, Y2 = cfg["X"][:70], cfg["Y"][:70]
    m.set_data((X2, Y2))
    rm, rv = gpr_predict_f(X2, Y2, cfg["lengthscales"], cfg["variance"], cfg["noise"], xs)
    _check(*m.predict_f(xs), rm, rv, cfg["variance"])
    m.models[1].kernel.lengthscales.assign(cfg["lengthscales"][1] * 1.3)
    ls = cfg["lengthscales"].copy()
    ls[1] *= 1.3
    rm, rv = gpr_predict_f(X2, Y2, ls, cfg["variance"], cfg["noise"], xs)
    _check(*m.predict_f(xs), rm, rv, cfg["variance"])
