"""Input Jacobians of the GP posterior on the MI355X: pilco_gp_predict_points_jac (csrc/predict_jac.hip, DESIGN.md section
12, docs/predict_jacobians.md), MGPR / SMGPR / GPModelView.predict_f_jacobian and PILCO.linearize on top.  The yardstick is
tests/helpers/predict_jac_restatement.py (NumPy / SciPy Cholesky factors and triangular solves),
pinned in tests/test_predict_jac_cpu.py.  Bounds, per output e (the predict_f tolerances carried to a derivative's scale):
  |d dmean_e| <= 1e-8 max_{t,d} |dmean_e|,    |d dvar_e| <= 1e-8 sf2_e / min_d l_ed.
Every measured figure is printed before it is asserted (pytest -s); docs/predict_jacobians.md quotes them."""
import ctypes as C
import os

import numpy as np
import pytest

from helpers import predict_jac_restatement as jr
from pilco_amd import synthetic

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
E_SHAPE, E_STATE = 1, 5
TOL = 1e-8
_CTX = None


def _g(name):
    g = np.load(os.path.join(GOLDEN, name))
    return {k: g[k] for k in g.files if k != "provenance"}


@pytest.fixture(scope="module", autouse=True)
def own_ctx():
    from pilco_amd import _lib
    global _CTX
    _CTX = _lib.Context(device=0)
    yield _CTX
    _CTX.close()


def _set_hyp(model, cfg):
    for i, mdl in enumerate(model.models):
        mdl.kernel.lengthscales.assign(cfg["lengthscales"][i])
        mdl.kernel.variance.assign(cfg["variance"][i])
        mdl.likelihood.variance.assign(cfg["noise"][i])
    return model


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


def _model(N, D, E, seed):
    """A smooth random model of any shape: inputs in the unit cube, lengthscales of the order of sqrt(D)."""
    rs = np.random.RandomState(seed)
    X = rs.rand(N, D)
    Y = np.sin(X @ rs.randn(D, E)) + 0.1 * rs.randn(N, E)
    return dict(X=X, Y=Y, lengthscales=np.sqrt(D) * (0.4 + 0.6 * rs.rand(E, D)), variance=0.5 + rs.rand(E),
                noise=np.full(E, 1e-2))


def _restated(cfg, xs, Z=None):
    args = (cfg["lengthscales"], cfg["variance"], cfg["noise"], xs)
    if Z is None:
        return jr.gpr_predict_f_jac(cfg["X"], cfg["Y"], *args)
    return jr.fitc_predict_f_jac(cfg["X"], cfg["Y"], Z, *args)


def _check_jac(what, dmean, dvar, ref_dmean, ref_dvar, cfg, outputs=None):
    """dmean, dvar (Nt, E', D) of the device against the restatement's (E', Nt, D), per output"""
    dmean, dvar = np.asarray(dmean).transpose(1, 0, 2), np.asarray(dvar).transpose(1, 0, 2)
    assert dmean.shape == ref_dmean.shape and dvar.shape == ref_dvar.shape, (what, dmean.shape, ref_dmean.shape)
    outputs = range(ref_dmean.shape[0]) if outputs is None else outputs
    worst_m = worst_v = 0.0
    bad = []
    for j, e in enumerate(outputs):
        sm = np.abs(ref_dmean[j]).max()
        sv = cfg["variance"][e] / np.min(cfg["lengthscales"][e])
        em, ev = np.abs(dmean[j] - ref_dmean[j]).max() / sm, np.abs(dvar[j] - ref_dvar[j]).max() / sv
        worst_m, worst_v = max(worst_m, em), max(worst_v, ev)
        if not (em <= TOL and ev <= TOL):
            bad.append((e, em, ev))
    print("FIGURE %-44s dmean %.2e  dvar %.2e  (bound %.0e)" % (what, worst_m, worst_v, TOL))
    assert not bad, (what, bad)


def _same_values(m, xs, mean, var):
    mf, vf = m.predict_f(xs)
    assert np.array_equal(np.asarray(mean), np.asarray(mf)) and np.array_equal(np.asarray(var), np.asarray(vf))


NTS = (1, 31, 32, 33, 63, 64, 65)


@pytest.mark.parametrize("N", [15, 16, 17, 63, 64, 65, 100, 257])
def test_exact_gp_at_every_edge_of_the_point_count_and_the_batch(N):
    cfg = _model(N, 3, 2, 100 + N)
    m = _mgpr(cfg)
    xs = _inputs(cfg["X"], 65, N)
    _, _, rdm, rdv = _restated(cfg, xs)
    for Nt in NTS:   # (a point's results do not depend on the batch: the restatement of the 65 serves every prefix)
        mean, var, dmean, dvar = m.predict_f_jacobian(xs[:Nt])
        assert mean.shape == (Nt, 2) and var.shape == (Nt, 2) and dmean.shape == (Nt, 2, 3) and dvar.shape == (Nt, 2, 3)
        _same_values(m, xs[:Nt], mean, var)
        _check_jac("exact N=%d Nt=%d" % (N, Nt), dmean, dvar, rdm[:, :Nt], rdv[:, :Nt], cfg)


# the mean unit takes four input dimensions per pass: D at both sides of its block edges, D = 1, and 31, 32 (the slot's largest)
@pytest.mark.parametrize("D,E", [(1, 2), (3, 2), (4, 2), (5, 2), (8, 2), (9, 2), (31, 2), (32, 2), (5, 1), (5, 10)])
def test_exact_gp_at_every_input_width_and_output_count(D, E):
    cfg = _model(100, D, E, 7 * D + E)
    m = _mgpr(cfg)
    xs = _inputs(cfg["X"], 33, D)
    _, _, rdm, rdv = _restated(cfg, xs)
    mean, var, dmean, dvar = m.predict_f_jacobian(xs)
    _same_values(m, xs, mean, var)
    _check_jac("exact D=%d E=%d" % (D, E), dmean, dvar, rdm, rdv, cfg)
    for i in (0, E - 1):   # the per-output view: (Nt, 1), (Nt, 1, D), the same bits
        mi, vi, dmi, dvi = m.models[i].predict_f_jacobian(xs)
        assert mi.shape == (33, 1) and dmi.shape == (33, 1, D)
        assert np.array_equal(np.asarray(dmi)[:, 0], np.asarray(dmean)[:, i]) and np.array_equal(np.asarray(dvi)[:, 0], np.asarray(dvar)[:, i])
        assert np.array_equal(np.asarray(mi)[:, 0], np.asarray(mean)[:, i]) and np.array_equal(np.asarray(vi)[:, 0], np.asarray(var)[:, i])


def test_golden_models_against_the_restatement():
    for name in ("predictions.npz",):
        cfg = _g(name)
        m = _mgpr(cfg)
        xs = _inputs(cfg["X"], 65, 7)
        _, _, rdm, rdv = _restated(cfg, xs)
        mean, var, dmean, dvar = m.predict_f_jacobian(xs)
        _same_values(m, xs, mean, var)
        _check_jac(name, dmean, dvar, rdm, rdv, cfg)


def _ctx_model(cfg, Z=None):
    from pilco_amd import _lib
    cx = _lib.Context(device=0)
    cx.gp_set_data(0, cfg["X"], cfg["Y"])
    cx.gp_set_hyp(0, cfg["lengthscales"], cfg["variance"], cfg["noise"])
    if Z is not None:
        cx.gp_set_inducing(0, Z)
    cx.gp_factorize(0)
    return cx


def test_c2_size_across_a_chunk_boundary_values_and_bits():
    """N = 1000, D = E = 10: 1600 test points fill a chunk, the 1601st opens the next."""
    cfg = synthetic.config_c2(N=1000, D=10, E=10)
    D, E, Nt = 10, 10, 1601
    cx = _ctx_model(cfg)
    try:
        xs = _inputs(cfg["X"], Nt, 21)
        mean, var, dmean, dvar = cx.gp_predict_points_jac(0, xs, D, E)
        pm, pv = cx.gp_predict_points(0, xs, D, E)
        assert np.array_equal(mean, pm) and np.array_equal(var, pv)                      # the bits of pilco_gp_predict_points
        again = cx.gp_predict_points_jac(0, xs, D, E)
        assert all(np.array_equal(a, b) for a, b in zip((mean, var, dmean, dvar), again))   # run to run
        sub = np.r_[0, 1, 2, 31, 32, 1598, 1599, 1600, np.random.RandomState(1).choice(np.arange(3, 1598), 24, replace=False)]
        _, _, rdm, rdv = _restated(cfg, xs[sub])                                          # (a subset: per-point results)
        _check_jac("C2 N=1000 Nt=1601", dmean[:, sub].transpose(1, 0, 2), dvar[:, sub].transpose(1, 0, 2), rdm, rdv, cfg)
        for t in (0, 1, 1599, 1600):                                                      # alone = in the batch, at the chunk boundary
            _, _, da, va = cx.gp_predict_points_jac(0, xs[t:t + 1], D, E)
            assert np.array_equal(da[:, 0], dmean[:, t]) and np.array_equal(va[:, 0], dvar[:, t]), t
        perm = np.random.RandomState(2).permutation(Nt)                                   # a permuted batch
        _, _, dp, vp = cx.gp_predict_points_jac(0, xs[perm], D, E)
        assert np.array_equal(dp, dmean[:, perm]) and np.array_equal(vp, dvar[:, perm])
        for e in (0, 7):                                                                  # one output: other chunking, same bits
            me, ve, de, we = cx.gp_predict_points_jac(0, xs, D, E, output=e)
            assert np.array_equal(de[0], dmean[e]) and np.array_equal(we[0], dvar[e])
            assert np.array_equal(me[0], mean[e]) and np.array_equal(ve[0], var[e])
    finally:
        cx.close()


def test_low_noise_model_against_40_digit_truth():
    cfg = _g("predictions_lownoise.npz")
    xs = _inputs(cfg["X"], 4, 9)
    tm, tv = jr.mp_jacobians(cfg, xs)
    _, _, rdm, rdv = _restated(cfg, xs)
    _, _, dmean, dvar = _mgpr(cfg).predict_f_jacobian(xs)
    dmean, dvar = np.asarray(dmean).transpose(1, 0, 2), np.asarray(dvar).transpose(1, 0, 2)
    for e in range(2):
        sm, sv = np.abs(tm[e]).max(), cfg["variance"][e] / cfg["lengthscales"][e].min()
        for what, dev, ref, truth, scale in (("dmean", dmean[e], rdm[e], tm[e], sm), ("dvar", dvar[e], rdv[e], tv[e], sv)):
            err_np, err_gpu = np.abs(ref - truth).max(), np.abs(dev - truth).max()
            print("FIGURE low noise output %d %-5s device %.2e  restatement %.2e  (of the scale: %.2e, %.2e)"
                  % (e, what, err_gpu, err_np, err_gpu / scale, err_np / scale))
            assert err_gpu <= 10 * err_np + 1e-14 * scale, (e, what, err_gpu, err_np)


@pytest.mark.parametrize("kind", ["exact", "sparse"])
def test_single_points_agree_with_predict_on_noisy_inputs_at_zero_variance(kind):
    """mgpr.py:102-118 at s = 0: the input-output covariance V is d mean / d x."""
    if kind == "exact":
        cfg = _g("predictions.npz")
        m = _mgpr(cfg)
    else:
        cfg = _g("sparse_predictions.npz")
        m = _smgpr(cfg, [cfg["Z"]] * 2)   # every model on model 0's Z: the moment matching's model
    D = cfg["X"].shape[1]
    for x in _inputs(cfg["X"], 5, 2):
        _, _, V = m.predict_on_noisy_inputs(x.reshape(1, D), np.zeros((D, D)))
        _, _, dmean, _ = m.predict_f_jacobian(x.reshape(1, D))
        dmean, V = np.asarray(dmean)[0], np.asarray(V).T   # (E, D)
        err = np.abs(dmean - V).max(axis=1) / np.abs(V).max(axis=1)
        print("FIGURE %s dmean vs predict_on_noisy_inputs V: %s" % (kind, err))
        assert np.all(err <= TOL)


def _own_z(M, D, E, seed, first=None):
    rs = np.random.RandomState(seed)
    Zs = [rs.rand(M, D) for _ in range(E)]
    if first is not None:
        Zs[0] = first
    return Zs


@pytest.mark.parametrize("which", ["sparse_predictions", "c4"])
def test_fitc_with_every_outputs_own_z(which):
    if which == "c4":
        cfg = synthetic.config_c4(N=5000, M=200)
        Zs = _own_z(200, 10, 10, 3, cfg["Z"])
    else:
        cfg = _g("sparse_predictions.npz")
        Zs = _own_z(cfg["Z"].shape[0], 3, 2, 4, cfg["Z"])
    m = _smgpr(cfg, Zs)
    xs = _inputs(cfg["X"], 1000, 11)
    _, _, rdm, rdv = _restated(cfg, xs, np.stack(Zs))
    for Nt in (1, 63, 1000):
        mean, var, dmean, dvar = m.predict_f_jacobian(xs[:Nt])
        _same_values(m, xs[:Nt], mean, var)
        _check_jac("FITC %s own Z Nt=%d" % (which, Nt), dmean, dvar, rdm[:, :Nt], rdv[:, :Nt], cfg)
    i = len(Zs) - 1                          # one output alone: its OWN Z, the same bits as in the call for all
    _, _, dmi, dvi = m.models[i].predict_f_jacobian(xs[:63])
    assert np.array_equal(np.asarray(dmi)[:, 0], np.asarray(dmean)[:63, i]) and np.array_equal(np.asarray(dvi)[:, 0], np.asarray(dvar)[:63, i])
    # ... and not what model 0's Z gives (the slot's factorisation, used by the rollout)
    _, _, shared, _ = _restated(cfg, xs[:50], Zs[0])
    _, _, dm1, _ = m.models[1].predict_f_jacobian(xs[:50])
    assert np.abs(np.asarray(dm1)[:, 0] - shared[1]).max() > 1e-6 * np.abs(shared[1]).max()


def test_fitc_on_the_slots_shared_z():
    cfg = _g("sparse_predictions.npz")
    cx = _ctx_model(cfg, cfg["Z"])
    try:
        xs = _inputs(cfg["X"], 65, 5)
        _, _, rdm, rdv = _restated(cfg, xs, cfg["Z"])
        mean, var, dmean, dvar = cx.gp_predict_points_jac(0, xs, 3, 2)
        pm, pv = cx.gp_predict_points(0, xs, 3, 2)
        assert np.array_equal(mean, pm) and np.array_equal(var, pv)
        _check_jac("FITC shared Z", dmean.transpose(1, 0, 2), dvar.transpose(1, 0, 2), rdm, rdv, cfg)
    finally:
        cx.close()


def test_a_nan_row_poisons_only_itself_and_far_points_give_zeros():
    cfg = _model(100, 5, 2, 3)
    m = _mgpr(cfg)
    xs = _inputs(cfg["X"], 40, 1)
    clean = [np.asarray(a) for a in m.predict_f_jacobian(xs)]
    bad = xs.copy()
    bad[7] = np.nan
    got = [np.asarray(a) for a in m.predict_f_jacobian(bad)]
    keep = np.arange(40) != 7
    for a, b in zip(clean, got):
        assert np.array_equal(a[keep], b[keep])
    assert np.all(np.isnan(got[2][7])) and np.all(np.isnan(got[3][7]))
    far = cfg["X"][:3] + 50 * cfg["lengthscales"].max()     # 50 lengthscales from the data in every dimension
    _, _, dmean, dvar = (np.asarray(a) for a in m.predict_f_jacobian(far))
    assert np.all(np.isfinite(dmean)) and np.all(np.isfinite(dvar))
    assert np.abs(dmean).max() <= 1e-300 and np.abs(dvar).max() <= 1e-300


def _raw(cx, slot, Xs, Nt, output, Z_all, mean, var, dmean, dvar):
    p = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    return cx.lib.pilco_gp_predict_points_jac(cx.h, slot, p(Xs), Nt, output, p(Z_all), p(mean), p(var), p(dmean), p(dvar))


def test_refusals_leave_the_outputs_untouched_and_a_valid_call_follows():
    from pilco_amd import _lib
    cfg = _g("predictions.npz")
    D, E, Nt = 3, 2, 10
    xs = _inputs(cfg["X"], Nt, 3)
    mark = -777.0
    out = [np.full((E, Nt), mark), np.full((E, Nt), mark), np.full((E, Nt, D), mark), np.full((E, Nt, D), mark)]
    untouched = lambda: all(np.all(a == mark) for a in out)
    _, _, rdm, rdv = _restated(cfg, xs)
    cx = _ctx_model(cfg)
    try:
        assert _raw(cx, 0, None, Nt, -1, None, *out) == E_SHAPE and untouched()
        assert _raw(cx, 0, xs, Nt, -1, None, out[0], out[1], None, out[3]) == E_SHAPE and untouched()
        assert _raw(cx, 0, xs, Nt, -1, None, out[0], out[1], out[2], None) == E_SHAPE and untouched()
        assert _raw(cx, 0, xs, 0, -1, None, *out) == E_SHAPE and untouched()
        assert _raw(cx, 0, xs, Nt, E, None, *out) == E_SHAPE and untouched()
        assert _raw(cx, 0, xs, Nt, -2, None, *out) == E_SHAPE and untouched()
        assert _raw(cx, 0, xs, Nt, -1, np.zeros((E, 5, D)), *out) == E_SHAPE and untouched()   # Z_all on an exact slot
        iK, beta = cx.gp_get_factors(0, E)
        cx.gp_set_factors(0, iK, beta)
        assert _raw(cx, 0, xs, Nt, -1, None, *out) == E_STATE and untouched()                  # factors of pilco_gp_set_factors
        cx.gp_factorize(0)
        assert _raw(cx, 0, xs, Nt, -1, None, None, None, out[2], out[3]) == 0                  # mean, var may be NULL
        assert np.all(out[0] == mark) and np.all(out[1] == mark)
        _check_jac("after the refusals", out[2].transpose(1, 0, 2), out[3].transpose(1, 0, 2), rdm, rdv, cfg)
        d2, v2 = out[2].copy(), out[3].copy()
        assert _raw(cx, 0, xs, Nt, -1, None, *out) == 0
        pm, pv = cx.gp_predict_points(0, xs, D, E)
        assert np.array_equal(out[0], pm) and np.array_equal(out[1], pv) and np.array_equal(out[2], d2) and np.array_equal(out[3], v2)
    finally:
        cx.close()
    out = [np.full((E, Nt), mark), np.full((E, Nt), mark), np.full((E, Nt, D), mark), np.full((E, Nt, D), mark)]
    sh = _lib.Context(device=0)
    try:
        sh.shard_set(0, 2)
        sh.gp_set_data(0, cfg["X"], cfg["Y"])
        sh.gp_set_hyp(0, cfg["lengthscales"], cfg["variance"], cfg["noise"])
        assert _raw(sh, 0, xs, Nt, -1, None, *out) == E_STATE and untouched()                  # sharded context
    finally:
        sh.close()


def _pilco(cfg, controller):
    from pilco_amd.models import PILCO
    p = PILCO((cfg["X"], cfg["Y"]), controller=controller, horizon=5, ctx=_CTX)
    _set_hyp(p.mgpr, cfg)
    return p


@pytest.mark.parametrize("kind", ["linear", "rbf", "none"])
def test_linearize(kind):
    from pilco_amd.controllers import LinearController, RbfController
    rs = np.random.RandomState(5)
    E = 3
    U = {"linear": 1, "rbf": 2, "none": 0}[kind]
    cfg = _model(60, E + U, E, 40 + U)
    if kind == "linear":
        ctrl = LinearController(E, U, max_action=1.5, ctx=_CTX)
        ctrl.W.assign(rs.randn(U, E))
        ctrl.b.assign(rs.randn(1, U))
    elif kind == "rbf":
        g = _g("rbf_controller.npz")
        ctrl = RbfController(E, U, g["X"].shape[0], max_action=0.8, ctx=_CTX)
        ctrl.set_data((g["X"], 0.3 * g["Y"]))
        for i, mdl in enumerate(ctrl.models):
            mdl.kernel.lengthscales.assign(g["lengthscales"][i])
    else:
        ctrl = None
    p = _pilco(cfg, ctrl)
    if kind == "none":
        assert p.controller is None
    X = _inputs(cfg["X"][:, :E], 5, 8)
    lin = p.linearize(X)
    u = lin.u
    assert u.shape == (5, U) and lin.A.shape == (5, E, E) and lin.B.shape == (5, E, U) and lin.x_next.shape == (5, E)
    assert lin.var.shape == (5, E) and lin.dvar_dx.shape == (5, E, E) and lin.dvar_du.shape == (5, E, U)
    if U:
        for t in range(5):   # the action is compute_action's, K its Jacobian, A_cl by definition
            assert np.array_equal(u[t], np.asarray(p.compute_action(X[t:t + 1])).reshape(-1))
            assert np.array_equal(lin.K[t], ctrl.action_jacobian(X[t]))
        assert lin.K.shape == (5, U, E) and np.array_equal(lin.A_cl, lin.A + lin.B @ lin.K)
        # K against a central difference of the device's own action (step h: error ~ h^2 |u'''| + eps / h)
        h = 1e-5
        for d in range(E):
            dx = np.zeros(E)
            dx[d] = h
            fd = (np.asarray(p.compute_action((X[0] + dx)[None])) - np.asarray(p.compute_action((X[0] - dx)[None]))).reshape(-1) / (2 * h)
            assert np.abs(fd - lin.K[0][:, d]).max() <= 1e-6 * max(1.0, np.abs(lin.K[0]).max())
    else:
        assert lin.K is None and lin.A_cl is None
    xu = np.hstack([X, u])
    mean, var, dmean, dvar = (np.asarray(a) for a in p.mgpr.predict_f_jacobian(xu))
    # bitwise the slices: B as it stands; A = I + the slice, so A - I gives the slice back exactly off the diagonal (on it
    # (1 + x) - 1 rounds x to the spacing of 1 + x: there the identity that holds bit for bit is A = I + slice)
    off = ~np.eye(E, dtype=bool)
    assert np.array_equal(lin.B, dmean[..., E:]) and np.array_equal(lin.A, np.eye(E) + dmean[..., :E])
    assert np.array_equal((lin.A - np.eye(E))[:, off], dmean[..., :E][:, off])
    assert np.array_equal(lin.dvar_dx, dvar[..., :E]) and np.array_equal(lin.dvar_du, dvar[..., E:])
    assert np.array_equal(lin.x_next, X + mean) and np.array_equal(lin.var, var)
    _, _, rdm, rdv = _restated(cfg, xu)
    _check_jac("linearize %s" % kind, np.concatenate([lin.A - np.eye(E), lin.B], axis=-1),
               np.concatenate([lin.dvar_dx, lin.dvar_du], axis=-1), rdm, rdv, cfg)
    one = p.linearize(X[2])                  # a single state: the same fields without the leading axis
    assert one.A.shape == (E, E) and one.B.shape == (E, U) and one.x_next.shape == (E,) and one.u.shape == (U,)
    for f in ("x_next", "var", "A", "B", "dvar_dx", "dvar_du", "u", "K", "A_cl"):
        a, b = getattr(one, f), getattr(lin, f)
        assert (a is None and b is None) or np.array_equal(a, b[2]), f
    if U:
        given = p.linearize(X, u=u)          # a given action: no K, no closed loop; the same open-loop model
        assert given.K is None and given.A_cl is None
        assert np.array_equal(given.A, lin.A) and np.array_equal(given.B, lin.B)
