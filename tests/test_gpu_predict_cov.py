"""The full posterior covariance between test points and joint samples of the latent functions on the MI355X:
pilco_gp_predict_points_cov, pilco_gp_sample_points (csrc/predict_cov.hip, docs/predict_cov.md) and predict_f(full_cov=True) /
predict_f_samples of MGPR and SMGPR, predict_f_full_cov / predict_f_samples of the output models.  Yardsticks: the 40-digit truth and units of
tests/golden/predict_cov.npz (tools/gen_golden_predict_cov.py; pinned on the CPU in tests/test_predict_cov_cpu.py), the
GPflow-ordered float64 restatement of helpers/predict_cov_restatement.py for the larger shapes, numpy.linalg.cholesky's own
backward error for the factor, and the Python restatement of Philox domain 5 for the draws."""
import ctypes as C
import os

import numpy as np
import pytest

from helpers import predict_cov_cases as cc
from helpers import predict_cov_restatement as cr
from pilco_amd import synthetic

pytestmark = pytest.mark.gpu
U53 = 2.0 ** -53
E_SHAPE, E_NOT_PD, E_STATE = 1, 2, 5
_CTX = None


@pytest.fixture(scope="module", autouse=True)
def own_ctx():
    from pilco_amd import _lib
    global _CTX
    _CTX = _lib.Context(device=0)
    yield _CTX
    _CTX.close()


def _load_model(cx, X, Y, ls, var, noise, Z=None):
    cx.gp_set_data(0, X, Y)
    cx.gp_set_hyp(0, ls, var, noise)
    cx.gp_set_inducing(0, Z)
    cx.gp_factorize(0)


def _case_model(cx, c, d):
    _load_model(cx, d["X"], d["Y"], d["ls"], d["var"], d["noise"], d["Z"][0] if c["M"] else None)


def _check_against_truth(tag, mean, cov, ref_mean, d, outputs):
    assert np.all(np.isfinite(cov)) and np.all(np.isfinite(mean)), tag
    assert np.array_equal(mean, ref_mean), tag                            # the bits of gp_predict_points
    assert np.array_equal(cov, cov.transpose(0, 2, 1)), tag               # symmetric to the bit
    truth, unit = d["cov"][outputs], d["unit"][outputs]
    err = np.abs(cov - truth) / unit
    K, i = err.max(), np.unravel_index(err.argmax(), err.shape)
    Kd = np.einsum("eaa->ea", err).max()
    print("%-32s K = %.3g at %s (diagonal %.3g), cap %.3g" % (tag, K, i, Kd, d["cap"]))
    assert Kd <= d["cap"], (tag, "diagonal", Kd)
    assert K <= d["cap"], (tag, K, i)


@pytest.mark.parametrize("name", cc.case_ids())
def test_every_case_of_the_fixture_on_every_route(name):
    c = cc.by_name(name)
    d = cc.load(c)
    D, E = c["D"], c["E"]
    _case_model(_CTX, c, d)
    za = cc.z_arg(c, d)
    ref_mean, ref_var = _CTX.gp_predict_points(0, d["xs"], D, E, Z_all=za)
    mean, cov = _CTX.gp_predict_points_cov(0, d["xs"], D, E, Z_all=za)
    assert mean.shape == (E, c["Nt"]) and cov.shape == (E, c["Nt"], c["Nt"])
    _check_against_truth(name, mean, cov, ref_mean, d, slice(None))
    if E > 1:                                                             # one output alone
        m1, c1 = _CTX.gp_predict_points_cov(0, d["xs"], D, E, output=1, Z_all=za)
        _check_against_truth(name + " output=1", m1, c1, ref_mean[1:2], d, slice(1, 2))
        assert np.array_equal(c1[0], cov[1])
    if c["M"] and not c["own"]:                                           # the shared Z handed over as every output's own
        m2, c2 = _CTX.gp_predict_points_cov(0, d["xs"], D, E, Z_all=np.stack([d["Z"][0]] * E))
        rm2, _ = _CTX.gp_predict_points(0, d["xs"], D, E, Z_all=np.stack([d["Z"][0]] * E))
        _check_against_truth(name + " Z_all=shared", m2, c2, rm2, d, slice(None))


@pytest.mark.parametrize("name", ["x65_t65_d4_e1_lo", "f65_t17_d4_e3_own_lo", "x65_t15_d11_e3", "f64_t65_d4_e1"])
def test_bit_contracts(name):
    from pilco_amd import _lib
    c = cc.by_name(name)
    d = cc.load(c)
    D, E, Nt = c["D"], c["E"], c["Nt"]
    rng = np.random.RandomState(3)
    xs = np.concatenate([d["xs"], rng.uniform(-1, 1, (65 - Nt, D))]) if Nt < 65 else d["xs"]
    cx = _lib.Context(device=0)
    try:
        _case_model(cx, c, d)
        za = cc.z_arg(c, d)
        p0 = cx.gp_predict_points(0, xs, D, E, Z_all=za)
        mean, cov = cx.gp_predict_points_cov(0, xs, D, E, Z_all=za)
        m2, c2 = cx.gp_predict_points_cov(0, xs, D, E, Z_all=za)
        assert np.array_equal(mean, m2) and np.array_equal(cov, c2)                           # run to run
        perm = rng.permutation(65)
        mp_, cp = cx.gp_predict_points_cov(0, xs[perm], D, E, Z_all=za)
        assert np.array_equal(mp_, mean[:, perm]) and np.array_equal(cp, cov[:, perm][:, :, perm])   # wherever the points stand
        m17, c17 = cx.gp_predict_points_cov(0, xs[:17], D, E, Z_all=za)
        assert np.array_equal(m17, mean[:, :17]) and np.array_equal(c17, cov[:, :17, :17])   # whatever Nt is
        big = np.concatenate([rng.uniform(-1, 1, (64, D)), xs])                              # ... and in another tile
        _, cb = cx.gp_predict_points_cov(0, big, D, E, Z_all=za)
        assert np.array_equal(cb[:, 64:, 64:], cov)
        for e in range(E):                                                                   # alone or with the others
            me, ce = cx.gp_predict_points_cov(0, xs, D, E, output=e, Z_all=za)
            assert np.array_equal(me[0], mean[e]) and np.array_equal(ce[0], cov[e])
        # a moment-matching rollout and the marginal predictions around the new path: their bits unchanged
        S = c["E"]
        if D > S:
            U = D - S
            pol = dict(kind=_lib.POLICY_LINEAR, state_dim=S, control_dim=U, W=0.1 * rng.randn(U, S), b=np.zeros(U), max_action=1.3, squash=True)
            rw = [dict(kind=_lib.REWARD_EXPONENTIAL, coef=1.0, W=np.eye(S), t=np.zeros(S))]
            m0, S0 = 0.1 * rng.randn(1, S), 0.05 * np.eye(S)
            r0 = cx.rollout(pol, rw, m0, S0, 4)
            cx.gp_predict_points_cov(0, xs, D, E, Z_all=za)
            cx.gp_sample_points(0, xs, D, E, 3, Z_all=za)
            r1 = cx.rollout(pol, rw, m0, S0, 4)
            assert all(np.array_equal(a, b) for a, b in zip(r0, r1))
        p1 = cx.gp_predict_points(0, xs, D, E, Z_all=za)
        assert np.array_equal(p0[0], p1[0]) and np.array_equal(p0[1], p1[1])
        _, c3 = cx.gp_predict_points_cov(0, xs, D, E, Z_all=za)
        assert np.array_equal(c3, cov)
    finally:
        cx.close()


def _uniform_like(X, n, seed):
    rs = np.random.RandomState(seed)
    lo, hi = X.min(0), X.max(0)
    return lo + (hi - lo) * rs.rand(n, X.shape[1])


@pytest.mark.parametrize("shape", ["N257_Nt200", "N1000_Nt1100", "fitc_M200_Nt300"])
def test_larger_shapes_against_the_gpflow_ordered_restatement(shape):
    if shape == "N257_Nt200":
        cfg, Z, Nt = synthetic.config_c2(N=257, D=5, E=2, seed=5), None, 200
    elif shape == "N1000_Nt1100":
        cfg, Z, Nt = synthetic.config_c2(N=1000, D=11, E=2), None, 1100
    else:
        cfg, Nt = synthetic.config_c4(N=1000, M=200, D=6, E=2), 300
        Z = cfg["Z"]
    E, D = 2, cfg["X"].shape[1]
    xs = _uniform_like(cfg["X"], Nt, 8)
    c = dict(E=E, M=0 if Z is None else len(Z), own=False)
    d = dict(X=cfg["X"], ls=cfg["lengthscales"], var=cfg["variance"], noise=cfg["noise"], xs=xs, Z=None if Z is None else Z[None])
    ref = cr.restate_a(c, d)
    _load_model(_CTX, cfg["X"], cfg["Y"], cfg["lengthscales"], cfg["variance"], cfg["noise"], Z)
    ref_mean, _ = _CTX.gp_predict_points(0, xs, D, E)
    mean, cov = _CTX.gp_predict_points_cov(0, xs, D, E)
    assert np.array_equal(mean, ref_mean) and np.array_equal(cov, cov.transpose(0, 2, 1))
    for e in range(E):
        err = np.abs(cov[e] - ref[e]).max()
        print("%s output %d: largest |cov - restatement| = %.3g sf2" % (shape, e, err / cfg["variance"][e]))
        assert err <= 1e-8 * cfg["variance"][e], (e, err)


def _backward_ratio(Cf, A):
    """max_ab |C C^T - A|_ab / (2^-53 (|C||C|^T)_ab), the products in extended precision."""
    L = Cf.astype(np.longdouble)
    res = np.abs(L @ L.T - A.astype(np.longdouble))
    den = U53 * (np.abs(L) @ np.abs(L).T)
    assert np.all(res[den == 0] == 0)        # (the far point: exact zeros on both sides)
    return float(np.max(res[den > 0] / den[den > 0]))


def _check_factor(tag, chol, cov, jitter):
    for e in range(cov.shape[0]):
        A = cov[e] + jitter * np.eye(cov.shape[1])
        assert np.all(np.isfinite(chol[e])), tag
        assert np.array_equal(chol[e], np.tril(chol[e])), (tag, "not lower triangular")
        ref = _backward_ratio(np.linalg.cholesky(A), A)
        got = _backward_ratio(chol[e], A)
        print("%-40s output %d: backward error %.3g (numpy.linalg.cholesky %.3g)" % (tag, e, got, ref))
        assert got <= max(8.0, 8.0 * ref), (tag, e, got, ref)


SAMPLE_CASES = [("x64_t1_d1_e1", 3), ("x65_t17_d4_e3_lo", 65), ("f65_t17_d4_e3_own_lo", 3), ("x65_t65_d4_e1_lo", 1),
                ("f64_t65_d4_e1", 65), ("x130_t130_d4_e1", 3), ("f130_t130_d4_e1", 65), ("f64_t17_d4_e3", 1)]


@pytest.mark.parametrize("name,S", SAMPLE_CASES)
def test_samples_from_supplied_draws(name, S):
    c = cc.by_name(name)
    d = cc.load(c)
    D, E, Nt = c["D"], c["E"], c["Nt"]
    _case_model(_CTX, c, d)
    za = cc.z_arg(c, d)
    z = np.random.RandomState(S + Nt).randn(S, Nt, E)
    mean, cov = _CTX.gp_predict_points_cov(0, d["xs"], D, E, Z_all=za)
    smp, parts = _CTX.gp_sample_points(0, d["xs"], D, E, S, Z_all=za, draws=z, parts=True)
    assert smp.shape == (S, Nt, E)
    assert np.array_equal(parts["cov"], cov) and np.array_equal(parts["mean"], mean) and np.array_equal(parts["draws"], z)
    _check_factor(name, parts["chol"], cov, 1e-6)
    for e in range(E):                                                     # the plain product, from the DEVICE's factor
        Cf = parts["chol"][e]
        ref = z[:, :, e] @ Cf.T
        bound = 8 * U53 * (np.abs(z[:, :, e]) @ np.abs(Cf).T)
        got = smp[:, :, e] - mean[e][None]
        # (the sample is fl(mean + C z): its own rounding, half an ulp of the sample, and the subtraction's are not the product's)
        slack = U53 * (np.abs(smp[:, :, e]) + np.abs(got))
        ratio = np.max((np.abs(got - ref) - slack) / np.maximum(bound, 1e-300))
        print("%-40s output %d: |C z - product| / (8 eps |C||z|) = %.3g" % (name, e, ratio))
        assert ratio <= 1.0, (name, e, ratio)
    assert np.array_equal(smp, _CTX.gp_sample_points(0, d["xs"], D, E, S, Z_all=za, draws=z))


def test_samples_drawn_on_the_device():
    c = cc.by_name("x65_t17_d4_e3_lo")
    d = cc.load(c)
    D, E, Nt = c["D"], c["E"], c["Nt"]
    _case_model(_CTX, c, d)
    a, pa = _CTX.gp_sample_points(0, d["xs"], D, E, 65, seed=1234, parts=True)
    z, r = cr.cov_normals(1234, 65, Nt, range(E))
    dz = np.abs(pa["draws"] - z)
    bound = 16 * U53 * np.maximum(1.0, r)
    print("device draws: largest |dz| / bound = %.3g over %d draws" % ((dz / bound).max(), dz.size))
    assert np.all(dz <= bound)
    b, pb = _CTX.gp_sample_points(0, d["xs"], D, E, 65, seed=1234, parts=True)
    assert np.array_equal(a, b) and np.array_equal(pa["draws"], pb["draws"])             # the same seed: the same bits
    o, po = _CTX.gp_sample_points(0, d["xs"], D, E, 65, seed=1235, parts=True)
    assert np.abs(po["draws"] - pa["draws"]).max() > 1.0                                # another seed: other draws
    assert np.array_equal(a, _CTX.gp_sample_points(0, d["xs"], D, E, 65, draws=pa["draws"]))   # the draws fed back
    s3 = _CTX.gp_sample_points(0, d["xs"], D, E, 3, seed=1234)
    assert np.array_equal(s3, a[:3])                                                    # a sample does not depend on S
    s1, p1 = _CTX.gp_sample_points(0, d["xs"], D, E, 65, output=1, seed=1234, parts=True)
    assert np.array_equal(p1["draws"][:, :, 0], pa["draws"][:, :, 1]) and np.array_equal(s1[:, :, 0], a[:, :, 1])   # (seed, s, a, e) only
    big = 2 ** 64 - 3                                                                   # both key words in use
    _, pbig = _CTX.gp_sample_points(0, d["xs"][:2], D, E, 2, seed=big, parts=True)
    zb, rb = cr.cov_normals(big, 2, 2, range(E))
    assert np.all(np.abs(pbig["draws"] - zb) <= 16 * U53 * np.maximum(1.0, rb))


def test_sample_covariance_of_many_draws():
    """Loose on purpose: catches a transposed factor or a stream reused across points, which the exact checks cannot."""
    c = cc.by_name("x65_t17_d4_e3_lo")
    d = cc.load(c)
    D, E, S = c["D"], c["E"], 4096
    xs = d["xs"][[0, 2, 4, 6, 7, 8]]
    _case_model(_CTX, c, d)
    smp, parts = _CTX.gp_sample_points(0, xs, D, E, S, seed=77, parts=True)
    for e in range(E):
        A = parts["cov"][e] + 1e-6 * np.eye(6)
        dev = smp[:, :, e] - parts["mean"][e][None]
        emp = dev.T @ dev / S
        se = np.sqrt((np.outer(np.diag(A), np.diag(A)) + A * A) / S)
        print("output %d: largest |sample covariance - cov| / standard error = %.3g" % (e, np.max(np.abs(emp - A) / se)))
        assert np.all(np.abs(emp - A) <= 5 * se), e


def _raw_sample(cx, Xs, Nt, output, Z_all, S, z_in, jitter, samples, mean=None, cov=None, chol=None, z_out=None, slot=0, seed=0):
    p = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    return cx.lib.pilco_gp_sample_points(cx.h, slot, p(Xs), Nt, output, p(Z_all), S, seed, p(z_in), jitter, p(samples), p(mean), p(cov),
                                         p(chol), p(z_out))


def _raw_cov(cx, Xs, Nt, output, Z_all, mean, cov, slot=0):
    p = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    return cx.lib.pilco_gp_predict_points_cov(cx.h, slot, p(Xs), Nt, output, p(Z_all), p(mean), p(cov))


def test_duplicated_test_points_without_jitter():
    from pilco_amd import _lib
    c = cc.by_name("x65_t17_d4_e3_lo")
    d = cc.load(c)
    D, E, Nt, S = c["D"], c["E"], c["Nt"], 2
    _case_model(_CTX, c, d)
    xs = np.ascontiguousarray(d["xs"])
    assert np.array_equal(xs[0], xs[1])
    mark = 12345.0
    bufs = [np.full(s, mark) for s in ((S, Nt, E), (E, Nt), (E, Nt, Nt), (E, Nt, Nt), (S, Nt, E))]
    rc = _raw_sample(_CTX, xs, Nt, -1, None, S, None, 0.0, *bufs)
    if rc == E_NOT_PD:
        assert all(np.all(b == mark) for b in bufs)                       # nothing written
        assert 0 <= _CTX.lib.pilco_last_not_pd_output(_CTX.h) < E
        msg = _CTX.lib.pilco_last_error(_CTX.h).decode()
        assert "output %d" % _CTX.lib.pilco_last_not_pd_output(_CTX.h) in msg, msg
        with pytest.raises(_lib.NotPositiveDefiniteError):
            _CTX.gp_sample_points(0, xs, D, E, S, jitter=0.0)
    else:
        assert rc == 0
        assert all(np.all(np.isfinite(b)) for b in bufs)
        _check_factor("duplicates, jitter 0", bufs[3], bufs[2], 0.0)
    smp, parts = _CTX.gp_sample_points(0, xs, D, E, S, parts=True)        # the default jitter: the same points succeed
    assert np.all(np.isfinite(smp))
    _check_factor("duplicates, jitter 1e-6", parts["chol"], parts["cov"], 1e-6)


def test_contract_errors_and_the_budget():
    from pilco_amd import _lib
    c = cc.by_name("x65_t17_d4_e3_lo")
    d = cc.load(c)
    D, E, Nt, S = c["D"], c["E"], c["Nt"], 2
    xs = np.ascontiguousarray(d["xs"])
    smp, mean, cov = np.empty((S, Nt, E)), np.empty((E, Nt)), np.empty((E, Nt, Nt))
    cx = _lib.Context(device=0)
    try:
        _case_model(cx, c, d)
        assert _raw_cov(cx, xs, Nt, -1, None, mean, cov) == 0 and _raw_cov(cx, xs, Nt, -1, None, None, cov) == 0
        assert _raw_cov(cx, xs, Nt, -1, None, mean, None) == E_SHAPE
        assert _raw_cov(cx, xs, 0, -1, None, mean, cov) == E_SHAPE and _raw_cov(cx, None, Nt, -1, None, mean, cov) == E_SHAPE
        assert _raw_cov(cx, xs, Nt, E, None, mean, cov) == E_SHAPE and _raw_cov(cx, xs, Nt, -2, None, mean, cov) == E_SHAPE
        assert _raw_sample(cx, xs, Nt, -1, None, S, None, 1e-6, smp) == 0
        assert _raw_sample(cx, xs, Nt, -1, None, S, None, -1e-6, smp) == E_SHAPE
        assert _raw_sample(cx, xs, Nt, -1, None, S, None, float("nan"), smp) == E_SHAPE
        assert _raw_sample(cx, xs, Nt, -1, None, S, None, float("inf"), smp) == E_SHAPE
        assert _raw_sample(cx, xs, Nt, -1, None, 0, None, 1e-6, smp) == E_SHAPE
        assert _raw_sample(cx, xs, Nt, -1, None, S, None, 1e-6, None) == E_SHAPE
        za = np.zeros((E, 5, D))
        assert _raw_cov(cx, xs, Nt, -1, za, mean, cov) == E_SHAPE                       # Z_all on an exact slot
        assert _raw_sample(cx, xs, Nt, -1, za, S, None, 1e-6, smp) == E_SHAPE
        # the budget: refused with the largest Nt that fits in the message; that Nt then succeeds
        x200 = np.random.RandomState(1).uniform(-1, 1, (200, D))
        old = os.environ.get("PILCO_PREDICT_COV_BUDGET")
        os.environ["PILCO_PREDICT_COV_BUDGET"] = str(2 * E * 128 * 128 + E * 128 * 128)   # (two operands of 128 x npad 128, one matrix)
        try:
            with pytest.raises(_lib.PilcoError) as ei:
                cx.gp_predict_points_cov(0, x200, D, E)
            assert ei.value.code == E_SHAPE and "largest Nt that fits is 128" in str(ei.value), str(ei.value)
            _, c128 = cx.gp_predict_points_cov(0, x200[:128], D, E)
            with pytest.raises(_lib.PilcoError) as ei:
                cx.gp_sample_points(0, x200[:128], D, E, S)
            assert ei.value.code == E_SHAPE and "largest Nt that fits is 64" in str(ei.value), str(ei.value)
            cx.gp_sample_points(0, x200[:64], D, E, S)
        finally:
            if old is None:
                del os.environ["PILCO_PREDICT_COV_BUDGET"]
            else:
                os.environ["PILCO_PREDICT_COV_BUDGET"] = old
        _, call = cx.gp_predict_points_cov(0, x200, D, E)
        assert np.array_equal(call[:, :128, :128], c128)
        iK, beta = cx.gp_get_factors(0, E)
        cx.gp_set_factors(0, iK, beta)
        assert _raw_cov(cx, xs, Nt, -1, None, mean, cov) == E_STATE                     # factors of pilco_gp_set_factors
        assert _raw_sample(cx, xs, Nt, -1, None, S, None, 1e-6, smp) == E_STATE
        cx.gp_factorize(0)
        assert _raw_cov(cx, xs, Nt, -1, None, mean, cov) == 0
    finally:
        cx.close()
    sh = _lib.Context(device=0)
    try:
        sh.shard_set(0, 2)
        sh.gp_set_data(0, d["X"], d["Y"])
        sh.gp_set_hyp(0, d["ls"], d["var"], d["noise"])
        assert _raw_cov(sh, xs, Nt, -1, None, mean, cov) == E_STATE                     # sharded context
        assert _raw_sample(sh, xs, Nt, -1, None, S, None, 1e-6, smp) == E_STATE
    finally:
        sh.close()


def _set_hyp(model, d):
    for i, mdl in enumerate(model.models):
        mdl.kernel.lengthscales.assign(d["ls"][i])
        mdl.kernel.variance.assign(d["var"][i])
        mdl.likelihood.variance.assign(d["noise"][i])
    return model


@pytest.mark.parametrize("name", ["x65_t17_d4_e3_lo", "f65_t17_d4_e3_own_lo"])
def test_through_the_models(name):
    from pilco_amd.models import MGPR, SMGPR
    c = cc.by_name(name)
    d = cc.load(c)
    D, E, Nt, S = c["D"], c["E"], c["Nt"], 3
    xs = d["xs"]
    if c["M"]:
        m = _set_hyp(SMGPR((d["X"], d["Y"]), num_induced_points=c["M"], ctx=_CTX), d)
        for mdl, Z in zip(m.models, d["Z"]):
            mdl.inducing_variable.Z.assign(Z)
        za = d["Z"]
    else:
        m, za = _set_hyp(MGPR((d["X"], d["Y"]), ctx=_CTX), d), None
    mean, cov = m.predict_f(xs, full_cov=True)
    assert mean.shape == (Nt, E) and cov.shape == (E, Nt, Nt)                            # GPflow's shapes
    rm, rc = _CTX.gp_predict_points_cov(0, xs, D, E, Z_all=za)
    assert np.array_equal(mean, rm.T) and np.array_equal(cov, rc)
    assert cr.k_of(np.asarray(cov), d) <= d["cap"]
    m1, c1 = m.models[1].predict_f_full_cov(xs)
    assert m1.shape == (Nt, 1) and c1.shape == (1, Nt, Nt)
    assert np.array_equal(m1[:, 0], rm[1]) and np.array_equal(c1[0], rc[1])
    with pytest.raises(NotImplementedError):
        m.models[0].predict_f(xs, full_output_cov=True)
    with pytest.raises(NotImplementedError):
        m.models[0].predict_y(xs, full_cov=True)
    smp, parts = m.predict_f_samples(xs, S, seed=9, return_parts=True)
    assert smp.shape == (S, Nt, E) and parts["mean"].shape == (Nt, E) and parts["chol"].shape == (E, Nt, Nt)
    assert np.array_equal(smp, _CTX.gp_sample_points(0, xs, D, E, S, Z_all=za, seed=9))
    assert np.array_equal(smp, m.predict_f_samples(xs, S, draws=parts["draws"]))         # the draws fed back
    assert np.array_equal(parts["cov"], rc)
    one = m.models[1].predict_f_samples(xs, S, seed=9)
    assert one.shape == (S, Nt, 1) and np.array_equal(one[:, :, 0], smp[:, :, 1])
    assert m.models[1].predict_f_samples(xs, seed=9).shape == (Nt, 1) and m.predict_f_samples(xs).shape == (Nt, E)
    assert np.array_equal(m.models[1].predict_f_samples(xs, seed=9)[:, 0], smp[0, :, 1])
    # the marginals: mean + sqrt(var) z on predict_f's bits, the same stream (host restatement of the draws)
    pm, pv = m.predict_f(xs)
    sm, pp = m.predict_f_samples(xs, S, full_cov=False, seed=9, return_parts=True)
    assert np.array_equal(sm, np.asarray(pm)[None] + np.sqrt(np.asarray(pv))[None] * np.asarray(pp["draws"]))
    assert np.array_equal(pp["mean"], pm) and np.array_equal(pp["var"], pv)
    z, r = cr.cov_normals(9, S, Nt, range(E))
    assert np.all(np.abs(np.asarray(pp["draws"]) - z) <= 16 * U53 * np.maximum(1.0, r))
    assert np.all(np.abs(np.asarray(pp["draws"]) - np.asarray(parts["draws"])) <= 16 * U53 * np.maximum(1.0, r))
    assert np.array_equal(sm, m.predict_f_samples(xs, S, full_cov=False, draws=pp["draws"]))
