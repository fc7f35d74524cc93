"""The device training objectives at their edge shapes: pilco_gp_fitc_nlml (gpflow GPRFITC's training loss and its
gradient w.r.t. lengthscales, kernel variance, noise variance and each output's own inducing inputs Z; csrc/fitc_train.hip)
and pilco_gp_nlml (GPR's; launch_nlml_grad in csrc/linalg.hip), the two objectives MGPR.optimize / SMGPR.optimize call at
every iteration.  The yardsticks are plain float64 restatements: tests/helpers/fitc_objective.py (torch autograd) and
oracle/gp_train.py, both pinned to the executed reference in tests/test_training_objectives_cpu.py.  The device is compared
with itself only where the check is bit identity.

Shapes that matter to the FITC objective: Mp = M and Np = N padded to 64 (the buffer layout), N >= 2048 (the matrix-core
kernel-derivative reductions split the points over FT_NSPLIT slices), D <= 14 (matrix cores) against D > 14 (the VALU
reductions k_fitc_kgrad<DT>, also forced with PILCO_FITC_KGRAD_VALU), E up to 32 (every d_info slot).  For the exact GP:
the k_nlml_grad_partial<DT> instantiation (DT = 4, 8, 12, 16, 24, 32) and N around the 64-row tile."""
import functools

import numpy as np
import pytest

from helpers.fitc_objective import fitc_reference
from oracle.gp_train import nlml_and_grad

pytestmark = pytest.mark.gpu
_CTX = None


@pytest.fixture(scope="module", autouse=True)
def own_ctx():
    """The objectives of this module run on a context of their own (closed at the end), not on the process-wide default."""
    from pilco_amd import _lib
    global _CTX
    _CTX = _lib.Context(device=0)
    yield _CTX
    _CTX.close()


# ---------------------------------------------------------------------------------------------------------- problems
def _problem(N, M, D, E, seed, offset=0.0, c4=False):
    """Data, hyper-parameters and per-output inducing inputs.  offset: X and Z shifted by that many lengthscales."""
    if c4:
        from pilco_amd import synthetic
        c = synthetic.config_c4(N=N, M=M, D=D, E=E)
        Z_all = np.random.RandomState(99).rand(E, M, D)          # smgpr.py:20's rand(M, D), one set per output
        return c["X"], c["Y"], c["lengthscales"], c["variance"], c["noise"], Z_all
    rs = np.random.RandomState(seed)
    X = 1.5 * rs.randn(N, D)
    A = rs.randn(D, E) / np.sqrt(D)
    Y = np.sin(X) @ A + 0.05 * rs.randn(N, E)
    ls = 1.0 + rs.rand(E, D)
    var = 0.6 + rs.rand(E)
    noise = 0.01 + 0.02 * rs.rand(E)
    Z_all = np.empty((E, M, D))
    for e in range(E):
        if M <= N:
            Z_all[e] = X[rs.choice(N, M, replace=False)] + 0.2 * rs.randn(M, D)
        else:
            Z_all[e] = 1.5 * rs.randn(M, D)
    if offset:
        shift = offset * ls.mean(0)
        X, Z_all = X + shift, Z_all + shift
    return X, Y, ls, var, noise, Z_all


# (id, N, M, D, E, extra): every shape named for the branch it takes
FITC_CASES = [
    ("overflow_M70_N100_MpEqNp", 100, 70, 3, 2, {}),
    ("M_eq_N_64", 64, 64, 5, 2, {}),
    ("M96_gt_N64", 64, 96, 5, 2, {}),
    ("M1_N50", 50, 1, 3, 2, {}),
    ("nsp_N2047", 2047, 40, 5, 2, {}),
    ("nsp_N2048", 2048, 40, 5, 2, {}),
    ("nsp_N2049", 2049, 40, 5, 2, {}),
    ("config4_M200_N5000_D10_E10", 5000, 200, 10, 10, {"c4": True}),
    ("mfma_D1", 90, 20, 1, 2, {}),
    ("mfma_D13", 130, 33, 13, 2, {}),
    ("mfma_D14", 130, 33, 14, 2, {}),
    ("valu_D15", 130, 33, 15, 2, {}),
    ("valu_D16", 130, 33, 16, 2, {}),
    ("valu_D17", 130, 33, 17, 2, {}),
    ("valu_D24", 100, 20, 24, 2, {}),
    ("valu_D32", 100, 20, 32, 2, {}),
    ("E32_all_info_slots", 80, 17, 3, 32, {}),
    ("offset_30_lengthscales", 300, 50, 3, 2, {"offset": 30.0}),
]
_FITC_BY_ID = {c[0]: c for c in FITC_CASES}


@functools.lru_cache(maxsize=None)
def _fitc_case(cid):
    _, N, M, D, E, extra = _FITC_BY_ID[cid]
    X, Y, ls, var, noise, Z_all = _problem(N, M, D, E, seed=sum(map(ord, cid)), **extra)
    ref = fitc_reference(X, Y, Z_all, ls, var, noise)
    return (X, Y, ls, var, noise, Z_all), ref


def _fitc_on(cx, prob, want_grad=True, slot=0):
    X, Y, ls, var, noise, Z_all = prob
    cx.gp_set_data(slot, X, Y)
    cx.gp_set_hyp(slot, ls, var, noise)
    return cx.gp_fitc_nlml(slot, Z_all, X.shape[1], Y.shape[1], want_grad=want_grad)


def _check_grad(got, ref, floor_scale, what):
    """|got - ref| <= 1e-6 |ref| + 1e-8 max|reference gradient of the output|, per output."""
    for e in range(ref.shape[0]):
        err = np.abs(got[e] - ref[e])
        lim = 1e-6 * np.abs(ref[e]) + 1e-8 * floor_scale[e]
        bad = err > lim
        assert not bad.any(), f"{what} output {e}: worst excess {np.max(err - lim):.3e} at {np.unravel_index(np.argmax(err - lim), err.shape)}"


def _check_fitc(out, ref):
    nlml, gh, gz = out
    rn, rh, rz = ref
    np.testing.assert_allclose(nlml, rn, rtol=1e-9, atol=0)
    E = rn.shape[0]
    scale = np.array([max(np.abs(rh[e]).max(), np.abs(rz[e]).max()) for e in range(E)])
    D = rz.shape[2]
    _check_grad(gh[:, :D], rh[:, :D], scale, "d lengthscales")
    _check_grad(gh[:, D:D + 1], rh[:, D:D + 1], scale, "d variance")
    _check_grad(gh[:, D + 1:], rh[:, D + 1:], scale, "d noise")
    _check_grad(gz, rz, scale, "d Z")


# ---------------------------------------------------------------------------------------------------------- FITC
@pytest.mark.parametrize("cid", [c[0] for c in FITC_CASES])
def test_fitc_objective_and_gradients_match_the_reference(cid, monkeypatch):
    monkeypatch.delenv("PILCO_FITC_KGRAD_VALU", raising=False)
    prob, ref = _fitc_case(cid)
    out = _fitc_on(_CTX, prob)
    _check_fitc(out, ref)
    # a value-only call sums |gamma|^2 on the host instead of in k_fitc_kgrad_fin: the same value
    nv, gh, gz = _CTX.gp_fitc_nlml(0, prob[5], prob[0].shape[1], prob[1].shape[1], want_grad=False)
    assert gh is None and gz is None
    np.testing.assert_allclose(nv, out[0], rtol=1e-12, atol=0)


@pytest.mark.parametrize("cid", [c[0] for c in FITC_CASES if c[3] <= 14])
def test_fitc_valu_reductions_match_the_reference_and_the_matrix_cores(cid, monkeypatch):
    """The same cases with the kernel-derivative reductions forced onto k_fitc_kgrad<DT> (read at call time; the path is
    part of the cached graph's key): both paths against the reference, and against each other to 1e-10."""
    prob, ref = _fitc_case(cid)
    monkeypatch.delenv("PILCO_FITC_KGRAD_VALU", raising=False)
    mf = _fitc_on(_CTX, prob)
    monkeypatch.setenv("PILCO_FITC_KGRAD_VALU", "1")
    va = _fitc_on(_CTX, prob)
    _check_fitc(va, ref)
    _check_fitc(mf, ref)
    np.testing.assert_allclose(va[0], mf[0], rtol=1e-10, atol=0)
    E = ref[0].shape[0]
    for e in range(E):
        s = max(np.abs(ref[1][e]).max(), np.abs(ref[2][e]).max())
        np.testing.assert_allclose(va[1][e], mf[1][e], rtol=1e-10, atol=1e-10 * s)
        np.testing.assert_allclose(va[2][e], mf[2][e], rtol=1e-10, atol=1e-10 * s)


def _same(a, b):
    for x, y in zip(a, b):
        if x is None or y is None:
            assert x is None and y is None
        else:
            assert np.array_equal(np.asarray(x), np.asarray(y))


def test_fitc_stale_state_and_cached_graphs_leave_later_results_unchanged(monkeypatch):
    """One context runs the FITC objective at M = 30, then at M = 70 with N = 100 (where Mp == Np and the result block at
    the end of the slot's vector buffer was once sized too small), then at M = 30 again; then the FITC factorisation and a
    rollout on the same slot, and a prediction from a second, exact model on the same context.  Each result is bit-identical
    to the one a fresh context gives.  This catches writes that land in a neighbouring buffer or state left behind by an
    earlier shape; it cannot prove that no write goes past an allocation (one that lands in unused memory changes nothing)."""
    from pilco_amd import _lib
    monkeypatch.delenv("PILCO_FITC_KGRAD_VALU", raising=False)
    N, D, E = 100, 3, 2
    X, Y, ls, var, noise, Z70 = _problem(N, 70, D, E, seed=5)
    Z30 = Z70[:, :30].copy()
    rs = np.random.RandomState(6)
    Xe, Ye = rs.randn(120, D), rs.randn(120, E)
    Xs = rs.randn(40, D)
    pol = dict(kind=_lib.POLICY_LINEAR, state_dim=E, control_dim=D - E, W=0.3 * rs.randn(D - E, E), b=np.zeros(D - E), max_action=1.0,
               squash=True)
    rw = [dict(kind=_lib.REWARD_EXPONENTIAL, coef=1.0, W=np.eye(E), t=np.zeros(E))]
    m0, S0 = 0.1 * rs.randn(E), 0.05 * np.eye(E)

    def fitc(cx, Z):
        cx.gp_set_data(0, X, Y)
        cx.gp_set_hyp(0, ls, var, noise)
        return cx.gp_fitc_nlml(0, Z, D, E)

    def rollout(cx):
        cx.gp_set_data(0, X, Y)
        cx.gp_set_hyp(0, ls, var, noise)
        cx.gp_set_inducing(0, Z70[0])
        cx.gp_factorize(0)
        return cx.rollout(pol, rw, m0, S0, 4, want_traj=True)

    def predict(cx):
        cx.gp_set_data(1, Xe, Ye)
        cx.gp_set_hyp(1, ls, var, noise)
        cx.gp_factorize(1)
        return cx.gp_predict_points(1, Xs, D, E)

    cx = _lib.Context(device=0)
    try:
        shared = [fitc(cx, Z30), fitc(cx, Z70), fitc(cx, Z30), rollout(cx), predict(cx)]
    finally:
        cx.close()
    fresh = []
    for step in (lambda c: fitc(c, Z30), lambda c: fitc(c, Z70), lambda c: fitc(c, Z30), rollout, predict):
        c = _lib.Context(device=0)
        try:
            fresh.append(step(c))
        finally:
            c.close()
    for i, (a, b) in enumerate(zip(shared, fresh)):
        try:
            _same(a, b)
        except AssertionError:
            raise AssertionError(f"step {i} differs from a fresh context's")
    _same(shared[0], shared[2])
    assert np.all(np.isfinite(shared[3][3]))


@pytest.mark.parametrize("cid", ["overflow_M70_N100_MpEqNp", "valu_D17"])
@pytest.mark.parametrize("nranks", [2, 3])
def test_sharded_fitc_objective_is_bit_identical(cid, nranks, monkeypatch):
    """_lib.group_fitc_nlml over contexts of one process that shard the outputs (a rank may own none: E = 2 over 3 ranks)."""
    from pilco_amd import _lib
    monkeypatch.delenv("PILCO_FITC_KGRAD_VALU", raising=False)
    prob, _ = _fitc_case(cid)
    X, Y, ls, var, noise, Z_all = prob
    D, E = X.shape[1], Y.shape[1]
    single = _fitc_on(_CTX, prob)
    made = []
    try:
        for r in range(nranks):
            c = _lib.Context(device=0)
            made.append(c)
            c.shard_set(r, nranks)
            c.gp_set_data(0, X, Y)
            c.gp_set_hyp(0, ls, var, noise)
        got = _lib.group_fitc_nlml(made, 0, Z_all, D, E)
    finally:
        for c in made:
            c.close()
    _same(single, got)


# ---------------------------------------------------------------------------------------------------------- exact GP
EXACT_CASES = ([(f"D{D}", 100, D, 3) for D in (1, 5, 8, 9, 12, 13, 16, 17, 24, 25, 32)]
               + [(f"N{N}", N, 4, 3) for N in (1, 63, 64, 65, 1000)]
               + [("E32", 90, 3, 32)])


@pytest.mark.parametrize("cid,N,D,E", EXACT_CASES, ids=[c[0] for c in EXACT_CASES])
def test_exact_objective_and_gradient_match_the_oracle(cid, N, D, E):
    X, Y, ls, var, noise, _ = _problem(N, 1, D, E, seed=1000 + N + 37 * D + E)
    _CTX.gp_set_data(0, X, Y)
    _CTX.gp_set_hyp(0, ls, var, noise)
    nlml, g = _CTX.gp_nlml(0, D, E)
    rn, rg = np.empty(E), np.empty((E, D + 2))
    for a in range(E):
        rn[a], rg[a] = nlml_and_grad(X, Y[:, a], ls[a], var[a], noise[a])
    np.testing.assert_allclose(nlml, rn, rtol=1e-9, atol=0)
    _check_grad(g, rg, np.abs(rg).max(1), "exact gradient")
