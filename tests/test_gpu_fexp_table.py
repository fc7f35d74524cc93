"""GPU checks of the pair kernels' table exp with the biased table (the exponent inserted into the table value before the
final FMA, csrc/mm_device.h: fexp_scale): the self-test over [-720, 700], a state far from the training data (exponents
below the -700 clamp) against the NumPy oracle, and bitwise repeatability of the headline rollout."""
import numpy as np
import pytest

from oracle import tf_path as tp
from pilco_amd import synthetic

pytestmark = pytest.mark.gpu
RTOL = 1e-5


@pytest.fixture(scope="module")
def ctx():
    from pilco_amd import _lib
    return _lib.get_context()


def _mgpr(cfg):
    from pilco_amd.models import MGPR
    m = MGPR((cfg["X"], cfg["Y"]))
    for i, mdl in enumerate(m.models):
        mdl.kernel.lengthscales.assign(cfg["lengthscales"][i])
        mdl.kernel.variance.assign(cfg["variance"][i])
        mdl.likelihood.variance.assign(cfg["noise"][i])
    return m


def test_fexp_selftest_over_full_range(ctx):
    ctx.selftest()   # k_selftest_fexp: x over [-720, 700] against the library exp, then the MFMA layout


def test_far_state_takes_the_clamp_and_matches_oracle(ctx):
    """N = 1000, D = E = 10 (the stream-K pair kernel) with the mean 24 units out in every coordinate: most exponents of
    the pair sums lie below -700 (clamped), the nearest points' above it."""
    c = synthetic.config_c2()
    m0 = np.full((1, 10), 24.0)
    S0 = 0.1 * np.eye(10)
    Xc = c["X"] - m0
    z2 = (Xc ** 2) @ (1.0 / c["lengthscales"] ** 2).T          # [N, E]: z' Lambda_a^-1 z
    assert z2.min() < 1400.0 and z2.max() > 1400.0             # pair exponents ~ -(z_a + z_b) / 2 straddle -700
    m = _mgpr(c)
    iK, beta = tp.calculate_factorizations(c["X"], c["Y"], c["lengthscales"], c["variance"], c["noise"])
    M, S, V = m.predict_on_noisy_inputs(m0, S0)
    Mo, So, Vo = tp.predict_given_factorizations_pairs(c["X"], c["lengthscales"], c["variance"], m0, S0, iK, beta)
    assert np.all(np.isfinite(M)) and np.all(np.isfinite(S)) and np.all(np.isfinite(V))
    np.testing.assert_allclose(M, Mo, rtol=RTOL, atol=1e-12)
    np.testing.assert_allclose(S, So, rtol=RTOL, atol=1e-10)
    np.testing.assert_allclose(V, Vo, rtol=RTOL, atol=1e-12)
    M2, S2, V2 = m.predict_on_noisy_inputs(m0, S0)
    assert np.array_equal(M, M2) and np.array_equal(S, S2) and np.array_equal(V, V2)


def test_headline_rollout_bitwise_repeatable(ctx):
    from pilco_amd import _lib
    c = synthetic.config_c2()
    cx = _lib.Context()
    cx.gp_set_data(0, c["X"], c["Y"])
    cx.gp_set_hyp(0, c["lengthscales"], c["variance"], c["noise"])
    cx.gp_factorize(0)
    pol = dict(kind=_lib.POLICY_NONE, state_dim=10, control_dim=0)
    rw = [dict(kind=_lib.REWARD_EXPONENTIAL, coef=1.0, W=np.eye(10), t=np.zeros(10))]
    a = cx.rollout(pol, rw, c["m0"], c["S0"], 40)
    b = cx.rollout(pol, rw, c["m0"], c["S0"], 40)
    assert all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))
