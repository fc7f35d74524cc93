"""The yardsticks of the device training objectives (tests/test_gpu_training_objectives.py) held to the executed reference:
the torch restatement of gpflow GPRFITC's loss in tests/helpers/fitc_objective.py against tests/golden/fitc_objective.npz,
its autograd gradient against central differences of the NumPy value, and the exact-GP oracle (oracle/gp_train.py) at the
end point of the executed reference's model fit (tests/golden/models_optimisation.npz)."""
import os

import numpy as np
import pytest

from helpers.cpu_objective_context import CpuObjectiveContext
from helpers.fitc_objective import fitc_grad_fd, fitc_loss_and_grad, fitc_loss_np, fitc_reference
from oracle.gp_train import nlml_and_grad
from pilco_amd.training import _dsoftplus, _gamma_logpdf_and_grad, _softplus_inv

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_fitc_helper_equals_the_executed_reference():
    g = np.load(os.path.join(GOLDEN, "fitc_objective.npz"))
    nlml, gh, gz = fitc_reference(g["X"], g["Y"], g["Z_all"], g["lengthscales"], g["variance"], g["noise"])
    np.testing.assert_allclose(nlml, g["loss"], rtol=1e-10, atol=0)
    np.testing.assert_allclose(gh[:, :3], g["dloss_dls"], rtol=1e-10, atol=0)
    np.testing.assert_allclose(gh[:, 3], g["dloss_dvar"], rtol=1e-10, atol=0)
    np.testing.assert_allclose(gh[:, 4], g["dloss_dnoise"], rtol=1e-10, atol=0)
    np.testing.assert_allclose(gz, g["dloss_dZ"], rtol=1e-10, atol=1e-10 * np.abs(g["dloss_dZ"]).max())
    for e in range(2):
        np.testing.assert_allclose(fitc_loss_np(g["X"], g["Y"][:, e], g["Z_all"][e], g["lengthscales"][e], g["variance"][e], g["noise"][e]),
                                   g["loss"][e], rtol=1e-10)


def test_cpu_objective_context_uses_the_helper():
    """The model fits' CPU stand-in returns the helper's numbers, bit for bit."""
    g = np.load(os.path.join(GOLDEN, "fitc_objective.npz"))
    cx = CpuObjectiveContext()
    cx.gp_set_data(0, g["X"], g["Y"])
    cx.gp_set_hyp(0, g["lengthscales"], g["variance"], g["noise"])
    got = cx.gp_fitc_nlml(0, g["Z_all"], 3, 2)
    want = fitc_reference(g["X"], g["Y"], g["Z_all"], g["lengthscales"], g["variance"], g["noise"])
    for a, b in zip(got, want):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("N,M,D,seed", [(40, 7, 2, 1), (33, 12, 4, 2)])
def test_fitc_autograd_gradient_equals_central_differences(N, M, D, seed):
    rs = np.random.RandomState(seed)
    X = rs.randn(N, D)
    y = np.sin(X @ rs.randn(D)) + 0.05 * rs.randn(N)
    Z = X[rs.choice(N, M, replace=False)] + 0.1 * rs.randn(M, D)
    ls, var, noise = 0.8 + rs.rand(D), 0.7 + rs.rand(), 0.01 + 0.05 * rs.rand()
    f, dls, dvar, dnoise, dZ = fitc_loss_and_grad(X, y, Z, ls, var, noise)
    np.testing.assert_allclose(f, fitc_loss_np(X, y, Z, ls, var, noise), rtol=1e-12)
    fls, fvar, fnoise, fZ = fitc_grad_fd(X, y, Z, ls, var, noise)
    scale = max(np.abs(dls).max(), abs(dvar), abs(dnoise), np.abs(dZ).max())
    for a, b in [(dls, fls), (dvar, fvar), (dnoise, fnoise), (dZ, fZ)]:
        np.testing.assert_allclose(a, b, rtol=1e-6, atol=1e-6 * scale)


@pytest.mark.parametrize("prefix", ["", "r_"])
def test_exact_oracle_at_the_executed_reference_end_point(prefix):
    """models_optimisation.npz keeps the end point of the reference's MAP fit and its loss (the NLML minus the Gamma log-priors
    on the lengthscales and the kernel variance, mgpr.py:33-34): the oracle gives that loss, and at the end point the MAP
    gradient in the optimiser's softplus coordinates is near zero.  (The fixture stores no gradient: L-BFGS-B stops at its
    tolerance, so stationarity is checked loosely.)"""
    g = np.load(os.path.join(GOLDEN, "models_optimisation.npz"))
    for a in range(g["Y"].shape[1]):
        ls, var, noise = g[prefix + "ls_end"][a], float(g[prefix + "var_end"][a]), float(g[prefix + "noise_end"][a])
        f, grad = nlml_and_grad(g["X"], g["Y"][:, a], ls, var, noise)
        lp_l, dlp_l = _gamma_logpdf_and_grad(ls, 1.1, 0.1)
        lp_v, dlp_v = _gamma_logpdf_and_grad(var, 1.5, 0.5)
        np.testing.assert_allclose(f - lp_l.sum() - lp_v, g[prefix + "loss_end"][a], rtol=1e-12)
        gu = np.concatenate([(grad[:3] - dlp_l) * _dsoftplus(_softplus_inv(ls)), [(grad[3] - dlp_v) * _dsoftplus(_softplus_inv(var))],
                             [grad[4] * _dsoftplus(_softplus_inv(noise - 1e-6))]])
        assert np.abs(gu).max() < 1e-3, gu
