"""Input Jacobians of the GP posterior (pilco_gp_predict_points_jac, csrc/predict_jac.hip; docs/predict_jacobians.md),
checked without a GPU:
  * the yardstick of the GPU tests, tests/helpers/predict_jac_restatement.py (Cholesky factors and triangular solves), agrees
    with torch autograd through a float64 torch transcription of the VALUE restatement (helpers/predict_restatement.py), for
    GPR and FITC with shared and per-output Z; three mutants of it (sign of X - x, l for l^2, the factor 2) do not;
  * its mean Jacobian is the third output V of the executed reference's predict_on_noisy_inputs(x, 0) (mgpr.py:102-118 at
    s = 0: V = sum_i (X_i - m) / l^2 beta_i k_i), MGPR and SMGPR; skipped where the reference source is absent;
  * its variance Jacobian against a 40-digit evaluation of -2 sum_i a_i k_i (X_id - x_d) / l_d^2 on the low-noise model;
  * action_jacobian of both controllers against autograd through the action formula of docs/particles.md;
  * the kernel's gfx950 code passes both MFMA scanners; the header declares the entry point, the binding carries it.
Bounds: two float64 routes through factors of condition up to 1e9 (the low-noise model) differ by a few 1e-10 of the scale of
the result (measured 6e-10 there, 5e-12 on predictions.npz); 1e-8 of that scale is what the device is held to, and the
yardstick must leave it room: 1e-9 against autograd on the well-conditioned models, 1e-8 against the 40-digit truth."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from helpers import predict_jac_restatement as jr
from pilco_amd import synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _g(name):
    g = np.load(os.path.join(GOLDEN, name))
    return {k: g[k] for k in g.files if k != "provenance"}


def _inputs(X, n, seed):
    rs = np.random.RandomState(seed)
    lo, hi = X.min(0), X.max(0)
    return lo + (hi - lo) * rs.rand(n, X.shape[1])


# ------------------------------------------------------------------ torch transcription of helpers/predict_restatement.py
def _t_se(torch, A, B, ls, var):
    d = (A[:, None, :] - B[None, :, :]) / ls
    return var * torch.exp(-0.5 * torch.sum(d * d, dim=-1))


def _t_gpr(torch, X, y, ls, sf2, sn2, Xs):
    L = torch.linalg.cholesky(_t_se(torch, X, X, ls, sf2) + sn2 * torch.eye(X.shape[0], dtype=torch.float64))
    A = torch.linalg.solve_triangular(L, _t_se(torch, X, Xs, ls, sf2), upper=False)
    mean = A.T @ torch.linalg.solve_triangular(L, y[:, None], upper=False)[:, 0]
    return mean, sf2 - torch.sum(A * A, dim=0)


def _t_fitc(torch, X, y, Z, ls, sf2, sn2, Xs, jitter=1e-6):
    eye = torch.eye(Z.shape[0], dtype=torch.float64)
    Luu = torch.linalg.cholesky(_t_se(torch, Z, Z, ls, sf2) + jitter * eye)
    V = torch.linalg.solve_triangular(Luu, _t_se(torch, Z, X, ls, sf2), upper=False)
    nu = sf2 - torch.sum(V * V, dim=0) + sn2
    LB = torch.linalg.cholesky(eye + (V / nu) @ V.T)
    gamma = torch.linalg.solve_triangular(LB, (V @ (y / nu))[:, None], upper=False)[:, 0]
    w = torch.linalg.solve_triangular(Luu, _t_se(torch, Z, Xs, ls, sf2), upper=False)
    tmp = torch.linalg.solve_triangular(LB, w, upper=False)
    return tmp.T @ gamma, sf2 - torch.sum(w * w, dim=0) + torch.sum(tmp * tmp, dim=0)


def _autograd(cfg, xs, Z=None):
    """(dmean, dvar) (E, Nt, D) by autograd: every test point enters its own mean and variance only, so the gradient of
    the sum over the points is the per-point Jacobian."""
    import torch
    t = lambda a: torch.tensor(np.asarray(a, np.float64))
    X, Y = t(cfg["X"]), t(cfg["Y"])
    E = Y.shape[1]
    dm, dv = [], []
    for e in range(E):
        ls, sf2, sn2 = t(cfg["lengthscales"][e]), t(cfg["variance"][e]), t(cfg["noise"][e])
        for which, out in ((0, dm), (1, dv)):
            x = t(xs).requires_grad_(True)
            if Z is None:
                r = _t_gpr(torch, X, Y[:, e], ls, sf2, sn2, x)
            else:
                Ze = t(Z[e] if np.ndim(Z) == 3 else Z)
                r = _t_fitc(torch, X, Y[:, e], Ze, ls, sf2, sn2, x)
            r[which].sum().backward()
            out.append(x.grad.numpy().copy())
    return np.stack(dm), np.stack(dv)


def _scales(cfg, ref_dmean):
    """per output: max |dmean_e| and sf2_e / min_d l_ed, the scales of the GPU test's bounds"""
    return np.abs(ref_dmean).max(axis=(1, 2)), np.asarray(cfg["variance"]) / np.asarray(cfg["lengthscales"]).min(axis=1)


def _own_z(Z0, E, seed):
    rs = np.random.RandomState(seed)
    return np.stack([Z0] + [rs.rand(*Z0.shape) for _ in range(E - 1)])


def _cases():
    sp = _g("sparse_predictions.npz")
    return [("predictions", _g("predictions.npz"), None), ("sparse_shared_z", sp, sp["Z"]),
            ("sparse_own_z", sp, _own_z(sp["Z"], 2, 4)), ("c2_n300", synthetic.config_c2(N=300), None)]


def _restated(cfg, xs, Z):
    args = (cfg["lengthscales"], cfg["variance"], cfg["noise"], xs)
    if Z is None:
        return jr.gpr_predict_f_jac(cfg["X"], cfg["Y"], *args)
    return jr.fitc_predict_f_jac(cfg["X"], cfg["Y"], Z, *args)


_AUTOGRAD = {}


def _autograd_of(name, cfg, Z):
    """autograd's Jacobians of a case, computed once and shared by the agreement test and the mutant guard"""
    if name not in _AUTOGRAD:
        xs = _inputs(cfg["X"], 12, 5)
        _AUTOGRAD[name] = (xs,) + _autograd(cfg, xs, Z)
    return _AUTOGRAD[name]


def _worst(name, cfg, Z):
    """largest error of the restated Jacobians against autograd's, in units of the two scales"""
    xs, dm_ag, dv_ag = _autograd_of(name, cfg, Z)
    _, _, dm, dv = _restated(cfg, xs, Z)
    sm, sv = _scales(cfg, dm_ag)
    return (np.abs(dm - dm_ag).max(axis=(1, 2)) / sm).max(), (np.abs(dv - dv_ag).max(axis=(1, 2)) / sv).max()


@pytest.mark.parametrize("case", _cases(), ids=lambda c: c[0])
def test_restatement_matches_torch_autograd(case):
    name, cfg, Z = case
    em, ev = _worst(name, cfg, Z)
    print("%s: restatement vs autograd: dmean %.2e, dvar %.2e of their scales" % (name, em, ev))
    assert em <= 1e-9 and ev <= 1e-9
    # the values it returns beside them are the value restatement's
    from helpers.predict_restatement import fitc_predict_f, gpr_predict_f
    xs = _autograd_of(name, cfg, Z)[0]
    args = (cfg["lengthscales"], cfg["variance"], cfg["noise"], xs)
    m0, v0 = gpr_predict_f(cfg["X"], cfg["Y"], *args) if Z is None else fitc_predict_f(cfg["X"], cfg["Y"], Z, *args)
    m1, v1, _, _ = _restated(cfg, xs, Z)
    assert np.array_equal(m0, m1) and np.array_equal(v0, v1)


@pytest.mark.parametrize("mutant", ["sign", "l_for_l2", "no_factor_2"])
def test_mutants_of_the_restatement_fail_the_autograd_check(mutant, monkeypatch):
    if mutant == "sign":
        monkeypatch.setattr(jr, "SIGN", -1.0)
    elif mutant == "l_for_l2":
        monkeypatch.setattr(jr, "LS_POWER", 1)
    else:
        monkeypatch.setattr(jr, "VAR_FACTOR", 1.0)
    for name, cfg, Z in _cases():
        em, ev = _worst(name, cfg, Z)
        assert max(em, ev) > 1e-3, (mutant, name, em, ev)   # far outside the 1e-9 of the check above, on every case


def _reference_models():
    from oracle import ref_exec
    R = ref_exec.load()
    out = []
    for kind, name in (("exact", "predictions.npz"), ("sparse", "sparse_predictions.npz")):
        g = _g(name)
        if kind == "exact":
            mdl = R.MGPR((g["X"], g["Y"]))
        else:
            np.random.seed(11)
            mdl = R.SMGPR((g["X"], g["Y"]), num_induced_points=g["Z"].shape[0])
            for m in mdl.models:
                m.inducing_variable.Z.assign(g["Z"])
        for i, m in enumerate(mdl.models):
            m.kernel.lengthscales.assign(g["lengthscales"][i])
            m.kernel.variance.assign(g["variance"][i])
            m.likelihood.variance.assign(g["noise"][i])
        out.append((kind, g, mdl))
    return out


def test_mean_jacobian_is_the_executed_references_input_output_covariance_at_zero_variance():
    from oracle import ref_exec
    if not ref_exec.available():
        pytest.skip("the reference source is not on this machine")
    for kind, g, mdl in _reference_models():
        xs = _inputs(g["X"], 6, 3)
        D = xs.shape[1]
        Z = None if kind == "exact" else g["Z"]
        _, _, dm, _ = _restated(g, xs, Z)
        for t, x in enumerate(xs):
            V = ref_exec.to_np(mdl.predict_on_noisy_inputs(x.reshape(1, D), np.zeros((D, D)))[2])   # (D, E)
            err = np.abs(dm[:, t, :] - V.T).max(axis=1) / np.abs(dm).max(axis=(1, 2))
            assert np.all(err <= 1e-8), (kind, t, err)


def test_variance_jacobian_against_a_40_digit_evaluation_on_the_low_noise_model():
    cfg = _g("predictions_lownoise.npz")
    X, ls, sf2 = cfg["X"], cfg["lengthscales"], cfg["variance"]
    xs = _inputs(X, 5, 9)
    truth_m, truth_v = jr.mp_jacobians(cfg, xs)
    _, _, dm, dv = jr.gpr_predict_f_jac(X, cfg["Y"], ls, sf2, cfg["noise"], xs)
    sm, sv = _scales(cfg, truth_m)
    em = np.abs(dm - truth_m).max(axis=(1, 2)) / sm
    ev = np.abs(dv - truth_v).max(axis=(1, 2)) / sv
    print("low noise, restatement vs 40 digits: dmean %s, dvar %s of their scales" % (em, ev))
    assert np.all(em <= 1e-8) and np.all(ev <= 1e-8)


def test_action_jacobians_against_autograd_through_the_action_formula():
    import torch
    from pilco_amd.controllers import LinearController, RbfController
    rs = np.random.RandomState(3)
    E, U = 4, 2
    lin = LinearController(E, U, max_action=np.array([1.3, 0.7]))
    lin.W.assign(rs.randn(U, E))
    lin.b.assign(rs.randn(1, U))
    t = lambda a: torch.tensor(np.asarray(a, np.float64))
    for x in rs.randn(3, E):
        f = lambda xx: t(lin.max_action) * torch.sin(t(lin.W.numpy()) @ xx + t(lin.b.numpy()).reshape(-1))
        J = torch.autograd.functional.jacobian(f, t(x)).numpy()
        got = lin.action_jacobian(x)
        assert got.shape == (U, E)
        np.testing.assert_allclose(got, J, rtol=1e-12, atol=1e-14)
    g = _g("rbf_controller.npz")
    C, Y = g["X"], g["Y"]
    rbf = RbfController(C.shape[1], Y.shape[1], C.shape[0], max_action=2.0)
    rbf.set_data((C, Y))
    for i, m in enumerate(rbf.models):
        m.kernel.lengthscales.assign(g["lengthscales"][i])
    noise = np.asarray(rbf.noise).reshape(-1)

    def act(xx):
        out = []
        for k in range(Y.shape[1]):
            ls = t(g["lengthscales"][k])
            K = _t_se(torch, t(C), t(C), ls, 1.0) + noise[k] * torch.eye(C.shape[0], dtype=torch.float64)
            beta = torch.linalg.solve(K, t(Y[:, k]))
            out.append(2.0 * np.exp(-5e-7) * torch.sin(_t_se(torch, xx[None, :], t(C), ls, 1.0)[0] @ beta))
        return torch.stack(out)

    for x in _inputs(C, 3, 2):
        J = torch.autograd.functional.jacobian(act, t(x)).numpy()
        got = rbf.action_jacobian(x)
        assert got.shape == (Y.shape[1], C.shape[1])
        assert np.abs(got - J).max() <= 1e-9 * np.abs(J).max()   # (beta through a solve of condition ~1e4 on both sides)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_jacobian_kernel_compiles_and_passes_both_mfma_scanners(tmp_path):
    asm = str(tmp_path / "predict_jac.s")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
           "-mllvm", "-amdgpu-mfma-vgpr-form", "-S", "--cuda-device-only", "-o", asm,
           os.path.join(ROOT, "pilco_amd", "csrc", "predict_jac.hip")]
    pr = subprocess.run(cmd, capture_output=True, text=True, timeout=1500)
    assert pr.returncode == 0, pr.stderr[-2000:]
    text = open(asm).read()
    assert "k_predict_points_jac" in text and "v_mfma_f64_16x16x4_f64" in text
    assert re.search(r"\.private_segment_fixed_size:\s*0\b", text) and not re.search(r"\.private_segment_fixed_size:\s*[1-9]", text)   # no scratch
    for tool in ("mfma_overlap_check.py", "mfma_hazard_check.py"):
        chk = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), asm], capture_output=True, text=True, timeout=300)
        assert chk.returncode == 0, "%s:\n%s" % (tool, chk.stdout[-3000:])


def test_header_declares_the_entry_point_and_the_binding_carries_it():
    from pilco_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "pilco_hip.h")).read()
    assert re.search(r"int pilco_gp_predict_points_jac\(pilco_ctx\* ctx, int slot, const double\* Xs, int Nt, int output, "
                     r"const double\* Z_all,\s+double\* mean, double\* var, double\* dmean, double\* dvar\);", hdr)
    assert re.search(r"#define PILCO_HIP_ABI_VERSION 2\b", hdr)
    assert len(_lib.SIGNATURES["pilco_gp_predict_points_jac"][1]) == 10
    assert hasattr(_lib.Context, "gp_predict_points_jac")


def test_linearize_refuses_actions_that_do_not_fit_the_model_before_any_device_call():
    from pilco_amd.models import PILCO
    rs = np.random.RandomState(0)
    free = PILCO((rs.rand(20, 3), rs.rand(20, 3)))           # no control input
    with pytest.raises(ValueError, match="no control input"):
        free.linearize(np.zeros(3), np.zeros(1))
    with pytest.raises(ValueError, match="x must be"):
        free.linearize(np.zeros(4))
    ctl = PILCO((rs.rand(20, 4), rs.rand(20, 3)))            # one control input
    for x, u in ((np.zeros((2, 3)), np.zeros((3, 1))), (np.zeros((2, 3)), np.zeros((2, 2))), (np.zeros(3), np.zeros((1, 1)))):
        with pytest.raises(ValueError, match="u must be"):
            ctl.linearize(x, u)
    ctl.controller = None
    with pytest.raises(ValueError, match="no controller"):
        ctl.linearize(np.zeros(3))
