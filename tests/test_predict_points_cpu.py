"""GP posterior prediction at deterministic inputs (pilco_gp_predict_points, csrc/predict.hip), checked without a GPU:
  * the kernel's gfx950 code passes both MFMA scanners (tests/test_build_isa.py explains what they guard against);
  * the NumPy restatement the GPU tests measure against (tests/helpers/predict_restatement.py) is pinned to the executed
    reference: its predict_on_noisy_inputs(x, 0) gives M = k*^T beta and diag S = the latent variance (mgpr.py:91-149 with
    s = 0), for MGPR and for SMGPR with one shared Z.  Where the reference source is absent the stored end values of that
    execution (tests/golden/predict_points_reference.npz) stand in for it;
  * the restated GPRFITC with Z = X is the restated GPR up to the effect of the 1e-6 jitter."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from helpers.predict_restatement import fitc_predict_f, gpr_predict_f

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
STORED = os.path.join(GOLDEN, "predict_points_reference.npz")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_predict_kernel_compiles_and_passes_both_mfma_scanners(tmp_path):
    asm = str(tmp_path / "predict.s")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
           "-mllvm", "-amdgpu-mfma-vgpr-form", "-S", "--cuda-device-only", "-o", asm, os.path.join(ROOT, "pilco_amd", "csrc", "predict.hip")]
    pr = subprocess.run(cmd, capture_output=True, text=True, timeout=1500)
    assert pr.returncode == 0, pr.stderr[-2000:]
    text = open(asm).read()
    assert "k_predict_points" in text and "v_mfma_f64_16x16x4_f64" in text
    for tool in ("mfma_overlap_check.py", "mfma_hazard_check.py"):
        chk = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), asm], capture_output=True, text=True, timeout=300)
        assert chk.returncode == 0, "%s:\n%s" % (tool, chk.stdout[-3000:])


def _test_inputs(X, n, seed):
    rs = np.random.RandomState(seed)
    lo, hi = X.min(0), X.max(0)
    return lo + (hi - lo) * rs.rand(n, X.shape[1])


def _executed_reference():
    """The reference's own predict_on_noisy_inputs(x, 0) at single points: MGPR on the predictions.npz model, SMGPR (model
    0's Z serves every output, smgpr.py:47-52) on the sparse_predictions.npz model."""
    from oracle import ref_exec
    R = ref_exec.load()
    n_ = ref_exec.to_np
    out = {}
    for kind, name in (("exact", "predictions.npz"), ("sparse", "sparse_predictions.npz")):
        g = np.load(os.path.join(GOLDEN, name))
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
        xs = _test_inputs(g["X"], 6, 3)
        D = xs.shape[1]
        Ms, Ss = [], []
        for x in xs:
            M, S, _ = [n_(a) for a in mdl.predict_on_noisy_inputs(x.reshape(1, D), np.zeros((D, D)))]
            Ms.append(M.ravel())
            Ss.append(np.diag(S))
        out["x_" + kind], out["M_" + kind], out["S_" + kind] = xs, np.array(Ms), np.array(Ss)
    return out


def _reference_points():
    from oracle import ref_exec
    if not ref_exec.available():
        g = np.load(STORED)
        return {k: g[k] for k in g.files}
    live = _executed_reference()
    stored = np.load(STORED)
    for k, v in live.items():   # the stored end values are the executed reference's
        np.testing.assert_allclose(stored[k], v, rtol=1e-12, atol=1e-14)
    return live


@pytest.mark.parametrize("kind", ["exact", "sparse"])
def test_restatement_matches_the_executed_reference_at_zero_input_variance(kind):
    ref = _reference_points()
    name = "predictions.npz" if kind == "exact" else "sparse_predictions.npz"
    g = np.load(os.path.join(GOLDEN, name))
    xs = ref["x_" + kind]
    args = (g["X"], g["Y"], g["lengthscales"], g["variance"], g["noise"])
    if kind == "exact":
        mean, var = gpr_predict_f(*args, xs)
    else:
        mean, var = fitc_predict_f(g["X"], g["Y"], g["Z"], g["lengthscales"], g["variance"], g["noise"], xs)
    M, S = ref["M_" + kind].T, ref["S_" + kind].T   # (E, Nt)
    # the reference forms S as beta^T Q beta - M^2 + ..., which cancels: its error is relative to max(sf2, M^2)
    scale = np.maximum(g["variance"][:, None], M * M)
    assert np.all(np.abs(mean - M) <= 1e-10 * scale)
    assert np.all(np.abs(var - S) <= 1e-10 * scale)


def test_restated_fitc_with_z_equal_x_is_the_restated_gpr_up_to_the_jitter():
    g = np.load(os.path.join(GOLDEN, "predictions.npz"))
    X, Y, ls, sf2 = g["X"][:60], g["Y"][:60], g["lengthscales"], g["variance"]
    nz = np.full(Y.shape[1], 1e-2)
    xs = _test_inputs(X, 40, 5)
    m0, v0 = gpr_predict_f(X, Y, ls, sf2, nz, xs)
    m1, v1 = fitc_predict_f(X, Y, X, ls, sf2, nz, xs)
    m2, v2 = fitc_predict_f(X, Y, X, ls, sf2, nz, xs, jitter=1e-9)
    d1 = max(np.abs(m1 - m0).max() / np.abs(m0).max(), np.abs(v1 - v0).max() / sf2.max())
    d2 = max(np.abs(m2 - m0).max() / np.abs(m0).max(), np.abs(v2 - v0).max() / sf2.max())
    assert d1 < 1e-3          # the jitter moves the answer by about jitter / noise ...
    assert d2 < d1 / 30       # ... and by proportionally less as it shrinks: Z = X with no jitter is the exact GP
