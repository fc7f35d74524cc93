"""Particle rollouts (pilco_rollout_particles, csrc/particles.hip) checked without a GPU:
  * the random stream: csrc/philox_normal.h compiled into a host probe gives the Random123 known answers of Philox4x32-10, the
    words of the Python restatement (tests/helpers/particles_restatement.py) exactly, and its normals within the bound the GPU
    seed-path test uses;
  * the restatement of one particle step is pinned to the executed reference (PILCO.propagate(x, 0) and compute_action(x, 0),
    tests/helpers/particles_reference.py); where the reference source is absent the stored end values of that execution
    (tests/golden/particles_reference.npz) stand in for it;
  * particles.hip compiles for gfx950 and passes both MFMA scanners (it holds no MFMA kernel of its own: the walk it calls
    is predict.hip's, scanned by tests/test_predict_points_cpu.py);
  * the header declares the entry point, the binding carries its signature.

WHERE THE OFF-DIAGONALS OF S CAN BE HELD TO 1e-12 sf2.  The reference forms S_ab = beta_a^T L beta_b - M_a M_b: at s = 0 two
equal products of the sums M_a = sum_i beta_ai k_ai, which cancel.  Its own rounding is therefore of the order
rho = 2^-53 (sum_i |beta_ai k_ai|) (sum_j |beta_bj k_bj|), a figure known BEFORE the reference is executed (beta and k from the
restatement).  On the predictions.npz model as stored (likelihood variance 1e-4, |beta| ~ 1e3) rho = 1.2e-10: a hundred times
the bound, so there the bound would measure the reference's cancellation, not the structure of the step (the executed
reference gives 2.4e-11 there, inside rho).  The bound is held on models whose rho is at most a tenth of it: the same data
and kernels with likelihood variance 0.1 ("exact_n", rho = 2.7e-14) and the sparse model; on the stored model the
off-diagonals are held to rho itself.  M - x and diag S are held to 1e-9 relative on all three."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from helpers import particles_reference as pref
from helpers import particles_restatement as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CSRC = os.path.join(ROOT, "pilco_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# ------------------------------------------------------------------ the random stream
PROBE = r'''#include <cstdio>
#include <cstdlib>
#include "philox_normal.h"
using namespace pilco;
int main(int argc, char** argv) {
    if (atoi(argv[1]) == 0) {   // raw blocks: c0 c1 c2 c3 k0 k1 (hex)
        for (int i = 2; i + 5 < argc; i += 6) {
            uint32_t v[6];
            for (int k = 0; k < 6; ++k) v[k] = (uint32_t)strtoul(argv[i + k], nullptr, 16);
            const PhiloxWords w = philox4x32_10(v[0], v[1], v[2], v[3], v[4], v[5]);
            std::printf("%08x %08x %08x %08x\n", w.w[0], w.w[1], w.w[2], w.w[3]);
        }
        return 0;
    }
    unsigned long long seed;
    unsigned t, p, j;
    while (std::scanf("%llu %u %u %u", &seed, &t, &p, &j) == 4) {
        const PhiloxWords w = philox_particle_words(seed, t, p, j);
        double z0, z1;
        philox_normal_pair(seed, t, p, j, &z0, &z1);
        std::printf("%08x %08x %08x %08x %.17g %.17g\n", w.w[0], w.w[1], w.w[2], w.w[3], z0, z1);
    }
    return 0;
}
'''
KNOWN_ANSWERS = [   # Random123 kat_vectors, philox4x32 10 rounds: counter, key -> words
    ("00000000 00000000 00000000 00000000", "00000000 00000000", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("philox_probe")
    src = d / "philox_probe.hip"
    src.write_text(PROBE)
    exe = d / "philox_probe"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-I" + CSRC, "-I/opt/rocm/include", str(src), "-o", str(exe)],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(exe)


def test_python_philox_gives_the_random123_known_answers():
    for ctr, key, want in KNOWN_ANSWERS:
        got = pr.philox4x32_10([int(w, 16) for w in ctr.split()], [int(w, 16) for w in key.split()])
        assert " ".join("%08x" % w for w in got) == want


def test_probe_philox_gives_the_random123_known_answers(probe):
    args = [w for ctr, key, _ in KNOWN_ANSWERS for w in (ctr + " " + key).split()]
    out = subprocess.run([probe, "0"] + args, capture_output=True, text=True, timeout=60, check=True).stdout.strip().split("\n")
    assert out == [want for _, _, want in KNOWN_ANSWERS]


def _stream_cases():
    rs = np.random.RandomState(17)
    cases = [(0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (2 ** 64 - 1, 39, 4096, 15), (2 ** 32, 3, 7, 2)]
    for _ in range(400):
        cases.append((int(rs.randint(0, 2 ** 31)) * int(rs.randint(1, 2 ** 31)) + int(rs.randint(0, 2 ** 31)),
                      int(rs.randint(0, 200)), int(rs.randint(0, 200000)), int(rs.randint(0, 16))))
    return cases


def test_probe_words_and_normals_match_the_python_restatement(probe):
    cases = _stream_cases()
    txt = "".join("%d %d %d %d\n" % c for c in cases)
    out = subprocess.run([probe, "1"], input=txt, capture_output=True, text=True, timeout=60, check=True).stdout.strip().split("\n")
    assert len(out) == len(cases)
    worst = 0.0
    for (seed, t, p, j), line in zip(cases, out):
        f = line.split()
        assert tuple(int(w, 16) for w in f[:4]) == pr.particle_words(seed, t, p, j), (seed, t, p, j)
        z0, z1, r = pr.normal_pair(seed, t, p, j)
        bound = 16 * 2.0 ** -53 * max(1.0, r)   # log, sin, cos within 2 ulp each and the rounding of 2 pi u2, with margin
        for got, want in ((float(f[4]), z0), (float(f[5]), z1)):
            assert abs(got - want) <= bound, (seed, t, p, j, got, want)
            worst = max(worst, abs(got - want) / bound)
    print("host probe normals: largest |dz| / bound = %.3g" % worst)


def test_uniforms_stay_inside_their_intervals():
    assert pr.uniforms((0, 0, 0, 0)) == (1.0, 0.0)
    u1, u2 = pr.uniforms((0xFFFFFFFF,) * 4)
    assert u1 == 2.0 ** -53 and u2 == 1.0 - 2.0 ** -53


# ------------------------------------------------------------------ the restatement against the executed reference
@pytest.fixture(scope="module")
def ref():
    return pref.reference_values()


def _model(kind):
    g = np.load(os.path.join(GOLDEN, "sparse_predictions.npz" if kind == "sparse" else "predictions.npz"))
    m = {k: g[k] for k in ("X", "Y", "lengthscales", "variance", "noise")}
    if kind == "exact_n":
        m["noise"] = np.full(m["variance"].shape, pref.EXACT_N_NOISE)
    m["Z"] = g["Z"] if kind == "sparse" else None
    return m


def _reference_rounding(model, x):
    """rho = 2^-53 max over the points of (sum_i |beta_ai k_ai|) (sum_j |beta_bj k_bj|), a != b: the order of the rounding in
    the reference's S_ab = beta_a^T L beta_b - M_a M_b at s = 0 (exact GP), from the restated beta and k alone."""
    from helpers.predict_restatement import se_ard
    X, Y = model["X"], model["Y"]
    xu = np.concatenate([x, pr.action(STEP_POLICY, x)], axis=1)
    A = []
    for e in range(Y.shape[1]):
        K = se_ard(X, X, model["lengthscales"][e], model["variance"][e]) + model["noise"][e] * np.eye(X.shape[0])
        A.append(np.abs(se_ard(xu, X, model["lengthscales"][e], model["variance"][e]) * np.linalg.solve(K, Y[:, e])).sum(axis=1))
    E = len(A)
    return 2.0 ** -53 * max((A[a] * A[b]).max() for a in range(E) for b in range(E) if a != b)


STEP_POLICY = dict(kind="linear", W=pref.STEP_W, b=pref.STEP_B, max_action=pref.STEP_MAX_ACTION)


@pytest.mark.parametrize("kind", ["exact", "exact_n", "sparse"])
def test_restated_step_matches_the_executed_propagate_at_zero_input_variance(ref, kind):
    """propagate(x, 0) = (x + mu, S) with diag S the latent variance: M - x and diag S to 1e-9 relative (relative to the
    scale the reference's own cancelling sums run at, max(sf2, mu^2), as in tests/test_predict_points_cpu.py)."""
    model = _model(kind)
    x, M, S = ref["x_" + kind], ref["M_" + kind], ref["S_" + kind]
    assert x.shape[0] == 6
    xn, mu, v, _ = pr.step(model, STEP_POLICY, x, np.zeros_like(x))
    assert np.array_equal(xn, x + mu)
    scale = np.maximum(model["variance"][None, :], mu * mu)
    assert np.all(np.abs((M - x) - mu) <= 1e-9 * scale)
    assert np.all(np.abs(np.diagonal(S, axis1=1, axis2=2) - v) <= 1e-9 * scale)


def _largest_off_diagonal(S):
    E = S.shape[1]
    return max(abs(S[:, a, b]).max() for a in range(E) for b in range(E) if a != b)


@pytest.mark.parametrize("kind", ["exact_n", "sparse"])
def test_reference_step_covariance_is_diagonal(ref, kind):
    """At s = 0 the moment-matching step is the product of the outputs' posteriors: the off-diagonals of S are below
    1e-12 sf2 (of the smaller sf2), at six points each, on the models where the reference's own rounding lets the bound be
    resolved (module docstring)."""
    model = _model(kind)
    S = ref["S_" + kind]
    assert S.shape[0] == 6
    bound = 1e-12 * model["variance"].min()
    if kind == "exact_n":
        assert _reference_rounding(model, ref["x_" + kind]) <= 0.1 * bound
    off = _largest_off_diagonal(S)
    print("%s: largest off-diagonal of S = %.3g (bound %.3g)" % (kind, off, bound))
    assert off < bound


def test_reference_rounding_decides_where_the_off_diagonal_bound_is_held(ref):
    """On the predictions.npz model as stored the reference's own rounding, known a priori, is far above 1e-12 sf2: the
    off-diagonals of its S are held to that rounding instead (and are not exactly zero: the check sees them)."""
    model = _model("exact")
    rho = _reference_rounding(model, ref["x_exact"])
    off = _largest_off_diagonal(ref["S_exact"])
    print("exact: rho = %.3g, largest off-diagonal of S = %.3g, 1e-12 sf2 = %.3g" % (rho, off, 1e-12 * model["variance"].min()))
    assert rho > 50 * 1e-12 * model["variance"].min()
    assert 0 < off <= rho


def test_restated_actions_match_the_executed_compute_action(ref):
    """compute_action(x, 0)[0] to 1e-12 relative: LinearController, and RbfController (which pins the exp(-0.5e-6) of the
    1e-6 variance the reference leaves at s = 0: without it the actions differ by 5e-7 relative)."""
    g = np.load(os.path.join(GOLDEN, "linear_controller.npz"))
    u = pr.linear_action(ref["x_linear"], g["W"], g["b"], pref.ACTION_MAX)
    assert ref["u_linear"].shape == (6, 2)
    np.testing.assert_allclose(u, ref["u_linear"], rtol=1e-12, atol=0)
    g = np.load(os.path.join(GOLDEN, "rbf_controller.npz"))
    u = pr.rbf_action(ref["x_rbf"], g["X"], g["Y"], g["lengthscales"], g["noise"], pref.ACTION_MAX)
    assert ref["u_rbf"].shape == (6, 2)
    np.testing.assert_allclose(u, ref["u_rbf"], rtol=1e-12, atol=0)
    bare = pr.rbf_action(ref["x_rbf"], g["X"], g["Y"], g["lengthscales"], g["noise"], pref.ACTION_MAX, squash=False)
    assert np.abs(pref.ACTION_MAX * np.sin(bare) / ref["u_rbf"] - 1).min() > 4e-7


def test_restated_rewards_at_zero_covariance():
    g = np.load(os.path.join(GOLDEN, "reward.npz"))
    x = np.array([[0.3, -0.2], [1.0, 2.0]])
    d = x - g["t2"]
    want = np.exp(-0.5 * np.array([di @ g["W2"] @ di for di in d]))
    terms = [dict(kind="exponential", W=g["W2"], t=g["t2"], coef=0.7), dict(kind="linear", W=g["W_lin"], coef=-0.2)]
    np.testing.assert_allclose(pr.reward(terms, x), 0.7 * want - 0.2 * (x @ g["W_lin"]), rtol=1e-14)


# ------------------------------------------------------------------ the kernels and the boundary
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_particle_kernels_compile_and_pass_both_mfma_scanners(tmp_path):
    asm = str(tmp_path / "particles.s")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
           "-mllvm", "-amdgpu-mfma-vgpr-form", "-S", "--cuda-device-only", "-o", asm, os.path.join(CSRC, "particles.hip")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stderr[-2000:]
    text = open(asm).read()
    for k in ("k_particle_head", "k_particle_tail", "k_particle_partials", "k_particle_finish"):
        assert k in text
    assert "global_atomic" not in text and "flat_atomic" not in text   # the sums run in a fixed order: no atomics
    for tool in ("mfma_overlap_check.py", "mfma_hazard_check.py"):
        chk = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), asm], capture_output=True, text=True, timeout=300)
        assert chk.returncode == 0, "%s:\n%s" % (tool, chk.stdout[-3000:])


def test_header_declares_the_entry_point_and_the_binding_carries_it():
    import ctypes as C
    from pilco_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "pilco_hip.h")).read()
    assert re.search(r"\bint pilco_rollout_particles\s*\(", hdr) and "#define PILCO_HIP_ABI_VERSION 2" in hdr
    res, args = _lib.SIGNATURES["pilco_rollout_particles"]
    assert res is C.c_int and len(args) == 15 and args[8] is C.c_ulonglong
    assert hasattr(_lib.Context, "rollout_particles")
    from pilco_amd.models import PILCO
    assert hasattr(PILCO, "sample_trajectories")
