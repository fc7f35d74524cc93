"""The function-sample particle rollout (pilco_rollout_particles_fn, docs/particle_functions.md) without a device:
  * the four new streams of csrc/philox_normal.h (domains 1..4), compiled into a host probe, against the Python-integer
    restatement (tests/helpers/particle_fn_restatement.py) word for word, and the vectorised restatement against the same;
  * the mathematics of the restatement: over (w, xi) the mean of f_p(x) is the posterior mean and its variance the closed form
    |phi(x) - Phi(X)^T iK k*|^2 + noise |iK k*|^2; at the training inputs of data drawn from the model itself f_p(X) - y has
    the standard deviation of the likelihood noise;
  * the Python surface: header, binding, the new arguments and their refusals, reached before any device call."""
import ctypes as C
import inspect
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from helpers import particle_fn_restatement as rf
from helpers import particles_restatement as pr
from helpers.predict_restatement import se_ard

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CSRC = os.path.join(ROOT, "pilco_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

PROBE = r'''#include <cstdio>
#include "philox_normal.h"
using namespace pilco;
int main() {
    unsigned long long seed;
    unsigned c0, c1, c2, dom;
    while (std::scanf("%llu %u %u %u %u", &seed, &c0, &c1, &c2, &dom) == 5) {
        const PhiloxWords w = philox_domain_words(seed, c0, c1, c2, dom);
        double z0, z1;
        philox_domain_normal_pair(seed, c0, c1, c2, dom, &z0, &z1);
        std::printf("%08x %08x %08x %08x %.17g %.17g %.17g\n", w.w[0], w.w[1], w.w[2], w.w[3], z0, z1, philox_fn_phase(seed, c0, c1));
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("philox_fn_probe")
    src = d / "philox_fn_probe.hip"
    src.write_text(PROBE)
    exe = d / "philox_fn_probe"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-I" + CSRC, "-I/opt/rocm/include", str(src), "-o", str(exe)],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(exe)


def _cases():
    rs = np.random.RandomState(23)
    cases = [(0, 0, 0, 0, d) for d in (1, 2, 3, 4)] + [(2 ** 64 - 1, 4095, 31, 15, 1), (2 ** 32, 4096, 4999, 5, 4), (5, 129, 4095, 1, 3)]
    for _ in range(300):
        cases.append((int(rs.randint(0, 2 ** 31)) * int(rs.randint(1, 2 ** 31)) + int(rs.randint(0, 2 ** 31)),
                      int(rs.randint(0, 200000)), int(rs.randint(0, 5000)), int(rs.randint(0, 16)), int(rs.randint(1, 5))))
    return cases


def test_probe_words_normals_and_phases_match_the_restatement(probe):
    cases = _cases()
    txt = "".join("%d %d %d %d %d\n" % c for c in cases)
    out = subprocess.run([probe], input=txt, capture_output=True, text=True, timeout=60, check=True).stdout.strip().split("\n")
    assert len(out) == len(cases)
    worst = 0.0
    for (seed, c0, c1, c2, dom), line in zip(cases, out):
        f = line.split()
        assert tuple(int(w, 16) for w in f[:4]) == rf.domain_words(seed, c0, c1, c2, dom), (seed, c0, c1, c2, dom)
        z0, z1, r = rf.domain_normal_pair(seed, c0, c1, c2, dom)
        bound = 16 * 2.0 ** -53 * max(1.0, r)
        for got, want in ((float(f[4]), z0), (float(f[5]), z1)):
            assert abs(got - want) <= bound, (seed, c0, c1, c2, dom, got, want)
            worst = max(worst, abs(got - want) / bound)
        assert abs(float(f[6]) - rf.phase(seed, c0, c1)) <= 4 * 2.0 ** -53 * 2 * math.pi
    print("host probe, domains 1..4, %d counters: largest |dz| / bound = %.3g" % (len(cases), worst))


def test_the_existing_stream_is_domain_zero_and_the_domains_never_coincide():
    seed = 0x1234567890ABCDEF
    assert rf.domain_words(seed, 7, 3, 2, 0) == pr.particle_words(seed, 3, 7, 2)     # {p, t, j, 0}
    idx = [(a, b, c) for a in (0, 1, 129) for b in (0, 1, 63) for c in (0, 1)]
    counters = {(a, b, c, d) for (a, b, c) in idx for d in range(5)}
    assert len(counters) == 5 * len(idx)
    words = {rf.domain_words(seed, a, b, c, d) for (a, b, c, d) in counters}
    assert len(words) == len(counters)


def test_vectorised_streams_are_the_integer_restatement():
    seed, E, L, D, N = 2 ** 40 + 17, 3, 5, 5, 7
    z, r = rf.freq_normals(seed, E, L, D)
    ph = rf.phases(seed, E, L)
    w, _ = rf.weights(seed, [0, 4, 130], E, L)
    xi, _ = rf.xis(seed, [0, 4, 130], E, N)
    tol = 16 * 2.0 ** -53
    for e in range(E):
        for l in range(L):
            assert ph[e, l] == rf.phase(seed, l, e)
            for d in range(D):
                zz = rf.domain_normal_pair(seed, l, e, d // 2, rf.FREQ)
                assert abs(z[e, l, d] - zz[d % 2]) <= tol * max(1.0, zz[2]) and r[e, l, d] == pytest.approx(zz[2], rel=1e-15)
    for k, p in enumerate([0, 4, 130]):
        for e in range(E):
            for l in range(L):
                zz = rf.domain_normal_pair(seed, p, l, e // 2, rf.WEIGHT)
                assert abs(w[k, e, l] - zz[e % 2]) <= tol * max(1.0, zz[2])
            for i in range(N):
                zz = rf.domain_normal_pair(seed, p, i, e // 2, rf.XI)
                assert abs(xi[k, e, i] - zz[e % 2]) <= tol * max(1.0, zz[2])


# ------------------------------------------------------------------ the mathematics
def _predictions_model():
    g = np.load(os.path.join(GOLDEN, "predictions.npz"))
    m = {k: g[k] for k in ("X", "Y", "lengthscales", "variance")}
    m["noise"] = np.full(m["variance"].shape, 0.1)
    return m


def test_mean_and_variance_over_the_draws_are_the_closed_forms():
    model = _predictions_model()
    P, L = 4096, 256
    dr = rf.draws(3, model, P, L)
    X = model["X"]
    xs = np.concatenate([X[:3] + 0.05, 0.5 * (X[3:5] + X[5:7]), X.mean(axis=0, keepdims=True) + 1.5 * X.std(axis=0, keepdims=True)])
    assert xs.shape[0] == 6
    f = rf.sample_f(model, dr, xs)                      # (P, 6, E)
    mean, var = rf.closed_form(model, dr["omega"], dr["phase"], xs)
    exact = np.stack([model["variance"][e] - np.einsum("ni,ni->n", se_ard(xs, X, model["lengthscales"][e], model["variance"][e]),
                                                       np.linalg.solve(se_ard(X, X, model["lengthscales"][e], model["variance"][e])
                                                                       + 0.1 * np.eye(X.shape[0]),
                                                                       se_ard(xs, X, model["lengthscales"][e], model["variance"][e]).T).T)
                      for e in range(2)], axis=1)
    rm = np.abs(f.mean(axis=0) - mean) / (5 * np.sqrt(var / P))
    rv = np.abs(f.var(axis=0) - var) / (5 * var * math.sqrt(2.0 / P))
    print("mean: largest |mean_p f - k*^T beta| / (5 sqrt(var / P)) = %.3g;  variance: largest |var_p f - var_closed| / bound = %.3g;  "
          "var_closed / exact posterior variance at L = %d: %.3g .. %.3g" % (rm.max(), rv.max(), L, (var / exact).min(), (var / exact).max()))
    assert np.all(rm <= 1.0) and np.all(rv <= 1.0)


def test_function_samples_interpolate_the_data_up_to_the_noise():
    """Data drawn from the model itself (a function of the exact prior plus noise): jointly with y a posterior sample is
    distributed as the prior, so f_p(X) - y is the noise, N(0, noise) -- up to the feature approximation of the prior."""
    rs = np.random.RandomState(5)
    N, D, P, L, sn2 = 60, 3, 1024, 256, 0.1
    X = rs.uniform(-2.0, 2.0, (N, D))
    ls, var = np.array([[1.0, 1.5, 0.8]]), np.array([1.3])
    K = se_ard(X, X, ls[0], var[0])
    y = np.linalg.cholesky(K + 1e-10 * np.eye(N)) @ rs.randn(N) + math.sqrt(sn2) * rs.randn(N)
    model = dict(X=X, Y=y[:, None], lengthscales=ls, variance=var, noise=np.array([sn2]))
    dr = rf.draws(11, model, P, L)
    f = rf.sample_f(model, dr, X)[:, :, 0]               # (P, N)
    sd = float(np.sqrt(np.mean((f - y[None, :]) ** 2)))
    print("interpolation: sd of f_p(X) - y = %.4f, sqrt(noise) = %.4f, ratio %.4f" % (sd, math.sqrt(sn2), sd / math.sqrt(sn2)))
    assert abs(sd / math.sqrt(sn2) - 1.0) <= 0.10


def test_restated_step_is_mean_plus_a_deviation_with_the_closed_variance():
    """f_of (one point per particle) agrees with sample_f (host linear algebra) given the same V."""
    model = _predictions_model()
    P, L = 16, 32
    dr = rf.draws(9, model, P, L)
    X = model["X"]
    iK = [np.linalg.inv(se_ard(X, X, model["lengthscales"][e], model["variance"][e]) + 0.1 * np.eye(X.shape[0])) for e in range(2)]
    V, _ = rf.v_of(model, dr, iK)
    xu = X[:P] + 0.1
    f, m1, m2 = rf.f_of(model, dr, V, xu)
    g = rf.sample_f(model, dr, xu)
    want = np.stack([g[p, p] for p in range(P)])
    assert np.all(np.abs(f.astype(np.float64) - want) <= 1e-9 * (1.0 + m1.astype(np.float64)))


# ------------------------------------------------------------------ the boundary and the Python surface
def test_header_declares_the_entry_point_and_the_binding_carries_it():
    from pilco_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "pilco_hip.h")).read()
    assert re.search(r"\bint pilco_rollout_particles_fn\s*\(", hdr) and "#define PILCO_HIP_ABI_VERSION 2" in hdr
    assert "pilco_function_draws_out" in hdr and re.search(r"typedef struct pilco_function_draws\b", hdr)
    res, args = _lib.SIGNATURES["pilco_rollout_particles_fn"]
    assert res is C.c_int and len(args) == 21 and args[8] is C.c_ulonglong
    assert [f for f, _ in _lib.FunctionDraws._fields_] == ["L", "omega", "phase", "w", "xi"]
    assert [f for f, _ in _lib.FunctionDrawsOut._fields_] == ["omega", "phase", "w", "xi", "v"]
    assert hasattr(_lib.Context, "rollout_particles_fn")


def test_sample_trajectories_takes_dynamics_and_refuses_before_any_device_call():
    from pilco_amd.models import PILCO
    from pilco_amd.safe import SafePILCO
    sig = inspect.signature(PILCO.sample_trajectories).parameters
    assert sig["dynamics"].default == "marginal" and sig["num_features"].default == 512 and sig["function_draws"].default is None
    rsig = inspect.signature(SafePILCO.sample_risk).parameters
    assert rsig["dynamics"].default == "marginal" and rsig["num_features"].default == 512
    g = np.load(os.path.join(GOLDEN, "predictions.npz"))
    m0, S0 = g["X"][:1, :2], 0.05 * np.eye(2)

    class NoDevice:
        def __getattr__(self, name):
            raise AssertionError("the context was touched: " + name)

    p = PILCO((g["X"], g["Y"]))
    p._ctx = NoDevice()
    with pytest.raises(ValueError, match="dynamics"):
        p.sample_trajectories(m0, S0, 2, num_particles=4, dynamics="pathwise")
    s = PILCO((g["X"], g["Y"]), num_induced_points=10)
    s._ctx = NoDevice()
    with pytest.raises(NotImplementedError, match="exact GP"):
        s.sample_trajectories(m0, S0, 2, num_particles=4, dynamics="function")
    from pilco_amd.models.pilco import ParticleTrajectories
    t = ParticleTrajectories(np.zeros((1, 2)), np.zeros((1, 2, 2)), np.zeros(0), None, None)
    assert t.function_draws is None


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_function_kernels_compile_without_atomics_or_scratch(tmp_path):
    asm = str(tmp_path / "particles_fn.s")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
           "-mllvm", "-amdgpu-mfma-vgpr-form", "-S", "--cuda-device-only", "-o", asm, os.path.join(CSRC, "particles_fn.hip")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stderr[-2000:]
    text = open(asm).read()
    for k in ("k_particle_fn_step", "k_fn_features", "k_fn_weights", "k_fn_phix", "k_fn_resid"):
        assert k in text
    assert "global_atomic" not in text and "flat_atomic" not in text   # the sums run in a fixed order
    # the register builds of the step keep the particle's point and the lengthscales in registers: no scratch memory
    sizes = [int(m) for m in re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text)]
    assert sizes and max(sizes) == 0, sizes
