"""The path-conditioned particle rollout (pilco_rollout_particles_cond, docs/particle_conditioned.md) without a device:
  * the restatement (tests/helpers/particle_cond_restatement.py): its row-by-row path against the sampling map of
    helpers/predict_cov_restatement.py on a well-conditioned path, and its pivots on the ill-conditioned paths of the
    predictions.npz model (the condition under which the device cases can pass at all);
  * the group plan of csrc/particles_cond_plan.h, compiled into a host probe, against its Python mirror;
  * the words of Philox domain 6 (csrc/philox_normal.h) against the Python-integer restatement;
  * the boundary: declaration, export, ctypes signature, ABI version; and the Python refusals, reached before any device call.
Every test prints its figures before it asserts (run with -s; docs/particle_conditioned.md records them)."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from helpers import particle_cond_restatement as rq
from helpers import particle_fn_restatement as rf
from helpers import particles_restatement as pr
from helpers import predict_cov_restatement as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CSRC = os.path.join(ROOT, "pilco_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
LD = np.longdouble


def _predictions_model(noise=None, ls_scale=1.0):
    g = np.load(os.path.join(GOLDEN, "predictions.npz"))
    m = {k: np.array(g[k]) for k in ("X", "Y", "lengthscales", "variance", "noise")}
    m["lengthscales"] = m["lengthscales"] * ls_scale
    if noise is not None:
        m["noise"] = np.full(m["variance"].shape, noise)
    return m


# ------------------------------------------------------------------ the mathematics of the restatement
def test_row_by_row_path_is_the_sampling_map_on_a_well_conditioned_path():
    """Points a lengthscale apart: the path covariance is well conditioned, two factorisations agree, and the increments of
    the row-by-row restatement are mean + chol(cov + jitter I) z of the predict-cov helper."""
    m = _predictions_model()
    H, E = 7, 2
    rs = np.random.RandomState(3)
    ls = m["lengthscales"].max(axis=0)
    xs = m["X"].mean(axis=0)[None, :] + np.arange(H)[:, None] * ls[None, :] * np.array([1.0, -1.0, 1.0])   # a lengthscale apart
    c = dict(E=E, M=0, own=False)
    d = dict(X=m["X"], xs=xs, ls=m["lengthscales"], var=m["variance"], noise=m["noise"], Z=None)
    cov = rc.restate_a(c, d)
    mean = rs.randn(H, E)
    z = rs.randn(1, H, E)
    jitter = 1e-8
    worst = 0.0
    for e in range(E):
        je = jitter * m["variance"][e]
        want = rc.sample_map(mean[:, e:e + 1], cov[e:e + 1], z[:, :, e:e + 1], je)[0, :, 0]
        lam, ds, f = rq.path(cov[e], je, mean[:, e], z[0, :, e])
        cond = np.linalg.cond(cov[e] + je * np.eye(H))
        err = float(np.max(np.abs(f.astype(np.float64) - want)))
        print("output %d: condition number %.3g, smallest pivot / j_e = %.3g, largest |f_rows - f_map| = %.3g" %
              (e, cond, float(ds.min()) / je, err))
        worst = max(worst, err)
        assert np.all(ds > 0)
    assert worst <= 1e-10


def _cpu_rollout_pivots(model, policy, x0, H, jitter, seed):
    """A float64 rollout of the conditioned path with the factor rows in np.longdouble: -> the pivots d / j_e, (H, P, E)."""
    X = model["X"]
    E, P = len(model["variance"]), x0.shape[0]
    Linv = [np.linalg.inv(np.linalg.cholesky(rc.se_device(X, X, model["lengthscales"][e], model["variance"][e])
                                             + model["noise"][e] * np.eye(len(X)))) for e in range(E)]
    beta = [Linv[e].T @ (Linv[e] @ model["Y"][:, e]) for e in range(E)]
    z, _ = pr.normals(seed, H, P, E)
    x = x0.copy()
    pts, Wh = [], [[] for _ in range(E)]
    lam = np.zeros((P, E, H, H), LD)
    piv = np.zeros((H, P, E))
    for t in range(H):
        xu = np.concatenate([x, pr.action(policy, x)], axis=1)
        pts.append(xu)
        xn = x.copy()
        for e in range(E):
            ls, sf2 = model["lengthscales"][e], model["variance"][e]
            ks = rc.se_device(X, xu, ls, sf2)                # (N, P)
            Wh[e].append(Linv[e] @ ks)
            mu = ks.T @ beta[e]
            je = jitter * sf2
            for p in range(P):
                kk = rc.se_device(xu[p:p + 1], np.stack([q[p] for q in pts]), ls, sf2)[0]
                c = kk - np.array([Wh[e][t][:, p] @ Wh[e][s][:, p] for s in range(t + 1)])
                l, dd, f = rq.row(c, lam[p, e, :t, :t], je, mu[p], z[:t + 1, p, e])
                lam[p, e, t, :t + 1] = l
                piv[t, p, e] = float(dd) / je
                xn[p, e] = x[p, e] + float(f)
        x = xn
    return piv


@pytest.mark.parametrize("noise,ls_scale", [(1e-4, 1.0), (0.1, 1.0), (1e-4, 10.0), (0.1, 10.0)])
def test_pivots_of_the_ill_conditioned_paths_stay_above_half_the_jitter(noise, ls_scale):
    m = _predictions_model(noise, ls_scale)
    policy = dict(kind="linear", W=np.array([[0.7, -0.4]]), b=np.array([[0.15]]), max_action=1.3)
    P, H, jitter = 16, 40, 1e-8
    x0 = m["X"][:1, :2] + np.random.RandomState(1).randn(P, 2) * np.sqrt(0.05)
    piv = _cpu_rollout_pivots(m, policy, x0, H, jitter, seed=11)
    print("noise %g, lengthscales x %g, H = %d, P = %d: smallest pivot d / j_e = %.4g, share of pivots below 2 j_e = %.3g" %
          (noise, ls_scale, H, P, piv.min(), float(np.mean(piv < 2.0))))
    assert np.all(piv >= 0.5)


# ------------------------------------------------------------------ the group plan
PLAN_PROBE = r'''#include <cstdio>
#include "particles_cond_plan.h"
using namespace pilco;
int main() {
    int P, H, nops, E, D, npad, want, cap;
    unsigned long long budget;
    while (std::scanf("%d %d %d %d %d %d %d %llu %d", &P, &H, &nops, &E, &D, &npad, &want, &budget, &cap) == 9) {
        const CondPlan pl = cond_plan(P, H, nops, E, D, npad, want != 0, (size_t)budget, cap);
        std::printf("%d %d %zu %zu %d %zu\n", pl.G, pl.ngroups, pl.per_particle, pl.footprint, pl.H_fit, cond_col(H, H / 2));
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def plan_probe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or (HIPCC if os.path.exists(HIPCC) else None)
    if cxx is None:
        pytest.skip("no C++ compiler available")
    d = tmp_path_factory.mktemp("cond_plan_probe")
    src = d / "cond_plan_probe.cpp"
    src.write_text(PLAN_PROBE)
    exe = d / "cond_plan_probe"
    r = subprocess.run([cxx, "-O1", "-std=c++17", "-I" + CSRC, str(src), "-o", str(exe)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(exe)


def _plan_cases():
    cases = []
    c2u = dict(nops=1, E=10, D=11, npad=1024)
    per = rq.per_particle(40, 1, 10, 11, 1024, False)
    cap = rq.chunk_cap(10, 1024)
    for P in (1, 64, 65, 1024, 4096):
        for budget in (2 ** 29, 64 * per, 64 * per - 1, 128 * per, 128 * per - 1, 3 * 64 * per + 5):   # the edges of the budget
            cases.append((P, 40, 1, 10, 11, 1024, 0, budget, cap))
    cases += [(129, 6, 1, 2, 3, 128, 1, 64 * rq.per_particle(6, 1, 2, 3, 128, True), rq.chunk_cap(2, 128)),   # the smallest group: 3 groups
              (129, 6, 2, 2, 3, 64, 0, 2 ** 29, rq.chunk_cap(2, 64)),
              (3, 128, 1, 1, 1, 64, 1, 2 ** 29, rq.chunk_cap(1, 64)),
              (4096, 128, 1, 10, 11, 5056, 0, 2 ** 29, rq.chunk_cap(10, 5056)),     # refused: names the largest H that fits
              (10, 0, 1, 2, 3, 128, 0, 1, 64), (10, 5, 1, 2, 3, 128, 0, 1, 64)]      # H = 0 needs the chunk buffers; nothing fits
    return cases, c2u


def test_group_plan_probe_matches_the_python_mirror(plan_probe):
    cases, _ = _plan_cases()
    txt = "".join("%d %d %d %d %d %d %d %d %d\n" % c for c in cases)
    out = subprocess.run([plan_probe], input=txt, capture_output=True, text=True, timeout=60, check=True).stdout.strip().split("\n")
    assert len(out) == len(cases)
    refused = grouped = 0
    for c, line in zip(cases, out):
        got = tuple(int(v) for v in line.split())
        P, H, nops, E, D, npad, want, budget, cap = c
        G, ng, per, foot, hfit = rq.plan(P, H, nops, E, D, npad, bool(want), budget, cap)
        assert got[:5] == (G, ng, per, foot, hfit), (c, got)
        assert got[5] == (H // 2) * H - (H // 2) * (H // 2 - 1) // 2
        if G == 0:
            refused += 1
            assert hfit < H and (hfit < 0 or rq.per_particle(hfit, nops, E, D, npad, bool(want)) * 64 <= budget)
            assert rq.per_particle(hfit + 1, nops, E, D, npad, bool(want)) * 64 > budget
        else:
            grouped += ng > 1
            assert G % 64 == 0 and G <= cap and foot <= budget and ng * G >= P and (ng - 1) * G < P
            assert G == min((P + 63) // 64 * 64, cap) or per * (G + 64) > budget   # the largest group that fits
    per = rq.per_particle(40, 1, 10, 11, 1024, False)
    G, ng, _, foot, _ = rq.plan(4096, 40, 1, 10, 11, 1024, False, 2 ** 29, rq.chunk_cap(10, 1024))
    print("C2u, H = 40: %d doubles per particle; budget 2^29: groups of %d (%d groups at P = 4096, %.2f GB); %d cases refused, %d grouped"
          % (per, G, ng, foot * 8 / 1e9, refused, grouped))
    assert refused >= 3 and grouped >= 3
    g129 = rq.plan(*cases[30][:6], bool(cases[30][6]), *cases[30][7:])
    assert g129[:2] == (64, 3)


# ------------------------------------------------------------------ Philox domain 6
PHILOX_PROBE = r'''#include <cstdio>
#include "philox_normal.h"
using namespace pilco;
int main() {
    unsigned long long seed;
    unsigned c0, c1, c2;
    while (std::scanf("%llu %u %u %u", &seed, &c0, &c1, &c2) == 4) {
        const PhiloxWords w = philox_domain_words(seed, c0, c1, c2, PHILOX_COND_OBS);
        double z0, z1;
        philox_domain_normal_pair(seed, c0, c1, c2, PHILOX_COND_OBS, &z0, &z1);
        std::printf("%08x %08x %08x %08x %.17g %.17g %u\n", w.w[0], w.w[1], w.w[2], w.w[3], z0, z1, (unsigned)PHILOX_COND_OBS);
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def philox_probe(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("philox_cond_probe")
    src = d / "philox_cond_probe.hip"
    src.write_text(PHILOX_PROBE)
    exe = d / "philox_cond_probe"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-I" + CSRC, "-I/opt/rocm/include", str(src), "-o", str(exe)],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(exe)


def test_domain_six_words_and_normals_match_the_integer_restatement(philox_probe):
    rs = np.random.RandomState(29)
    cases = [(0, 0, 0, 0), (2 ** 64 - 1, 4095, 127, 15), (2 ** 32, 129, 64, 1)]
    for _ in range(300):
        cases.append((int(rs.randint(0, 2 ** 31)) * int(rs.randint(1, 2 ** 31)) + int(rs.randint(0, 2 ** 31)),
                      int(rs.randint(0, 200000)), int(rs.randint(0, 128)), int(rs.randint(0, 16))))
    txt = "".join("%d %d %d %d\n" % c for c in cases)
    out = subprocess.run([philox_probe], input=txt, capture_output=True, text=True, timeout=60, check=True).stdout.strip().split("\n")
    assert len(out) == len(cases)
    worst = 0.0
    for (seed, p, t, j), line in zip(cases, out):
        f = line.split()
        assert int(f[6]) == rq.COND_OBS == 6
        assert tuple(int(w, 16) for w in f[:4]) == rf.domain_words(seed, p, t, j, rq.COND_OBS), (seed, p, t, j)
        z0, z1, r = rf.domain_normal_pair(seed, p, t, j, rq.COND_OBS)
        bound = 16 * 2.0 ** -53 * max(1.0, r)
        for got, want in ((float(f[4]), z0), (float(f[5]), z1)):
            assert abs(got - want) <= bound
            worst = max(worst, abs(got - want) / bound)
    print("host probe, domain 6, %d counters: largest |dz| / bound = %.3g" % (len(cases), worst))


def test_the_observation_stream_is_its_own_domain_and_the_vectorised_draws_are_the_integer_ones():
    seed, H, P, E = 2 ** 40 + 19, 3, 5, 3
    zeta, r = rq.obs_normals(seed, H, P, E)
    for t in range(H):
        for p in range(P):
            for e in range(E):
                z = rf.domain_normal_pair(seed, p, t, e // 2, rq.COND_OBS)
                assert abs(zeta[t, p, e] - z[e % 2]) <= 16 * 2.0 ** -53 * max(1.0, z[2])
    words = {rf.domain_words(seed, p, t, j, d) for p in (0, 1, 129) for t in (0, 1, 127) for j in (0, 1) for d in range(7)}
    assert len(words) == 3 * 3 * 2 * 7
    assert rf.domain_words(seed, 7, 3, 1, 0) == pr.particle_words(seed, 3, 7, 1)      # the step stream stays domain 0, {p, t, j, 0}


# ------------------------------------------------------------------ the boundary and the Python surface
def test_header_declares_the_entry_point_and_the_binding_carries_it():
    from pilco_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "pilco_hip.h")).read()
    assert re.search(r"\bint pilco_rollout_particles_cond\s*\(", hdr) and "#define PILCO_HIP_ABI_VERSION 2" in hdr
    assert "#define PILCO_MAX_COND_STEPS 128" in hdr and re.search(r"typedef struct pilco_cond_out\b", hdr)
    res, args = _lib.SIGNATURES["pilco_rollout_particles_cond"]
    assert res is C.c_int and len(args) == 22 and args[8] is C.c_ulonglong and args[19] is C.c_double
    assert [f for f, _ in _lib.CondOut._fields_] == ["eps_obs", "path_cov", "path_factor"]
    assert _lib.MAX_COND_STEPS == 128 and hasattr(_lib.Context, "rollout_particles_cond")
    lib = _lib.load_library()
    assert hasattr(lib, "pilco_rollout_particles_cond") and lib.pilco_abi_version() == 2
    n_decl = len(set(re.findall(r"\bint (pilco_[a-z0-9_]+)\s*\(", hdr)) | set(re.findall(r"\bconst char\* (pilco_[a-z0-9_]+)\s*\(", hdr)))
    for doc in ("README.md", "INTEGRATION.md"):
        m = re.search(r"(\d+) entry points", open(os.path.join(ROOT, doc)).read())
        assert m and int(m.group(1)) == n_decl, (doc, m and m.group(1), n_decl)


def test_python_surface_and_refusals_before_any_device_call():
    from pilco_amd.models import PILCO
    from pilco_amd.models.pilco import ParticleTrajectories
    from pilco_amd.safe import SafePILCO
    sig = inspect.signature(PILCO.sample_trajectories).parameters
    assert sig["dynamics"].default == "marginal" and sig["jitter"].default == 1e-8 and sig["eps_obs"].default is None
    assert "dynamics" in inspect.signature(SafePILCO.sample_risk).parameters
    g = np.load(os.path.join(GOLDEN, "predictions.npz"))
    m0, S0 = g["X"][:1, :2], 0.05 * np.eye(2)

    class NoDevice:
        def __getattr__(self, name):
            raise AssertionError("the context was touched: " + name)

    for kw in (dict(), dict(num_induced_points=10)):
        p = PILCO((g["X"], g["Y"]), **kw)
        p._ctx = NoDevice()
        with pytest.raises(ValueError, match="dynamics"):
            p.sample_trajectories(m0, S0, 2, num_particles=4, dynamics="pathwise")
        with pytest.raises(ValueError, match="num_features"):
            p.sample_trajectories(m0, S0, 2, num_particles=4, dynamics="conditioned", num_features=64)
        with pytest.raises(ValueError, match="function_draws"):
            p.sample_trajectories(m0, S0, 2, num_particles=4, dynamics="conditioned", function_draws={})
        with pytest.raises(ValueError, match="eps_obs"):
            p.sample_trajectories(m0, S0, 2, num_particles=4, dynamics="marginal", eps_obs=np.zeros((2, 4, 2)))
        with pytest.raises(NotImplementedError, match="conditioned"):
            p.particle_value_and_gradient(m0, S0, 2, num_particles=4, dynamics="conditioned")
        with pytest.raises(NotImplementedError, match="conditioned"):
            p.optimize_policy(maxiter=1, objective="particles", particle_options=dict(dynamics="conditioned"))
    s = PILCO((g["X"], g["Y"]), num_induced_points=10)
    s._ctx = NoDevice()
    with pytest.raises(NotImplementedError, match="exact GP"):        # as before
        s.sample_trajectories(m0, S0, 2, num_particles=4, dynamics="function")
    t = ParticleTrajectories(np.zeros((1, 2)), np.zeros((1, 2, 2)), np.zeros(0), None, None)
    assert t.eps_obs is None and t.path_cov is None and t.path_factor is None
    t = ParticleTrajectories(np.zeros((1, 2)), np.zeros((1, 2, 2)), np.zeros(0), None, None, path_cov=1, path_factor=2, eps_obs=3)
    assert (t.eps_obs, t.path_cov, t.path_factor) == (3, 1, 2)
    with pytest.raises(TypeError):
        ParticleTrajectories(np.zeros((1, 2)), np.zeros((1, 2, 2)), np.zeros(0), None, None, None, None, None, 3)   # keyword fields


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_step_kernel_compiles_without_atomics_or_scratch(tmp_path):
    asm = str(tmp_path / "particles_cond.s")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
           "-mllvm", "-amdgpu-mfma-vgpr-form", "-S", "--cuda-device-only", "-o", asm, os.path.join(CSRC, "particles_cond.hip")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stderr[-2000:]
    text = open(asm).read()
    assert "k_particle_cond_step" in text
    assert "global_atomic" not in text and "flat_atomic" not in text and "ds_add" not in text   # the sums run in a fixed order
    assert "v_mfma" not in text                                                                  # plain VALU: bandwidth binds
    sizes = [int(m) for m in re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text)]
    assert sizes and max(sizes) == 0, sizes
