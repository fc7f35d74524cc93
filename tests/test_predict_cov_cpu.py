"""The yardsticks of the full posterior covariance and the joint samples, checked without a GPU (docs/predict_cov.md):
  * the case table covers what it must (helpers/predict_cov_cases.missing);
  * both float64 restatements (helpers/predict_cov_restatement.py) stay within the stored caps of the 40-digit truth in
    tests/golden/predict_cov.npz, and the caps recomputed from them agree with the stored ones;
  * the truth (helpers/predict_cov_truth.py) has oracle.mp_predict's variance on its diagonal and agrees with
    K** - K*^T iK K* evaluated in 40 digits by another route;
  * mutants of the device-ordered restatement are each more than 100 caps from the truth on some case;
  * Philox domain 5: csrc/philox_normal.h compiled into a host probe against the Python restatement, domains 0..4 unchanged;
  * the Python layer (shapes, refusals, SMGPR's own Z) on a small fake context; the ctypes signatures of the new symbols;
  * the new kernels compile without atomics or scratch and pass the MFMA scanners of tests/test_build_isa.py."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from helpers import particle_fn_restatement as rf
from helpers import particles_restatement as pr
from helpers import predict_cov_cases as cc
from helpers import predict_cov_restatement as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pilco_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
MP_CASES = ["x5_t17_d1_e1", "f5_t17_d1_e1", "x5_t65_d1_e1", "f5_t65_d1_e1"]   # cheap enough to recompute in 40 digits here


# ------------------------------------------------------------------ the table and the fixture
def test_the_table_covers_what_it_must_and_the_guard_notices_a_hole():
    assert cc.missing() == []
    assert len(set(cc.case_ids())) == len(cc.CASES)
    assert "exact: Nt = 130" in cc.missing([c for c in cc.CASES if c["Nt"] != 130])
    assert "FITC: n = 64 at Nt = 65" in cc.missing([c for c in cc.CASES if not (c["kind"] == "f" and c["n"] == 64 and c["Nt"] == 65)])
    assert "FITC: every output's own Z" in cc.missing([c for c in cc.CASES if not c["own"]])
    assert "one output alone (output = 1)" in cc.missing([c for c in cc.CASES if c["E"] == 1])
    assert "exact: noise 1e-6 at n = 130" in cc.missing([c for c in cc.CASES if not (c["kind"] == "x" and c["n"] == 130 and c["noise"] < 1e-3)])
    assert os.path.getsize(cc.PATH) < 2 ** 20
    assert "mpmath" in str(cc.get("_provenance"))


def test_the_fixture_holds_the_table_s_data_and_points():
    for c in cc.CASES:
        d, fx = cc.make_data(c), cc.load(c)
        d["xs"] = cc.make_points(c, d)
        for k in ("X", "Y", "ls", "var", "noise", "xs") + (("Z",) if c["M"] else ()):
            assert np.array_equal(d[k], fx[k]), (c["name"], k)
        assert fx["cov"].shape == (c["E"], c["Nt"], c["Nt"]) and np.all(np.isfinite(fx["cov"])) and np.all(fx["unit"] >= cc.TINY)
        if c["Nt"] >= 4:      # the duplicate: two equal rows; the far point: sf2 on the diagonal, ~ 0 off it
            assert np.array_equal(fx["cov"][:, 0], fx["cov"][:, 1]), c["name"]
            assert np.allclose(fx["cov"][:, 3, 3], fx["var"], rtol=1e-12) and np.all(np.abs(fx["cov"][:, 3, :3]) < 1e-150), c["name"]


@pytest.mark.parametrize("name", cc.case_ids())
def test_both_restatements_stay_within_the_stored_caps(name):
    c = cc.by_name(name)
    d = cc.load(c)
    ka, kb = cr.k_of(cr.restate_a(c, d), d), cr.k_of(cr.restate_b(c, d), d)
    print("%-24s K_ref (a) %.3g (b) %.3g cap %.3g" % (name, ka, kb, d["cap"]))
    assert ka <= d["cap"] and kb <= d["cap"]
    again = cr.cap_from(max(ka, kb))
    assert d["cap"] / 2 <= again <= 2 * d["cap"], (again, d["cap"])
    assert d["cap"] >= cc.CAP_FLOOR


@pytest.mark.parametrize("name", MP_CASES)
def test_the_truth_has_the_oracle_s_variance_on_its_diagonal_and_is_the_direct_formula(name):
    from helpers import predict_cov_truth as ct
    from oracle import mp_predict
    c = cc.by_name(name)
    d = cc.load(c)
    ls, sf2, sn2 = d["ls"][0], d["var"][0], d["noise"][0]
    ulp = lambda a: np.spacing(np.abs(a))
    if c["M"]:
        cov, unit = ct.fitc_cov(d["X"], d["Z"][0], ls, sf2, sn2, d["xs"], jitter=cc.JITTER)
        o = mp_predict.fitc(d["X"], d["Y"][:, 0], d["Z"][0], ls, sf2, sn2, d["xs"], jitter=cc.JITTER)
    else:
        cov, unit = ct.gpr_cov(d["X"], ls, sf2, sn2, d["xs"])
        o = mp_predict.gpr(d["X"], d["Y"][:, 0], ls, sf2, sn2, d["xs"])
        direct = ct.gpr_cov_direct(d["X"], ls, sf2, sn2, d["xs"])
        assert np.all(np.abs(direct - cov) <= ulp(cov)), np.abs(direct - cov).max()       # (two roundings of the same 40 digits)
    assert np.array_equal(cov, d["cov"][0])                                               # what the fixture holds
    assert np.all(unit >= d["unit"][0]) and np.all(unit <= d["unit"][0] * (1 + 1e-4))     # ... its units, rounded down
    assert np.all(np.abs(np.diag(cov) - o["var"]) <= ulp(o["var"]))
    assert np.all(np.abs(np.diag(unit) - o["uvar"]) <= 4 * ulp(o["uvar"]))


@pytest.mark.parametrize("mutant", cr.MUTANTS)
def test_a_mutant_of_the_device_ordered_restatement_is_far_from_the_truth(mutant):
    names = ["f64_t17_d4_e3", "f65_t17_d4_e3_own_lo", "f63_t17_d4_e1"] + ([] if mutant in cr.FITC_ONLY else ["x65_t17_d4_e3_lo", "x63_t17_d4_e1", "x64_t1_d1_e1"])
    worst = 0.0
    for name in names:
        c = cc.by_name(name)
        d = cc.load(c)
        k = cr.k_of(cr.restate_b(c, d, mutant), d)
        assert np.isfinite(k), (mutant, name)
        worst = max(worst, k / d["cap"])
    print("mutant %-14s %.3g caps from the truth" % (mutant, worst))
    assert worst > 100.0


def test_the_sampling_map_is_mean_plus_factor_times_draws():
    c = cc.by_name("x5_t17_d1_e1")
    d = cc.load(c)
    z = np.random.RandomState(0).randn(4, c["Nt"], 1)
    mean = np.random.RandomState(1).randn(c["Nt"], 1)
    s = cr.sample_map(mean, d["cov"], z)
    Cf = np.linalg.cholesky(d["cov"][0] + 1e-6 * np.eye(c["Nt"]))
    assert np.array_equal(s[2, :, 0], mean[:, 0] + Cf @ z[2, :, 0]) or np.allclose(s[2, :, 0], mean[:, 0] + Cf @ z[2, :, 0], rtol=1e-13)
    assert np.array_equal(cr.sample_map(mean, d["cov"], 0 * z)[1], mean)


# ------------------------------------------------------------------ Philox domain 5
PROBE = r'''#include <cstdio>
#include "philox_normal.h"
using namespace pilco;
int main() {
    unsigned long long seed;
    unsigned c0, c1, c2, dom;
    static_assert(PHILOX_COV_Z == 5u, "domain 5");
    while (std::scanf("%llu %u %u %u %u", &seed, &c0, &c1, &c2, &dom) == 5) {
        const PhiloxWords w = philox_domain_words(seed, c0, c1, c2, dom);
        double z0, z1;
        philox_domain_normal_pair(seed, c0, c1, c2, dom, &z0, &z1);
        std::printf("%08x %08x %08x %08x %.17g %.17g\n", w.w[0], w.w[1], w.w[2], w.w[3], z0, z1);
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("philox_cov_probe")
    src = d / "philox_cov_probe.hip"
    src.write_text(PROBE)
    exe = d / "philox_cov_probe"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-I" + CSRC, "-I/opt/rocm/include", str(src), "-o", str(exe)],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(exe)


def _counters():
    rs = np.random.RandomState(31)
    cases = [(0, 0, 0, 0, 5), (2 ** 64 - 1, 4095, 129, 15, 5), (2 ** 32, 64, 4095, 1, 5), (5, 65, 130, 0, 5)]
    for _ in range(300):
        cases.append((int(rs.randint(0, 2 ** 31)) * int(rs.randint(1, 2 ** 31)) + int(rs.randint(0, 2 ** 31)),
                      int(rs.randint(0, 5000)), int(rs.randint(0, 5000)), int(rs.randint(0, 16)), 5))
    return cases


def test_domain_5_of_the_header_is_the_python_restatement_word_for_word(probe):
    cases = _counters()
    txt = "".join("%d %d %d %d %d\n" % c for c in cases)
    out = subprocess.run([probe], input=txt, capture_output=True, text=True, timeout=60, check=True).stdout.strip().split("\n")
    assert len(out) == len(cases)
    worst = 0.0
    for (seed, s, a, j, dom), line in zip(cases, out):
        f = line.split()
        assert tuple(int(w, 16) for w in f[:4]) == rf.domain_words(seed, s, a, j, cr.COV_Z), (seed, s, a, j)
        z, r = cr.cov_normals(seed, s + 1, a + 1, [2 * j, 2 * j + 1])
        bound = 16 * 2.0 ** -53 * max(1.0, r[s, a, 0])
        for got, want in ((float(f[4]), z[s, a, 0]), (float(f[5]), z[s, a, 1])):
            assert abs(got - want) <= bound, (seed, s, a, j, got, want)
            worst = max(worst, abs(got - want) / bound)
    print("host probe, domain 5, %d counters: largest |dz| / bound = %.3g" % (len(cases), worst))


def test_the_library_s_host_draws_are_the_restatement_and_depend_on_seed_sample_point_output_only():
    from pilco_amd import _lib
    seed = 2 ** 40 + 17
    z, r = cr.cov_normals(seed, 5, 7, range(3))
    lz = _lib.philox_cov_normals(seed, 5, 7, range(3))
    assert lz.shape == (5, 7, 3) and np.all(np.abs(lz - z) <= 16 * 2.0 ** -53 * np.maximum(1.0, r))
    assert np.array_equal(_lib.philox_cov_normals(seed, 2, 3, [1]), lz[:2, :3, 1:2])
    for s, a, e in ((0, 0, 0), (4, 6, 2), (3, 1, 1)):
        zz = rf.domain_normal_pair(seed, s, a, e // 2, cr.COV_Z)
        assert abs(z[s, a, e] - zz[e % 2]) <= 16 * 2.0 ** -53 * max(1.0, zz[2])


def test_domains_0_to_4_are_unchanged_and_domain_5_coincides_with_none(probe):
    seed = 0x1234567890ABCDEF
    assert rf.domain_words(seed, 7, 3, 2, 0) == pr.particle_words(seed, 3, 7, 2)     # {p, t, j, 0}
    idx = [(a, b, c) for a in (0, 1, 129) for b in (0, 1, 63) for c in (0, 1)]
    words = {rf.domain_words(seed, a, b, c, d) for (a, b, c) in idx for d in range(6)}
    assert len(words) == 6 * len(idx)
    # the header's domains 0..4 on counters the existing suites use: still the integer restatement's words
    cases = [(0, 0, 0, 0, d) for d in range(5)] + [(2 ** 64 - 1, 4095, 31, 15, 1), (2 ** 32, 4096, 4999, 5, 4), (5, 129, 4095, 1, 3), (seed, 7, 3, 2, 0)]
    txt = "".join("%d %d %d %d %d\n" % c for c in cases)
    out = subprocess.run([probe], input=txt, capture_output=True, text=True, timeout=60, check=True).stdout.strip().split("\n")
    for (sd, c0, c1, c2, dom), line in zip(cases, out):
        assert tuple(int(w, 16) for w in line.split()[:4]) == rf.domain_words(sd, c0, c1, c2, dom), (sd, c0, c1, c2, dom)
    hdr = open(os.path.join(CSRC, "philox_normal.h")).read()
    assert re.search(r"PHILOX_STEP = 0u, PHILOX_FN_FREQ = 1u, PHILOX_FN_PHASE = 2u, PHILOX_FN_WEIGHT = 3u, PHILOX_FN_XI = 4u, PHILOX_COV_Z = 5u", hdr)


# ------------------------------------------------------------------ the boundary and the Python layer
def test_every_new_symbol_of_the_header_has_a_ctypes_signature():
    from pilco_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "pilco_hip.h")).read()
    for name, n_args in (("pilco_gp_predict_points_cov", 8), ("pilco_gp_sample_points", 15)):
        m = re.search(r"\bint %s\s*\(([^;]*)\);" % name, hdr)
        assert m, name
        assert len(m.group(1).split(",")) == n_args, (name, m.group(1))
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == n_args, name
    args = _lib.SIGNATURES["pilco_gp_sample_points"][1]
    assert args[6] is C.c_int and args[7] is C.c_ulonglong and args[9] is C.c_double
    assert hasattr(_lib.Context, "gp_predict_points_cov") and hasattr(_lib.Context, "gp_sample_points")


class FakeContext:
    """Just enough of _lib.Context for MGPR / SMGPR: records the calls, returns arrays of the right shapes."""

    def __init__(self):
        self._slot_owner = {}
        self.calls = []

    def gp_set_data(self, slot, X, Y, owner=None):
        self._slot_owner[slot] = owner

    def gp_set_hyp(self, slot, ls, var, noise, owner=None):
        self._slot_owner[slot] = owner

    def gp_set_inducing(self, slot, Z, owner=None):
        self._slot_owner[slot] = owner

    def gp_factorize(self, slot):
        pass

    def gp_predict_points(self, slot, Xs, D, E, output=-1, Z_all=None):
        self.calls.append(("points", output, Z_all))
        rows = E if output < 0 else 1
        return np.arange(rows * len(Xs), dtype=float).reshape(rows, len(Xs)), np.full((rows, len(Xs)), 4.0)

    def gp_predict_points_cov(self, slot, Xs, D, E, output=-1, Z_all=None):
        self.calls.append(("cov", output, Z_all))
        rows = E if output < 0 else 1
        return np.zeros((rows, len(Xs))), np.stack([np.eye(len(Xs))] * rows)

    def gp_sample_points(self, slot, Xs, D, E, S, output=-1, Z_all=None, seed=0, draws=None, jitter=1e-6, parts=False):
        self.calls.append(("sample", output, Z_all, S, seed, draws, jitter))
        rows, Nt = (E if output < 0 else 1), len(Xs)
        z = np.ones((S, Nt, rows)) if draws is None else np.asarray(draws)
        return z.copy(), dict(mean=np.zeros((rows, Nt)), cov=np.stack([np.eye(Nt)] * rows), chol=np.stack([np.eye(Nt)] * rows), draws=z)


def _models():
    from pilco_amd.models import MGPR, SMGPR
    rs = np.random.RandomState(0)
    X, Y = rs.rand(12, 3), rs.rand(12, 2)
    return MGPR((X, Y), ctx=FakeContext()), SMGPR((X, Y), num_induced_points=4, ctx=FakeContext()), rs.rand(5, 3)


def test_python_layer_shapes_refusals_and_smgpr_s_own_inducing_inputs():
    m, s, xs = _models()
    Nt, E = 5, 2
    for model in (m, s):
        mean, cov = model.predict_f(xs, full_cov=True)
        assert mean.shape == (Nt, E) and cov.shape == (E, Nt, Nt)
        m1, c1 = model.models[1].predict_f_full_cov(xs)
        assert m1.shape == (Nt, 1) and c1.shape == (1, Nt, Nt) and model.ctx.calls[-1][1] == 1
        assert model.predict_f_samples(xs, 3).shape == (3, Nt, E) and model.predict_f_samples(xs).shape == (Nt, E)
        assert model.models[0].predict_f_samples(xs, 3).shape == (3, Nt, 1) and model.models[0].predict_f_samples(xs).shape == (Nt, 1)
        assert model.predict_f_samples(xs, 3, full_cov=False).shape == (3, Nt, E)
        assert model.models[1].predict_f_samples(xs, full_cov=False).shape == (Nt, 1)
        smp, parts = model.predict_f_samples(xs, 3, return_parts=True)
        assert parts["mean"].shape == (Nt, E) and parts["cov"].shape == (E, Nt, Nt) and parts["chol"].shape == (E, Nt, Nt)
        assert parts["draws"].shape == (3, Nt, E)
        smp, parts = model.models[1].predict_f_samples(xs, return_parts=True)
        assert smp.shape == (Nt, 1) and parts["draws"].shape == (Nt, 1) and parts["mean"].shape == (Nt, 1)
        sm, pp = model.predict_f_samples(xs, 3, full_cov=False, seed=4, return_parts=True)
        assert np.array_equal(sm, np.asarray(pp["mean"])[None] + 2.0 * np.asarray(pp["draws"])) and pp["cov"] is None
        assert np.array_equal(sm, model.predict_f_samples(xs, 3, full_cov=False, draws=pp["draws"]))
        for call in (lambda: model.predict_f(xs, full_output_cov=True), lambda: model.models[0].predict_f(xs, full_output_cov=True),
                     lambda: model.models[0].predict_f(xs, full_cov=True, full_output_cov=True),
                     lambda: model.models[0].predict_f(xs, full_cov=True),     # (the view keeps refusing: predict_f_full_cov)
                     lambda: model.models[0].predict_y(xs, full_cov=True), lambda: model.models[0].predict_y(xs, full_output_cov=True),
                     lambda: model.predict_f_samples(xs, 3, full_output_cov=True),
                     lambda: model.models[0].predict_f_samples(xs, 3, full_output_cov=True)):
            with pytest.raises(NotImplementedError):
                call()
        sig = inspect.signature(type(model.models[0]).predict_f_samples).parameters
        assert [sig[k].default for k in ("num_samples", "full_cov", "full_output_cov", "seed", "draws", "jitter")] == [None, True, False, 0, None, 1e-6]
    assert all(call[2] is None for call in m.ctx.calls)
    own = [call[2] for call in s.ctx.calls]
    assert all(z is not None and z.shape == (2, 4, 3) for z in own)                       # SMGPR passes every output's own Z
    assert np.array_equal(own[0][1], s.models[1].inducing_variable.Z.numpy())


def test_draws_of_the_wrong_shape_are_refused_before_any_device_call():
    from pilco_amd import _lib
    m, s, xs = _models()

    class NoDevice:
        def __getattr__(self, name):
            raise AssertionError("the context was touched: " + name)

    for model in (m, s):
        model._ctx = NoDevice()
        for bad in (np.zeros((3, 5, 1)), np.zeros((2, 5, 2)), np.zeros((3, 4, 2)), np.zeros((5, 2))):
            with pytest.raises(ValueError, match="draws"):
                model.predict_f_samples(xs, 3, draws=bad)
            with pytest.raises(ValueError, match="draws"):
                model.predict_f_samples(xs, 3, draws=bad, full_cov=False)
        with pytest.raises(ValueError, match="draws"):
            model.models[0].predict_f_samples(xs, 3, draws=np.zeros((3, 5, 2)))
    # the binding itself refuses too, before it touches the library
    cx = object.__new__(_lib.Context)
    with pytest.raises(ValueError, match="draws"):
        _lib.Context.gp_sample_points(cx, 0, xs, 3, 2, 3, draws=np.zeros((3, 5, 1)))


# ------------------------------------------------------------------ the generated code
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_the_covariance_kernels_compile_without_atomics_or_scratch_and_pass_the_mfma_scanners(tmp_path):
    asm = str(tmp_path / "predict_cov.s")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
           "-mllvm", "-amdgpu-mfma-vgpr-form", "-S", "--cuda-device-only", "-o", asm, os.path.join(CSRC, "predict_cov.hip")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stderr[-2000:]
    text = open(asm).read()
    for k in ("k_predict_cov", "k_cov_draws", "k_cov_samples"):
        assert k in text
    assert "v_mfma_f64_16x16x4_f64" in text
    assert "global_atomic" not in text and "flat_atomic" not in text and "ds_add" not in text   # the sums run in a fixed order
    sizes = [int(m) for m in re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text)]
    assert sizes and max(sizes) == 0, sizes
    for tool in ("mfma_overlap_check.py", "mfma_hazard_check.py"):
        chk = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), asm], capture_output=True, text=True, timeout=300)
        assert chk.returncode == 0, "%s:\n%s" % (tool, chk.stdout[-3000:])
