"""The case table of the point-count tests (helpers/npoints_cases.py), checked on the CPU.

Mirror check: a host-only probe compiles the integer logic of the real host functions -- mm_prep_chunks (csrc/prep.hip),
pair_njb / mm_pair_nt / mm_pair_sk_steps (csrc/pair.hip), small_col_splits (csrc/rollout.hip), mm_bwd_geometry (csrc/bwd.hip),
cut out of their files with stand-ins for the device queries -- and the closed forms of the stream-K split from
csrc/pair_device.h as they are.  It must agree with the Python mirror on every npad from 64 to 8192 and every pair count P from
1 to 528.

Stream-K partition: for every npad, P, nd (diagonal pairs streaming iK) and a range of wave counts including the one build_work
computes, the boundaries are monotone and cover [0, T) exactly, sk_pair_waves agrees with them, whi - wlo + 1 stays within
mm_sk_maxw, and the computed cut keeps every wave within two pairs (sk_wave_range keeps two sums).  sk_max_pairs_per_wave, which
build_work uses to refuse PILCO_SK_WAVES / PILCO_SK_UNITS overrides, must agree with a step-by-step count.

Coverage: every geometry class (helpers/npoints_cases.REQUIRED) is reached; removing the only case of a class names it.

Sensitivity: for every case, two kernel errors -- the last real point left out of the pair sums, the first padded point let in
with the values a larger model left there -- must each move the trajectory by at least 10 x the forward tolerance."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from helpers import npoints_cases as nc
from helpers import widths_reference as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pilco_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
NPADS = range(64, 8192 + 1, 64)
PS = range(1, 529)


def _function(src, head):
    """The text of the function whose definition starts with `head` (brace matched)."""
    i = src.index(head)
    while src.find(";", i) < src.index("{", i):   # (a declaration: the definition comes later)
        i = src.index(head, i + 1)
    j = src.index("{", i)
    depth = 0
    for k in range(j, len(src)):
        depth += {"{": 1, "}": -1}.get(src[k], 0)
        if depth == 0:
            return src[i:k + 1]
    raise AssertionError("unbalanced braces after " + head)


def _e_of(P):
    E = 1
    while E * (E + 1) // 2 < P:
        E += 1
    return E


def probe_source():
    rd = lambda f: open(os.path.join(CSRC, f)).read()
    prep, pair, roll, bwd = rd("prep.hip"), rd("pair.hip"), rd("rollout.hip"), rd("bwd.hip")
    fns = [_function(prep, "void mm_prep_chunks(").replace("device_cus()", "g_cus"),
           _function(pair, "static int pair_njb("), _function(pair, "int mm_pair_nt("), _function(pair, "void mm_pair_sk_steps("),
           _function(bwd, "void mm_bwd_geometry(").replace("BWD_RT", "2"),
           _function(roll, "static int small_col_splits(").replace("device_cus_of(ctx->device)", "g_cus")]
    return r'''#include <cstdio>
#include <cstdlib>
#include "pair_device.h"
namespace pilco {
static int g_cus = 256;
struct ProbeWork { int NCH, NCHM, KP, PL, EL; };
struct ProbeSlot { int npad; ProbeWork wk; };
typedef ProbeSlot Slot;
typedef void pilco_ctx;
''' + "\n".join(fns) + r'''
}
using namespace pilco;
static int e_of(int P) { int E = 1; while (E * (E + 1) / 2 < P) ++E; return E; }
int main(int argc, char** argv) {
    const int mode = atoi(argv[1]);
    if (mode == 0) {   // geometry of every (npad, P)
        for (int npad = 64; npad <= 8192; npad += 64)
            for (int P = 1; P <= 528; ++P) {
                const int E = e_of(P);
                int nch, nchm, td, to, njs, nrb;
                mm_prep_chunks(npad, P, E, &nch, &nchm);
                mm_pair_sk_steps(npad, &td, &to);
                mm_bwd_geometry(npad, P, &njs, &nrb);
                Slot s{npad, {nch, nchm, 12, P, E}};
                std::printf("%d %d %d %d %d %d %d %d %d %d %d %d\n", npad, P, nch, nchm, mm_pair_nt(npad, 0, P), mm_pair_nt(npad, 2, P),
                            td, to, njs * nrb, small_col_splits(nullptr, s, true), small_col_splits(nullptr, s, false), pair_njb(npad, P));
            }
        return 0;
    }
    if (mode == 2) {   // sk_max_pairs_per_wave(waves, nd, tdiag, toff, n_pairs, ud, uo) of the arguments that follow
        std::printf("%d\n", sk_max_pairs_per_wave(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6]), atoi(argv[7]),
                                                  atoi(argv[8])));
        return 0;
    }
    // mode 1: stream-K partition invariants; prints one line per violation and a summary
    long bad = 0, checked = 0, worst_default = 0;
    const int fixed[] = {4, 8, 12, 64, 256, 1024, 2048, 3072};
    const int caps[] = {2048, 3072, 4096, 6144};
    for (int npad = 64; npad <= 8192; npad += 64)
        for (int P = 1; P <= 528; ++P)
            for (int ndk = 0; ndk < 2; ++ndk) {
                int tdiag, toff;
                mm_pair_sk_steps(npad, &tdiag, &toff);
                const int nd = ndk ? (e_of(P) < P ? e_of(P) : P) : 0;
                if (nd == 0) tdiag = toff;
                const long T = (long)nd * tdiag + (long)(P - nd) * toff;
                const int nd_steps = nd * tdiag;
                const int tb = (int)std::max<long>(4, (T + 3) / 4 * 4);
                int counts[16], nc = 0;
                for (int w : fixed) counts[nc++] = w;
                if (T < 8192) counts[nc++] = tb;
                for (int cap : caps) counts[nc++] = cap > T ? tb : cap;
                for (int ci = 0; ci < nc; ++ci) {
                    const int waves = counts[ci];
                    ++checked;
                    auto B = [&](int w) { return sk_boundary_of(w, waves, nd_steps, (int)T, 5, 4); };
                    if (B(0) != 0 || B(waves) != T) { ++bad; std::printf("ends %d %d %d %d\n", npad, P, nd, waves); continue; }
                    int prev = 0, most = 0;
                    bool mono = true;
                    for (int w = 1; w <= waves; ++w) {
                        const int b = B(w);
                        if (b < prev) mono = false;
                        if (b > prev) {   // wave w - 1 holds [prev, b): the pairs of its first and last step
                            auto pr = [&](int st) { return st < nd_steps ? st / tdiag : nd + (st - nd_steps) / toff; };
                            most = std::max(most, pr(b - 1) - pr(prev) + 1);
                        }
                        prev = b;
                    }
                    if (!mono) { ++bad; std::printf("monotone %d %d %d %d\n", npad, P, nd, waves); continue; }
                    if (most != sk_max_pairs_per_wave(waves, nd, tdiag, toff, P, 5, 4)) { ++bad; std::printf("maxpairs %d %d %d %d\n", npad, P, nd, waves); }
                    if (ci >= nc - 4) worst_default = std::max<long>(worst_default, most);
                    if (ci >= nc - 4 && most > 2) { ++bad; std::printf("three %d %d %d %d %d\n", npad, P, nd, waves, most); }
                    int maxw = 4;
                    for (int k = 0; k < P; ++k) {
                        int wlo, fs, whi;
                        sk_pair_waves(k, waves, nd, tdiag, toff, (int)T, 5, 4, wlo, fs, whi);
                        const long S0 = k < nd ? (long)k * tdiag : (long)nd_steps + (long)(k - nd) * toff;
                        const long S1 = S0 + (k < nd ? tdiag : toff);
                        const bool ok = wlo >= 0 && whi < waves && wlo <= whi && B(wlo) <= S0 && S0 < B(wlo + 1) && B(whi) <= S1 - 1 &&
                                        S1 - 1 < B(whi + 1) && fs == (B(wlo) < S0 ? 1 : 0);
                        if (!ok) { ++bad; std::printf("pairwaves %d %d %d %d k=%d\n", npad, P, nd, waves, k); break; }
                        maxw = std::max(maxw, whi - wlo + 1);
                    }
                    maxw = (maxw + 3) / 4 * 4;
                    for (int k = 0; k < P; ++k) {
                        int wlo, fs, whi;
                        sk_pair_waves(k, waves, nd, tdiag, toff, (int)T, 5, 4, wlo, fs, whi);
                        if (whi - wlo + 1 > maxw) { ++bad; std::printf("maxw %d %d %d %d\n", npad, P, nd, waves); break; }
                    }
                }
            }
    std::printf("summary %ld %ld %ld\n", checked, bad, worst_default);
    return 0;
}
'''


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("npoints_probe")
    src = d / "npoints_probe.hip"
    src.write_text(probe_source())
    exe = d / "npoints_probe"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                        "-I/opt/rocm/include", str(src), "-o", str(exe)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(exe)


def mirror_rows(m=nc):
    """What the Python mirror says for every (npad, P): the probe's mode-0 columns."""
    out = {}
    for npad in NPADS:
        for P in PS:
            E = _e_of(P)
            nch, nchm = m.prep_chunks(npad, P, E)
            td, to = m.sk_steps(npad)
            njs, nrb = m.bwd_geometry(npad, P)
            kp = 12
            out[(npad, P)] = (nch, nchm, m.pair_nt(npad, 0, P), m.pair_nt(npad, 2, P), td, to, njs * nrb,
                              m.small_col_splits(npad, nch, nchm, kp, P, E, True), m.small_col_splits(npad, nch, nchm, kp, P, E, False),
                              m.pair_njb(npad, P))
    return out


def mirror_mismatches(probe_exe, m=nc):
    got = {}
    txt = subprocess.run([probe_exe, "0"], capture_output=True, text=True, timeout=300, check=True).stdout
    for ln in txt.split("\n"):
        if ln.strip():
            v = [int(x) for x in ln.split()]
            got[(v[0], v[1])] = tuple(v[2:])
    want = mirror_rows(m)
    assert len(got) == len(want) == len(NPADS) * len(PS)
    return [(k, got[k], want[k]) for k in want if got[k] != want[k]]


def test_mirror_matches_the_host_functions(probe):
    bad = mirror_mismatches(probe)
    assert not bad, "Python mirror differs from the compiled host functions at %d (npad, P), first: %s" % (len(bad), bad[:3])


class _MisSized:
    """The mirror with one deliberate error: mm_prep_chunks' CU budget off by one workgroup."""
    def __getattr__(self, name):
        return getattr(nc, name)

    @staticmethod
    def prep_chunks(npad, PL, EL, cus=nc.CUS):
        return nc.prep_chunks(npad, PL, EL + 1, cus)


def test_mirror_check_rejects_a_mis_sized_mirror(probe):
    assert mirror_mismatches(probe, _MisSized()), "a mirror with a wrong CU budget passed the probe comparison"


def test_stream_k_partition_invariants(probe):
    txt = subprocess.run([probe, "1"], capture_output=True, text=True, timeout=900, check=True).stdout
    lines = [ln for ln in txt.split("\n") if ln.strip()]
    summary = [ln for ln in lines if ln.startswith("summary")]
    assert summary, txt[-2000:]
    checked, bad, worst = (int(x) for x in summary[0].split()[1:])
    assert checked > 100000
    assert bad == 0, "stream-K violations (first lines): %s" % lines[:10]
    assert worst == 2   # the computed cut does reach two pairs in one wave, never three


def test_an_override_that_spans_three_pairs_is_seen(probe):
    """The issue's example: PILCO_SK_WAVES=4, E = 3, npad = 64: 42 steps over 4 waves, pairs of 6 or 8 steps.  The compiled
    sk_max_pairs_per_wave (what build_work asks before it accepts an override) must see a wave spanning three pairs; the
    computed cut of the same model must not."""
    waves, T, tdiag, toff = nc.sk_cut(64, 6, 3, 4)
    assert (waves, T, tdiag, toff) == (4, 42, 6, 8)
    most = lambda w: int(subprocess.run([probe, "2", str(w), "3", str(tdiag), str(toff), "6", "5", "4"], capture_output=True, text=True,
                                        timeout=60, check=True).stdout)
    assert most(4) > 2
    assert most(nc.sk_cut(64, 6, 3, 3072)[0]) <= 2


def test_case_table_declares_what_the_mirror_computes():
    for c in nc.CASES:
        for cap in (nc.CAP_RANGE[0], 3072, nc.CAP_RANGE[1]):
            g = nc.geometry(c, nc.CUS, cap)
            for k in nc.DECLARED:
                assert c.get(k, False) == g[k], "%s: declares %s=%r, the mirror computes %r (capacity %d)" % (c["name"], k, c.get(k), g[k], cap)
    assert len({c["name"] for c in nc.CASES}) == len(nc.CASES)


def test_case_table_reaches_every_geometry_class():
    missing = nc.missing_classes(nc.CASES)
    assert not missing, "geometry classes no case of helpers/npoints_cases.py reaches: %s" % missing


def test_every_inducing_count_at_several_point_counts():
    ns = {}
    for c in nc.CASES:
        if c["M"]:
            ns.setdefault(c["M"], set()).add(c["N"])
    for M in (1, 63, 64, 65, 128, 192, 256, 257):
        assert len(ns.get(M, ())) >= 2, "M = %d at N = %s only" % (M, sorted(ns.get(M, ())))


def test_removing_the_only_case_of_a_class_fails_and_names_it():
    sole = 0
    for i, c in enumerate(nc.CASES):
        others = set()
        for j, o in enumerate(nc.CASES):
            if j != i:
                others |= nc.classes_of(o)
        own = (nc.classes_of(c) & nc.REQUIRED) - others
        if own:
            sole += 1
            missing = nc.missing_classes(nc.CASES[:i] + nc.CASES[i + 1:])
            assert set(missing) == own, (c["name"], missing, own)
    assert sole > 5
    # the issue's example: the gradient cases with an empty 64-row half block in the sweep's last 128-row block
    half = [c for c in nc.CASES if c["grad"] and nc.geometry(c)["half"]]
    assert half and "grad half block" in nc.missing_classes([c for c in nc.CASES if c not in half])


def _extra_point_trajectory(c, d):
    """The first padded point let in with the values of a model with one more point: its input, its beta column and its iK
    row / column stay where a larger model left them (buffers only grow), the first n points keep the current factors."""
    rs = np.random.RandomState(7)
    D = c["D"]
    x = rs.randn(1, D)
    if c["M"]:
        d2 = dict(d, Z=np.vstack([d["Z"], x]))
    else:
        y = 0.3 * np.sin(x @ np.ones((D, c["E"])) / np.sqrt(D))
        d2 = dict(d, X=np.vstack([d["X"], x]), Y=np.vstack([d["Y"], y]))
    iK, beta = wr.factors(c, d)
    iK2, beta2 = wr.factors(c, d2)
    n = iK.shape[1]
    iKa = iK2.copy()
    iKa[:, :n, :n] = iK
    betaa = beta2.copy()
    betaa[:, :n] = beta
    if c["factors"] == "user":
        iKa = np.zeros_like(iKa)
    pts = wr.points(c, d2)
    return wr._trajectory(lambda m, s: wr.pair_step(pts, d["ls"], d["var"], m, s, iKa, betaa), c, d)


def reference(c, d):
    """oracle trajectory of case c; user factors: beta of the exact model, no iK (gp_set_factors(iK=None))."""
    return wr.oracle_trajectory(c, d, zero_iK=c["factors"] == "user")


_FITC = [c for c in nc.CASES if c["M"]]


@pytest.mark.parametrize("case", _FITC, ids=[c["name"] for c in _FITC])
def test_fitc_cases_are_well_conditioned(case):
    """An inducing set that is nearly singular in few input dimensions (M = 128 points in D = 2: cond(Kmm) ~ 1e18) makes any
    two correct factorisations differ by far more than the forward tolerance: the table keeps cond(Kmm + 1e-6 I) below 1e8."""
    from oracle import tf_path as tp
    d = nc.make_data(case)
    for a in range(case["E"]):
        K = tp.se_ard_K(d["Z"], d["Z"], d["ls"][a], d["var"][a]) + 1e-6 * np.eye(case["M"])
        assert np.linalg.cond(K) < 1e8, "%s, output %d: cond(Kmm) %.1e" % (case["name"], a, np.linalg.cond(K))


@pytest.mark.parametrize("case", nc.CASES, ids=nc.case_ids())
def test_forward_tolerance_sees_a_dropped_point_and_an_admitted_padded_point(case):
    d = nc.make_data(case)
    ref, r_ref = reference(case, d)
    E = case["E"]
    assert np.abs(ref[-1, :E] - ref[0, :E]).max() > 1e-3, "%s: the states hardly move" % case["name"]
    if case["factors"] == "user":
        iK, beta = wr.factors(case, d)
        pts = wr.points(case, d)
        same = wr._trajectory(lambda m, s: wr.pair_step(pts, d["ls"], d["var"], m, s, np.zeros_like(iK), beta), case, d)[0]
        drop = wr._trajectory(lambda m, s: wr.pair_step(pts, d["ls"], d["var"], m, s, np.zeros_like(iK), beta, drop_point=True), case, d)[0]
    else:
        same = wr.perturbed_trajectory(case, d)[0]
        drop = wr.perturbed_trajectory(case, d, drop_point=True)[0]
    assert wr.normwise_error(same, ref, E) < 0.1 * nc.TOL_FWD
    for what, bad in (("the last real point left out", drop), ("the first padded point let in", _extra_point_trajectory(case, d)[0])):
        err = wr.normwise_error(bad, ref, E)
        assert err >= 10 * nc.TOL_FWD, "%s: %s moves the trajectory by %.2e only" % (case["name"], what, err)
