"""The case table of the sharded rollout tests (helpers/shard_cases.py), checked on the CPU.

Mirror check: a host-only probe compiles csrc/grad_layout.h (rev_dims, jac_gather) as it is and the host chain's assembly loop cut
out of csrc/grad_route.hip (forward_sharded), run on blocks whose every double holds its own index, so that what lands in the
assembled records names its source.  The library's pilco_shard_plan / _pair_slot / _output_slot give the ownership layout.  The
Python mirror must equal both for every E from 1 to 17, every W from 1 to 16, U in {0, 1, 4} and H in {0, 1, 3}, and there: the
pair slots partition the P pairs, the assembly map is a bijection onto JSg, the output records come from a rank that has pairs,
the blocks of different ranks do not overlap.

Mutants: PLcap by floor, out_off from P, kk % W and kk / W swapped, gblk from H: each fails its named check and the probe
comparison.

Coverage: every class of helpers/shard_cases.REQUIRED is reached; removing the only case of a class names it.

Sensitivity: the value of a single pair of the first step zeroed, or taken from its neighbour's slot in the dealing order, is put
into the NumPy step of helpers/widths_reference.py and the step run again, for the pair whose value (or whose difference to its
neighbour) is the smallest: the state that follows is more than the forward tolerance from the oracle's -- an exchange that
loses or misplaces one pair cannot pass the comparisons with the oracle."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from helpers import shard_cases as sc
from helpers import widths_reference as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pilco_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
ES, WS, US, HS = range(1, 18), range(1, 17), (0, 1, 4), (0, 1, 3)


def _block(src, head):
    """The text of the brace-matched block that starts with `head`."""
    i = src.index(head)
    assert src.find(head, i + 1) < 0, "more than one " + head
    j = src.index("{", i)
    depth = 0
    for k in range(j, len(src)):
        depth += {"{": 1, "}": -1}.get(src[k], 0)
        if depth == 0:
            return src[i:k + 1]
    raise AssertionError("unbalanced braces after " + head)


def probe_source():
    loop = _block(open(os.path.join(CSRC, "grad_route.hip")).read(), "for (int t = 0; t < H; ++t) {\n        double* dst = gc.jrec")
    assert "kk % W" in loop and "kk / W" in loop, loop
    return r'''#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "grad_layout.h"
using namespace pilco;
int main(int argc, char** argv) {
    const int mode = atoi(argv[1]);
    std::vector<double> all, rec;
    for (int E = 1; E <= 17; ++E)
        for (int W = 1; W <= 16; ++W)
            for (int U : {0, 1, 4})
                for (int H : {0, 1, 3}) {
                    const int D = E + U;
                    const RevDims d = rev_dims(E, U, D);
                    const JacGather gg = jac_gather(D, E, W, H);
                    if (mode == 0) {
                        std::printf("%d %d %d %d %d %d %d %d %zu %zu %zu %zu\n", E, W, U, H, d.recp, d.reco, gg.P, gg.PLcap, gg.out_off, gg.gstep, gg.gblk, gg.JSg);
                        continue;
                    }
                    // mode 1: the assembly loop on blocks whose doubles hold their own index
                    const size_t n_all = (size_t)W * gg.gblk, n_rec = (size_t)H * gg.JSg;
                    if (all.size() < n_all) {
                        const size_t o = all.size();
                        all.resize(n_all);
                        for (size_t i = o; i < n_all; ++i) all[i] = (double)i;
                    }
                    rec.assign(n_rec + 1, -1.0);
                    struct { double* jrec; } gc{rec.data()};
                    const double* h_all = all.data();
                    ''' + loop + r'''
                    // per step and record (P pair records, then the E output records as one): first source index, contiguous?
                    for (int t = 0; t < H; ++t)
                        for (int k = 0; k <= gg.P; ++k) {
                            const size_t o = (size_t)t * gg.JSg + (size_t)k * d.recp, len = k < gg.P ? (size_t)d.recp : (size_t)E * d.reco;
                            bool ok = true;
                            for (size_t i = 0; i < len; ++i) ok = ok && rec[o + i] == rec[o] + (double)i;
                            std::printf("%d %d %d %d %d %d %.0f %d\n", E, W, U, H, t, k, rec[o], ok ? 1 : 0);
                        }
                }
    return 0;
}
'''


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("shard_probe")
    src = d / "shard_probe.hip"
    src.write_text(probe_source())
    exe = d / "shard_probe"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                        "-I/opt/rocm/include", str(src), "-o", str(exe)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    out = {}
    for mode in ("0", "1"):
        txt = subprocess.run([str(exe), mode], capture_output=True, text=True, timeout=600, check=True).stdout
        out[mode] = [[int(x) for x in ln.split()] for ln in txt.split("\n") if ln.strip()]
    gather = {tuple(v[:4]): v[4:] for v in out["0"]}
    asm = {}
    for v in out["1"]:
        asm.setdefault(tuple(v[:4]), []).append(tuple(v[4:]))
    assert len(gather) == len(ES) * len(WS) * len(US) * len(HS)
    return gather, asm


def _grid():
    for E in ES:
        for W in WS:
            for U in US:
                for H in HS:
                    yield E, W, U, H


def gather_mismatches(probe, mirror=sc.Mirror):
    """(E, W, U, H) at which the mirror's jac_gather or assembly map differs from the compiled header and loop."""
    gather, asm = probe
    bad = []
    for E, W, U, H in _grid():
        m = mirror(E, U, W, H)
        g = m.jac_gather()
        want = [m.recp, m.reco, g["P"], g["PLcap"], g["out_off"], g["gstep"], g["gblk"], g["JSg"]]
        rows = [(t, dst // m.recp if dst < m.P * m.recp else m.P, blk * g["gblk"] + off, 1) for t, dst, ln, blk, off in m.assembly()]
        if gather[(E, W, U, H)] != want or asm.get((E, W, U, H), []) != rows:
            bad.append((E, W, U, H))
    return bad


def plan_mismatches(mirror=sc.Mirror):
    """(E, D, W) at which the mirror's ownership layout differs from the library's pure host functions."""
    from pilco_amd import _lib
    bad = []
    for E in ES:
        for W in WS:
            for U in US:
                m = mirror(E, U, W)
                D = E + U
                ok = all(_lib.shard_plan(E, D, W, r) == m.plan(r) for r in range(W))
                ok = ok and all(_lib.shard_pair_slot(E, D, W, a, b) == m.pair_slot(a, b) == m.pair_slot(b, a) for a, b in sc.pairs_in_order(E))
                ok = ok and all(_lib.shard_output_slot(E, D, W, a) == m.output_slot(a) for a in range(E))
                if not ok:
                    bad.append((E, D, W))
    return bad


def test_mirror_matches_the_library_and_the_layout_header(probe):
    bad = plan_mismatches()
    assert not bad, "ownership mirror differs from pilco_shard_plan / _pair_slot / _output_slot at %d (E, D, W), first: %s" % (len(bad), bad[:3])
    bad = gather_mismatches(probe)
    assert not bad, "mirror differs from grad_layout.h / the assembly loop at %d (E, W, U, H), first: %s" % (len(bad), bad[:3])


def test_the_owner_of_a_pair_is_the_library_s():
    """pilco_shard_owner_of_pair needs a context; deal_pairs (csrc/api.hip) is restated by the slots: owner = slot / SEG."""
    for E, W in ((1, 3), (2, 4), (5, 2), (10, 8), (17, 16)):
        m = sc.Mirror(E, 1, W)
        for kk, (a, b) in enumerate(sc.pairs_in_order(E)):
            assert sc.pair_index(E, a, b) == kk == sc.pair_index(E, b, a)
            assert m.pair_slot(a, b) // m.SEG == m.owner_of_pair(kk) and (a != b or m.owner_of_output(a) == m.owner_of_pair(kk))


def test_layout_invariants_over_the_grid():
    for E, W, U, H in _grid():
        sc.check_layout(sc.Mirror(E, U, W, H))
    for E in ES:   # what a rank holds by class
        for W in WS:
            m = sc.Mirror(E, 0, W)
            for r in range(W):
                k = m.rank_class(r)
                assert (k == "none") == (m.PL(r) == 0) and (k == "offdiag") == (m.PL(r) > 0 and m.EL(r) == 0), (E, W, r, k)
                assert m.nd(r) == m.EL(r) and m.nd(r, iK=False) == 0
            assert m.rank_class(0) in ("both", "diag")   # rank 0 always has pairs: the output records are read from its block


def _mutant(**flags):
    return type("Mutant", (sc.Mirror,), flags)


MUTANTS = {"PLcap by floor": (dict(plcap_floor=True), "overlap: rank"),
           "out_off from P": (dict(outoff_from_P=True), "overlap: step"),
           "kk % W and kk / W swapped": (dict(swap_mod_div=True), "owner: pair"),
           "gblk with H instead of max(H, 1)": (dict(gblk_from_H=True), "gblk: a rank's block")}


@pytest.mark.parametrize("name", list(MUTANTS))
def test_a_mutant_of_the_mirror_fails_its_named_check(name, probe):
    flags, check = MUTANTS[name]
    mut = _mutant(**flags)
    seen = set()
    for E, W, U, H in _grid():
        try:
            sc.check_layout(mut(E, U, W, H))
        except AssertionError as e:
            seen.add(" ".join(str(e).split(" ")[:4]))
    assert any(msg.startswith(check) for msg in seen), "%s: the layout checks that failed: %s" % (name, sorted(seen))
    assert gather_mismatches(probe, mut) or plan_mismatches(mut), "%s passed the comparison with the library and the header" % name


def test_case_table_is_well_formed():
    names = [c["name"] for c in sc.CASES]
    assert len(set(names)) == len(names)
    for c in sc.CASES:
        assert c["ranks"] and all(2 <= W <= 8 for W in c["ranks"]), c["name"]
        assert c["H"] in c["horizons"] and set(c["horizons"]) <= {0, 1, 2, 3}, c["name"]
        assert not c["grad"] or (c["U"] > 0 and c["D"] <= 14 and (c["M"] or c["N"]) <= 1025), c["name"]
    assert max(W for c in sc.CASES for W in c["ranks"]) == 8


def test_case_table_reaches_every_class():
    for cap in (2048, 3072):
        missing = [k for k in sc.missing_classes(sc.CASES, cap) if "stream-K" not in k]
        assert not missing, "classes no case of helpers/shard_cases.py reaches: %s" % missing
    missing = sc.missing_classes(sc.CASES)
    assert not missing, "classes no case of helpers/shard_cases.py reaches: %s" % missing


def test_removing_the_only_case_of_a_class_fails_and_names_it():
    sole = 0
    for i, c in enumerate(sc.CASES):
        others = set()
        for j, o in enumerate(sc.CASES):
            if j != i:
                others |= sc.classes_of(o)
        own = (sc.classes_of(c) & sc.REQUIRED) - others
        if own:
            sole += 1
            missing = sc.missing_classes(sc.CASES[:i] + sc.CASES[i + 1:])
            assert set(missing) == own, (c["name"], missing, own)
    assert sole > 5
    # the benchmark's split, and the ranks that own off-diagonal pairs only
    assert "55 pairs over 8 ranks" in sc.missing_classes([c for c in sc.CASES if not (c["E"] == 10 and 8 in c["ranks"])])
    no_off = [c for c in sc.CASES if not any(sc.Mirror(c["E"], c["U"], W).rank_class(r) == "offdiag" for W in c["ranks"] for r in range(W))]
    assert "rank offdiag" in sc.missing_classes(no_off)


def _first_step(c, d):
    """The first dynamics step of case c: (M, S, V) of the GP, and the S block of the state that follows."""
    from oracle import tf_path as tp
    iK, beta = wr.factors(c, d)
    if c["factors"] == "user":
        iK = np.zeros_like(iK)
    m, s = np.asarray(d["m0"], np.float64).reshape(1, -1), np.asarray(d["S0"], np.float64)
    m_u, s_u, c_xu = wr.np_controller(c, d)(m, s)
    mj = np.concatenate([m, m_u], axis=1)
    s1 = np.concatenate([s, s @ c_xu], axis=1)
    sj = np.concatenate([s1, np.concatenate([(s @ c_xu).T, s_u], axis=1)], axis=0)
    M, S, V = tp.predict_given_factorizations_pairs(wr.points(c, d), d["ls"], d["var"], mj, sj, iK, beta)
    return np.asarray(M).ravel(), np.asarray(S), S + s + s1 @ V + V.T @ s1.T


@pytest.mark.parametrize("case", sc.CASES, ids=[c["name"] for c in sc.CASES])
def test_forward_tolerance_sees_a_lost_and_a_misplaced_pair(case):
    """What a rank contributes for pair (a, b) is g_ab = S_ab + M_a M_b - delta_ab var_a (the value in the gather buffer); the
    assembled S_ab = g_ab + delta_ab var_a - M_a M_b enters the next state's covariance as it is.  Every pair is screened by what
    its g_ab zeroed, or replaced by the next pair's of the dealing order, does to that entry; for the pair that moves it least,
    each damage is put into the NumPy step (widths_reference.pair_step) and the step run again: the state that follows must be
    more than TOL_FWD from the oracle's, in the norm the GPU test measures with."""
    d = sc.make_data(case)
    E = case["E"]
    M, S, _ = _first_step(case, d)
    order = sc.pairs_in_order(E)
    g = np.array([S[a, b] + M[a] * M[b] - (d["var"][a] if a == b else 0.0) for a, b in order])
    P = len(order)
    lost = min(range(P), key=lambda kk: abs(g[kk]))
    damages = [("lost", lost, lambda v, kk: 0.0)]
    if P > 1:
        moved = min(range(P), key=lambda kk: abs(g[kk] - g[(kk + 1) % P]))
        damages.append(("taken from the next pair's slot", moved, lambda v, kk: v[order[(kk + 1) % P]]))
    c1 = dict(case, H=1)
    user = case["factors"] == "user"
    ref, _ = wr.oracle_trajectory(c1, d, zero_iK=user)
    for what, kk, value in damages:
        def hook(vals, kk=kk, value=value):
            assert sorted(vals) == sorted(order)
            return {**vals, order[kk]: value(vals, kk)}
        traj, _ = wr.perturbed_trajectory(c1, d, zero_iK=user, pair_hook=hook)
        move = wr.normwise_error(traj, ref, E)
        print("%s: pair %s %s moves the next state by %.2e" % (case["name"], order[kk], what, move))
        assert move > sc.TOL_FWD, "%s: pair %s %s moves the next state by %.2e only" % (case["name"], order[kk], what, move)
