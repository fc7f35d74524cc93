"""The link-edge table (helpers/link_cases.py) without a GPU: coverage guard, the link's branch predicates against their Python
mirror (csrc/link_predicates.h compiled into a host probe), the fixture against a regenerated subset, K_ref of the float64
restatement for every case and block (the table of docs/link_edges.md), and the sensitivity of every class to a mutated
restatement (a mutant must exceed the device's cap by 100 x on a case of its class)."""
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

from helpers import link_cases as lc
from helpers import link_reference as lr
from helpers import widths_reference as wr
from oracle import tf_path as tp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pilco_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
BFS = (1, 6, 10, 30, 40, 64, 80, 256)


# ------------------------------------------------------------------ coverage guard
def classes_of(c, d=None):
    d = d or lc.make_data(c)
    out = set()
    if c["U"] > 0:
        out.add("standalone:" + lc.squash_class(c["E"], c["U"], c["policy"], True, c["bf"]))
        if not c["stage"]:
            out.add("rollout:" + lc.squash_class(c["E"], c["U"], c["policy"], False, c["bf"]))
            if c["grad"]:
                out.add("grad:" + lc.squash_class(c["E"], c["U"], c["policy"], False, c["bf"]))
        if not c["squash"]:
            out.add("squash=False")
        if d["maxact"] is None:
            out.add("max_action=None")
    elif not c["stage"]:
        out.add("rollout:none")
    if not c["stage"] and c["D"] > 16:
        out.add("three-kernel step")
    out.add("terms=%d" % len(d["rewards"]))
    for tm in d["rewards"]:
        if tm["kind"] == "exp":
            out.add("reward:" + lc.path_class(tm["W"]))
            if c["grad"] and not c["stage"]:
                out.add("grad reward:" + lc.path_class(tm["W"]))
                # which reverse chain the default call takes (asserted on the GPU: declared_grad); every case runs the host one
                chain = "device" if lc.declared_grad(c)["chain"] == 1 else "host"
                out.add("grad %s-chain reward:%s" % (chain, lc.path_class(tm["W"])))
                if c["reward"] in ("zp", "zp_asym"):
                    out.add("grad %s-chain reward:zero-pivot %s" % (chain, lc.path_class(tm["W"])))
            if tm["t"] is None:
                out.add("t=None")
        if tm["coef"] <= 0:
            out.add("coef<=0")
    out.add("psd switch:%s=%s" % (c["reward"], lc.reward_path(d["rewards"][0]["W"])[:8]) if c["reward"] in ("asym14", "asym12", "neg13", "neg3") else "-")
    if c["policy"] == "none" or c["U"] > 0:
        out.add("S0:" + c["s0"])
    if c["grad"] == "mp":
        out.add("grad truth S0:" + c["s0"])
        out.add("grad truth ctrl:" + c["ctrl"])
    if c["grad"] and c["U"] > 0:
        out.add("grad %s-chain:%s" % ("device" if lc.declared_grad(c)["chain"] == 1 else "host", lc.squash_class(c["E"], c["U"], c["policy"], False, c["bf"])))
    for b in c["exact0"]:
        out.add("exact0:" + b)
    if c["E"] + c["U"] > 32:
        out.add("D>32")
    return out - {"-"}


REQUIRED = {
    "rollout:lin_fused", "rollout:combine", "rollout:combine_rounds(2)", "rollout:rbf_inline", "rollout:rbf_own", "rollout:none",
    "standalone:combine", "standalone:combine_rounds(2)", "standalone:rbf_own", "grad:lin_fused", "grad:combine", "grad:combine_rounds(2)",
    "grad:rbf_inline", "grad:rbf_own", "three-kernel step", "squash=False", "max_action=None", "terms=0", "terms=1", "terms=4", "coef<=0", "t=None",
    "reward:rank0", "reward:0<rank<E", "reward:rank=E", "reward:general", "grad reward:rank0", "grad reward:0<rank<E", "grad reward:general",
    "psd switch:asym14=factored", "psd switch:asym12=general", "psd switch:neg13=factored", "psd switch:neg3=general", "D>32",
    "exact0:M", "exact0:S", "exact0:rmu", "exact0:rew",
    # both reverse chains: the reward paths and the zero-pivot pair under the device chain too (the host chain runs for every
    # gradient case); the squash classes each chain can take (two rounds need U >= 8, the device chain takes U <= 4)
    "grad device-chain reward:rank0", "grad device-chain reward:0<rank<E", "grad device-chain reward:rank=E", "grad device-chain reward:general",
    "grad device-chain reward:zero-pivot rank=E", "grad device-chain reward:zero-pivot general",
    "grad device-chain:lin_fused", "grad device-chain:combine", "grad host-chain:combine_rounds(2)", "grad host-chain:rbf_inline",
    # gradients by value (50-digit truth) at the magnitudes of the forward ladder
    "grad truth S0:zero", "grad truth S0:t8", "grad truth S0:x400", "grad truth ctrl:big6",
} | {"S0:" + s for s in lc.S0_ALL}


def missing_classes(cases):
    have = set()
    for c in cases:
        have |= classes_of(c)
    return REQUIRED - have


def test_table_reaches_every_class_and_every_case_runs_somewhere():
    assert 60 <= len(lc.CASES) <= 90, len(lc.CASES)
    assert len(set(lc.case_ids())) == len(lc.CASES)
    assert not missing_classes(lc.CASES), missing_classes(lc.CASES)
    for c in lc.CASES:
        assert lc.forward_routes(c), (c["name"], "runs on no route")
        assert c["grad"] in (None, "mp", "ag") and (not c["grad"] or (c["U"] > 0 and c["squash"] and not c["stage"])), c["name"]
    # the shapes the issue names
    sc = lambda E, U: lc.squash_class(E, U, "linear")
    assert sc(6, 4) == "lin_fused" and sc(5, 4) == "combine" and sc(3, 16) == "combine"
    assert sc(1, 8) == sc(2, 16) == sc(1, 31) == "combine_rounds(2)"
    assert lc.policy_action_fits(20, 20) and lc.policy_action_fits(32, 8) and not lc.policy_action_fits(32, 32)


def test_deleting_a_sole_witness_fails_the_guard():
    per = {c["name"]: classes_of(c) for c in lc.CASES}
    sole = 0
    for cls in REQUIRED:
        wit = [n for n, s in per.items() if cls in s]
        if len(wit) == 1:
            sole += 1
            assert cls in missing_classes([c for c in lc.CASES if c["name"] != wit[0]]), cls
    assert sole >= 5   # (the guard has teeth: several classes hang on one case each)


# ------------------------------------------------------------------ predicates: host probe against the Python mirror
PROBE = r'''#include <cstdio>
#include <cstdlib>
#include "link_predicates.h"
#include "reward_factor.h"
using namespace pilco;
int main(int argc, char** argv) {
    if (atoi(argv[1]) == 0) {
        for (int E = 1; E <= 31; ++E)
            for (int U = 1; E + U <= 32; ++U) {
                std::printf("%d %d %d %d", E, U, (int)squash_lin_fused_fits(U, E + U), squash_round_cap(E + U));
                const int bfs[] = {1, 6, 10, 30, 40, 64, 80, 256};
                for (int bf : bfs) std::printf(" %d", link_rbf_inline_lds_doubles(E, U, bf));
                std::printf("\n");
            }
        return 0;
    }
    FILE* f = std::fopen(argv[2], "r");   // matrices: E, then E*E values, until the end of the file
    int E;
    while (std::fscanf(f, "%d", &E) == 1) {
        std::vector<double> W((size_t)E * E), F;
        for (double& w : W) if (std::fscanf(f, "%lf", &w) != 1) return 2;
        const int r = psd_factor(W.data(), E, F);
        std::printf("%d", r);
        for (int i = 0; i < (r > 0 ? E * r : 0); ++i) std::printf(" %.17g", F[i]);
        std::printf("\n");
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("link_probe")
    src = d / "link_probe.hip"
    src.write_text(PROBE)
    exe = d / "link_probe"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-I" + CSRC, "-I/opt/rocm/include", str(src), "-o", str(exe)],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(exe)


def test_the_link_uses_the_probed_predicates():
    """The link expands the macros the probed functions are made of (link_predicates.h says why: a call changes the generated
    code), so what ties probe and kernel together is the text."""
    rd = lambda f: open(os.path.join(CSRC, f)).read()
    glue, hdr = rd("glue_device.h"), rd("link_predicates.h")
    assert "PILCO_SQUASH_ROUND_CAP(nm)" in glue and "PILCO_SQUASH_LIN_FUSED_FITS(U, L.nm)" in glue and "5 * (U * U + U) <= L.nm" not in glue
    assert "return PILCO_SQUASH_ROUND_CAP(nm);" in hdr and "return PILCO_SQUASH_LIN_FUSED_FITS(U, nm);" in hdr
    assert "link_rbf_inline_lds_doubles(E, U, bf)" in rd("glue.hip")
    assert "pilco::psd_factor(" in rd("rollout.hip") and "pilco::psd_factor(" in rd("grad.hip") and "<vector>" not in hdr


def test_predicates_match_the_python_mirror(probe):
    txt = subprocess.run([probe, "0"], capture_output=True, text=True, timeout=300, check=True).stdout
    rows = [[int(x) for x in ln.split()] for ln in txt.split("\n") if ln.strip()]
    assert len(rows) == sum(32 - E for E in range(1, 32))
    for E, U, fits, cap, *inl in rows:
        assert bool(fits) == lc.lin_fused_fits(U, E + U), (E, U)
        assert cap == lc.squash_round_cap(E + U), (E, U)
        assert inl == [lc.rbf_inline_lds_doubles(E, U, bf) for bf in BFS], (E, U)
        n = lc.squash_rounds(U, E + U)
        assert 1 <= n <= 2, (E, U, n)   # (squash_inplace collects the new covariance in registers: any number of rounds is sound)


def _factor_rows(probe, mats, tmp_path):
    p = tmp_path / "mats.txt"
    p.write_text("\n".join("%d %s" % (W.shape[0], " ".join("%.17g" % x for x in W.ravel())) for W in mats) + "\n")
    txt = subprocess.run([probe, "1", str(p)], capture_output=True, text=True, timeout=300, check=True).stdout
    out = []
    for ln, W in zip([x for x in txt.split("\n") if x.strip()], mats):
        v = ln.split()
        r, E = int(v[0]), W.shape[0]
        out.append((r, np.array([float(x) for x in v[1:]]).reshape(E, r) if r > 0 else None))
    return out


def test_psd_factor_rank_of_every_reward_weight(probe, tmp_path):
    mats, names = [], []
    for c in lc.CASES:
        for tm in lc.make_data(c)["rewards"]:
            if tm["kind"] == "exp":
                mats.append(tm["W"])
                names.append(c["name"])
    got = _factor_rows(probe, mats, tmp_path)
    assert len(got) == len(mats)
    for (r, F), W, nm in zip(got, mats, names):
        want = lc.reward_path(W)
        have = "rank0" if r == 0 else "general" if r < 0 else "factored(%d)" % r
        assert have == want, (nm, have, want)
        rp, Fp = lc.psd_factor(W)   # the Python port (the caps' K_ref is measured through it): the same factor
        assert rp == r, (nm, rp, r)
        if r > 0:   # the factor reproduces the weight up to what psd_factor drops by design: 1e-13 of the scale
            assert np.abs(F @ F.T - W).max() <= 4e-13 * np.abs(W).max(), (nm, np.abs(F @ F.T - W).max())
            assert np.abs(Fp - F).max() <= 1e-13 * np.abs(F).max(), (nm, np.abs(Fp - F).max())


# ------------------------------------------------------------------ truth vs fixture
def test_fixture_holds_every_case_and_regenerates_bitwise():
    pytest.importorskip("mpmath")
    from oracle import gen_golden_link as gg
    for c in lc.CASES:
        fx = lr.fixture(c)
        assert all(np.all(np.isfinite(v)) for v in fx.values()), c["name"]
        assert ("traj" in fx) == (not c["stage"]) and ("g0" in fx) == (c["grad"] == "mp"), c["name"]
    assert os.path.getsize(lr.GOLDEN) < 1 << 20
    for name in gg.SUBSET:
        c = lc.by_name(name)
        new, old = gg.truth_of(c), lr.fixture(c)
        assert set(new) == set(old), name
        for k in new:
            assert np.array_equal(new[k], old[k]), (name, k)


# ------------------------------------------------------------------ K_ref
def test_k_ref_of_every_case_and_block():
    """Prints the K_ref table and the caps; the restatement is a fair yardstick at the rollout level (TOL_FWD / 8)."""
    table = lr.k_ref_table()
    for c in lc.CASES:
        ks = table[c["name"]]
        print("K_ref %-22s %-12s %s" % (c["name"], c["group"], "  ".join("%s %.3g" % (b, k) for b, k in ks.items())))
        assert all(np.isfinite(k) for k in ks.values()), (c["name"], ks)
    new = lr.compute_caps()
    assert set(new) == set(lr.caps()), set(new) ^ set(lr.caps())
    for key, cap in sorted(lr.caps().items()):
        print("cap %-14s %-5s %.4g  (recomputed here: %.4g)" % (key[0], key[1], cap, new[key]))
        assert 0.5 * cap <= new[key] <= 2.0 * cap, (key, cap, new[key])   # (the stored caps are not one machine's accident)
    for c in lc.CASES:
        if c["stage"]:
            continue
        d, fx = lc.make_data(c), lr.fixture(c)
        traj, total, act = lr.np_rollout(c, d)
        err = wr.normwise_error(traj, fx["traj"], c["E"])
        r_ref = fx["rew"][-1]
        rerr = abs(total - r_ref) / max(abs(r_ref), 1e-300) if "rew" not in c["exact0"] else abs(total) / lc.TINY * 1e-300
        print("fwd   %-22s states %.2e reward %.2e" % (c["name"], err, rerr))
        assert max(err, rerr) <= lr.fwd_tol(c, d, fx) / 8 * (1 + 1e-12), (c["name"], err, rerr)
        assert lr.fwd_tol(c, d, fx) == lc.TOL_FWD or c["policy"] == "rbf", c["name"]


# ------------------------------------------------------------------ sensitivity
def _squash_mutant(kind, c):
    E, U = c["E"], c["U"]

    def squash(m, s, max_action=None):
        m = np.asarray(m, np.float64).reshape(1, -1)
        s = np.asarray(s, np.float64)
        k = m.shape[1]
        e = np.ones((1, k)) if max_action is None else max_action * np.ones((1, k))
        if kind == "maxact0":
            e = e[0, 0] * np.ones((1, k))
        ds = np.diag(s)
        lq = -(ds[:, None] + ds[None, :]) / 2.0
        q = np.exp(lq)
        cm, cp = np.cos(m.T - m), np.cos(m.T + m)
        if kind == "cos_swapped":
            cm, cp = cp, cm
        S = (np.exp(lq + (-s if kind == "exp_sign" else s)) - q) * cm - (np.exp(lq - s) - q) * cp
        S = e * e.T * S / 2.0
        M = e * np.exp(-ds / 2.0) * np.sin(m)
        C = e * np.diag(np.exp(-ds / 2.0) * np.cos(m[0]))
        if kind == "round2_skipped":   # items beyond the first round keep what the buffers held: the pre-squash values
            done = lc.squash_round_cap(E + U) // 5
            Sf = S.ravel().copy()
            Sf[done:] = s.ravel()[done:]
            S = Sf.reshape(k, k)
            for u in range(k):
                if k * k + u >= done:
                    M[0, u], C[u, u] = m[0, u], 0.0
        return M, S, C.reshape(k, k)
    return squash


def _mutant(kind, c):
    m = types.SimpleNamespace(linear_controller=tp.linear_controller, rbf_controller=tp.rbf_controller,
                              exponential_reward=tp.exponential_reward, linear_reward=tp.linear_reward)
    if kind in ("maxact0", "cos_swapped", "exp_sign", "round2_skipped"):
        sq = _squash_mutant(kind, c)

        def lin(mm, s, W, b, max_action=1.0, squash=True):
            M, S, V = tp.linear_controller(mm, s, W, b, max_action, False)
            if squash:
                M, S, V2 = sq(M, S, max_action)
                V = V @ V2
            return M, S, V
        m.linear_controller = lin
    elif kind == "no_1e-6":
        def rbf(mm, s, cX, cY, cl, max_action=1.0, squash=True):
            M, S, V = tp.rbf_controller(mm, s, cX, cY, cl, max_action, False)
            S = S - np.diag(np.full(S.shape[0], 1e-6))
            if squash:
                M, S, V2 = tp.squash_sin(M, S, max_action)
                V = V @ V2
            return M, S, V
        m.rbf_controller = rbf
    elif kind == "t_ignored":
        m.exponential_reward = lambda mm, s, W=None, t=None: tp.exponential_reward(mm, s, W, None)
    elif kind == "no_pivot":
        def gj(A, B):   # unpivoted Gauss-Jordan, as gauss_jordan_spd runs it
            A, B = A.copy(), B.copy()
            n = A.shape[0]
            det = 1.0
            with np.errstate(all="ignore"):
                for k in range(n):
                    p = A[k, k]
                    det *= p
                    A[k], B[k] = A[k] / p, B[k] / p
                    for r in range(n):
                        if r != k:
                            f_ = A[r, k]
                            A[r], B[r] = A[r] - f_ * A[k], B[r] - f_ * B[k]
            return B, det

        def ex(mm, s, W=None, t=None):
            mm = np.asarray(mm, np.float64).reshape(1, -1)
            E = mm.shape[1]
            dd = mm - (0.0 if t is None else np.asarray(t).reshape(1, E))
            out = []
            for sc in (1.0, 2.0):
                X, det = gj((np.eye(E) + sc * s @ W).T, W.T)   # X^T, X = W (I + sc S W)^-1
                with np.errstate(all="ignore"):
                    out.append(np.exp(-0.5 * sc * float((dd @ X.T @ dd.T)[0, 0])) / np.sqrt(det))
            return np.array([[out[0]]]), np.array([[out[1] - out[0] ** 2]])
        m.exponential_reward = ex
    elif kind == "rank_E":
        def ex(mm, s, W=None, t=None):   # the factor's E x (E - 1) buffer read with E columns
            mm = np.asarray(mm, np.float64).reshape(1, -1)
            E = mm.shape[1]
            lam, Q = np.linalg.eigh(W)
            F = (Q * np.sqrt(np.maximum(lam, 0.0)))[:, lam > 1e-15 * lam.max()]
            Fw = np.concatenate([F.ravel(), np.zeros(E * E - F.size)]).reshape(E, E)
            dd = (mm - (0.0 if t is None else np.asarray(t).reshape(1, E))).ravel()
            out = []
            for sc in (1.0, 2.0):
                y = Fw.T @ dd
                A = np.eye(E) + sc * Fw.T @ s @ Fw
                out.append(np.exp(-0.5 * sc * y @ np.linalg.solve(A, y)) / np.sqrt(np.linalg.det(A)))
            return np.array([[out[0]]]), np.array([[out[1] - out[0] ** 2]])
        m.exponential_reward = ex
    else:
        raise KeyError(kind)
    return m


def _rounds2(c):
    return c["policy"] == "linear" and lc.squash_rounds(c["U"], c["D"]) == 2 and c["squash"]


MUTANTS = {
    # mutant: (cases of its class, blocks it must move)
    "no_pivot": (lambda c: c["reward"] == "zp_asym", ("rmu", "rvar")),
    "round2_skipped": (_rounds2, ("M", "S", "V")),
    "maxact0": (lambda c: c["maxact"] == "mixed", ("M", "S", "V")),
    "cos_swapped": (lambda c: c["policy"] == "linear" and c["squash"] and c["U"] > 1 and c["s0"] != "zero" and c["ctrl"] != "W0", ("S",)),
    "no_1e-6": (lambda c: c["policy"] == "rbf", ("S",)),
    "exp_sign": (lambda c: c["policy"] == "linear" and c["squash"] and c["s0"] != "zero" and c["ctrl"] != "W0", ("S",)),
    "t_ignored": (lambda c: c["reward"] in ("std", "t8", "rank1", "rankEm1", "asym", "zp") and c["stage"] is False, ("rmu",)),
    "rank_E": (lambda c: c["reward"] == "rankEm1", ("rmu", "rvar")),
}


@pytest.mark.parametrize("kind", sorted(MUTANTS))
def test_a_mutated_restatement_exceeds_the_cap_by_100(kind):
    sel, blocks = MUTANTS[kind]
    cases = [c for c in lc.CASES if sel(c)]
    assert cases, kind
    best = {}
    for c in cases:
        d, fx = lc.make_data(c), lr.fixture(c)
        ks = lr.stage_k(c, d, fx, lr.np_stage(c, d, _mutant(kind, c)))
        margin = max(ks[b] / lr.cap_of(c, b) for b in blocks if b in ks)
        best[c["name"]] = margin
        print("mutant %-15s %-22s margin over the cap %.3g" % (kind, c["name"], margin))
    # every CLASS is caught with the margin; for the mutants whose class is a single mechanism (squash classes) every case is
    assert max(best.values()) >= 100.0, (kind, best)
    if kind in ("round2_skipped", "maxact0", "no_pivot", "rank_E"):
        assert min(best.values()) >= 100.0, (kind, best)
