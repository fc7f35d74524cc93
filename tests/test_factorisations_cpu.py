"""CPU side of tests/test_gpu_factorisations.py: the case table covers the factorisation's block structure (coverage guard), the
extended-precision truth is right (oracle/hp_factor.py against 40-digit mpmath and against float64 LAPACK), and the GPU
criteria would catch a plausible kernel bug (a NumPy restatement of launch_trtri's recursive doubling, broken on purpose)."""
import os
import re

import numpy as np
import pytest
import scipy.linalg as sla

from helpers import fact_cases as fc
from helpers.trtri_doubling import doubling as _doubling, trtri_levels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REQUIRED_NBLK = (1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 31, 32, 33, 65)


def _header_const(name):
    src = open(os.path.join(ROOT, "pilco_amd", "csrc", "common.h")).read()
    return int(re.search(rf"constexpr int {name} = (\d+);", src).group(1))


NB = _header_const("NB")
KSPLIT = _header_const("FITC_KSPLIT")


def _pad(n):
    return -(-n // NB) * NB


def ksplit_spans(Np):
    """The FITC_KSPLIT slices [kbeg, kend) of the V V^T product over Np data columns (k_gemm64, k_mode 0)."""
    span = (-(-Np // KSPLIT) + 15) & ~15
    return [(min(sp * span, Np), min(sp * span + span, Np)) for sp in range(KSPLIT)]


def classes(case):
    """The structural classes one case covers."""
    out = set()
    if case["M"] == 0:
        N = case["N"]
        npad = _pad(N)
        out.add(f"nblk={npad // NB}")
        out.add(f"N%64={N % 64}")
        if N in (1, 2):
            out.add(f"N={N}")
        if any(rows < h for h, _, rows in trtri_levels(npad)):
            out.add("trtri clipped sub-problem")
        for k in ("E", "D"):
            if case[k] in (1, 32):
                out.add(f"{k}={case[k]}")
        if case["noise"] <= 1e-6:
            out.add("noise 1e-6")
    else:
        M, N = case["M"], case["N"]
        Mp, Np = _pad(M), _pad(N)
        if M in (1, 63, 64, 65, 130):
            out.add(f"FITC M={M}")
        if M == N:
            out.add("FITC M=N")
        if Mp > Np:
            out.add("FITC Mp>Np")
        if any(b >= e for b, e in ksplit_spans(Np)):
            out.add("FITC empty split-K slice")
        if Np // 64 > Mp:
            out.add("FITC Np/64>Mp (Tscr partials)")
        if (N, M) == (5000, 200):
            out.add("FITC config-4 size")
    return out


REQUIRED = ({f"nblk={b}" for b in REQUIRED_NBLK} | {"N%64=0", "N%64=1", "N%64=63", "N=1", "N=2", "trtri clipped sub-problem",
            "E=1", "E=32", "D=1", "D=32", "noise 1e-6"} | {f"FITC M={m}" for m in (1, 63, 64, 65, 130)} |
            {"FITC M=N", "FITC Mp>Np", "FITC empty split-K slice", "FITC Np/64>Mp (Tscr partials)", "FITC config-4 size"})


def missing(cases):
    """The required classes `cases` leave uncovered, sorted; noise 1e-6 must reach at least four block counts."""
    have = set().union(*(classes(c) for c in cases)) if cases else set()
    miss = REQUIRED - have
    ill = {_pad(c["N"]) // NB for c in cases if c["M"] == 0 and c["noise"] <= 1e-6}
    if len(ill) < 4:
        miss.add(f"noise 1e-6 at >= 4 block counts (have {len(ill)})")
    return sorted(miss)


def test_case_table_covers_every_required_class():
    assert missing(fc.CASES) == []
    assert len(fc.BY_NAME) == len(fc.CASES)


def test_removing_a_case_names_what_only_it_covered():
    for i, c in enumerate(fc.CASES):
        rest = fc.CASES[:i] + fc.CASES[i + 1:]
        only = classes(c) & REQUIRED - set().union(*(classes(o) for o in rest))
        miss = missing(rest)
        assert set(only) <= set(miss), (c["name"], only, miss)
        if c["M"] == 0 and c["noise"] <= 1e-6 and len({_pad(o["N"]) // NB for o in rest if o["M"] == 0 and o["noise"] <= 1e-6}) < 4:
            assert any(m.startswith("noise 1e-6 at") for m in miss), (c["name"], miss)
        if not only and not any(m.startswith("noise 1e-6 at") for m in miss):
            assert miss == [], (c["name"], miss)


def test_structure_recomputation():
    """The restated launch_trtri / split-K structure at hand-checked sizes."""
    assert trtri_levels(64) == []
    assert trtri_levels(320) == [(64, 2, 128), (128, 1, 192), (256, 1, 64)]        # 5 blocks: the last level is clipped
    assert trtri_levels(1024) == [(64, 8, 64), (128, 4, 128), (256, 2, 256), (512, 1, 512)]
    assert ksplit_spans(64)[:5] == [(0, 16), (16, 32), (32, 48), (48, 64), (64, 64)]
    assert all(b < e for b, e in ksplit_spans(5056))


def test_case_data_has_its_conditioning():
    """cond(K + s2 I) (FITC: of B = Kmm + Kmn Lam^-1 Knm) in the case's class, on the cases small enough to decide here."""
    from oracle import hp_factor as hp
    for c in fc.CASES:
        if (c["M"] or c["N"]) > 600 or c["N"] > 1200:
            continue
        d = fc.make_data(c)
        n = c["M"] or c["N"]
        P = fc.probes(n)
        r = hp.fitc(d["X"], d["Y"], d["Z"], d["ls"], d["var"], d["noise"], P, lapack=False) if c["M"] else \
            hp.exact(d["X"], d["Y"], d["ls"], d["var"], d["noise"], P, lapack=False)
        if c["cls"] == "well":
            assert np.max(r["cond"]) < (1e5 if c["M"] else 1e4), (c["name"], r["cond"])
        else:
            assert 3e7 < np.min(r["cond"]) and np.max(r["cond"]) < 1e10, (c["name"], r["cond"])


# ---------------------------------------------------------------- the truth itself
def _small(N, ill):
    rs = np.random.RandomState(N + 100 * ill)
    D, E = 3, 2
    if ill:
        X = 0.1 * rs.randn(N, D)
        var, noise = np.array([60.0, 50.0]), np.array([1e-6, 1e-6])
    else:
        X = 1.5 * rs.randn(N, D)
        var, noise = np.array([1.0, 0.7]), np.array([1e-2, 3e-2])
    ls = 1.0 + 0.3 * rs.rand(E, D)
    Y = np.sin(X @ rs.randn(D, E)) + 1e-3 * rs.randn(N, E)
    return X, Y, ls, var, noise


@pytest.mark.parametrize("ill", [False, True], ids=["well", "cond1e9"])
def test_hp_factor_matches_40_digit_truth(ill):
    from oracle import hp_factor as hp
    from oracle import mp_truth
    X, Y, ls, var, noise = _small(20, ill)
    P = fc.probes(20)
    r = hp.exact(X, Y, ls, var, noise, P)
    iKs, betas = mp_truth.factorize(X, Y, ls, var, noise, dps=40)
    for a in range(2):
        b40 = np.array([float(v) for v in betas[a]])
        iK40 = np.array(iKs[a].tolist(), dtype=float)
        eb = np.linalg.norm(r["beta"][a] - b40) / np.linalg.norm(b40)
        ep = np.linalg.norm(r["iKP"][a] - iK40 @ P) / np.linalg.norm(iK40 @ P)
        if ill:
            assert 3e8 < r["cond"][a] < 3e9, r["cond"]
            # about cond * 2^-64, and far below float64 LAPACK's error on the same case
            assert eb < 1e-3 * r["lapack_beta"][a] and ep < 1e-3 * r["lapack_iKP"][a], (eb, ep, r["lapack_beta"], r["lapack_iKP"])
        else:
            assert eb < 2e-16 and ep < 2e-16, (eb, ep)
        assert np.isclose(r["nlml"][a], float(_nlml40(iKs[a], betas[a], Y[:, a], X, ls[a], var[a], noise[a])), rtol=1e-12)


def _nlml40(iK, beta, y, X, ls, var, noise):
    import mpmath as mp
    N = len(y)
    yb = sum(mp.mpf(y[i]) * beta[i] for i in range(N))
    return yb / 2 - mp.log(mp.det(iK)) / 2 + N * mp.log(2 * mp.pi) / 2


def test_hp_factor_matches_lapack_on_well_conditioned_cases():
    from oracle import hp_factor as hp
    from oracle import tf_path as tp
    for name in ("e_n63", "e_n319"):
        d = fc.make_data(fc.BY_NAME[name])
        P = fc.probes(len(d["X"]))
        r = hp.exact(d["X"], d["Y"], d["ls"], d["var"], d["noise"], P, full_iK=True)
        iK, beta = tp.calculate_factorizations(d["X"], d["Y"], d["ls"], d["var"], d["noise"])
        for a in range(len(beta)):
            assert np.linalg.norm(beta[a] - r["beta"][a]) / np.linalg.norm(r["beta"][a]) < 1e-12
            assert np.linalg.norm(iK[a] - r["iK"][a]) / np.linalg.norm(r["iK"][a]) < 1e-12
    for name in ("f_m64_n64", "f_m130_n100"):
        d = fc.make_data(fc.BY_NAME[name])
        P = fc.probes(len(d["Z"]))
        r = hp.fitc(d["X"], d["Y"], d["Z"], d["ls"], d["var"], d["noise"], P)
        assert np.max(r["lapack_beta"]) < 1e-11 and np.max(r["lapack_iKP"]) < 1e-11, r


# ---------------------------------------------------------------- sensitivity of the GPU criteria
def _emulate(d, a, **kw):
    from oracle import hp_factor as hp
    N = len(d["X"])
    npad = _pad(N)
    A = np.eye(npad)
    A[:N, :N] = hp.gram(d["X"], d["X"], d["ls"][a], d["var"][a]).astype(np.float64) + d["noise"][a] * np.eye(N)
    Li = _doubling(np.linalg.cholesky(A), **kw)[:N, :N]
    return Li.T @ Li, Li.T @ (Li @ d["Y"][:, a])


@pytest.mark.parametrize("name,rel", [("e_n319", 1e-10), ("e_n575_ill", 3e-9)])
def test_criteria_catch_a_dropped_or_perturbed_tile(name, rel):
    """The restated doubling meets the GPU criteria; dropping the clipped last sub-problem, or scaling the last block row's
    first 64 x 64 tile of L^-1 by 1 + rel, misses at least one of them by >= 10x.  (A tile off by 1e-12 moves the normwise
    measures by about an eighth of their limits, well- and ill-conditioned alike: below what a normwise criterion can tell
    from rounding.)"""
    import test_gpu_factorisations as g
    from oracle import hp_factor as hp
    case = fc.BY_NAME[name]
    d = fc.make_data(case)
    N = case["N"]
    P = fc.probes(N)
    r = hp.exact(d["X"], d["Y"], d["ls"], d["var"], d["noise"], P)

    def worst(iK, beta):
        """The largest of the GPU test's measures over its limit (<= 1: passes)."""
        eb = np.linalg.norm(beta - r["beta"][0]) / np.linalg.norm(r["beta"][0])
        ep = np.linalg.norm(iK @ P - r["iKP"][0]) / np.linalg.norm(r["iKP"][0])
        res = hp.residual(d["X"], d["Y"][:, 0], d["ls"][0], d["var"][0], d["noise"][0], beta) / (g.C_RES * N * g.EPS)
        if case["cls"] == "well":
            return max(eb / g.TOL_WELL, ep / g.TOL_WELL, res)
        return max(eb / r["lapack_beta"][0] / g.RATIO_ILL, ep / r["lapack_iKP"][0] / g.RATIO_ILL, res)

    nblk = _pad(N) // NB
    assert worst(*_emulate(d, 0)) <= 1.0
    assert worst(*_emulate(d, 0, drop_clipped=True)) >= 10.0
    assert worst(*_emulate(d, 0, perturb=(nblk - 1, 0, rel))) >= 10.0
