"""The edge table of the GP posterior at test points (helpers/predict_cases.py) and its fixture (tests/golden/predict_edges.npz), on
the CPU: the coverage guard, the fixture's own conditions, the 40-digit truth (oracle/mp_predict.py) against the existing
40-digit evaluations and recomputed on two cases, K_ref of both float64 restatements per case and block, the caps recomputed,
and the sensitivity of the units: every mutant of the restatement exceeds the device's cap by more than 100 times.
docs/predict_edges.md."""
import os

import numpy as np
import pytest

from helpers import predict_cases as pc
from helpers import predict_edges_reference as pr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ------------------------------------------------------------------ the table
def test_every_family_point_and_shape_has_a_witness_on_every_route():
    assert pc.missing(pc.CASES) == []
    assert len(set(pc.case_ids())) == len(pc.CASES) <= 45
    for c in pc.CASES:
        assert pc.routes(c), c["name"]
        ls, var, noise = pc.hyper(c)
        if c["E"] > 1:      # an output index on the wrong row of ls, var or noise shows
            assert not np.array_equal(ls[0], ls[1]) or c["fam"] in ("ls_short", "ls_flat", "flat_floor"), c["name"]
            assert var[0] != var[1] and (noise[0] != noise[1] or c["fam"] == "dup"), c["name"]


@pytest.mark.parametrize("gone", ["x24_ls_ard", "f10_ls_ard", "x24_noise_m10,x65_noise_m10,x200_noise_m10", "f10_var_mixed", "x24_y0", "f10_dup", "x65_dup", "x200_noise_m10",
                                  "x65_flat_floor", "x24d1_std", "x24d9_std", "f65_std", "f130_std",
                                  "x200_noise_floor,x200_noise_m10,x200_flat_floor"])
def test_the_guard_sees_a_sole_witness_go(gone):
    names = gone.split(",")
    assert pc.missing([c for c in pc.CASES if c["name"] not in names]), gone


def test_a_case_without_a_route_and_a_missing_point_kind_are_reported(monkeypatch):
    monkeypatch.setattr(pc, "routes", lambda c: ())
    assert any("has no route" in m for m in pc.missing(pc.CASES[:1]))
    monkeypatch.undo()
    monkeypatch.setattr(pc, "point_kinds", lambda c: tuple(k for k in pc.POINT_KINDS if k != "denorm"))
    assert any("pt:denorm" in m for m in pc.missing(pc.CASES))


def test_shapes_are_the_smallest_that_reach_each_path():
    assert max(c["N"] for c in pc.CASES) == 200 and max(len(pc.point_kinds(c)) for c in pc.CASES) <= 8
    big = [c for c in pc.CASES if c["N"] == 200]
    assert len(big) <= 3 and all(c["E"] == 1 for c in big)


# ------------------------------------------------------------------ the fixture
def test_fixture_is_small_complete_and_meets_the_tables_conditions():
    assert os.path.getsize(pr.PATH) <= 263 * 1024
    for c in pc.CASES:
        d, truths = pr.case(c)
        kinds = pc.point_kinds(c)
        z = d["zeros"]
        assert d["xs"].shape == (len(kinds), c["D"]) and np.array_equal(z, pc.declared_zeros(c)), c["name"]
        P = d["Z"][0] if c["M"] else d["X"]
        assert np.array_equal(d["xs"][kinds.index("on")], d["X"][5]) and (not c["M"] or np.array_equal(d["xs"][kinds.index("on_z")], P[3])), c["name"]
        k = pc.se_ard(P, d["xs"][kinds.index("denorm")][None], d["ls"][0], d["var"][0])
        assert np.any((k > 0) & (k < pc.TINY)) and np.any(k == 0.0), c["name"]
        for e in range(c["E"]):
            for Pe in ([d["X"]] if not c["M"] else [d["Z"][0], d["Z"][e]]):
                assert np.all(pc.se_ard(Pe, d["xs"][kinds.index("far40")][None], d["ls"][e], d["var"][e]) == 0.0), c["name"]
        for tn, fx in truths.items():
            for key, v in fx.items():
                assert np.all(np.isfinite(v)), (c["name"], tn, key)
                assert key[0] != "u" or np.all(v >= pc.TINY), (c["name"], tn, key)
            assert np.all(fx["mean"][z[:, :, 0]] == 0.0) and np.all(fx["dmean"][z[:, :, 2]] == 0.0) and np.all(fx["dvar"][z[:, :, 3]] == 0.0), c["name"]
            assert np.all((fx["var"] == d["var"][:, None])[z[:, :, 1]]), c["name"]
            if tn == "t":    # on a training point: where a bound relative to sf2 sees nothing
                v = fx["var"][:, kinds.index("on")]
                assert np.all(v > 0.0) and np.all(v < 10.0 * d["noise"]), (c["name"], v)
        if c["fam"] == "dup":
            assert 0.0 < np.linalg.norm(d["X"][1] - d["X"][0]) <= 1.01e-7
    d = pr.case(pc.by_name("f10_var_tiny"))[0]
    assert d["var"].max() < pc.JITTER        # Kuu + jitter I is the jitter, nearly
    assert pr.case(pc.by_name("x24_noise_m10"))[0]["noise"].min() == 1e-10


# ------------------------------------------------------------------ the truth
def test_two_truths_recomputed():
    from oracle import gen_golden_predict as gg, mp_predict
    assert len(gg.SUBSET) == 2
    for name in gg.SUBSET:
        c = pc.by_name(name)
        d, truths = pr.case(c)
        for tn, fx in truths.items():
            for e in range(c["E"]):
                r = gg.truth_of((c, d, tn, e))[3]
                for key in ("mean", "var", "dmean", "dvar"):
                    assert np.array_equal(r[key], fx[key][e]), (name, tn, e, key)
                for key in ("umean", "uvar", "udmean", "udvar"):
                    assert np.allclose(r[key], fx[key][e], rtol=1e-12, atol=0.0), (name, tn, e, key)
        assert mp_predict.DPS == 40


def test_the_truth_against_the_existing_40_digit_evaluations_on_the_low_noise_model(monkeypatch):
    """oracle/mp_predict.gpr (Cholesky route) against helpers/predict_jac_restatement.mp_jacobians and the variance check of
    tests/test_gpu_predict_points.py (both through the 40-digit inverse of oracle/mp_truth.factorize): two 40-digit evaluations of one
    function agree to the float64 rounding of their results."""
    import mpmath as mp
    from helpers import predict_jac_restatement as jr
    from oracle import mp_predict, mp_truth
    g = np.load(os.path.join(GOLDEN, "predictions_lownoise.npz"))
    cfg = {k: g[k][..., :1] if k == "Y" else g[k] if k == "X" else g[k][:1] for k in ("X", "Y", "lengthscales", "variance", "noise")}   # output 0
    X, ls, sf2 = cfg["X"], cfg["lengthscales"], cfg["variance"]
    rs = np.random.RandomState(9)
    xs = X.min(0) + (X.max(0) - X.min(0)) * rs.rand(3, X.shape[1])
    cache = {}
    plain = mp_truth.factorize
    monkeypatch.setattr(mp_truth, "factorize", lambda *a, **kw: cache.setdefault("f", plain(*a, **kw)))
    dm, dv = jr.mp_jacobians(cfg, xs)
    iKs, betas = mp_truth.factorize(X, cfg["Y"], ls, sf2, cfg["noise"])
    f = mp.mpf
    for e in range(1):
        r = mp_predict.gpr(X, cfg["Y"][:, e], ls[e], sf2[e], cfg["noise"][e], xs)
        for t, x in enumerate(xs):
            k = mp.matrix([f(sf2[e]) * mp.exp(-sum(((f(X[i, d]) - f(x[d])) / f(ls[e, d])) ** 2 for d in range(X.shape[1])) / 2)
                           for i in range(X.shape[0])])
            want_v, want_m = float(f(sf2[e]) - (k.T * iKs[e] * k)[0]), float((k.T * betas[e])[0])
            assert abs(r["var"][t] - want_v) <= 2 * pc.EPS * abs(want_v) and abs(r["mean"][t] - want_m) <= 2 * pc.EPS * abs(want_m), (e, t)
        # (two 40-digit results that cancel by up to 1e9 differ by 1e-30: they round to the same float64, or to neighbours)
        assert np.allclose(r["dmean"], dm[e], rtol=2 * pc.EPS, atol=0.0) and np.allclose(r["dvar"], dv[e], rtol=2 * pc.EPS, atol=0.0), e
        assert np.all(r["uvar"] >= pc.EPS * sf2[e]) and np.all(r["umean"] > 0)


# ------------------------------------------------------------------ K_ref and the caps
def test_k_ref_of_every_case_and_block_and_the_caps():
    caps = pr.compute_caps()
    stored = pr.stored_caps()
    assert set(caps) == set(stored)
    for c in pc.CASES:
        k = pr.k_ref(c)
        _, a, b = pr._KREF[c["name"]]
        big = [blk for blk in pc.BLOCKS if b[blk] > 10.0 * max(a[blk], 1e-3)]
        print("K_ref %-18s %-24s GPflow order %s | device order %s%s" % (c["name"], c["cls"], " ".join("%9.3g" % a[blk] for blk in pc.BLOCKS),
                                                                         " ".join("%9.3g" % b[blk] for blk in pc.BLOCKS),
                                                                         "  (b) > 10 (a): " + ",".join(big) if big else ""))
        assert all(np.isfinite(k[blk]) for blk in pc.BLOCKS), c["name"]
    for key in sorted(caps):
        print("cap %-26s %-5s %10.3g (stored %.3g)" % (key + (caps[key], stored[key])))
        assert stored[key] >= pr.CAP_FLOOR and 0.5 <= caps[key] / stored[key] <= 2.0, (key, caps[key], stored[key])
    assert len({c["cls"] for c in pc.CASES}) >= 2 * len(pc.FAMILIES)          # one class per family and kind, the ill-conditioned apart
    for f in pc.ILL:
        assert len({c["cls"] for c in pc.CASES if c["fam"] == f}) == len([c for c in pc.CASES if c["fam"] == f])


# ------------------------------------------------------------------ sensitivity
def test_a_mutated_restatement_exceeds_the_cap_by_100():
    """Every mutant of the device-ordered restatement is more than 100 caps away from the truth, by a finite number, in some
    block of some case; `flush` (k flushed to zero below 2^-1022) on the denormal point."""
    margins = {}
    for c in pc.CASES:
        d, truths = pr.case(c)
        den = pc.point_kinds(c).index("denorm")
        for mu in pr.MUTANTS:
            for tn, fx in truths.items():
                if tn == "t" and mu in ("no_jitter", "iat_sign"):         # (the exact GP has neither term)
                    continue
                try:
                    res = pr.restate_b(d, tn, mu)
                except np.linalg.LinAlgError:                              # (without its jitter Kuu may not factor: no witness)
                    continue
                if mu == "flush":
                    res = [r[:, den:den + 1] for r in res]
                    fxx = {k: v[:, den:den + 1] for k, v in fx.items()}
                else:
                    fxx = fx
                k = pc.ks(res, fxx)
                m = max(k[b] / pr.cap_of(c, b) for b in pc.BLOCKS)
                if np.isfinite(m) and m > margins.get(mu, (0.0, ""))[0]:
                    margins[mu] = (m, c["name"] + "/" + tn)
    for mu in pr.MUTANTS:
        m, name = margins.get(mu, (0.0, "-"))
        print("mutant %-12s margin %.3g (%s)" % (mu, m, name))
        assert m > 100.0, (mu, m, name)


def test_the_unmutated_restatement_is_no_mutant():
    for c in pc.CASES:
        d, truths = pr.case(c)
        for tn, fx in truths.items():
            k = pc.ks(pr.restate_b(d, tn), fx)
            assert all(k[b] <= pr.cap_of(c, b) for b in pc.BLOCKS), (c["name"], tn, k)
