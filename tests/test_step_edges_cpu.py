"""The edge-input table of the GP moment-matching step (helpers/step_cases.py) and its fixture (tests/golden/step_edges.npz), on the
CPU: the coverage guard, the fixture's own conditions, oracle/mp_step against oracle/mp_truth.moments_mp, three truths
recomputed, K_ref per case and block and the caps recomputed, the gradient truth against autograd, and the sensitivity of the
units: every mutant of the restatement exceeds the device's cap by more than 100 times.  docs/step_edges.md."""
import os

import numpy as np
import pytest

from helpers import step_cases as sc
from helpers import step_reference as sr


# ------------------------------------------------------------------ the table
def test_every_dimension_has_a_witness_on_every_route_it_can_reach():
    assert sc.missing(sc.CASES) == []
    assert len(set(sc.case_ids())) == len(sc.CASES)
    for c in sc.CASES:
        assert sc.routes(c), c["name"]


@pytest.mark.parametrize("gone", ["cov_corr12", "cov_negeig", "ls_off", "var_mixed", "mean_far30", "mean_below", "beta_cancel", "ik_asym",
                                  "d15_std", "d32_det290", "n256_std,n256_corr6", "n200_ard,n257_ard", "n257_straddle", "ik_none_p3",
                                  "d18_std,d18_p3", "e3_std,e3_mixed,d11_std,d11_mixed,d15_std"])
def test_the_guard_sees_a_sole_witness_go(gone):
    names = gone.split(",")
    assert sc.missing([c for c in sc.CASES if c["name"] not in names]), gone


def test_a_case_without_a_route_is_reported(monkeypatch):
    monkeypatch.setattr(sc, "route_classes", lambda c: set())
    assert any("has no route" in m for m in sc.missing(sc.CASES[:1]))


def test_shapes_are_the_smallest_that_reach_each_path():
    big = [c for c in sc.CASES if c["N"] >= 256]
    assert len(big) <= 10 and all(c["E"] <= 2 and c["D"] <= 4 for c in big)
    assert len(sc.GRAD_CASES) >= 10 and all(c["N"] <= 24 and c["D"] <= 4 for c in sc.GRAD_CASES)
    assert {c["cls"] for c in sc.GRAD_CASES} >= {"ordinary", "largecov", "corr", "mixed", "ls_flat", "ls_ard", "ls_crossed"}


# ------------------------------------------------------------------ the fixture
def test_fixture_is_small_complete_and_finite():
    assert os.path.getsize(sr.PATH) <= 300 * 1024
    for c in sc.CASES:
        d, fx = sr.case(c)
        for k, v in fx.items():
            assert np.all(np.isfinite(v)), (c["name"], k)     # (a determinant that is not positive would leave NaN in ldetB / ldetR)
        assert np.all(fx["uM"] >= sc.TINY) and np.all(fx["uS"] >= sc.TINY) and np.all(fx["uV"] >= sc.TINY), c["name"]
        assert np.array_equal(fx["S"], fx["S"].T), c["name"]
        if d["iKt"] is not None:
            assert np.array_equal(d["iKt"], np.swapaxes(d["iKt"], 1, 2)), c["name"]
        if c["mean"] == "straddle":
            assert np.any((fx["xr"][:, 0] < sc.CLAMP) & (fx["xr"][:, 1] > sc.CLAMP)), c["name"]
        if c["mean"] == "below":
            assert np.all(fx["xr"][:, 1] < sc.CLAMP), c["name"]
        if c["mean"] == "on":
            assert np.all(fx["xr"][:, 1] == 0.0), c["name"]    # the zero zeta row
        if c["beta"] == "zero":
            assert np.all(fx["M"] == 0.0) and np.all(fx["V"] == 0.0), c["name"]
        if c["beta"] == "cancel":
            assert np.all(np.abs(fx["M"]) < 1e-8 * fx["uM"] / sc.EPS), c["name"]
    c = sc.by_name("d32_det290")
    fx = sr.case(c)[1]
    assert 270 < fx["ldetB"][0] < 308 and 280 < fx["ldetR"][0, 0] < 308, (fx["ldetB"], fx["ldetR"])
    assert np.log(1e6 * 1e6) > 27.6 and sr.case(sc.by_name("var_huge"))[0]["var"].max() == 1e6


def test_asymmetric_ik_reaches_the_device_asymmetric():
    d = sr.case(sc.by_name("ik_asym"))[0]
    assert not np.allclose(d["iK"], np.swapaxes(d["iK"], 1, 2)) and np.array_equal(d["iKt"], 0.5 * (d["iK"] + np.swapaxes(d["iK"], 1, 2)))


def test_large_model_factors_are_rebuilt_to_the_bit():
    """iK_a = diag(d_a) - outer(g_a, g_a): one correctly rounded product and at most one correctly rounded subtraction per entry."""
    c = sc.by_name("n257_std")
    d = sr.case(c)[0]
    f = sr.get("_model/n257")
    E, N = c["E"], c["N"]
    dd, g = f[E * N:2 * E * N].reshape(E, N), f[2 * E * N:].reshape(E, N)
    for a in range(E):
        ref = np.array([[(dd[a, i] if i == j else 0.0) - g[a, i] * g[a, j] for j in range(0, N, 37)] for i in range(0, N, 41)])
        assert np.array_equal(d["iK"][a][::41, ::37], ref)


# ------------------------------------------------------------------ the truth
@pytest.mark.parametrize("name", ["e2u2_std", "e3_std"])
def test_mp_step_against_moments_mp(name):
    import mpmath as mp
    from oracle import mp_step, mp_truth
    c = sc.by_name(name)
    d, _ = sr.case(c)
    mp.mp.dps = 40
    f = mp.mpf
    N, E, D = c["N"], c["E"], c["D"]
    iKm = []
    for a in range(E):
        A = mp.matrix(N, N)
        for i in range(N):
            for j in range(N):
                A[i, j] = f(float(d["iKt"][a, i, j]))
        iKm.append(A)
    bm = [mp.matrix([f(float(d["beta"][a, i])) for i in range(N)]) for a in range(E)]
    mm, sm = mp_step._mp_inputs(d["m"], d["s"], D)
    M, S, V = mp_truth.moments_mp(d["X"], d["ls"], d["var"], (iKm, bm), mm, sm)
    r = mp_step.step_mp(d["X"], d["ls"], d["var"], mm, sm, d["iK"], d["beta"], units=False)
    rel = lambda a, b: abs(a - b) / abs(b)
    worst = max([rel(r["M"][a], M[a]) for a in range(E)] + [rel(r["S"][(min(a, b), max(a, b))], S[a, b]) for a in range(E) for b in range(E)] +
                [rel(r["V"][a][k], V[a][k]) for a in range(E) for k in range(D)])
    print("mp_step vs moments_mp %s: %s" % (name, mp.nstr(worst, 3)))
    assert worst < mp.mpf("1e-35")


def test_three_truths_recomputed():
    from oracle import gen_golden_step as gg, mp_step
    assert len(gg.SUBSET) == 3
    for name in gg.SUBSET:
        c = sc.by_name(name)
        d, fx = sr.case(c)
        r = mp_step.step(d["X"], d["ls"], d["var"], d["m"], d["s"], d["iK"], d["beta"])
        for k in ("M", "S", "V"):
            assert np.array_equal(r[k], fx[k]), (name, k)
        for k in ("uM", "uS", "uV"):
            assert np.allclose(r[k], fx[k], rtol=1e-12, atol=0.0), (name, k)


def test_gradient_truth_against_autograd_and_the_measured_tolerance():
    """The fixture's central differences against torch autograd through oracle.torch_path: the tolerance the GPU test holds
    pilco_gp_predict_vjp to is max(TOL_GRAD, 8 x this error)."""
    for c in sc.GRAD_CASES:
        d, fx = sr.case(c)
        gm, gs = sr.autograd_gradient(d)
        em, es = sr.block_error(gm, fx["gm"]), sr.block_error(gs, fx["gs"])
        print("autograd vs 40-digit differences %-12s dm %.2e ds %.2e -> tol %.1e %.1e" % ((c["name"], em, es) + sr.grad_tol(c)))
        assert np.array_equal(fx["gs"], fx["gs"].T)
        assert em < 1e-6 and es < 1e-6, c["name"]     # the differences are gradients of the same function


def test_policy_gradient_truth_against_autograd():
    """The 50-digit central differences of the H = 3 rollout (reward, dW, db) against torch autograd on the same factors: the GPU
    test's tolerance is max(TOL_GRAD, 8 x this error)."""
    assert len(sc.WGRAD_CASES) >= 10 and {c["ls"] for c in sc.WGRAD_CASES} >= {"std", "ard", "crossed", "flat"}
    for c in sc.WGRAD_CASES:
        assert c["N"] <= 24 and c["D"] <= 4 and c["U"] > 0
        d, t = sr.wgrad_case(c)
        tol, errs = sr.wgrad_tol(c)
        print("autograd vs 50-digit differences %-12s reward %.2e dW %.2e db %.2e -> tol %.1e %.1e %.1e" % ((c["name"],) + errs + tol))
        assert np.abs(d["W"]).min() > 0 and np.abs(t["dW"]).max() > 0 and np.abs(t["db"]).max() > 0, c["name"]
        assert max(errs) < 1e-6, (c["name"], errs)


# ------------------------------------------------------------------ K_ref and the caps
def test_k_ref_of_every_case_and_block_and_the_caps():
    caps = sr.compute_caps()
    stored = sr.stored_caps()
    assert set(caps) == set(stored)
    for c in sc.CASES:
        a, b = sr.k_ref(c), sr.k_ref_device_order(c)
        print("K_ref %-16s %-10s tf_path %s | device-ordered %s" % (c["name"], c["cls"], " ".join("%9.3g" % a[k] for k in sc.BLOCKS),
                                                                " ".join("%9.3g" % b[k] for k in sc.BLOCKS)))
        assert all(np.isfinite(min(a[k], b[k])) for k in sc.BLOCKS), c["name"]
    for key in sorted(caps):
        print("cap %-12s %-3s %10.3g (stored %.3g)" % (key + (caps[key], stored[key])))
        assert stored[key] >= 4.0 and 0.5 <= caps[key] / stored[key] <= 2.0, (key, caps[key], stored[key])


def test_the_plain_mutable_restatement_is_no_mutant():
    for c in sc.CASES:
        d, fx = sr.case(c)
        k = sc.ks(*sr.mutable_step(d), fx)
        ref = sr.k_ref(c)
        assert all(k[b] <= max(8.0 * ref[b], 4.0) for b in sc.BLOCKS), (c["name"], k, ref)


def test_reward_restatement_at_the_sweep_cases_states():
    """The reward the GPU test compares a value-and-gradient rollout's with is oracle.tf_path's at the truth's states: within
    1e-12 of the 50-digit evaluation (TOL_FWD is 1e-9)."""
    from oracle import mp_link as ml
    n = 0
    for c in sc.CASES:
        if not any(r[1] == "grad" for r in sc.routes(c)):
            continue
        d, fx = sr.case(c)
        H = sr.sweep_horizon(c, d, fx)
        m1, S1, _, _ = sr.state1(c, d, fx)
        E = c["E"]
        want = ml.exponential_reward(ml.vec(d["m0"]), ml.mat(d["S0"], E, E), ml.mat(np.eye(E), E, E))[0]
        if H == 2:
            want += ml.exponential_reward(ml.vec(m1), ml.mat(S1, E, E), ml.mat(np.eye(E), E, E))[0]
        got = sr.reward_ref(c, d, fx, H)
        assert abs(got - float(want)) <= 1e-12 * abs(float(want)) + 4 * sc.TINY, (c["name"], got, float(want))
        n += H == 2
    assert n >= 12     # the produced state is a covariance, and the reward sees it, in most cases


# ------------------------------------------------------------------ sensitivity
def test_a_mutated_restatement_exceeds_the_cap_by_100():
    """Every mutant must be more than 100 caps away from the truth in some block of some case; `no_v` (the vsep layouts' failure
    mode) on a vsep and on a non-vsep case."""
    margins = {}
    for c in sc.CASES:
        d, fx = sr.case(c)
        vsep = bool(sc.geometry(c)["vsep"])
        for mu in sr.MUTANTS:
            try:
                k = sc.ks(*sr.mutable_step(d, mu), fx)
            except np.linalg.LinAlgError:      # (R without the + I is singular at s = 0: no witness)
                continue
            m = max(k[b] / sr.cap_of(c, b) for b in sc.BLOCKS)
            if not np.isfinite(m):             # (a NaN is no measurement either: the witness must be a finite, wrong number)
                continue
            key = (mu, vsep) if mu == "no_v" else (mu,)
            if m > margins.get(key, (0.0, ""))[0]:
                margins[key] = (m, c["name"])
    for key in [(mu,) for mu in sr.MUTANTS if mu != "no_v"] + [("no_v", True), ("no_v", False)]:
        m, name = margins.get(key, (0.0, "-"))
        print("mutant %-22s margin %.3g (%s)" % (" ".join(map(str, key)), m, name))
        assert m > 100.0, (key, m, name)
