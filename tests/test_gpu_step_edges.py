"""The GP moment-matching step (operand work, pair sums, mean block, reverse sweep) at its edge hyper-parameters and inputs
(cases: helpers/step_cases.py) against the 40-digit truth in tests/golden/step_edges.npz (oracle/mp_step.py; docs/step_edges.md).

One module-scoped context; every case uploads its model with caller-supplied factors (gp_set_factors), so the step's error is
not mixed with the factorisation's.
- values: every route of step_cases.routes -- gp_predict under pair-kernel variants 0 and 2 (1 where the library has it), and,
  read from rollout_tape's step record, the one-launch small step, the fused head and the three-kernel step.  Per entry
  |device - truth| <= K unit, K capped per class and block at 8 x the float64 restatement's own K (floor 4); every result finite;
  a second call repeats the bits; the rollout's route is asserted from last_route(), the model's padding from geometry(); the
  fused head and the three-kernel step agree to the bit; the joint Gaussian the link hands to the step is the case's input to
  the bit.
- the forward half of a value-and-gradient rollout (rollout_grad, W = 0 controller, ExponentialReward; H = 2, or 1 where the
  produced state is no covariance: helpers/step_reference.sweep_horizon), whose pair sums
  run in other code (small_sweep inside the head, or the reverse-sweep launch of bwd.hip): the state after step 0, read from
  the trajectory a seed callback is handed, against the truth's (M, S, V) carried through pilco.py:151-152 with its units
  (helpers/step_reference.state1); the reward against the restatement at the truth's states (TOL_FWD); under the Jacobian and
  the plain tape, the device and the host reverse chain, each asserted from last_route(); bitwise repeatable.
- gradients: gp_predict_vjp against the fixture's 40-digit central differences, normwise within max(TOL_GRAD, 8 x the error of
  torch autograd through oracle.torch_path).
- policy gradients through the step: rollout_grad's reward, dW and db at H = 3 with a non-zero W (step_cases.WGRAD_CASES) against
  50-digit central differences of the whole rollout on the case's factors, under the Jacobian tape, the host chain and the plain
  tape, each asserted from last_route(); tolerance normwise max(TOL_GRAD, 8 x autograd's error), the link's rule.
- the overflowing determinant: D = 32 with s = 1e10 diag(l^2); det B = (1 + 1e10)^32 is not a float64.  Either the call refuses,
  or every output is finite and within the units of the restatement's answer (c_a = 0)."""
import numpy as np
import pytest

from helpers import step_cases as sc
from helpers import step_reference as sr
from test_gpu_parity import _has_valu_kernel
from test_gpu_rollout_widths import _settings

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cx():
    from pilco_amd import _lib
    c = _lib.Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def has_valu(cx):
    return _has_valu_kernel(cx)


def _upload(cx, c, d):
    cx.gp_set_data(0, d["X"], np.zeros((c["N"], c["E"])))
    cx.gp_set_hyp(0, d["ls"], d["var"], d["noise"])
    cx.gp_set_factors(0, d["iK"], d["beta"])


def _policy(c):
    from pilco_amd import _lib
    E, U = c["E"], c["U"]
    if U == 0:
        return dict(kind=_lib.POLICY_NONE, state_dim=E, control_dim=0)
    return dict(kind=_lib.POLICY_LINEAR, state_dim=E, control_dim=U, W=np.zeros((U, E)), b=np.zeros(U), max_action=1.0, squash=True)


def _tape_step(c, rec):
    """[jm (D) | js (D, D) | s1 (E, D) | M (E) | S (E, E) | V (D, E)] of a step record."""
    E, D = c["E"], c["D"]
    o = D + D * D + E * D
    return (rec[:D], rec[D:D + D * D].reshape(D, D), rec[o:o + E][None, :], rec[o + E:o + E + E * E].reshape(E, E),
            rec[o + E + E * E:o + E + E * E + D * E].reshape(D, E))


def _assert_k(c, ks, what):
    for b, k in ks.items():
        print("K %-16s %-14s %-3s %10.3g  (cap %.3g)" % (c["name"], what, b, k, sr.cap_of(c, b)))
    bad = {b: (k, sr.cap_of(c, b)) for b, k in ks.items() if not k <= sr.cap_of(c, b)}
    assert not bad, "%s / %s: K over its cap: %s" % (c["name"], what, bad)


@pytest.mark.parametrize("c", sc.CASES, ids=sc.case_ids())
def test_values_on_every_route(cx, has_valu, c):
    d, fx = sr.case(c)
    g = sc.geometry(c)
    D = c["D"]
    try:
        _upload(cx, c, d)
        runs = {}
        for name, kind, kw, step in sc.routes(c):
            if kind == "grad" or (name == "predict_v1" and not has_valu):
                continue    # (the value-and-gradient rollouts: test_forward_half_of_a_value_and_gradient_rollout)
            _settings(cx, **kw)
            if kind == "predict":
                call = lambda: cx.gp_predict(0, d["m"], d["s"], D, c["E"])
                M, S, V = call()
                again = call()
                assert cx.geometry()["npad"] == g["npad"], (c["name"], name, cx.geometry())
            else:
                call = lambda: cx.rollout_tape(_policy(c), [], d["m0"], d["S0"], 1)
                jm, js, M, S, V = _tape_step(c, call()[4][0])
                rt = cx.last_route()
                again = _tape_step(c, call()[4][0])[2:]
                assert cx.last_route() == rt, (c["name"], name)
                assert rt["entry"] == 1 and rt["step"] == step and rt["H"] == 1 and rt["npad"] == g["npad"], (c["name"], name, rt)
                assert rt["KP"] == g["KP"] and rt["vsep"] == int(g["vsep"]) and rt["pair"] == (3 if step == 2 else 0), (c["name"], name, rt)
                # the link hands the step the case's input: the joint of the state with an action N(0, 0)
                assert np.array_equal(jm, d["m"].ravel()) and np.array_equal(js, d["s"]), (c["name"], name, "the joint Gaussian is not the case's input")
            assert all(np.array_equal(x, y) for x, y in zip((M, S, V), again)), "%s / %s: not bitwise repeatable" % (c["name"], name)
            assert np.all(np.isfinite(M)) and np.all(np.isfinite(S)) and np.all(np.isfinite(V)), (c["name"], name, "NaN / inf")
            _assert_k(c, sc.ks(M, S, V, fx), name)
            runs[name] = (M, S, V)
        # the fused head and the three-kernel step run the same code in the same order
        fused = "tape_no_small" if "tape_no_small" in runs else "tape_default"
        if fused in runs and "tape_three" in runs:
            assert all(np.array_equal(x, y) for x, y in zip(runs[fused], runs["tape_three"])), (c["name"], "fused head vs three-kernel step")
    finally:
        _settings(cx)


def test_the_pair_kernel_variant_knob_selects_another_kernel(cx):
    """last_route() does not cover gp_predict and no debug field reports the pair kernel that ran.  What can be shown: the
    stream-K kernel (variant 0) and the tiled one (variant 2) split a model of several tiles differently, so their sums differ
    in some bit while both are within the caps (test_values_on_every_route) -- the knob reaches gp_predict."""
    c = sc.by_name("n257_std")
    d, _ = sr.case(c)
    _upload(cx, c, d)
    try:
        out = []
        for v in (0, 2):
            cx.set_pair_kernel(v)
            out.append(np.concatenate([np.ravel(x) for x in cx.gp_predict(0, d["m"], d["s"], c["D"], c["E"])]))
    finally:
        cx.set_pair_kernel(0)
    assert not np.array_equal(out[0], out[1])
    assert np.abs(out[0] - out[1]).max() <= 1e-12 * np.abs(out[0]).max()


_SWEEP = [c for c in sc.CASES if any(r[1] == "grad" for r in sc.routes(c))]
TOL_FWD = 1e-9


@pytest.mark.parametrize("c", _SWEEP, ids=sc.case_ids(_SWEEP))
def test_forward_half_of_a_value_and_gradient_rollout(cx, c):
    from pilco_amd import _lib
    d, fx = sr.case(c)
    E, H = c["E"], sr.sweep_horizon(c, d, fx)
    m1, S1, um, uS = sr.state1(c, d, fx)
    cap_m, cap_S = sr.state1_caps(c)
    r_ref = sr.reward_ref(c, d, fx, H)
    g = sc.geometry(c)
    rw = [dict(kind=_lib.REWARD_EXPONENTIAL, coef=1.0, W=np.eye(E), t=np.zeros(E))]
    try:
        _upload(cx, c, d)
        for name, kind, kw, want in sc.routes(c):
            if kind != "grad":
                continue
            _settings(cx, **kw)
            seen = []

            def seeds(traj):
                seen.append(traj.copy())
                return np.zeros_like(traj)
            a = cx.rollout_grad(_policy(c), rw, d["m0"], d["S0"], H, seed_fn=seeds)
            rt = cx.last_route()
            b = cx.rollout_grad(_policy(c), rw, d["m0"], d["S0"], H, seed_fn=seeds)
            what = "%s / %s" % (c["name"], name)
            assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(seen[0], seen[1]), (what, "not bitwise repeatable")
            assert rt["entry"] == 2 and rt["H"] == H and rt["npad"] == g["npad"] and rt["tape"] == want["tape"] and rt["chain"] == want["chain"], (what, rt, want)
            if want["pair"] is not None:
                assert rt["pair"] == want["pair"], (what, rt, want)
            traj = seen[0]
            assert np.all(np.isfinite(traj)) and np.isfinite(a[0]) and np.all(np.isfinite(a[1])) and np.all(np.isfinite(a[2])), (what, "NaN / inf")
            assert np.array_equal(traj[0, :E], d["m0"].ravel()) and np.array_equal(traj[0, E:].reshape(E, E), d["S0"]), what
            km = sc.k_of(traj[1, :E], m1, um)
            kS = sc.k_of(traj[1, E:].reshape(E, E), S1, uS)
            rerr = max(abs(a[0] - r_ref) - 4 * sc.TINY, 0.0) / max(abs(r_ref), sc.TINY)   # (a reward that underflows: absolute)
            print("F %-16s %-16s pair %d tape %d chain %d  K m %.3g (cap %.3g) S %.3g (cap %.3g) reward %.2e" % (c["name"], name, rt["pair"], rt["tape"], rt["chain"], km, cap_m, kS, cap_S, rerr))
            assert km <= cap_m and kS <= cap_S, (what, km, cap_m, kS, cap_S)
            assert rerr <= TOL_FWD, (what, a[0], r_ref)
    finally:
        _settings(cx)


@pytest.mark.parametrize("c", sc.GRAD_CASES, ids=sc.case_ids(sc.GRAD_CASES))
def test_vjp_vs_40_digit_central_differences(cx, c):
    d, fx = sr.case(c)
    tol_m, tol_s = sr.grad_tol(c)
    _upload(cx, c, d)
    call = lambda: cx.gp_predict_vjp(0, d["m"], d["s"], d["Mbar"], d["Sbar"], d["Vbar"], c["D"], c["E"])
    mbar, sbar = call()
    again = call()
    assert np.array_equal(mbar, again[0]) and np.array_equal(sbar, again[1]), (c["name"], "not bitwise repeatable")
    em, es = sr.block_error(mbar, fx["gm"]), sr.block_error(sbar, fx["gs"])
    print("G %-16s dm %.2e (tol %.1e)  ds %.2e (tol %.1e)" % (c["name"], em, tol_m, es, tol_s))
    assert em <= tol_m and es <= tol_s, (c["name"], em, tol_m, es, tol_s)


@pytest.mark.parametrize("c", sc.WGRAD_CASES, ids=sc.case_ids(sc.WGRAD_CASES))
def test_policy_gradients_vs_truth(cx, c):
    from helpers import link_cases as lc
    from pilco_amd import _lib
    d, t = sr.wgrad_case(c)
    tol, _ = sr.wgrad_tol(c)
    E, U, H = c["E"], c["U"], sc.WGRAD_H
    pol = dict(kind=_lib.POLICY_LINEAR, state_dim=E, control_dim=U, W=d["W"], b=d["b"], max_action=1.0, squash=True)
    rw = [dict(kind=_lib.REWARD_EXPONENTIAL, coef=1.0, W=np.eye(E), t=np.zeros(E))]
    dev = lc.rev_chain_supported(E, U)
    try:
        _upload(cx, c, d)
        got = {}
        for name, kw, want in (("default", {}, dict(tape=2, chain=1 if dev else 2)), ("host_chain", dict(dev_chain=0), dict(tape=2, chain=2)),
                               ("plain_tape", dict(grad_mode=0), dict(tape=1, chain=2))):
            _settings(cx, **kw)
            g = cx.rollout_grad(pol, rw, d["m0"], d["S0"], H)
            rt = cx.last_route()
            g2 = cx.rollout_grad(pol, rw, d["m0"], d["S0"], H)
            what = "%s / %s" % (c["name"], name)
            assert g[0] == g2[0] and np.array_equal(g[1], g2[1]) and np.array_equal(g[2], g2[2]), (what, "not bitwise repeatable")
            assert rt["entry"] == 2 and rt["H"] == H and rt["tape"] == want["tape"] and rt["chain"] == want["chain"], (what, rt, want)
            errs = (abs(g[0] - t["R"]) / abs(t["R"]), sr.block_error(np.reshape(g[1], (U, E)), t["dW"]), sr.block_error(np.ravel(g[2]), t["db"]))
            print("W %-12s %-10s chain %d tape %d pair %d  reward %.2e dW %.2e db %.2e" % ((c["name"], name, rt["chain"], rt["tape"], rt["pair"]) + errs))
            assert all(e <= tl for e, tl in zip(errs, tol)), (what, errs, tol)
            got[name] = g
    finally:
        _settings(cx)


def test_a_determinant_that_overflows_is_refused_or_finite(cx):
    """det B = (1 + 1e10)^32 > 1.8e308: the reference's formula gives c_a = var / sqrt(inf) = 0 and stays finite.  (Before the
    guard in det_rsqrt, csrc/mm_device.h: the Newton steps of the reciprocal square root made NaN of the overflowed determinant
    -- M, S and V were NaN with status OK.)"""
    from pilco_amd import _lib
    c = sc.by_name("d32_std")
    d, _ = sr.case(c)
    s = 1e10 * np.diag(d["ls"][0] ** 2)
    d = dict(d, s=s)
    with np.errstate(all="ignore"):
        Mo, So, Vo = sr.restatement(d)
    assert np.all(np.isfinite(So)) and np.all(Mo == 0.0) and np.all(Vo == 0.0)
    _upload(cx, c, d)
    for variant in (0, 2):
        cx.set_pair_kernel(variant)
        try:
            try:
                M, S, V = cx.gp_predict(0, d["m"], s, c["D"], c["E"])
            except _lib.PilcoError:
                continue    # a refusal is an answer
        finally:
            cx.set_pair_kernel(0)
        assert np.all(np.isfinite(M)) and np.all(np.isfinite(S)) and np.all(np.isfinite(V)), (variant, M, S, V)
        # the restatement's answer: M = V = 0 and S = var exactly (c_a = 0 and 1 / sqrt(det R) = 0); units: the clamp floor of
        # the absolute weight sums is 0 x anything = 0 here, var_a remains: 2^-53 var for S, 2^-1022 for M and V
        assert np.all(np.abs(M) <= 4 * sc.TINY) and np.all(np.abs(V) <= 4 * sc.TINY), (variant, M, V)
        assert np.all(np.abs(S - So) <= 4 * sc.EPS * np.abs(So)), (variant, S, So)
