"""Rollouts and policy gradients at every input-width instantiation (cases: helpers/dims_cases.py).

Per case, on a context of its own:
- forward: rollout(want_traj=True) on every route the shape allows (default, no one-launch small step, three-kernel step, MFMA
  tiled pair kernel; for an RbfController inline on and off).  pilco_debug_last_route must name the route the case declares.
  Every state (m, S) and the reward against oracle.tf_path (FITC: tf_path.fitc_factorizations), normwise per step and per block
  (TOL_FWD); the routes against each other, bitwise where the launch structures run the same code in the same order (fused head
  vs three-kernel step, same policy evaluation, same pair kernel) and to TOL_ROUTES otherwise; every route bitwise repeatable.
- gradient (U > 0): reward and every entry of dW, db (RbfController: d centres, d targets, d lengthscales) against torch autograd
  through oracle.torch_path (TOL_GRAD) for the Jacobian tape, the plain tape, the device and the host reverse chain.
- lanes (one case per DT bucket): rollout_batch (B = 3) and rollout_grad_batch (B = 2) bit-identical to their solo calls."""
import numpy as np
import pytest

from helpers import dims_cases as dc
from helpers import widths_reference as wr

pytestmark = pytest.mark.gpu

STEP = {"fused": 1, "small": 2, "three": 3, "fused_rbf": 4}
_REF = {}


def _ref(case):
    if case["name"] not in _REF:
        d = dc.make_data(case)
        _REF[case["name"]] = (d, wr.oracle_trajectory(case, d))
    return _REF[case["name"]]


def _context(case, d):
    from pilco_amd import _lib
    cx = _lib.Context()
    cx.gp_set_data(0, d["X"], d["Y"])
    cx.gp_set_hyp(0, d["ls"], d["var"], d["noise"])
    if case["M"]:
        cx.gp_set_inducing(0, d["Z"])
    cx.gp_factorize(0)
    if case["policy"] == "rbf":
        U = case["U"]
        cx.gp_set_data(_lib.SLOT_POLICY, d["cX"], d["cY"])
        cx.gp_set_hyp(_lib.SLOT_POLICY, d["cl"], np.ones(U), 1e-4 * np.ones(U))
        cx.gp_factorize(_lib.SLOT_POLICY)
    return cx


def _policy(case, d, W=None, b=None):
    from pilco_amd import _lib
    E, U = case["E"], case["U"]
    if case["policy"] == "linear":
        return dict(kind=_lib.POLICY_LINEAR, state_dim=E, control_dim=U, W=d["W"] if W is None else W, b=d["b"] if b is None else b,
                    max_action=d["maxact"], squash=True)
    if case["policy"] == "rbf":
        return dict(kind=_lib.POLICY_RBF, state_dim=E, control_dim=U, max_action=d["maxact"], squash=True)
    return dict(kind=_lib.POLICY_NONE, state_dim=E, control_dim=0)


def _rewards(case, d):
    from pilco_amd import _lib
    ex = dict(kind=_lib.REWARD_EXPONENTIAL, W=d["Wr"], t=d["tr"].ravel())
    li = dict(kind=_lib.REWARD_LINEAR, W=d["Wl"].ravel())
    return {"exp": [dict(ex, coef=1.0)], "lin": [dict(li, coef=1.0)], "comb": [dict(ex, coef=0.7), dict(li, coef=-0.4)]}[case["reward"]]


def _settings(cx, small=1, fused=1, variant=0, inline=1, grad_mode=1, dev_chain=1):
    cx.set_small_step(small)
    cx.set_fused_step(fused)
    cx.set_pair_kernel(variant)
    cx.set_inline_policy(inline)
    cx.set_grad_mode(grad_mode)
    cx.set_reverse_chain(dev_chain)


def _forward_routes(case):
    """(name, settings) of every route the case's shape allows."""
    out = [("default", {}), ("no_small", dict(small=0)), ("three", dict(fused=0)), ("tiled", dict(variant=2))]
    if case["policy"] == "rbf":
        out += [("inline_off", dict(inline=0)), ("inline_off_three", dict(inline=0, fused=0))]
    return out


def _expected_forward(case, name, rt):
    """The witness of forward route `name` must show what the case declares (see dims_cases)."""
    fwd = case["fwd"]
    own = case.get("policy_route") == "own"
    if name == "default":
        exp_step = STEP[fwd]
    elif name in ("no_small", "tiled"):
        exp_step = STEP["fused"] if fwd == "small" else STEP[fwd]
    elif name == "inline_off":
        exp_step = STEP["fused_rbf"] if fwd in ("small", "fused", "fused_rbf") else STEP["three"]
    else:
        exp_step = STEP["three"]
    assert rt["step"] == exp_step, (name, rt)
    assert rt["entry"] == 1 and rt["H"] == case["H"] and rt["tape"] == 0, (name, rt)
    assert rt["DT"] == _dt(case["D"]) and rt["KP"] == _kp(case["D"]) and rt["vsep"] == int(_vsep(case["D"])), (name, rt)
    if case["policy"] == "rbf":
        inline = name in ("default", "no_small", "tiled") and not own and rt["step"] != STEP["three"]
        assert rt["policy"] == (1 if inline else 2), (name, rt)
    else:
        assert rt["policy"] == 0, (name, rt)
    if rt["step"] == STEP["small"]:
        assert rt["pair"] == 3, (name, rt)
    else:
        assert rt["pair"] == (2 if name == "tiled" else 0), (name, rt)


def _vsep(D):
    return (D + 2) % 4 == 1


def _kp(D):
    return D + 1 if _vsep(D) else (D + 2 + 3) // 4 * 4


def _dt(D):
    for lim, dt in ((4, 4), (6, 6), (8, 8), (10, 10), (11, 11), (12, 12), (14, 14), (16, 16)):
        if D <= lim:
            return dt
    return 32


def _check_forward(case, d, ref, r_ref, traj, rew, what):
    E = case["E"]
    err = wr.normwise_error(traj, ref, E)
    rerr = abs(float(np.asarray(rew).ravel()[0]) - r_ref) / max(abs(r_ref), 1e-300)
    assert err <= dc.TOL_FWD and rerr <= dc.TOL_FWD, "%s: states %.2e, reward %.2e (tol %.0e)" % (what, err, rerr, dc.TOL_FWD)
    return max(err, rerr)


def _bitwise_pair(ra, rb):
    """Two forward routes that run the same code in the same order: fused head (2 launches) vs three-kernel step, with the same
    evaluation of the policy and the same pair kernel (both produce bitwise identical results)."""
    return {ra["step"], rb["step"]} <= {1, 3, 4} and ra["policy"] == rb["policy"] and ra["pair"] == rb["pair"]


@pytest.mark.parametrize("case", dc.CASES, ids=dc.case_ids())
def test_forward_routes_vs_oracle_and_each_other(case):
    d, (ref, r_ref) = _ref(case)
    cx = _context(case, d)
    try:
        pol, rw = _policy(case, d), _rewards(case, d)
        runs = {}
        for name, kw in _forward_routes(case):
            _settings(cx, **kw)
            a = cx.rollout(pol, rw, d["m0"], d["S0"], case["H"], want_traj=True)
            rt = cx.last_route()
            b = cx.rollout(pol, rw, d["m0"], d["S0"], case["H"], want_traj=True)
            assert cx.last_route() == rt, name   # (the second call replays the captured graph)
            for x, y in zip(a, b):
                assert np.array_equal(x, y), "%s / %s: not bitwise repeatable" % (case["name"], name)
            E, H = case["E"], case["H"]
            assert np.array_equal(a[0].ravel(), a[3][H, :E]) and np.array_equal(a[1].ravel(), a[3][H, E:]), (case["name"], name)
            _expected_forward(case, name, rt)
            _check_forward(case, d, ref, r_ref, a[3], a[2], "%s / %s" % (case["name"], name))
            runs[name] = (a, rt)
        names = list(runs)
        for i, na in enumerate(names):
            for nb in names[i + 1:]:
                (a, ra), (b, rb) = runs[na], runs[nb]
                if _bitwise_pair(ra, rb):
                    assert np.array_equal(a[3], b[3]) and np.array_equal(a[2], b[2]), "%s: %s vs %s not bitwise" % (case["name"], na, nb)
                else:
                    err = wr.normwise_error(a[3], b[3], case["E"])
                    assert err <= dc.TOL_ROUTES, "%s: %s vs %s %.2e" % (case["name"], na, nb, err)
                    assert abs(a[2][0, 0] - b[2][0, 0]) <= dc.TOL_ROUTES * abs(b[2][0, 0]), (case["name"], na, nb)
    finally:
        cx.close()


_GRAD_CASES = [c for c in dc.CASES if c["U"] > 0]


@pytest.mark.parametrize("case", _GRAD_CASES, ids=[c["name"] for c in _GRAD_CASES])
def test_policy_gradients_vs_autograd(case):
    d, (ref, r_ref) = _ref(case)
    R, G = wr.torch_gradient(case, d)
    cx = _context(case, d)
    try:
        pol, rw = _policy(case, d), _rewards(case, d)
        H, D = case["H"], case["D"]
        modes = [("default", {}), ("host_chain", dict(dev_chain=0)), ("plain_tape", dict(grad_mode=0))]
        for name, kw in modes:
            _settings(cx, **kw)
            if case["policy"] == "rbf":
                call = lambda: cx.rollout_grad_rbf(pol, rw, d["m0"], d["S0"], H, d["cX"], d["cY"], d["cl"], 1e-4 * np.ones(case["U"]))
            else:
                call = lambda: cx.rollout_grad(pol, rw, d["m0"], d["S0"], H)
            g = call()
            rt = cx.last_route()
            g2 = call()
            assert g[0] == g2[0] and all(np.array_equal(x, y) for x, y in zip(g[1:], g2[1:])), (case["name"], name, "not repeatable")
            what = "%s / %s" % (case["name"], name)
            assert rt["entry"] == 2 and rt["H"] == H, (what, rt)
            jac = name != "plain_tape" and D <= 14
            assert rt["tape"] == (2 if jac else 1), (what, rt)
            if name == "default":
                assert rt["tape"] == (2 if case["grad"] == "jac" else 1), (what, rt)
                assert rt["chain"] == (1 if case["chain"] == "device" else 2), (what, rt)
                if case["chain"] == "device":
                    assert (rt["rev_lds"] > 65536) == (case["rev"] == "above"), (what, rt)
            else:
                assert rt["chain"] == 2, (what, rt)
            if jac:
                assert rt["pair"] in (4, 5), (what, rt)
            errs = [abs(g[0] - R) / abs(R)] + [wr.block_error(np.asarray(x).reshape(np.shape(y)), y) for x, y in zip(g[1:], G)]
            assert max(errs) <= dc.TOL_GRAD, "%s: reward / gradient blocks %s (tol %.0e)" % (what, ["%.2e" % e for e in errs], dc.TOL_GRAD)
            assert abs(g[0] - r_ref) <= dc.TOL_FWD * abs(r_ref), what
    finally:
        cx.close()


_LANE_CASES = [c for c in dc.CASES if c.get("lanes")]


@pytest.mark.parametrize("case", _LANE_CASES, ids=[c["name"] for c in _LANE_CASES])
def test_batch_lanes_are_bit_identical_to_their_solo_calls(case):
    d, _ = _ref(case)
    cx = _context(case, d)
    E, U, H = case["E"], case["U"], case["H"]
    try:
        rw = _rewards(case, d)
        rs = np.random.RandomState(11)
        pols = [_policy(case, d, **({} if U == 0 else dict(W=d["W"] + 0.05 * rs.randn(U, E), b=d["b"] + 0.05 * rs.randn(U)))) for _ in range(3)]
        m0 = np.stack([d["m0"].ravel() + 0.02 * i for i in range(3)])
        S0 = np.stack([d["S0"] * (1.0 + 0.1 * i) for i in range(3)])
        solo = [cx.rollout(pols[i], rw, m0[i], S0[i], H) for i in range(3)]
        mH, SH, rew = cx.rollout_batch(pols, rw, m0, S0, H)
        for i in range(3):
            assert np.array_equal(mH[i], solo[i][0].ravel()) and np.array_equal(SH[i], solo[i][1]) and rew[i] == solo[i][2][0, 0], i
        if U == 0:
            return
        gsolo = [cx.rollout_grad(pols[i], rw, m0[i], S0[i], H) for i in range(2)]
        r, dW, db = cx.rollout_grad_batch(pols[:2], rw, m0[:2], S0[:2], H)
        for i in range(2):
            assert r[i] == gsolo[i][0] and np.array_equal(dW[i], gsolo[i][1].reshape(U, E)) and np.array_equal(db[i], gsolo[i][2].reshape(U)), i
    finally:
        cx.close()
