"""The step's serial link (controller, squash_sin, joint Gaussian, reward) at its edge inputs (cases: helpers/link_cases.py)
against the 50-digit truth in tests/golden/link_edges.npz (oracle/mp_link.py; docs/link_edges.md).

Per case, on a context of its own:
- stages: policy_action and reward_eval at (m0, S0): |device - truth| <= K unit per block, K capped at 8 x the float64
  restatement's own K of the block's class (helpers/link_reference.caps); a block the case declares exactly 0 within 2^-1022 K.
- rollouts on every route of test_gpu_rollout_widths._forward_routes: trajectory and reward against the truth (TOL_FWD),
  pilco_debug_last_route, bitwise repeatable, the routes against each other (bitwise where _bitwise_pair says so, else
  TOL_ROUTES); the action moments INSIDE the rollout from rollout_tape's joint Gaussian, fused head and three-kernel step:
  step 0 with the stage's K unit, later steps normwise.
- gradients: Jacobian tape, host chain, plain tape against the fixture's 50-digit gradient (grad = "mp") or torch autograd
  ("ag"), the chains against each other to TOL_ROUTES; the entry points refuse squash=False.
- lanes: rollout_batch (B = 3) / rollout_grad_batch (B = 2) with edge inputs that differ per lane, bitwise equal to solo calls.
- refusals: 5 reward terms, a policy_action shape whose link does not fit the LDS -- PilcoError, then one good call."""
import numpy as np
import pytest

from helpers import link_cases as lc
from helpers import link_reference as lr
from helpers import widths_reference as wr
from test_gpu_rollout_widths import _bitwise_pair, _expected_forward, _forward_routes, _settings

pytestmark = pytest.mark.gpu

_DATA = {}


def _data(c):
    if c["name"] not in _DATA:
        _DATA[c["name"]] = (lc.make_data(c), lr.fixture(c))
    return _DATA[c["name"]]


def _context(c, d):
    from pilco_amd import _lib
    cx = _lib.Context()
    if not c["stage"]:
        cx.gp_set_data(0, d["X"], d["Y"])
        cx.gp_set_hyp(0, d["ls"], d["var"], d["noise"])
        cx.gp_factorize(0)
    if c["policy"] == "rbf":
        U = c["U"]
        cx.gp_set_data(_lib.SLOT_POLICY, d["cX"], d["cY"])
        cx.gp_set_hyp(_lib.SLOT_POLICY, d["cl"], np.ones(U), 1e-4 * np.ones(U))
        cx.gp_factorize(_lib.SLOT_POLICY)
    return cx


def _policy(c, d, squash=None, **over):
    from pilco_amd import _lib
    E, U = c["E"], c["U"]
    sq = c["squash"] if squash is None else squash
    if c["policy"] == "linear":
        return dict(kind=_lib.POLICY_LINEAR, state_dim=E, control_dim=U, W=over.get("W", d["W"]), b=over.get("b", d["b"]), max_action=d["maxact"], squash=sq)
    if c["policy"] == "rbf":
        return dict(kind=_lib.POLICY_RBF, state_dim=E, control_dim=U, max_action=d["maxact"], squash=sq)
    return dict(kind=_lib.POLICY_NONE, state_dim=E, control_dim=0)


def _rewards(d):
    from pilco_amd import _lib
    return [dict(kind=_lib.REWARD_EXPONENTIAL, coef=t["coef"], W=t["W"], t=t["t"]) if t["kind"] == "exp" else
            dict(kind=_lib.REWARD_LINEAR, coef=t["coef"], W=t["W"]) for t in d["rewards"]]


def _lib_kind(kind):
    from pilco_amd import _lib
    return _lib.REWARD_EXPONENTIAL if kind == "exp" else _lib.REWARD_LINEAR


def _assert_k(c, ks, what):
    for b, k in ks.items():
        cap = lr.cap_of(c, b)
        print("K %-22s %-12s %-5s %10.3g  (cap %.3g)" % (c["name"], what, b, k, cap))
    bad = {b: (k, lr.cap_of(c, b)) for b, k in ks.items() if not k <= lr.cap_of(c, b)}
    assert not bad, "%s / %s: K over its cap: %s" % (c["name"], what, bad)


# ------------------------------------------------------------------ stages
@pytest.mark.parametrize("c", lc.CASES, ids=lc.case_ids())
def test_stages_vs_truth(c):
    d, fx = _data(c)
    cx = _context(c, d)
    try:
        vals = {}
        if c["U"] > 0:
            M, S, V = cx.policy_action(_policy(c, d), d["m0"], d["S0"])
            M2, S2, V2 = cx.policy_action(_policy(c, d), d["m0"], d["S0"])
            assert np.array_equal(M, M2) and np.array_equal(S, S2) and np.array_equal(V, V2), c["name"]
            vals.update(M=M.ravel(), S=S, V=V)
        if d["rewards"]:
            mu, var = cx.reward_eval(_rewards(d), c["E"], d["m0"], d["S0"])
            vals.update(rmu=mu[0, 0], rvar=var[0, 0])
            if len(d["rewards"]) == 4:   # each term alone: the staging offsets of a 1-term call
                for i, tm in enumerate(_rewards(d)):
                    m1, v1 = cx.reward_eval([dict(tm, coef=1.0)], c["E"], d["m0"], d["S0"])
                    row = fx["rw"][i]   # the term's own truth: [mean, variance, q, r2], with the units and caps of the other blocks
                    if tm["kind"] == _lib_kind("exp"):
                        um, uv = lc.unit_reward_mean(row[0], row[2]), lc.unit_reward_var(row[0], row[3], row[2])
                    else:
                        w = np.asarray(tm["W"], np.float64)
                        um = lc.EPS * float(np.abs(np.ravel(d["m0"]) * w).sum())
                        uv = lc.EPS * float(np.abs(w[:, None] * d["S0"] * w[None, :]).sum())
                    _assert_k(c, dict(rmu=lr.k_of(m1[0, 0], row[0], um), rvar=lr.k_of(v1[0, 0], row[1], uv)), "term %d" % i)
        assert all(np.all(np.isfinite(np.asarray(v))) for v in vals.values()), (c["name"], "NaN / inf in a stage")
        _assert_k(c, lr.stage_k(c, d, fx, vals), "stage")
    finally:
        cx.close()


def test_refused_calls_leave_the_context_usable():
    from pilco_amd import _lib
    c = lc.by_name("e3u1_std")
    d, fx = _data(c)
    cx = _context(c, d)
    try:
        pol, rw = _policy(c, d), _rewards(d)
        good = cx.rollout(pol, rw, d["m0"], d["S0"], c["H"])
        five = [dict(rw[0], coef=0.2)] * 5
        with pytest.raises(_lib.PilcoError):
            cx.reward_eval(five, c["E"], d["m0"], d["S0"])
        mu, _ = cx.reward_eval(rw, c["E"], d["m0"], d["S0"])
        assert abs(mu[0, 0] - fx["rw"][-1, 0]) <= 1e-12 * abs(fx["rw"][-1, 0])
        with pytest.raises(_lib.PilcoError):
            cx.rollout(pol, five, d["m0"], d["S0"], c["H"])
        again = cx.rollout(pol, rw, d["m0"], d["S0"], c["H"])
        assert all(np.array_equal(x, y) for x, y in zip(good, again))
        # every gradient entry point refuses squash=False
        nosq = _policy(c, d, squash=False)
        with pytest.raises(_lib.PilcoError):
            cx.rollout_grad(nosq, rw, d["m0"], d["S0"], c["H"])
        with pytest.raises(_lib.PilcoError):
            cx.rollout_grad_batch([nosq, nosq], rw, np.stack([d["m0"].ravel()] * 2), np.stack([d["S0"]] * 2), c["H"])
        g = cx.rollout_grad(pol, rw, d["m0"], d["S0"], c["H"])
        assert abs(g[0] - fx["rew"][-1]) <= lc.TOL_FWD * abs(fx["rew"][-1])
        # policy_action with 32 < E + U <= 64: supported where the link's buffers fit the LDS (st_e20u20, st_e32u8 above),
        # refused before any launch where they do not
        for E, U in ((32, 32), (32, 24), (24, 32)):
            assert not lc.policy_action_fits(E, U)
            with pytest.raises(_lib.PilcoError) as ei:
                cx.policy_action(dict(kind=_lib.POLICY_LINEAR, state_dim=E, control_dim=U, W=np.zeros((U, E)), b=np.zeros(U), squash=True),
                                 np.zeros(E), np.eye(E))
            assert "PILCO_E_SHAPE" in str(ei.value) or getattr(ei.value, "code", None) == 1, str(ei.value)
        M, S, V = cx.policy_action(pol, d["m0"], d["S0"])
        assert lr.k_of(M.ravel(), fx["pa"][:1], lc.unit_squash_mean(lr.maxact_vec(c, d), fx["pre"])) <= lr.cap_of(c, "M")
    finally:
        cx.close()


def test_rbf_entry_points_refuse_too():
    """rollout_grad_rbf refuses squash=False; policy_action's RbfController branch has an LDS check of its own."""
    from pilco_amd import _lib
    c = lc.by_name("rbf_std")
    d, fx = _data(c)
    cx = _context(c, d)
    try:
        pol, rw, U = _policy(c, d), _rewards(d), c["U"]
        call = lambda p: cx.rollout_grad_rbf(p, rw, d["m0"], d["S0"], c["H"], d["cX"], d["cY"], d["cl"], 1e-4 * np.ones(U))
        with pytest.raises(_lib.PilcoError):
            call(_policy(c, d, squash=False))
        g = call(pol)
        assert abs(g[0] - fx["rew"][-1]) <= lr.fwd_tol(c, d, fx) * abs(fx["rew"][-1])
        # a policy GP from 32 states to 32 controls: D = 64, 275 KB of LDS for the link
        rs = np.random.RandomState(3)
        cx.gp_set_data(_lib.SLOT_POLICY, rs.randn(4, 32), 0.3 * rs.randn(4, 32))
        cx.gp_set_hyp(_lib.SLOT_POLICY, 6.0 * np.ones((32, 32)), np.ones(32), 1e-4 * np.ones(32))
        cx.gp_factorize(_lib.SLOT_POLICY)
        with pytest.raises(_lib.PilcoError) as ei:
            cx.policy_action(dict(kind=_lib.POLICY_RBF, state_dim=32, control_dim=32, squash=True), np.zeros(32), 0.04 * np.eye(32))
        assert "PILCO_E_SHAPE" in str(ei.value) or getattr(ei.value, "code", None) == 1, str(ei.value)
        # ... and the context goes on: the case's own controller again
        cx.gp_set_data(_lib.SLOT_POLICY, d["cX"], d["cY"])
        cx.gp_set_hyp(_lib.SLOT_POLICY, d["cl"], np.ones(U), 1e-4 * np.ones(U))
        cx.gp_factorize(_lib.SLOT_POLICY)
        M, S, V = cx.policy_action(pol, d["m0"], d["S0"])
        _assert_k(c, lr.stage_k(c, d, fx, dict(M=M.ravel(), S=S, V=V)), "after the refusal")
    finally:
        cx.close()


# ------------------------------------------------------------------ rollouts
_ROLL = [c for c in lc.CASES if not c["stage"]]


def _check_actions(c, d, fx, tape, what):
    """The action moments inside the rollout (the tape's joint Gaussian) against the truth's."""
    if c["U"] == 0:
        return
    e, pre = lr.maxact_vec(c, d), fx["pre"]
    for t in range(c["H"]):
        M, S, C = lr.tape_action(c, tape[t])
        Mt, St, Ct = lr.act_blocks(c, fx["act"][t])
        assert np.all(np.isfinite(M)) and np.all(np.isfinite(S)) and np.all(np.isfinite(C)), (what, t)
        if t == 0:
            blocks = lr.stage_blocks(c, d, fx)
            ks = dict(M=lr.k_of(M, *blocks["M"][:2], "M" in c["exact0"]), S=lr.k_of(S, *blocks["S"][:2], "S" in c["exact0"]))
            # s V C: the cross block, per control normwise in its column of the truth
            ks["V"] = lr.k_of(C, Ct, lc.unit_cross(Ct, pre) if c["squash"] else lc.EPS * max(np.abs(Ct).max(), lc.TINY), "C" in c["exact0"])
            _assert_k(c, ks, what + " step 0")
        else:
            # later steps: the device's own state went in (TOL_FWD from the truth's), so normwise -- on the scale the units
            # use, e_u (e_u e_v for the covariance): a squashed action's error is not relative to a small S_uv
            for a, b, nm in ((M, Mt, "M"), (S, St, "S"), (C, Ct, "C")):
                scale = max(np.abs(b).max(), np.abs(e).max() ** (2 if nm == "S" else 1) if c["squash"] else 0.0, 1e-300)
                assert np.abs(a - b).max() <= lr.fwd_tol(c, d, fx) * scale, (what, t, nm, np.abs(a - b).max(), scale)


@pytest.mark.parametrize("c", _ROLL, ids=lc.case_ids(_ROLL))
def test_rollout_routes_vs_truth_and_each_other(c):
    d, fx = _data(c)
    cd = dict(c, **lc.declared_routes(c))
    cx = _context(c, d)
    E, H = c["E"], c["H"]
    r_ref = fx["rew"][-1]
    try:
        pol, rw = _policy(c, d), _rewards(d)
        runs = {}
        for name, kw in _forward_routes(c):
            _settings(cx, **kw)
            a = cx.rollout(pol, rw, d["m0"], d["S0"], H, want_traj=True)
            rt = cx.last_route()
            b = cx.rollout(pol, rw, d["m0"], d["S0"], H, want_traj=True)
            assert cx.last_route() == rt, name
            for x, y in zip(a, b):
                assert np.array_equal(x, y), "%s / %s: not bitwise repeatable" % (c["name"], name)
            assert np.all(np.isfinite(a[3])) and np.isfinite(a[2][0, 0]), (c["name"], name, "NaN / inf")
            assert np.array_equal(a[0].ravel(), a[3][H, :E]) and np.array_equal(a[1].ravel(), a[3][H, E:]), (c["name"], name)
            _expected_forward(cd, name, rt)
            err = wr.normwise_error(a[3], fx["traj"], E)
            if "rew" in c["exact0"]:
                rerr = 0.0 if abs(a[2][0, 0]) <= 4 * lc.TINY else float("inf")
            else:
                rerr = abs(a[2][0, 0] - r_ref) / max(abs(r_ref), 1e-300)
            print("R %-22s %-16s states %.2e reward %.2e" % (c["name"], name, err, rerr))
            tol = lr.fwd_tol(c, d, fx)
            assert err <= tol and rerr <= tol, "%s / %s: states %.2e, reward %.2e (tol %.1e)" % (c["name"], name, err, rerr, tol)
            runs[name] = (a, rt)
        names = list(runs)
        for i, na in enumerate(names):
            for nb in names[i + 1:]:
                (a, ra), (b, rb) = runs[na], runs[nb]
                if _bitwise_pair(ra, rb):
                    assert np.array_equal(a[3], b[3]) and np.array_equal(a[2], b[2]), "%s: %s vs %s not bitwise" % (c["name"], na, nb)
                else:
                    # (TOL_ROUTES; where the restatement itself cannot hold TOL_FWD -- lr.fwd_tol -- two correct float64
                    # evaluations of the controller need not agree better than that either)
                    rtol = lc.TOL_ROUTES if lr.fwd_tol(c, d, fx) == lc.TOL_FWD else lr.fwd_tol(c, d, fx)
                    err = wr.normwise_error(a[3], b[3], E)
                    print("X %-22s %-16s %-16s %.2e" % (c["name"], na, nb, err))
                    assert err <= rtol, "%s: %s vs %s %.2e" % (c["name"], na, nb, err)
                    assert abs(a[2][0, 0] - b[2][0, 0]) <= rtol * abs(b[2][0, 0]), (c["name"], na, nb)
        # the action moments inside the rollout: fused head (or one-launch step) and k_glue of the three-kernel step
        tapes, steps, pols_ = [], [], []
        for name, kw in (("default", {}), ("three", dict(fused=0))):
            _settings(cx, **kw)
            tp_ = cx.rollout_tape(pol, rw, d["m0"], d["S0"], H)
            steps.append(cx.last_route()["step"])
            pols_.append(cx.last_route()["policy"])
            assert wr.normwise_error(tp_[3], fx["traj"], E) <= lr.fwd_tol(c, d, fx), (c["name"], name, "tape trajectory")
            _check_actions(c, d, fx, tp_[4], "tape/" + name)
            tapes.append(tp_[4])
        D = c["D"]
        # the link's two hosts run the same code: the joint Gaussians agree to the bit -- all of them where the pair sums do
        # (fused head against three-kernel step), the first one where the one-launch step sums its pairs in another order
        # (an RbfController evaluated inline and by its own launches is two codes: nothing to compare then)
        n = 0 if pols_[0] != pols_[1] else H if 2 not in steps else 1
        assert np.array_equal(tapes[0][:n, :D + D * D], tapes[1][:n, :D + D * D]), (c["name"], steps, "joint Gaussians of the link's two hosts differ")
    finally:
        cx.close()


# ------------------------------------------------------------------ gradients
_GRAD = [c for c in _ROLL if c["grad"]]


@pytest.mark.parametrize("c", _GRAD, ids=lc.case_ids(_GRAD))
def test_policy_gradients(c):
    d, fx = _data(c)
    if c["grad"] == "mp":
        R, G = fx["rew"][-1], [fx["g%d" % i] for i in range(3 if c["policy"] == "rbf" else 2)]
    else:
        R, G = lr.torch_gradient(c, d)
    cx = _context(c, d)
    H, U = c["H"], c["U"]
    try:
        pol, rw = _policy(c, d), _rewards(d)
        got = {}
        for name, kw in (("default", {}), ("host_chain", dict(dev_chain=0)), ("plain_tape", dict(grad_mode=0))):
            _settings(cx, **kw)
            if c["policy"] == "rbf":
                call = lambda: cx.rollout_grad_rbf(pol, rw, d["m0"], d["S0"], H, d["cX"], d["cY"], d["cl"], 1e-4 * np.ones(U))
            else:
                call = lambda: cx.rollout_grad(pol, rw, d["m0"], d["S0"], H)
            g = call()
            rt = cx.last_route()
            g2 = call()
            assert g[0] == g2[0] and all(np.array_equal(x, y) for x, y in zip(g[1:], g2[1:])), (c["name"], name, "not repeatable")
            assert rt["entry"] == 2 and rt["H"] == H, (name, rt)
            # the chain and the tape that ran are what the mirror declares (lc.declared_grad: csrc/rev.hip rev_chain_supported):
            # "device chain against host chain" below compares two chains only where the default call took the device one
            want = lc.declared_grad(c)
            if name == "default":
                assert rt["chain"] == want["chain"] and rt["tape"] == want["tape"], (c["name"], name, rt, want)
                if want["chain"] == 1:
                    assert rt["rev_lds"] > 0, (c["name"], rt)
            else:
                assert rt["chain"] == 2 and rt["tape"] == (want["tape"] if name == "host_chain" else 1), (c["name"], name, rt)
            assert all(np.all(np.isfinite(np.asarray(x))) for x in g[1:]) and np.isfinite(g[0]), (c["name"], name, "NaN / inf in a gradient")
            errs = [abs(g[0] - R) / max(abs(R), 1e-300)] + [wr.block_error(np.asarray(x).reshape(np.shape(y)), y) for x, y in zip(g[1:], G)]
            print("G %-22s %-10s chain %d tape %d  %s" % (c["name"], name, rt["chain"], rt["tape"], " ".join("%.2e" % e for e in errs)))
            assert max(errs) <= lc.TOL_GRAD, "%s / %s: reward / gradient blocks %s" % (c["name"], name, ["%.2e" % e for e in errs])
            got[name] = g
        for x, y in zip(got["default"][1:], got["host_chain"][1:]):
            assert wr.block_error(x, y) <= lc.TOL_ROUTES, (c["name"], "device chain vs host chain", wr.block_error(x, y))
    finally:
        cx.close()


# ------------------------------------------------------------------ lanes
_LANES = [c for c in _ROLL if c["lanes"]]


@pytest.mark.parametrize("c", _LANES, ids=lc.case_ids(_LANES))
def test_lanes_with_edge_inputs_that_differ_per_lane(c):
    d, _ = _data(c)
    cx = _context(c, d)
    E, U, H = c["E"], c["U"], c["H"]
    try:
        rw = _rewards(d)
        rs = np.random.RandomState(5)
        A = rs.randn(E, E)
        spd = np.eye(E) + A @ A.T / E
        S0 = np.stack([np.zeros((E, E)), 400.0 * spd, d["S0"]])
        m0 = np.stack([d["m0"].ravel(), d["m0"].ravel() + 0.1, np.zeros(E)])
        pols = [_policy(c, d, **({} if U == 0 else dict(W=d["W"] * s, b=d["b"] + o))) for s, o in ((1.0, 0.0), (0.0, 0.3), (1.5, 1e2))]
        solo = [cx.rollout(pols[i], rw, m0[i], S0[i], H) for i in range(3)]
        mH, SH, rew = cx.rollout_batch(pols, rw, m0, S0, H)
        for i in range(3):
            assert np.all(np.isfinite(mH[i])) and np.all(np.isfinite(SH[i])), i
            assert np.array_equal(mH[i], solo[i][0].ravel()) and np.array_equal(SH[i], solo[i][1]) and rew[i] == solo[i][2][0, 0], i
        if U == 0:
            return
        gsolo = [cx.rollout_grad(pols[i], rw, m0[i], S0[i], H) for i in range(2)]
        r, dW, db = cx.rollout_grad_batch(pols[:2], rw, m0[:2], S0[:2], H)
        for i in range(2):
            assert np.all(np.isfinite(dW[i])) and np.all(np.isfinite(db[i])), i
            assert r[i] == gsolo[i][0] and np.array_equal(dW[i], gsolo[i][1].reshape(U, E)) and np.array_equal(db[i], gsolo[i][2].reshape(U)), i
    finally:
        cx.close()
