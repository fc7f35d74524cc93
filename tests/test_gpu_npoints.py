"""Rollouts and policy gradients at every point-count edge (cases: helpers/npoints_cases.py), and one context reused across shapes.

Per case, on a context of its own:
- forward: rollout(want_traj=True) on every route the shape allows (default, no one-launch small step, three-kernel step, MFMA
  tiled pair kernel; for an RbfController inline off).  pilco_debug_last_route must name the declared step and npad, and
  pilco_debug_geometry the chunks, column splits and stream-K cut the mirror computes for this device's CU count and capacity.
  Every state and the reward against oracle.tf_path (TOL_FWD, normwise); same-code routes bitwise, the others to TOL_ROUTES;
  every route bitwise repeatable.
- gradient (U > 0, up to N = 1025): reward and every policy-gradient entry against torch autograd through oracle.torch_path
  (TOL_GRAD) for the default route (Jacobian tape where D <= 14), the host chain and the plain tape.
- lanes (a few cases): rollout_batch and rollout_grad_batch bit-identical to their solo calls.
Reused context: one context walked through sequences of shapes (growing data as the PILCO loop does, sparse and exact models
in the same slot, changes of E, U and the RBF basis, user factors, the pooled default context of the Python surface); at every
stage rollout, rollout_grad and rollout_batch must equal a fresh context's bitwise and the oracle to the tolerances above.
A PILCO_SK_WAVES override under which a wave would span three pairs must be refused for the computed cut."""
import gc
import os

import numpy as np
import pytest

from helpers import npoints_cases as nc
from helpers import widths_reference as wr

pytestmark = pytest.mark.gpu

STEP = {"fused": 1, "small": 2, "three": 3, "fused_rbf": 4}
_REF = {}
_MEASURED = {}   # case -> worst errors seen (written to $NPOINTS_REPORT as JSON when it is set: the source of docs/point_counts.md)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("NPOINTS_REPORT")
    if path:
        import json
        with open(path, "w") as f:
            json.dump(_MEASURED, f, indent=1, sort_keys=True)


def _note(name, key, value):
    ent = _MEASURED.setdefault(name, {})
    ent[key] = max(ent.get(key, 0.0), float(value))


def _ref(case):
    if case["name"] not in _REF:
        d = nc.make_data(case)
        _REF[case["name"]] = (d, wr.oracle_trajectory(case, d, zero_iK=case["factors"] == "user"))
    return _REF[case["name"]]


def _load(cx, case, d):
    """Put case's model (and RBF policy GP) into slots 0 / 1 of cx."""
    from pilco_amd import _lib
    cx.gp_set_data(0, d["X"], d["Y"])
    cx.gp_set_hyp(0, d["ls"], d["var"], d["noise"])
    cx.gp_set_inducing(0, d["Z"] if case["M"] else None)
    if case["factors"] == "user":
        _, beta = wr.factors(case, d)
        cx.gp_set_factors(0, None, beta)
    else:
        cx.gp_factorize(0)
    if case["policy"] == "rbf":
        U = case["U"]
        cx.gp_set_data(_lib.SLOT_POLICY, d["cX"], d["cY"])
        cx.gp_set_hyp(_lib.SLOT_POLICY, d["cl"], np.ones(U), 1e-4 * np.ones(U))
        cx.gp_factorize(_lib.SLOT_POLICY)


def _context(case, d):
    from pilco_amd import _lib
    cx = _lib.Context()
    _load(cx, case, d)
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


def _grad_call(cx, case, d, pol, rw):
    if case["policy"] == "rbf":
        return cx.rollout_grad_rbf(pol, rw, d["m0"], d["S0"], case["H"], d["cX"], d["cY"], d["cl"], 1e-4 * np.ones(case["U"]))
    return cx.rollout_grad(pol, rw, d["m0"], d["S0"], case["H"])


def _check_forward(case, ref, r_ref, traj, rew, what):
    err = wr.normwise_error(traj, ref, case["E"])
    rerr = abs(float(np.asarray(rew).ravel()[0]) - r_ref) / max(abs(r_ref), 1e-300)
    assert err <= nc.TOL_FWD and rerr <= nc.TOL_FWD, "%s: states %.2e, reward %.2e (tol %.0e)" % (what, err, rerr, nc.TOL_FWD)
    return max(err, rerr)


def _check_grad(g, R, G, what):
    errs = [abs(g[0] - R) / abs(R)] + [wr.block_error(np.asarray(x).reshape(np.shape(y)), y) for x, y in zip(g[1:], G)]
    assert max(errs) <= nc.TOL_GRAD, "%s: reward / gradient blocks %s (tol %.0e)" % (what, ["%.2e" % e for e in errs], nc.TOL_GRAD)
    return max(errs)


def _forward_routes(case):
    out = [("default", {}), ("no_small", dict(small=0)), ("three", dict(fused=0)), ("tiled", dict(variant=2))]
    if case["policy"] == "rbf":
        out += [("inline_off", dict(inline=0))]
    return out


def _expected_step(case, name):
    fwd = case["fwd"]
    if name == "default":
        return STEP[fwd]
    if name in ("no_small", "tiled"):
        return STEP["fused"] if fwd == "small" else STEP[fwd]
    if name == "inline_off":
        return STEP["fused_rbf"] if fwd != "three" else STEP["three"]
    return STEP["three"]


TOL_ROUTES_4160 = 6e-10   # npad = 4160 (n4097_fwd): default vs MFMA tiled measured 4.5e-10 on MI355X (docs/point_counts.md)


def _tol_routes(case):
    """Routes that sum in different orders: TOL_ROUTES (1e-10) up to npad = 1088, where the worst measured is about 1.5e-11; the one
    larger case, 17M exponent terms per pair sum, has its own bound chosen from its measurement (the routes are deterministic:
    bitwise repeatable on the same device)."""
    return nc.TOL_ROUTES if case["npad"] <= 1088 else TOL_ROUTES_4160


def _bitwise_pair(ra, rb):
    return {ra["step"], rb["step"]} <= {1, 3, 4} and ra["policy"] == rb["policy"] and ra["pair"] == rb["pair"]


def _check_geometry(case, geo):
    """pilco_debug_geometry after the default route against the mirror at this device's CU count and capacity."""
    g = nc.geometry(case, geo["cus"], geo["sk_capacity"])
    want = dict(npad=g["npad"], NCH=g["NCH"], NCHM=g["NCHM"], NT=g["NT"], sk_waves=g["sk_waves"], sk_total=g["sk_total"],
                sk_nd=g["sk_nd"], NCS_reward=g["NCS"])
    got = {k: geo[k] for k in want}
    _MEASURED.setdefault(case["name"], {})["geometry"] = dict(geo)
    assert got == want, "%s: geometry %s, mirror %s" % (case["name"], got, want)
    for k in nc.DECLARED:
        assert case.get(k, False) == g[k], "%s: declared %s=%r, on this device %r" % (case["name"], k, case.get(k), g[k])


@pytest.mark.parametrize("case", nc.CASES, ids=nc.case_ids())
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
            if name == "default":
                _check_geometry(case, cx.geometry())
            b = cx.rollout(pol, rw, d["m0"], d["S0"], case["H"], want_traj=True)
            assert cx.last_route() == rt, name
            for x, y in zip(a, b):
                assert np.array_equal(x, y), "%s / %s: not bitwise repeatable" % (case["name"], name)
            assert rt["step"] == _expected_step(case, name) and rt["npad"] == case["npad"] and rt["H"] == case["H"], (case["name"], name, rt)
            _note(case["name"], "fwd", _check_forward(case, ref, r_ref, a[3], a[2], "%s / %s" % (case["name"], name)))
            runs[name] = (a, rt)
        names = list(runs)
        for i, na in enumerate(names):
            for nb in names[i + 1:]:
                (a, ra), (b, rb) = runs[na], runs[nb]
                if _bitwise_pair(ra, rb):
                    assert np.array_equal(a[3], b[3]) and np.array_equal(a[2], b[2]), "%s: %s vs %s not bitwise" % (case["name"], na, nb)
                    _note(case["name"], "bitwise_pairs", _MEASURED[case["name"]].get("bitwise_pairs", 0) + 1)
                else:
                    err = wr.normwise_error(a[3], b[3], case["E"])
                    rerr = abs(a[2][0, 0] - b[2][0, 0]) / abs(b[2][0, 0])
                    _note(case["name"], "routes", max(err, rerr))
                    assert err <= _tol_routes(case), "%s: %s vs %s states %.2e" % (case["name"], na, nb, err)
                    assert rerr <= _tol_routes(case), "%s: %s vs %s reward %.2e" % (case["name"], na, nb, rerr)
    finally:
        cx.close()


_GRAD_CASES = [c for c in nc.CASES if c["grad"]]


@pytest.mark.parametrize("case", _GRAD_CASES, ids=[c["name"] for c in _GRAD_CASES])
def test_policy_gradients_vs_autograd(case):
    d, (ref, r_ref) = _ref(case)
    R, G = wr.torch_gradient(case, d, zero_iK=case["factors"] == "user")
    cx = _context(case, d)
    try:
        pol, rw = _policy(case, d), _rewards(case, d)
        D = case["D"]
        for name, kw in [("default", {}), ("host_chain", dict(dev_chain=0)), ("plain_tape", dict(grad_mode=0))]:
            _settings(cx, **kw)
            g = _grad_call(cx, case, d, pol, rw)
            rt = cx.last_route()
            g2 = _grad_call(cx, case, d, pol, rw)
            what = "%s / %s" % (case["name"], name)
            assert g[0] == g2[0] and all(np.array_equal(x, y) for x, y in zip(g[1:], g2[1:])), (what, "not repeatable")
            assert rt["entry"] == 2 and rt["npad"] == case["npad"], (what, rt)
            jac = name != "plain_tape" and D <= 14
            assert rt["tape"] == (2 if jac else 1), (what, rt)
            if jac:
                assert rt["pair"] == (5 if case["jsmall"] else 4), (what, rt)
            _note(case["name"], "grad", _check_grad(g, R, G, what))
            assert abs(g[0] - r_ref) <= nc.TOL_FWD * abs(r_ref), what
    finally:
        cx.close()


def test_jacobian_tape_where_the_record_kernel_asks_for_more_than_64_kb():
    """E = 1, U = 1 (D = 2), N = 6600 (npad = 6656), H = 2: the smallest shape at which k_mm_jac_rec's dynamic LDS -- 6 x 256 +
    (1 + D + D^2) + 3 D^2 + D + 2 + 1 + npad doubles, 65 728 bytes -- is above the 64 KB a launch gets without opting in (the
    sweep is at 80 KB there).  Value and gradient on the Jacobian tape against the plain tape of the same context at TOL_GRAD,
    the bound both routes are held to against autograd at the sizes where autograd can be run."""
    assert 8 * (6 * 256 + (1 + 2 + 4) + 3 * 4 + 2 + 2 + 1 + 6656) == 65728 > 65536 >= 8 * (6 * 256 + 7 + 12 + 4 + 1 + 6592)
    case = nc._c("n6600_rec64k", 6600, 1, 1, H=2)
    d = nc.make_data(case)
    cx = _context(case, d)
    try:
        pol, rw = _policy(case, d), _rewards(case, d)
        _settings(cx)
        g = _grad_call(cx, case, d, pol, rw)
        rt = cx.last_route()
        assert rt["entry"] == 2 and rt["tape"] == 2 and rt["pair"] == 4 and rt["npad"] == 6656 and rt["H"] == 2, rt
        _settings(cx, grad_mode=0)
        p = _grad_call(cx, case, d, pol, rw)
        rp = cx.last_route()
        assert rp["entry"] == 2 and rp["tape"] == 1 and rp["npad"] == 6656, rp
        for x in list(g) + list(p):
            assert np.all(np.isfinite(np.asarray(x, dtype=np.float64))), "non-finite result"
        errs = [abs(g[0] - p[0]) / abs(p[0])] + [wr.block_error(np.asarray(x).reshape(np.shape(y)), np.asarray(y)) for x, y in zip(g[1:], p[1:])]
        print("n6600_rec64k: Jacobian tape vs plain tape, reward / gradient blocks %s" % ["%.2e" % e for e in errs])
        _note(case["name"], "jac_vs_plain", max(errs))
        assert max(errs) <= nc.TOL_GRAD, "reward / gradient blocks %s (tol %.0e)" % (["%.2e" % e for e in errs], nc.TOL_GRAD)
    finally:
        cx.close()


def test_jacobian_tape_where_the_sweep_needs_a_further_column_split():
    """E = 10, U = 1 (D = 11, 55 pairs), N = 4200 (npad = 4224), H = 2: mm_bwd_geometry leaves the columns whole (33 row blocks x
    55 pairs >= 1536), and this is the smallest npad at which the sweep's workgroup with one split -- 8 (4 x 4224 + 2 x 1216 +
    1152) = 163 840 dynamic bytes and the 2 048 of its exp table -- is above the 163 840 a workgroup can have; mm_bwd_split runs
    it with two.  The Jacobian tape against the plain tape at TOL_GRAD as above; both take their value from the sweep, so the
    reward is also held to the forward rollout's (the pair kernel's sums): each is held to the oracle at TOL_FWD where the oracle
    can be run, hence 2 TOL_FWD between them."""
    assert 8 * (4 * 4224 + 2 * 1216 + 1152) + 2048 > 160 * 1024 >= 8 * (4 * 4160 + 2 * 1216 + 1152) + 2048 and nc.bwd_geometry(4224, 55) == (1, 33)
    case = nc._c("n4200_split", 4200, 10, 1, H=2)
    d = nc.make_data(case)
    cx = _context(case, d)
    try:
        pol, rw = _policy(case, d), _rewards(case, d)
        _settings(cx)
        fwd = cx.rollout(pol, rw, d["m0"], d["S0"], case["H"])
        r_fwd = float(np.asarray(fwd[2]).ravel()[0])
        g = _grad_call(cx, case, d, pol, rw)
        rt = cx.last_route()
        assert rt["entry"] == 2 and rt["tape"] == 2 and rt["pair"] == 4 and rt["npad"] == 4224, rt
        _settings(cx, grad_mode=0)
        p = _grad_call(cx, case, d, pol, rw)
        assert cx.last_route()["tape"] == 1
        for x in list(g) + list(p):
            assert np.all(np.isfinite(np.asarray(x, dtype=np.float64))), "non-finite result"
        errs = [abs(g[0] - p[0]) / abs(p[0])] + [wr.block_error(np.asarray(x).reshape(np.shape(y)), np.asarray(y)) for x, y in zip(g[1:], p[1:])]
        rerr = max(abs(g[0] - r_fwd), abs(p[0] - r_fwd)) / abs(r_fwd)
        print("n4200_split: Jacobian tape vs plain tape %s, reward vs the forward rollout %.2e" % (["%.2e" % e for e in errs], rerr))
        _note(case["name"], "jac_vs_plain", max(errs))
        assert max(errs) <= nc.TOL_GRAD, "reward / gradient blocks %s (tol %.0e)" % (["%.2e" % e for e in errs], nc.TOL_GRAD)
        assert rerr <= 2 * nc.TOL_FWD, "reward against the forward rollout %.2e" % rerr
    finally:
        cx.close()


_LANE_CASES = [c for c in nc.CASES if c["lanes"]]


def _batch_inputs(case, d, B):
    E, U = case["E"], case["U"]
    rs = np.random.RandomState(11)
    pols = [_policy(case, d, **({} if U == 0 or case["policy"] != "linear" else
                                dict(W=d["W"] + 0.05 * rs.randn(U, E), b=d["b"] + 0.05 * rs.randn(U)))) for _ in range(B)]
    m0 = np.stack([d["m0"].ravel() + 0.02 * i for i in range(B)])
    S0 = np.stack([d["S0"] * (1.0 + 0.1 * i) for i in range(B)])
    return pols, m0, S0


@pytest.mark.parametrize("case", _LANE_CASES, ids=[c["name"] for c in _LANE_CASES])
def test_batch_lanes_are_bit_identical_to_their_solo_calls(case):
    d, _ = _ref(case)
    cx = _context(case, d)
    E, U, H = case["E"], case["U"], case["H"]
    try:
        rw = _rewards(case, d)
        pols, m0, S0 = _batch_inputs(case, d, 3)
        solo = [cx.rollout(pols[i], rw, m0[i], S0[i], H) for i in range(3)]
        mH, SH, rew = cx.rollout_batch(pols, rw, m0, S0, H)
        for i in range(3):
            assert np.array_equal(mH[i], solo[i][0].ravel()) and np.array_equal(SH[i], solo[i][1]) and rew[i] == solo[i][2][0, 0], i
        gsolo = [cx.rollout_grad(pols[i], rw, m0[i], S0[i], H) for i in range(2)]
        r, dW, db = cx.rollout_grad_batch(pols[:2], rw, m0[:2], S0[:2], H)
        for i in range(2):
            assert r[i] == gsolo[i][0] and np.array_equal(dW[i], gsolo[i][1].reshape(U, E)) and np.array_equal(db[i], gsolo[i][2].reshape(U)), i
    finally:
        cx.close()


# ---- one context reused across shapes ---------------------------------------------------------------------------------------

def _stage(name, N, E, U, M=0, policy="linear", bf=0, factors="device", reward="comb", H=3, data_of=None):
    c = dict(name=data_of or name, N=N, E=E, U=U, D=E + U, policy=policy, bf=bf, reward=reward, M=M, H=H, factors=factors)
    return name, c


def _run_stage(cx, case, d):
    """rollout (with trajectory), value-and-gradient and a two-lane rollout_batch of case on cx (default settings)."""
    _settings(cx)
    pol, rw = _policy(case, d), _rewards(case, d)
    fwd = cx.rollout(pol, rw, d["m0"], d["S0"], case["H"], want_traj=True)
    route = cx.last_route()
    grad = _grad_call(cx, case, d, pol, rw) if case["U"] > 0 else None
    batch = None
    if case["policy"] != "rbf":   # (rollout_batch has no RbfController lanes: one policy GP slot per context)
        pols, m0, S0 = _batch_inputs(case, d, 2)
        batch = cx.rollout_batch(pols, rw, m0, S0, case["H"])
    return fwd, route, grad, batch


def _same(a, b):
    if a is None or b is None:
        return a is b
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return a == b
    return np.array_equal(np.asarray(a), np.asarray(b))


def _walk(seq_name, stages):
    from pilco_amd import _lib
    cx = _lib.Context()
    try:
        for stage, case in stages:
            what = "sequence %s, stage %s" % (seq_name, stage)
            d = nc.make_data(case)
            try:
                _load(cx, case, d)
                fwd, route, grad, batch = _run_stage(cx, case, d)
            except Exception as e:   # (a stale launch sequence can also end in an error: name where)
                raise AssertionError("%s: the reused context failed: %s" % (what, e)) from e
            fresh = _lib.Context()
            try:
                _load(fresh, case, d)
                f_fwd, f_route, f_grad, f_batch = _run_stage(fresh, case, d)
            finally:
                fresh.close()
            assert route == f_route, "%s: route %s, a fresh context %s" % (what, route, f_route)
            assert _same(fwd, f_fwd), "%s: rollout differs from a fresh context's" % what
            assert _same(grad, f_grad), "%s: rollout_grad differs from a fresh context's" % what
            assert _same(batch, f_batch), "%s: rollout_batch differs from a fresh context's" % what
            ref, r_ref = wr.oracle_trajectory(case, d, zero_iK=case["factors"] == "user")
            _note("seq " + seq_name, "fwd", _check_forward(case, ref, r_ref, fwd[3], fwd[2], what))
            if grad is not None and (case["M"] or case["N"]) <= 1100:
                R, G = wr.torch_gradient(case, d, zero_iK=case["factors"] == "user")
                _note("seq " + seq_name, "grad", _check_grad(grad, R, G, what))
    finally:
        cx.close()


SEQUENCES = {
    "growing data": [_stage("N=%d" % n, n, 2, 1, data_of="grow%d" % n) for n in (40, 64, 65, 128, 129, 192, 256, 257, 320, 513, 1000, 1025, 130)],
    "sparse and exact, M = 200": [_stage("SMGPR M=200 N=5000", 5000, 3, 5, M=200, data_of="sx5000"),
                                  _stage("MGPR N=200", 200, 3, 5, data_of="sx200"),
                                  _stage("SMGPR M=200 other Z", 5000, 3, 5, M=200, data_of="sx5000b")],
    "sparse and exact, M = N = 64": [_stage("SMGPR M=64 N=64", 64, 3, 1, M=64, data_of="sq64"),
                                     _stage("MGPR N=64", 64, 3, 1, data_of="sq64"),
                                     _stage("SMGPR M=64 other Z", 64, 3, 1, M=64, data_of="sq64b")],
    "E and U": [_stage("E=3 U=1", 100, 3, 1, data_of="eu31"), _stage("E=2 U=2", 100, 2, 2, data_of="eu22"),
                _stage("E=3 U=2", 100, 3, 2, data_of="eu32"), _stage("E=3 U=1 (same KP, P, NCH, NCHM)", 100, 3, 1, data_of="eu31b"),
                _stage("E=4 U=1", 100, 4, 1, data_of="eu41")],
    "RBF basis": [_stage("bf=10", 120, 3, 1, policy="rbf", bf=10, data_of="rbf10"), _stage("bf=6", 120, 3, 1, policy="rbf", bf=6, data_of="rbf6"),
                  _stage("bf=12", 120, 3, 1, policy="rbf", bf=12, data_of="rbf12")],
    "user factors": [_stage("user factors, iK None", 150, 3, 1, factors="user", data_of="uf150"),
                     _stage("device factorisation", 150, 3, 1, data_of="uf150"),
                     _stage("user factors again", 150, 3, 1, factors="user", data_of="uf150b")],
}


@pytest.mark.parametrize("seq", list(SEQUENCES), ids=[s.replace(" ", "_").replace(",", "").replace("=", "") for s in SEQUENCES])
def test_reused_context_equals_a_fresh_one(seq):
    _walk(seq, SEQUENCES[seq])


def _pilco_objects(d, sparse, seed):
    from pilco_amd.models import PILCO
    np.random.seed(seed)
    p = PILCO((d["X"], d["Y"]), num_induced_points=d["X"].shape[0] if sparse else None, horizon=3,
              m_init=d["m0"], S_init=d["S0"])
    for i, mdl in enumerate(p.mgpr.models):
        mdl.kernel.lengthscales.assign(d["ls"][i])
        mdl.kernel.variance.assign(d["var"][i])
        mdl.likelihood.variance.assign(d["noise"][i])
    p.controller.W.assign(d["W"])
    p.controller.b.assign(d["b"])
    p.controller.max_action = d["maxact"]
    return p


def test_pooled_default_context_after_a_sparse_pilco():
    from pilco_amd import _lib
    old = _lib._default_ctx
    case = dict(name="pool64", N=64, E=2, U=1, D=3, policy="linear", bf=0, reward="exp", M=0, H=3, factors="device")
    d = nc.make_data(case)
    try:
        _lib.set_context(_lib.Context())
        sp = _pilco_objects(d, True, 5)
        r_sparse = sp.compute_reward()   # (the sparse model runs on the default context and leaves its graphs there)
        assert np.isfinite(np.asarray(r_sparse, dtype=float)).all()
        del sp
        gc.collect()
        p = _pilco_objects(d, False, 6)
        r = np.asarray(p.compute_reward(), dtype=float)
        assert p.ctx is _lib.get_context(), "the exact PILCO did not receive the pooled default context"
        vg = p.value_and_gradient()
        del p
        gc.collect()
        _lib.set_context(_lib.Context())
        q = _pilco_objects(d, False, 6)
        r_fresh = np.asarray(q.compute_reward(), dtype=float)
        vg_fresh = q.value_and_gradient()
        assert np.array_equal(r, r_fresh), "compute_reward on the reused default context: %r, fresh: %r" % (r, r_fresh)
        assert _same(list(vg), list(vg_fresh)), "value_and_gradient differs from a fresh default context's"
        del q
        gc.collect()
    finally:
        _lib.set_context(old)


def test_a_stream_k_override_spanning_three_pairs_is_refused():
    """PILCO_SK_WAVES=4 with E = 3 at npad = 64: 42 steps on 4 waves, pairs of 6 or 8 steps -- a wave would span three pairs
    and lose the sums of the first (sk_wave_range keeps two).  build_work must fall back to the computed cut."""
    case = dict(name="sk_override", N=60, E=3, U=1, D=4, policy="linear", bf=0, reward="exp", M=0, H=3, factors="device")
    d = nc.make_data(case)
    ref, r_ref = wr.oracle_trajectory(case, d)
    prev = os.environ.get("PILCO_SK_WAVES")
    os.environ["PILCO_SK_WAVES"] = "4"
    cx = None
    try:
        cx = _context(case, d)
        _settings(cx, small=0)   # the fused head + stream-K pair launch
        a = cx.rollout(_policy(case, d), _rewards(case, d), d["m0"], d["S0"], case["H"], want_traj=True)
        geo = cx.geometry()
        _MEASURED["device"] = dict(cus=geo["cus"], sk_capacity_kc2=geo["sk_capacity"])
        g = nc.geometry(case, geo["cus"], geo["sk_capacity"])
        assert geo["sk_waves"] == g["sk_waves"] and geo["sk_waves"] != 4, "PILCO_SK_WAVES=4 kept (%d waves, the computed cut %d)" % (
            geo["sk_waves"], g["sk_waves"])
        _check_forward(case, ref, r_ref, a[3], a[2], "PILCO_SK_WAVES=4")
    finally:
        if prev is None:
            os.environ.pop("PILCO_SK_WAVES", None)
        else:
            os.environ["PILCO_SK_WAVES"] = prev
        if cx is not None:
            cx.close()
