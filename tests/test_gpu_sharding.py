"""Sharded rollouts and policy gradients at every rank split and point count (cases: helpers/shard_cases.py), as groups of
contexts of this process on one GPU.  At most one group and one single-rank reference context are alive at a time.

Per case and rank count W:
- forward, host-mediated group (pilco_rollout_group), at every horizon of the case: no mismatch between the ranks; trajectory and
  reward bitwise equal to the single-rank run under the rank-count-independent pair kernel (variant 2, which shard_set selects),
  within TOL_FWD of oracle.tf_path, bitwise repeatable; every rank's route record and geometry equal the mirror.
- forced stream-K kernel (variant 0): within TOL_ROUTES of the single-rank run; every rank's stream-K cut equals the mirror's.
- peer exchange attached: bitwise the same with the graph on and off, at two horizons in a row and after detaching; the step
  is the peer step exactly where the mirror says so (D > 16: the three-kernel step on every rank).
- gradient (U > 0, D <= 14; LinearController on the device chain and on the host chain, RbfController): all ranks bitwise equal
  and equal to the single-rank call with the small step off, within TOL_GRAD of torch autograd, bitwise repeatable, the
  route record names the group exchange (none at H = 0).
Once: a one-rank communicator (the ncclAllGather branch of the records' exchange), groups reused across shapes, layouts and
with the peer exchange attached, the refusals, the sharded training objectives.

Every test records its worst error before it asserts; with $SHARD_REPORT set they are written there as JSON (the source of
docs/sharding.md)."""
import json
import os
import time

import numpy as np
import pytest

from helpers import npoints_cases as nc
from helpers import shard_cases as sc
from helpers import widths_reference as wr

pytestmark = pytest.mark.gpu

_REF = {}
_MEASURED = {}
_T0 = time.time()


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    _MEASURED["seconds"] = round(time.time() - _T0, 1)
    path = os.environ.get("SHARD_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(_MEASURED, f, indent=1, sort_keys=True)


def _note(name, key, value):
    ent = _MEASURED.setdefault(name, {})
    ent[key] = max(ent.get(key, 0.0), float(value))
    print("%s: %s %.3e" % (name, key, float(value)))


def _count(name, key, n=1):
    ent = _MEASURED.setdefault(name, {})
    ent[key] = ent.get(key, 0) + n


def _at(case, H):
    return case if case["H"] == H else dict(case, H=H)


def _ref(case):
    key = (case["name"], case["H"])
    if key not in _REF:
        d = sc.make_data(case)
        _REF[key] = (d, wr.oracle_trajectory(case, d, zero_iK=case["factors"] == "user"))
    return _REF[key]


def _load(cx, case, d):
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


def _policy(case, d):
    from pilco_amd import _lib
    E, U = case["E"], case["U"]
    if case["policy"] == "linear":
        return dict(kind=_lib.POLICY_LINEAR, state_dim=E, control_dim=U, W=d["W"], b=d["b"], max_action=d["maxact"], squash=True)
    if case["policy"] == "rbf":
        return dict(kind=_lib.POLICY_RBF, state_dim=E, control_dim=U, max_action=d["maxact"], squash=True)
    return dict(kind=_lib.POLICY_NONE, state_dim=E, control_dim=0)


def _rewards(case, d):
    from pilco_amd import _lib
    ex = dict(kind=_lib.REWARD_EXPONENTIAL, W=d["Wr"], t=d["tr"].ravel())
    li = dict(kind=_lib.REWARD_LINEAR, W=d["Wl"].ravel())
    return {"exp": [dict(ex, coef=1.0)], "lin": [dict(li, coef=1.0)], "comb": [dict(ex, coef=0.7), dict(li, coef=-0.4)]}[case["reward"]]


class _Contexts:
    """Every context a test makes, closed in `finally` (with ... as made)."""
    def __enter__(self):
        self.made = []
        return self

    def __exit__(self, *exc):
        for cx in self.made:
            cx.close()
        return False

    def one(self):
        from pilco_amd import _lib
        cx = _lib.Context()
        self.made.append(cx)
        return cx

    def reference(self, case, d):
        """The single-rank run a sharded one must reproduce to the bit: variant 2, the small step off."""
        cx = self.one()
        cx.set_pair_kernel(2)
        cx.set_small_step(0)
        _load(cx, case, d)
        return cx

    def group(self, case, d, W):
        from pilco_amd import _lib
        grp = []
        for r in range(W):
            cx = self.one()
            cx.shard_set(r, W)
            _load(cx, case, d)
            grp.append(cx)
        _lib.group_sync_model(grp)
        return grp


def _same(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return np.array_equal(np.asarray(a), np.asarray(b))


def _fwd_error(case, ref, r_ref, traj, rew):
    err = wr.normwise_error(traj, ref, case["E"])
    rerr = abs(float(np.asarray(rew).ravel()[0]) - r_ref) / max(abs(r_ref), 1e-300)
    return max(err, rerr)


def _grad_reference(case, d):
    """(reward, [d parameter]) of case: torch autograd through oracle.torch_path.  H = 1: the rollout's reward is that of the
    initial state alone (pilco.py:133: the reward of state t before its propagation), which no policy parameter reaches -- the
    reference is the oracle's reward and a gradient of exact zeros (autograd has no graph to differentiate there)."""
    if case["H"] > 1:
        return wr.torch_gradient(case, d, zero_iK=case["factors"] == "user")
    E, U = case["E"], case["U"]
    shapes = [(case["bf"], E), (case["bf"], U), (U, E)] if case["policy"] == "rbf" else [(U, E), (U,)]
    return _ref(case)[1][1], [np.zeros(sh) for sh in shapes]


def _grad_errors(g, R, G):
    return [abs(g[0] - R) / abs(R)] + [wr.block_error(np.asarray(x).reshape(np.shape(y)), y) for x, y in zip(g[1:], G)]


def _expected_route(case, m, r, H, step):
    steps = m.PL(r) > 0 and H > 0
    return dict(entry=1, step=step if H > 0 else 0, policy=1 if case["policy"] == "rbf" else 0, DT=nc.prep_dt(case["D"]), KP=nc.mm_kp(case["D"]),
                vsep=int(nc.mm_vsep(case["D"])), tape=0, H=H, npad=case["npad"]), steps


def _check_ranks(case, grp, H, step, variant, what):
    """Every rank's route record and geometry against the mirror."""
    W = len(grp)
    m = sc.Mirror(case["E"], case["U"], W, H)
    waves = []
    for r, cx in enumerate(grp):
        rt, geo = cx.last_route(), cx.geometry()
        want, steps = _expected_route(case, m, r, H, step)
        want["pair"] = variant if steps else -1
        got = {k: rt[k] for k in want}
        assert got == want, "%s, rank %d: route %s, mirror %s" % (what, r, got, want)
        g = m.rank_geometry(r, case["npad"], variant, case["factors"] != "user", geo["cus"], geo["sk_capacity"])
        if geo["sk_waves"] == 0 and g["sk_waves"] == 0:   # no stream-K cut: the step and diagonal counts are not in use (a workspace
            g.pop("sk_total"), g.pop("sk_nd")             # rebuilt for another variant keeps the last cut's)
        ggot = {k: geo[k] for k in g}
        assert ggot == g, "%s, rank %d (%s): geometry %s, mirror %s" % (what, r, m.rank_class(r), ggot, g)
        waves.append(geo["sk_waves"])
    return waves


@pytest.mark.parametrize("case,W", sc.case_runs(), ids=sc.case_ids())
def test_sharded_forward_rollout(case, W):
    from pilco_amd import _lib
    tag = "%s W=%d" % (case["name"], W)
    d = sc.make_data(case)
    m = sc.Mirror(case["E"], case["U"], W)
    _MEASURED.setdefault(tag, {}).update(npad=case["npad"], E=case["E"], U=case["U"], ranks=[m.rank_class(r) for r in range(W)],
                                         model="FITC M=%d" % case["M"] if case["M"] else "user factors" if case["factors"] == "user" else "exact",
                                         N=case["N"], horizons=list(case["horizons"]))
    with _Contexts() as made:
        ref = made.reference(case, d)
        grp = made.group(case, d, W)
        pol, rw = _policy(case, d), _rewards(case, d)
        host = {}
        for H in case["horizons"]:
            ch = _at(case, H)
            _, (otraj, orew) = _ref(ch)
            what = "%s, H=%d" % (tag, H)
            one = ref.rollout(pol, rw, d["m0"], d["S0"], H, want_traj=True)
            a = _lib.rollout_group(grp, pol, rw, d["m0"], d["S0"], H, want_traj=True)
            _check_ranks(case, grp, H, 3, 2, what)
            b = _lib.rollout_group(grp, pol, rw, d["m0"], d["S0"], H, want_traj=True)
            _note(tag, "fwd", _fwd_error(ch, otraj, orew, a[3], a[2]))
            assert a[4] == 0 and b[4] == 0, "%s: the ranks ended with different bits" % what
            assert _same(a[:4], one), "%s: not bitwise the single-rank run" % what
            assert _same(a[:4], b[:4]), "%s: not bitwise repeatable" % what
            assert _fwd_error(ch, otraj, orew, a[3], a[2]) <= sc.TOL_FWD, "%s: %.2e from the oracle (tol %.0e)" % (what, _fwd_error(ch, otraj, orew, a[3], a[2]), sc.TOL_FWD)
            _count(tag, "bitwise", 2)
            host[H] = a[:4]
        # the stream-K kernel forced on every rank: its sums depend on what a rank holds
        H = case["H"]
        for cx in grp:
            cx.set_pair_kernel(0)
        v0 = _lib.rollout_group(grp, pol, rw, d["m0"], d["S0"], H, want_traj=True)
        waves = _check_ranks(case, grp, H, 3, 0, tag + ", variant 0")
        _MEASURED[tag]["waves"] = waves
        err = max(wr.normwise_error(v0[3], host[H][3], case["E"]), abs(v0[2][0, 0] - host[H][2][0, 0]) / abs(host[H][2][0, 0]))
        _note(tag, "routes", err)
        assert v0[4] == 0 and err <= sc.TOL_ROUTES, "%s, variant 0: mismatch %d, %.2e from the single-rank run (tol %.0e)" % (tag, v0[4], err, sc.TOL_ROUTES)
        for cx in grp:
            cx.set_pair_kernel(2)
        # the peer exchange: bitwise the host-mediated run, graph on and off, two horizons in a row, and after detaching
        _lib.group_peer_attach(grp)
        assert all(cx.peer_attached() for cx in grp)
        hs = list(case["horizons"]) + [case["H"] - 1, case["H"]]
        for i, H in enumerate(hs):
            if H not in host:
                host[H] = ref.rollout(pol, rw, d["m0"], d["S0"], H, want_traj=True)
            what = "%s, peer exchange, H=%d (call %d)" % (tag, H, i)
            p = _lib.rollout_group(grp, pol, rw, d["m0"], d["S0"], H, want_traj=True)
            _check_ranks(case, grp, H, sc.peer_step(case, W, H), 2, what)
            assert p[4] == 0 and _same(p[:4], host[H]), "%s: not bitwise the host-mediated run" % what
            _count(tag, "bitwise")
        for cx in grp:
            cx.use_graph(False)
        p = _lib.rollout_group(grp, pol, rw, d["m0"], d["S0"], case["H"], want_traj=True)
        assert p[4] == 0 and _same(p[:4], host[case["H"]]), "%s, peer exchange without the graph: not bitwise the host-mediated run" % tag
        for cx in grp:
            cx.use_graph(True)
            cx.peer_detach()
        assert not any(cx.peer_attached() for cx in grp)
        p = _lib.rollout_group(grp, pol, rw, d["m0"], d["S0"], case["H"], want_traj=True)
        _check_ranks(case, grp, case["H"], 3, 2, tag + ", detached")
        assert p[4] == 0 and _same(p[:4], host[case["H"]]), "%s, detached: not bitwise the host-mediated run" % tag
        _count(tag, "bitwise", 2)


_GRAD_RUNS = [(c, W) for c, W in sc.case_runs() if c["grad"]]


def _grad_single(cx, case, d, pol, rw, H):
    if case["policy"] == "rbf":
        return cx.rollout_grad_rbf(pol, rw, d["m0"], d["S0"], H, d["cX"], d["cY"], d["cl"], 1e-4 * np.ones(case["U"]))
    return cx.rollout_grad(pol, rw, d["m0"], d["S0"], H)


def _grad_group(grp, case, d, pol, rw, H):
    from pilco_amd import _lib
    if case["policy"] == "rbf":
        return _lib.rollout_grad_rbf_group(grp, pol, rw, d["m0"], d["S0"], H, d["cX"], d["cY"], d["cl"], 1e-4 * np.ones(case["U"]))
    return _lib.rollout_grad_group(grp, pol, rw, d["m0"], d["S0"], H)


def _check_group_gradient(case, d, ref, grp, pol, rw, H, what, tag, autograd=True):
    """One sharded value-and-gradient call against the single-rank one (bitwise, every rank), itself (bitwise) and autograd."""
    W = len(grp)
    one = _grad_single(ref, case, d, pol, rw, H)
    rt1 = ref.last_route()
    out = _grad_group(grp, case, d, pol, rw, H)
    again = _grad_group(grp, case, d, pol, rw, H)
    for r, cx in enumerate(grp):
        rt = cx.last_route()
        want = dict(entry=2, tape=2, chain=rt1["chain"], exchange=2 if H > 0 else 0, H=H, npad=rt1["npad"])
        assert {k: rt[k] for k in want} == want, "%s, rank %d: route %s, expected %s" % (what, r, rt, want)
    if autograd and H > 0:
        R, G = _grad_reference(_at(case, H), d)
        errs = _grad_errors([out[0][0]] + [x[0] for x in out[1:]], R, G)
        _note(tag, "grad", max(errs))
    for r in range(W):
        assert out[0][r] == one[0] and all(np.array_equal(x[r], np.asarray(y).reshape(x[r].shape)) for x, y in zip(out[1:], one[1:])), \
            "%s: rank %d is not bitwise the single-rank call" % (what, r)
    assert _same(out, again), "%s: not bitwise repeatable" % what
    _count(tag, "bitwise", W + 1)
    if H == 0:   # no step: no reward is collected and no parameter is reached -- exact zeros, whatever the chain
        assert one[0] == 0.0 and all(not np.any(np.asarray(x)) for x in one[1:]), "%s: reward %r and gradient %s, expected exact zeros" % (what, one[0], one[1:])
        _count(tag, "bitwise")
    if autograd and H > 0:
        assert max(errs) <= sc.TOL_GRAD, "%s: reward / gradient blocks %s (tol %.0e)" % (what, ["%.2e" % e for e in errs], sc.TOL_GRAD)
    return rt1


@pytest.mark.parametrize("case,W", _GRAD_RUNS, ids=["%s-W%d" % (c["name"], W) for c, W in _GRAD_RUNS])
def test_sharded_policy_gradient(case, W):
    tag = "%s W=%d" % (case["name"], W)
    d = sc.make_data(case)
    with _Contexts() as made:
        ref = made.reference(case, d)
        grp = made.group(case, d, W)
        pol, rw = _policy(case, d), _rewards(case, d)
        chains = [("rbf", None)] if case["policy"] == "rbf" else [("device chain", 1), ("host chain", 0)]
        for name, dev in chains:
            if dev is not None:
                for cx in [ref] + grp:
                    cx.set_reverse_chain(dev)
            for H in case["horizons"]:
                rt1 = _check_group_gradient(case, d, ref, grp, pol, rw, H, "%s, %s, H=%d" % (tag, name, H), tag)
                if name == "host chain" or name == "rbf":
                    assert rt1["chain"] == 2, (tag, name, rt1)
                elif case["U"] <= 4:
                    assert rt1["chain"] == 1, (tag, name, rt1)


# ---- the records' exchange over a communicator, on one rank ------------------------------------------------------------------

@pytest.mark.parametrize("name", ["n0063_lin", "n0257", "f065_n400", "n0064_rbf"])
def test_one_rank_communicator_takes_the_collective_exchange(name):
    """comm_init(id, 0, 1) makes the context sharded: the rollout runs pack -> ncclAllGather -> assemble, the gradient compacts its
    records into the gather block, all-gathers them and the chains read them with the block geometry (GRAD_XCH_COMM).  Each result
    equals a plain context's under the same step settings (the small step off: a sharded step is never the one-launch step)."""
    case = next(c for c in sc.CASES if c["name"] == name)
    d = sc.make_data(case)
    tag = "comm " + name
    with _Contexts() as made:
        plain = made.one()
        plain.set_small_step(0)
        _load(plain, case, d)
        cx = made.one()
        cx.comm_init(cx.comm_unique_id(), 0, 1)
        assert cx.comm_count() == 1
        _load(cx, case, d)
        pol, rw = _policy(case, d), _rewards(case, d)
        for H in (0, 1, 3):
            what = "%s, H=%d" % (tag, H)
            a = cx.rollout(pol, rw, d["m0"], d["S0"], H, want_traj=True)
            rt = cx.last_route()
            b = plain.rollout(pol, rw, d["m0"], d["S0"], H, want_traj=True)
            assert rt["step"] == (3 if H > 0 else 0), (what, rt)
            assert _same(a, b), "%s: rollout differs from a plain context's" % what
            for chain in ((None,) if case["policy"] == "rbf" else (1, 0)):
                if chain is not None:
                    cx.set_reverse_chain(chain)
                    plain.set_reverse_chain(chain)
                g = _grad_single(cx, case, d, pol, rw, H)
                rt = cx.last_route()
                g1 = _grad_single(plain, case, d, pol, rw, H)
                rt1 = plain.last_route()
                assert rt["exchange"] == (1 if H > 0 else 0) and rt1["exchange"] == 0 and rt["chain"] == rt1["chain"] and rt["tape"] == 2, (what, rt, rt1)
                assert rt["chain"] == (1 if chain == 1 else 2), (what, chain, rt)
                assert _same(g, g1), "%s, chain %s: gradient differs from a plain context's" % (what, chain)
                _count(tag, "bitwise", 1)
                if H == 3 and case["H"] == 3:
                    R, G = wr.torch_gradient(case, d)
                    errs = _grad_errors(g, R, G)
                    _note(tag, "grad", max(errs))
                    assert max(errs) <= sc.TOL_GRAD, (what, errs)


# ---- groups reused across shapes ---------------------------------------------------------------------------------------------

def _stage(name, N, E, U, M=0, policy="linear", bf=0, reward="comb", H=3, data_of=None):
    return name, dict(name=data_of or name, N=N, E=E, U=U, D=E + U, policy=policy, bf=bf, reward=reward, M=M, H=H, factors="device",
                      npad=nc.round_up(M or N), grad=U > 0)


def _run_stage(grp, case, d):
    from pilco_amd import _lib
    pol, rw = _policy(case, d), _rewards(case, d)
    fwd = _lib.rollout_group(grp, pol, rw, d["m0"], d["S0"], case["H"], want_traj=True)
    routes = [cx.last_route() for cx in grp]
    grad = _grad_group(grp, case, d, pol, rw, case["H"])
    return fwd, routes, grad


def _check_stage(seq, what, case, d, got, fresh):
    fwd, routes, grad = got
    f_fwd, f_routes, f_grad = fresh
    ref, r_ref = wr.oracle_trajectory(case, d)
    _note("seq " + seq, "fwd", _fwd_error(case, ref, r_ref, fwd[3], fwd[2]))
    R, G = wr.torch_gradient(case, d)
    errs = _grad_errors([grad[0][0]] + [x[0] for x in grad[1:]], R, G)
    _note("seq " + seq, "grad", max(errs))
    assert fwd[4] == 0 and _same(fwd, f_fwd), "%s: rollout differs from a fresh group's" % what
    assert _same(grad, f_grad), "%s: gradient differs from a fresh group's" % what
    _count("seq " + seq, "bitwise", 2)
    assert _fwd_error(case, ref, r_ref, fwd[3], fwd[2]) <= sc.TOL_FWD and max(errs) <= sc.TOL_GRAD, (what, errs)
    return routes, f_routes


def _reload(grp, case, d):
    from pilco_amd import _lib
    for cx in grp:
        _load(cx, case, d)
    _lib.group_sync_model(grp)


def _fresh_results(stages, Ws):
    """What a fresh group of W ranks gives at every stage (one group alive at a time)."""
    out = []
    for (stage, case), W in zip(stages, Ws):
        d = sc.make_data(case)
        with _Contexts() as made:
            out.append(_run_stage(made.group(case, d, W), case, d))
    return out


SEQUENCES = {
    "growing data": (3, [_stage("N=%d" % n, n, 3, 1, data_of="sgrow%d" % n) for n in (60, 64, 65, 128, 129, 192, 257, 513, 130)]),
    "sparse and exact": (2, [_stage("SMGPR M=64 N=200", 200, 3, 1, M=64, data_of="ssx200"), _stage("MGPR N=64", 64, 3, 1, data_of="ssx64"),
                             _stage("SMGPR M=64 other Z", 200, 3, 1, M=64, data_of="ssx200b"), _stage("MGPR N=200", 200, 3, 1, data_of="ssx200")]),
    "E and U": (4, [_stage("E=3 U=1", 100, 3, 1, data_of="seu31"), _stage("E=2 U=2 (a rank without pairs)", 100, 2, 2, data_of="seu22"),
                    _stage("E=4 U=1", 100, 4, 1, data_of="seu41"), _stage("E=3 U=1 again", 100, 3, 1, data_of="seu31b"),
                    _stage("E=1 U=1 (one rank works)", 100, 1, 1, data_of="seu11")]),
    "RBF basis": (2, [_stage("bf=10", 120, 3, 1, policy="rbf", bf=10, data_of="srbf10"), _stage("bf=6", 120, 3, 1, policy="rbf", bf=6, data_of="srbf6"),
                      _stage("bf=12", 120, 3, 1, policy="rbf", bf=12, data_of="srbf12")]),
}


@pytest.mark.parametrize("seq", list(SEQUENCES), ids=[s.replace(" ", "_") for s in SEQUENCES])
def test_reused_group_equals_a_fresh_one(seq):
    W, stages = SEQUENCES[seq]
    fresh = _fresh_results(stages, [W] * len(stages))
    with _Contexts() as made:
        grp = None
        for (stage, case), fr in zip(stages, fresh):
            what = "sequence %s, stage %s" % (seq, stage)
            d = sc.make_data(case)
            try:
                if grp is None:
                    grp = made.group(case, d, W)
                else:
                    _reload(grp, case, d)
                got = _run_stage(grp, case, d)
            except Exception as e:
                raise AssertionError("%s: the reused group failed: %s" % (what, e)) from e
            routes, f_routes = _check_stage(seq, what, case, d, got, fr)
            assert routes == f_routes, "%s: routes %s, a fresh group's %s" % (what, routes, f_routes)


def test_live_contexts_resharded_2_3_2():
    """The same contexts under another layout: shard_set invalidates what was factorised under the old one (a rank factorises
    the outputs it owns), a rollout on the stale factor is refused; after re-factorising and syncing it is a fresh group's."""
    from pilco_amd import _lib
    name, case = _stage("E=4 U=1", 150, 4, 1, data_of="sreshard")
    d = sc.make_data(case)
    fresh = _fresh_results([(name, case)] * 2, [2, 3])
    with _Contexts() as made:
        cxs = [made.one() for _ in range(3)]
        pol, rw = _policy(case, d), _rewards(case, d)
        for i, W in enumerate((2, 3, 2)):
            what = "re-sharded to %d ranks (stage %d)" % (W, i)
            grp = cxs[:W]
            for r, cx in enumerate(grp):
                cx.shard_set(r, W)
            if i > 0:
                with pytest.raises(_lib.PilcoError, match="factoris"):
                    _lib.rollout_group(grp, pol, rw, d["m0"], d["S0"], case["H"])
                with pytest.raises(_lib.PilcoError, match="factoris"):
                    _lib.group_sync_model(grp)
            _reload(grp, case, d)
            _check_stage("re-sharded 2 3 2", what, case, d, _run_stage(grp, case, d), fresh[W - 2])


def test_shape_change_with_the_peer_exchange_attached():
    """The peer exchange's graphs have the exchange baked in: a group that stays attached while its model changes shape must not
    replay them.  Forward rollouts run the peer step, the gradient rollouts beside them the group exchange."""
    from pilco_amd import _lib
    stages = [_stage("N=100 E=3 U=1", 100, 3, 1, data_of="speer100"), _stage("N=200 E=2 U=2", 200, 2, 2, data_of="speer200"),
              _stage("SMGPR M=100 N=300 E=3 U=1", 300, 3, 1, M=100, data_of="speer300"), _stage("N=100 E=3 U=1 again", 100, 3, 1, data_of="speer100b"),
              _stage("N=65 E=3 U=1", 65, 3, 1, data_of="speer65")]
    fresh = _fresh_results(stages, [2] * len(stages))
    with _Contexts() as made:
        grp = None
        for (stage, case), fr in zip(stages, fresh):
            what = "peer exchange attached, stage %s" % stage
            d = sc.make_data(case)
            if grp is None:
                grp = made.group(case, d, 2)
                _lib.group_peer_attach(grp)
            else:
                _reload(grp, case, d)
            assert all(cx.peer_attached() for cx in grp), what
            got = _run_stage(grp, case, d)
            routes, f_routes = _check_stage("peer exchange attached", what, case, d, got, fr)
            assert [rt["step"] for rt in routes] == [5, 5] and [rt["step"] for rt in f_routes] == [3, 3], (what, routes)
            again = _run_stage(grp, case, d)
            assert _same(again[0], got[0]) and _same(again[2], got[2]), "%s: not repeatable" % what


# ---- refusals ----------------------------------------------------------------------------------------------------------------

def _refusal_group(made, name, W):
    case = next(c for c in sc.CASES if c["name"] == name)
    d = sc.make_data(case)
    grp = made.group(case, d, W)
    return case, d, grp, _policy(case, d), _rewards(case, d)


def _forward(grp, case, d, pol, rw):
    from pilco_amd import _lib
    out = _lib.rollout_group(grp, pol, rw, d["m0"], d["S0"], case["H"], want_traj=True)
    assert out[4] == 0
    return out


def test_refusal_of_a_wide_sharded_gradient():
    """D = 15 takes the plain tape, whose per-step adjoint is single rank only: refused by the plan on every rank alike, before
    anything collective is enqueued; the call returns and the group works as before."""
    from pilco_amd import _lib
    with _Contexts() as made:
        case, d, grp, pol, rw = _refusal_group(made, "d15_e14u1", 3)
        before = _forward(grp, case, d, pol, rw)
        for cx in grp:   # outside a group call a sharded context is refused for that; it leaves another last error on every member
            with pytest.raises(_lib.PilcoError, match="needs a communicator"):
                cx.rollout_grad(pol, rw, d["m0"], d["S0"], case["H"])
        t0 = time.time()
        with pytest.raises(_lib.PilcoError, match="D > 14 takes the plain tape, which is single rank only"):
            _lib.rollout_grad_group(grp, pol, rw, d["m0"], d["S0"], case["H"])
        assert time.time() - t0 < 30.0
        for r, cx in enumerate(grp):   # every member refused for the same reason of its own (none was merely released by another)
            msg = cx.lib.pilco_last_error(cx.h).decode()
            assert "D > 14 takes the plain tape, which is single rank only" in msg and "another" not in msg, "rank %d: %s" % (r, msg)
        assert _same(_forward(grp, case, d, pol, rw), before), "the group's rollout changed after the refusal"


def test_refusal_of_the_plain_tape_in_a_group():
    from pilco_amd import _lib
    with _Contexts() as made:
        case, d, grp, pol, rw = _refusal_group(made, "n0063_lin", 2)
        before = _forward(grp, case, d, pol, rw)
        g0 = _lib.rollout_grad_group(grp, pol, rw, d["m0"], d["S0"], case["H"])
        for cx in grp:
            cx.set_grad_mode(0)
        with pytest.raises(_lib.PilcoError, match="grad_mode 0 takes the plain tape, which is single rank only"):
            _lib.rollout_grad_group(grp, pol, rw, d["m0"], d["S0"], case["H"])
        grp[0].set_grad_mode(1)   # one member only: its rank is named, the other is released
        with pytest.raises(_lib.PilcoError, match="rank 1: .*grad_mode 0"):
            _lib.rollout_grad_group(grp, pol, rw, d["m0"], d["S0"], case["H"])
        grp[1].set_grad_mode(1)
        os.environ["PILCO_JAC_GB"] = "1e-6"   # the sweep buffers of the rollout over the cap: the third way to the plain tape
        try:
            with pytest.raises(_lib.PilcoError, match="a rollout over PILCO_JAC_GB takes the plain tape, which is single rank only"):
                _lib.rollout_grad_group(grp, pol, rw, d["m0"], d["S0"], case["H"])
        finally:
            del os.environ["PILCO_JAC_GB"]
        assert _same(_forward(grp, case, d, pol, rw), before), "the group's rollout changed after the refusal"
        assert _same(_lib.rollout_grad_group(grp, pol, rw, d["m0"], d["S0"], case["H"]), g0), "the group's gradient changed after the refusal"


def test_refusals_of_single_rank_calls_on_a_sharded_context():
    from pilco_amd import _lib
    with _Contexts() as made:
        case, d, grp, pol, rw = _refusal_group(made, "n0063_lin", 2)
        E, D = case["E"], case["D"]
        before = _forward(grp, case, d, pol, rw)
        with pytest.raises(_lib.PilcoError, match="rollout_batch: single rank only"):
            grp[0].rollout_batch([pol, pol], rw, np.stack([d["m0"].ravel()] * 2), np.stack([d["S0"]] * 2), case["H"])
        with pytest.raises(_lib.PilcoError, match="rollout_grad_batch: single rank only"):
            grp[1].rollout_grad_batch([pol, pol], rw, np.stack([d["m0"].ravel()] * 2), np.stack([d["S0"]] * 2), case["H"])
        with pytest.raises(_lib.PilcoError, match="predict_vjp: single rank only"):
            grp[0].gp_predict_vjp(0, np.zeros(D), 0.1 * np.eye(D), np.ones(E), np.eye(E), np.ones((D, E)), D, E)
        with pytest.raises(_lib.PilcoError, match="communicator"):
            grp[0].rollout_grad(pol, rw, d["m0"], d["S0"], case["H"])
        assert _same(_forward(grp, case, d, pol, rw), before), "the group's rollout changed after the refusals"


def test_refusal_of_an_rbf_controller_with_launches_of_its_own():
    from pilco_amd import _lib
    with _Contexts() as made:
        case, d, grp, pol, rw = _refusal_group(made, "n0064_rbf", 2)
        before = _forward(grp, case, d, pol, rw)
        for cx in grp:
            cx.set_inline_policy(0)
        with pytest.raises(_lib.PilcoError, match="several ranks.*RbfController"):
            _lib.rollout_group(grp, pol, rw, d["m0"], d["S0"], case["H"])
        with pytest.raises(_lib.PilcoError, match="several ranks.*RbfController"):
            _grad_group(grp, case, d, pol, rw, case["H"])
        for cx in grp:
            cx.set_inline_policy(1)
        assert _same(_forward(grp, case, d, pol, rw), before), "the group's rollout changed after the refusal"


def test_refusal_names_the_member_whose_beta_was_not_synced():
    from pilco_amd import _lib
    with _Contexts() as made:
        case, d, grp, pol, rw = _refusal_group(made, "n0257", 4)
        before = _forward(grp, case, d, pol, rw)
        grp[2].gp_set_hyp(0, d["ls"], d["var"], d["noise"])   # (the same values: the factorisation is redone all the same)
        grp[2].gp_factorize(0)   # its own outputs' beta rows only again
        t0 = time.time()
        with pytest.raises(_lib.PilcoError, match="rank 2: .*beta of the other ranks is missing"):
            _lib.rollout_group(grp, pol, rw, d["m0"], d["S0"], case["H"])
        with pytest.raises(_lib.PilcoError, match="rank 2: .*beta of the other ranks is missing"):
            _lib.rollout_grad_group(grp, pol, rw, d["m0"], d["S0"], case["H"])
        assert time.time() - t0 < 30.0   # the other members were released
        _lib.group_sync_model(grp)
        assert _same(_forward(grp, case, d, pol, rw), before), "the group's rollout changed after the refusal"


# ---- training objectives -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,E,W,M", [(64, 3, 2, 64), (65, 3, 2, 65), (257, 4, 3, 64), (65, 1, 2, 65), (130, 5, 8, 64)])
def test_sharded_training_objectives(N, E, W, M):
    """pilco_gp_nlml and pilco_gp_fitc_nlml sharded by output: exactly the owned outputs come back, and combined they are the
    single-rank evaluation to the last bit."""
    from pilco_amd import _lib
    D = E + 1
    case = dict(name="snlml%d_%d" % (N, E), N=N, E=E, U=1, D=D, policy="linear", bf=0, reward="exp", M=0, H=1)
    d = sc.make_data(case)
    Z_all = np.stack([d["X"][np.random.RandomState(3 + a).permutation(N)[:M]] + 0.05 for a in range(E)])
    with _Contexts() as made:
        def ctx_for(r, n):
            cx = made.one()
            if n > 1:
                cx.shard_set(r, n)
            cx.gp_set_data(0, d["X"], d["Y"])
            cx.gp_set_hyp(0, d["ls"], d["var"], d["noise"])
            return cx
        ref = ctx_for(0, 1)
        n1, g1 = ref.gp_nlml(0, D, E)
        f1 = ref.gp_fitc_nlml(0, Z_all, D, E)
        assert np.all(np.isfinite(n1)) and np.all(np.isfinite(g1)) and all(np.all(np.isfinite(x)) for x in f1)
        grp = [ctx_for(r, W) for r in range(W)]
        for r, cx in enumerate(grp):
            own = list(range(r, E, W))
            n, g = cx.gp_nlml(0, D, E)
            assert list(np.nonzero(~np.isnan(n))[0]) == own, (r, n)   # exactly the outputs the rank owns
            f = cx.gp_fitc_nlml(0, Z_all, D, E)
            assert list(np.nonzero(~np.isnan(f[0]))[0]) == own, (r, f[0])
        n2, g2 = _lib.group_nlml(grp, 0, D, E)
        f2 = _lib.group_fitc_nlml(grp, 0, Z_all, D, E)
        assert np.array_equal(n1, n2) and np.array_equal(g1, g2), "N=%d E=%d W=%d: nlml differs from the single-rank evaluation" % (N, E, W)
        assert _same(f1, f2), "N=%d E=%d W=%d M=%d: FITC objective differs from the single-rank evaluation" % (N, E, W, M)
        _count("objectives", "bitwise", 2)
