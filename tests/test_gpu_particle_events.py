"""Constraint events on particle rollouts on the MI355X: pilco_rollout_particles_events (k_particle_events,
k_particle_events_finish in csrc/particles.hip), Context.rollout_particles(events=), PILCO.sample_trajectories(events=) and
SafePILCO.sample_risk.  Counts and first hits are integers: they are held to the NumPy restatement
(tests/helpers/particle_events_restatement.py, which tests/test_particle_events_cpu.py pins to the header's host probe) on the
returned particles with array_equal, no tolerance.  Every test prints its figures before it asserts (run with -s;
docs/particles.md records them).  The models are those of tests/test_gpu_particles.py."""
import ctypes as C
import os

import numpy as np
import pytest
from scipy.stats import norm

from helpers import particle_events_restatement as er
from pilco_amd import synthetic

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
E_SHAPE = 1
U53 = 2.0 ** -53
INF, NAN = float("inf"), float("nan")
_CTX = None
_SETUPS = {}


@pytest.fixture(scope="module", autouse=True)
def own_ctx():
    """The models of this module live on a context of their own (closed at the end), not on the process-wide default."""
    from pilco_amd import _lib
    global _CTX
    _CTX = _lib.Context(device=0)
    yield _CTX
    _SETUPS.clear()
    _CTX.close()


def _config(name):
    """-> (data and hyper-parameters, controller or None, m0, S0) as tests/test_gpu_particles.py builds them."""
    from pilco_amd import controllers
    if name == "predictions":          # tests/golden/predictions.npz: state 2 + 1 control, linear policy
        g = np.load(os.path.join(GOLDEN, "predictions.npz"))
        cfg = {k: g[k] for k in ("X", "Y", "lengthscales", "variance", "noise")}
        ctl = controllers.LinearController(2, 1, max_action=1.3, ctx=_CTX)
        ctl.W.assign(np.array([[0.7, -0.4]]))
        ctl.b.assign(np.array([[0.15]]))
        return cfg, ctl, cfg["X"][:1, :2], 0.05 * np.eye(2)
    if name == "c2u":                  # the C2u shape: N = 1000, state 10 + 1 control, linear policy
        cfg = synthetic.config_c2(N=1000, D=11, E=10, control_dim=1)
        ctl = controllers.LinearController(10, 1, max_action=1.5, ctx=_CTX)
        ctl.W.assign(cfg["W"] * 5.0)
        ctl.b.assign(cfg["b"] + 0.2)
        return cfg, ctl, cfg["m0"], 0.05 * np.eye(10)
    if name == "rbf":                  # N = 300, state 3 + 2 controls, an RbfController on the rbf_controller.npz policy
        cfg = synthetic.config_c2(N=300, D=5, E=3, control_dim=2, seed=21)
        g = np.load(os.path.join(GOLDEN, "rbf_controller.npz"))
        ctl = controllers.RbfController(3, 2, g["X"].shape[0], max_action=2.0, ctx=_CTX)
        ctl.set_data((g["X"], g["Y"]))
        for i, mdl in enumerate(ctl.models):
            mdl.kernel.lengthscales.assign(g["lengthscales"][i])
        return cfg, ctl, cfg["m0"], 0.05 * np.eye(3)
    raise KeyError(name)


def _set_hyp(model, cfg):
    for i, mdl in enumerate(model.models):
        mdl.kernel.lengthscales.assign(cfg["lengthscales"][i])
        mdl.kernel.variance.assign(cfg["variance"][i])
        mdl.likelihood.variance.assign(cfg["noise"][i])


def _setup(name):
    """-> (PILCO object on this module's context with PILCO's default reward, m0, S0)."""
    if name not in _SETUPS:
        from pilco_amd.models import PILCO
        cfg, ctl, m0, S0 = _config(name)
        p = PILCO((cfg["X"], cfg["Y"]), controller=ctl, ctx=_CTX)
        _set_hyp(p.mgpr, cfg)
        _SETUPS[name] = (p, m0, S0, cfg)
    return _SETUPS[name][:3]


def _events_from(parts, K):
    """The events of a case, with thresholds taken from the particles (T, P, E) of a first call without events (particles are
    bit-reproducible per seed).  Event 0: dim 0 between its median and its largest value at the last state -- both bounds are
    particles' own coordinates, bit for bit -- as the Safe-PILCO constraint object a user would pass (E = 3: a
    RiskOfCollision box on dims 0 and 2, E = 2: a SingleConstraint).  Returns (events, index of the particle whose coordinate
    is event 0's low bound)."""
    from pilco_amd.safe import RiskOfCollision, SingleConstraint
    T, P, E = parts.shape
    last = parts[-1]
    order = np.argsort(last[:, 0], kind="stable")
    q = int(order[P // 2])
    med, top = float(last[q, 0]), float(last[:, 0].max())
    lo2, hi2 = float(parts[..., E - 1].min()), float(parts[..., E - 1].max())
    if E == 3:
        first = RiskOfCollision(3, [med, lo2], [top, hi2])
    else:
        first = SingleConstraint(0, high=top, low=med)
    if K == 1:
        return [first], q
    d = E - 1
    q10, q90 = (float(v) for v in np.quantile(parts[..., 0], [0.1, 0.9]))
    r10, r90 = (float(v) for v in np.quantile(parts[..., d], [0.1, 0.9]))
    mid = float(np.median(parts[T // 2][:, d]))
    events = [first,
              dict(clauses=[(0, med, None)], complement=False),                       # an unbounded side
              SingleConstraint(d, high=r90, low=r10, inside=False),                   # a complement
              dict(clauses=[(0, q10, q90), (d, r10, r90), (0, None, top), (d, lo2, None)], complement=False),   # four clauses
              dict(clauses=[(d, float(last[q, d]), float(last[q, d]))], complement=False),   # low = high = particle q's own coordinate
              dict(clauses=[(d, None, mid)], complement=True),
              dict(clauses=[(0, None, None)], complement=False),                      # no bound at all: every particle, every state
              dict(clauses=[(0, q90, q90 + 1e-3), (d, None, r10)], complement=False)]  # a rare corner
    assert len(events) == 8
    return events, q


def _specs(events):
    return [ev.event_spec() if hasattr(ev, "event_spec") else ev for ev in events]


def _same_rollout(a, b):
    return all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("mean", "cov", "reward_steps", "particles", "eps", "reward"))


CASES = [(n, P, H, K) for n in ("predictions", "rbf") for P in (1, 127, 128, 129, 1000) for H in (0, 1, 6) for K in (1, 8)]


@pytest.mark.parametrize("name,P,H,K", CASES, ids=["%s-P%d-H%d-K%d" % c for c in CASES])
def test_exact_counts_and_first_hits(name, P, H, K):
    """event_counts and first_hit equal the restatement on the returned particles exactly, and nothing else of the call moves:
    mean, cov, reward_steps, particles and eps are bitwise those of the same call without events."""
    p, m0, S0 = _setup(name)
    kw = dict(num_particles=P, seed=11 + P + H, return_particles=True)
    base = p.sample_trajectories(m0, S0, H, **kw)
    assert base.event_counts is None and base.event_prob is None and base.first_hit is None
    events, q = _events_from(base.particles, K)
    res = p.sample_trajectories(m0, S0, H, events=events, **kw)
    want_c, want_f = er.counts(_specs(events), res.particles), er.first_hit(_specs(events), res.particles)
    print("events %s P=%d H=%d K=%d: counts at the last state %s, particles that ever hit %s"
          % (name, P, H, K, res.event_counts[-1].tolist(), (res.first_hit >= 0).sum(axis=0).tolist()))
    assert res.event_counts.shape == (H + 1, K) and res.event_counts.dtype == np.int64
    assert res.first_hit.shape == (P, K) and res.first_hit.dtype == np.int32
    assert np.array_equal(res.event_counts, want_c)
    assert np.array_equal(res.first_hit, want_f)
    assert np.array_equal(res.event_prob, res.event_counts / P)
    assert _same_rollout(res, base)
    # the particle whose coordinate IS event 0's low bound counts as inside at the last state
    assert er.hit(_specs(events)[0], res.particles[-1, q]) and 0 <= res.first_hit[q, 0] <= H
    if P >= 2:   # no case passes on all-zero (or all-P) counts
        assert np.any((res.event_counts > 0) & (res.event_counts < P))
        assert res.event_counts[-1, 0] == P - P // 2
    if K == 8:
        assert np.all(res.event_counts[:, 6] == P) and np.all(res.first_hit[:, 6] == 0)


@pytest.mark.parametrize("name", ["predictions", "rbf"])
def test_nothing_else_moves_without_the_particles(name):
    """Without return_particles the states of a step live in two alternating slabs: the counting launches read the slab
    before the next step overwrites it.  Counts and first hits equal those of the call that keeps the particles, and mean, cov,
    reward_steps and eps are bitwise those of the call without events."""
    p, m0, S0 = _setup(name)
    P, H = 385, 5
    kept = p.sample_trajectories(m0, S0, H, num_particles=P, seed=3, return_particles=True)
    events, _ = _events_from(kept.particles, 8)
    plain = p.sample_trajectories(m0, S0, H, num_particles=P, seed=3)
    res = p.sample_trajectories(m0, S0, H, num_particles=P, seed=3, events=events)
    print("slabs %s: counts per state of event 0 %s" % (name, res.event_counts[:, 0].tolist()))
    assert res.particles is None
    assert all(np.array_equal(getattr(res, f), getattr(plain, f)) for f in ("mean", "cov", "reward_steps", "eps"))
    assert np.array_equal(res.event_counts, er.counts(_specs(events), kept.particles))
    assert np.array_equal(res.first_hit, er.first_hit(_specs(events), kept.particles))


def test_chunk_boundary():
    """C2u shape (N = 1000, state 10 + 1 control): 1600 particles are one chunk of the GP step, the 1601st is a chunk of its
    own.  The counting launches see all particles of a step at once."""
    p, m0, S0 = _setup("c2u")
    P, H = 1601, 2
    base = p.sample_trajectories(m0, S0, H, num_particles=P, seed=4, return_particles=True)
    events, q = _events_from(base.particles, 8)
    last = base.particles[-1, -1]
    events[7] = dict(clauses=[(3, float(last[3]), float(last[3]))], complement=False)   # the particle past the chunk, alone
    res = p.sample_trajectories(m0, S0, H, num_particles=P, seed=4, return_particles=True, events=events)
    print("chunk boundary: counts %s, first hit of particle 1600: %s" % (res.event_counts.tolist(), res.first_hit[-1].tolist()))
    assert _same_rollout(res, base)
    assert np.array_equal(res.event_counts, er.counts(_specs(events), res.particles))
    assert np.array_equal(res.first_hit, er.first_hit(_specs(events), res.particles))
    assert res.first_hit[1600, 7] == H and res.event_counts[H, 7] >= 1
    assert np.any((res.event_counts > 0) & (res.event_counts < P))


def _raw_run(name, x0, H, eps, events):
    p, _, _ = _setup(name)
    p.mgpr._user_factors = None
    p.mgpr._ensure_factorized()
    return _CTX.rollout_particles(p._policy_spec(), p._reward_terms(), x0, H, eps=eps, want_particles=True, events=events)


def test_permuted_particles_give_permuted_first_hits_and_equal_counts():
    p, m0, S0 = _setup("rbf")
    P, H = 300, 3
    base = p.sample_trajectories(m0, S0, H, num_particles=P, seed=6, return_particles=True)
    events = _specs(_events_from(base.particles, 8)[0])
    x0, eps = base.particles[0], base.eps
    full = _raw_run("rbf", x0, H, eps, events)
    perm = np.random.RandomState(5).permutation(P)
    pm = _raw_run("rbf", x0[perm], H, eps[:, perm], events)
    print("permutation: counts %s" % full[5].tolist())
    assert np.array_equal(full[3], base.particles) and np.array_equal(pm[3], full[3][:, perm])
    assert np.array_equal(pm[6], full[6][perm]) and np.array_equal(pm[5], full[5])
    assert np.array_equal(full[5], er.counts(events, full[3])) and np.array_equal(full[6], er.first_hit(events, full[3]))
    assert np.any((full[5] > 0) & (full[5] < P))


def test_a_nan_row_counts_as_complement_says():
    """H = 0 launches no GP work: x0 itself is counted.  One NaN row (in the second block of 128)."""
    p, m0, S0 = _setup("predictions")
    P = 130
    x0 = m0 + np.random.RandomState(2).randn(P, 2) * 0.2
    x0[129] = NAN
    box = [(0, float(m0[0, 0]) - 0.1, float(m0[0, 0]) + 0.1)]
    events = [dict(clauses=box, complement=False), dict(clauses=box, complement=True),
              dict(clauses=[(1, None, None)], complement=False), dict(clauses=[(1, None, None)], complement=True)]
    res = p.sample_trajectories(None, None, 0, x0=x0, events=events, return_particles=True)
    n_in = int(((x0[:129, 0] >= box[0][1]) & (x0[:129, 0] <= box[0][2])).sum())
    print("NaN row: counts %s (inside the box among the 129 finite rows: %d); first hits of the NaN row %s"
          % (res.event_counts.tolist(), n_in, res.first_hit[129].tolist()))
    assert 0 < n_in < 129
    assert res.event_counts.tolist() == [[n_in, P - n_in, P - 1, 1]]
    assert res.first_hit[129].tolist() == [-1, 0, -1, 0]
    assert np.array_equal(res.event_counts, er.counts(events, res.particles))
    assert np.array_equal(res.first_hit, er.first_hit(events, res.particles))


# ------------------------------------------------------------------ refusals
def _event_array(events):
    from pilco_amd import _lib
    arr = (_lib.Event * max(len(events), 1))()
    for k, (n_clauses, complement, clauses) in enumerate(events):
        arr[k].n_clauses, arr[k].complement = n_clauses, complement
        for j, (dim, low, high) in enumerate(clauses[:4]):
            arr[k].clause[j].dim, arr[k].clause[j].low, arr[k].clause[j].high = dim, low, high
    return arr


def test_refusals():
    from pilco_amd import _lib
    g = np.load(os.path.join(GOLDEN, "predictions.npz"))
    E, U, P, H = 2, 1, 10, 2
    x0 = np.random.RandomState(0).randn(P, E)
    mean, cov = np.empty((H + 1, E)), np.empty((H + 1, E, E))
    parts = np.empty((H + 1, P, E))
    spec = dict(kind=_lib.POLICY_LINEAR, state_dim=E, control_dim=U, W=np.ones((U, E)), b=np.zeros(U), max_action=1.0)
    rw = [dict(kind=_lib.REWARD_EXPONENTIAL, coef=1.0, W=np.eye(E), t=None)]
    good = (1, 0, [(0, -1.0, 1.0)])
    cx = _lib.Context(device=0)
    try:
        cx.gp_set_data(0, g["X"], g["Y"])
        cx.gp_set_hyp(0, g["lengthscales"], g["variance"], g["noise"])
        pol, k1 = cx._policy(spec)
        terms, k2 = cx._rewards(rw, E)
        q = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))

        def raw(events, n_events, counts, first, null_table=False, P_=P):
            cp = None if counts is None else counts.ctypes.data_as(C.POINTER(C.c_longlong))
            fp = None if first is None else first.ctypes.data_as(C.POINTER(C.c_int))
            return cx.lib.pilco_rollout_particles_events(cx.h, C.byref(pol), terms, 1, q(x0), P_, H, None, C.c_ulonglong(0), 0,
                                                         q(mean), q(cov), None, q(parts), None,
                                                         None if null_table else _event_array(events), n_events, cp, fp)
        counts, first = np.full((H + 1, 8), -7, np.int64), np.full((P, 8), -7, np.int32)
        bad = [("n_events < 0", [good], -1, {}), ("n_events > 8", [good] * 9, 9, {}),
               ("null event table", [good], 1, dict(null_table=True)), ("null counts", [good], 1, dict(no_counts=True)),
               ("no clause", [(0, 0, [])], 1, {}), ("five clauses", [(5, 0, [(0, -1.0, 1.0)] * 4)], 1, {}),
               ("dim < 0", [(1, 0, [(-1, -1.0, 1.0)])], 1, {}), ("dim = E", [(1, 0, [(E, -1.0, 1.0)])], 1, {}),
               ("NaN low", [(1, 0, [(0, NAN, 1.0)])], 1, {}), ("NaN high", [(1, 0, [(0, -1.0, NAN)])], 1, {}),
               ("low > high", [(1, 0, [(0, 1.0, -1.0)])], 1, {}),
               ("a fault in the second event", [good, (2, 0, [(0, -1.0, 1.0), (1, 2.0, 1.0)])], 2, {}),
               ("P = 0: an existing refusal", [good], 1, dict(P_=0))]
        for what, events, n_events, kw in bad:
            no_counts = kw.pop("no_counts", False)
            rc = raw(events, n_events, None if no_counts else counts, first, **kw)
            print("refusal %-30s -> %d  %s" % (what, rc, cx.lib.pilco_last_error(cx.h).decode()))
            assert rc == E_SHAPE, what
            assert b"rollout_particles" in cx.lib.pilco_last_error(cx.h)
            assert np.all(counts == -7) and np.all(first == -7)          # refused before anything was written
        # a valid call afterwards: correct results; first_hit may be NULL; n_events = 0 takes no table at all
        events = [good, (2, 1, [(0, -0.5, 0.5), (1, -INF, 0.0)])]
        dicts = [dict(clauses=c, complement=bool(comp)) for _, comp, c in events]
        c2 = np.full((H + 1, 2), -7, np.int64)
        f2 = np.full((P, 2), -7, np.int32)
        assert raw(events, 2, c2, f2) == 0
        assert np.array_equal(c2, er.counts(dicts, parts)) and np.array_equal(f2, er.first_hit(dicts, parts))
        c3 = np.full((H + 1, 2), -7, np.int64)
        assert raw(events, 2, c3, None) == 0 and np.array_equal(c3, c2)
        keep = parts.copy()
        assert raw([], 0, None, None, null_table=True) == 0 and np.array_equal(parts, keep)
    finally:
        cx.close()


# ------------------------------------------------------------------ the Python surface
def test_a_constraint_in_the_reward_is_counted_on_the_device():
    """ObjectiveFunction(ExponentialReward, SingleConstraint) as the reward -- the pattern of the reference's
    safe_swimmer_run.py: reward_steps = the device reward of the exponential term alone + c * counts[t] / P, c = -mu."""
    from pilco_amd import rewards
    from pilco_amd.models import PILCO
    from pilco_amd.safe import ObjectiveFunction, SingleConstraint
    p, m0, S0 = _setup("predictions")
    cfg = _SETUPS["predictions"][3]
    P, H, mu = 500, 4, 0.7
    base = p.sample_trajectories(m0, S0, H, num_particles=P, seed=8, return_particles=True)     # PILCO's default reward: exp, W = I, t = 0
    con = SingleConstraint(0, high=float(np.median(base.particles[2][:, 0])), inside=True)
    q = PILCO((cfg["X"], cfg["Y"]), controller=p.controller, reward=ObjectiveFunction(rewards.ExponentialReward(2), con, mu=mu), ctx=_CTX)
    _set_hyp(q.mgpr, cfg)
    res = q.sample_trajectories(m0, S0, H, num_particles=P, seed=8, events=[con])
    none = q.sample_trajectories(m0, S0, H, num_particles=P, seed=8)            # the reward's own event is counted without being asked for
    want = np.array([base.reward_steps[t] + (-mu) * float(res.event_counts[t, 0]) / P for t in range(H)])
    rel = np.abs(res.reward_steps - want) / np.abs(want)
    print("constraint in the reward: counts %s, reward_steps %s, largest relative difference %.3g (bound %.3g)"
          % (res.event_counts[:, 0].tolist(), res.reward_steps.tolist(), rel.max(), 4 * U53))
    assert np.array_equal(res.event_counts, er.counts([con.event_spec()], base.particles))
    assert np.any((res.event_counts > 0) & (res.event_counts < P))
    assert np.all(rel <= 4 * U53)
    assert res.reward[0, 0] == res.reward_steps.sum()
    assert none.event_counts is None and np.array_equal(none.reward_steps, res.reward_steps)
    assert np.array_equal(res.mean, base.mean) and np.array_equal(res.eps, base.eps)


def test_sample_risk_fields_are_their_definitions():
    from pilco_amd import rewards
    from pilco_amd.safe import RiskOfCollision, SafePILCO, SingleConstraint
    p, m0, S0 = _setup("rbf")
    cfg = _SETUPS["rbf"][3]
    P, n, mu, E = 600, 5, -3.0, 3
    probe = p.sample_trajectories(m0, S0, n, num_particles=P, seed=9, return_particles=True)
    lo = np.quantile(probe.particles[..., [0, 2]].reshape(-1, 2), 0.3, axis=0)
    hi = np.quantile(probe.particles[..., [0, 2]].reshape(-1, 2), 0.8, axis=0)
    risk = RiskOfCollision(E, lo, hi)
    sp = SafePILCO((cfg["X"], cfg["Y"]), controller=p.controller, reward_add=rewards.ExponentialReward(E), reward_mult=risk,
                   mu=mu, horizon=n, ctx=_CTX)
    _set_hyp(sp.mgpr, cfg)
    r = sp.sample_risk(m0, S0, n, num_particles=P, seed=9, return_particles=True)
    tr = r.trajectories
    spec = risk.event_spec()
    hits = er.hit(spec, tr.particles)                                  # (n+1, P)
    traj = sp.predict_trajectory(m0, S0, n)[3]
    mm = np.array([float(risk.compute_reward(traj[t, :E].reshape(1, E), traj[t, E:].reshape(E, E))[0]) for t in range(n)])
    first = er.first_hit([spec], tr.particles)[:, 0]
    any_p = float(np.mean((first >= 0) & (first < n)))
    any_mm = 1.0 - np.prod(1.0 - mm)
    obj_p = tr.reward_steps.sum() + mu * any_p
    obj_mm = float(np.ravel(sp.predict(m0, S0, n)[2])[0])
    print("sample_risk: risk_particles %s\n             risk_moment_matched %s\n             any hit: particles %.6g, moment matched %.6g"
          "; objective: particles %.6g, moment matched %.6g"
          % (r.risk_particles.tolist(), r.risk_moment_matched.tolist(), r.any_hit_particles, r.any_hit_moment_matched,
             r.objective_particles, r.objective_moment_matched))
    close = lambda a, b: np.all(np.abs(np.asarray(a) - np.asarray(b)) <= 4 * U53 * np.abs(np.asarray(b)))
    assert np.array_equal(tr.particles, probe.particles)               # the same seed: the same particles
    assert np.array_equal(tr.event_prob[:, 0], hits.sum(axis=1) / P) and np.array_equal(tr.first_hit[:, 0], first)
    assert r.risk_particles.shape == (n,) and np.array_equal(r.risk_particles, hits[:n].sum(axis=1) / P)
    assert r.risk_moment_matched.shape == (n,) and close(r.risk_moment_matched, mm)
    assert 0 < any_p < 1 and close(r.any_hit_particles, any_p)
    assert close(r.any_hit_moment_matched, any_mm)
    assert close(r.objective_particles, obj_p) and close(r.objective_moment_matched, obj_mm)
    # a hit at the last state only (t = n) is no hit within the horizon
    assert np.mean(first >= 0) >= any_p
    sp.reward_mult = type("NoEvent", (), {"compute_reward": lambda self, m, s: (0.0, 0.0)})()
    with pytest.raises(TypeError, match="event_spec"):
        sp.sample_risk(m0, S0, n, num_particles=8)
    assert SingleConstraint(0, high=1.0).event_spec()["clauses"] == [(0, None, 1.0)]


def test_known_answer_for_gaussian_initial_particles():
    """H = 0, P = 4096, x0 ~ N(m, S) drawn on the host with seed 0: the fraction inside [a, b] on dim 0 against
    Phi((b - m) / sd) - Phi((a - m) / sd), sd = sqrt(S_00), within 5 standard errors sqrt(p (1 - p) / P)."""
    p, m0, S0 = _setup("predictions")
    P, sd = 4096, float(np.sqrt(S0[0, 0]))
    a, b = float(m0[0, 0]) - 0.1, float(m0[0, 0]) + 0.2
    res = p.sample_trajectories(m0, S0, 0, num_particles=P, seed=0, events=[dict(clauses=[(0, a, b)], complement=False)])
    exact = norm.cdf((b - m0[0, 0]) / sd) - norm.cdf((a - m0[0, 0]) / sd)
    bound = 5 * np.sqrt(exact * (1 - exact) / P)
    print("known answer: event_prob %.6f, exact %.6f, |difference| %.3g (bound %.3g)"
          % (res.event_prob[0, 0], exact, abs(res.event_prob[0, 0] - exact), bound))
    assert res.event_prob.shape == (1, 1)
    assert abs(res.event_prob[0, 0] - exact) <= bound
