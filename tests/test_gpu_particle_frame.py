"""The host frames under the particle entry points on the MI355X (csrc/particle_frame.hip, docs/particle_frame.md): the
three forward rollouts stand on one frame, nothing leaks from one call to the next through the workspace they share, and a
refused conditioned call still writes nothing.  Everything here is bitwise: the frames change no arithmetic."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _build(name):
    """tests/golden/(sparse_)predictions.npz on a context of its own: state 2 + 1 control, linear policy (the "predictions"
    and "sparse" models of tests/test_gpu_particle_cond.py) -> (context, PILCO, m0, S0)"""
    from pilco_amd import _lib, controllers
    from pilco_amd.models import PILCO
    ctx = _lib.Context(device=0)
    g = np.load(os.path.join(GOLDEN, "predictions.npz" if name == "predictions" else "sparse_predictions.npz"))
    Z = g["Z"] if name == "sparse" else None
    ctl = controllers.LinearController(2, 1, max_action=1.3, ctx=ctx)
    ctl.W.assign(np.array([[0.7, -0.4]]))
    ctl.b.assign(np.array([[0.15]]))
    p = PILCO((g["X"], g["Y"]), num_induced_points=None if Z is None else Z.shape[0], controller=ctl, ctx=ctx)
    for i, mdl in enumerate(p.mgpr.models):
        mdl.kernel.lengthscales.assign(g["lengthscales"][i])
        mdl.kernel.variance.assign(g["variance"][i])
        mdl.likelihood.variance.assign(g["noise"][i])
        if Z is not None:
            mdl.inducing_variable.Z.assign(Z)
    p.mgpr._user_factors = None
    p.mgpr._ensure_factorized()
    return ctx, p, g["X"][:1, :2], 0.05 * np.eye(2)


def _events(m0):
    return [dict(clauses=[(0, None, float(m0[0, 0]))], complement=False), dict(clauses=[(0, -0.5, 0.5), (1, -0.5, 0.5)], complement=True)]


def _bits(a):
    return None if a is None else np.ascontiguousarray(a).tobytes()


def _same_bits(a, b):
    """two results (tuples of arrays, dicts of arrays, floats or None), bit for bit"""
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same_bits(u, v) for u, v in zip(a, b))
    if isinstance(a, dict):
        return sorted(a) == sorted(b) and all(_same_bits(a[k], b[k]) for k in a)
    return _bits(a) == _bits(b)


# ------------------------------------------------------------------ one frame under the three forward rollouts
@pytest.mark.parametrize("name", ["predictions", "sparse"])
def test_without_steps_the_three_rollouts_are_the_frame_alone(name):
    """H = 0: no step runs, so mean, cov, counts and first_hit are the frame's work alone and the entry points agree bit for
    bit -- P = 1, a full block and a block plus one particle, whose row is NaN (it hits the complemented event only).  The
    function-sample rollout needs the exact GP."""
    ctx, p, m0, S0 = _build(name)
    try:
        spec, terms, ev = p._policy_spec(), p._reward_terms(), _events(m0)
        for P in (1, 128, 129):
            x0 = p._initial_particles(m0, S0, P, 3 + P)
            if P == 129:
                x0[128] = np.nan
            runs = {"marginal": ctx.rollout_particles(spec, terms, x0, 0, events=ev),
                    "conditioned": ctx.rollout_particles_cond(spec, terms, x0, 0, events=ev)}
            if name == "predictions":
                runs["function"] = ctx.rollout_particles_fn(spec, terms, x0, 0, num_features=64, events=ev)
            ref = runs["marginal"]
            assert ref[0].shape == (1, 2) and ref[1].shape == (1, 2, 2) and ref[5].shape == (1, 2) and ref[6].shape == (P, 2)
            assert np.isnan(ref[0]).all() == (P == 129)
            if P == 129:
                assert ref[6][128].tolist() == [-1, 0] and ref[5][0, 1] >= 1
            for who, out in runs.items():
                print("%s P=%d %s: mean %s, counts %s" % (name, P, who, out[0].tolist(), out[5].tolist()))
                assert out[2].shape == (0,), who
                assert all(_same_bits(out[k], ref[k]) for k in (0, 1, 5, 6)), who
    finally:
        ctx.close()


# ------------------------------------------------------------------ nothing leaks through the shared workspace
def _calls(p, m0, S0, name):
    """the calls of the sequence, each a closure on the context of p: 2 slabs against H + 1, pt_rew against pc2_rew, a P that
    shrinks and grows.  The sparse model has no function samples."""
    ctx, spec, terms, ev = p.ctx, p._policy_spec(), p._reward_terms(), _events(m0)
    x = lambda P: p._initial_particles(m0, S0, P, 11 + P)
    calls = [("marginal P=129 H=3 particles", lambda: ctx.rollout_particles(spec, terms, x(129), 3, seed=5, want_particles=True)),
             ("conditioned P=65 H=2 noise path", lambda: ctx.rollout_particles_cond(spec, terms, x(65), 2, seed=6, observation_noise=True,
                                                                                    want_particles=True, want_path=True)),
             ("function P=130 H=3 L=64 events", lambda: ctx.rollout_particles_fn(spec, terms, x(130), 3, num_features=64, seed=7,
                                                                                 events=ev, want_draws=True)),
             ("marginal gradient P=129 H=3 dx0", lambda: ctx.rollout_particles_grad(spec, terms, x(129), 3, seed=8, want_dx0=True)),
             ("function gradient P=64 H=2", lambda: ctx.rollout_particles_fn_grad(spec, terms, x(64), 2, num_features=64, seed=9)),
             ("marginal P=1 H=3", lambda: ctx.rollout_particles(spec, terms, x(1), 3, seed=10))]
    if name == "sparse":
        calls = [c for c in calls if not c[0].startswith("function")]
    return calls + [calls[0]]


@pytest.mark.parametrize("name", ["predictions", "sparse"])
def test_a_call_has_the_bits_of_the_same_call_made_first_on_a_fresh_context(name):
    ctx, p, m0, S0 = _build(name)
    try:
        shared = [(what, run()) for what, run in _calls(p, m0, S0, name)]
    finally:
        ctx.close()
    for k, (what, got) in enumerate(shared[:-1]):
        fctx, fp, _, _ = _build(name)
        try:
            fresh = _calls(fp, m0, S0, name)[k][1]()
        finally:
            fctx.close()
        print("%s, call %d (%s): against a fresh context" % (name, k, what))
        assert _same_bits(got, fresh), what
        if k == 0:
            assert _same_bits(shared[-1][1], fresh), "the first call again"


# ------------------------------------------------------------------ the conditioned refusal
def test_a_refused_conditioned_call_writes_nothing_and_a_valid_call_follows():
    from pilco_amd import _lib
    ctx, p, m0, S0 = _build("predictions")
    fctx, fp, _, _ = _build("predictions")
    try:
        P, H, E, HMAX = 5, 3, 2, _lib.MAX_COND_STEPS
        x0 = p._initial_particles(m0, S0, P, 1)
        ev = _events(m0)
        pol, k1 = ctx._policy(p._policy_spec())
        rw, k2 = ctx._rewards(p._reward_terms(), E)
        evs, dp = ctx._events(ev), _lib._ptr
        outs = [np.full(s, 777.0) for s in ((HMAX + 2, E), (HMAX + 2, E, E), (HMAX + 1,), (HMAX + 2, P, E), (HMAX + 1, P, E),
                                             (P, E, HMAX, HMAX), (P, E, HMAX, HMAX), (HMAX + 1, P, E))]
        counts, first = np.full((HMAX + 2, 2), 777, np.int64), np.full((P, 2), 777, np.int32)
        co = _lib.CondOut(dp(outs[7]), dp(outs[5]), dp(outs[6]))
        rc = ctx.lib.pilco_rollout_particles_cond(ctx.h, C.byref(pol), rw, len(p._reward_terms()), dp(x0), P, HMAX + 1, None, C.c_ulonglong(2),
                                                  1, dp(outs[0]), dp(outs[1]), dp(outs[2]), dp(outs[3]), dp(outs[4]), evs, 2,
                                                  counts.ctypes.data_as(C.POINTER(C.c_longlong)), first.ctypes.data_as(C.POINTER(C.c_int)),
                                                  C.c_double(1e-8), None, C.byref(co))
        msg = ctx.lib.pilco_last_error(ctx.h).decode()
        print("H = %d: status %d, %s" % (HMAX + 1, rc, msg))
        assert rc == 1 and msg == "rollout_particles_cond: H must be at most 128 (PILCO_MAX_COND_STEPS)"
        assert all(np.all(o == 777.0) for o in outs) and np.all(counts == 777) and np.all(first == 777)
        kw = dict(seed=2, observation_noise=True, want_particles=True, events=ev, want_path=True)
        after = ctx.rollout_particles_cond(p._policy_spec(), p._reward_terms(), x0, H, **kw)
        fresh = fctx.rollout_particles_cond(fp._policy_spec(), fp._reward_terms(), x0, H, **kw)
        assert _same_bits(after, fresh)
    finally:
        ctx.close()
        fctx.close()
