#!/usr/bin/env python
"""Constraint events on particle rollouts: what the two counting launches per state cost, and what they save.  C2u size
(N = 1000, state 10 + 1 control, H = 40), P = 1024 and 4096, K = 2 events; median (min-max) of --reps repetitions after
--warmup, host clock around calls that end in a device synchronisation, all in one process:

  (a) PILCO.sample_trajectories without events
  (b) the same call with events=: counts and first hits from the device (pilco_rollout_particles_events)
  (c) what a user did before: return_particles=True, then counts and first hits in NumPy on the (H+1, P, E) download

The expectation: (b) is not slower than (c); (b) - (a) per step is reported.  (b) and (c) are checked to count the same.
Prints one JSON line per P and a markdown table (docs/particles.md holds a run).

    python tools/particle_events_bench.py [--reps 12] [--warmup 3] [--N 1000] [--H 40] [--P 1024 4096]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def numpy_counts(events, parts):
    """Counts (H+1, K) and first hits (P, K) of box events on downloaded particles (H+1, P, E), vectorised."""
    T, P, _ = parts.shape
    counts = np.empty((T, len(events)), np.int64)
    first = np.empty((P, len(events)), np.int32)
    for k, ev in enumerate(events):
        ins = np.ones((T, P), bool)
        for dim, low, high in ev["clauses"]:
            v = parts[..., dim]
            ins &= (v >= (-np.inf if low is None else low)) & (v <= (np.inf if high is None else high))
        hit = ~ins if ev["complement"] else ins
        counts[:, k] = hit.sum(axis=1)
        first[:, k] = np.where(hit.any(axis=0), hit.argmax(axis=0), -1)
    return counts, first


def stats_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts)), 1e3 * float(np.min(ts)), 1e3 * float(np.max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--N", type=int, default=1000)
    ap.add_argument("--H", type=int, default=40)
    ap.add_argument("--P", type=int, nargs="+", default=[1024, 4096])
    a = ap.parse_args()
    if a.reps < 10:
        ap.error("--reps: at least 10 repetitions")
    from pilco_amd import controllers, synthetic
    from pilco_amd.models import PILCO
    E, U = 10, 1
    c = synthetic.config_c2(N=a.N, D=E + U, E=E, control_dim=U)
    ctl = controllers.LinearController(E, U, max_action=1.5)
    ctl.W.assign(c["W"] * 5.0)
    ctl.b.assign(c["b"] + 0.2)
    p = PILCO((c["X"], c["Y"]), controller=ctl, horizon=a.H)
    for i, mdl in enumerate(p.mgpr.models):
        mdl.kernel.lengthscales.assign(c["lengthscales"][i])
        mdl.kernel.variance.assign(c["variance"][i])
        mdl.likelihood.variance.assign(c["noise"][i])
    rows = []
    for P in a.P:
        x0 = c["m0"] + np.sqrt(0.05) * np.random.default_rng(1).standard_normal((P, E))
        kw = dict(x0=x0, seed=7)
        parts = p.sample_trajectories(None, None, a.H, return_particles=True, **kw).particles
        q = np.quantile(parts[..., [0, 2]].reshape(-1, 2), [0.3, 0.8], axis=0)
        events = [dict(clauses=[(0, float(q[0, 0]), float(q[1, 0])), (2, float(q[0, 1]), float(q[1, 1]))], complement=False),
                  dict(clauses=[(1, None, float(np.median(parts[..., 1])))], complement=True)]
        plain = stats_ms(lambda: p.sample_trajectories(None, None, a.H, **kw), a.reps, a.warmup)
        dev = stats_ms(lambda: p.sample_trajectories(None, None, a.H, events=events, **kw), a.reps, a.warmup)
        host = stats_ms(lambda: numpy_counts(events, p.sample_trajectories(None, None, a.H, return_particles=True, **kw).particles),
                        a.reps, a.warmup)
        r = p.sample_trajectories(None, None, a.H, events=events, **kw)
        hc, hf = numpy_counts(events, parts)
        assert np.array_equal(r.event_counts, hc) and np.array_equal(r.first_hit, hf), "device and NumPy count differently"
        row = dict(N=a.N, E=E, U=U, H=a.H, P=P, K=len(events), reps=a.reps,
                   plain_ms=plain[0], plain_min_ms=plain[1], plain_max_ms=plain[2],
                   events_ms=dev[0], events_min_ms=dev[1], events_max_ms=dev[2],
                   download_numpy_ms=host[0], download_numpy_min_ms=host[1], download_numpy_max_ms=host[2],
                   events_cost_per_step_us=1e3 * (dev[0] - plain[0]) / a.H, numpy_over_events=host[0] / dev[0],
                   any_hit=[float(np.mean(r.first_hit[:, k] >= 0)) for k in range(len(events))])
        rows.append(row)
        print(json.dumps(row))
    print()
    print("| P | (a) without events (ms) | (b) with events (ms) | (c) particles + NumPy (ms) | (b) - (a) per step (us) | (c) / (b) |")
    print("|---|---|---|---|---|---|")
    for r in rows:
        print("| %d | %.2f (%.2f-%.2f) | %.2f (%.2f-%.2f) | %.2f (%.2f-%.2f) | %.1f | %.2f |"
              % (r["P"], r["plain_ms"], r["plain_min_ms"], r["plain_max_ms"], r["events_ms"], r["events_min_ms"], r["events_max_ms"],
                 r["download_numpy_ms"], r["download_numpy_min_ms"], r["download_numpy_max_ms"], r["events_cost_per_step_us"],
                 r["numpy_over_events"]))
    for r in rows:
        print("- P = %d: with events %.2f ms, particles + NumPy %.2f ms (expectation: (b) not slower than (c) -- %s); the events cost "
              "%.1f us per step beside %.3f ms a step." % (r["P"], r["events_ms"], r["download_numpy_ms"],
                                                            "met" if r["events_ms"] <= r["download_numpy_ms"] else "NOT met",
                                                            r["events_cost_per_step_us"], r["plain_ms"] / r["H"]))


if __name__ == "__main__":
    main()
