#!/usr/bin/env python
"""Particle rollouts: the device-resident loop (PILCO.sample_trajectories -> pilco_rollout_particles) against what a user
could do before it existed, on the same library, in the same process: H calls of MGPR.predict_f on P points with the
controller, the update and the statistics in NumPy.  C2u size (N = 1000, state 10 + 1 control, H = 40), P = 1024 and 4096;
median of --reps repetitions after --warmup.  Also one predict_f(P) call beside the loop's time per step: how much of a step
is the existing walk over the operator.  Prints one JSON line per P and a markdown table (docs/particles.md holds a run).

    python tools/particles_bench.py [--reps 12] [--warmup 3] [--N 1000] [--H 40] [--P 1024 4096]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def host_loop(p, W, b, maxact, x0, H, rng):
    """The baseline: one predict_f round trip per step, everything else in NumPy."""
    P, E = x0.shape
    x = x0
    mean, cov, rew = [x.mean(0)], [np.cov(x.T, bias=True)], []
    for _ in range(H):
        rew.append(np.exp(-0.5 * np.sum(x * x, axis=1)).mean())          # PILCO's default reward (W = I, t = 0) at zero covariance
        u = maxact * np.sin(x @ W.T + b)
        mu, v = p.mgpr.predict_f(np.concatenate([x, u], axis=1))
        x = x + np.asarray(mu) + np.sqrt(np.maximum(np.asarray(v), 0.0)) * rng.standard_normal((P, E))
        mean.append(x.mean(0))
        cov.append(np.cov(x.T, bias=True))
    return np.array(mean), np.array(cov), np.array(rew)


def median_ms(fn, reps, warmup):
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
    W, b, maxact = c["W"] * 5.0, c["b"] + 0.2, 1.5
    ctl = controllers.LinearController(E, U, max_action=maxact)
    ctl.W.assign(W)
    ctl.b.assign(b)
    p = PILCO((c["X"], c["Y"]), controller=ctl, horizon=a.H)
    for i, mdl in enumerate(p.mgpr.models):
        mdl.kernel.lengthscales.assign(c["lengthscales"][i])
        mdl.kernel.variance.assign(c["variance"][i])
        mdl.likelihood.variance.assign(c["noise"][i])
    rows = []
    for P in a.P:
        x0 = c["m0"] + np.sqrt(0.05) * np.random.default_rng(1).standard_normal((P, E))
        rng = np.random.default_rng(2)
        dev = median_ms(lambda: p.sample_trajectories(None, None, a.H, x0=x0, seed=7), a.reps, a.warmup)
        base = median_ms(lambda: host_loop(p, W, b, maxact, x0, a.H, rng), a.reps, a.warmup)
        xu = np.concatenate([x0, maxact * np.sin(x0 @ W.T + b)], axis=1)
        one = median_ms(lambda: p.mgpr.predict_f(xu), max(a.reps, 20), a.warmup)
        # the two loops compute the same thing: the same statistics up to the sampling error of P particles
        r = p.sample_trajectories(None, None, a.H, x0=x0, seed=7)
        hm, hc, hr = host_loop(p, W, b, maxact, x0, a.H, rng)
        row = dict(N=a.N, E=E, U=U, H=a.H, P=P, reps=a.reps, device_ms=dev[0], device_min_ms=dev[1], device_max_ms=dev[2],
                   host_loop_ms=base[0], host_loop_min_ms=base[1], host_loop_max_ms=base[2], ratio_host_over_device=base[0] / dev[0],
                   device_step_ms=dev[0] / a.H, predict_f_ms=one[0],
                   mean_gap_in_sigma=float(np.max(np.abs(r.mean[-1] - hm[-1]) / np.sqrt(np.diag(hc[-1]) / P))))
        rows.append(row)
        print(json.dumps(row))
    print()
    print("| P | device loop (ms) | H x predict_f + NumPy (ms) | host / device | device per step (ms) | one predict_f(P) (ms) |")
    print("|---|---|---|---|---|---|")
    for r in rows:
        print("| %d | %.2f (%.2f-%.2f) | %.2f (%.2f-%.2f) | %.2f | %.3f | %.3f |"
              % (r["P"], r["device_ms"], r["device_min_ms"], r["device_max_ms"], r["host_loop_ms"], r["host_loop_min_ms"],
                 r["host_loop_max_ms"], r["ratio_host_over_device"], r["device_step_ms"], r["predict_f_ms"]))


if __name__ == "__main__":
    main()
