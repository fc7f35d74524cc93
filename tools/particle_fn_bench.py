#!/usr/bin/env python
"""Particle rollouts on posterior function samples (PILCO.sample_trajectories(dynamics="function") ->
pilco_rollout_particles_fn) beside the marginal rollout, on the same library in the same process.  C2u size (N = 1000, state
10 + 1 control, H = 40), P = 1024 and 4096, L = 512; median (min-max) of --reps repetitions after --warmup calls, host clock
around calls that end in a device synchronisation.
  (a) the marginal call (pilco_rollout_particles): the baseline
  (b) the function-sample call
  (c) its set-up alone: (b) at H = 0
Also reported, not asserted: the ratio of the particles' variance after one step from s_x = 0 to propagate(m, 0)'s S.
Prints one JSON line per P and a markdown table (docs/particle_functions.md holds a run).

    python tools/particle_fn_bench.py [--reps 12] [--warmup 3] [--N 1000] [--H 40] [--L 512] [--P 1024 4096]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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
    ap.add_argument("--L", type=int, default=512)
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
        fn = dict(dynamics="function", num_features=a.L)
        marg = median_ms(lambda: p.sample_trajectories(None, None, a.H, x0=x0, seed=7), a.reps, a.warmup)
        func = median_ms(lambda: p.sample_trajectories(None, None, a.H, x0=x0, seed=7, **fn), a.reps, a.warmup)
        setup = median_ms(lambda: p.sample_trajectories(None, None, 0, x0=x0, seed=7, **fn), a.reps, a.warmup)
        # one step from s_x = 0: the particles' variance beside the moment-matched S (the feature bias and the sampling error)
        z = np.zeros((E, E))
        S = np.diag(p.propagate(c["m0"], z)[1])
        one = p.sample_trajectories(c["m0"], z, 1, num_particles=P, seed=7, **fn)
        ratio = np.diag(one.cov[1]) / S
        row = dict(N=a.N, E=E, U=U, H=a.H, L=a.L, P=P, reps=a.reps, marginal_ms=marg[0], marginal_min_ms=marg[1], marginal_max_ms=marg[2],
                   function_ms=func[0], function_min_ms=func[1], function_max_ms=func[2], setup_ms=setup[0], setup_min_ms=setup[1],
                   setup_max_ms=setup[2], function_step_ms=(func[0] - setup[0]) / max(a.H, 1), marginal_step_ms=marg[0] / max(a.H, 1),
                   function_over_marginal=func[0] / marg[0], variance_over_S_min=float(ratio.min()), variance_over_S_max=float(ratio.max()))
        rows.append(row)
        print(json.dumps(row))
    print()
    print("| P | (a) marginal (ms) | (b) function samples (ms) | (c) set-up, H = 0 (ms) | ((b) - (c)) per step (ms) | (a) per step (ms) | (b) / (a) | variance / S |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %d | %.2f (%.2f-%.2f) | %.2f (%.2f-%.2f) | %.2f (%.2f-%.2f) | %.3f | %.3f | %.2f | %.2f-%.2f |"
              % (r["P"], r["marginal_ms"], r["marginal_min_ms"], r["marginal_max_ms"], r["function_ms"], r["function_min_ms"],
                 r["function_max_ms"], r["setup_ms"], r["setup_min_ms"], r["setup_max_ms"], r["function_step_ms"], r["marginal_step_ms"],
                 r["function_over_marginal"], r["variance_over_S_min"], r["variance_over_S_max"]))
    for r in rows:
        met = "met" if r["function_ms"] <= r["marginal_ms"] else "NOT met"
        print("- P = %d: function samples %.2f ms, marginal draws %.2f ms (expectation: (b) not slower than (a) -- %s)"
              % (r["P"], r["function_ms"], r["marginal_ms"], met))


if __name__ == "__main__":
    main()
