#!/usr/bin/env python
"""Path-conditioned particle rollouts (PILCO.sample_trajectories(dynamics="conditioned") -> pilco_rollout_particles_cond)
beside the marginal rollout, on the same library in the same process.  C2u size (N = 1000, state 10 + 1 control, H = 40),
P = 1024 and 4096; median (min-max) of --reps repetitions after --warmup calls, host clock around calls that end in a device
synchronisation.
  (a) the marginal call (pilco_rollout_particles): the baseline
  (b) the conditioned call
  (c) (b) at H = 1
Also: (b) at H = 10, 20, 30 -- the time per step against t is the slope between neighbouring horizons -- and the bytes of
history the step kernel reads in a call, sum_t (t + 1) P E nops npad 8, over (b) - (a): what the conditioned call spends beyond the
marginal one covers the W launch and the step kernel, so the figure is a LOWER bound of the step kernel's read rate, to hold
against the 8 TB/s HBM peak of an MI355X.
Prints one JSON line per P and a markdown table (docs/particle_conditioned.md holds a run).

    python tools/particle_cond_bench.py [--reps 12] [--warmup 3] [--N 1000] [--H 40] [--P 1024 4096]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12   # bytes / s


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
    ctl = controllers.LinearController(E, U, max_action=1.5)
    ctl.W.assign(c["W"] * 5.0)
    ctl.b.assign(c["b"] + 0.2)
    p = PILCO((c["X"], c["Y"]), controller=ctl, horizon=a.H)
    for i, mdl in enumerate(p.mgpr.models):
        mdl.kernel.lengthscales.assign(c["lengthscales"][i])
        mdl.kernel.variance.assign(c["variance"][i])
        mdl.likelihood.variance.assign(c["noise"][i])
    npad = (a.N + 63) // 64 * 64
    sweep = sorted({h for h in (1, a.H // 4, a.H // 2, 3 * a.H // 4, a.H) if h >= 1})
    rows = []
    for P in a.P:
        x0 = c["m0"] + np.sqrt(0.05) * np.random.default_rng(1).standard_normal((P, E))
        marg = median_ms(lambda: p.sample_trajectories(None, None, a.H, x0=x0, seed=7), a.reps, a.warmup)
        cond = {h: median_ms(lambda: p.sample_trajectories(None, None, h, x0=x0, seed=7, dynamics="conditioned"), a.reps, a.warmup)
                for h in sweep}
        full, one = cond[a.H], cond[1]
        hist = sum((t + 1) * P * E * npad * 8 for t in range(a.H))
        extra = max(full[0] - marg[0], 1e-9) * 1e-3
        slopes = {"%d-%d" % (sweep[k], sweep[k + 1]): (cond[sweep[k + 1]][0] - cond[sweep[k]][0]) / (sweep[k + 1] - sweep[k])
                  for k in range(len(sweep) - 1)}
        row = dict(N=a.N, E=E, U=U, H=a.H, P=P, reps=a.reps, marginal_ms=marg[0], marginal_min_ms=marg[1], marginal_max_ms=marg[2],
                   conditioned_ms=full[0], conditioned_min_ms=full[1], conditioned_max_ms=full[2], h1_ms=one[0], h1_min_ms=one[1],
                   h1_max_ms=one[2], conditioned_over_marginal=full[0] / marg[0], sweep_ms={str(h): cond[h][0] for h in sweep},
                   step_ms_between=slopes, history_bytes=hist, read_rate_lower_bound=hist / extra,
                   share_of_hbm_peak=hist / extra / HBM_PEAK)
        rows.append(row)
        print(json.dumps(row))
    print()
    print("| P | (a) marginal (ms) | (b) conditioned (ms) | (c) conditioned, H = 1 (ms) | (b) / (a) | history read (GB) | read rate >= (TB/s) | of 8 TB/s |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %d | %.2f (%.2f-%.2f) | %.2f (%.2f-%.2f) | %.2f (%.2f-%.2f) | %.2f | %.1f | %.2f | %.2f |"
              % (r["P"], r["marginal_ms"], r["marginal_min_ms"], r["marginal_max_ms"], r["conditioned_ms"], r["conditioned_min_ms"],
                 r["conditioned_max_ms"], r["h1_ms"], r["h1_min_ms"], r["h1_max_ms"], r["conditioned_over_marginal"],
                 r["history_bytes"] / 1e9, r["read_rate_lower_bound"] / 1e12, r["share_of_hbm_peak"]))
    print()
    print("| P | " + " | ".join("(b) at H = %d (ms)" % h for h in sweep) + " | " +
          " | ".join("ms per step, t in %s" % k for k in rows[0]["step_ms_between"]) + " |")
    print("|---|" + "---|" * (2 * len(sweep) - 1))
    for r in rows:
        print("| %d | " % r["P"] + " | ".join("%.2f" % r["sweep_ms"][str(h)] for h in sweep) + " | " +
              " | ".join("%.3f" % v for v in r["step_ms_between"].values()) + " |")


if __name__ == "__main__":
    main()
