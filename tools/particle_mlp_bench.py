#!/usr/bin/env python
"""Particle policy gradients with a neural-network policy (controllers.MlpController; pilco_rollout_particles_grad_mlp /
_fn_grad_mlp, docs/particle_mlp.md) beside the LinearController's, on the same library in the same process:
  (a) PILCO.particle_value_and_gradient with a LinearController (the baseline),
  (b) the same with an MlpController of 64 hidden units,
  (c) the same with 256 hidden units,
each for dynamics="function" (L features) and for the marginal gradient.  C2u size (N = 1000, state 10 + 1 control, H = 40),
P = 1024 and 4096; median (min-max) of --reps calls after --warmup, host clock around calls that end in a device
synchronisation.  The policy and its adjoint are about 4e3 fused multiply-adds per particle and step at 64 hidden units
against 6e5 of the function-sample step: (b) / (a) is expected within a few percent of 1.  Prints one JSON line per P and a
markdown table (docs/particle_mlp.md holds a run).

    python tools/particle_mlp_bench.py [--reps 12] [--warmup 3] [--N 1000] [--H 40] [--L 512] [--P 1024 4096] [--hidden 64 256]
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
    ap.add_argument("--hidden", type=int, nargs="+", default=[64, 256])
    a = ap.parse_args()
    if a.reps < 10:
        ap.error("--reps: at least 10 repetitions")
    from pilco_amd import controllers, synthetic
    from pilco_amd.models import PILCO
    E, U = 10, 1
    c = synthetic.config_c2(N=a.N, D=E + U, E=E, control_dim=U)
    lin = controllers.LinearController(E, U, max_action=1.5)
    lin.W.assign(c["W"] * 5.0)
    lin.b.assign((c["b"] + 0.2).reshape(lin.b.shape))
    p = PILCO((c["X"], c["Y"]), controller=lin, horizon=a.H)
    for i, mdl in enumerate(p.mgpr.models):
        mdl.kernel.lengthscales.assign(c["lengthscales"][i])
        mdl.kernel.variance.assign(c["variance"][i])
        mdl.likelihood.variance.assign(c["noise"][i])
    np.random.seed(3)
    ctls = [("linear", lin)] + [("mlp%d" % Hn, controllers.MlpController(E, U, num_hidden=Hn, max_action=1.5, ctx=p.ctx)) for Hn in a.hidden]
    rows = []
    for P in a.P:
        x0 = c["m0"] + np.sqrt(0.05) * np.random.default_rng(1).standard_normal((P, E))
        row = dict(N=a.N, E=E, U=U, H=a.H, L=a.L, P=P, reps=a.reps)
        for dyn, kw in (("function", dict(dynamics="function", num_features=a.L)), ("marginal", dict())):
            for name, ctl in ctls:
                p.controller = ctl
                J, grads = p.particle_value_and_gradient(x0=x0, seed=7, **kw)
                assert np.isfinite(J) and all(np.all(np.isfinite(g)) for g in grads)
                row["%s_%s_ms" % (dyn, name)] = median_ms(lambda: p.particle_value_and_gradient(x0=x0, seed=7, **kw), a.reps, a.warmup)
        rows.append(row)
        print(json.dumps(row))
    names = [n for n, _ in ctls]
    print()
    for dyn in ("function", "marginal"):
        print("| P | " + " | ".join("%s gradient, %s (ms)" % (dyn, n) for n in names) + " | "
              + " | ".join("%s / linear" % n for n in names[1:]) + " |")
        print("|---" * (2 * len(names)) + "|")
        for r in rows:
            t = [r["%s_%s_ms" % (dyn, n)] for n in names]
            print("| %d | " % r["P"] + " | ".join("%.2f (%.2f-%.2f)" % v for v in t) + " | "
                  + " | ".join("%.3f" % (v[0] / t[0][0]) for v in t[1:]) + " |")
        print()


if __name__ == "__main__":
    main()
