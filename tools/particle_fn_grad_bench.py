#!/usr/bin/env python
"""Policy gradients through function-sample particle rollouts: PILCO.particle_value_and_gradient(dynamics="function")
(pilco_rollout_particles_fn_grad: set-up once, fused value-and-Jacobian step, reverse sweep and parameter sums on the device)
beside, on the same library in the same process,
  (a) the function-sample forward call, PILCO.sample_trajectories(dynamics="function"),
  (b) the new gradient call, and
  (c) the marginal particle gradient, PILCO.particle_value_and_gradient() (pilco_rollout_particles_grad).
C2u size (N = 1000, state 10 + 1 control, LinearController, H = 40), L = 512, P = 1024 and 4096; median (min-max) of --reps
calls after --warmup, host clock around calls that end in a device synchronisation.  Asserts that (b), at the reduced horizon
--check-H on the first P (the host side holds every particle's V), agrees to 1e-9 of the largest gradient entry with a NumPy
reverse pass over host-side evaluations of the step matrices on the device's own states and draws.  Reports (b) / (a) and
(b) / (c) (expected: (b) not slower than (c)).  Prints one JSON line per P and a markdown table
(docs/particle_fn_gradients.md holds a run).

    python tools/particle_fn_grad_bench.py [--reps 12] [--warmup 3] [--N 1000] [--H 40] [--L 512] [--P 1024 4096] [--check-H 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def host_step_matrices(c, dr, z):
    """A (P, E, D) at z (P, D) in float64: [e == d] - A_e sum_l w_l sin(omega_l . z + b_l) omega_ld - var_e sum_i k_i v_i (z_d -
    X_id) / l_ed^2, the sums as matrix products."""
    X, ls, var = c["X"], c["lengthscales"], c["variance"]
    P, D = z.shape
    E = ls.shape[0]
    A = np.zeros((P, E, D))
    for e in range(E):
        om, ph, w, v = dr["omega"][e], dr["phase"][e], dr["w"][:, e, :], dr["v"][:, e, :]
        amp = np.sqrt(2.0 * var[e] / om.shape[0])
        A[:, e, :] = -amp * ((w * np.sin(z @ om.T + ph[None, :])) @ om)
        d2 = (((z / ls[e]) ** 2).sum(1)[:, None] + ((X / ls[e]) ** 2).sum(1)[None, :] - 2.0 * (z / ls[e]) @ (X / ls[e]).T)
        kv = var[e] * np.exp(-0.5 * np.maximum(d2, 0.0)) * v
        A[:, e, :] -= (z * kv.sum(1)[:, None] - kv @ X) / ls[e] ** 2
        A[:, e, e] += 1.0
    return A


def host_gradient(c, W, b, maxact, dr, xs):
    """The reverse chain in NumPy on the device's states xs (H+1, P, E); PILCO's default reward (W = I, t = 0).  -> (dW, db)"""
    H, (P, E) = xs.shape[0] - 1, xs.shape[1:]
    lam, dW, db = np.zeros((P, E)), np.zeros_like(W), np.zeros(W.shape[0])
    for t in range(H - 1, -1, -1):
        x = xs[t]
        if t < H - 1:
            u = maxact * np.sin(x @ W.T + b)
            A = host_step_matrices(c, dr, np.concatenate([x, u], axis=1))
            ds = np.einsum("ped,pe->pd", A[:, :, E:], lam) * maxact * np.cos(x @ W.T + b)
            dW += ds.T @ x
            db += ds.sum(axis=0)
            lam = np.einsum("ped,pe->pd", A[:, :, :E], lam) + ds @ W
        lam = lam - np.exp(-0.5 * np.sum(x * x, axis=1))[:, None] * x
    return dW / P, db / P


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
    ap.add_argument("--check-H", type=int, default=5, dest="check_H")
    a = ap.parse_args()
    if a.reps < 10:
        ap.error("--reps: at least 10 repetitions")
    from pilco_amd import controllers, synthetic
    from pilco_amd.models import PILCO
    E, U = 10, 1
    c = synthetic.config_c2(N=a.N, D=E + U, E=E, control_dim=U)
    W, b, maxact = c["W"] * 5.0, (c["b"] + 0.2).reshape(-1), 1.5
    ctl = controllers.LinearController(E, U, max_action=maxact)
    ctl.W.assign(W)
    ctl.b.assign(b.reshape(ctl.b.shape))
    p = PILCO((c["X"], c["Y"]), controller=ctl, horizon=a.H)
    for i, mdl in enumerate(p.mgpr.models):
        mdl.kernel.lengthscales.assign(c["lengthscales"][i])
        mdl.kernel.variance.assign(c["variance"][i])
        mdl.likelihood.variance.assign(c["noise"][i])
    fn = dict(dynamics="function", num_features=a.L)
    rows = []
    for k, P in enumerate(a.P):
        x0 = c["m0"] + np.sqrt(0.05) * np.random.default_rng(1).standard_normal((P, E))
        gap = None
        if k == 0:   # the agreement with the host-side reverse pass, at the reduced horizon
            tr = p.sample_trajectories(None, None, a.check_H, x0=x0, seed=7, return_particles=True, **fn)
            J, (dW, db) = p.particle_value_and_gradient(n=a.check_H, x0=x0, seed=7, **fn)
            assert abs(J - tr.reward_steps.sum()) <= 1e-12 * max(1.0, abs(J))
            dWh, dbh = host_gradient(c, W, b, maxact, tr.function_draws, tr.particles)
            scale = max(np.abs(dWh).max(), np.abs(dbh).max())
            gap = max(np.abs(dW - dWh).max(), np.abs(db.ravel() - dbh).max()) / scale
            assert gap <= 1e-9, gap
            del tr
        fwd = median_ms(lambda: p.sample_trajectories(None, None, a.H, x0=x0, seed=7, **fn), a.reps, a.warmup)
        dev = median_ms(lambda: p.particle_value_and_gradient(x0=x0, seed=7, **fn), a.reps, a.warmup)
        marg = median_ms(lambda: p.particle_value_and_gradient(x0=x0, seed=7), a.reps, a.warmup)
        row = dict(N=a.N, E=E, U=U, H=a.H, L=a.L, P=P, reps=a.reps, forward_ms=fwd[0], forward_min_ms=fwd[1], forward_max_ms=fwd[2],
                   grad_ms=dev[0], grad_min_ms=dev[1], grad_max_ms=dev[2], marginal_grad_ms=marg[0], marginal_grad_min_ms=marg[1],
                   marginal_grad_max_ms=marg[2], grad_over_forward=dev[0] / fwd[0], grad_over_marginal_grad=dev[0] / marg[0],
                   check_H=a.check_H if gap is not None else None, agreement=None if gap is None else float(gap))
        rows.append(row)
        print(json.dumps(row))
    print()
    print("| P | (a) function-sample forward (ms) | (b) function-sample gradient (ms) | (c) marginal gradient (ms) | (b) / (a) | (b) / (c) |")
    print("|---|---|---|---|---|---|")
    for r in rows:
        print("| %d | %.2f (%.2f-%.2f) | %.2f (%.2f-%.2f) | %.2f (%.2f-%.2f) | %.2f | %.3f |"
              % (r["P"], r["forward_ms"], r["forward_min_ms"], r["forward_max_ms"], r["grad_ms"], r["grad_min_ms"], r["grad_max_ms"],
                 r["marginal_grad_ms"], r["marginal_grad_min_ms"], r["marginal_grad_max_ms"], r["grad_over_forward"],
                 r["grad_over_marginal_grad"]))
    for r in rows:
        met = "met" if r["grad_ms"] <= r["marginal_grad_ms"] else "NOT met"
        print("- P = %d: function-sample gradient %.2f ms, marginal gradient %.2f ms (expectation: (b) not slower than (c) -- %s)"
              % (r["P"], r["grad_ms"], r["marginal_grad_ms"], met))
    if rows and rows[0]["agreement"] is not None:
        print("- agreement of (b) with the host-side reverse pass at H = %d, P = %d: %.3g of the largest gradient entry (asserted <= 1e-9)"
              % (rows[0]["check_H"], rows[0]["P"], rows[0]["agreement"]))


if __name__ == "__main__":
    main()
