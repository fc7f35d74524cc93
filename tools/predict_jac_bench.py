"""Timing of MGPR / SMGPR.predict_f_jacobian (pilco_gp_predict_points_jac, csrc/predict_jac.hip) beside what it replaces.

Exact GP at N = 1000, D = E = 10 (C2 size) and the sparse model of config 4 (M = 200, N = 5000, every output on its own Z),
Nt in {64, 1000, 10000}.  One process; per size the median of 12 repetitions after 3 warm-up calls of
  (a) predict_f(xs)                     values only
  (b) predict_f_jacobian(xs)            values and both Jacobians, one call
  (c) predict_f on the 2 D Nt points xs +- h e_d and the central differences formed from them: what a user did before
Host-synchronised wall clock of the whole call (upload, kernels, download).  (b) and (c) must agree to the accuracy of the
differences: with h = 1e-4 their truncation error is h^2 / 6 |f'''| ~ 1e-8 of the derivative's scale and the rounding of
predict_f enters as its error / h; 1e-5 of the scale (max |dmean_e|, sf2_e / min_d l_ed) bounds both with room.
The kernels' own time comes from a trace taken on its own:
    rocprofv3 --kernel-trace --stats -d jac_trace -o jac -- python tools/predict_jac_bench.py --quick"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pilco_amd import synthetic  # noqa: E402
from pilco_amd.models import MGPR, SMGPR  # noqa: E402

H = 1e-4
FD_TOL = 1e-5


def _model(cls, cfg, **kw):
    m = cls((cfg["X"], cfg["Y"]), **kw)
    for i, mdl in enumerate(m.models):
        mdl.kernel.lengthscales.assign(cfg["lengthscales"][i])
        mdl.kernel.variance.assign(cfg["variance"][i])
        mdl.likelihood.variance.assign(cfg["noise"][i])
    return m


def _median(fn, reps, warm):
    for _ in range(warm):
        out = fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), out


def central_differences(m, xs):
    """(dmean, dvar) (Nt, E, D) from one predict_f call on the 2 D Nt shifted points."""
    Nt, D = xs.shape
    pts = np.repeat(xs[:, None, :], 2 * D, axis=1)            # (Nt, 2 D, D)
    for d in range(D):
        pts[:, 2 * d, d] += H
        pts[:, 2 * d + 1, d] -= H
    mean, var = (np.asarray(a).reshape(Nt, D, 2, -1) for a in m.predict_f(pts.reshape(-1, D)))
    diff = lambda a: ((a[:, :, 0] - a[:, :, 1]) / (2 * H)).transpose(0, 2, 1)
    return diff(mean), diff(var)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="one repetition, one warm-up call per size (for a kernel trace)")
    args = ap.parse_args()
    reps, warm = (1, 1) if args.quick else (12, 3)
    rs = np.random.RandomState(0)
    c2 = synthetic.config_c2(N=1000, D=10, E=10)
    c4 = synthetic.config_c4(N=5000, M=200)
    sparse = _model(SMGPR, c4, num_induced_points=200)
    for i, mdl in enumerate(sparse.models):
        mdl.inducing_variable.Z.assign(c4["Z"] if i == 0 else rs.rand(200, 10))
    for label, m, cfg in (("exact N=1000 D=10 E=10", _model(MGPR, c2), c2),
                          ("FITC M=200 N=5000 D=10 E=10 (own Z per output)", sparse, c4)):
        lo, hi = cfg["X"].min(0), cfg["X"].max(0)
        scale_v = cfg["variance"] / cfg["lengthscales"].min(axis=1)
        for Nt in (64, 1000, 10000):
            xs = lo + (hi - lo) * rs.rand(Nt, 10)
            ta, _ = _median(lambda: m.predict_f(xs), reps, warm)
            tb, jac = _median(lambda: m.predict_f_jacobian(xs), reps, warm)
            tc, fd = _median(lambda: central_differences(m, xs), reps, warm)
            dmean, dvar = np.asarray(jac[2]), np.asarray(jac[3])
            em = (np.abs(fd[0] - dmean).max(axis=(0, 2)) / np.abs(dmean).max(axis=(0, 2))).max()
            ev = (np.abs(fd[1] - dvar).max(axis=(0, 2)) / scale_v).max()
            print(json.dumps(dict(model=label, Nt=Nt, predict_f_ms=1e3 * ta, jacobian_ms=1e3 * tb, central_differences_ms=1e3 * tc,
                                  jacobian_over_predict_f=tb / ta, central_differences_over_jacobian=tc / tb,
                                  fd_vs_jacobian_dmean=em, fd_vs_jacobian_dvar=ev)), flush=True)
            assert em <= FD_TOL and ev <= FD_TOL, (label, Nt, em, ev)


if __name__ == "__main__":
    main()
