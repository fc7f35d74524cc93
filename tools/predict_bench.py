"""Timing of MGPR.predict_f / SMGPR.predict_f (pilco_gp_predict_points, csrc/predict.hip) at deterministic test inputs.

Exact GP at N = 1000, D = 10, E = 10 and Nt in {1, 64, 1000, 10000, 100000}; the sparse model at M = 200, N = 5000 (every
output on its own Z, as SMGPR passes them).  Host-synchronised wall clock of the whole call (the call returns with the
results on the host: upload, cross-covariance, kernel, download); the kernels' own time comes from a trace:
    rocprofv3 --kernel-trace --stats -d predict_trace -o predict -- python tools/predict_bench.py --quick
Algorithmic FLOP from the shapes: the triangular product and its squares, E * Nt * n^2 (n = N, or 2 * M^2 for FITC's two
operator blocks), plus the mean (2 E Nt n); share of the f64 matrix peak of 78.6 TF (MI355X)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pilco_amd import synthetic  # noqa: E402
from pilco_amd.models import MGPR, SMGPR  # noqa: E402

PEAK = 78.6e12


def _model(cls, cfg, **kw):
    m = cls((cfg["X"], cfg["Y"]), **kw)
    for i, mdl in enumerate(m.models):
        mdl.kernel.lengthscales.assign(cfg["lengthscales"][i])
        mdl.kernel.variance.assign(cfg["variance"][i])
        mdl.likelihood.variance.assign(cfg["noise"][i])
    return m


def _time(m, xs, reps):
    m.predict_f(xs)   # warm-up: factorisation, allocations
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        m.predict_f(xs)
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="one repetition per size (for a kernel trace)")
    args = ap.parse_args()
    reps = 1 if args.quick else 5
    rs = np.random.RandomState(0)
    rows = []
    c2 = synthetic.config_c2(N=1000, D=10, E=10)
    m = _model(MGPR, c2)
    for Nt in (1, 64, 1000, 10000, 100000):
        xs = rs.randn(Nt, 10)
        t = _time(m, xs, reps if Nt < 100000 else max(1, reps // 2))
        flop = 10 * Nt * (1000.0 ** 2 + 2 * 1000)
        rows.append(dict(model="exact N=1000 D=10 E=10", Nt=Nt, ms=1e3 * t, gflops=flop / t / 1e9, peak_share=flop / t / PEAK))
    c4 = synthetic.config_c4(N=5000, M=200)
    s = _model(SMGPR, c4, num_induced_points=200)
    for i, mdl in enumerate(s.models):
        mdl.inducing_variable.Z.assign(c4["Z"] if i == 0 else rs.rand(200, 10))
    for Nt in (1, 1000, 10000, 100000):
        xs = rs.randn(Nt, 10)
        t = _time(s, xs, reps if Nt < 100000 else max(1, reps // 2))
        flop = 10 * Nt * (2 * 200.0 ** 2 + 2 * 200)
        rows.append(dict(model="FITC M=200 N=5000 D=10 E=10 (own Z per output)", Nt=Nt, ms=1e3 * t, gflops=flop / t / 1e9,
                         peak_share=flop / t / PEAK))
    for r in rows:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
