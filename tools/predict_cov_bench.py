"""Timing of the full posterior covariance and the joint samples (pilco_gp_predict_points_cov, pilco_gp_sample_points;
csrc/predict_cov.hip, docs/predict_cov.md) at N = 1000, D = 11, E = 10 and Nt in {64, 256, 1024, 4096}.

Per Nt, one JSON line:
  cov_call_ms     pilco_gp_predict_points_cov, median of host-synchronised calls (upload, kernels, download)
  sample_call_ms  pilco_gp_sample_points at S = 64, the same way
  kernel_ms       k_predict_cov alone, between events on the stream
  parts_ms        the yardstick: the same matrix from the kernels the fused one replaces (launch_gram for K**, launch_gemm
                  for W W^T on symmetric tiles, an add), between the same events in the same call
  peak_share      E Nt^2 npad multiply-adds (both triangles counted once) = 2 E Nt^2 npad FLOP over kernel_ms, as a share of
                  the fp64 matrix peak (--peak-tflops)
  max_diff        largest difference between the fused matrix and the yardstick's
kernel_ms, parts_ms and max_diff need a library built with -DPILCO_DEV (make EXTRA=-DPILCO_DEV BUILD=... OUT=..., named by the
environment variable PILCO_LIB); with the shipped library they are reported as null."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pilco_amd import _lib, synthetic  # noqa: E402


def _median(fn, reps, warm):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--peak-tflops", type=float, default=78.6, help="fp64 matrix peak of the device (MI355X: 78.6)")
    ap.add_argument("--nts", type=int, nargs="*", default=[64, 256, 1024, 4096])
    ap.add_argument("--quick", action="store_true", help="one repetition, one warm-up call (for a kernel trace)")
    args = ap.parse_args()
    reps, warm = (1, 1) if args.quick else (9, 2)
    N, D, E, S = 1000, 11, 10, 64
    cfg = synthetic.config_c2(N=N, D=D, E=E)
    cx = _lib.Context(device=0)
    cx.gp_set_data(0, cfg["X"], cfg["Y"])
    cx.gp_set_hyp(0, cfg["lengthscales"], cfg["variance"], cfg["noise"])
    cx.gp_factorize(0)
    npad = -(-N // 64) * 64
    rs = np.random.RandomState(0)
    lo, hi = cfg["X"].min(0), cfg["X"].max(0)
    for Nt in args.nts:
        xs = lo + (hi - lo) * rs.rand(Nt, D)
        row = dict(N=N, D=D, E=E, Nt=Nt, S=S)
        row["cov_call_ms"] = _median(lambda: cx.gp_predict_points_cov(0, xs, D, E), reps, warm)
        row["sample_call_ms"] = _median(lambda: cx.gp_sample_points(0, xs, D, E, S, seed=1), reps, warm)
        try:
            k, p, d = cx.predict_cov_timed(0, xs, 1 if args.quick else 20)
            row.update(kernel_ms=k, parts_ms=p, parts_over_kernel=p / k, max_diff=d,
                       peak_share=2.0 * E * Nt * Nt * npad / (k * 1e-3) / (args.peak_tflops * 1e12))
        except _lib.PilcoError as err:
            if err.code != 5:
                raise
            row.update(kernel_ms=None, parts_ms=None, max_diff=None, peak_share=None)
        print(json.dumps(row), flush=True)
    cx.close()


if __name__ == "__main__":
    main()
