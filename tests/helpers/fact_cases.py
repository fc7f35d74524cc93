"""Factorisation cases: one table for tests/test_factorisations_cpu.py (coverage guard, reference checks, sensitivity of the
criteria) and tests/test_gpu_factorisations.py (every case against the extended-precision truth of oracle/hp_factor.py).

Plain data.  A case names N data points, D inputs, E outputs, M inducing points (0 = exact GP), the noise variance and its
conditioning class:
  well  spread points (about `target` neighbours within a lengthscale per point), noise 1e-2: cond(K + s2 I) <= 1e4
  ill   close points (most pairs within a lengthscale), noise 1e-6 (GPflow's floor, where MGPR.optimize ends): cond 1e8 .. 1e10
For FITC cases the Gram matrix named is Kmm + 1e-6 I (smgpr.py:27), the inducing inputs are spread and the data points lie
among them.

The block structure the table must cover (test_factorisations_cpu.py recomputes it from N and M): nblk = ceil(N / 64) 64-row
blocks, every launch_trtri level shape (2^k - 1, 2^k and 2^k + 1 blocks, clipped last sub-problems), N = 0, 1, 63 (mod 64), and
for FITC the FITC_KSPLIT slices of the V V^T product over the data points (empty ones when Np is small) and the right-hand
side's per-block partials (Np / 64 > Mp).
"""
from __future__ import annotations

import zlib

import numpy as np

NOISE_WELL = 1e-2
NOISE_ILL = 1e-6      # GPflow's noise floor
JITTER = 1e-6         # smgpr.py:27


def _c(name, N, D, E, cls="well", M=0):
    return dict(name=name, N=N, D=D, E=E, M=M, cls=cls, noise=NOISE_WELL if cls == "well" else NOISE_ILL)


CASES = [
    # exact GP, nblk = 1
    _c("e_n1_d1", 1, 1, 1),
    _c("e_n2", 2, 3, 2),
    _c("e_n63", 63, 4, 3),
    _c("e_n64_e32", 64, 4, 32),
    # nblk = 2 .. 9
    _c("e_n65_d32", 65, 32, 2),
    _c("e_n128_ill", 128, 3, 3, "ill"),
    _c("e_n129_e32", 129, 5, 32),
    _c("e_n256_ill", 256, 2, 2, "ill"),
    _c("e_n319", 319, 6, 3),
    _c("e_n321_d1", 321, 1, 2),
    _c("e_n448_ill", 448, 4, 2, "ill"),
    _c("e_n449", 449, 8, 2),
    _c("e_n575_ill", 575, 3, 1, "ill"),
    # nblk = 15, 16, 17
    _c("e_n960", 960, 4, 1),
    _c("e_n961_d32", 961, 32, 3),
    _c("e_n1087_ill", 1087, 4, 1, "ill"),
    # nblk = 31, 32, 33, 65
    _c("e_n1984", 1984, 5, 1),
    _c("e_n1985", 1985, 3, 1),
    _c("e_n2111_ill", 2111, 4, 1, "ill"),
    _c("e_n4160_ill", 4160, 4, 1, "ill"),
    # FITC (rollout factorisation, one Z shared by the outputs)
    _c("f_m1_n50", 50, 3, 2, M=1),
    _c("f_m63_n4500", 4500, 4, 2, M=63),
    _c("f_m64_n64", 64, 4, 3, M=64),
    _c("f_m65_n300", 300, 5, 2, M=65),
    _c("f_m130_n100", 100, 4, 2, M=130),
    _c("f_m130_n1000", 1000, 6, 2, M=130),
    _c("f_m200_n5000", 5000, 10, 2, M=200),
]

BY_NAME = {c["name"]: c for c in CASES}


def _spread(n, D, ls, target):
    """Per-dimension standard deviation w of N(0, w^2) points such that a point has about `target` others within the
    squared-exponential kernel's reach: n (1 + 2 w^2 / l^2)^(-D/2) = target."""
    if n <= target:
        return 3.0 * ls
    return ls * np.sqrt(0.5 * ((n / target) ** (2.0 / D) - 1.0))


def make_data(case):
    """float64 inputs of the case: X (N, D), Y (N, E), lengthscales (E, D), variance (E), noise (E), Z (M, D) or None."""
    rs = np.random.RandomState(zlib.crc32(case["name"].encode()) & 0x7FFFFFFF)
    N, D, E, M = case["N"], case["D"], case["E"], case["M"]
    l0 = np.sqrt(D)
    ls = l0 * (0.8 + 0.4 * rs.rand(E, D))
    var = 0.5 + rs.rand(E)
    noise = case["noise"] * (1.0 + rs.rand(E)) if case["cls"] == "well" else np.full(E, case["noise"])
    Z = None
    if M:
        Z = _spread(M, D, l0, 2.0) * rs.randn(M, D)
        X = Z[rs.randint(0, M, N)] + 0.5 * l0 / np.sqrt(D) * rs.randn(N, D)
    elif case["cls"] == "well":
        X = _spread(N, D, l0, 3.0) * rs.randn(N, D)
    else:
        X = 0.35 * l0 / np.sqrt(D) * rs.randn(N, D)
    A = rs.randn(D, E) / np.sqrt(D)
    Y = np.sin(X / l0 @ A * 2.0) + (1e-1 if case["cls"] == "well" else 1e-3) * rs.randn(N, E)
    return dict(X=X, Y=Y, ls=ls, var=var, noise=noise, Z=Z)


def probes(n, k=8):
    """The fixed probe vectors iK is applied to (n, k)."""
    return np.random.RandomState(20240611 + n).randn(n, k)
