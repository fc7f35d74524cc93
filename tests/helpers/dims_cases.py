"""Rollout cases over the input widths D = E + U: one table for tests/test_rollout_widths_cpu.py (coverage guard, sensitivity of
the tolerances) and tests/test_gpu_rollout_widths.py (every route against the restatement and against each other).

Plain data.  A case names its shape (N points, E states, U controls, M inducing points or 0 for the exact GP), its policy
(none / linear / rbf with `bf` basis functions), its reward (exp / lin / comb), the horizon H and the routes the planner must
report for it (pilco_debug_last_route):
  fwd    default forward step: "small" (one launch per step), "fused" (fused head + pair launch), "three" (three-kernel step),
         "fused_rbf" (fused heads with the RbfController's own launches)
  policy_route  "inline" / "own" for an RbfController under the default (inline allowed) setting
  grad   "jac" (Jacobian tape) / "plain" (tape + per-step adjoint) under the default grad mode
  chain  "device" / "host" reverse chain of the default value-and-gradient rollout
  rev    "above" / "below": the device chain's k_rev_step LDS against the 64 KB default limit
  lanes  the DT bucket's batch case (rollout_batch B = 3, rollout_grad_batch B = 2 against their solo calls)

Data (make_data): inputs N(0, 1) per dimension, lengthscales (0.6 .. 1.0) * sqrt(D) so that a wide input still sees its
neighbours (squared scaled distances O(1), not O(D)), targets 0.3 sin(X A / sqrt(D)), noise variance 1e-2.
"""
from __future__ import annotations

import numpy as np

TOL_FWD = 1e-9     # normwise, per step and per m / S / reward block
TOL_GRAD = 1e-7    # normwise, per reward / dW / db (dX / dY / dls) block
TOL_ROUTES = 1e-10  # normwise, routes of the same rollout against each other where they are not bitwise


def _c(name, N, E, U, policy="linear", bf=0, reward="exp", M=0, H=3, **routes):
    c = dict(name=name, N=N, E=E, U=U, D=E + U, policy=policy, bf=bf, reward=reward, M=M, H=H)
    c.update(routes)
    return c


CASES = [
    # DT = 4
    _c("d01_e1_none", 64, 1, 0, "none", H=4, fwd="fused", lanes=True),
    _c("d03_e2u1", 100, 2, 1, reward="comb", H=4, fwd="fused", grad="jac", chain="device", rev="below"),
    _c("d04_e3u1", 130, 3, 1, H=4, fwd="small", grad="jac", chain="device", rev="below"),
    # DT = 6, 8, 10, 11, 12, 14
    _c("d05_e4u1", 200, 4, 1, reward="comb", H=5, fwd="small", grad="jac", chain="device", rev="below", lanes=True),
    _c("d06_e5u1", 180, 5, 1, reward="lin", H=4, fwd="small", grad="jac", chain="device", rev="below"),
    _c("d07_e5u2_rbf", 120, 5, 2, "rbf", bf=12, H=4, fwd="fused", policy_route="inline", grad="jac", chain="host"),
    _c("d08_e6u2_n257", 257, 6, 2, reward="lin", H=3, fwd="fused", grad="jac", chain="device", rev="below", lanes=True),
    _c("d09_e8u1", 150, 8, 1, H=3, fwd="small", grad="jac", chain="device", rev="below", lanes=True),
    _c("d10_e9u1", 220, 9, 1, H=3, fwd="small", grad="jac", chain="device", rev="below"),
    _c("d11_e10u1", 130, 10, 1, reward="comb", H=3, fwd="small", grad="jac", chain="device", rev="below", lanes=True),
    _c("d12_e6u6_hostchain", 120, 6, 6, H=3, fwd="small", grad="jac", chain="host", lanes=True),
    _c("d13_e12u1_rbf_inline", 130, 12, 1, "rbf", bf=20, H=3, fwd="small", policy_route="inline", grad="jac", chain="host"),
    _c("d14_e13u1_revabove", 110, 13, 1, H=3, fwd="small", grad="jac", chain="device", rev="above", lanes=True),
    _c("d14_e10u4", 140, 10, 4, reward="comb", H=3, fwd="small", grad="jac", chain="device", rev="above"),
    _c("d14_e12u2_rbf_own", 100, 12, 2, "rbf", bf=80, H=3, fwd="fused_rbf", policy_route="own", grad="jac", chain="host"),
    # DT = 16
    _c("d15_e14u1", 130, 14, 1, H=3, fwd="fused", grad="plain", chain="host"),
    _c("d16_e12u4_n400", 400, 12, 4, H=3, fwd="fused", grad="plain", chain="host", lanes=True),
    # DT = 32: the fused heads do not fit the LDS, every step is the three-kernel step
    _c("d17_e16u1_fitc257", 400, 16, 1, M=257, H=3, fwd="three", grad="plain", chain="host"),
    _c("d19_e18u1", 100, 18, 1, reward="lin", H=3, fwd="three", grad="plain", chain="host"),
    # (an RbfController small enough for the inline evaluation, on a step that cannot take it: the policy GP's own launches)
    _c("d20_e16u4_rbf_three", 150, 16, 4, "rbf", bf=10, H=3, fwd="three", policy_route="own", grad="plain", chain="host"),
    _c("d21_e20u1_rbf", 100, 20, 1, "rbf", bf=10, H=3, fwd="three", policy_route="own", grad="plain", chain="host"),
    _c("d23_e22u1", 90, 22, 1, H=3, fwd="three", grad="plain", chain="host"),
    _c("d24_e8u16_n520", 520, 8, 16, H=3, fwd="three", grad="plain", chain="host", lanes=True),
    _c("d26_e24u2_fitc64", 200, 24, 2, M=64, reward="comb", H=3, fwd="three", grad="plain", chain="host"),
    _c("d27_e26u1_fitc65", 150, 26, 1, M=65, H=3, fwd="three", grad="plain", chain="host"),
    _c("d29_e25u4", 80, 25, 4, H=3, fwd="three", grad="plain", chain="host"),
    _c("d31_e30u1", 90, 30, 1, H=3, fwd="three", grad="plain", chain="host"),
    _c("d32_e32_none", 100, 32, 0, "none", H=3, fwd="three"),
    _c("d32_e31u1", 130, 31, 1, H=3, fwd="three", grad="plain", chain="host"),
    _c("d32_e28u4", 90, 28, 4, reward="comb", H=3, fwd="three", grad="plain", chain="host"),
    _c("d32_e4u28_n300", 300, 4, 28, H=3, fwd="three", grad="plain", chain="host"),
]


def case_ids():
    return [c["name"] for c in CASES]


def make_data(c):
    """Deterministic model, policy, reward and initial state of a case (plain NumPy; see the module docstring)."""
    N, E, U, D, M = c["N"], c["E"], c["U"], c["D"], c["M"]
    rs = np.random.RandomState(sum(ord(ch) for ch in c["name"]) * 7919 % (2 ** 31))
    X = rs.randn(N, D)
    Y = 0.3 * np.sin(X @ rs.randn(D, E) / np.sqrt(D)) + 1e-2 * rs.randn(N, E)
    d = dict(X=X, Y=Y, ls=(0.6 + 0.4 * rs.rand(E, D)) * np.sqrt(D), var=0.3 + 0.7 * rs.rand(E), noise=1e-2 * np.ones(E))
    d["Z"] = X[rs.permutation(N)[:M]] + 0.1 * rs.randn(M, D) if M else None
    d["m0"] = 0.2 * rs.randn(1, E)
    A = rs.randn(E, E)
    d["S0"] = 0.04 * np.eye(E) + 0.01 * A @ A.T / E
    d["maxact"] = 0.8 + rs.rand(U)
    if c["policy"] == "linear":
        d["W"] = 0.6 * rs.randn(U, E) / np.sqrt(E)
        d["b"] = 0.3 * rs.randn(U)
    elif c["policy"] == "rbf":
        bf = c["bf"]
        d["cX"] = rs.randn(bf, E)
        d["cY"] = 0.4 * rs.randn(bf, U)
        d["cl"] = (0.7 + 0.4 * rs.rand(U, E)) * np.sqrt(E)
    B = rs.randn(E, E)
    d["Wr"] = (0.3 * np.eye(E) + 0.1 * B @ B.T / E)
    d["tr"] = 0.3 * rs.randn(1, E)
    d["Wl"] = 0.3 * rs.randn(E, 1)
    return d
