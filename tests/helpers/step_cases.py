"""Edge hyper-parameters and inputs of the GP moment-matching step (operand work, pair sums, mean block): one table for
tests/test_step_edges_cpu.py (coverage guard, K_ref, caps, sensitivity), oracle/gen_golden_step.py (the 40-digit truth with
units in tests/golden/step_edges.npz) and tests/test_gpu_step_edges.py (every route).  docs/step_edges.md describes it.

Plain data.  A case names a MODEL (points, lengthscales, signal variances: MODELS; its factors come from the fixture, the
factorisation is not under test) and what it feeds the step:
  cov    the input covariance: a family name, or (family, scale); "l2" in `units` scales it by diag(l) . diag(l) of output 0
  mean   where the input mean lies
  beta   "stored" (the model's), "zero", "zero0" (output 0 only), "x1e6", "cancel" (alternating signs; stored per case)
  ik     "stored", "none" (the policy-GP form, iK = NULL) or "asym" (a strongly asymmetric iK: the C ABI keeps its symmetric part)
  grad   True: the fixture holds the 40-digit gradient of <Mbar, M> + <Sbar, S> + <Vbar, V> with respect to (m, s)
  cls    the edge family the caps of K are taken over
A model with U = 0 has D = E and runs in a rollout with POLICY_NONE: the state's covariance is the step's input as it stands.
A model with U > 0 runs with a LinearController W = 0, b = 0: the joint covariance is blockdiag(s, 0) exactly (squash_sin of
an action N(0, 0)), which is what `cov` describes for such a model: the E x E block.
"""
from __future__ import annotations

import zlib

import numpy as np

from helpers import link_cases as lc
from helpers import npoints_cases as nc

TOL_GRAD = 1e-7
TINY = 2.0 ** -1022
EPS = 2.0 ** -53
CLAMP = -700.0
BLOCKS = ("M", "Sd", "So", "V")

# name: (N, E, U, lengthscales, variances, data)
MODELS = {
    # the family models: dense 4 x 4 covariances on every route (one-launch small step, fused head, three-kernel step)
    "q4": (24, 4, 0, "std", "std", "std"),
    "q4_short": (24, 4, 0, "short", "std", "std"),
    "q4_flat": (24, 4, 0, "flat", "std", "std"),
    "q4_ard": (24, 4, 0, "ard", "std", "std"),
    "q4_crossed": (24, 4, 0, "crossed", "std", "std"),
    "q4_off": (24, 4, 0, "off", "std", "std"),
    "q4_vtiny": (24, 4, 0, "std", "tiny", "std"),
    "q4_vhuge": (24, 4, 0, "std", "huge", "std"),
    "q4_vmixed": (24, 4, 0, "std", "mixed", "std"),
    "q4_big6": (24, 4, 0, "std", "std", "big6"),
    # shapes
    "e1": (24, 1, 0, "std", "std", "std"),         # E = 1: the diagonal pair only; D = 1
    "e3": (24, 3, 0, "std", "std", "std"),         # D = 3: vsep at KP = 4, fused head
    "e2u2": (24, 2, 2, "std", "std", "std"),       # the zero row with a controller
    "e2u2_ard": (24, 2, 2, "ard", "std", "std"),   # the policy-gradient cases' models (WGRAD)
    "e2u2_crossed": (24, 2, 2, "crossed", "std", "std"),
    "e2u2_flat": (24, 2, 2, "flat", "std", "std"),
    "e2u2_vmixed": (24, 2, 2, "std", "mixed", "std"),
    "e2u8": (24, 2, 8, "std", "std", "std"),       # D = 10: KP = 12
    "e3u8": (24, 3, 8, "std", "std", "std"),       # D = 11: vsep at KP = 12
    "e2u12": (24, 2, 12, "std", "std", "std"),     # D = 14: KP = 16, the last width with the operands in LDS
    "e2u13": (24, 2, 13, "std", "std", "std"),     # D = 15: vsep at KP = 16
    "e2u16": (24, 2, 16, "std", "std", "std"),     # D = 18: three-kernel step
    "e1u31": (24, 1, 31, "std", "std", "std"),     # D = 32
    "n200": (200, 2, 2, "std", "std", "std"),      # one-launch small step: several row chunks, column splits
    "n200_ard": (200, 2, 2, "ard", "std", "std"),
    "n256": (256, 2, 2, "std", "std", "std"),      # the largest one-launch step
    "n257": (257, 2, 2, "std", "std", "std"),      # the smallest model on the fused head + stream-K pair kernel
    "n257_ard": (257, 2, 2, "ard", "std", "std"),
}


def _c(name, model, cov="std", mean="near", beta="stored", ik="stored", units="", grad=False, cls=None):
    N, E, U, ls, var, data = MODELS[model]
    cov = cov if isinstance(cov, tuple) else (cov, 1.0)
    if cls is None:
        big = cov[0] == "spd" and cov[1] >= 1e3
        # ARD and a covariance with its own scale per dimension: K_ref of S's off-diagonal spans 1e3 .. 1e8 with the covariance's
        # scale, so every scale is a class of its own (one cap over all of them would judge nothing at the milder ones)
        hard = ("ard_mixed" if cov[0] == "mixed" else "ard_cov_%g" % cov[1] if units == "l2" and cov[1] >= 1e-8 else None) if ls == "ard" else None
        cls = (hard if hard else "ls_" + ls if ls != "std" else "var" if var != "std" else "big6" if data != "std" else
               "far" if mean in ("far30", "straddle", "below") else "beta" if beta in ("x1e6", "cancel") else
               "mixed" if cov[0] in ("mixed", "mixedcorr") else "corr" if cov[0] == "corr" else "largecov" if big else "ordinary")
    return dict(name=name, model=model, N=N, E=E, U=U, D=E + U, M=0, ls=ls, var=var, data=data, cov=cov, mean=mean, beta=beta, ik=ik,
                units=units, grad=grad, cls=cls)


CASES = [
    # ---- input covariance (dense, D = E = 4)
    _c("cov_zero", "q4", cov="zero", grad=True),
    _c("cov_m16", "q4", cov=("spd", 1e-16)), _c("cov_m8", "q4", cov=("spd", 1e-8), grad=True), _c("cov_m1", "q4", cov=("spd", 0.1), grad=True),
    _c("cov_p3", "q4", cov=("spd", 1e3), grad=True), _c("cov_p6", "q4", cov=("spd", 1e6)), _c("cov_p12", "q4", cov=("spd", 1e12)),
    _c("cov_m16_l2", "q4_ard", cov=("spd", 1e-16), units="l2"), _c("cov_m8_l2", "q4_ard", cov=("spd", 1e-8), units="l2"),
    _c("cov_m1_l2", "q4_ard", cov=("spd", 0.1), units="l2"), _c("cov_p3_l2", "q4_ard", cov=("spd", 1e3), units="l2"),
    _c("cov_p6_l2", "q4_ard", cov=("spd", 1e6), units="l2"), _c("cov_p12_l2", "q4_ard", cov=("spd", 1e12), units="l2"),
    _c("cov_rank1", "q4", cov="rank1", grad=True), _c("cov_zerorow", "q4", cov="zerorow"),
    _c("cov_corr6", "q4", cov=("corr", 1e-6), grad=True), _c("cov_corr12", "q4", cov=("corr", 1e-12)),
    _c("cov_mixed", "q4", cov="mixed", grad=True), _c("cov_mixedcorr", "q4", cov="mixedcorr"), _c("cov_negeig", "q4", cov="negeig"),
    # ---- lengthscales
    _c("ls_short", "q4_short"), _c("ls_short_on", "q4_short", mean="on"), _c("ls_flat", "q4_flat", grad=True),
    _c("ls_ard", "q4_ard", grad=True), _c("ls_ard_mixed", "q4_ard", cov="mixed"), _c("ls_crossed", "q4_crossed", grad=True),
    _c("ls_crossed_p3", "q4_crossed", cov=("spd", 1e3)), _c("ls_off", "q4_off"),
    # ---- signal variance
    _c("var_tiny", "q4_vtiny"), _c("var_huge", "q4_vhuge"), _c("var_mixed", "q4_vmixed"),
    # ---- mean
    _c("mean_on", "q4", mean="on"), _c("mean_far30", "q4", cov=("spd", 400.0), mean="far30"),
    _c("mean_straddle", "q4", cov=("spd", 1e-3), mean="straddle"), _c("mean_below", "q4", cov=("spd", 1e-3), mean="below"),
    _c("mean_big6", "q4_big6"),
    # ---- beta and iK
    _c("beta_zero", "q4", beta="zero"), _c("beta_zero0", "q4", beta="zero0"), _c("beta_1e6", "q4", beta="x1e6"),
    _c("beta_cancel", "q4", beta="cancel"), _c("ik_none", "q4", ik="none"), _c("ik_none_p3", "e2u2", ik="none", cov=("spd", 1e3)),
    _c("ik_asym", "q4", ik="asym"),
    # ---- shapes
    _c("e1_std", "e1"), _c("e1_p3", "e1", cov=("spd", 1e3)), _c("e3_std", "e3"), _c("e3_mixed", "e3", cov="mixed"),
    _c("e2u2_std", "e2u2"), _c("e2u2_corr6", "e2u2", cov=("corr", 1e-6)),
    _c("d10_std", "e2u8"), _c("d11_std", "e3u8"), _c("d11_mixed", "e3u8", cov="mixed"), _c("d14_std", "e2u12"), _c("d15_std", "e2u13"),
    _c("d18_std", "e2u16"), _c("d18_p3", "e2u16", cov=("spd", 1e3)), _c("d32_std", "e1u31"), _c("d32_det290", "e1u31", cov="det290", cls="largecov"),
    _c("n200_std", "n200"), _c("n200_mixed", "n200", cov="mixed"), _c("n200_ard", "n200_ard", cov=("spd", 1e3)),
    _c("n256_std", "n256"), _c("n256_corr6", "n256", cov=("corr", 1e-6)),
    _c("n257_std", "n257"), _c("n257_p6", "n257", cov=("spd", 1e6)), _c("n257_mixed", "n257", cov="mixed"),
    _c("n257_straddle", "n257", cov=("spd", 1e-3), mean="straddle"), _c("n257_ard", "n257_ard"),
    _c("n257_none", "n257", ik="none"),
]


def case_ids(cases=None):
    return [c["name"] for c in (CASES if cases is None else cases)]


def by_name(name):
    return next(c for c in CASES + WGRAD_CASES if c["name"] == name)


GRAD_CASES = [c for c in CASES if c["grad"]]

# Policy gradients through the step: rollout_grad's reward, dW and db at H = 3 with a non-zero W (make_data: W, b), against
# 40-digit central differences of the whole rollout (oracle/mp_link.gradient on the case's factors).  Not part of CASES: no
# value truth, no caps; the models are small (N = 24, E = 2, U = 2) so that the truth costs seconds.
WGRAD_H = 3
WGRAD_CASES = [
    _c("wg_std", "e2u2"), _c("wg_zero", "e2u2", cov="zero"), _c("wg_m8", "e2u2", cov=("spd", 1e-8)), _c("wg_x30", "e2u2", cov=("spd", 30.0)),
    _c("wg_corr6", "e2u2", cov=("corr", 1e-6)), _c("wg_rank1", "e2u2", cov="rank1"),
    _c("wg_ard", "e2u2_ard"), _c("wg_crossed", "e2u2_crossed"), _c("wg_flat", "e2u2_flat"), _c("wg_vmixed", "e2u2_vmixed"),
]


# ------------------------------------------------------------------ data
def _seed(s):
    return zlib.crc32(s.encode()) % (2 ** 31)


def _spd(rs, n):
    A = rs.randn(n, n)
    return np.eye(n) + A @ A.T / n


def lengthscales(kind, E, D):
    rs = np.random.RandomState(_seed("ls" + kind) + 31 * E + D)
    std = (0.6 + 0.4 * rs.rand(E, D)) * np.sqrt(D)
    if kind == "std":
        return std
    if kind == "short":
        return 1e-2 * np.ones((E, D))
    if kind == "flat":
        return 1e3 * np.ones((E, D))
    if kind == "ard":      # 1e-2 .. 1e4 inside every output, in another order per output
        base = np.logspace(-2, 4, D) if D > 1 else np.array([1e-2])
        return np.stack([np.roll(base, a) for a in range(E)])
    if kind == "crossed":  # output a short where output a + 1 is long: Lambda_a^-1 + Lambda_b^-1 is led by another output per dimension
        base = np.logspace(-2, 2, D)
        return np.stack([base if a % 2 == 0 else base[::-1] for a in range(E)])
    if kind == "off":      # one dimension switched off
        std[:, 1 % D] = 1e8
        return std
    raise KeyError(kind)


def variances(kind, E):
    rs = np.random.RandomState(_seed("var" + kind) + E)
    if kind == "std":
        return 0.3 + 0.7 * rs.rand(E)
    if kind == "tiny":
        return 1e-8 * np.ones(E)
    if kind == "huge":     # log(var_a var_b) = 27.6: the top of the table exp's stated range
        return 1e6 * np.ones(E)
    if kind == "mixed":
        return np.array([1e-8, 1e6] * E)[:E]
    raise KeyError(kind)


def make_model(name):
    """Points, targets and hyper-parameters of a model (the targets only feed the generator's factorisation)."""
    N, E, U, lsk, vark, data = MODELS[name]
    D = E + U
    rs = np.random.RandomState(_seed("model" + name.split("_")[0]) + N)
    X = rs.randn(N, D)
    Y = 0.3 * np.sin(X @ rs.randn(D, E) / np.sqrt(D)) + 1e-2 * rs.randn(N, E)
    if data == "big6":
        X = X + 1e6
    return dict(X=X, Y=Y, ls=lengthscales(lsk, E, D), var=variances(vark, E), noise=1e-2 * np.ones(E))


def covariance(c, ls):
    """The covariance block the case describes: (n, n) with n = E (the state's: U > 0 adds the exact zero rows) or D."""
    n = c["E"]
    kind, scale = c["cov"]
    rs = np.random.RandomState(_seed("cov" + kind) + n)
    spd = _spd(rs, n)
    sig = 0.3 + 0.3 * rs.rand(n)
    if kind == "std":
        s = 0.1 * spd
    elif kind == "zero":
        s = np.zeros((n, n))
    elif kind == "spd":
        s = scale * spd
    elif kind == "rank1":
        v = rs.randn(n, 1)
        s = 0.2 * v @ v.T
    elif kind == "zerorow":   # the joint of a state with a deterministic control
        s = 0.1 * spd
        s[-1, :] = 0.0
        s[:, -1] = 0.0
    elif kind == "corr":      # correlation 1 - scale between every two dimensions
        rho = 1.0 - scale
        s = np.outer(sig, sig) * (rho + (1.0 - rho) * np.eye(n))
    elif kind in ("mixed", "mixedcorr"):
        C = np.diag(np.logspace(-8, 4, n)) if n > 1 else np.array([[1e4]])
        base = spd if kind == "mixed" else (1.0 - 1e-6) + 1e-6 * np.eye(n)
        s = C @ base @ C
    elif kind == "negeig":    # one eigenvalue of -1e-12 times the largest: a propagated covariance after rounding
        w, Q = np.linalg.eigh(0.1 * spd)
        w[0] = -1e-12 * w[-1]
        s = (Q * w) @ Q.T
    elif kind == "det290":    # det B ~ 1e278, det R ~ 1e288 at D = 32 (in the units of l^2 by construction): finite, and must stay so
        return None
    else:
        raise KeyError(kind)
    s = 0.5 * (s + s.T)
    if "l2" in c["units"]:
        s = s * np.outer(ls[0, :n], ls[0, :n])
    return s


def make_data(c):
    """Everything of a case but the factors: X, ls, var, noise, the step's input (m (1, D), s (D, D)), the rollout's (m0, S0)."""
    d = make_model(c["model"])
    E, D, N = c["E"], c["D"], c["N"]
    rs = np.random.RandomState(_seed("state" + c["name"]))
    lbar = float(np.mean(d["ls"][:, :E]))
    dirn = rs.randn(E)
    dirn /= np.linalg.norm(dirn)
    near = 0.2 * rs.randn(E)
    mk = c["mean"]
    if mk == "near":
        mx = near + (1e6 if c["data"] == "big6" else 0.0)
    elif mk == "on":          # exactly on a training point: a zero zeta row
        mx = d["X"][5, :E].copy()
    elif mk == "far30":       # 30 units out with s = 400 SPD: the parts of the exponent are ~1e3 and cancel
        mx = 30.0 * dirn
    elif mk == "straddle":    # sum_d (m_d / l_0d)^2 / 2 = 700: output 0's exponents lie on both sides of the clamp
        mx = np.sqrt(1400.0 / np.sum(np.square(dirn / d["ls"][0, :E]))) * dirn
    elif mk == "below":       # everything below the clamp
        mx = 60.0 * lbar * dirn
    else:
        raise KeyError(mk)
    if mk == "on" and c["U"] > 0:
        raise ValueError("a mean on a training point needs U = 0 (the action's mean is 0)")
    if c["cov"][0] == "det290":
        assert c["U"] > 0
        sfull = 5e8 * np.diag(d["ls"][0] ** 2)
        S0 = sfull[:E, :E].copy()
        dense = True
    else:
        S0 = covariance(c, d["ls"])
        sfull = np.zeros((D, D))
        sfull[:E, :E] = S0
        dense = False
    m = np.zeros((1, D))
    m[0, :E] = mx
    d.update(m=m, s=sfull, m0=mx[None, :].copy(), S0=S0, rollable=not dense)
    d["Mbar"], d["Sbar"], d["Vbar"] = rs.randn(1, E), rs.randn(E, E), rs.randn(D, E)
    U = c["U"]
    if U > 0:    # the non-zero controller of the policy-gradient cases (the value cases run W = 0, b = 0)
        d["W"], d["b"] = 0.6 * rs.randn(U, E) / np.sqrt(E), 0.3 * rs.randn(U)
    return d


# ------------------------------------------------------------------ factors (from the fixture)
def factors_from(c, get):
    """(iK as the device gets it or None, beta, iK as the truth sees it or None) of a case; get(key) reads the fixture.
    N <= 32: the model's 40-digit inverse rounded, stored as its upper triangle; larger: iK_a = diag(d_a) - outer(g_a, g_a), every
    entry one correctly rounded product and at most one correctly rounded subtraction -- numpy reproduces it to the bit."""
    N, E = c["N"], c["E"]
    f = get("_model/" + c["model"])        # [beta (E, N) | iK upper triangles (E, N (N + 1) / 2)] or [beta | d (E, N) | g (E, N)]
    beta = f[:E * N].reshape(E, N).copy()
    if N <= 32:
        tri = f[E * N:].reshape(E, -1)
        iK = np.zeros((E, N, N))
        iu = np.triu_indices(N)
        for a in range(E):
            iK[a][iu] = tri[a]
            iK[a] = iK[a] + np.triu(iK[a], 1).T
    else:
        dd, g = f[E * N:2 * E * N].reshape(E, N), f[2 * E * N:].reshape(E, N)
        iK = np.stack([np.diag(dd[a]) - np.outer(g[a], g[a]) for a in range(E)])
    if c["beta"] == "zero":
        beta = np.zeros_like(beta)
    elif c["beta"] == "zero0":
        beta = beta.copy()
        beta[0] = 0.0
    elif c["beta"] == "x1e6":
        beta = beta * 1e6
    elif c["beta"] == "cancel":
        beta = get(c["name"] + "/beta")
    if c["ik"] == "none":
        return None, beta, None
    if c["ik"] == "asym":
        rs = np.random.RandomState(7)
        iKa = iK * (1.0 + 0.3 * rs.rand(*iK.shape))
        return iKa, beta, 0.5 * (iKa + np.swapaxes(iKa, 1, 2))
    return iK, beta, iK


# ------------------------------------------------------------------ routes
def geometry(c):
    return nc.geometry(dict(c, factors="user" if c["ik"] == "none" else "device"))


def routes(c):
    """The routes a case runs on: (name, kind, settings, expected).
    predict  gp_predict under a pair-kernel variant (predict_v1 only where the library has the plain-VALU kernel: the GPU test asks)
    tape     rollout_tape's step record; expected: the step of last_route() (1 fused head, 2 one-launch small step, 3 three-kernel)
    grad     the forward half of a value-and-gradient rollout (H = 2, W = 0 controller, ExponentialReward): its pair sums run in
             other code -- small_sweep inside the head (pair 5) or the reverse-sweep launch of bwd.hip (pair 4) on the Jacobian
             tape, the forward kernels on the plain tape; expected: dict(tape, pair or None, chain)"""
    out = [("predict_v0", "predict", dict(variant=0), None), ("predict_v2", "predict", dict(variant=2), None),
           ("predict_v1", "predict", dict(variant=1), None)]
    rollable = c["cov"][0] != "det290"
    if rollable:
        g = geometry(c)
        fwd = g["fwd"]
        step = {"small": 2, "fused": 1, "three": 3}
        out.append(("tape_default", "tape", {}, step[fwd]))
        if fwd == "small":
            out.append(("tape_no_small", "tape", dict(small=0), 1))
        if fwd != "three":
            out.append(("tape_three", "tape", dict(fused=0), 3))
    if rollable and c["U"] > 0:
        jac = c["D"] <= 14
        dev = lc.rev_chain_supported(c["E"], c["U"])
        pair = (5 if g["jsmall"] else 4) if jac else None
        out.append(("grad_default", "grad", {}, dict(tape=2 if jac else 1, pair=pair, chain=1 if dev else 2)))
        if dev:
            out.append(("grad_host_chain", "grad", dict(dev_chain=0), dict(tape=2 if jac else 1, pair=pair, chain=2)))
        if jac:
            out.append(("grad_plain_tape", "grad", dict(grad_mode=0), dict(tape=1, pair=None, chain=2)))
    return out


def route_classes(c):
    """The route classes a case witnesses: predict, small, fused, three, and for the gradient rollout's forward half sweep_small
    (small_sweep), sweep_bwd (bwd.hip), plain_tape."""
    cl = {"predict"}
    for name, kind, kw, exp in routes(c):
        if kind == "tape":
            cl.add({1: "fused", 2: "small", 3: "three"}[exp])
        elif kind == "grad":
            cl.add("plain_tape" if exp["tape"] == 1 else "sweep_small" if exp["pair"] == 5 else "sweep_bwd")
    return cl


def dims_of(c):
    """The dimensions of the table a case is a witness of."""
    g = geometry(c)
    t = {"cov:%s" % c["cov"][0] + ("" if c["cov"][0] not in ("spd", "corr") else ":%g" % c["cov"][1]), "ls:" + c["ls"], "var:" + c["var"],
         "mean:" + (c["mean"] if c["data"] == "std" else "big6"), "beta:" + c["beta"], "ik:" + c["ik"]}
    if "l2" in c["units"]:
        t.add("cov:l2:%g" % c["cov"][1])
    return t, {"N:%d" % c["N"], "D:%d" % c["D"], "E:%d" % c["E"], "KP:%d" % g["KP"], "vsep:%d" % int(g["vsep"]), "zerorow:%d" % int(c["U"] > 0)}


# every family dimension needs a witness on every route class; every shape dimension a witness at all
FAMILY_DIMS = (["cov:zero", "cov:rank1", "cov:zerorow", "cov:mixed", "cov:mixedcorr", "cov:negeig", "cov:corr:1e-06", "cov:corr:1e-12"] +
               ["cov:spd:%g" % v for v in (1e-16, 1e-8, 0.1, 1e3, 1e6, 1e12)] +
               ["ls:short", "ls:flat", "ls:ard", "ls:crossed", "ls:off", "var:tiny", "var:huge", "var:mixed",
                "mean:on", "mean:far30", "mean:straddle", "mean:below", "mean:big6",
                "beta:zero", "beta:zero0", "beta:x1e6", "beta:cancel", "ik:none", "ik:asym"])
PREDICT_DIMS = ["cov:l2:%g" % v for v in (1e-16, 1e-8, 0.1, 1e3, 1e6, 1e12)] + ["cov:det290"]
SHAPE_DIMS = ["N:24", "N:200", "N:256", "N:257", "D:3", "D:11", "D:4", "D:10", "D:14", "D:15", "D:18", "D:32", "E:1", "E:2", "E:3",
              "KP:8", "KP:12", "KP:16", "vsep:1", "vsep:0", "zerorow:1"]
ROUTE_CLASSES = ("predict", "small", "fused", "three")
GRAD_ROUTE_CLASSES = ("sweep_small", "sweep_bwd", "plain_tape")
# what the value-and-gradient rollout's forward half must have seen (it needs a controller: the models with U > 0)
GRAD_DIMS = {"sweep_small": ("N:24", "N:200", "N:256", "KP:8", "KP:12", "KP:16", "vsep:1", "cov:mixed", "cov:corr:1e-06", "cov:spd:1000", "ls:ard", "ik:none"),
             "sweep_bwd": ("N:257", "cov:mixed", "cov:spd:1e+06", "mean:straddle", "ls:ard", "ik:none"),
             "plain_tape": ("D:15", "D:18", "D:32", "N:257", "cov:spd:1000")}


def missing(cases):
    """What the guard of tests/test_step_edges_cpu.py reports: the dimensions without a witness."""
    out = []
    have = {r: set() for r in ROUTE_CLASSES}
    shapes = {r: set() for r in ROUTE_CLASSES}
    for c in cases:
        fam, shp = dims_of(c)
        rc = route_classes(c)
        if not rc:
            out.append("%s has no route" % c["name"])
        for r in rc & set(ROUTE_CLASSES):
            have[r] |= fam
            shapes[r] |= shp
    for r in ROUTE_CLASSES:
        out += ["%s on %s" % (t, r) for t in FAMILY_DIMS if t not in have[r]]
    out += ["%s on predict" % t for t in PREDICT_DIMS if t not in have["predict"]]
    out += [t for t in SHAPE_DIMS if not any(t in shapes[r] for r in ROUTE_CLASSES)]
    # the shapes that reach a route must show it: the one-launch step at one chunk, at several and at its largest; the fused
    # head at N = 257 and with vsep; the three-kernel step at D = 18 and D = 32
    for r, ts in (("small", ("N:24", "N:200", "N:256", "KP:8", "KP:12", "KP:16", "vsep:1")), ("fused", ("N:257", "D:3", "D:15")),
                  ("three", ("D:18", "D:32"))):
        out += ["%s on %s" % (t, r) for t in ts if t not in shapes[r]]
    seen = {r: set() for r in GRAD_ROUTE_CLASSES}
    for c in cases:
        fam, shp = dims_of(c)
        for r in route_classes(c):
            if r in seen:
                seen[r] |= fam | shp
    for r in GRAD_ROUTE_CLASSES:
        out += ["%s on %s" % (t, r) for t in GRAD_DIMS[r] if t not in seen[r]]
    vs = [c for c in cases if geometry(c)["vsep"]]
    if not vs or len(vs) == len(cases):
        out.append("vsep and non-vsep witnesses")
    return out


# ------------------------------------------------------------------ blocks, K
def blocks_of(M, S, V):
    """The four blocks a K is taken over: M, S diagonal, S off-diagonal, V."""
    S = np.asarray(S)
    E = S.shape[0]
    off = ~np.eye(E, dtype=bool)
    return dict(M=np.ravel(M), Sd=np.diag(S).copy(), So=S[off], V=np.ravel(V))


def k_of(got, truth, unit):
    """max |got - truth| / unit; inf for a NaN or an infinity."""
    got, truth, unit = np.ravel(got), np.ravel(truth), np.ravel(unit)
    if got.size == 0:
        return 0.0
    if not np.all(np.isfinite(got)):
        return float("inf")
    return float(np.max(np.abs(got - truth) / unit))


def ks(M, S, V, fx):
    """K per block of a result against a case's fixture (fx: dict with M, S, V, uM, uS, uV)."""
    g = blocks_of(M, S, V)
    t = blocks_of(fx["M"], fx["S"], fx["V"])
    u = blocks_of(fx["uM"], fx["uS"], fx["uV"])
    return {b: k_of(g[b], t[b], u[b]) for b in BLOCKS}


# ------------------------------------------------------------------ the fixture's records
TRUTH_KEYS = ("M", "S", "V", "uM", "uS", "uV", "xr", "ldetB", "ldetR")


def truth_shapes(c):
    E, D = c["E"], c["D"]
    return dict(M=(1, E), S=(E, E), V=(D, E), uM=(1, E), uS=(E, E), uV=(D, E), xr=(E, 2), ldetB=(E,), ldetR=(E, E))


def pack_truth(c, t):
    return np.concatenate([np.asarray(t[k], np.float64).reshape(-1) for k in TRUTH_KEYS])


def unpack_truth(c, vec):
    out, o = {}, 0
    for k, shp in truth_shapes(c).items():
        n = int(np.prod(shp))
        out[k] = vec[o:o + n].reshape(shp)
        o += n
    assert o == vec.size, c["name"]
    return out
