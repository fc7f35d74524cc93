"""The yardsticks of the posterior's edge table (helpers/predict_cases.py, tests/golden/predict_edges.npz): the fixture's
records, two independent float64 restatements of GPR.predict_f / GPRFITC.predict_f and their input Jacobians, K_ref and the caps.

  (a) GPflow's order: Cholesky factors and triangular solves (helpers/predict_restatement.py, helpers/predict_jac_restatement.py)
  (b) the device's order: the kernel's scaled differences as k_gram forms them, (x - y) fl(1 / l) -- one more rounding than
      (x - y) / l, the same for every point, so that k is off by up to q eps, q = -log(k / sf2), coherently --, the Jacobians'
      weights (X - x) fl(1 / l^2), L^-1 by launch_trtri's recursive doubling on 64-blocks (helpers/trtri_doubling.py), then plain
      products -- beta = L^-T (L^-1 y), W = L^-1 k*, a = L^-T W; FITC: Luu^-1, G = sqrt(1 + nu' / sn2), Am = chol(V V^T + sn2 I),
      iAt = Am^-1 Luu^-1, beta = iAt^T Am^-1 V (y / G), var = sf2 - ||Luu^-1 k*||^2 + sn2 ||iAt k*||^2 (csrc/predict.hip)
K_ref of a case and block is the LARGER of the two against the 40-digit truth, in the truth's units; the device's cap per class
and block is 8 x the largest K_ref of the class, at least 4.  (b) takes mutants for the sensitivity test."""
import os

import numpy as np

from helpers import predict_cases as pc
from helpers import predict_jac_restatement as jr
from helpers.trtri_doubling import padded_inverse

PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "predict_edges.npz")
CAP_FACTOR, CAP_FLOOR = 8.0, 4.0
MUTANTS = ("ls_swap", "noise_swap", "no_jitter", "iat_sign", "no_2", "flip", "ls_pow", "n_minus_1", "flush")
_FX = None
_CASE = {}
_KREF = {}


def get(key):
    global _FX
    if _FX is None:
        _FX = dict(np.load(PATH))
    return _FX[key]


def case(c):
    """(d, truths): the case's data with its test points `xs` and declared zeros `zeros`; truths: {"t" | "ts", "to": record}."""
    if c["name"] not in _CASE:
        base = {k: get("_data/%s/%s" % (c["data"], k)) for k in (("X", "Y", "Z") if c["M"] else ("X", "Y"))}
        d = pc.make_data(c, base)
        d["xs"] = get(c["name"] + "/xs")
        d["zeros"] = get(c["name"] + "/zeros").astype(bool)
        _CASE[c["name"]] = (d, {tn: pc.unpack_truth(c, get(c["name"] + "/" + tn)) for tn in pc.truth_names(c)})
    return _CASE[c["name"]]


def z_of(d, tn):
    """The inducing inputs of a truth: (M, D) shared, (E, M, D) own, None for the exact GP."""
    return None if tn == "t" else d["Z"][0] if tn == "ts" else d["Z"]


def se_device(A, B, ls, var):
    """k_gram's order: the difference times the rounded reciprocal lengthscale."""
    dd = (A[:, None, :] - B[None, :, :]) * (1.0 / np.asarray(ls, np.float64))
    return float(var) * np.exp(-0.5 * np.sum(dd * dd, axis=-1))


def restate_a(d, tn):
    """(mean, var (E, Nt), dmean, dvar (E, Nt, D)) in GPflow's order."""
    if tn == "t":
        return jr.gpr_predict_f_jac(d["X"], d["Y"], d["ls"], d["var"], d["noise"], d["xs"])
    return jr.fitc_predict_f_jac(d["X"], d["Y"], z_of(d, tn), d["ls"], d["var"], d["noise"], d["xs"])


def restate_b(d, tn, mutant=None):
    """The same in the device's order; mutant: one of MUTANTS."""
    X, Y, xs = d["X"], d["Y"], d["xs"]
    E, Nt, D = Y.shape[1], xs.shape[0], X.shape[1]
    if mutant == "n_minus_1" and tn == "t":
        X, Y = X[:-1], Y[:-1]
    mean, var = np.empty((E, Nt)), np.empty((E, Nt))
    dmean, dvar = np.empty((E, Nt, D)), np.empty((E, Nt, D))
    for e in range(E):
        o = (e + 1) % E
        ls = d["ls"][o if mutant == "ls_swap" else e]
        sf2, sn2 = d["var"][e], d["noise"][o if mutant == "noise_swap" else e]
        if tn == "t":
            P = X
            L = np.linalg.cholesky(se_device(X, X, ls, sf2) + sn2 * np.eye(len(X)))
            ops = [(padded_inverse(L), 1.0)]
            beta = ops[0][0].T @ (ops[0][0] @ Y[:, e])
        else:
            Z = d["Z"][0] if tn == "ts" else d["Z"][e]
            P = Z[:-1] if mutant == "n_minus_1" else Z
            M = len(P)
            Lui = padded_inverse(np.linalg.cholesky(se_device(P, P, ls, sf2) + (0.0 if mutant == "no_jitter" else pc.JITTER) * np.eye(M)))
            V = Lui @ se_device(P, X, ls, sf2)
            G = np.sqrt(1.0 + (sf2 - np.sum(V * V, axis=0)) / sn2)
            V = V / G
            Ami = padded_inverse(np.linalg.cholesky(V @ V.T + sn2 * np.eye(M)))
            iAt = Ami @ Lui
            beta = iAt.T @ (Ami @ (V @ (Y[:, e] / G)))
            ops = [(Lui, 1.0), (iAt, -sn2)]
        k = se_device(P, xs, ls, sf2)
        if mutant == "flush":
            k = np.where(np.abs(k) < pc.TINY, 0.0, k)
        mean[e] = k.T @ beta
        v = np.full(Nt, sf2)
        a = np.zeros_like(k)
        for op, sc in ops:
            W = op @ k
            v = v - (-sc if mutant == "iat_sign" else sc) * np.sum(W * W, axis=0)
            a = a + sc * (op.T @ W)
        var[e] = v
        w = (-1.0 if mutant == "flip" else 1.0) * (P[:, None, :] - xs[None, :, :]) * (1.0 / (ls if mutant == "ls_pow" else ls * ls))
        dmean[e] = np.einsum("i,it,itd->td", beta, k, w)
        dvar[e] = -(1.0 if mutant == "no_2" else 2.0) * np.einsum("it,it,itd->td", a, k, w)
    return mean, var, dmean, dvar


def _worst(c, fn):
    d, truths = case(c)
    out = {b: 0.0 for b in pc.BLOCKS}
    for tn, fx in truths.items():
        k = pc.ks(fn(d, tn), fx)
        out = {b: max(out[b], k[b]) for b in pc.BLOCKS}
    return out


def k_ref_a(c):
    return _worst(c, restate_a)


def k_ref_b(c):
    return _worst(c, restate_b)


def k_ref(c):
    """K_ref per block: the larger of the two restatements, over the case's truths."""
    if c["name"] not in _KREF:
        a, b = k_ref_a(c), k_ref_b(c)
        _KREF[c["name"]] = ({k: max(a[k], b[k]) for k in pc.BLOCKS}, a, b)
    return _KREF[c["name"]][0]


def compute_caps(cases=None):
    caps = {}
    for c in (pc.CASES if cases is None else cases):
        k = k_ref(c)
        for b in pc.BLOCKS:
            caps[(c["cls"], b)] = max(caps.get((c["cls"], b), CAP_FLOOR), CAP_FACTOR * k[b])
    return caps


def stored_caps():
    return {tuple(k.split("|")): float(v) for k, v in zip(get("_caps_keys"), get("_caps"))}


def cap_of(c, b):
    return stored_caps()[(c["cls"], b)]
