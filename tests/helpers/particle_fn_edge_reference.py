"""The yardstick of the function-sample edge table (helpers/particle_fn_edge_cases.py): two float64 restatements of the
set-up, the value step and the step matrix, their K_ref against the 40-digit truth of helpers/particle_fn_edge_truth.py, the
caps (8 x the larger K_ref of a class and block, at least 4) and the mutants of restatement (b).  docs/particle_fn_edges.md.

  (a)  helpers/particle_fn_restatement.py / particle_fn_grad_restatement.py in plain NumPy order with every sum in float64
  (b)  the device's order (fn_step_body, csrc/particles_fn.h): (x - X) fl(1 / l), one fused square-accumulate per dimension,
       eight wave sums over the index shares 8 w .. 8 w + 7 of every tile of 64 combined in wave order, f = fma(A, F, sf2 K);
       the Jacobian sums and A[e][d] = [e == d] + fma(-(sf2 il^2), JK, -(A JF)) likewise.  A fused multiply-add is formed in
       np.longdouble and rounded once more (within 2^-11 ulp of the fused result).
In both, v comes from a float64 iK (Cholesky of the float64 Gram matrix); the truth is evaluated on the same v."""
from __future__ import annotations

import numpy as np

from helpers import particle_fn_edge_cases as ec
from helpers import particle_fn_edge_truth as et
from helpers import particles_restatement as pr
from helpers.predict_restatement import se_ard

LD = np.longdouble
TINY = 2.0 ** -1022
MUTANTS = ("ls_swap", "omega_next", "no_phase", "no_sf2", "amp_Lpad", "drop_point", "drop_feature", "flush", "A_ls1", "A_flip",
           "A_nodelta")


def fma(a, b, c):
    return (np.asarray(a, LD) * np.asarray(b, LD) + np.asarray(c, LD)).astype(np.float64)


def ik64(model):
    """iK (E, N, N) from the float64 Cholesky factor (raises numpy.linalg.LinAlgError where it fails)."""
    X = np.asarray(model["X"], np.float64)
    out = []
    for e in range(np.asarray(model["Y"]).shape[1]):
        K = se_ard(X, X, model["lengthscales"][e], model["variance"][e]) + model["noise"][e] * np.eye(X.shape[0])
        Li = np.linalg.inv(np.linalg.cholesky(K))
        out.append(Li.T @ Li)
    return np.stack(out)


def xt_of(policy, x0):
    return np.concatenate([x0, pr.action(policy, x0)], axis=1)


# ------------------------------------------------------------------ (a): plain NumPy order
def setup_a(model, dr, iK):
    X, Y = np.asarray(model["X"], np.float64), np.asarray(model["Y"], np.float64)
    P, E, L = dr["w"].shape
    V = np.empty((P, E, X.shape[0]))
    for e in range(E):
        phi = np.sqrt(2.0 * model["variance"][e] / L) * np.cos(X @ dr["omega"][e].T + dr["phase"][e][None, :])
        R = Y[:, e][:, None] - phi @ dr["w"][:, e, :].T - np.sqrt(model["noise"][e]) * dr["xi"][:, e, :].T
        V[:, e, :] = (iK[e] @ R).T
    return V


def step_a(model, dr, v, xt, eps=None, matrix=True):
    X = np.asarray(model["X"], np.float64)
    P, E, L = dr["w"].shape
    D = X.shape[1]
    xn, G = np.empty((P, E)), np.empty((P, E, D))
    diff = xt[:, None, :] - X[None, :, :]
    for e in range(E):
        ls, sf2 = np.asarray(model["lengthscales"][e], np.float64), float(model["variance"][e])
        d = diff / ls
        k = sf2 * np.exp(-0.5 * np.sum(d * d, axis=2))
        amp = np.sqrt(2.0 * sf2 / L)
        arg = xt @ dr["omega"][e].T + dr["phase"][e][None, :]
        w = dr["w"][:, e, :]
        f = (w * (amp * np.cos(arg))).sum(axis=1) + (k * v[:, e, :]).sum(axis=1)
        xn[:, e] = xt[:, e] + f
        if eps is not None:
            xn[:, e] += np.sqrt(model["noise"][e]) * eps[:, e]
        if matrix:
            t1 = (-amp * w * np.sin(arg))[:, :, None] * dr["omega"][e][None, :, :]
            t2 = -(k * v[:, e, :])[:, :, None] * diff / (ls ** 2)[None, None, :]
            A = t1.sum(axis=1) + t2.sum(axis=1)
            A[:, e] += 1.0
            A[:, e] += 1.0          # the sweep adds the reward's gradient e_a
            G[:, e, :] = A
    return xn, (G if matrix else None)


# ------------------------------------------------------------------ (b): the device's order, and its mutants
def setup_b(model, dr, iK):
    X, Y = np.asarray(model["X"], np.float64), np.asarray(model["Y"], np.float64)
    P, E, L = dr["w"].shape
    N, D = X.shape
    V = np.empty((P, E, N))
    for e in range(E):
        arg = np.tile(dr["phase"][e][None, :], (N, 1))
        for d in range(D):
            arg = fma(dr["omega"][e][None, :, d], X[:, d][:, None], arg)
        phi = np.sqrt(2.0 * model["variance"][e] / L) * np.cos(arg)               # (N, L)
        S = np.zeros((N, P))
        for l in range(L):
            S = S + phi[:, l][:, None] * dr["w"][:, e, l][None, :]
        R = (Y[:, e][:, None] - S) - np.sqrt(model["noise"][e]) * dr["xi"][:, e, :].T
        Vv = np.zeros((N, P))
        for j in range(N):
            Vv = Vv + iK[e][:, j][:, None] * R[j][None, :]
        V[:, e, :] = Vv.T
    return V


def _waves(parts):
    s = parts[0]
    for q in range(1, 8):
        s = s + parts[q]
    return s


def step_b(model, dr, v, xt, eps=None, matrix=True, mut=None):
    """-> xn (P, E), G (P, E, D) or None.  Arrays are (E, P) inside: every output at once."""
    X = np.asarray(model["X"], np.float64)
    ls, sf2 = np.asarray(model["lengthscales"], np.float64), np.asarray(model["variance"], np.float64)
    P, E, L = dr["w"].shape
    N, D = X.shape
    om, ph = dr["omega"], dr["phase"]
    if mut == "omega_next":
        om = np.roll(om, -1, axis=1)
    if mut == "no_phase":
        ph = np.zeros_like(ph)
    il = 1.0 / ls                                               # (E, D)
    ilv = np.roll(il, -1, axis=0) if mut == "ls_swap" else il   # the value's lengthscales
    Ne = N - 1 if mut == "drop_point" else N
    Le = L - 1 if mut == "drop_feature" else L
    sK, sF = np.zeros((8, E, P)), np.zeros((8, E, P))
    J = np.zeros((8, E, P, D))
    for i in range(Ne):
        wv = (i % 64) // 8
        r2 = np.zeros((E, P))
        for d in range(D):
            s = (xt[:, d] - X[i, d])[None, :] * ilv[:, d][:, None]
            r2 = fma(s, s, r2)
        ek = np.exp(-0.5 * r2)
        if mut == "flush":
            ek = np.where(ek < TINY, 0.0, ek)
        vi = v[:, :, i].T
        sK[wv] = fma(ek, vi, sK[wv])
        if matrix:
            g = ek * vi
            for d in range(D):
                dz = xt[:, d] - X[i, d]
                J[wv, :, :, d] = fma(g, (-dz if mut == "A_flip" else dz)[None, :], J[wv, :, :, d])
    K = _waves(sK)
    JK = _waves(J) if matrix else None
    J = np.zeros((8, E, P, D))
    for l in range(Le):
        wv = (l % 64) // 8
        arg = np.tile(ph[:, l][:, None], (1, P))
        for d in range(D):
            arg = fma(om[:, l, d][:, None], xt[:, d][None, :], arg)
        wl = dr["w"][:, :, l].T
        sF[wv] = fma(wl, np.cos(arg), sF[wv])
        if matrix:
            g = wl * np.sin(arg)
            for d in range(D):
                J[wv, :, :, d] = fma(g, om[:, l, d][:, None], J[wv, :, :, d])
    F = _waves(sF)
    amp = np.sqrt(2.0 * sf2 / float((L + 63) // 64 * 64 if mut == "amp_Lpad" else L))
    kh = K if mut == "no_sf2" else sf2[:, None] * K
    f = fma(amp[:, None], F, kh)
    xe = xt[:, :E].T + f
    if eps is not None:
        xe = xe + np.sqrt(np.maximum(np.asarray(model["noise"], np.float64), 0.0))[:, None] * eps.T
    if not matrix:
        return xe.T.copy(), None
    JF = _waves(J)
    sc = il if mut == "A_ls1" else il * il
    sc = sc if mut == "no_sf2" else sf2[:, None] * sc
    df = fma(-sc[:, None, :], JK, -(amp[:, None, None] * JF))            # (E, P, D)
    delta = np.eye(E, D)[:, None, :]
    A = df if mut == "A_nodelta" else delta + df
    return xe.T.copy(), (A + delta).transpose(1, 0, 2).copy()


# ------------------------------------------------------------------ K_ref and the caps
_REF = {}


def reference(c):
    """The CPU side of a case, computed once: dict(iK, v, xt, setup=(V, unit), truth=step truth on v) -- v: restatement (a)'s."""
    if c["name"] not in _REF:
        d = ec.case(c)
        model, dr = d["model"], d["draws"]
        iK = ik64(model)
        v = setup_a(model, dr, iK)
        xt = xt_of(d["policy"], d["x0"])
        eps = None if d["eps"] is None else d["eps"][0]
        r = dict(iK=iK, v=v, xt=xt, eps=eps, setup=et.setup(model, dr, iK) if "setup" in c["blocks"] else None,
                 truth=et.step(model, dr, v, xt, eps=eps, matrix="matrix" in c["blocks"]))
        _REF[c["name"]] = r
    return _REF[c["name"]]


def ks_of(c, V, xn, G):
    """K per block of a case's results against its CPU reference (None: the block is not compared)."""
    r = reference(c)
    out = {}
    if "setup" in c["blocks"] and V is not None:
        out["setup"] = ec.k_of(V, *r["setup"])
    if xn is not None:
        out["value"] = ec.k_of(xn, r["truth"]["xn"], r["truth"]["uxn"])
    if "matrix" in c["blocks"] and G is not None:
        E = c["E"]
        out["matrix"] = ec.k_of(G[:, :, :E], r["truth"]["G"][:, :, :E], r["truth"]["uG"][:, :, :E])
    return out


def k_ref(c):
    """{"a": {block: K}, "b": {block: K}} of a case."""
    d = ec.case(c)
    r = reference(c)
    m = "matrix" in c["blocks"]
    s = "setup" in c["blocks"]
    args = (d["model"], d["draws"], r["v"], r["xt"])
    return {"a": ks_of(c, r["v"] if s else None, *step_a(*args, eps=r["eps"], matrix=m)),
            "b": ks_of(c, setup_b(d["model"], d["draws"], r["iK"]) if s else None, *step_b(*args, eps=r["eps"], matrix=m))}


def mutant_ks(c, mut):
    d = ec.case(c)
    r = reference(c)
    return ks_of(c, None, *step_b(d["model"], d["draws"], r["v"], r["xt"], eps=r["eps"], matrix="matrix" in c["blocks"], mut=mut))


def compute_caps(cases=None):
    caps = {}
    for c in (ec.CASES if cases is None else cases):
        k = k_ref(c)
        for b in c["blocks"]:
            key = (c["cls"], b)
            caps[key] = max(caps.get(key, 4.0), 8.0 * max(k["a"][b], k["b"][b]))
    return caps


def cap_of(c, block):
    fx = ec.fixture()
    return float(fx["_caps"][list(fx["_caps_keys"]).index("%s|%s" % (c["cls"], block))])


# ------------------------------------------------------------------ the conditions on the inputs
def conditions(c):
    """What the table asks of a case's inputs and truth (asserted by the generator, re-checked by the CPU suite on the stored
    fixture): finite particles, draws and truth; the float64 Cholesky of the restatements succeeds (reference() raises where it
    does not); the declared exact results are exact in the truth; the denormal particle sees a denormal and a zero k.
    -> the list of what fails."""
    from helpers import predict_cases as pc
    d = ec.case(c)
    r = reference(c)
    bad = []
    if not (np.all(np.isfinite(d["x0"])) and all(np.all(np.isfinite(a)) for a in d["draws"].values())):
        bad.append("an x0 row or a draw is not finite")
    t = r["truth"]
    arrays = [t["xn"], t["uxn"]] + ([t["G"], t["uG"]] if t["G"] is not None else []) + (list(r["setup"]) if r["setup"] else [])
    if not all(np.all(np.isfinite(a)) for a in arrays) or not np.all(np.isfinite(r["v"])):
        bad.append("a truth value is not finite")
    far, zero_out = ec.declared(c)
    if far is not None:
        if np.any(t["kern"][far] != 0.0) or (t["Gk"] is not None and np.any(t["Gk"][far] != 0.0)):
            bad.append("a kernel value at the far particle is not exactly 0")
    if zero_out:
        E = c["E"]
        if np.any(r["setup"][0][:, 0, :] != 0.0) or np.any(t["xn"][:, 0] != d["x0"][:, 0]) or np.any(t["G"][:, 0, :E] != 2.0 * np.eye(E)[0]):
            bad.append("output 0 of y = 0 is not exactly zero")
    if c["kind"] == "table" and not c["policy"]:
        i = pc.POINT_KINDS.index("denorm")
        k = se_ard(np.asarray(d["model"]["X"], np.float64), d["x0"][i:i + 1], d["model"]["lengthscales"][0], d["model"]["variance"][0])
        if not (np.any((k > 0) & (k < TINY)) and np.any(k == 0.0)):
            bad.append("the denormal particle has no denormal or no zero k")
    return bad
