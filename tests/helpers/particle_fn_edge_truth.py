"""40-digit (mpmath) truth, with a unit per entry, of the three blocks of the function-sample edge table
(helpers/particle_fn_edge_cases.py, docs/particle_fn_edges.md): the set-up V = iK (y - Phi(X) w - sqrt(noise) xi), the
teacher-forced value step x' = x + f(x~) and the step matrix A = I + df/dz as dreturn_dx0 shows it.  Built on the primitives of
oracle/mp_predict.py (object arrays of mpf; every operation in DPS digits from the float64 inputs, only the results rounded).

A model is the dict of helpers/particle_fn_restatement.py (X, Y, lengthscales, variance, noise); dr holds omega (E, L, D),
phase (E, L), w (P, E, L), xi (P, E, N); v (P, E, N) and iK (E, N, N) are float64 GIVENS: the device's own on the GPU, a
float64 restatement's on the CPU.  Units (derived in docs/particle_fn_edges.md from fn_step_body):
  set-up  2^-53 [ |iK| (|y| + |Phi||w| + sn |xi|) + |iK| (A |w| (sum_d |omega_ld X_id| + |b_l|)) ],  at least 2^-1022
  value   2^-53 [ sum_i |sf2 k_i v_i| (1 + q_i) + sum_l |A w_l cos(arg_l)| + sum_l |A w_l| (sum_d |omega_ld x~_d| + |b_l|) + |x'| ]
          (observation noise: + |x + f| + sn |eps|: the sum it is added to and the product it adds),  q_i = r_i^2 / 2
  matrix  2^-53 [ sum_i |sf2 k_i v_i (z_d - X_id) / l_d^2| (1 + q_i) + sum_l |A w_l sin(arg_l) omega_ld|
                  + sum_l |A w_l omega_ld| (sum_d |omega_ld z_d| + |b_l|) + |A_ed| + [e == d] |A_ed + 1| ]
          at least (N + L + 4) 2^-1074: a term in the denormal range carries an absolute rounding of 2^-1075 whatever its size."""
from __future__ import annotations

import mpmath as mp
import numpy as np

from oracle.mp_predict import DPS, EPS, TINY, _f, _o

_cos, _sin, _exp, _abs = (np.frompyfunc(f, 1, 1) for f in (mp.cos, mp.sin, mp.exp, abs))
QUANTUM = 2.0 ** -1074


def _arg(om_e, ph_e, pts):
    """arg (n, L) = pts . omega_l + b_l and sum_d |omega_ld pts_d| + |b_l| from object arrays."""
    return np.dot(pts, om_e.T) + ph_e[None, :], np.dot(_abs(pts), _abs(om_e).T) + _abs(ph_e)[None, :]


def setup(model, dr, iK, dps=DPS):
    """-> V (P, E, N) and its unit, float64."""
    mp.mp.dps = dps
    X, Y = _o(model["X"]), _o(model["Y"])
    P, E, L = np.asarray(dr["w"]).shape
    N = X.shape[0]
    V, U = np.empty((P, E, N), dtype=object), np.empty((P, E, N), dtype=object)
    for e in range(E):
        amp = mp.sqrt(2 * mp.mpf(float(model["variance"][e])) / L)
        sn = mp.sqrt(mp.mpf(float(model["noise"][e])))
        arg, mag = _arg(_o(dr["omega"][e]), _o(dr["phase"][e]), X)
        phi = amp * _cos(arg)
        w, xi, ik = _o(np.asarray(dr["w"])[:, e, :]), _o(np.asarray(dr["xi"])[:, e, :]), _o(iK[e])
        aw = _abs(w)
        R = Y[:, e][:, None] - np.dot(phi, w.T) - sn * xi.T
        M = _abs(Y[:, e])[:, None] + np.dot(_abs(phi), aw.T) + sn * _abs(xi).T + np.dot(amp * mag, aw.T)
        V[:, e, :] = np.dot(ik, R).T
        U[:, e, :] = np.dot(_abs(ik), M).T
    return _f(V), np.maximum(EPS * _f(U), TINY)


def step(model, dr, v, xt, eps=None, matrix=True, dps=DPS):
    """One step from x~ = xt (P, D) (the state is xt[:, :E]) with the given v.  -> dict of float64: xn (P, E) and its unit uxn;
    kern, feat (P, E): the two halves of f;  G (P, E, D) = A + I's first E columns (what dreturn_dx0 of an H = 2 call with the
    linear reward e_a shows of row a), its unit uG and Gk: the kernel half of A (matrix=False: those three are None)."""
    mp.mp.dps = dps
    X, xt_o = _o(model["X"]), _o(xt)
    P, E, L = np.asarray(dr["w"]).shape
    N, D = X.shape
    out = {k: np.empty((P, E), dtype=object) for k in ("xn", "uxn", "kern", "feat")}
    G, uG, Gk = (np.empty((P, E, D), dtype=object) for _ in range(3))
    diff = xt_o[:, None, :] - X[None, :, :]                          # (P, N, D)
    for e in range(E):
        ls = _o(model["lengthscales"][e])
        sf2 = mp.mpf(float(model["variance"][e]))
        amp = mp.sqrt(2 * sf2 / L)
        s = diff / ls[None, None, :]
        q = (s * s).sum(axis=2) / 2                                   # (P, N)
        kv = sf2 * _exp(-q) * _o(np.asarray(v)[:, e, :])
        om, w = _o(dr["omega"][e]), _o(np.asarray(dr["w"])[:, e, :])
        arg, mag = _arg(om, _o(dr["phase"][e]), xt_o)                  # (P, L)
        aw = amp * w
        t = aw * _cos(arg)
        out["kern"][:, e], out["feat"][:, e] = kv.sum(axis=1), t.sum(axis=1)
        f = out["kern"][:, e] + out["feat"][:, e]
        xn = xt_o[:, e] + f
        u = (_abs(kv) * (1 + q)).sum(axis=1) + _abs(t).sum(axis=1) + (_abs(aw) * mag).sum(axis=1)
        if eps is not None:
            add = mp.sqrt(mp.mpf(float(model["noise"][e]))) * _o(np.asarray(eps)[:, e])
            u = u + _abs(xn) + _abs(add)
            xn = xn + add
        out["xn"][:, e], out["uxn"][:, e] = xn, u + _abs(xn)
        if matrix:
            t2 = -(kv[:, :, None] * diff) / (ls * ls)[None, None, :]                 # (P, N, D)
            t1 = -(aw * _sin(arg))[:, :, None] * om[None, :, :]                      # (P, L, D)
            Gk[:, e, :] = t2.sum(axis=1)
            A = Gk[:, e, :] + t1.sum(axis=1)
            A[:, e] += 1
            uG[:, e, :] = ((_abs(t2) * (1 + q)[:, :, None]).sum(axis=1) + _abs(t1).sum(axis=1)
                           + ((_abs(aw) * mag)[:, :, None] * _abs(om)[None, :, :]).sum(axis=1) + _abs(A))
            A[:, e] += 1                      # the sweep adds the reward's gradient e_a
            uG[:, e, e] += _abs(A[:, e])
            G[:, e, :] = A
    res = {k: _f(a) for k, a in out.items()}
    res["uxn"] = np.maximum(EPS * res["uxn"], TINY)
    if matrix:
        res.update(G=_f(G), Gk=_f(Gk), uG=np.maximum(EPS * _f(uG), (N + L + 4) * QUANTUM))
    else:
        res.update(G=None, Gk=None, uG=None)
    return res
