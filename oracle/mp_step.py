"""One moment-matching step (pilco/models/mgpr.py:91-149) in 40-digit arithmetic from float64 inputs, with the units that the
edge-input tests of the step hold the device to (tests/helpers/step_cases.py, docs/step_edges.md).

TEST INFRASTRUCTURE ONLY.  oracle/mp_truth.moments_mp stays what the older fixtures were made with; this evaluator computes
the same formulas from caller-supplied factors (iK, beta as the device gets them, float64) and returns, next to M, S, V, the
sum of absolute terms behind every entry: the unit of |device - truth| <= K unit.

    M_a   2^-53 sum_i c_a |beta_i| l_i (1 + |x_i|)                      x_i = -iN_i B^-1 iN_i / 2 the exponent's argument
    V_da  the same sum with |t_id / l_d| inside it                      t_i = B^-1 iN_i
    S_ab  2^-53 [ sum_ij (|beta_i beta_j| + d_ab |iK_ij|) L_ij (1 + |u_i| + |v_j| + sum_d |p_id w_jd|) / sqrt(det R)
                  + |M_a M_b| + d_ab var_a ]
Each term carries the rounding of its own exponent, which the device assembles from parts of those magnitudes.  The device's
table exp returns e^-700 for anything smaller: every unit gets the additive floor e^-700 x its absolute weight sum; no unit
goes below 2^-1022.

Differences from moments_mp, none of which changes a value beyond 1e-35 (tests/test_step_edges_cpu.py):
- S_ab = S_ba: pairs a <= b only; on a diagonal pair L_ij = L_ji and the weight is symmetric (the C ABI stores the symmetric
  part of iK), so j >= i only, off-diagonal terms twice;
- the D x D inverses and determinants run with 30 more digits (R = s Lambda + I is not symmetric and at mixed scales its
  condition number eats 25 digits); the N^2 loops run at `dps`;
- a term whose exponent is below -3000 is skipped: with weights below 1e300 it is below 2^-1022 of any unit.
"""
from __future__ import annotations

import mpmath as mp
import numpy as np

DPS = 40
EPS = 2.0 ** -53
TINY = 2.0 ** -1022
CLAMP = -700.0
SKIP = -3000


def _mat(a, r, c):
    m = mp.matrix(r, c)
    for i in range(r):
        for j in range(c):
            m[i, j] = mp.mpf(float(a[i][j]))
    return m


def _inv_det(A, dps):
    mp.mp.dps = dps + 30
    try:
        inv, det = mp.inverse(A), mp.det(A)
    finally:
        mp.mp.dps = dps
    return inv, det


def sym_part(iK):
    """What the C ABI stores for a caller-supplied iK: 0.5 (iK + iK^T), entry by entry in float64."""
    iK = np.asarray(iK, np.float64)
    return 0.5 * (iK + np.swapaxes(iK, -1, -2))


def step_mp(X, lengthscales, variance, m, sm, iK, beta, dps=DPS, units=True):
    """m: list of D mpf, sm: mp.matrix (D, D); iK (E, N, N) float64 or None (all zero), beta (E, N) float64.
    -> dict of unrounded results: M [E], S {(a, b): mpf, a <= b}, V [E][D], detB [E], detR {(a, b)}, and float64 unit sums
    aM (E), aV (E, D), aS (E, E), floors fM, fV, fS (the e^-700 weight sums)."""
    mp.mp.dps = dps
    f = mp.mpf
    X = np.asarray(X, np.float64)
    ls = np.asarray(lengthscales, np.float64)
    N, D = X.shape
    E = ls.shape[0]
    beta = np.asarray(beta, np.float64)
    iKs = None if iK is None else sym_part(iK)
    zeta = [[f(float(X[i, d])) - m[d] for d in range(D)] for i in range(N)]
    lsm = [[f(float(ls[a, d])) for d in range(D)] for a in range(E)]
    var = [f(float(v)) for v in np.ravel(variance)]
    bet = [[f(float(beta[a, i])) for i in range(N)] for a in range(E)]
    M, V, kk, detB = [f(0)] * E, [[f(0)] * D for _ in range(E)], [], []
    aM, aV, fM, fV = np.zeros(E), np.zeros((E, D)), np.zeros(E), np.zeros((E, D))
    xr = np.zeros((E, 2))   # smallest and largest exponent of the mean sums, per output
    for a in range(E):
        la = lsm[a]
        B = mp.matrix(D, D)
        for i in range(D):
            for j in range(D):
                B[i, j] = sm[i, j] / (la[i] * la[j]) + (1 if i == j else 0)
        iB, dB = _inv_det(B, dps)
        detB.append(dB)
        c = var[a] / mp.sqrt(dB)
        iBl = [[iB[i, j] for j in range(D)] for i in range(D)]
        Ma, Va, ka = f(0), [f(0)] * D, []
        for i in range(N):
            iN = [zeta[i][d] / la[d] for d in range(D)]
            t = [mp.fsum(iBl[d][e] * iN[e] for e in range(D)) for d in range(D)]
            x = -mp.fsum(iN[d] * t[d] for d in range(D)) / 2
            xr[a] = (float(x), float(x)) if i == 0 else (min(xr[a, 0], float(x)), max(xr[a, 1], float(x)))
            lb = mp.exp(x) * bet[a][i] * c
            Ma += lb
            tl = [t[d] / la[d] for d in range(D)]
            for d in range(D):
                Va[d] += tl[d] * lb
            ka.append(mp.log(var[a]) - mp.fsum(v * v for v in iN) / 2)
            if units:
                w = float(abs(lb)) * (1.0 + float(abs(x)))
                aM[a] += w
                fl = float(abs(bet[a][i]) * c)
                fM[a] += fl
                for d in range(D):
                    aV[a, d] += w * float(abs(tl[d]))
                    fV[a, d] += fl * float(abs(tl[d]))
        M[a], V[a] = Ma, Va
        kk.append(ka)
    S, detR = {}, {}
    aS, fS = np.zeros((E, E)), np.zeros((E, E))
    for a in range(E):
        for b in range(a, E):
            Lam = [1 / lsm[a][d] ** 2 + 1 / lsm[b][d] ** 2 for d in range(D)]
            Rm = mp.matrix(D, D)
            for i in range(D):
                for j in range(D):
                    Rm[i, j] = sm[i, j] * Lam[j] + (1 if i == j else 0)
            iR, dR = _inv_det(Rm, dps)
            detR[(a, b)] = dR
            mp.mp.dps = dps + 30
            Qm = iR * sm / 2
            mp.mp.dps = dps
            Q = [[+Qm[i, j] for j in range(D)] for i in range(D)]
            za = [[zeta[i][d] / lsm[a][d] ** 2 for d in range(D)] for i in range(N)]
            wb = za if a == b else [[zeta[i][d] / lsm[b][d] ** 2 for d in range(D)] for i in range(N)]
            quad = lambda z: mp.fsum(z[d] * Q[d][e] * z[e] for d in range(D) for e in range(D))
            u = [kk[a][i] + quad(za[i]) for i in range(N)]
            v = u if a == b else [kk[b][j] + quad(wb[j]) for j in range(N)]
            # (z + w)^T Q (z + w) = z^T Q z + w^T Q w + z^T (Q + Q^T) w
            p = [[mp.fsum((Q[d][e] + Q[e][d]) * za[i][e] for e in range(D)) for d in range(D)] for i in range(N)]
            Lf = np.zeros((N, N))
            acc = f(0)
            bi, bj = bet[a], bet[b]
            ik = None if (a != b or iKs is None) else iKs[a]
            for i in range(N):
                pi, ui, row = p[i], u[i], f(0)
                for j in range(i if a == b else 0, N):
                    wj = wb[j]
                    e = ui + v[j]
                    for d in range(D):
                        e += pi[d] * wj[d]
                    if e < SKIP:
                        continue
                    L = mp.exp(e)
                    wgt = bi[i] * bj[j]
                    if ik is not None:
                        wgt -= f(float(ik[i, j]))
                    if a == b and j > i:
                        wgt *= 2
                        Lf[j, i] = float(L)
                    Lf[i, j] = float(L)
                    row += wgt * L
                acc += row
            isd = 1 / mp.sqrt(dR)
            S[(a, b)] = acc * isd - M[a] * M[b] + (var[a] if a == b else 0)
            if units:
                uf, vf = np.array([float(x) for x in u]), np.array([float(x) for x in v])
                pf = np.array([[float(x) for x in r] for r in p])
                wf = np.array([[float(x) for x in r] for r in wb])
                W = np.abs(np.outer(beta[a], beta[b]))
                if ik is not None:
                    W = W + np.abs(ik)
                cond = 1.0 + np.abs(uf)[:, None] + np.abs(vf)[None, :] + np.abs(pf) @ np.abs(wf).T
                fi = float(isd)
                aS[a, b] = aS[b, a] = float((W * Lf * cond).sum()) * fi + abs(float(M[a] * M[b])) + (float(var[a]) if a == b else 0.0)
                fS[a, b] = fS[b, a] = float(W.sum()) * fi
    return dict(M=M, S=S, V=V, detB=detB, detR=detR, aM=aM, aV=aV, aS=aS, fM=fM, fV=fV, fS=fS, xr=xr)


def _mp_inputs(m, s, D):
    f = mp.mpf
    return [f(float(x)) for x in np.ravel(m)], _mat(np.asarray(s, np.float64), D, D)


def units_of(r):
    """The units (float64 arrays shaped like M (1, E), S (E, E), V (D, E)) from step_mp's absolute sums."""
    fl = np.exp(CLAMP)
    uM = np.maximum(EPS * r["aM"] + fl * r["fM"], TINY)[None, :]
    uS = np.maximum(EPS * r["aS"] + fl * r["fS"], TINY)
    uV = np.maximum(EPS * r["aV"] + fl * r["fV"], TINY).T
    return uM, uS, uV


def step(X, lengthscales, variance, m, s, iK, beta, dps=DPS):
    """Float64 in, rounded once at the end: dict(M (1, E), S (E, E), V (D, E), uM, uS, uV the units, ldetB (E), ldetR (E, E)
    log10 of the determinants -- NaN where one is not positive)."""
    mp.mp.dps = dps
    X = np.asarray(X, np.float64)
    D = X.shape[1]
    E = np.asarray(lengthscales).shape[0]
    mm, sm = _mp_inputs(m, s, D)
    r = step_mp(X, lengthscales, variance, mm, sm, iK, beta, dps)
    S = np.zeros((E, E))
    ldR = np.zeros((E, E))
    l10 = lambda x: float(mp.log10(x)) if x > 0 else float("nan")
    for (a, b), val in r["S"].items():
        S[a, b] = S[b, a] = float(val)
        ldR[a, b] = ldR[b, a] = l10(r["detR"][(a, b)])
    uM, uS, uV = units_of(r)
    return dict(M=np.array([[float(x) for x in r["M"]]]), S=S, V=np.array([[float(r["V"][a][d]) for a in range(E)] for d in range(D)]),
                uM=uM, uS=uS, uV=uV, xr=r["xr"], ldetB=np.array([l10(x) for x in r["detB"]]), ldetR=ldR)


def gradient(X, lengthscales, variance, m, s, iK, beta, Mbar, Sbar, Vbar, dps=DPS, rel=1e-15):
    """d <Mbar, M> + <Sbar, S> + <Vbar, V> / d (m, s) by central differences in the same arithmetic (the convention of
    pilco_gp_predict_vjp: s_ij and s_ji move together, the result is symmetric and d/ds_ij carries half of the pair's
    derivative, as the symmetrised autograd gradient does).  Step: `rel` of the entry's scale."""
    mp.mp.dps = dps
    f = mp.mpf
    X = np.asarray(X, np.float64)
    D = X.shape[1]
    E = np.asarray(lengthscales).shape[0]
    Mb, Sb, Vb = np.asarray(Mbar, np.float64).ravel(), np.asarray(Sbar, np.float64), np.asarray(Vbar, np.float64)
    m0, s0 = _mp_inputs(m, s, D)

    def phi(mm, ss):
        r = step_mp(X, lengthscales, variance, mm, ss, iK, beta, dps, units=False)
        out = mp.fsum(f(float(Mb[a])) * r["M"][a] for a in range(E))
        out += mp.fsum(f(float(Sb[a, b])) * r["S"][(min(a, b), max(a, b))] for a in range(E) for b in range(E))
        out += mp.fsum(f(float(Vb[d, a])) * r["V"][a][d] for a in range(E) for d in range(D))
        return out

    sm_scale = max(float(np.abs(np.asarray(m)).max()), float(np.abs(X).max()), 1e-300)
    ss_scale = max(float(np.abs(np.asarray(s)).max()), float(np.min(np.asarray(lengthscales)) ** 2))
    gm, gs = np.zeros((1, D)), np.zeros((D, D))
    for d in range(D):
        h = f(rel) * f(sm_scale)
        up, dn = list(m0), list(m0)
        up[d] += h
        dn[d] -= h
        gm[0, d] = float((phi(up, s0) - phi(dn, s0)) / (2 * h))
    for i in range(D):
        for j in range(i, D):
            h = f(rel) * f(ss_scale)
            up, dn = s0.copy(), s0.copy()
            up[i, j] += h
            dn[i, j] -= h
            if j != i:
                up[j, i] += h
                dn[j, i] -= h
            g = float((phi(m0, up) - phi(m0, dn)) / (2 * h))
            gs[i, j] = gs[j, i] = g if i == j else g / 2
    return gm, gs
