"""The fixture of the step's edge cases (tests/golden/step_edges.npz), the float64 restatement's own K against it (K_ref), the caps
of the device's K, and a restatement of the step with one switch per mutant (tests/test_step_edges_cpu.py's sensitivity test).
No mpmath here: the GPU test imports this module."""
from __future__ import annotations

import os

import numpy as np

from helpers import step_cases as sc
from oracle import tf_path as tp

PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "step_edges.npz")
_FX = None
_CASE = {}


def raw():
    global _FX
    if _FX is None:
        with np.load(PATH) as z:
            _FX = {k: z[k] for k in z.files}
    return _FX


def get(key):
    return raw()[key]


def case(c):
    """(data, fixture) of a case: make_data with the factors as the device gets them (iK, beta) and as the truth saw them
    (iKt: the symmetric part), and the truth's arrays M, S, V, uM, uS, uV, ldetB, ldetR (gm, gs)."""
    if c["name"] not in _CASE:
        d = sc.make_data(c)
        d["iK"], d["beta"], d["iKt"] = sc.factors_from(c, get)
        fx = sc.unpack_truth(c, get(c["name"] + "/t"))
        if c["grad"]:
            D = c["D"]
            g = get(c["name"] + "/g")
            fx.update(gm=g[:D].reshape(1, D), gs=g[D:].reshape(D, D))
        _CASE[c["name"]] = (d, fx)
    return _CASE[c["name"]]


def restatement(d):
    """oracle.tf_path on the case's inputs, with the factors the truth saw."""
    E, N = d["beta"].shape
    iK = np.zeros((E, N, N)) if d["iKt"] is None else d["iKt"]
    with np.errstate(all="ignore"):
        return tp.predict_given_factorizations(d["X"], d["ls"], d["var"], d["m"], d["s"], iK, d["beta"])


def k_ref(c):
    """K of oracle.tf_path against the truth, per block."""
    d, fx = case(c)
    return sc.ks(*restatement(d), fx)


def k_ref_device_order(c):
    """K of the second, device-ordered restatement (mutable_step(device_order=True))."""
    d, fx = case(c)
    return sc.ks(*mutable_step(d, device_order=True), fx)


def k_ref_smaller(c):
    a, b = k_ref(c), k_ref_device_order(c)
    return {blk: min(a[blk], b[blk]) for blk in sc.BLOCKS}


def compute_caps(cases=None):
    """{(class, block): 8 x the largest K_ref of the class, floor 4}; K_ref of a case and block is the smaller of the two
    restatements' (oracle.tf_path and the device-ordered one)."""
    worst = {}
    for c in (sc.CASES if cases is None else cases):
        for b, k in k_ref_smaller(c).items():
            worst[(c["cls"], b)] = max(worst.get((c["cls"], b), 0.0), k)
    return {key: max(4.0, 8.0 * k) for key, k in worst.items()}


def cap_of(c, block):
    return float(stored_caps()[(c["cls"], block)])


def stored_caps():
    """{(class, block): cap} as the generator stored them."""
    return {tuple(k.split("|")): float(v) for k, v in zip(get("_caps_keys"), get("_caps"))}


# ------------------------------------------------------------------ a restatement with switches (pairs form of mgpr.py:91-149)
MUTANTS = ("lb_for_la", "no_iK", "half_offdiag", "R_noI", "no_logvar", "T_noLam", "no_v", "clamp600", "detB_for_detR")


def gj_unpivoted(A, B):
    """(A^-1 B, det A) by the Gauss-Jordan of csrc/mm_device.h gj_wave in float64: no pivoting, the pivot row scaled by the
    pivot's reciprocal, the determinant the running product of the pivots (numpy has no fma: two roundings where the device has one)."""
    n = A.shape[0]
    G = np.concatenate([np.array(A, np.float64), np.array(B, np.float64)], axis=1)
    det = 1.0
    for k in range(n):
        piv = G[k, k]
        det *= piv
        pk = G[k] * (1.0 / piv)
        f = G[:, k].copy()
        G -= np.outer(f, pk)
        G[k] = pk
    return G[:, n:], det


def mutable_step(d, mutant=None, device_order=False):
    """oracle.tf_path.predict_given_factorizations_pairs with every pair evaluated (no mirror), and one wrong thing switched on.
    device_order: the second, device-ordered restatement -- T = (s + Lambda^2)^-1 and Q = R^-1 s / 2 by the unpivoted
    Gauss-Jordan and the determinants as pivot products, as the operand kernel forms them (csrc/prep_device.h)."""
    X, ls, var, m, s, beta = d["X"], d["ls"], d["var"], np.reshape(d["m"], (1, -1)), d["s"], d["beta"]
    E, D = ls.shape
    N = X.shape[0]
    iK = np.zeros((E, N, N)) if d["iKt"] is None else d["iKt"]
    ex = (lambda x: np.exp(np.maximum(x, -600.0))) if mutant == "clamp600" else np.exp
    zeta = X - m
    M, V, k, detB = np.empty(E), np.empty((E, D)), np.empty((E, N)), np.empty(E)
    with np.errstate(all="ignore"):
        for a in range(E):
            iL = np.diag(1.0 / ls[a])
            iN = zeta @ iL
            B = iL @ s @ iL + np.eye(D)
            if device_order:
                iB, detB[a] = gj_unpivoted(B, np.eye(D))
                t = iN @ iB
            else:
                t = np.linalg.solve(B.T, iN.T).T
                detB[a] = np.linalg.det(B)
            lb = ex(-0.5 * np.sum(iN * t, 1)) * beta[a]
            c = var[a] / np.sqrt(detB[a])
            M[a] = lb.sum() * c
            V[a] = (t if mutant == "T_noLam" else t @ iL).T @ lb * c
            k[a] = (0.0 if mutant == "no_logvar" else np.log(var[a])) - 0.5 * np.sum(iN * iN, 1)
        S = np.zeros((E, E))
        for a in range(E):
            for b in range(E):
                za = zeta / np.square(ls[b] if mutant == "lb_for_la" else ls[a])
                wb = -zeta / np.square(ls[b])
                R = s @ np.diag(1.0 / np.square(ls[a]) + 1.0 / np.square(ls[b])) + (0.0 if mutant == "R_noI" else np.eye(D))
                if device_order:
                    Q, detR = gj_unpivoted(R, s)
                    Q = Q / 2.0
                else:
                    Q, detR = np.linalg.solve(R, s) / 2.0, np.linalg.det(R)
                zQ = za @ Q
                vj = 0.0 if mutant == "no_v" else (k[b] + np.sum(wb @ Q * wb, 1))[None, :]
                L = ex(k[a][:, None] + np.sum(zQ * za, 1)[:, None] + vj - 2.0 * zQ @ wb.T)
                Wt = np.outer(beta[a], beta[b])
                if a == b and mutant != "no_iK":
                    Wt = Wt - iK[a]
                if a == b and mutant == "half_offdiag":
                    Wt = np.triu(Wt)
                val = np.sum(Wt * L)
                S[a, b] = val / np.sqrt(detB[a] if mutant == "detB_for_detR" else detR)
        S = S + np.diag(var) - np.outer(M, M)
    return M[None, :].copy(), S, V.T.copy()


# ------------------------------------------------------------------ gradients
def autograd_gradient(d):
    """d <Mbar, M> + <Sbar, S> + <Vbar, V> / d (m, s) by torch autograd through oracle.torch_path (the convention of
    test_moment_matching_vjp_vs_autograd: the gradient with respect to s symmetrised)."""
    import torch
    from oracle import torch_path as tq
    E, N = d["beta"].shape
    iK = np.zeros((E, N, N)) if d["iKt"] is None else d["iKt"]
    mt = torch.tensor(d["m"], dtype=torch.float64, requires_grad=True)
    st = torch.tensor(d["s"], dtype=torch.float64, requires_grad=True)
    M, S, V = tq.predict_given_factorizations(d["X"], d["ls"], d["var"], mt, st, iK, d["beta"])
    ((torch.tensor(d["Mbar"]) * M).sum() + (torch.tensor(d["Sbar"]) * S).sum() + (torch.tensor(d["Vbar"]) * V).sum()).backward()
    gs = st.grad.numpy()
    return mt.grad.numpy().reshape(1, -1), 0.5 * (gs + gs.T)


def block_error(got, ref):
    got, ref = np.ravel(got), np.ravel(ref)
    if not np.all(np.isfinite(got)):
        return float("inf")
    scale = np.abs(ref).max()
    return float(np.abs(got - ref).max() / (scale if scale > 0 else 1.0))


def grad_tol(c):
    """max(TOL_GRAD, 8 x the error of autograd through oracle.torch_path against the 40-digit gradient), per block (m, s)."""
    d, fx = case(c)
    gm, gs = autograd_gradient(d)
    return (max(sc.TOL_GRAD, 8.0 * block_error(gm, fx["gm"])), max(sc.TOL_GRAD, 8.0 * block_error(gs, fx["gs"])))


# ------------------------------------------------------------------ the state after the step (value-and-gradient rollouts)
def state1(c, d, fx):
    """The state after one step from the truth's (M, S, V): m1 = m0 + M, S1 = S + S0 + s1 V + (s1 V)^T with s1 the states' rows
    of the joint covariance (pilco.py:151-152), combined in float64, and its units: the step's own units carried through the
    combination plus the combination's roundings (one per addition; D + 1 per entry of the product s1 V).
    -> (m1 (E), S1 (E, E), unit of m1, unit of S1)."""
    E, D = c["E"], c["D"]
    s1 = d["s"][:E, :]
    M, S, V = fx["M"].ravel(), fx["S"], fx["V"]
    C = s1 @ V
    m1 = d["m0"].ravel() + M
    S1 = S + d["S0"] + C + C.T
    aC = np.abs(s1) @ np.abs(V)
    um = fx["uM"].ravel() + 2 * sc.EPS * (np.abs(d["m0"].ravel()) + np.abs(M))
    uC = np.abs(s1) @ fx["uV"] + (D + 1) * sc.EPS * aC
    uS = fx["uS"] + uC + uC.T + 4 * sc.EPS * (np.abs(S) + np.abs(d["S0"]) + aC + aC.T)
    return m1, S1, np.maximum(um, sc.TINY), np.maximum(uS, sc.TINY)


def state1_caps(c):
    """The caps of the state's K: the mean under M's; the covariance under the largest of the blocks it is made of."""
    return cap_of(c, "M"), max(cap_of(c, "Sd"), cap_of(c, "So"), cap_of(c, "V"))


def sweep_horizon(c, d, fx):
    """The horizon of the value-and-gradient rollout of a case: 2, so that the reward sees the produced state -- or 1 where that
    state is no covariance.  (The large models' iK = diag(d) - g g^T is the device's input to the bit, not a consistent inverse:
    with a small input covariance the step's S is negative there, e.g. -1.6e3 for n200_std.  The step under test is step 0
    either way; a second step from an indefinite covariance would test nothing.)"""
    _, S1, _, _ = state1(c, d, fx)
    return 2 if np.linalg.eigvalsh(0.5 * (S1 + S1.T)).min() > 0 else 1


def reward_ref(c, d, fx, H):
    """The reward of the H-step rollout with ExponentialReward(W = I, t = 0): of state 0 and, for H = 2, of the truth's state 1
    (float64 restatement; tests/test_step_edges_cpu.py holds it to the 50-digit evaluation of oracle/mp_link at these states)."""
    m1, S1, _, _ = state1(c, d, fx)
    with np.errstate(all="ignore"):
        r = float(tp.exponential_reward(d["m0"], d["S0"])[0][0, 0])
        if H == 2:
            r += float(tp.exponential_reward(m1[None, :], S1)[0][0, 0])
    return r


# ------------------------------------------------------------------ policy gradients through the step (step_cases.WGRAD_CASES)
def wgrad_case(c):
    """(data with the factors, truth dict(R, dW, db)) of a policy-gradient case."""
    d = sc.make_data(c)
    d["iK"], d["beta"], d["iKt"] = sc.factors_from(c, get)
    g = get(c["name"] + "/wg")
    U, E = c["U"], c["E"]
    return d, dict(R=float(g[0]), dW=g[1:1 + U * E].reshape(U, E), db=g[1 + U * E:])


def wgrad_autograd(c, d):
    """(reward, dW, db) of the H = 3 rollout by torch autograd through oracle.torch_path on the case's own factors."""
    import torch
    from oracle import torch_path as tq
    E, U = c["E"], c["U"]
    gp = lambda m, s: tq.predict_given_factorizations(d["X"], d["ls"], d["var"], m, s, d["iKt"], d["beta"])
    prm = [torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (d["W"], d["b"])]
    pol = lambda m, s: tq.linear_controller(m, s, prm[0], prm[1], tq.t(np.ones(U)))
    rew = lambda m, s: tq.exponential_reward(m, s, np.eye(E), np.zeros((1, E)))
    _, _, R = tq.predict(gp, pol, rew, tq.t(d["m0"]), tq.t(d["S0"]), sc.WGRAD_H)
    R = R.sum()
    R.backward()
    return float(R.detach()), prm[0].grad.numpy().copy(), prm[1].grad.numpy().copy()


def wgrad_tol(c):
    """max(TOL_GRAD, 8 x the error of autograd against the 40-digit truth) per block (reward, dW, db): the link's rule."""
    d, t = wgrad_case(c)
    R, dW, db = wgrad_autograd(c, d)
    errs = (abs(R - t["R"]) / max(abs(t["R"]), sc.TINY), block_error(dW, t["dW"]), block_error(db, t["db"]))
    return tuple(max(sc.TOL_GRAD, 8.0 * e) for e in errs), errs
