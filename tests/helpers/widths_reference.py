"""Reference trajectories of the cases in helpers/dims_cases.py, on the CPU in float64.

`oracle_trajectory`: every state of the H-step rollout and its reward from oracle.tf_path (pilco.py:118-153, mgpr.py:91-149,
smgpr.py:24-48), the restatement the CPU suite holds to the executed reference.  `pair_step` / `perturbed_trajectory`: the same
step with the pair sums written out per output pair, so that the sensitivity test can damage them the way a kernel bug would.
`torch_gradient`: reward and policy gradients by torch autograd through oracle.torch_path."""
from __future__ import annotations

import numpy as np

from oracle import tf_path as tp


def factors(c, d):
    if c["M"]:
        return tp.fitc_factorizations(d["X"], d["Y"], d["Z"], d["ls"], d["var"], d["noise"])
    return tp.calculate_factorizations(d["X"], d["Y"], d["ls"], d["var"], d["noise"])


def points(c, d):
    return d["Z"] if c["M"] else d["X"]


def np_controller(c, d):
    if c["policy"] == "linear":
        return lambda m, s: tp.linear_controller(m, s, d["W"], d["b"], d["maxact"])
    if c["policy"] == "rbf":
        return lambda m, s: tp.rbf_controller(m, s, d["cX"], d["cY"], d["cl"], max_action=d["maxact"], squash=True)
    return tp.no_controller


def np_reward(c, d):
    ex = lambda m, s: tp.exponential_reward(m, s, d["Wr"], d["tr"])
    li = lambda m, s: tp.linear_reward(m, s, d["Wl"])
    if c["reward"] == "exp":
        return ex
    if c["reward"] == "lin":
        return li
    return lambda m, s: tp.combined_rewards(m, s, [ex, li], [0.7, -0.4])


def _trajectory(step, c, d):
    """(H+1, E + E*E) states [m | S] and the summed reward (the reward of state t before its propagation, pilco.py:133)."""
    ctl, rew = np_controller(c, d), np_reward(c, d)
    m, s = np.asarray(d["m0"], np.float64).reshape(1, -1), np.asarray(d["S0"], np.float64)
    rows, total = [np.concatenate([m.ravel(), s.ravel()])], 0.0
    for _ in range(c["H"]):
        total += float(np.asarray(rew(m, s)[0]).ravel()[0])
        m_u, s_u, c_xu = ctl(m, s)
        mj = np.concatenate([m, m_u], axis=1)
        s1 = np.concatenate([s, s @ c_xu], axis=1)
        sj = np.concatenate([s1, np.concatenate([(s @ c_xu).T, s_u], axis=1)], axis=0)
        M, S, V = step(mj, sj)
        m, s = M.reshape(1, -1) + m, S + s + s1 @ V + V.T @ s1.T
        rows.append(np.concatenate([m.ravel(), s.ravel()]))
    return np.stack(rows), total


def oracle_trajectory(c, d, zero_iK=False):
    """zero_iK: the model of gp_set_factors(iK=None, beta) -- the pair sums without the iK term."""
    iK, beta = factors(c, d)
    if zero_iK:
        iK = np.zeros_like(iK)
    pts = points(c, d)
    return _trajectory(lambda m, s: tp.predict_given_factorizations_pairs(pts, d["ls"], d["var"], m, s, iK, beta), c, d)


def pair_step(pts, ls, var, m, s, iK, beta, drop_point=False, drop_dim=False, pair_hook=None):
    """mgpr.py:91-149 with the pair sums per output pair (b <= a).  drop_point: the last point is left out of the pair sums
    (beta_a' L beta_b and tr(iK_a L)) while iK and beta stay those of all points; drop_dim: the last input dimension is left
    out of the pair exponent log(var_a) + log(var_b) + k_a + k_b + maha only.  pair_hook: called with the finished pair sums
    {(a, b): value} (b <= a; what the ranks of a sharded step exchange, up to the mean product) and returns the ones the
    covariance is assembled from."""
    m = m.reshape(1, -1)
    E, D = ls.shape
    zeta = pts - m
    eye = np.eye(D)
    M, V, k = np.empty(E), np.empty((D, E)), []
    for a in range(E):
        iL = np.diag(1.0 / ls[a])
        iN = zeta @ iL
        B = iL @ s @ iL + eye
        t = np.linalg.solve(B.T, iN.T).T
        lb = np.exp(-0.5 * np.sum(iN * t, 1)) * beta[a]
        cc = var[a] / np.sqrt(np.linalg.det(B))
        M[a] = lb.sum() * cc
        V[:, a] = (t @ iL).T @ lb * cc
    nd = D - 1 if drop_dim else D
    zk, sk = zeta[:, :nd], s[:nd, :nd]
    for a in range(E):
        k.append(np.log(var[a]) - 0.5 * np.sum((zk / ls[a, :nd]) ** 2, 1))
    n = pts.shape[0] - (1 if drop_point else 0)
    vals = {}
    for a in range(E):
        for b in range(a + 1):
            R = s @ np.diag(1.0 / ls[a] ** 2 + 1.0 / ls[b] ** 2) + eye
            Rk = sk @ np.diag(1.0 / ls[a, :nd] ** 2 + 1.0 / ls[b, :nd] ** 2) + np.eye(nd)
            Q = np.linalg.solve(Rk, sk) / 2.0
            za, wb = zk[:n] / ls[a, :nd] ** 2, -zk[:n] / ls[b, :nd] ** 2
            zQ = za @ Q
            maha = -2.0 * zQ @ wb.T + np.sum(zQ * za, 1)[:, None] + np.sum(wb @ Q * wb, 1)[None, :]
            L = np.exp(k[a][:n, None] + k[b][None, :n] + maha)
            val = beta[a, :n] @ L @ beta[b, :n]
            if a == b:
                val -= np.sum(iK[a][:n, :n] * L)
            vals[(a, b)] = val / np.sqrt(np.linalg.det(R))
    if pair_hook:
        vals = pair_hook(vals)
    S = np.empty((E, E))
    for (a, b), val in vals.items():
        S[a, b] = S[b, a] = val
    S = S + np.diag(var) - np.outer(M, M)
    return M, S, V


def perturbed_trajectory(c, d, zero_iK=False, **damage):
    iK, beta = factors(c, d)
    if zero_iK:
        iK = np.zeros_like(iK)
    pts = points(c, d)
    return _trajectory(lambda m, s: pair_step(pts, d["ls"], d["var"], m, s, iK, beta, **damage), c, d)


def normwise_error(dev, ref, E):
    """max over steps and over the m / S blocks of max|dev - ref| / max|ref| (rows of (H+1, E + E*E) trajectories)."""
    dev, ref = np.asarray(dev, np.float64), np.asarray(ref, np.float64)
    worst = 0.0
    for t in range(ref.shape[0]):
        for sl in (slice(0, E), slice(E, E + E * E)):
            scale = np.abs(ref[t, sl]).max()
            worst = max(worst, np.abs(dev[t, sl] - ref[t, sl]).max() / (scale if scale > 0 else 1.0))
    return worst


def block_error(dev, ref):
    dev, ref = np.asarray(dev, np.float64).ravel(), np.asarray(ref, np.float64).ravel()
    scale = np.abs(ref).max() if ref.size else 0.0
    return float(np.abs(dev - ref).max() / (scale if scale > 0 else 1.0)) if ref.size else 0.0


def torch_gradient(c, d, zero_iK=False):
    """(reward, [d parameter] ) by torch autograd: (dW, db) for a LinearController, (d centres, d targets, d lengthscales)
    for an RbfController.  zero_iK: as in oracle_trajectory."""
    import torch
    from oracle import torch_path as tq
    iK, beta = factors(c, d)
    if zero_iK:
        iK = np.zeros_like(iK)
    pts, U = points(c, d), c["U"]
    gp = lambda m, s: tq.predict_given_factorizations(pts, d["ls"], d["var"], m, s, iK, beta)
    if c["policy"] == "linear":
        prm = [torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (d["W"], d["b"])]
        pol = lambda m, s: tq.linear_controller(m, s, prm[0], prm[1], tq.t(d["maxact"]))
    else:
        prm = [torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (d["cX"], d["cY"], d["cl"])]
        pol = lambda m, s: tq.rbf_controller(m, s, prm[0], prm[1], prm[2], torch.full((U,), 1e-4, dtype=torch.float64), tq.t(d["maxact"]))
    ex = lambda m, s: tq.exponential_reward(m, s, d["Wr"], d["tr"])
    li = lambda m, s: m @ tq.t(d["Wl"])
    rew = {"exp": ex, "lin": li, "comb": lambda m, s: 0.7 * ex(m, s) - 0.4 * li(m, s)}[c["reward"]]
    _, _, R = tq.predict(gp, pol, rew, tq.t(d["m0"]), tq.t(d["S0"]), c["H"])
    R = R.sum()
    R.backward()
    return float(R.detach()), [p.grad.numpy().copy() for p in prm]
