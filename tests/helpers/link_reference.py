"""What the link-edge tests share: the fixture, the float64 restatement of a case (oracle.tf_path: the YARDSTICK, not the
truth), the units and K = |value - truth| / unit per block, the caps, and torch autograd for the cases without a 50-digit
gradient.  CPU only; the GPU test imports it too (it reads the fixture and oracle.tf_path, nothing else)."""
from __future__ import annotations

import os

import numpy as np

from helpers import link_cases as lc
from oracle import tf_path as tp

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "link_edges.npz")
_FX = None


def fixture(c):
    """dict key -> array of the case's truth."""
    global _FX
    if _FX is None:
        z = np.load(GOLDEN)
        _FX = {k: z[k] for k in z.files}
    pre = c["name"] + "/"
    out = {k[len(pre):]: v for k, v in _FX.items() if k.startswith(pre)}
    assert out, "no truth for %s in the fixture (python -m oracle.gen_golden_link %s)" % (c["name"], c["name"])
    return out


def maxact_vec(c, d):
    return np.ones(c["U"]) if d["maxact"] is None else np.asarray(d["maxact"], np.float64)


def np_controller(c, d, tpm=tp):
    if c["policy"] == "linear":
        return lambda m, s: tpm.linear_controller(m, s, d["W"], d["b"], maxact_vec(c, d), c["squash"])
    if c["policy"] == "rbf":
        return lambda m, s: tpm.rbf_controller(m, s, d["cX"], d["cY"], d["cl"], max_action=maxact_vec(c, d), squash=c["squash"])
    return tp.no_controller


def np_reward_terms(d, tpm=tp):
    """[(coef, callable (m, s) -> (mean, variance))]."""
    out = []
    for tm in d["rewards"]:
        if tm["kind"] == "exp":
            out.append((tm["coef"], lambda m, s, tm=tm: tpm.exponential_reward(m, s, tm["W"], tm["t"])))
        else:
            out.append((tm["coef"], lambda m, s, tm=tm: tpm.linear_reward(m, s, tm["W"])))
    return out


def np_reward(d, tpm=tp):
    terms = np_reward_terms(d, tpm)

    def rew(m, s):
        if not terms:
            return np.zeros((1, 1)), np.zeros((1, 1))
        mu, var = tp.combined_rewards(m, s, [f for _, f in terms], [k for k, _ in terms])
        return np.asarray(mu, np.float64).reshape(1, 1), np.asarray(var, np.float64).reshape(1, 1)
    return rew


def np_stage(c, d, tpm=tp):
    """The restatement's stages at (m0, S0): dict M (U), S (U,U), V (E,U), rmu, rvar."""
    out = {}
    if c["U"] > 0:
        M, S, V = np_controller(c, d, tpm)(d["m0"], d["S0"])
        out.update(M=np.ravel(M), S=np.asarray(S), V=np.asarray(V))
    if d["rewards"]:
        mu, var = np_reward(d, tpm)(d["m0"], d["S0"])
        out.update(rmu=float(mu[0, 0]), rvar=float(var[0, 0]))
    return out


def np_rollout(c, d, tpm=tp):
    """The restatement's rollout: traj (H+1, E + E*E), total reward, act (H, U + U*U + E*U) = [M | S | s V]."""
    iK, beta = tp.calculate_factorizations(d["X"], d["Y"], d["ls"], d["var"], d["noise"])
    ctl, rew = np_controller(c, d, tpm), np_reward(d, tpm)
    m, s = np.asarray(d["m0"], np.float64).reshape(1, -1), np.asarray(d["S0"], np.float64)
    rows, acts, total = [np.concatenate([m.ravel(), s.ravel()])], [], 0.0
    for _ in range(c["H"]):
        total += float(rew(m, s)[0][0, 0])
        m_u, s_u, c_xu = ctl(m, s)
        acts.append(np.concatenate([np.ravel(m_u), np.ravel(s_u), np.ravel(s @ c_xu)]))
        mj = np.concatenate([m, m_u], axis=1)
        s1 = np.concatenate([s, s @ c_xu], axis=1)
        sj = np.concatenate([s1, np.concatenate([(s @ c_xu).T, s_u], axis=1)], axis=0)
        M, S, V = tp.predict_given_factorizations_pairs(d["X"], d["ls"], d["var"], mj, sj, iK, beta)
        m, s = M.reshape(1, -1) + m, S + s + s1 @ V + V.T @ s1.T
        rows.append(np.concatenate([m.ravel(), s.ravel()]))
    return np.stack(rows), total, np.stack(acts)


_FWD_TOL = {}


def fwd_tol(c, d=None, fx=None):
    """The rollout-level tolerance of a case: TOL_FWD, except where the float64 restatement itself cannot hold it: an
    RbfController's beta comes from a float64 factorisation of its own Gram matrix (lengthscales 1e2: beta ~ 1e4, condition
    ~ 1e8, the restatement 1.7e-9 from the truth).  For an RbfController: max(TOL_FWD, 8 x the restatement's own normwise
    error), as for the stage caps; TOL_FWD for every other case."""
    if c["policy"] != "rbf":
        return lc.TOL_FWD
    if c["name"] not in _FWD_TOL:
        d, fx = d or lc.make_data(c), fx or fixture(c)
        traj, total, _ = np_rollout(c, d)
        from helpers import widths_reference as wr
        err = max(wr.normwise_error(traj, fx["traj"], c["E"]), abs(total - fx["rew"][-1]) / abs(fx["rew"][-1]))
        _FWD_TOL[c["name"]] = max(lc.TOL_FWD, 8.0 * err)
    return _FWD_TOL[c["name"]]


# ------------------------------------------------------------------ units and K
def stage_blocks(c, d, fx):
    """block -> (truth, unit, exact0) of the two stages at (m0, S0)."""
    E, U = c["E"], c["U"]
    out = {}
    if U > 0:
        e, pre = maxact_vec(c, d), fx["pre"]
        M, S, V = fx["pa"][:U], fx["pa"][U:U + U * U].reshape(U, U), fx["pa"][U + U * U:].reshape(E, U)
        if c["squash"]:
            uM, uS = lc.unit_squash_mean(e, pre), lc.unit_squash_cov(e, pre)
        else:   # (no squash: a dot product and W s W^T, normwise)
            uM, uS = lc.EPS * (1.0 + np.abs(pre)), lc.EPS * max(np.abs(S).max(), lc.TINY) * np.ones_like(S)
        out.update(M=(M, uM, "M" in c["exact0"]), S=(S, uS, "S" in c["exact0"]), V=(V, lc.unit_cross(V, pre), False))
    if "rw" in fx:
        mu, var = fx["rw"][-1, 0], fx["rw"][-1, 1]
        um = uv = 0.0
        for tm, row in zip(d["rewards"], fx["rw"][:-1]):   # (a combination: the terms' units, weighted as the terms are)
            if tm["kind"] == "exp":
                um += abs(tm["coef"]) * lc.unit_reward_mean(row[0], row[2])
                uv += tm["coef"] ** 2 * lc.unit_reward_var(row[0], row[3], row[2])
            else:
                um += abs(tm["coef"]) * lc.EPS * float(np.abs(np.ravel(d["m0"]) * tm["W"]).sum())
                uv += tm["coef"] ** 2 * lc.EPS * float(np.abs(tm["W"][:, None] * d["S0"] * tm["W"][None, :]).sum())
        out.update(rmu=(mu, um, "rmu" in c["exact0"]), rvar=(var, uv, "rvar" in c["exact0"]))
    return out


def k_of(val, truth, unit, exact0=False):
    """max |val - truth| / unit; exact0: against 2^-1022 (the truth is 0 or denormal).  NaN -> inf."""
    val, truth = np.asarray(val, np.float64), np.asarray(truth, np.float64)
    # (no unit below the smallest normal number: under it float64 is absolute, in steps of 2^-1074)
    unit = np.full(truth.shape, lc.TINY) if exact0 else np.maximum(np.broadcast_to(np.asarray(unit, np.float64), truth.shape), lc.TINY)
    diff = np.abs(val.reshape(truth.shape) - truth)
    if not np.all(np.isfinite(val)):
        return float("inf")
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.where(diff == 0.0, 0.0, diff / unit)
    return float(np.max(k)) if k.size else 0.0


def stage_k(c, d, fx, vals):
    """K per block of stage values `vals` (dict as np_stage returns)."""
    return {b: k_of(vals[b], tr, un, ex) for b, (tr, un, ex) in stage_blocks(c, d, fx).items() if b in vals}


_CAPS = None
REWARD_BLOCKS = ("rmu", "rvar")


def factored_data(d):
    """The case's data with every weight that takes the factored device path replaced by what that path evaluates: F F^T,
    F from psd_factor's Jacobi rotations (backward error ~ E 2^-53 |W|; a slightly negative eigenvalue dropped)."""
    d2 = dict(d, rewards=[dict(tm) for tm in d["rewards"]])
    for tm in d2["rewards"]:
        if tm["kind"] == "exp":
            r, F = lc.psd_factor(tm["W"])
            if r > 0:
                tm["W"] = F @ F.T
    return d2


def k_ref_table(cases=None):
    """case name -> {block: K_ref} of the float64 restatement against the truth.  A reward block's K_ref is the larger of two
    evaluations of the restatement: with the weight as given, and with the weight the factored device path works from
    (factored_data) -- rounding the kernel is entitled to, measured instead of argued (st_e32_rankEm1: 4.8 and 52)."""
    out = {}
    for c in (lc.CASES if cases is None else cases):
        d, fx = lc.make_data(c), fixture(c)
        ks = stage_k(c, d, fx, np_stage(c, d))
        if d["rewards"]:
            kf = stage_k(c, d, fx, np_stage(c, factored_data(d)))
            for b in REWARD_BLOCKS:
                ks[b] = max(ks[b], kf[b])
        out[c["name"]] = ks
    return out


def class_of(c, block):
    """The class a block's cap is taken over.  The controller blocks: the case's group.  The reward never sees the policy: its
    class is the magnitude of the state covariance, with the wide states (E >= 16: the factor's error grows with E) and the
    two cases on the near side of psd_factor's switches (a perturbation of 1e-13 |W| is dropped by design) on their own."""
    if block in REWARD_BLOCKS:
        if c["reward"] in ("neg13", "asym14"):
            return "reward/switch"
        if c["E"] >= 16:
            return "reward/wide"
        return "reward/large" if c["group"].endswith("/large") else "reward/small"
    return c["group"]


def compute_caps():
    """(class, block) -> cap of the device's K: 8 x the restatement's worst K_ref of the class (three bits: FMA contraction,
    fast_rcp / fast_rsqrt for divisions, another summation order -- the same formulas), floor 4."""
    worst = {}
    for c in lc.CASES:
        for b, k in k_ref_table([c])[c["name"]].items():
            key = (class_of(c, b), b)
            worst[key] = max(worst.get(key, 0.0), k)
    return {key: max(4.0, 8.0 * k) for key, k in worst.items()}


def caps():
    """The caps the fixture holds (oracle/gen_golden_link.py stores compute_caps() under "_caps/class|block"): the device is
    held to the same numbers on every machine; the CPU suite checks that a recomputation agrees within a factor of 2."""
    global _CAPS
    if _CAPS is None:
        fixture(lc.CASES[0])
        _CAPS = {tuple(k[len("_caps/"):].split("|")): float(v) for k, v in _FX.items() if k.startswith("_caps/")}
        assert _CAPS, "no caps in the fixture (python -m oracle.gen_golden_link <any case>)"
    return _CAPS


def cap_of(c, block):
    return caps()[(class_of(c, block), block)]


def act_blocks(c, row):
    """[M | S | s V] row of the fixture's / a tape's action record -> (M, S, C)."""
    E, U = c["E"], c["U"]
    return row[:U], row[U:U + U * U].reshape(U, U), row[U + U * U:].reshape(E, U)


def tape_action(c, rec):
    """The action's moments in a tape record [jm (D) | js (D,D) | ...]: mean, covariance, cross block s V."""
    E, D = c["E"], c["D"]
    jm, js = rec[:D], rec[D:D + D * D].reshape(D, D)
    return jm[E:], js[E:, E:], js[:E, E:]


# ------------------------------------------------------------------ autograd
def torch_gradient(c, d):
    """(reward, [d parameter]) by torch autograd through oracle.torch_path, for any reward recipe."""
    import torch
    from oracle import torch_path as tq
    iK, beta = tp.calculate_factorizations(d["X"], d["Y"], d["ls"], d["var"], d["noise"])
    U = c["U"]
    gp = lambda m, s: tq.predict_given_factorizations(d["X"], d["ls"], d["var"], m, s, iK, beta)
    ma = tq.t(maxact_vec(c, d))
    if c["policy"] == "linear":
        prm = [torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (d["W"], d["b"])]
        pol = lambda m, s: tq.linear_controller(m, s, prm[0], prm[1], ma)
    else:
        prm = [torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (d["cX"], d["cY"], d["cl"])]
        pol = lambda m, s: tq.rbf_controller(m, s, prm[0], prm[1], prm[2], torch.full((U,), 1e-4, dtype=torch.float64), ma)

    def rew(m, s):
        tot = torch.zeros((1, 1), dtype=torch.float64)
        for tm in d["rewards"]:
            if tm["kind"] == "exp":
                tot = tot + tm["coef"] * tq.exponential_reward(m, s, tm["W"], tm["t"])
            else:
                tot = tot + tm["coef"] * (m @ tq.t(tm["W"]).reshape(-1, 1))
        return tot
    _, _, R = tq.predict(gp, pol, rew, tq.t(d["m0"]), tq.t(d["S0"]), c["H"])
    R = R.sum()
    if not d["rewards"]:
        return 0.0, [np.zeros_like(p.detach().numpy()) for p in prm]
    R.backward()
    return float(R.detach()), [(p.grad.numpy().copy() if p.grad is not None else np.zeros(p.shape)) for p in prm]
