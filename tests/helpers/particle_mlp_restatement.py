"""NumPy restatement of the MLP policy of the particle paths (PILCO_POLICY_MLP; csrc/particles.hip, csrc/particles_grad.hip,
docs/particle_mlp.md) -- the yardstick of tests/test_gpu_particle_mlp.py, itself pinned to torch autograd in
tests/test_particle_mlp_cpu.py.  The action, its Jacobian, the reverse recursion and the four parameter adjoints, every sum in
np.longdouble; the dynamics part -- the step matrices and their per-entry bounds -- comes from the existing restatements
(helpers/particle_grad_restatement.py: posterior_jac; helpers/particle_fn_grad_restatement.py: jacobian_fn).  It shares no code
with the kernels.

policy: dict(W1 (Hn, E), b1 (Hn,), W2 (U, Hn), b2 (U,), max_action, squash)
  a = W1 x + b1,  h = tanh(a),  s = W2 h + b2,  u = squash ? max_action sin(s) : s
  ds_k = g_u[k] (squash ? max_action_k cos(s_k) : 1),  delta_j = (1 - h_j^2) sum_k W2_kj ds_k,  lam' += W1^T delta
  dW1 = sum_p delta x^T,  db1 = sum_p delta,  dW2 = sum_p ds h^T,  db2 = sum_p ds          (over P)."""
import numpy as np

from helpers import particle_fn_grad_restatement as fg
from helpers import particle_fn_restatement as rf
from helpers import particle_grad_restatement as pg
from helpers import particles_restatement as pr

LD = np.longdouble
U53 = 2.0 ** -53

# The kernels' count of rounding steps (docs/particle_mlp.md, "The constant c"), read off k_particle_head and k_pg_reverse before
# anything was measured.  Per term of s_k = b2_k + sum_j W2_kj h_j: Hn fused multiply-adds and the addition of b2_k (Hn + 1),
# tanh within 2 ulp (2), then on the sum sin within 2 ulp (2), cos within 2 ulp (2), the product with max_action (1) and the
# product max_action * cos(s) of the adjoint (1), one spare (1).  Per term of a_j = b1_j + sum_e W1_je x_e: E fused multiply-adds
# and the addition of b1_j.
def c_mlp(E, Hn):
    """(c, c_a): roundings per term of the s sums (tanh, sin, cos included) and of the pre-activation sums."""
    return Hn + 9, E + 1


def _parts(policy, x):
    W1, b1, W2, b2 = (np.asarray(policy[k], LD) for k in ("W1", "b1", "W2", "b2"))
    b1, b2 = b1.reshape(-1), b2.reshape(-1)
    x = np.asarray(x, LD)
    a = x @ W1.T + b1[None, :]
    h = np.tanh(a)
    s = h @ W2.T + b2[None, :]
    U = W2.shape[0]
    squash = bool(policy.get("squash", True))
    scale = np.broadcast_to(np.asarray(policy.get("max_action", 1.0), LD).reshape(-1), (U,)) if squash else np.ones(U, LD)
    return W1, b1, W2, b2, x, a, h, s, scale, squash


def action(policy, x):
    """x (P, E) -> u (P, U), float64 from longdouble sums."""
    *_, s, scale, squash = _parts(policy, x)
    return ((scale[None, :] * np.sin(s)) if squash else s).astype(np.float64)


def action_jacobian(policy, x):
    """d u / d x (P, U, E)."""
    W1, _, W2, _, _, _, h, s, scale, squash = _parts(policy, x)
    c = scale[None, :] * np.cos(s) if squash else np.ones_like(s)
    J = np.einsum("kj,pj,je->pke", W2, 1.0 - h * h, W1)
    return (c[:, :, None] * J).astype(np.float64)


def ds_factor(policy, x):
    """(P, U): d u_k / d s_k."""
    *_, s, scale, squash = _parts(policy, x)
    return (scale[None, :] * np.cos(s) if squash else np.ones_like(s)).astype(np.float64)


def action_bound(policy, x):
    """(P, U): the per-entry bound of the device's action against `action`,
      |scale_k| [2^-53 c (sum_j |W2_kj h_j| + |b2_k|) + sum_j |W2_kj| (1 - h_j^2) 2^-53 c_a (sum_e |W1_je x_e| + |b1_j|)]
    (the second term: the pre-activation error through tanh's slope), and the absolute-sum scale |scale_k| (sum_j |W2_kj h_j| +
    |b2_k|)."""
    W1, b1, W2, b2, x, _, h, _, scale, _ = _parts(policy, x)
    c, ca = c_mlp(W1.shape[1], W1.shape[0])
    ma = np.abs(x) @ np.abs(W1).T + np.abs(b1)[None, :]
    ms = np.abs(h) @ np.abs(W2).T + np.abs(b2)[None, :]
    slope = ((1.0 - h * h) * (U53 * ca) * ma) @ np.abs(W2).T
    sc = np.abs(scale)[None, :] * ms
    return (np.abs(scale)[None, :] * (U53 * c * ms + slope)).astype(np.float64), sc.astype(np.float64)


class MlpAdj:
    """The parameter cotangents of one reverse sweep.  step: the exact sums.  scale_step: the same sums with every term in
    absolute value.  bound_step: their first-order error for cotangent errors dds >= 0 and the kernel's own rounding of h, s,
    cos(s) and delta with the constants of c_mlp."""

    def __init__(self, policy):
        self.p = policy
        Hn, E = np.asarray(policy["W1"]).shape
        U = np.asarray(policy["W2"]).shape[0]
        self.g = [np.zeros((Hn, E), LD), np.zeros(Hn, LD), np.zeros((U, Hn), LD), np.zeros(U, LD)]

    def _add(self, delta, x, ds, h):
        self.g[0] += np.einsum("pj,pe->je", delta, x)
        self.g[1] += delta.sum(axis=0)
        self.g[2] += np.einsum("pk,pj->kj", ds, h)
        self.g[3] += ds.sum(axis=0)

    def step(self, x, ds):
        """x (P, E), ds (P, U) -> (ds / dx)^T ds (P, E); adds the step's parameter sums."""
        W1, _, W2, _, x, _, h, _, _, _ = _parts(self.p, x)
        ds = np.asarray(ds, LD)
        delta = (1.0 - h * h) * (ds @ W2)
        self._add(delta, x, ds, h)
        return (delta @ W1).astype(np.float64)

    def scale_step(self, x, sds):
        W1, _, W2, _, x, _, h, _, _, _ = _parts(self.p, x)
        sds = np.asarray(sds, LD)
        delta = (1.0 - h * h) * (sds @ np.abs(W2))
        self._add(delta, np.abs(x), sds, np.abs(h))
        return (delta @ np.abs(W1)).astype(np.float64)

    def rounding(self, x):
        """(dh (P, Hn), dc (P, U)): the kernel's error of h_j and of d u_k / d s_k."""
        W1, b1, W2, b2, x, _, h, s, scale, squash = _parts(self.p, x)
        c, ca = c_mlp(W1.shape[1], W1.shape[0])
        ma = np.abs(x) @ np.abs(W1).T + np.abs(b1)[None, :]
        dh = (1.0 - h * h) * (U53 * ca) * ma + 2 * U53 * np.abs(h)
        dss = dh @ np.abs(W2).T + U53 * c * (np.abs(h) @ np.abs(W2).T + np.abs(b2)[None, :])
        dc = np.abs(scale)[None, :] * (np.abs(np.sin(s)) * dss + 3 * U53 * np.abs(np.cos(s))) if squash else np.zeros_like(s)
        return dh, dc

    def bound_step(self, x, ads, dds):
        """ads (P, U) = |ds|, dds (P, U) its error bound -> the error bound of (ds / dx)^T ds (P, E); adds the sums' bounds."""
        W1, _, W2, _, x, _, h, _, _, _ = _parts(self.p, x)
        dh, _ = self.rounding(x)
        ads, dds = np.asarray(ads, LD), np.asarray(dds, LD)
        T, dT = ads @ np.abs(W2), dds @ np.abs(W2)
        ddelta = (1.0 - h * h) * dT + (2 * np.abs(h) * dh + 2 * U53) * T
        self.g[0] += np.einsum("pj,pe->je", ddelta, np.abs(x))
        self.g[1] += ddelta.sum(axis=0)
        self.g[2] += np.einsum("pk,pj->kj", dds, np.abs(h)) + np.einsum("pk,pj->kj", ads, dh)
        self.g[3] += dds.sum(axis=0)
        return (ddelta @ np.abs(W1)).astype(np.float64)

    def finish(self, P):
        b2_shape = np.asarray(self.p["b2"]).shape
        out = [(g / P).astype(np.float64) for g in self.g]
        out[3] = out[3].reshape(b2_shape)
        return tuple(out)


# ------------------------------------------------------------------ the step matrices of the two dynamics, and their bounds
def step_matrix_marginal(model, policy, x, eps, observation_noise=False, bound=False):
    """A (P, E, D) of particle_grad_restatement.step_matrix at z = [x, action(x)]; bound: also dA, the per-entry bound of
    particle_grad_restatement.reverse_bound."""
    x, eps = np.asarray(x, np.float64), np.asarray(eps, np.float64)
    E = x.shape[1]
    _, v, dmu, dv = pg.posterior_jac(model, np.concatenate([x, action(policy, x)], axis=1))
    if observation_noise:
        v = v + np.asarray(model["noise"], np.float64).reshape(1, -1)
    pos = v > 0.0
    sd = np.sqrt(np.maximum(v, 0.0))
    g = np.where(pos, eps / (2.0 * np.where(pos, sd, 1.0)), 0.0)
    A = dmu + g[:, :, None] * dv
    A[:, np.arange(E), np.arange(E)] += 1.0
    if not bound:
        return A
    assert np.all(pos)
    sf2 = np.asarray(model["variance"], np.float64)
    lmin = np.asarray(model["lengthscales"], np.float64).min(axis=1)
    dg = np.abs(g) * (1e-8 * sf2)[None, :] / (2.0 * v)
    dA = (1e-8 * np.abs(dmu).max(axis=(0, 2)))[None, :, None] + np.abs(g)[:, :, None] * (1e-8 * sf2 / lmin)[None, :, None] \
        + dg[:, :, None] * np.abs(dv)
    return A, dA


def step_matrix_fn(model, policy, dr, v, x, bound=False):
    """A (P, E, D) of particle_fn_grad_restatement.step_matrix_fn at z = [x, action(x)]; bound: also its dA."""
    x = np.asarray(x, np.float64)
    E = x.shape[1]
    dF, m1, m2 = fg.jacobian_fn(model, dr, v, np.concatenate([x, action(policy, x)], axis=1))
    dF = dF.copy()
    dF[:, np.arange(E), np.arange(E)] += LD(1.0)
    A = dF.astype(np.float64)
    if not bound:
        return A
    N, D = np.asarray(model["X"]).shape
    L = np.asarray(dr["omega"]).shape[1]
    return A, (U53 * (fg.c_prime(N, L, D) * m1 + (D + 2) * m2)).astype(np.float64)


def step_marginal(model, policy, x, eps, observation_noise=False):
    """particles_restatement.step with the MLP's action: x' (P, E)."""
    x = np.asarray(x, np.float64)
    mu, v = pr.posterior(model, np.concatenate([x, action(policy, x)], axis=1))
    if observation_noise:
        v = v + np.asarray(model["noise"], np.float64).reshape(1, -1)
    return x + mu + np.sqrt(np.maximum(v, 0.0)) * np.asarray(eps, np.float64), mu, v


def step_fn(model, policy, dr, v, x):
    """particle_fn_restatement.step with the MLP's action: (x', f, m1, m2)."""
    f, m1, m2 = rf.f_of(model, dr, v, np.concatenate([np.asarray(x, np.float64), action(policy, x)], axis=1))
    return (np.asarray(x, LD) + f).astype(np.float64), f, m1, m2


# ------------------------------------------------------------------ the sweep on supplied matrices
def reverse(policy, terms, xs, mats):
    """The recursion of particle_grad_restatement.reverse on SUPPLIED matrices: xs (>= H, P, E), mats the H - 1 matrices of
    t = 0 .. H-2 (H = len(mats) + 1).  -> ((dW1, db1, dW2, db2), dx0 (P, E))."""
    xs = np.asarray(xs, np.float64)
    H = len(mats) + 1
    P, E = xs.shape[1:]
    adj = MlpAdj(policy)
    lam = np.zeros((P, E))
    for t in range(H - 1, -1, -1):
        x = xs[t]
        if t < H - 1:
            A = mats[t]
            ds = np.einsum("ped,pe->pd", A[:, :, E:], lam) * ds_factor(policy, x)
            lam = np.einsum("ped,pe->pd", A[:, :, :E], lam) + adj.step(x, ds)
        lam = lam + pg.reward_grad(terms, x)
    return adj.finish(P), lam


def reverse_bound(policy, terms, xs, mats, dmats):
    """Bounds on |device - reverse| for a sweep on the SAME states, and the absolute-sum scale of every quantity: the first-order
    propagation of particle_grad_restatement.reverse_bound with the supplied per-entry bounds dmats of the matrices, extended by
    the MLP's own rounding (MlpAdj.rounding, MlpAdj.bound_step).  -> ((bounds, dlam), (scales, slam))."""
    xs = np.asarray(xs, np.float64)
    H = len(mats) + 1
    P, E = xs.shape[1:]
    bnd, scl, exact = MlpAdj(policy), MlpAdj(policy), MlpAdj(policy)
    lam, dlam, slam = np.zeros((P, E)), np.zeros((P, E)), np.zeros((P, E))
    for t in range(H - 1, -1, -1):
        x = xs[t]
        if t < H - 1:
            A, dA = mats[t], dmats[t]
            cs = ds_factor(policy, x)
            c, aA = np.abs(cs), np.abs(A)
            _, dc = bnd.rounding(x)
            gu = np.einsum("ped,pe->pd", A[:, :, E:], lam)
            dds = c * (np.einsum("ped,pe->pd", aA[:, :, E:], dlam) + np.einsum("ped,pe->pd", dA[:, :, E:], np.abs(lam))) \
                + dc.astype(np.float64) * np.einsum("ped,pe->pd", aA[:, :, E:], np.abs(lam))
            sds = c * np.einsum("ped,pe->pd", aA[:, :, E:], slam)
            ds = cs * gu
            dlam = np.einsum("ped,pe->pd", aA[:, :, :E], dlam) + np.einsum("ped,pe->pd", dA[:, :, :E], np.abs(lam)) \
                + bnd.bound_step(x, np.abs(ds), dds)
            slam = np.einsum("ped,pe->pd", aA[:, :, :E], slam) + scl.scale_step(x, sds)
            lam = np.einsum("ped,pe->pd", A[:, :, :E], lam) + exact.step(x, ds)
        lam = lam + pg.reward_grad(terms, x)
        slam = slam + np.abs(reward_grad_abs(terms, x))
    return (bnd.finish(P), dlam), (scl.finish(P), slam)


def reward_grad_abs(terms, x):
    return np.abs(pg.reward_grad(terms, x))


def zeros_like_grads(policy, P):
    return MlpAdj(policy).finish(1), np.zeros((P, np.asarray(policy["W1"]).shape[1]))


def policy_of(controller, squash=True):
    """The restatement's policy dict of a pilco_amd.controllers.MlpController."""
    return dict(W1=controller.W1.numpy(), b1=controller.b1.numpy(), W2=controller.W2.numpy(), b2=controller.b2.numpy(),
                max_action=controller.max_action, squash=squash)
