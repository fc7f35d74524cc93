"""NumPy float64 restatement of the particle rollout (pilco_rollout_particles, csrc/particles.hip) -- the yardstick of
tests/test_gpu_particles.py, itself pinned to the executed reference in tests/test_particles_cpu.py:
  * one particle step: the policy's deterministic action (what the reference's PILCO.compute_action(x) returns), the GP
    posterior at [x, u] (helpers/predict_restatement.py) and the update x' = x + mu + sqrt(max(v, 0)) eps;
  * the reward terms at zero covariance;
  * the random stream: Philox4x32-10 and the Box-Muller map of csrc/philox_normal.h, in Python integers."""
import math

import numpy as np

from helpers.predict_restatement import fitc_predict_f, gpr_predict_f, se_ard

RBF_SQUASH_VARIANCE = 1e-6   # S - diag(variance - 1e-6) at s = 0 (the reference's controllers.py:117)


# ------------------------------------------------------------------ the policy at a point
def linear_action(x, W, b, max_action=1.0, squash=True):
    """x (P, E) -> (P, U): max_action * sin(x W^T + b)."""
    a = np.asarray(x, np.float64) @ np.asarray(W, np.float64).T + np.asarray(b, np.float64).reshape(1, -1)
    return np.asarray(max_action, np.float64) * np.sin(a) if squash else a


def rbf_action(x, centres, targets, lengthscales, noise, max_action=1.0, squash=True):
    """The deterministic-GP controller at a point: mean_u = sum_i beta_ui k_u(x, c_i) with unit signal variance and
    beta_u = (K_u + noise_u I)^-1 y_u; squashed with the 1e-6 variance the reference leaves at s = 0."""
    x, C, Y = (np.asarray(a, np.float64) for a in (x, centres, targets))
    U = Y.shape[1]
    noise = np.broadcast_to(np.asarray(noise, np.float64).reshape(-1), (U,))
    a = np.empty((x.shape[0], U))
    for u in range(U):
        K = se_ard(C, C, lengthscales[u], 1.0) + noise[u] * np.eye(C.shape[0])
        a[:, u] = se_ard(x, C, lengthscales[u], 1.0) @ np.linalg.solve(K, Y[:, u])
    if not squash:
        return a
    return np.asarray(max_action, np.float64) * math.exp(-0.5 * RBF_SQUASH_VARIANCE) * np.sin(a)


def action(policy, x):
    """policy: None, dict(kind='linear', W, b, max_action) or dict(kind='rbf', X, Y, lengthscales, noise, max_action)."""
    if policy is None:
        return np.empty((np.asarray(x).shape[0], 0))
    if policy["kind"] == "linear":
        return linear_action(x, policy["W"], policy["b"], policy.get("max_action", 1.0))
    return rbf_action(x, policy["X"], policy["Y"], policy["lengthscales"], policy["noise"], policy.get("max_action", 1.0))


# ------------------------------------------------------------------ one step
def posterior(model, xu):
    """model: dict(X, Y, lengthscales, variance, noise[, Z]) -> latent mean and variance at xu (P, D): (P, E) each."""
    xu = np.asarray(xu, np.float64)
    mus, vs = [], []
    for i in range(0, xu.shape[0], 2048):   # (blocks of points: the restated kernels form N x Nt x D arrays)
        args = (model["lengthscales"], model["variance"], model["noise"], xu[i:i + 2048])
        if model.get("Z") is not None:
            mu, v = fitc_predict_f(model["X"], model["Y"], model["Z"], *args)
        else:
            mu, v = gpr_predict_f(model["X"], model["Y"], *args)
        mus.append(mu.T)
        vs.append(v.T)
    return np.concatenate(mus), np.concatenate(vs)


def step(model, policy, x, eps, observation_noise=False):
    """x (P, E), eps (P, E) -> x' (P, E), and (mu, v, u) of the step (v: the variance the draw was scaled by, unclamped)."""
    x = np.asarray(x, np.float64)
    u = action(policy, x)
    mu, v = posterior(model, np.concatenate([x, u], axis=1))
    if observation_noise:
        v = v + np.asarray(model["noise"], np.float64).reshape(1, -1)
    return x + mu + np.sqrt(np.maximum(v, 0.0)) * np.asarray(eps, np.float64), mu, v, u


# ------------------------------------------------------------------ rewards at zero covariance
def reward(terms, x):
    """terms: list of dict(kind='exponential', W, t, coef) / dict(kind='linear', W, coef); x (P, E) -> (P,)."""
    x = np.asarray(x, np.float64)
    total = np.zeros(x.shape[0])
    for t in terms:
        if t["kind"] == "exponential":
            d = x - (np.zeros(x.shape[1]) if t.get("t") is None else np.asarray(t["t"], np.float64).reshape(1, -1))
            r = np.exp(-0.5 * np.einsum("pi,ij,pj->p", d, np.asarray(t["W"], np.float64), d))
        else:
            r = x @ np.asarray(t["W"], np.float64).reshape(-1)
        total += float(t.get("coef", 1.0)) * r
    return total


# ------------------------------------------------------------------ Philox4x32-10 + Box-Muller
M32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    c0, c1, c2, c3 = (int(c) & M32 for c in counter)
    k0, k1 = (int(k) & M32 for k in key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def particle_words(seed, t, p, j):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return philox4x32_10((p, t, j, 0), (seed & M32, seed >> 32))


def uniforms(words):
    """exact: integer arithmetic, then one exact conversion (53 bits)."""
    w0, w1, w2, w3 = words
    n1, n2 = (w0 >> 5) * (1 << 26) + (w1 >> 6), (w2 >> 5) * (1 << 26) + (w3 >> 6)
    return ((1 << 53) - n1) / float(1 << 53), n2 / float(1 << 53)


def normal_pair(seed, t, p, j):
    """-> (z_2j, z_2j+1, r)."""
    u1, u2 = uniforms(particle_words(seed, t, p, j))
    r = math.sqrt(-2.0 * math.log(u1))
    a = 2.0 * math.pi * u2
    return r * math.cos(a), r * math.sin(a), r


def normals(seed, H, P, E, particles=None):
    """The draws (H, P, E) of the stream, and the radius r behind each (the error bound of a draw scales with it).
    particles: only these particle indices (the other rows stay NaN)."""
    z = np.full((H, P, E), np.nan)
    r = np.full((H, P, E), np.nan)
    for t in range(H):
        for p in (range(P) if particles is None else particles):
            for j in range((E + 1) // 2):
                z0, z1, rr = normal_pair(seed, t, p, j)
                z[t, p, 2 * j], r[t, p, 2 * j] = z0, rr
                if 2 * j + 1 < E:
                    z[t, p, 2 * j + 1], r[t, p, 2 * j + 1] = z1, rr
    return z, r
