"""NumPy restatement of the function-sample particle rollout (pilco_rollout_particles_fn, csrc/particles_fn.hip;
docs/particle_functions.md) -- the yardstick of tests/test_gpu_particle_fn.py and tests/test_particle_fn_cpu.py:
  * the four streams of csrc/philox_normal.h (domains 1..4) on the Python-integer Philox of helpers/particles_restatement.py,
    and the same streams vectorised in NumPy (held to the former in the CPU suite);
  * the features, the residuals R, V = iK R and one step, with the sums in np.longdouble;
  * the closed-form mean and variance of f_p(x) over (w, xi)."""
import math

import numpy as np

from helpers import particles_restatement as pr
from helpers.predict_restatement import se_ard

LD = np.longdouble
FREQ, PHASE, WEIGHT, XI = 1, 2, 3, 4
TWO_PI = 2.0 * math.pi


# ------------------------------------------------------------------ the streams, one block at a time (Python integers)
def domain_words(seed, c0, c1, c2, domain):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return pr.philox4x32_10((c0, c1, c2, domain), (seed & pr.M32, seed >> 32))


def domain_normal_pair(seed, c0, c1, c2, domain):
    """-> (z0, z1, r) of the block {c0, c1, c2, domain}."""
    u1, u2 = pr.uniforms(domain_words(seed, c0, c1, c2, domain))
    r = math.sqrt(-2.0 * math.log(u1))
    a = TWO_PI * u2
    return r * math.cos(a), r * math.sin(a), r


def phase(seed, l, e):
    return TWO_PI * pr.uniforms(domain_words(seed, l, e, 0, PHASE))[1]


# ------------------------------------------------------------------ the streams, vectorised
def philox_words_np(c0, c1, c2, c3, seed):
    """Philox4x32-10 on arrays of counters (broadcast together) -> four uint64 arrays holding 32-bit words."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    M = np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3 = np.broadcast_arrays(*(np.asarray(c, np.uint64) for c in (c0, c1, c2, c3)))
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & M, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & M
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def uniforms_np(words):
    w0, w1, w2, w3 = words
    n1 = (w0 >> np.uint64(5)) * np.uint64(1 << 26) + (w1 >> np.uint64(6))
    n2 = (w2 >> np.uint64(5)) * np.uint64(1 << 26) + (w3 >> np.uint64(6))
    return (np.uint64(1 << 53) - n1).astype(np.float64) / float(1 << 53), n2.astype(np.float64) / float(1 << 53)


def normal_pairs_np(c0, c1, c2, domain, seed):
    """-> z0, z1, r of the blocks {c0, c1, c2, domain}."""
    u1, u2 = uniforms_np(philox_words_np(c0, c1, c2, domain, seed))
    r = np.sqrt(-2.0 * np.log(u1))
    a = TWO_PI * u2
    return r * np.cos(a), r * np.sin(a), r


def _pairs_to_axis(z0, z1, r, n):
    """(.., J) pairs -> (.., n) with entries 2j, 2j + 1 from pair j."""
    z = np.stack([z0, z1], axis=-1).reshape(z0.shape[:-1] + (-1,))[..., :n]
    rr = np.stack([r, r], axis=-1).reshape(r.shape[:-1] + (-1,))[..., :n]
    return z, rr


def freq_normals(seed, E, L, D):
    """z (E, L, D) of domain 1 {l, e, j, 1} and the radius behind each."""
    J = (D + 1) // 2
    e, l, j = np.meshgrid(np.arange(E), np.arange(L), np.arange(J), indexing="ij")
    return _pairs_to_axis(*normal_pairs_np(l, e, j, FREQ, seed), D)


def phases(seed, E, L):
    e, l = np.meshgrid(np.arange(E), np.arange(L), indexing="ij")
    return TWO_PI * uniforms_np(philox_words_np(l, e, 0, PHASE, seed))[1]


def weights(seed, particles, E, L):
    """w (len(particles), E, L) of domain 3 {p, l, j, 3} (outputs 2j, 2j + 1) and the radii."""
    J = (E + 1) // 2
    p, l, j = np.meshgrid(np.asarray(particles), np.arange(L), np.arange(J), indexing="ij")
    z, r = _pairs_to_axis(*normal_pairs_np(p, l, j, WEIGHT, seed), E)       # (P, L, E)
    return np.ascontiguousarray(z.transpose(0, 2, 1)), np.ascontiguousarray(r.transpose(0, 2, 1))


def xis(seed, particles, E, N):
    """xi (len(particles), E, N) of domain 4 {p, i, j, 4} and the radii."""
    J = (E + 1) // 2
    p, i, j = np.meshgrid(np.asarray(particles), np.arange(N), np.arange(J), indexing="ij")
    z, r = _pairs_to_axis(*normal_pairs_np(p, i, j, XI, seed), E)
    return np.ascontiguousarray(z.transpose(0, 2, 1)), np.ascontiguousarray(r.transpose(0, 2, 1))


def draws(seed, model, P, L, particles=None):
    """The draws a call with this seed generates: dict(omega (E, L, D), phase (E, L), w (P', E, L), xi (P', E, N))."""
    X, ls = np.asarray(model["X"], np.float64), np.asarray(model["lengthscales"], np.float64)
    E, D, N = ls.shape[0], X.shape[1], X.shape[0]
    particles = np.arange(P) if particles is None else np.asarray(particles)
    z, _ = freq_normals(seed, E, L, D)
    return dict(omega=z / ls[:, None, :], phase=phases(seed, E, L), w=weights(seed, particles, E, L)[0], xi=xis(seed, particles, E, N)[0])


# ------------------------------------------------------------------ features, residuals, V, one step
def features(omega_e, phase_e, variance_e, x):
    """phi (n, L) of one output at the points x (n, D), in np.longdouble; also sum_d |omega_ld x_d| + |b_l| (n, L)."""
    om, x = np.asarray(omega_e, LD), np.asarray(x, LD)
    arg = x @ om.T + np.asarray(phase_e, LD)[None, :]
    mag = np.abs(x) @ np.abs(om).T + np.abs(np.asarray(phase_e, LD))[None, :]
    A = np.sqrt(LD(2.0) * LD(variance_e) / LD(om.shape[0]))
    return A * np.cos(arg), mag


def residual(model, dr, e):
    """R_e (N, P) = y_e - Phi_e(X) w_e - sqrt(noise_e) xi_e, and the magnitude |y| + |Phi||w| + sqrt(noise)|xi| (N, P)."""
    X, y = np.asarray(model["X"], np.float64), np.asarray(model["Y"], LD)[:, e]
    phi, _ = features(dr["omega"][e], dr["phase"][e], model["variance"][e], X)
    w, xi = np.asarray(dr["w"], LD)[:, e, :], np.asarray(dr["xi"], LD)[:, e, :]
    sn = np.sqrt(LD(model["noise"][e]))
    R = y[:, None] - phi @ w.T - sn * xi.T
    mag = np.abs(y)[:, None] + np.abs(phi) @ np.abs(w).T + sn * np.abs(xi).T
    return R, mag


def v_of(model, dr, iK):
    """V (P, E, N) = iK_e R_e in np.longdouble and its magnitude |iK| (|y| + |Phi||w| + sqrt(noise)|xi|)."""
    P, E, N = np.asarray(dr["xi"]).shape
    V, mag = np.empty((P, E, N), LD), np.empty((P, E, N), LD)
    for e in range(E):
        R, m = residual(model, dr, e)
        V[:, e, :] = (np.asarray(iK[e], LD) @ R).T
        mag[:, e, :] = (np.abs(np.asarray(iK[e], LD)) @ m).T
    return V, mag


def kernel_rows(model, e, xu):
    """k_e(xu, X) (P, N) in np.longdouble."""
    X, xu = np.asarray(model["X"], LD), np.asarray(xu, LD)
    d = (xu[:, None, :] - X[None, :, :]) / np.asarray(model["lengthscales"], LD)[e][None, None, :]
    return LD(model["variance"][e]) * np.exp(LD(-0.5) * (d * d).sum(axis=2))


def f_of(model, dr, v, xu):
    """f (P, E) of particle p's function at its own point xu[p] (P, D), in np.longdouble; the magnitudes
    sum_l |w_l phi_l| + sum_i |k_i v_i| (P, E) and A sum_l |w_l| (sum_d |omega_ld x_d| + |b_l|) (P, E)."""
    P, E = np.asarray(dr["w"]).shape[:2]
    f, m1, m2 = np.empty((P, E), LD), np.empty((P, E), LD), np.empty((P, E), LD)
    for e in range(E):
        phi, mag = features(dr["omega"][e], dr["phase"][e], model["variance"][e], xu)
        w, ve = np.asarray(dr["w"], LD)[:, e, :], np.asarray(v, LD)[:, e, :]
        k = kernel_rows(model, e, xu)
        A = np.sqrt(LD(2.0) * LD(model["variance"][e]) / LD(phi.shape[1]))
        f[:, e] = (w * phi).sum(axis=1) + (k * ve).sum(axis=1)
        m1[:, e] = np.abs(w * phi).sum(axis=1) + np.abs(k * ve).sum(axis=1)
        m2[:, e] = A * (np.abs(w) * mag).sum(axis=1)
    return f, m1, m2


def step(model, policy, dr, v, x):
    """One noiseless step of every particle on its own function: x (P, E) -> x' (P, E) in float64, and (f, m1, m2, u)."""
    x = np.asarray(x, np.float64)
    u = pr.action(policy, x)
    f, m1, m2 = f_of(model, dr, v, np.concatenate([x, u], axis=1))
    return (np.asarray(x, LD) + f).astype(np.float64), f, m1, m2, u


def step_bound(model, L, f_m1, f_m2, xn):
    """The teacher-forced bound of docs/particle_functions.md ("The constant c")."""
    N, D = np.asarray(model["X"]).shape
    c = max(N, L) + 3 + 3 * D + 16
    eps = 2.0 ** -53
    return (eps * (c * f_m1 + (D + 2) * f_m2) + 4 * eps * np.abs(np.asarray(xn, LD))).astype(np.float64)


# ------------------------------------------------------------------ closed forms over (w, xi)
def closed_form(model, omega, phase_, xs):
    """At the points xs (n, D): posterior mean k*^T beta (n, E) and the variance of f_p(x) over (w, xi),
    |phi(x) - Phi(X)^T iK k*|^2 + noise |iK k*|^2 (n, E) -- the posterior variance of the L-feature prior."""
    X, Y = np.asarray(model["X"], np.float64), np.asarray(model["Y"], np.float64)
    n, E = np.asarray(xs).shape[0], Y.shape[1]
    mean, var = np.empty((n, E)), np.empty((n, E))
    for e in range(E):
        K = se_ard(X, X, model["lengthscales"][e], model["variance"][e]) + model["noise"][e] * np.eye(X.shape[0])
        ks = se_ard(np.asarray(xs, np.float64), X, model["lengthscales"][e], model["variance"][e])   # (n, N)
        a = np.linalg.solve(K, ks.T)                                                               # iK k*  (N, n)
        mean[:, e] = a.T @ Y[:, e]
        phix = features(omega[e], phase_[e], model["variance"][e], X)[0].astype(np.float64)       # (N, L)
        phis = features(omega[e], phase_[e], model["variance"][e], xs)[0].astype(np.float64)      # (n, L)
        var[:, e] = ((phis - a.T @ phix) ** 2).sum(axis=1) + model["noise"][e] * (a ** 2).sum(axis=0)
    return mean, var


def sample_f(model, dr, xs):
    """f_p at the SAME points xs (n, D) for every particle: (P, n, E) float64 (host linear algebra; statistics only)."""
    X, Y = np.asarray(model["X"], np.float64), np.asarray(model["Y"], np.float64)
    P, E = np.asarray(dr["w"]).shape[:2]
    out = np.empty((P, np.asarray(xs).shape[0], E))
    for e in range(E):
        K = se_ard(X, X, model["lengthscales"][e], model["variance"][e]) + model["noise"][e] * np.eye(X.shape[0])
        phix = features(dr["omega"][e], dr["phase"][e], model["variance"][e], X)[0].astype(np.float64)
        phis = features(dr["omega"][e], dr["phase"][e], model["variance"][e], xs)[0].astype(np.float64)
        ks = se_ard(np.asarray(xs, np.float64), X, model["lengthscales"][e], model["variance"][e])
        w, xi = dr["w"][:, e, :], dr["xi"][:, e, :]
        R = Y[:, e][:, None] - phix @ w.T - math.sqrt(model["noise"][e]) * xi.T        # (N, P)
        out[:, :, e] = (phis @ w.T + ks @ np.linalg.solve(K, R)).T
    return out
