"""NumPy restatement of the pathwise gradient of the FUNCTION-sample particle return (pilco_rollout_particles_fn_grad /
_grad_rbf, csrc/particles_fn_grad.hip; docs/particle_fn_gradients.md) -- the yardstick of tests/test_gpu_particle_fn_grad.py,
itself pinned to torch autograd in tests/test_particle_fn_grad_cpu.py.  Built from helpers/particle_fn_restatement.py (the
features, the kernel rows, the step) and the policy adjoints, reward gradients and recursion of
helpers/particle_grad_restatement.py; it shares no code with the kernels.

With z = [x, u], u = action(x), A_e = sqrt(2 var_e / L), k_i = exp(-1/2 sum_d ((z_d - X_id) / l_ed)^2):
  d f_pe / d z_d = -A_e sum_l w_pel sin(omega_el . z + b_el) omega_eld - var_e sum_i k_i v_pei (z_d - X_id) / l_ed^2
  A[e, d] = [e == d] + d f_pe / d z_d          (t < H - 1; additive observation noise does not enter)
and the recursion of particle_grad_restatement.reverse on these matrices.  SINE_SIGN, USE_OMEGA, LS_POWER, USE_AMP and
USE_DELTA exist for the mutant guard of tests/test_particle_fn_grad_cpu.py only."""
import numpy as np

from helpers import particle_fn_restatement as rf
from helpers import particles_restatement as pr
from helpers.particle_grad_restatement import _PolicyAdj, policy_scale, reward_grad, sine_arguments

LD = np.longdouble
SINE_SIGN = -1.0    # d cos = -sin: a mutant flips it
USE_OMEGA = True    # the chain rule's omega_ld: a mutant drops it
LS_POWER = 2        # (z_d - X_id) / l^2: a mutant writes 1 / l
USE_AMP = True      # A_e = sqrt(2 var_e / L): a mutant drops it
USE_DELTA = True    # x' = x + f: the identity block: a mutant drops it

# The kernel's count of rounding steps per term of a Jacobian sum (docs/particle_fn_gradients.md, "The constant c'"), read off
# fn_step_body before anything was measured: the count c of the value sums (docs/particle_functions.md) and six more
EXTRA_ROUNDINGS = 6


def c_prime(N, L, D):
    return max(N, L) + 3 + 3 * D + 16 + EXTRA_ROUNDINGS


def jacobian_fn(model, dr, v, xu):
    """d f_p / d z (P, E, D) of particle p's function at its own point xu[p] (P, D), the sums in np.longdouble, and the two
    magnitudes of the bound (P, E, D):  m1 = sum_l |A w_l sin(.) omega_ld| + sum_i |var k_i v_i (z_d - X_id) / l_d^2|,
    m2 = sum_l |A w_l omega_ld| (sum_d |omega_ld z_d| + |b_l|)."""
    X = np.asarray(model["X"], LD)
    xu = np.asarray(xu, LD)
    P, E = np.asarray(dr["w"]).shape[:2]
    D = X.shape[1]
    dF, m1, m2 = np.empty((P, E, D), LD), np.empty((P, E, D), LD), np.empty((P, E, D), LD)
    diff = xu[:, None, :] - X[None, :, :]                                    # (P, N, D)
    for e in range(E):
        om, ph = np.asarray(dr["omega"][e], LD), np.asarray(dr["phase"][e], LD)
        L = om.shape[0]
        w, ve = np.asarray(dr["w"], LD)[:, e, :], np.asarray(v, LD)[:, e, :]
        arg = xu @ om.T + ph[None, :]                                        # (P, L)
        mag = np.abs(xu) @ np.abs(om).T + np.abs(ph)[None, :]
        amp = np.sqrt(LD(2.0) * LD(model["variance"][e]) / LD(L)) if USE_AMP else LD(1.0)
        chain = om[None, :, :] if USE_OMEGA else np.ones((1, L, D), LD)
        t1 = (LD(SINE_SIGN) * amp * w * np.sin(arg))[:, :, None] * chain      # (P, L, D)
        k = rf.kernel_rows(model, e, xu)                                     # (P, N), the variance inside
        ls = np.asarray(model["lengthscales"], LD)[e]
        t2 = -(k * ve)[:, :, None] * diff / (ls ** LS_POWER)[None, None, :]   # (P, N, D)
        dF[:, e, :] = t1.sum(axis=1) + t2.sum(axis=1)
        m1[:, e, :] = np.abs(t1).sum(axis=1) + np.abs(t2).sum(axis=1)
        m2[:, e, :] = ((amp * np.abs(w) * mag)[:, :, None] * np.abs(om)[None, :, :]).sum(axis=1)
    return dF, m1, m2


def step_matrix_fn(model, policy, dr, v, x, magnitudes=False):
    """A (P, E, D) in float64 at the states x (P, E): [e == d] + d f_pe / d z_d at z = [x, action(x)].  magnitudes: also
    (m1, m2) of jacobian_fn."""
    x = np.asarray(x, np.float64)
    E = x.shape[1]
    dF, m1, m2 = jacobian_fn(model, dr, v, np.concatenate([x, pr.action(policy, x)], axis=1))
    if USE_DELTA:
        dF = dF.copy()
        dF[:, np.arange(E), np.arange(E)] += LD(1.0)
    A = dF.astype(np.float64)
    return (A, m1.astype(np.float64), m2.astype(np.float64)) if magnitudes else A


def reverse_fn(policy, terms, xs, mats):
    """The recursion of particle_grad_restatement.reverse on SUPPLIED matrices: xs (H or H+1, P, E) the states, mats the H - 1
    step matrices (P, E, D) of t = 0 .. H-2 (H = len(mats) + 1; for H = 0 pass xs of length 0 or 1 and use value 0).
    -> (grads, dx0 (P, E))."""
    xs = np.asarray(xs, np.float64)
    H = len(mats) + 1
    P, E = xs.shape[1:]
    adj = _PolicyAdj(policy)
    scale = policy_scale(policy)
    lam = np.zeros((P, E))
    for t in range(H - 1, -1, -1):
        x = xs[t]
        if t < H - 1:
            A = mats[t]
            gu = np.einsum("ped,pe->pd", A[:, :, E:], lam)
            ds = gu * scale * np.cos(sine_arguments(policy, x))
            lam = np.einsum("ped,pe->pd", A[:, :, :E], lam) + adj.step(x, ds)
        lam = lam + reward_grad(terms, x)
    return adj.finish(P), lam


def reverse_on(model, policy, terms, dr, v, xs, H):
    """reverse_fn on the restatement's own matrices at the GIVEN states xs (>= H, P, E).  H = 0: zeros."""
    xs = np.asarray(xs, np.float64)
    if H == 0:
        return tuple(np.zeros_like(g) for g in _PolicyAdj(policy).finish(1)), np.zeros(xs.shape[1:])
    mats = [step_matrix_fn(model, policy, dr, v, xs[t]) for t in range(H - 1)]
    return reverse_fn(policy, terms, xs[:H], mats)


def forward_fn(model, policy, terms, dr, v, x0, H, eps=None):
    """xs (H+1, P, E) and J = sum_t mean_p r(x_t^p) over the pre-step states, by particle_fn_restatement.step; eps (H, P, E):
    the observation noise sqrt(noise_e) eps added to every step."""
    xs, J = [np.asarray(x0, np.float64)], 0.0
    for t in range(H):
        J += pr.reward(terms, xs[-1]).mean()
        xn = rf.step(model, policy, dr, v, xs[-1])[0]
        if eps is not None:
            xn = xn + np.sqrt(np.asarray(model["noise"], np.float64))[None, :] * np.asarray(eps[t], np.float64)
        xs.append(xn)
    return np.stack(xs), J


def reverse_bound_fn(model, policy, terms, dr, v, xs, H):
    """Bounds (the structure of reverse_fn's results) on |device - restatement| for a sweep on the SAME states and draws, and
    the absolute-sum scale of every quantity: the first-order propagation of particle_grad_restatement.reverse_bound with the
    per-entry bound of A counted from the kernel,
      |dA[e, d]| <= 2^-53 [c' m1[e, d] + (D + 2) m2[e, d]],      c' = c_prime(N, L, D)."""
    xs = np.asarray(xs, np.float64)
    P, E = xs.shape[1:]
    N, D = np.asarray(model["X"]).shape
    L = np.asarray(dr["omega"]).shape[1]
    u53 = 2.0 ** -53
    bnd, scl = _PolicyAdj(policy, absolute=True), _PolicyAdj(policy, absolute=True)
    scale = np.abs(policy_scale(policy))
    lam, dlam, slam = np.zeros((P, E)), np.zeros((P, E)), np.zeros((P, E))
    for t in range(H - 1, -1, -1):
        x = xs[t]
        if t < H - 1:
            A, m1, m2 = step_matrix_fn(model, policy, dr, v, x, magnitudes=True)
            dA = u53 * (c_prime(N, L, D) * m1 + (D + 2) * m2)
            cs = scale * np.cos(sine_arguments(policy, x))
            c, aA = np.abs(cs), np.abs(A)
            dds = c * (np.einsum("ped,pe->pd", aA[:, :, E:], dlam) + np.einsum("ped,pe->pd", dA[:, :, E:], np.abs(lam)))
            sds = c * np.einsum("ped,pe->pd", aA[:, :, E:], slam)
            ds = cs * np.einsum("ped,pe->pd", A[:, :, E:], lam)
            dlam = np.einsum("ped,pe->pd", aA[:, :, :E], dlam) + np.einsum("ped,pe->pd", dA[:, :, :E], np.abs(lam)) + bnd.step(x, dds)
            slam = np.einsum("ped,pe->pd", aA[:, :, :E], slam) + scl.step(x, sds)
            lam = np.einsum("ped,pe->pd", A[:, :, :E], lam) + _PolicyAdj(policy).step(x, ds)
        lam = lam + reward_grad(terms, x)
        slam = slam + np.abs(reward_grad(terms, x))
    return (bnd.finish(P), dlam), (scl.finish(P), slam)
