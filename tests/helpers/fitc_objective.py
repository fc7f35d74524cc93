"""Float64 yardsticks of gpflow GPRFITC's training loss (one output, no priors: smgpr.py sets none), the objective the
device computes in pilco_gp_fitc_nlml (csrc/fitc_train.hip):

  * fitc_loss_and_grad -- torch autograd of the restated bound: the loss and its gradient w.r.t. the lengthscales, the
    kernel variance, the noise variance and the inducing inputs Z.  The CPU stand-in context of the model fits
    (cpu_objective_context.py) and the GPU tests (test_gpu_training_objectives.py) both use it.
  * fitc_loss_np -- the same value in NumPy / SciPy, and fitc_grad_fd its central differences: a route to the gradient
    that does not go through autograd.

tests/test_training_objectives_cpu.py pins both to the executed reference (tests/golden/fitc_objective.npz)."""
import numpy as np
import scipy.linalg as sla
import torch

JITTER = 1e-6   # gpflow default_jitter on Kuu


class NotPositiveDefinite(Exception):
    pass


def fitc_loss_and_grad(X, y, Z, ls, var, noise):
    """-log N(y | 0, Qff + diag(Kff - Qff) + noise I) for one output by the inducing-point identities, and its gradient:
    (loss, dls (D,), dvar, dnoise, dZ (M, D))."""
    X, y = torch.from_numpy(np.asarray(X, np.float64)), torch.from_numpy(np.asarray(y, np.float64))
    ls = torch.tensor(np.asarray(ls, np.float64), requires_grad=True)
    var = torch.tensor(float(var), dtype=torch.float64, requires_grad=True)
    nz = torch.tensor(float(noise), dtype=torch.float64, requires_grad=True)
    Z = torch.tensor(np.asarray(Z, np.float64), requires_grad=True)
    N, M = X.shape[0], Z.shape[0]

    def k(A, B):
        d = (A / ls)[:, None, :] - (B / ls)[None, :, :]
        return var * torch.exp(-0.5 * (d * d).sum(-1))
    try:
        Luu = torch.linalg.cholesky(k(Z, Z) + JITTER * torch.eye(M, dtype=torch.float64))
        V = torch.linalg.solve_triangular(Luu, k(Z, X), upper=False)
        nu = var - (V * V).sum(0) + nz
        L = torch.linalg.cholesky(torch.eye(M, dtype=torch.float64) + (V / nu) @ V.T)
    except torch.linalg.LinAlgError as exc:
        raise NotPositiveDefinite(str(exc)) from exc
    gamma = torch.linalg.solve_triangular(L, (V @ (y / nu))[:, None], upper=False)
    loss = (0.5 * (y * y / nu).sum() - 0.5 * (gamma * gamma).sum() + 0.5 * N * np.log(2 * np.pi)
            + 0.5 * torch.log(nu).sum() + torch.log(torch.diagonal(L)).sum())
    g = torch.autograd.grad(loss, [ls, var, nz, Z])
    return float(loss.detach()), g[0].numpy(), float(g[1]), float(g[2]), g[3].numpy()


def fitc_reference(X, Y, Z_all, lengthscales, variance, noise):
    """fitc_loss_and_grad for every output, in the layout of Context.gp_fitc_nlml: nlml (E), dhyp (E, D + 2), dZ (E, M, D)."""
    E, (M, D) = Y.shape[1], np.shape(Z_all)[1:]
    nlml, gh, gz = np.empty(E), np.empty((E, D + 2)), np.empty((E, M, D))
    for a in range(E):
        nlml[a], gh[a, :D], gh[a, D], gh[a, D + 1], gz[a] = fitc_loss_and_grad(X, Y[:, a], Z_all[a], lengthscales[a], variance[a], noise[a])
    return nlml, gh, gz


def se_ard(A, B, ls, var):
    d = (A[:, None, :] - B[None, :, :]) / np.asarray(ls, np.float64)
    return float(var) * np.exp(-0.5 * np.sum(d * d, axis=-1))


def fitc_loss_np(X, y, Z, ls, var, noise, jitter=JITTER):
    """NumPy restatement of gpflow GPRFITC's negative log marginal likelihood (one output)."""
    N, M = X.shape[0], Z.shape[0]
    Kuf = se_ard(Z, X, ls, var)
    Kuu = se_ard(Z, Z, ls, var) + jitter * np.eye(M)
    Luu = np.linalg.cholesky(Kuu)
    V = sla.solve_triangular(Luu, Kuf, lower=True)
    nu = var - np.sum(V * V, 0) + noise
    B = np.eye(M) + (V / nu) @ V.T
    L = np.linalg.cholesky(B)
    gamma = sla.solve_triangular(L, V @ (y / nu), lower=True)
    f = -0.5 * np.sum(y * y / nu) + 0.5 * gamma @ gamma - 0.5 * N * np.log(2 * np.pi) - 0.5 * np.sum(np.log(nu)) - np.sum(np.log(np.diag(L)))
    return -f


def fitc_grad_fd(X, y, Z, ls, var, noise, rel=1e-5):
    """Central differences of fitc_loss_np with relative steps: (dls (D,), dvar, dnoise, dZ (M, D))."""
    ls, Z = np.array(ls, np.float64), np.array(Z, np.float64)

    def diff(f, x):
        h = rel * max(abs(x), 1e-3)
        return (f(x + h) - f(x - h)) / (2 * h)
    dls = np.empty_like(ls)
    for d in range(ls.size):
        def f(v, d=d):
            l2 = ls.copy()
            l2[d] = v
            return fitc_loss_np(X, y, Z, l2, var, noise)
        dls[d] = diff(f, ls[d])
    dvar = diff(lambda v: fitc_loss_np(X, y, Z, ls, v, noise), float(var))
    dnoise = diff(lambda v: fitc_loss_np(X, y, Z, ls, var, v), float(noise))
    dZ = np.empty_like(Z)
    for i in np.ndindex(Z.shape):
        def f(v, i=i):
            Z2 = Z.copy()
            Z2[i] = v
            return fitc_loss_np(X, y, Z2, ls, var, noise)
        dZ[i] = diff(f, Z[i])
    return dls, dvar, dnoise, dZ
