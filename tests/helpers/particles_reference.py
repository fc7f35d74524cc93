"""What the executed reference says about one particle step (tests/test_particles_cpu.py): PILCO.propagate(x, 0) at single
points -- M - x is the posterior mean at [x, u], diag S the latent variance, the off-diagonals of S vanish -- on the
predictions.npz model (MGPR: "exact"; and "exact_n", the same data and kernels with the likelihood variance EXACT_N_NOISE, a model
on which the reference's own rounding leaves the off-diagonals of S resolvable: tests/test_particles_cpu.py) and the
sparse_predictions.npz model (SMGPR, model 0's Z for every output) under a LinearController, and compute_action(x, 0)[0] of a
LinearController (linear_controller.npz) and an RbfController (rbf_controller.npz).  `python -m helpers.particles_reference` (from tests/, where the reference source is present) writes
these end values to tests/golden/particles_reference.npz."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden")
STORED = os.path.join(GOLDEN, "particles_reference.npz")
NPTS = 6
# the controller of the propagate checks: state 2 -> control 1 (the models of predictions.npz map 3 inputs to 2 outputs)
STEP_W = np.array([[0.7, -0.4]])
STEP_B = np.array([[0.15]])
STEP_MAX_ACTION = 1.3
EXACT_N_NOISE = 0.1
ACTION_MAX = 2.0   # max_action of the two compute_action checks


def points(lo, hi, n, seed):
    rs = np.random.RandomState(seed)
    return lo + (hi - lo) * rs.rand(n, len(lo))


def executed():
    from oracle import ref_exec
    R = ref_exec.load()
    n_ = ref_exec.to_np
    out = {}
    for kind, name in (("exact", "predictions.npz"), ("exact_n", "predictions.npz"), ("sparse", "sparse_predictions.npz")):
        g = np.load(os.path.join(GOLDEN, name))
        X, Y = g["X"], g["Y"]
        E = Y.shape[1]
        ctl = R.controllers.LinearController(E, X.shape[1] - E, max_action=STEP_MAX_ACTION)
        ctl.W.assign(STEP_W)
        ctl.b.assign(STEP_B)
        if kind != "sparse":
            p = R.PILCO((X, Y), controller=ctl)
        else:
            np.random.seed(11)
            p = R.PILCO((X, Y), num_induced_points=g["Z"].shape[0], controller=ctl)
            for m in p.mgpr.models:
                m.inducing_variable.Z.assign(g["Z"])
        for i, m in enumerate(p.mgpr.models):
            m.kernel.lengthscales.assign(g["lengthscales"][i])
            m.kernel.variance.assign(g["variance"][i])
            m.likelihood.variance.assign(EXACT_N_NOISE if kind == "exact_n" else g["noise"][i])
        xs = points(X[:, :E].min(0), X[:, :E].max(0), NPTS, 5)
        Ms, Ss = [], []
        for x in xs:
            M, S = [n_(a) for a in p.propagate(x.reshape(1, E), np.zeros((E, E)))]
            Ms.append(M.ravel())
            Ss.append(S)
        out["x_" + kind], out["M_" + kind], out["S_" + kind] = xs, np.array(Ms), np.array(Ss)
    # compute_action(x, 0)[0]
    g = np.load(os.path.join(GOLDEN, "linear_controller.npz"))
    U, E = g["W"].shape
    ctl = R.controllers.LinearController(E, U, max_action=ACTION_MAX)
    ctl.W.assign(g["W"])
    ctl.b.assign(g["b"])
    xs = points(-2.0 * np.ones(E), 2.0 * np.ones(E), NPTS, 6)
    out["x_linear"] = xs
    out["u_linear"] = np.array([n_(ctl.compute_action(x.reshape(1, E), np.zeros((E, E)))[0]).ravel() for x in xs])
    g = np.load(os.path.join(GOLDEN, "rbf_controller.npz"))
    E, U = g["X"].shape[1], g["Y"].shape[1]
    np.random.seed(3)
    ctl = R.controllers.RbfController(E, U, g["X"].shape[0], max_action=ACTION_MAX)
    for m in ctl.models:
        m.X.assign(g["X"])
    for i, m in enumerate(ctl.models):
        m.Y.assign(g["Y"][:, i:i + 1])
        m.kernel.lengthscales.assign(g["lengthscales"][i])
    xs = points(g["X"].min(0), g["X"].max(0), NPTS, 7)
    out["x_rbf"] = xs
    out["u_rbf"] = np.array([n_(ctl.compute_action(x.reshape(1, E), np.zeros((E, E)))[0]).ravel() for x in xs])
    return out


def reference_values():
    """The executed reference where its source is present (and then the stored values must be its own), the stored end
    values elsewhere."""
    from oracle import ref_exec
    stored = np.load(STORED)
    if not ref_exec.available():
        return {k: stored[k] for k in stored.files}
    live = executed()
    for k, v in live.items():
        np.testing.assert_allclose(stored[k], v, rtol=1e-12, atol=1e-14)
    return live


if __name__ == "__main__":
    np.savez(STORED, **executed())
    print("wrote", STORED)
