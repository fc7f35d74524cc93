"""The models, policies, rewards and shapes of the particle-gradient tests: what tests/test_gpu_particle_grad.py runs on the
device and tests/test_particle_grad_cpu.py checks the input condition of (the propagated bound stays below 1e-5 of every
quantity's absolute-sum scale) under the restatement alone.  The models are those of tests/test_gpu_particles.py."""
import os

import numpy as np

from pilco_amd import synthetic

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden")
_CACHE = {}


def _g(name):
    return np.load(os.path.join(GOLDEN, name))


def setup(name):
    """-> dict(cfg, Z, W, b, maxact, rbf (the rbf_controller.npz arrays or None), model, policy, terms, m0, S0): model, policy
    and terms as helpers/particles_restatement.py takes them."""
    if name in _CACHE:
        return _CACHE[name]
    Z = rbf = W = b = maxact = None
    if name == "predictions":          # tests/golden/predictions.npz: state 2 + 1 control, linear
        g = _g("predictions.npz")
        cfg = {k: g[k] for k in ("X", "Y", "lengthscales", "variance", "noise")}
        W, b, maxact = np.array([[0.7, -0.4]]), np.array([[0.15]]), 1.3
        m0, S0 = cfg["X"][:1, :2], 0.05 * np.eye(2)
    elif name == "fitc":               # tests/golden/sparse_predictions.npz: FITC on 30 shared inducing inputs, linear
        g = _g("sparse_predictions.npz")
        cfg = {k: g[k] for k in ("X", "Y", "lengthscales", "variance", "noise")}
        Z = g["Z"]
        W, b, maxact = np.array([[-0.5, 0.6]]), np.array([[-0.1]]), 0.9
        m0, S0 = cfg["X"][:1, :2], 0.05 * np.eye(2)
    elif name == "c2":                 # N = 1000, D = E = 10, no policy
        cfg = synthetic.config_c2(N=1000, D=10, E=10)
        m0, S0 = cfg["m0"], 0.05 * np.eye(10)
    elif name == "c2u":                # the C2u shape: state 10 + 1 control, linear
        cfg = synthetic.config_c2(N=1000, D=11, E=10, control_dim=1)
        W, b, maxact = cfg["W"] * 5.0, cfg["b"] + 0.2, 1.5
        m0, S0 = cfg["m0"], 0.05 * np.eye(10)
    elif name == "rbf":                # an RbfController on the rbf_controller.npz policy (state 3 -> 2 controls), N = 300
        cfg = synthetic.config_c2(N=300, D=5, E=3, control_dim=2, seed=21)
        maxact = 2.0
        m0, S0 = cfg["m0"], 0.05 * np.eye(3)
        rbf = {k: _g("rbf_controller.npz")[k] for k in ("X", "Y", "lengthscales")}
    elif name == "rbfg":               # the same model under a WELL-CONDITIONED RbfController: 27 centres on a grid 2.5 apart with
        # lengthscales 0.8 to 1, so that K + noise I is close to the identity and beta does not cancel.  With the hundred
        # crowded centres of rbf_controller.npz (noise 1e-4) the basis functions cancel against each other, and a first-order
        # bound taken term by term in absolute value comes out larger than the gradient itself: it would check nothing.
        # 27 centres: 5 * 27 + 6 = 141 quantities, more than one pass of the 128 threads that add them.
        import itertools
        cfg = synthetic.config_c2(N=300, D=5, E=3, control_dim=2, seed=21)
        maxact = 2.0
        m0, S0 = cfg["m0"], 0.05 * np.eye(3)
        r = np.random.RandomState(31)
        grid = np.array(list(itertools.product((-2.5, 0.0, 2.5), repeat=3)))
        rbf = dict(X=np.asarray(m0).reshape(1, 3) + grid + 0.1 * r.randn(27, 3), Y=0.5 * r.randn(27, 2),
                   lengthscales=0.8 + 0.2 * r.rand(2, 3))
    else:
        raise KeyError(name)
    E = cfg["Y"].shape[1]
    U = cfg["X"].shape[1] - E
    policy = None
    if rbf is not None:
        policy = dict(kind="rbf", X=rbf["X"], Y=rbf["Y"], lengthscales=rbf["lengthscales"], noise=np.full(U, 1e-4), max_action=maxact)
    elif U > 0:
        policy = dict(kind="linear", W=W, b=b, max_action=maxact)
    model = dict(X=cfg["X"], Y=cfg["Y"], lengthscales=cfg["lengthscales"], variance=cfg["variance"], noise=cfg["noise"], Z=Z)
    # an exponential reward with an ASYMMETRIC weight matrix and a target, and a linear term: combined by coef
    r = np.random.RandomState(11)
    Wr = np.eye(E) + 0.3 * r.randn(E, E) / np.sqrt(E)
    terms = [dict(kind="exponential", W=Wr, t=0.2 * r.randn(E), coef=1.0), dict(kind="linear", W=0.1 * r.randn(E), coef=-0.5)]
    _CACHE[name] = dict(cfg=cfg, Z=Z, W=W, b=b, maxact=maxact, rbf=rbf, model=model, policy=policy, terms=terms,
                        m0=np.asarray(m0, np.float64).reshape(1, E), S0=S0, E=E, U=U)
    return _CACHE[name]


def x0_of(name, P, seed):
    s = setup(name)
    return s["m0"] + np.random.RandomState(seed).randn(P, s["E"]) * np.sqrt(np.diag(s["S0"]))


# (model, P, H, observation_noise): every P of the block and wave edges at H = 2, every H at P = 65, on the odd state width
# (rbfg: E = 3, U = 2); E = 2 / U = 1, E = 10 / U = 1, U = 0 and FITC beside it; one chunk boundary (C2u: 1600 points per chunk)
CASES = [("rbfg", P, 2, False) for P in (1, 63, 64, 65, 127, 128, 129, 257)]
CASES += [("rbfg", 65, H, True) for H in (0, 1, 5)]
CASES += [("predictions", 1, 5, False), ("predictions", 129, 5, True), ("predictions", 64, 1, False)]
CASES += [("fitc", 65, 5, False), ("fitc", 128, 2, True)]
CASES += [("c2", 63, 2, False), ("c2u", 65, 2, True), ("c2u", 1601, 2, False)]
CASE_IDS = ["%s-P%d-H%d-obs%d" % c for c in CASES]
