"""The models, policies, rewards and shapes of the function-sample gradient tests: what tests/test_gpu_particle_fn_grad.py runs
on the device and tests/test_particle_fn_grad_cpu.py checks the input conditions of under the restatement alone.  The models
are those of tests/test_gpu_particle_fn.py (predictions, the N = 300 model, syn1 / syn65 / syn100) under the rewards of
helpers/particle_grad_cases.py and, for the N = 300 model, its well-conditioned RbfController rbfg (the reason is written
there); and one synthetic model per input width at the edges of the step kernel's register builds."""
import numpy as np

from helpers import particle_grad_cases as pgc
from pilco_amd import synthetic

_CACHE = {}
WIDTHS = (3, 4, 7, 8, 11, 12, 15, 16, 23, 24, 31, 32)    # D: every register build (4, 8, 12, 16, 24, 32) and the width below it


def _terms(E):
    r = np.random.RandomState(11)
    Wr = np.eye(E) + 0.3 * r.randn(E, E) / np.sqrt(E)
    return [dict(kind="exponential", W=Wr, t=0.2 * r.randn(E), coef=1.0), dict(kind="linear", W=0.1 * r.randn(E), coef=-0.5)]


def setup(name):
    """-> dict(cfg, W, b, maxact, rbf, model, policy, terms, m0, S0, E, U) as helpers/particle_grad_cases.setup."""
    if name in _CACHE:
        return _CACHE[name]
    if name == "predictions":
        s = pgc.setup("predictions")
    elif name == "rbf":                     # the N = 300 model under the well-conditioned controller
        s = pgc.setup("rbfg")
    elif name.startswith("syn") or name.startswith("w"):
        if name.startswith("syn"):          # N in {1, 65, 100}, state 3, no policy
            cfg = synthetic.config_c2(N=int(name[3:]), D=3, E=3, seed=33)
            W = b = maxact = policy = None
        else:                               # N = 65, D inputs of which one is a control, a LinearController
            D = int(name[1:])
            cfg = synthetic.config_c2(N=65, D=D, E=D - 1, control_dim=1, seed=50 + D)
            W, b, maxact = cfg["W"] * 3.0, cfg["b"] + 0.1, 1.2
            policy = dict(kind="linear", W=W, b=b, max_action=maxact)
        E = cfg["Y"].shape[1]
        model = dict(X=cfg["X"], Y=cfg["Y"], lengthscales=cfg["lengthscales"], variance=cfg["variance"], noise=cfg["noise"], Z=None)
        s = dict(cfg=cfg, Z=None, W=W, b=b, maxact=maxact, rbf=None, model=model, policy=policy, terms=_terms(E),
                 m0=np.asarray(cfg["m0"], np.float64).reshape(1, E), S0=0.05 * np.eye(E), E=E, U=cfg["X"].shape[1] - E)
    else:
        raise KeyError(name)
    _CACHE[name] = s
    return s


def x0_of(name, P, seed):
    s = setup(name)
    return s["m0"] + np.random.RandomState(seed).randn(P, s["E"]) * np.sqrt(np.diag(s["S0"]))


# (model, P, L, H, observation_noise): every P of the wave, workgroup and block edges at H = 2 on the odd state width (E = 3,
# U = 2, an RbfController); every H beside it; E = 2 / U = 1; N = 1, 65 (a second tile of one point), 100 without a policy; L at
# 1, below, at and above a tile; then every register build
CASES = [("rbf", P, 100, 2, False) for P in (1, 63, 64, 65, 127, 128, 129, 257)]
CASES += [("rbf", 65, 63, H, True) for H in (0, 1, 5)]
CASES += [("predictions", 1, 1, 5, False), ("predictions", 129, 64, 5, True), ("predictions", 64, 100, 1, False)]
CASES += [("syn1", 65, 64, 3, False), ("syn65", 65, 65, 3, True), ("syn100", 129, 100, 4, False)]
CASES += [("w%d" % D, 65, 65, 2, False) for D in WIDTHS]
CASE_IDS = ["%s-P%d-L%d-H%d-obs%d" % c for c in CASES]
