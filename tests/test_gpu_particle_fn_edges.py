"""The function-sample particle step on the MI355X (k_particle_fn_step, k_particle_fn_step_jac and the set-up launches of
csrc/particles_fn.hip) at the edge hyper-parameters, particles and widths of helpers/particle_fn_edge_cases.py: the set-up V,
the teacher-forced value step and the step matrix per entry against a 40-digit truth evaluated here from the values the device
returns (helpers/particle_fn_edge_truth.py), |device - truth| <= K unit with K under the fixture's cap of the case's class and
block (helpers/particle_fn_edge_reference.py; tests/test_particle_fn_edges_cpu.py holds the yardstick).
docs/particle_fn_edges.md.  Every measured K is printed before it is asserted (pytest -s)."""
import numpy as np
import pytest

from helpers import particle_fn_edge_cases as ec
from helpers import particle_fn_edge_reference as er
from helpers import particle_fn_edge_truth as et

pytestmark = pytest.mark.gpu
_CTX = None
SLOT = 0


@pytest.fixture(scope="module", autouse=True)
def own_ctx():
    from pilco_amd import _lib
    global _CTX
    _CTX = _lib.Context(device=0)
    yield _CTX
    _CTX.close()


def _load(model):
    _CTX.gp_set_data(SLOT, model["X"], model["Y"])
    _CTX.gp_set_inducing(SLOT, None)
    _CTX.gp_set_hyp(SLOT, model["lengthscales"], model["variance"], model["noise"])


def _spec(c, policy):
    from pilco_amd import _lib
    E = c["E"]
    if policy is None:
        return dict(kind=_lib.POLICY_NONE, state_dim=E, control_dim=0)
    return dict(kind=_lib.POLICY_LINEAR, state_dim=E, control_dim=c["D"] - E, W=policy["W"], b=policy["b"], max_action=policy["max_action"])


def _expo(E):
    from pilco_amd import _lib
    return [dict(kind=_lib.REWARD_EXPONENTIAL, coef=1.0, W=np.eye(E), t=None)]


def _linear(E, a):
    from pilco_amd import _lib
    return [dict(kind=_lib.REWARD_LINEAR, coef=1.0, W=np.eye(E)[a])]


def _forward(c, d, spec, terms, H, draws=None, x0=None):
    kw = dict(function_draws=d["draws"] if draws is None else draws, want_particles=True, want_draws=True)
    if c["obs"]:
        kw.update(observation_noise=True, eps=np.tile(d["eps"], (H, 1, 1))[:H])
    return _CTX.rollout_particles_fn(spec, terms, d["x0"] if x0 is None else x0, H, **kw)


def _matrix(c, d, spec, draws=None, x0=None):
    """G (P, E, E): row a is dreturn_dx0 of the H = 2 call under the linear reward e_a -- row a of the first step's A plus the
    reward's gradient e_a (both exact constants); and the calls' reward_steps."""
    E = c["E"]
    x0 = d["x0"] if x0 is None else x0
    G, steps = np.empty((len(x0), E, E)), []
    for a in range(E):
        g = _CTX.rollout_particles_fn_grad(spec, _linear(E, a), x0, 2, function_draws=d["draws"] if draws is None else draws, want_dx0=True)
        G[:, a, :] = g[4]
        steps.append(g[1])
    return G, steps


def _run(c, x0=None):
    """The device's side of a case (x0: other initial particles): dict(v, iK, xt, parts (2, P, E), rew, G or None)."""
    d = ec.case(c) if x0 is None else dict(ec.case(c), x0=x0)
    _load(d["model"])
    spec = _spec(c, d["policy"])
    res = _forward(c, d, spec, _expo(c["E"]), 1)
    out = dict(v=res[7]["v"], parts=res[3], rew=res[2], draws=res[7], spec=spec, d=d)
    out["iK"] = _CTX.gp_get_factors(SLOT, c["E"])[0]
    u = _CTX.particle_actions(spec, d["x0"]) if d["policy"] is not None else np.empty((c["P"], 0))
    out["xt"] = np.concatenate([d["x0"], u], axis=1)
    out["G"] = None
    if "matrix" in c["blocks"]:
        out["G"], out["steps"] = _matrix(c, d, spec)
    return out


@pytest.mark.parametrize("c", ec.CASES, ids=ec.case_ids())
def test_setup_value_step_and_step_matrix_at_the_edges(c):
    r = _run(c)
    d, E = r["d"], c["E"]
    model, dr = d["model"], d["draws"]
    assert np.array_equal(r["parts"][0], d["x0"])
    got = {"value": r["parts"][1]}
    truth = et.step(model, dr, r["v"], r["xt"], eps=None if d["eps"] is None else d["eps"][0], matrix="matrix" in c["blocks"])
    ks = {"value": ec.k_of(got["value"], truth["xn"], truth["uxn"])}
    if "setup" in c["blocks"]:
        V, uV = et.setup(model, dr, r["iK"])
        got["setup"] = r["v"]
        ks["setup"] = ec.k_of(r["v"], V, uV)
    if "matrix" in c["blocks"]:
        got["matrix"] = r["G"]
        ks["matrix"] = ec.k_of(r["G"], truth["G"][:, :, :E], truth["uG"][:, :, :E])
    caps = {b: er.cap_of(c, b) for b in c["blocks"]}
    print("FIGURE K %-20s %-22s %s" % (c["name"], c["cls"], "  ".join("%s %9.3g (cap %.3g)" % (b, ks[b], caps[b]) for b in c["blocks"])))
    assert all(np.all(np.isfinite(g)) for g in got.values()) and np.all(np.isfinite(r["iK"])), c["name"]
    # the reward of the pre-step state against pilco_reward_eval(x, 0)
    want = np.array([float(np.ravel(_CTX.reward_eval(_expo(E), E, x, np.zeros((E, E)))[0])[0]) for x in d["x0"]])
    assert abs(r["rew"][0] - want.mean()) <= 1e-12 * np.abs(want).max(), (c["name"], r["rew"][0], want.mean())
    # the declared exact results
    far, zero_out = ec.declared(c)
    if far is not None:
        assert np.all(truth["kern"][far] == 0.0), c["name"]
    if zero_out:
        assert not r["v"][:, 0, :].any() and np.array_equal(r["parts"][1][:, 0], d["x0"][:, 0]), c["name"]
        assert np.all(r["G"][:, 0, :] == 2.0 * np.eye(E)[0]), c["name"]
    if "matrix" in c["blocks"]:
        # the gradient calls' rewards have the bits of the forward call on the same reward, and its states are this call's
        for a in range(E):
            fwd = _forward(c, d, r["spec"], _linear(E, a), 2)
            assert np.array_equal(fwd[2], r["steps"][a]) and np.array_equal(fwd[3][1], r["parts"][1]), (c["name"], a)
    assert all(ks[b] <= caps[b] for b in c["blocks"]), (c["name"], ks, caps)


def test_the_far_particle_moves_by_the_feature_half_alone():
    """Every kernel value at far40 is exactly 0, so the kernel half adds nothing whatever V holds: std and y1e6 (the same inputs,
    lengthscales and draws; targets and so V a million times apart) give the far particle the same x' and the same row of A bit
    for bit, and so does y0 on the outputs whose draws it shares."""
    std = ec.by_name("x24_std")
    runs = {f: _run(ec.by_name("x24_" + f), x0=ec.case(std)["x0"]) for f in ("std", "y1e6", "y0")}     # (std's particles for all three)
    far = ec.declared(std)[0]
    a, b, z = runs["std"], runs["y1e6"], runs["y0"]
    assert not np.array_equal(a["v"][far], b["v"][far])
    assert np.array_equal(a["parts"][1][far], b["parts"][1][far]) and np.array_equal(a["G"][far], b["G"][far])
    assert np.array_equal(a["parts"][1][far, 1:], z["parts"][1][far, 1:]) and np.array_equal(a["G"][far, 1:], z["G"][far, 1:])
    assert not np.array_equal(a["parts"][1][:far], b["parts"][1][:far])           # (near the data V matters)


@pytest.mark.parametrize("name", ["x24_ls_ard", "x24_var_huge"])
def test_bit_contracts_at_the_edges(name):
    """Every call repeats its bits, the returned draws fed back reproduce them, and a particle alone -- the far one among
    them -- has the bits it has among the seven."""
    c = ec.by_name(name)
    r, again = _run(c), _run(c)
    d = r["d"]
    for k in ("v", "parts", "rew", "G", "iK"):
        assert np.array_equal(r[k], again[k]), (name, k)
    back = _forward(c, d, r["spec"], _expo(c["E"]), 1, draws=r["draws"])
    assert np.array_equal(back[3], r["parts"]) and np.array_equal(back[7]["v"], r["v"]) and np.array_equal(back[2], r["rew"])
    assert np.array_equal(_matrix(c, d, r["spec"], draws=r["draws"])[0], r["G"])
    for q in range(c["P"]):
        own = dict(d["draws"], w=d["draws"]["w"][q:q + 1], xi=d["draws"]["xi"][q:q + 1])
        one = _forward(c, d, r["spec"], _expo(c["E"]), 1, draws=own, x0=d["x0"][q:q + 1])
        assert np.array_equal(one[3][:, 0], r["parts"][:, q]) and np.array_equal(one[7]["v"][0], r["v"][q]), (name, q)
        assert np.array_equal(_matrix(c, d, r["spec"], draws=own, x0=d["x0"][q:q + 1])[0][0], r["G"][q]), (name, q)
