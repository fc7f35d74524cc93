"""The GP posterior at deterministic test points and its input Jacobians on the MI355X (csrc/predict.hip, csrc/predict_jac.hip,
k_gram) at the edge hyper-parameters and test points of helpers/predict_cases.py, against the 40-digit truth of
tests/golden/predict_edges.npz: per entry |device - truth| <= K unit with K under the fixture's cap of the case's class and block
(helpers/predict_edges_reference.py; tests/test_predict_edges_cpu.py holds the yardstick).  docs/predict_edges.md.
Every measured K is printed before it is asserted (pytest -s)."""
import numpy as np
import pytest

from helpers import predict_cases as pc
from helpers import predict_edges_reference as pr

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


def _load(d, Z=None):
    """The case's model into the slot, through the C boundary (a noise of 1e-10 is legal there)."""
    _CTX.gp_set_data(SLOT, d["X"], d["Y"])
    _CTX.gp_set_inducing(SLOT, Z)
    _CTX.gp_set_hyp(SLOT, d["ls"], d["var"], d["noise"])


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _single(c):
    return 1 if c["E"] > 1 else 0


@pytest.mark.parametrize("c", pc.CASES, ids=pc.case_ids())
def test_values_and_jacobians_at_the_edges(c):
    d, truths = pr.case(c)
    D, E, xs, z = c["D"], c["E"], d["xs"], d["zeros"]
    _load(d, d["Z"][0] if c["M"] else None)
    for tn, fx in truths.items():
        Za = d["Z"] if tn == "to" else None
        val = _CTX.gp_predict_points(SLOT, xs, D, E, Z_all=Za)
        jac = _CTX.gp_predict_points_jac(SLOT, xs, D, E, Z_all=Za)
        k = pc.ks(jac, fx)
        caps = {b: pr.cap_of(c, b) for b in pc.BLOCKS}
        print("FIGURE K %-18s %-2s %-24s %s | caps %s" % (c["name"], tn, c["cls"], " ".join("%9.3g" % k[b] for b in pc.BLOCKS),
                                                        " ".join("%9.3g" % caps[b] for b in pc.BLOCKS)))
        assert all(np.all(np.isfinite(r)) for r in jac), (c["name"], tn)
        assert _same(val, jac[:2]), (c["name"], tn, "the Jacobian call's values are not the value call's")
        # the declared zeros are exact
        assert np.all(jac[0][z[:, :, 0]] == 0.0) and np.all(jac[2][z[:, :, 2]] == 0.0) and np.all(jac[3][z[:, :, 3]] == 0.0), (c["name"], tn)
        assert np.all((jac[1] == d["var"][:, None])[z[:, :, 1]]), (c["name"], tn)
        assert all(k[b] <= caps[b] for b in pc.BLOCKS), (c["name"], tn, k, caps)
        # run to run, every point alone, one output alone: the same bits
        assert _same(jac, _CTX.gp_predict_points_jac(SLOT, xs, D, E, Z_all=Za)) and _same(val, _CTX.gp_predict_points(SLOT, xs, D, E, Z_all=Za))
        for t in range(len(xs)):
            one = _CTX.gp_predict_points_jac(SLOT, xs[t:t + 1], D, E, Z_all=Za)
            assert _same([r[:, t] for r in jac], [r[:, 0] for r in one]), (c["name"], tn, t)
            assert _same([r[:, t] for r in val], [r[:, 0] for r in _CTX.gp_predict_points(SLOT, xs[t:t + 1], D, E, Z_all=Za)]), (c["name"], tn, t)
        o = _single(c)
        assert _same([r[o:o + 1] for r in jac], _CTX.gp_predict_points_jac(SLOT, xs, D, E, output=o, Z_all=Za)), (c["name"], tn)
        assert _same([r[o:o + 1] for r in val], _CTX.gp_predict_points(SLOT, xs, D, E, output=o, Z_all=Za)), (c["name"], tn)


def _set_hyp(model, d):
    for i, mdl in enumerate(model.models):
        mdl.kernel.lengthscales.assign(d["ls"][i])
        mdl.kernel.variance.assign(d["var"][i])
        mdl.likelihood.variance.assign(d["noise"][i])
    return model


PY_CASES = [c for c in pc.CASES if c["data"] in ("x24", "f10") and c["fam"] != "noise_m10"]   # (1e-10 is below the models' floor)


@pytest.mark.parametrize("c", PY_CASES, ids=pc.case_ids(PY_CASES))
def test_python_layer_has_the_bits_of_the_context_call(c):
    from pilco_amd.models import MGPR, SMGPR
    d, _ = pr.case(c)
    D, E, xs = c["D"], c["E"], d["xs"]
    _load(d, d["Z"][0] if c["M"] else None)
    want = _CTX.gp_predict_points_jac(SLOT, xs, D, E, Z_all=d["Z"] if c["M"] else None)
    if c["M"]:
        m = _set_hyp(SMGPR((d["X"], d["Y"]), num_induced_points=c["M"], ctx=_CTX), d)
        for mdl, Z in zip(m.models, d["Z"]):
            mdl.inducing_variable.Z.assign(Z)
    else:
        m = _set_hyp(MGPR((d["X"], d["Y"]), ctx=_CTX), d)
    mean, var, dmean, dvar = (np.asarray(r) for r in m.predict_f_jacobian(xs))
    assert _same(want, (mean.T, var.T, dmean.transpose(1, 0, 2), dvar.transpose(1, 0, 2))), c["name"]
    mf, vf = (np.asarray(r) for r in m.predict_f(xs))
    my, vy = (np.asarray(r) for r in m.predict_y(xs))
    assert np.array_equal(mf, mean) and np.array_equal(vf, var) and np.array_equal(my, mf), c["name"]
    assert np.array_equal(vy, vf + d["noise"][None, :]), c["name"]


ROLL_CASES = [c for c in pc.CASES if c["data"] == "x24"]


@pytest.mark.parametrize("c", ROLL_CASES, ids=pc.case_ids(ROLL_CASES))
def test_one_step_particle_rollout_sees_the_same_posterior(c):
    """A D = E = 3 model from the case (a third output from the two: y0 - y1, output 0's lengthscales reversed), its test points as
    the initial particles, no controller, the draws given: x' = (x + mu) + sqrt(max(v, 0)) eps with (mu, v) of the value call.
    The device rounds x + mu, the product and the last sum (or fuses the last two); so does the comparison: they differ by at
    most one rounding of each, 4 x 2^-53 (|x| + |mu| + |sd eps|)."""
    from pilco_amd import _lib
    d, _ = pr.case(c)
    E = D = c["D"]
    x0 = d["xs"]
    m3 = dict(X=d["X"], Y=np.column_stack([d["Y"], d["Y"][:, 0] - d["Y"][:, 1]]), ls=np.vstack([d["ls"], d["ls"][:1, ::-1]]),
              var=np.append(d["var"], d["var"][0] * 3.0), noise=np.append(d["noise"], d["noise"][1] * 2.0))
    _load(m3)
    mu, v = _CTX.gp_predict_points(SLOT, x0, D, E)
    eps = np.random.RandomState(11).randn(1, len(x0), E)
    policy = dict(kind=_lib.POLICY_NONE, state_dim=E, control_dim=0)
    terms = [dict(kind=_lib.REWARD_EXPONENTIAL, coef=1.0, W=np.eye(E), t=None)]
    parts = _CTX.rollout_particles(policy, terms, x0, 1, eps=eps, want_particles=True)[3]
    assert np.array_equal(parts[0], x0)
    sd = np.sqrt(np.maximum(v.T, 0.0)) * eps[0]
    want = (x0 + mu.T) + sd
    err = np.abs(parts[1] - want)
    bound = 4.0 * pc.EPS * (np.abs(x0) + np.abs(mu.T) + np.abs(sd))
    print("FIGURE rollout %-18s worst error over its bound %.3g" % (c["name"], np.max(err / np.maximum(bound, pc.TINY))))
    assert np.all(np.isfinite(parts[1])) and np.all(err <= bound), (c["name"], err.max())
    far = pc.point_kinds(c).index("far40")
    assert np.all(mu[:, far] == 0.0) and np.array_equal(v[:, far], m3["var"])     # mean exactly 0, variance exactly sf2
