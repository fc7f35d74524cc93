"""Edge hyper-parameters, particles and draws of the function-sample particle step (k_particle_fn_step, k_particle_fn_step_jac
and the set-up launches of csrc/particles_fn.hip): one table for tests/test_particle_fn_edges_cpu.py (conditions, coverage
guard, K_ref, caps, sensitivity), oracle/gen_golden_particle_fn_edges.py (tests/golden/particle_fn_edges.npz: inputs, draws and
caps) and tests/test_gpu_particle_fn_edges.py.  docs/particle_fn_edges.md describes it.

Plain data.  Three kinds of case:
  table   the data sets x24 / x65 and the families of helpers/predict_cases.py as the D = E = 3 no-policy model of
          tests/test_gpu_predict_edges.py (a third output y0 - y1 with output 0's lengthscales reversed), or -- policy "lin0",
          "linW" -- the data set's own E = 2 outputs with the third input a LinearController's action; the particles are the
          seven kinds of test point of predict_cases (P = 65: cycled, with offsets); all three blocks (no Jacobian with a policy)
  width   helpers/particle_fn_grad_cases.setup("w<D>"): N = 65, std hyper-parameters, D on both sides of every register build;
          the value step only
  bigL    x65_std at P = 1 with L = 128, 129, 4096 features; the value step only
The draws of a table case come from the fixture (normals of the stream restatement, seed SEED; omega = z / lengthscale is
formed here); a width or bigL case regenerates its draws from SEED with the stream restatement.  noise_m10 (1e-10) is below
what a model may carry and below what the path needs: it is not in the table."""
from __future__ import annotations

import os

import numpy as np

from helpers import particle_fn_restatement as rf
from helpers import predict_cases as pc

BLOCKS = ("setup", "value", "matrix")
FAMS = tuple(f for f in pc.FAMILIES if f != "noise_m10")
ILL = ("noise_floor", "flat_floor", "dup")
WIDTHS = (4, 5, 8, 9, 12, 13, 16, 17, 24, 25, 32)
BIG_L = (128, 129, 4096)
SEED = 20261020
PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "particle_fn_edges.npz")
POLICIES = {"lin0": dict(W=[[0.0, 0.0]], b=[0.0], max_action=1.0), "linW": dict(W=[[0.7, -0.4]], b=[0.15], max_action=1.3)}


def _t(name, data, fam, **kw):
    c = dict(name=name, kind="table", data=data, fam=fam, policy=None, P=7, L=65, obs=False, zero_w0=False,
             N=pc.DATA[data][0], D=3, E=3, blocks=BLOCKS)
    c.update(kw)
    if c["policy"]:
        c.update(E=2, blocks=BLOCKS[:2])
    c["cls"] = "%s_%s" % (data, fam) + ("_ctl" if c["policy"] else "")
    return c


CASES = [_t("x24_" + f, "x24", f) for f in FAMS] + [_t("x65_" + f, "x65", f) for f in ILL]
CASES += [_t("x24_std_P65", "x24", "std", P=65), _t("x24_std_L1", "x24", "std", L=1),
          _t("x24_std_w0", "x24", "std", zero_w0=True)]      # (output 0 without a feature half: the kernel half of A stands alone)
CASES += [_t("x24_%s_obs" % f, "x24", f, obs=True, blocks=BLOCKS[:2]) for f in ("noise_floor", "noise_dom")]
CASES += [_t("x24_%s_%s" % (f, p), "x24", f, policy=p) for f in ("std", "ls_ard") for p in POLICIES]
CASES += [dict(name="w%d" % D, kind="width", data="w%d" % D, fam="std", policy="w", P=2, L=65, obs=False, N=65, D=D, E=D - 1,
               blocks=("value",), cls="width") for D in WIDTHS]
CASES += [dict(name="x65_std_L%d" % L, kind="bigL", data="x65", fam="std", policy=None, P=1, L=L, obs=False, N=65, D=3, E=3,
               blocks=("value",), cls="x65_std_bigL") for L in BIG_L]


def case_ids(cases=None):
    return [c["name"] for c in (CASES if cases is None else cases)]


def by_name(name):
    return next(c for c in CASES if c["name"] == name)


def draw_key(c):
    return "_draws/E%d_D%d_L%d_P%d_N%d" % (c["E"], c["D"], c["L"], c["P"], c["N"])


def pc_case(c):
    """The predict_cases case whose hyper-parameters and data the table case uses."""
    return pc._c("%s_%s" % (c["data"], c["fam"]), c["data"], c["fam"])


# ------------------------------------------------------------------ the coverage guard
def dims_of(c):
    d = {"fam:" + c["fam"], "D:%d" % c["D"], "L:%d" % c["L"], "P:%d" % c["P"]}
    if c["kind"] != "width":
        d |= {"pt:" + k for k in (pc.POINT_KINDS if c["kind"] == "table" else ("half",))}
    if c["obs"]:
        d.add("obs:" + c["fam"])
    if c["policy"] in POLICIES:
        d.add("policy:%s:%s" % (c["policy"], c["fam"]))
    return d


WANTED = {b: ["fam:" + f for f in FAMS] + ["pt:" + k for k in pc.POINT_KINDS] for b in BLOCKS}
WANTED["value"] = WANTED["value"] + ["D:%d" % D for D in WIDTHS] + ["L:%d" % L for L in (1, 65) + BIG_L] + ["P:65"] + \
    ["obs:noise_floor", "obs:noise_dom"] + ["policy:%s:%s" % (p, f) for f in ("std", "ls_ard") for p in POLICIES]
WANTED["setup"] = WANTED["setup"] + ["L:1", "L:65", "P:65"]
WANTED["matrix"] = WANTED["matrix"] + ["L:1", "L:65", "P:65"]


def missing(cases):
    """The dimensions without a witness: every family and every kind of particle on each of the three blocks, every width,
    feature count, the second particle group, the observation noise and both controllers on the value block, and every
    ill-conditioned family at N = 65 on all three."""
    have = {b: set() for b in BLOCKS}
    for c in cases:
        for b in c["blocks"]:
            have[b] |= dims_of(c)
    out = ["%s on %s" % (t, b) for b in BLOCKS for t in WANTED[b] if t not in have[b]]
    for f in ILL:
        for b in BLOCKS:
            if not any(c["fam"] == f and c["N"] == 65 and b in c["blocks"] for c in cases):
                out.append("fam:%s at N:65 on %s" % (f, b))
    return out


# ------------------------------------------------------------------ the inputs of a case
def normals(E, D, L, P, N):
    """The draw set of a shape from the stream restatement: z (E, L, D) (omega = z / lengthscale), phase, w, xi."""
    return dict(z=rf.freq_normals(SEED, E, L, D)[0], phase=rf.phases(SEED, E, L), w=rf.weights(SEED, np.arange(P), E, L)[0],
                xi=rf.xis(SEED, np.arange(P), E, N)[0])


def table_model(c, base):
    """dict(X, Y, lengthscales, variance, noise) of a table case from its data set (dict with X, Y)."""
    d = pc.make_data(pc_case(c), base)
    if c["policy"]:
        return dict(X=d["X"], Y=d["Y"], lengthscales=d["ls"], variance=d["var"], noise=d["noise"]), d
    return dict(X=d["X"], Y=np.column_stack([d["Y"], d["Y"][:, 0] - d["Y"][:, 1]]), lengthscales=np.vstack([d["ls"], d["ls"][:1, ::-1]]),
                variance=np.append(d["var"], d["var"][0] * 3.0), noise=np.append(d["noise"], d["noise"][1] * 2.0)), d


def make_x0(c, d):
    """(generator only) the initial particles of a table case: the seven kinds of point, their first E coordinates."""
    xs = pc.make_points(pc_case(c), d)[:, :c["E"]]
    if c["P"] > len(xs):
        rs = np.random.RandomState(pc._seed("particles" + c["name"]))
        idx = np.arange(c["P"]) % len(xs)
        xs = xs[idx] + np.where(np.arange(c["P"])[:, None] < len(xs), 0.0, 0.05 * rs.randn(c["P"], c["E"]))
    return np.ascontiguousarray(xs)


def policy_of(c, setup=None):
    """The restatement's policy dict (helpers/particles_restatement.action) or None."""
    if c["policy"] in POLICIES:
        p = POLICIES[c["policy"]]
        return dict(kind="linear", W=np.array(p["W"]), b=np.array(p["b"]), max_action=p["max_action"])
    return setup["policy"] if c["policy"] == "w" else None


def _finish_draws(c, model, n):
    dr = dict(omega=n["z"] / np.asarray(model["lengthscales"], np.float64)[:, None, :], phase=n["phase"], w=np.array(n["w"]), xi=np.array(n["xi"]))
    if c["fam"] == "y0":            # output 0: y = 0, w = 0, xi = 0 -- V, f and row 0 of A - I are exactly zero
        dr["w"][:, 0, :] = 0.0
        dr["xi"][:, 0, :] = 0.0
    if c.get("zero_w0"):
        dr["w"][:, 0, :] = 0.0
    return dr


_FX = None
_CASE = {}


def fixture():
    global _FX
    if _FX is None:
        with np.load(PATH) as z:
            _FX = {k: z[k] for k in z.files}
    return _FX


def case(c, fx=None):
    """-> dict(model, policy, x0 (P, E), draws, eps (1, P, E) or None) of a case, from the fixture (fx: the generator's dict)."""
    if fx is None and c["name"] in _CASE:
        return _CASE[c["name"]]
    fx_ = fixture() if fx is None else fx
    eps = None
    if c["kind"] == "width":
        from helpers import particle_fn_grad_cases as gc
        s = gc.setup(c["data"])
        model = {k: np.asarray(s["model"][k], np.float64) for k in ("X", "Y", "lengthscales", "variance", "noise")}
        policy, x0 = policy_of(c, s), gc.x0_of(c["data"], c["P"], 5)
        dr = _finish_draws(c, model, normals(c["E"], c["D"], c["L"], c["P"], c["N"]))
    else:
        base = {k: fx_["_data/%s/%s" % (c["data"], k)] for k in ("X", "Y")}
        model, _ = table_model(c, base)
        policy = policy_of(c)
        if c["kind"] == "bigL":
            x0 = fx_["_bigL/x0"]
            n = normals(c["E"], c["D"], c["L"], c["P"], c["N"])
        else:
            x0 = fx_[c["name"] + "/x0"]
            n = {k: fx_["%s/%s" % (draw_key(c), k)] for k in ("z", "phase", "w", "xi")}
            if c["obs"]:
                eps = fx_[c["name"] + "/eps"]
        dr = _finish_draws(c, model, n)
    out = dict(model=model, policy=policy, x0=np.asarray(x0, np.float64), draws=dr, eps=eps)
    if fx is None:
        _CASE[c["name"]] = out
    return out


def declared(c):
    """The exact results a case declares: the index of the far particle (every kernel value is 0: x' - x is the feature half
    alone and the kernel half of A is exactly 0) or None, and whether output 0 is the zero output of the y0 family."""
    return (pc.POINT_KINDS.index("far40") if c["kind"] == "table" else None), c["fam"] == "y0"


def k_of(got, truth, unit):
    return pc.k_of(got, truth, unit)
