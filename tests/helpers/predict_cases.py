"""Edge hyper-parameters and test points of the GP posterior at deterministic inputs and of its input Jacobians
(csrc/predict.hip, csrc/predict_jac.hip, k_gram): one table for tests/test_predict_edges_cpu.py (coverage guard, K_ref, caps,
sensitivity), oracle/gen_golden_predict.py (the 40-digit truth with units in tests/golden/predict_edges.npz) and
tests/test_gpu_predict_edges.py (every route).  docs/predict_edges.md describes it.

Plain data.  A case names a data set (DATA: points, targets, inducing inputs; stored in the fixture), a hyper-parameter family
(`fam`) and the shape.  E = 2 unless the data set says otherwise, and the outputs always carry different lengthscales, signal
variances and noises.  A FITC case (M > 0) runs on the slot's shared inducing inputs Z_all[0] and with every output's own
Z_all[e]; the fixture holds a truth for each.  Every case has the same kinds of test points (POINT_KINDS)."""
from __future__ import annotations

import zlib

import numpy as np

TINY = 2.0 ** -1022
EPS = 2.0 ** -53
LOG_ZERO = 1075 * np.log(2.0)      # exp(-q) rounds to zero past q = 745.13
BLOCKS = ("mean", "var", "dmean", "dvar")
JITTER = 1e-6

# name: (N, M, D, E)
DATA = {
    "x24": (24, 0, 3, 2),       # one 64-row group
    "x65": (65, 0, 3, 2),       # two groups, the first trtri doubling level, kcend clipped
    "x200": (200, 0, 3, 1),     # G = 4: five work units over four waves; the Jacobian kernel's mean unit falls to wave 0
    "x24d1": (24, 0, 1, 2),
    "x24d9": (24, 0, 9, 2),     # the mean unit's four-dimension passes have a remainder
    "f10": (150, 10, 4, 2),
    "f65": (150, 65, 4, 2),
    "f130": (100, 130, 4, 2),   # 2 * 3 + 1 = 7 units, M > N
}

# family: what differs from "std" (lengthscales kind, variances, noises, data transform)
FAMILIES = {
    "std": {},
    "ls_short": dict(ls="short"), "ls_flat": dict(ls="flat"), "ls_ard": dict(ls="ard"), "ls_crossed": dict(ls="crossed"),
    "var_tiny": dict(var=(1e-8, 2e-8)), "var_huge": dict(var=(1e6, 2e6)), "var_mixed": dict(var=(1e-8, 1e6)),
    "noise_floor": dict(noise=(1e-6, 4e-6)), "noise_m10": dict(noise=(1e-10, 3e-10)),
    "noise_dom": dict(noise=(1e2, 2e2), var=(1e-4, 2e-4)),
    "flat_floor": dict(ls="flat", noise=(1e-6, 4e-6)),
    "big6": dict(data="big6"), "dup": dict(data="dup", noise=(1e-6, 1e-6)), "y1e6": dict(data="y1e6"), "y0": dict(data="y0"),
}
ILL = ("noise_floor", "noise_m10", "flat_floor", "dup")     # cond(K) >= 1e8: classes of their own, and they run at N = 65 and 200
POINT_KINDS = ("on", "beside", "centroid", "half", "three", "denorm", "far40")   # FITC adds "on_z"


def _c(name, data, fam):
    N, M, D, E = DATA[data]
    kind = "fitc" if M else "exact"
    cls = "%s_%s" % (kind, fam) + ("" if data in ("x24", "f10") else "_" + data)     # (the shapes and the larger ill-conditioned models apart)
    return dict(name=name, data=data, fam=fam, N=N, M=M, D=D, E=E, cls=cls)


CASES = ([_c("x24_" + f, "x24", f) for f in FAMILIES] + [_c("f10_" + f, "f10", f) for f in FAMILIES] +
         [_c("x65_" + f, "x65", f) for f in ILL] + [_c("x200_" + f, "x200", f) for f in ILL if f != "dup"] +
         [_c("x24d1_std", "x24d1", "std"), _c("x24d9_std", "x24d9", "std"), _c("f65_std", "f65", "std"), _c("f130_std", "f130", "std")])


def case_ids(cases=None):
    return [c["name"] for c in (CASES if cases is None else cases)]


def by_name(name):
    return next(c for c in CASES if c["name"] == name)


def truth_names(c):
    """The truths a case has in the fixture: "t" (exact GP), or "ts" (shared Z) and "to" (own Z)."""
    return ("ts", "to") if c["M"] else ("t",)


def point_kinds(c):
    return POINT_KINDS[:1] + (("on_z",) if c["M"] else ()) + POINT_KINDS[1:]


# ------------------------------------------------------------------ data
def _seed(s):
    return zlib.crc32(s.encode()) % (2 ** 31)


def make_base(name):
    """The data set's points, targets and inducing inputs (generator only: the tests read them from the fixture)."""
    N, M, D, E = DATA[name]
    rs = np.random.RandomState(_seed("predict" + name))
    X = rs.randn(N, D)
    Y = 0.3 * np.sin(X @ rs.randn(D, E) / np.sqrt(D)) + 1e-2 * rs.randn(N, E)
    out = dict(X=X, Y=Y)
    if M:
        P = X if M <= N // 2 else np.concatenate([X, rs.randn(2 * M, D)])
        out["Z"] = np.stack([P[e * M:(e + 1) * M] + 0.05 * rs.randn(M, D) for e in range(E)])
    return out


def hyper(c):
    """(ls (E, D), var (E), noise (E)) of a case."""
    E, D = c["E"], c["D"]
    f = FAMILIES[c["fam"]]
    rs = np.random.RandomState(_seed("hyp") + 31 * E + D)
    kind = f.get("ls", "std")
    if kind == "std":
        ls = (0.6 + 0.4 * rs.rand(E, D)) * np.sqrt(D)
    elif kind == "short":
        ls = 1e-2 * np.ones((E, D))
    elif kind == "flat":
        ls = 1e3 * np.ones((E, D))
    elif kind == "ard":        # 1e-2 .. 1e4 inside every output, in another order per output
        base = np.logspace(-2, 4, D)
        ls = np.stack([np.roll(base, a) for a in range(E)])
    elif kind == "crossed":    # output 0 short where output 1 is long
        base = np.logspace(-2, 2, D)
        ls = np.stack([base if a % 2 == 0 else base[::-1] for a in range(E)])
    var = np.array(f.get("var", (0.7, 1.3)))[:E]
    noise = np.array(f.get("noise", (1e-2, 3e-2)))[:E]
    return ls, var.astype(np.float64), noise.astype(np.float64)


def make_data(c, base):
    """X, Y, Z (E, M, D) or None, ls, var, noise of a case from its data set (base: dict with X, Y, Z)."""
    X, Y = np.array(base["X"], np.float64), np.array(base["Y"], np.float64)
    Z = np.array(base["Z"], np.float64) if c["M"] else None
    ls, var, noise = hyper(c)
    kind = FAMILIES[c["fam"]].get("data", "std")
    if kind == "big6":         # inputs near 1e6
        X = X + 1e6
        Z = None if Z is None else Z + 1e6
    elif kind == "dup":        # two training points 1e-7 apart
        X[1] = X[0] + 1e-7 / np.sqrt(c["D"])
    elif kind == "y1e6":
        Y = Y * 1e6
    elif kind == "y0":
        Y[:, 0] = 0.0
    return dict(X=X, Y=Y, Z=Z, ls=ls, var=var, noise=noise)


def se_ard(A, B, ls, var):
    d = (A[:, None, :] - B[None, :, :]) / np.asarray(ls, np.float64)
    return float(var) * np.exp(-0.5 * np.sum(d * d, axis=-1))


def make_points(c, d):
    """The test points of a case (generator only; the fixture stores them), in the order of point_kinds(c).  Lengths are output
    0's lengthscales; the points of the cross-covariance are the training inputs (FITC: output 0's inducing inputs)."""
    X, l0 = d["X"], d["ls"][0]
    P = d["Z"][0] if c["M"] else X
    D = c["D"]
    rs = np.random.RandomState(_seed("points" + c["name"]))
    u = rs.randn(D)
    u /= np.linalg.norm(u)
    pts = {"on": P[5].copy() if not c["M"] else X[5].copy(), "beside": P[7] + 1e-9 * l0 * u, "centroid": P.mean(0),
           "half": P[2] + 0.5 * l0 * u, "three": P[2] + 3.0 * l0.min() * u}
    if c["M"]:
        pts["on_z"] = P[3].copy()
    # some k_i denormal, others exactly zero: outwards from the extreme point in direction u.  Where the points' distances
    # spread enough, the nearest k is about 2^-1023 (a mistake with denormal operands is then as large as it can be); where they do
    # not (a flat kernel), the nearest k is just above the threshold of rounding to zero and the farthest below it.
    j = int(np.argmax((P / l0) @ u))
    lv = np.log(d["var"][0])
    # (k = fl(sf2 fl(exp(-q))): for sf2 >= 1/4 it is zero exactly when the exponential has rounded to zero)
    zero_at = LOG_ZERO + (lv if d["var"][0] < 0.25 else 0.0)

    def q(t):
        x = P[j] + t * l0 * u
        return np.sort(0.5 * np.sum(((P - x) / l0) ** 2, axis=1)), x

    def nearest_at(target):
        lo, hi = 0.0, 100.0
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            if q(mid)[0][0] < target:
                lo = mid
            else:
                hi = mid
        return q(lo)

    qs, x = nearest_at(lv + 1023 * np.log(2.0))
    if qs[-1] < zero_at + 0.05:
        delta = 0.5
        for _ in range(3):
            qs, x = nearest_at(zero_at - delta)
            delta = min(0.5, 0.5 * (qs[-1] - qs[0]))
    pts["denorm"] = x
    k = se_ard(P, x[None], l0, d["var"][0])[:, 0]
    assert np.any((k > 0) & (k < TINY)) and np.any(k == 0.0), (c["name"], "denormal point", np.sort(k)[[0, -1]])
    # 40 l_max beyond the data in every dimension: every k of every output is exactly zero
    allp = X if not c["M"] else np.concatenate([X] + list(d["Z"]))
    pts["far40"] = allp.max(0) + 40.0 * d["ls"].max()
    xs = np.stack([pts[k] for k in point_kinds(c)])
    for e in range(c["E"]):
        for Pe in ([X] if not c["M"] else [d["Z"][0], d["Z"][e]]):
            assert np.all(se_ard(Pe, xs[-1:], d["ls"][e], d["var"][e]) == 0.0), (c["name"], "far point")
    return xs


def declared_zeros(c):
    """(E, Nt, 4) bool: the entries (of every d for the Jacobians) that are exactly zero -- the variance: exactly sf2 -- by the
    case's construction: the far point, and output 0 of the y = 0 family (mean and dmean)."""
    kinds = point_kinds(c)
    z = np.zeros((c["E"], len(kinds), 4), bool)
    z[:, kinds.index("far40"), :] = True
    if c["fam"] == "y0":
        z[0, :, 0] = z[0, :, 2] = True
    return z


# ------------------------------------------------------------------ routes and the guard
ROUTES = ("values", "jac", "shared", "own", "single")


def routes(c):
    """exact: gp_predict_points, gp_predict_points_jac, and both with output = 1 (E = 1: output = 0) alone;
    FITC: both calls on the shared Z, with every output's own Z, and the single output on both."""
    return ("shared", "own", "single") if c["M"] else ("values", "jac", "single")


FAMILY_DIMS = ["fam:" + f for f in FAMILIES if f != "std"] + ["pt:" + k for k in POINT_KINDS]
SHAPE_DIMS = {"values": ("N:24", "N:65", "N:200", "E:1", "E:2", "D:1", "D:3", "D:9"), "jac": ("N:24", "N:65", "N:200", "D:1", "D:9", "E:1"),
              "shared": ("M:10", "M:65", "M:130", "pt:on_z"), "own": ("M:10", "M:65", "M:130", "pt:on_z"), "single": ("E:1", "E:2")}


def dims_of(c):
    fam = {"fam:" + c["fam"]} | {"pt:" + k for k in point_kinds(c)}
    shp = {"N:%d" % c["N"], "D:%d" % c["D"], "E:%d" % c["E"]} | ({"M:%d" % c["M"]} if c["M"] else set())
    return fam, shp


def missing(cases):
    """The dimensions without a witness: every family and every kind of test point on each of the five routes, every shape on
    the routes it exists for, every ill-conditioned family at N = 65 and (but the duplicate pair) at N = 200."""
    have = {r: set() for r in ROUTES}
    for c in cases:
        fam, shp = dims_of(c)
        rs = routes(c)
        if not rs:
            return ["%s has no route" % c["name"]]
        for r in rs:
            have[r] |= fam | shp
    out = ["%s on %s" % (t, r) for r in ROUTES for t in FAMILY_DIMS if t not in have[r]]
    out += ["%s on %s" % (t, r) for r in ROUTES for t in SHAPE_DIMS[r] if t not in have[r]]
    for f in ILL:
        for n in (65,) if f == "dup" else (65, 200):
            if not any(c["fam"] == f and c["N"] == n and not c["M"] for c in cases):
                out.append("fam:%s at N:%d" % (f, n))
    return out


# ------------------------------------------------------------------ K
def k_of(got, truth, unit):
    """max |got - truth| / unit; inf for a NaN or an infinity."""
    got, truth, unit = np.ravel(got), np.ravel(truth), np.ravel(unit)
    if not np.all(np.isfinite(got)):
        return float("inf")
    with np.errstate(over="ignore"):
        return float(np.max(np.abs(got - truth) / unit)) if got.size else 0.0


def ks(res, fx, outputs=None):
    """K per block of a result (mean, var (E', Nt), dmean, dvar (E', Nt, D); None: not computed) against a truth record fx."""
    sel = slice(None) if outputs is None else list(outputs)
    return {b: k_of(r, fx[b][sel], fx["u" + b][sel]) for b, r in zip(BLOCKS, res) if r is not None}


# ------------------------------------------------------------------ the fixture's records
TRUTH_KEYS = ("mean", "var", "dmean", "dvar", "umean", "uvar", "udmean", "udvar")


def truth_shapes(c):
    E, D, Nt = c["E"], c["D"], len(point_kinds(c))
    s = dict(mean=(E, Nt), var=(E, Nt), dmean=(E, Nt, D), dvar=(E, Nt, D))
    s.update({"u" + k: v for k, v in list(s.items())})
    return s


def pack_truth(t):
    return np.concatenate([np.asarray(t[k], np.float64).reshape(-1) for k in TRUTH_KEYS])


def unpack_truth(c, vec):
    out, o = {}, 0
    shapes = truth_shapes(c)
    for k in TRUTH_KEYS:
        n = int(np.prod(shapes[k]))
        out[k] = vec[o:o + n].reshape(shapes[k])
        o += n
    assert o == vec.size, c["name"]
    return out
