"""The case table of the full posterior covariance (pilco_gp_predict_points_cov; docs/predict_cov.md): the smallest shapes at
which k_predict_cov can go wrong -- the edges of its 64 x 64 tiles and 16-wide MFMA tiles on both axes (Nt) and of the walk over
the operator rows (N, or M for FITC with N = 2 M + 3) --, the data of a case, its test points, and the fixture's records
(tests/golden/predict_cov.npz, written by tools/gen_golden_predict_cov.py).

Test points of a case, in this order as far as Nt reaches (POINT_KINDS): a random point, the SAME point again (a duplicate: two
equal rows and columns), a training (FITC: inducing) point, a point 30 lengthscales out (cov ~ sf2 on the diagonal, ~ 0 off it), a
point 1e-7 from the training point, a second training point, then random points."""
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "predict_cov.npz")
JITTER = 1e-6          # Kuu + jitter I of the FITC factorisation (gpflow default_jitter)
EPS, TINY = 2.0 ** -53, 2.0 ** -1022
CAP_FACTOR, CAP_FLOOR = 8.0, 4.0
POINT_KINDS = ("random", "duplicate", "on", "far", "near", "on2")
NTS = (1, 2, 15, 16, 17, 63, 64, 65, 130)
NS = (5, 63, 64, 65, 130)


def _c(kind, n, Nt, D, E, noise, own=False):
    M = n if kind == "f" else 0
    N = 2 * n + 3 if kind == "f" else n
    name = "%s%d_t%d_d%d_e%d%s%s" % (kind, n, Nt, D, E, "_own" if own else "", "_lo" if noise < 1e-3 else "")
    return dict(name=name, kind=kind, N=N, M=M, n=n, Nt=Nt, D=D, E=E, noise=noise, own=own)


def _table(kind):
    own = kind == "f"
    return [
        _c(kind, 64, 1, 1, 1, 1e-2), _c(kind, 63, 2, 4, 1, 1e-2), _c(kind, 65, 15, 11, 3, 1e-2, own), _c(kind, 130, 16, 4, 1, 1e-6),
        _c(kind, 5, 17, 1, 1, 1e-2), _c(kind, 63, 17, 4, 1, 1e-2), _c(kind, 64, 17, 4, 1, 1e-2), _c(kind, 65, 17, 4, 3, 1e-6, own),
        _c(kind, 130, 17, 11, 1, 1e-2),
        _c(kind, 64, 63, 4, 1, 1e-2), _c(kind, 63, 64, 1, 1, 1e-2),
        _c(kind, 5, 65, 1, 1, 1e-2), _c(kind, 63, 65, 4, 1, 1e-2), _c(kind, 64, 65, 4, 1, 1e-2), _c(kind, 65, 65, 4, 1, 1e-6),
        _c(kind, 130, 65, 11, 1, 1e-6),
        _c(kind, 130, 130, 4, 1, 1e-2),
    ]


CASES = _table("x") + _table("f") + [_c("f", 64, 17, 4, 3, 1e-2, False)]   # (the last: three outputs on the SHARED Z)


def case_ids():
    return [c["name"] for c in CASES]


def by_name(name):
    return next(c for c in CASES if c["name"] == name)


def missing(cases=None):
    """The requirements of the table a list of cases leaves uncovered (empty: none)."""
    cases = CASES if cases is None else cases
    out = []
    for kind, label in (("x", "exact"), ("f", "FITC")):
        mine = [c for c in cases if c["kind"] == kind]
        out += ["%s: Nt = %d" % (label, nt) for nt in NTS if not any(c["Nt"] == nt for c in mine)]
        out += ["%s: n = %d at Nt = %d" % (label, n, nt) for nt in (17, 65) for n in NS if not any(c["Nt"] == nt and c["n"] == n for c in mine)]
        out += ["%s: noise 1e-6 at n = %d" % (label, n) for n in (65, 130) if not any(c["n"] == n and c["noise"] == 1e-6 for c in mine)]
        out += ["%s: E = %d" % (label, e) for e in (1, 3) if not any(c["E"] == e for c in mine)]
        out += ["%s: D = %d" % (label, d) for d in (1, 4, 11) if not any(c["D"] == d for c in mine)]
    f = [c for c in cases if c["kind"] == "f" and c["E"] > 1]
    if not any(c["own"] for c in f):
        out.append("FITC: every output's own Z")
    if not any(not c["own"] for c in f):
        out.append("FITC: several outputs on the shared Z")
    if not any(c["E"] > 1 for c in cases):
        out.append("one output alone (output = 1)")
    return out


def make_data(c):
    """The model of a case: X (N, D), Y (N, E), Z (E, M, D) or None (Z[0] is the shared set), ls (E, D), var, noise (E)."""
    import zlib
    rng = np.random.RandomState(zlib.crc32(c["name"].encode()) & 0x7FFFFFFF)
    N, M, D, E = c["N"], c["M"], c["D"], c["E"]
    X = rng.uniform(-1.0, 1.0, (N, D))
    ls = np.sqrt(D) * rng.uniform(0.6, 1.4, (E, D))
    var = rng.uniform(0.5, 2.0, E)
    Y = np.stack([np.sin(X @ rng.randn(D)) for _ in range(E)], axis=1) + 0.1 * rng.randn(N, E)
    Z = rng.uniform(-1.0, 1.0, (E, M, D)) if M else None
    return dict(X=X, Y=Y, Z=Z, ls=ls, var=var, noise=np.full(E, c["noise"]))


def points_of(c, d, e=0):
    """The points the cross-covariances are taken with: X, or the inducing inputs of output e (own) / the shared set."""
    return d["X"] if not c["M"] else d["Z"][e if c["own"] else 0]


def make_points(c, d):
    import zlib
    rng = np.random.RandomState(zlib.crc32((c["name"] + "/xs").encode()) & 0x7FFFFFFF)
    P, D = points_of(c, d), c["D"]
    xs = rng.uniform(-1.0, 1.0, (c["Nt"], D))
    special = {"duplicate": xs[0], "on": P[0], "far": P[0] + 30.0 * d["ls"].max(axis=0), "near": P[0] + 1e-7, "on2": P[len(P) // 2]}
    for i, kind in enumerate(POINT_KINDS):
        if i and i < c["Nt"]:
            xs[i] = special[kind]
    return xs


def tril_pack(A):
    """(E, Nt, Nt) symmetric -> (E, Nt (Nt + 1) / 2): the lower triangles, row by row."""
    i, j = np.tril_indices(A.shape[-1])
    return A[:, i, j]


def tril_unpack(v, Nt):
    i, j = np.tril_indices(Nt)
    A = np.zeros((v.shape[0], Nt, Nt), v.dtype)
    A[:, i, j] = v
    A[:, j, i] = v
    return A


_FX = None


def get(key):
    global _FX
    if _FX is None:
        _FX = dict(np.load(PATH))
    return _FX[key]


def load(c):
    """A case from the fixture: its data with `xs`, the truth `cov` (E, Nt, Nt), its `unit` and the cap of the device's K.
    The units are stored as float32 log2, rounded DOWN: a stored unit is the truth's unit or up to 2^-16 of it smaller."""
    d = {k: get(c["name"] + "/" + k) for k in ("X", "Y", "ls", "var", "noise", "xs")}
    d["Z"] = get(c["name"] + "/Z") if c["M"] else None
    d["cov"] = tril_unpack(get(c["name"] + "/cov"), c["Nt"])
    d["unit"] = np.maximum(np.exp2(tril_unpack(get(c["name"] + "/lunit"), c["Nt"]).astype(np.float64)), TINY)
    d["cap"] = float(get("_caps")[list(get("_caps_keys")).index(c["name"])])
    return d


def pack_unit(unit):
    """float64 units -> float32 log2, rounded down."""
    l = np.log2(unit)
    l32 = l.astype(np.float32)
    return np.where(l32.astype(np.float64) > l, np.nextafter(l32, np.float32(-np.inf)), l32).astype(np.float32)


def z_arg(c, d):
    """What the device calls take as Z_all: (E, M, D) for a case on every output's own Z, None otherwise."""
    return d["Z"] if c["own"] else None
