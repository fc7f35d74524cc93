"""Edge inputs of the step's serial link (controller, squash_sin, joint Gaussian, reward): one table for
tests/test_link_edges_cpu.py (coverage guard, predicate mirror, K_ref, sensitivity), oracle/gen_golden_link.py (the
50-digit truth in tests/golden/link_edges.npz) and tests/test_gpu_link_edges.py (stages, every route, gradients, lanes).

Plain data.  A case names a SHAPE (one small, well conditioned GP per shape: the GP is not under test) and what it feeds the
link: the initial state covariance `s0`, the controller `ctrl`, `maxact`, `squash`, the reward recipe `reward`, the horizon.
  grad    "mp": the fixture holds the 50-digit gradient; "ag": torch autograd is the yardstick; None: forward only
  exact0  blocks whose truth is exactly 0 or denormal: compared absolutely (|dev| <= 2^-1022 K)
  group   the class the K caps are taken over (tests/test_link_edges_cpu.py prints K_ref per class)
  stage   True: no GP, policy_action / reward_eval only (shapes beyond what a rollout takes)
docs/link_edges.md describes the dimensions and what was found.
"""
from __future__ import annotations

import numpy as np

TOL_FWD = 1e-9
TOL_GRAD = 1e-7
TOL_ROUTES = 1e-10
TINY = 2.0 ** -1022
EPS = 2.0 ** -53

# name: (N, E, U, policy, bf)
SHAPES = {
    "e6u4": (40, 6, 4, "linear", 0),      # lin_fused at its boundary: 5 (16 + 4) = 100 = D^2
    "e5u4": (40, 5, 4, "linear", 0),      # one short of it: 100 > 81
    "e1u8": (30, 1, 8, "linear", 0),      # two rounds
    "e2u16": (24, 2, 16, "linear", 0),    # two rounds, three-kernel step (D = 18)
    "e1u31": (24, 1, 31, "linear", 0),    # two rounds, D = 32
    "e3u16": (24, 3, 16, "linear", 0),    # one short of two rounds
    "e1u1": (20, 1, 1, "linear", 0),      # E = 1 and U = 1
    "e3u1": (16, 3, 1, "linear", 0),      # U = 1; tiny: 50-digit gradients
    "e2u1": (16, 2, 1, "linear", 0),      # E = 2: the zero-pivot pair; tiny
    "e2u2": (16, 2, 2, "linear", 0),      # tiny, two controls
    "e16u2": (20, 16, 2, "linear", 0),    # three-kernel step with many states
    "e3u0": (30, 3, 0, "none", 0),        # no controller
    "e3u1r": (16, 3, 1, "rbf", 6),        # RbfController evaluated inline
    "e6u2r": (24, 6, 2, "rbf", 80),       # RbfController with its own launches (3 * 80^2 > 16384)
    "e32": (0, 32, 0, "none", 0),         # stage only: reward staging at E = 32
    "e20u20": (0, 20, 20, "linear", 0),   # stage only: policy_action with 32 < D <= 64
    "e32u8": (0, 32, 8, "linear", 0),
    "e8u32": (0, 8, 32, "linear", 0),     # stage only: U = 32, squash_inplace's four registers per thread exactly full
}


def _c(name, shape, s0="std", ctrl="std", maxact="std", squash=True, reward="std", H=2, grad=None, exact0=(), group=None, bf=None,
       lanes=False):
    N, E, U, policy, sbf = SHAPES[shape]
    big = s0 in ("x30", "x400", "x1500")
    if group is None:
        # (an RbfController's K_ref is that of its own Gram matrix: 6 centres evaluated inline and 80 with launches of their own
        # are classes apart)
        group = ("rbf_own" if shape == "e6u2r" else "rbf" if policy == "rbf" else "lin") + ("/large" if big else "/bigmean" if ctrl in ("big2", "big6") else "/small")
    return dict(name=name, shape=shape, N=N, E=E, U=U, D=E + U, M=0, policy=policy, bf=sbf if bf is None else bf, s0=s0, ctrl=ctrl,
                maxact=maxact, squash=squash, reward=reward, H=H, grad=grad, exact0=tuple(exact0), group=group, stage=N == 0, lanes=lanes)


S0_ALL = ("zero", "t16", "t12", "t8", "rank1", "std", "x30", "x400", "x1500", "corr")
CASES = []
for _sh in ("e6u4", "e1u8"):
    for _s in S0_ALL:
        if _sh == "e1u8" and _s in ("rank1", "corr", "t12", "x30"):
            continue   # (E = 1: no off-diagonal; the middle of each magnitude ladder is e6u4's)
        CASES.append(_c("%s_%s" % (_sh, _s), _sh, s0=_s, exact0=("S", "C") if _s == "zero" else (), H=3 if _s in ("zero", "x400") else 2,
                        grad="ag" if _s in ("std", "t8", "corr") else None, lanes=_s == "std"))
CASES += [
    _c("e5u4_zero", "e5u4", s0="zero", exact0=("S", "C")), _c("e5u4_std", "e5u4", grad="ag", lanes=True),
    _c("e2u16_std", "e2u16", grad="ag", lanes=True), _c("e2u16_x400", "e2u16", s0="x400"),
    _c("e1u31_std", "e1u31", grad="ag"), _c("e1u31_zero", "e1u31", s0="zero", exact0=("S", "C")),
    _c("e3u16_std", "e3u16", grad="ag"), _c("e3u16_x1500", "e3u16", s0="x1500"),
    _c("e1u1_std", "e1u1", grad="ag"), _c("e1u1_zero", "e1u1", s0="zero", exact0=("S", "C")), _c("e1u1_t16", "e1u1", s0="t16"),
    _c("e16u2_std", "e16u2", grad="ag"),
    _c("e3u0_std", "e3u0"), _c("e3u0_zero", "e3u0", s0="zero", H=3, lanes=True),
    # controller
    _c("e6u4_W0", "e6u4", ctrl="W0", exact0=("S", "C")), _c("e6u4_zeroact", "e6u4", ctrl="zero", exact0=("M",)),
    _c("e6u4_big2", "e6u4", ctrl="big2"), _c("e6u4_big6", "e6u4", ctrl="big6"),
    _c("e6u4_meq", "e6u4", ctrl="meq", grad="ag"), _c("e6u4_mopp", "e6u4", ctrl="mopp", grad="ag"),
    _c("e6u4_ma_none", "e6u4", maxact=None, grad="ag"), _c("e6u4_ma_m3", "e6u4", maxact="1e-3"), _c("e6u4_ma_p3", "e6u4", maxact="1e3"),
    _c("e6u4_ma_mixed", "e6u4", maxact="mixed", grad="ag"), _c("e6u4_nosquash", "e6u4", squash=False),
    _c("e1u8_W0", "e1u8", ctrl="W0", exact0=("S", "C")), _c("e1u8_big6", "e1u8", ctrl="big6"), _c("e1u8_meq", "e1u8", ctrl="meq", grad="ag"),
    _c("e1u8_ma_mixed", "e1u8", maxact="mixed", grad="ag"), _c("e1u8_nosquash", "e1u8", squash=False),
    # (adjoints by value at the magnitudes of the forward ladder; H = 3: the second policy application sees a produced state)
    _c("e3u1_zero_g", "e3u1", s0="zero", H=3, grad="mp", exact0=("S", "C")), _c("e3u1_x400_g", "e3u1", s0="x400", H=3, grad="mp"),
    _c("e3u1_big6_g", "e3u1", ctrl="big6", H=3, grad="mp"),
    _c("e3u1_std", "e3u1", grad="mp", lanes=True), _c("e3u1_t8", "e3u1", s0="t8", grad="mp"), _c("e2u2_mopp", "e2u2", ctrl="mopp", grad="mp"),
    # RbfController
    _c("rbf_std", "e3u1r", grad="mp"), _c("rbf_bf1", "e3u1r", bf=1, grad="ag"), _c("rbf_far", "e3u1r", ctrl="far", exact0=("M",)),
    _c("rbf_on", "e3u1r", ctrl="on", grad="ag"), _c("rbf_ls_m2", "e3u1r", ctrl="ls-2", group="rbf/narrow"),
    _c("rbf_ls_p2", "e3u1r", ctrl="ls2", group="rbf/flat"), _c("rbf_zero_s", "e3u1r", s0="zero"),
    _c("rbf_own_std", "e6u2r", grad="ag"), _c("rbf_own_x30", "e6u2r", s0="x30"), _c("rbf_own_nosquash", "e6u2r", squash=False),
    # reward
    _c("rw_none", "e3u1", reward="none", grad="mp"), _c("rw_four", "e3u1", reward="four", grad="mp"),
    _c("rw_W0", "e3u1", reward="W0", grad="ag"), _c("rw_rank1", "e3u1", reward="rank1", grad="mp"),
    _c("rw_rankEm1", "e6u4", reward="rankEm1", grad="ag"), _c("rw_rank2of3", "e3u1", reward="rankEm1", grad="mp"),
    _c("rw_diag0", "e3u1", reward="diag0", grad="ag"), _c("rw_cond12", "e6u4", reward="cond12", grad="ag"),
    _c("rw_asym", "e3u1", reward="asym", grad="mp"), _c("rw_asym14", "e3u1", reward="asym14"), _c("rw_asym12", "e3u1", reward="asym12"),
    _c("rw_neg13", "e3u1", reward="neg13"), _c("rw_neg3", "e3u1", reward="neg3", grad="ag"),
    _c("rw_zp", "e2u1", s0="zp", reward="zp", grad="mp"), _c("rw_zp_asym", "e2u1", s0="zp", reward="zp_asym", grad="mp"),
    _c("rw_t0", "e3u1", reward="t0", H=1), _c("rw_t8", "e3u1", reward="t8", grad="ag"),
    _c("rw_t40", "e3u1", reward="t40", exact0=("rmu", "rvar", "rew")), _c("rw_tnone", "e3u1", reward="tnone"),
    _c("rw_x1500", "e3u1", s0="x1500", reward="std"), _c("rw_e1u8_rank0", "e1u8", reward="W0", grad="ag"),
    _c("rw_e1u8_four", "e1u8", reward="four", grad="ag"),
    # stage only
    _c("st_e32_four", "e32", reward="four"), _c("st_e32_asym", "e32", reward="asym"), _c("st_e32_rankEm1", "e32", reward="rankEm1"),
    _c("st_e20u20", "e20u20"), _c("st_e32u8", "e32u8"), _c("st_e8u32", "e8u32"),
]


def case_ids(cases=None):
    return [c["name"] for c in (CASES if cases is None else cases)]


def by_name(name):
    return next(c for c in CASES if c["name"] == name)


# ------------------------------------------------------------------ mirrors of the link's branch predicates (csrc/link_predicates.h)
def squash_round_cap(nm):
    """Slots of one round of squash_inplace's evaluations in the link's own scratch (t1 .. js)."""
    return (4 * nm * nm + nm) // 5 * 5


def squash_rounds(U, nm):
    need, cap = 5 * (U * U + U), squash_round_cap(nm)
    return (need + cap - 1) // cap


def lin_fused_fits(U, nm):
    return 5 * (U * U + U) <= nm * nm


def rbf_inline_layout_total(E, U, bf):
    P = U * (U + 1) // 2
    nmat = U + P
    o = bf * E + U * bf + U * E + U + U + 2 * nmat * E * 2 * E + nmat * E + U * E * E + P * E * E + nmat + bf * (2 * E + 2) + bf * 16 \
        + 4 * (E + 2) + 4
    return (o + 1) & ~1


def rbf_inline_lds_doubles(E, U, bf):
    if E < 1 or E > 16 or U < 1 or U > 4 or bf < 1 or bf > 256:
        return 0
    if U * (U + 1) // 2 * bf * bf > 16384:
        return 0
    t = rbf_inline_layout_total(E, U, bf)
    return t if t <= 8192 else 0


def squash_class(E, U, kind, standalone=False, bf=0):
    """Which squash code a (state, control, policy) shape runs: 'none' (no controller), 'lin_fused' (evaluations +
    write_joint_lin_squash: a LinearController inside a rollout whose 5 (U^2 + U) slots fit one D x D buffer),
    'combine' / 'combine_rounds(n)' (squash_inplace's combining phase, in n rounds), 'rbf_inline' / 'rbf_own' (the same
    combining code behind an RbfController evaluated in the link / by its own launches)."""
    if kind == "none" or U == 0:
        return "none"
    nm = E + U
    n = squash_rounds(U, nm)
    if kind == "rbf":
        own = standalone or E + U > 16 or rbf_inline_lds_doubles(E, U, bf) == 0
        return ("rbf_own" if own else "rbf_inline") + ("" if n == 1 else "_rounds(%d)" % n)
    if not standalone and lin_fused_fits(U, nm):
        return "lin_fused"
    return "combine" if n == 1 else "combine_rounds(%d)" % n


def glue_lds_doubles(E, D):
    nm = max(E, D)
    return 3 * nm + 7 * nm * nm + 256 + (E + 4 * E * E + E * (E + 1) + E + 16)


LDS_LIMIT = 160 * 1024   # bytes of LDS a workgroup can have on gfx950


def policy_action_fits(E, U):
    return 8 * glue_lds_doubles(E, E + U) <= LDS_LIMIT


# ------------------------------------------------------------------ reward paths (mirror of psd_factor's switches)
_PSD = {}


def psd_factor(W):
    """csrc/reward_factor.h psd_factor, operation for operation: (rank, F (E, rank)); rank -1: not symmetric PSD (general path)."""
    W = np.ascontiguousarray(W, dtype=np.float64)
    key = W.tobytes()
    if key not in _PSD:
        _PSD[key] = _psd_factor(W)
    return _PSD[key]


def _psd_factor(W):
    E = W.shape[0]
    scale = np.abs(W).max()
    if scale == 0.0:
        return 0, np.zeros((E, 0))
    for i in range(E):
        for j in range(i):
            if abs(W[i, j] - W[j, i]) > 1e-13 * scale:
                return -1, None
    A, V = W.copy(), np.eye(E)
    old = np.seterr(over="ignore")   # (theta overflows for a tiny a_pq, as it does in the C routine: t becomes 0)
    for _ in range(60):
        off = 0.0
        for i in range(E):
            for j in range(i):
                off += A[i, j] * A[i, j]
        if off <= 1e-32 * scale * scale:
            break
        for p in range(E):
            for q in range(p + 1, E):
                apq = A[p, q]
                if apq == 0.0:
                    continue
                theta = (A[q, q] - A[p, p]) / (2.0 * apq)
                t = (1.0 if theta >= 0 else -1.0) / (abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                sn = t * c
                for M, cols in ((A, True), (A, False), (V, True)):
                    x, y = (M[:, p].copy(), M[:, q].copy()) if cols else (M[p, :].copy(), M[q, :].copy())
                    if cols:
                        M[:, p], M[:, q] = c * x - sn * y, sn * x + c * y
                    else:
                        M[p, :], M[q, :] = c * x - sn * y, sn * x + c * y
    np.seterr(**old)
    lam = np.diag(A)
    lmax = max(lam.max(), 0.0)
    if lam.min() < -1e-12 * max(lmax, scale):
        return -1, None
    keep = [i for i in range(E) if lam[i] > 1e-15 * lmax]
    return len(keep), V[:, keep] * np.sqrt(lam[keep])[None, :]


def reward_path(W):
    """'rank0', 'factored(r)' or 'general' as psd_factor decides."""
    r = psd_factor(W)[0]
    return "rank0" if r == 0 else "general" if r < 0 else "factored(%d)" % r


def path_class(W):
    p, E = reward_path(W), np.shape(W)[0]
    if p.startswith("factored"):
        r = int(p[9:-1])
        return "rank=E" if r == E else "0<rank<E"
    return p


# ------------------------------------------------------------------ data
def _seed(s):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(s)) * 7919 % (2 ** 31)


def _spd(rs, E):
    A = rs.randn(E, E)
    return np.eye(E) + A @ A.T / E


def _orth(rs, E):
    return np.linalg.qr(rs.randn(E, E))[0]


def rewards_of(c, rs, m0):
    """The reward recipe of a case: list of dict(kind 'exp' | 'lin', coef, W, t)."""
    E, r = c["E"], c["reward"]
    B = rs.randn(E, E)
    Wstd = 0.3 * np.eye(E) + 0.1 * B @ B.T / E
    dirn = rs.randn(E)
    dirn /= np.linalg.norm(dirn)
    t03 = m0.ravel() + 0.3 * dirn
    ex = lambda W, t=t03, coef=1.0: dict(kind="exp", coef=coef, W=np.ascontiguousarray(W, dtype=np.float64), t=None if t is None else np.asarray(t, np.float64))
    v = rs.randn(E, 1)
    Q = _orth(rs, E)
    A = rs.randn(E, E)
    if r == "none":
        return []
    if r == "std":
        return [ex(Wstd)]
    if r == "four":
        return [ex(Wstd, coef=0.7), dict(kind="lin", coef=-0.4, W=0.3 * rs.randn(E)), ex(v @ v.T, coef=0.0), dict(kind="lin", coef=1.3, W=np.zeros(E))]
    if r == "W0":
        return [ex(np.zeros((E, E)))]
    if r == "rank1":
        return [ex(v @ v.T)]
    if r == "rankEm1":
        Bm = rs.randn(E, E - 1)
        return [ex(Bm @ Bm.T / E)]
    if r == "diag0":
        return [ex(np.diag([1.0, 0.0, 2.0][:E] + [0.0] * max(E - 3, 0)))]
    if r == "cond12":
        W = (Q * np.logspace(0, -12, E)) @ Q.T
        return [ex(0.5 * (W + W.T))]
    if r == "asym":
        return [ex(Wstd + 0.1 * (A - A.T) / E)]
    if r in ("asym14", "asym12"):
        W = Wstd.copy()
        W[0, 1] += (1e-14 if r == "asym14" else 1e-12) * np.abs(W).max()
        return [ex(W)]
    if r in ("neg13", "neg3"):
        lam = np.linspace(1.0, 0.4, E)
        lam[-1] = -1e-13 if r == "neg13" else -1e-3
        W = (Q * lam) @ Q.T
        return [ex(0.5 * (W + W.T))]
    if r == "zp":
        return [ex(np.array([[1.0, -1.0], [-1.0, 2.0]]))]
    if r == "zp_asym":
        return [ex(np.array([[1.0, -1.0 + 1e-9], [-1.0 - 1e-9, 2.0]]))]
    if r == "t0":
        return [ex(Wstd, t=m0.ravel().copy())]
    if r == "t8":
        return [ex(np.eye(E), t=m0.ravel() + 8.0 * dirn)]
    if r == "t40":
        return [ex(np.eye(E), t=m0.ravel() + 40.0 * dirn)]
    if r == "tnone":
        return [ex(Wstd, t=None)]
    raise KeyError(r)


def make_data(c):
    """Deterministic GP (by shape), policy, reward and initial state (by case) of a case: plain NumPy."""
    N, E, U, D = c["N"], c["E"], c["U"], c["D"]
    d = {}
    if N:
        rs = np.random.RandomState(_seed(c["shape"]))
        X = rs.randn(N, D)
        d.update(X=X, Y=0.3 * np.sin(X @ rs.randn(D, E) / np.sqrt(D)) + 1e-2 * rs.randn(N, E), ls=(0.6 + 0.4 * rs.rand(E, D)) * np.sqrt(D),
                 var=0.3 + 0.7 * rs.rand(E), noise=1e-2 * np.ones(E))
    rs = np.random.RandomState(_seed(c["name"]))
    m0 = 0.2 * rs.randn(1, E)
    spd = _spd(rs, E)
    s0 = c["s0"]
    if s0 == "zero":
        S0 = np.zeros((E, E))
    elif s0 in ("t16", "t12", "t8"):
        S0 = {"t16": 1e-16, "t12": 1e-12, "t8": 1e-8}[s0] * spd
    elif s0 == "rank1":
        v = rs.randn(E, 1)
        S0 = 0.04 * v @ v.T
    elif s0 == "std":
        S0 = 0.04 * np.eye(E) + 0.01 * (spd - np.eye(E))
    elif s0 in ("x30", "x400", "x1500"):
        S0 = float(s0[1:]) * spd
    elif s0 == "corr":
        sd = 0.1 + 0.2 * rs.rand(E)
        S0 = np.outer(sd, sd) * (0.001 * np.eye(E) + 0.999)
    elif s0 == "zp":
        S0 = np.array([[1.0, 2.0], [2.0, 5.0]])
    else:
        raise KeyError(s0)
    S0 = 0.5 * (S0 + S0.T)
    ctrl = c["ctrl"]
    if c["policy"] == "linear":
        W = 0.6 * rs.randn(U, E) / np.sqrt(E)
        b = 0.3 * rs.randn(U)
        if ctrl == "W0":
            W = np.zeros((U, E))
        elif ctrl == "zero":
            b = np.zeros(U)
            m0 = np.zeros((1, E))
        elif ctrl == "big2":
            b = b + 1e2 * (1.0 + 0.3 * rs.rand(U))
        elif ctrl == "big6":
            b = b + 1e6 * (1.0 + 0.3 * rs.rand(U))
        elif ctrl == "meq":
            W = np.tile(W[:1], (U, 1))
            b = np.full(U, b[0])
        elif ctrl == "mopp":
            W[1], b[1] = -W[0], -b[0]
        if s0 in ("x30", "x400", "x1500"):
            # rows scaled so that the action variances w S0 w^T span 0.85 .. 1.07 of the factor: at 1500, exp(-s/2) runs from a
            # small normal number through the denormals to an exact 0
            k = float(s0[1:])
            tgt = k * (np.linspace(0.85, 1.07, U) if U > 1 else np.array([0.97]))
            W = W * np.sqrt(tgt / np.einsum("ue,ef,uf->u", W, S0, W))[:, None]
        d.update(W=W, b=b)
    elif c["policy"] == "rbf":
        bf = c["bf"]
        cX = rs.randn(bf, E)
        cl = (0.7 + 0.4 * rs.rand(U, E)) * np.sqrt(E)
        if ctrl == "far":
            cX = cX + 60.0
        if ctrl in ("on", "ls-2"):
            cX[0] = m0.ravel()
        if ctrl == "ls-2":
            cl = 1e-2 * cl
        if ctrl == "ls2":
            cl = 1e2 * cl
        d.update(cX=cX, cY=0.4 * rs.randn(bf, U), cl=cl)
    ma = c["maxact"]
    if U == 0 or ma is None:
        d["maxact"] = None
    elif ma == "std":
        d["maxact"] = 0.8 + rs.rand(U)
    elif ma == "mixed":
        d["maxact"] = np.array(([1e-3, 1e3, 1.0, 0.5] * U)[:U])
    else:
        d["maxact"] = np.full(U, float(ma))
    d.update(m0=m0, S0=S0)
    d["rewards"] = rewards_of(c, rs, m0)
    return d


def forward_routes(c):
    """Names of everything a case runs on: the two stages and the rollout routes of test_gpu_rollout_widths._forward_routes."""
    out = []
    if c["U"] > 0:
        out.append("stage_policy")
    if c["reward"] != "none":
        out.append("stage_reward")
    if not c["stage"]:
        out += ["default", "no_small", "three", "tiled"]
        if c["policy"] == "rbf":
            out += ["inline_off", "inline_off_three"]
    return out


def declared_routes(c):
    """What test_gpu_rollout_widths._expected_forward wants a case to declare (from the planner's Python mirror)."""
    from helpers import npoints_cases as nc
    fwd = nc.geometry(dict(c, factors="device"))["fwd"]
    out = dict(fwd=fwd)
    if c["policy"] == "rbf":
        own = c["D"] > 16 or rbf_inline_lds_doubles(c["E"], c["U"], c["bf"]) == 0
        out["policy_route"] = "own" if own else "inline"
        if own and fwd != "three":
            out["fwd"] = "fused_rbf"
    return out


# ------------------------------------------------------------------ units: |dev - truth| <= K * unit
def unit_squash_mean(e, m_pre):
    """e_u exp(-s/2) sin(m_u): exp <= 1, and sin moves by the rounding of its argument, 2^-53 |m_u|."""
    return EPS * np.abs(e) * (1.0 + np.abs(m_pre))


def unit_squash_cov(e, m_pre):
    """e_u e_v (...) / 2: differences of exponentials <= 1 times cos(m_u -+ m_v), whose arguments round by 2^-53 (|m_u| + |m_v|)."""
    a = np.abs(m_pre)
    return EPS * np.abs(np.outer(e, e)) * (1.0 + a[:, None] + a[None, :])


def unit_cross(V_truth, m_pre):
    """V C (and s V C): per control, normwise in its column, times the rounding of cos's argument."""
    V_truth = np.asarray(V_truth)
    return EPS * (1.0 + np.abs(m_pre))[None, :] * np.abs(V_truth).max(axis=0, keepdims=True) * np.ones_like(V_truth)


def unit_reward_mean(mu, q):
    """exp(-q / 2) / sqrt(det): the exponent's rounding 2^-53 q moves the value by mu q."""
    return EPS * abs(mu) * (1.0 + abs(q))


def unit_reward_var(mu, r2, q):
    """r2 - mu^2: both terms round on their own, r2 with an exponent of about 2 q."""
    return EPS * max(abs(r2), mu * mu) * (1.0 + 2.0 * abs(q))


# ------------------------------------------------------------------ gradient routes (mirror of csrc/rev.hip rev_chain_supported)
def rev_chain_supported(E, U):
    D, P = E + U, E * (E + 1) // 2
    NX, NT2 = E + P, D * (D + 1) // 2
    NR, NOUT = NX + U * E + U, D + NT2
    loc = E + E * E + 2 * U * E + 2 * U + 9 * U * U
    lds = NX * NOUT + 2 * E * D + E + E + E * E + loc + U * E + NX * (U + U * U) + (P + 1) // 2 + 2
    return 0 < U <= 4 and D <= 14 and NR <= 512 and 8 * lds <= 160 * 1024


def declared_grad(c):
    """chain (1 device, 2 host) and tape (2 Jacobian, 1 plain) of the DEFAULT value-and-gradient rollout of a case."""
    dev = c["policy"] == "linear" and rev_chain_supported(c["E"], c["U"])
    return dict(chain=1 if dev else 2, tape=2 if c["D"] <= 14 else 1)
