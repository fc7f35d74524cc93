"""Rollout cases over the point counts (N for the exact GP, M for FITC): one table for tests/test_npoints_cpu.py (mirror of
the host geometry, stream-K partition invariants, coverage guard, sensitivity of the tolerances) and tests/test_gpu_npoints.py
(every route against the oracle and against each other, gradients, lanes, a context reused across shapes).

After padding to npad = round_up(n, 64) the launch geometry of a step follows from npad and the output count.  The functions
below restate the host functions that choose it (csrc/prep.hip mm_prep_chunks, csrc/pair.hip pair_njb / mm_pair_nt /
mm_pair_sk_steps, the stream-K cut of csrc/api.hip build_work, csrc/rollout.hip small_col_splits / plan_route,
csrc/bwd.hip mm_bwd_geometry); test_npoints_cpu.py compiles the real ones and compares.  `cus` is the CU count (256 on MI355X),
`cap` the stream-K capacity of the pair kernel's instantiation (resident waves: occupancy x CUs x 4).

A case names its shape and data like helpers/dims_cases.py (make_data is reused) and declares what the planner must choose:
  fwd     default forward step: "small" (one launch per step), "fused" (fused head + pair launch), "three" (three-kernel step)
  jsmall  the value-and-gradient rollout runs its steps as the one-launch small step (U > 0 only)
  npad, NCH, NCHM, NCS   padded points, operand / mean row chunks, column splits of the one-launch small step (with a reward)
  bound   "T": the stream-K wave count is the step count T rounded up to 4; "cap": it is the capacity
  half    npad % 128 == 64: the last 128-row block of the reverse sweep has an empty 64-row half
  grad    False: forward only (torch autograd through the oracle at that size is too slow on a CPU)
  factors "user": gp_set_factors(iK=None, beta) in place of the device factorisation (no diagonal pair streams iK: nd = 0)
"""
from __future__ import annotations

from helpers.dims_cases import TOL_FWD, TOL_GRAD, TOL_ROUTES, make_data  # noqa: F401  (the same tolerances and data)

CUS = 256            # MI355X
CAP_RANGE = (2048, 6144)   # stream-K capacities a declared bound must hold for (the GPU test reads the real one)
PAIR_RT = 2          # csrc/pair_device.h
BWD_RT = 2           # csrc/bwd.hip


def round_up(n, b=64):
    return (n + b - 1) // b * b


def mm_vsep(D):
    return (D + 2) % 4 == 1


def mm_kp(D):
    return D + 1 if mm_vsep(D) else (D + 2 + 3) // 4 * 4


def prep_dt(D):
    for lim, dt in ((4, 4), (6, 6), (8, 8), (10, 10), (11, 11), (12, 12), (14, 14), (16, 16)):
        if D <= lim:
            return dt
    return 32


def prep_chunks(npad, PL, EL, cus=CUS):
    """csrc/prep.hip mm_prep_chunks -> (NCH, NCHM)."""
    nb = npad // 64
    nch = 1
    while nch * 2 <= nb and nb % (nch * 2) == 0 and PL * nch * 2 + EL + 1 <= cus:
        nch *= 2
    nchm = 1
    while nchm * 2 <= nb and nb % (nchm * 2) == 0 and nchm * 2 <= nch and PL * nch + EL * nchm * 2 + 1 <= cus:
        nchm *= 2
    return nch, nchm


def pair_njb(npad, PL):
    nb = npad // 64
    njb = 1
    while njb * 2 <= nb and nb % (njb * 2) == 0 and PL * (npad // (16 * PAIR_RT)) * njb < 1536:
        njb *= 2
    return njb


def pair_nt(npad, variant, PL):
    """csrc/pair.hip mm_pair_nt (variants 0 and 2)."""
    if variant == 2:
        nb, njb = npad // 64, 1
        while njb * 2 <= nb and nb % (njb * 2) == 0 and njb < 4:
            njb *= 2
        return (npad // (16 * PAIR_RT)) * njb
    return (npad // (16 * PAIR_RT)) * pair_njb(npad, PL)


def sk_steps(npad):
    """csrc/pair.hip mm_pair_sk_steps -> (tdiag, toff)."""
    NS, NTI = npad // 16, npad // (16 * PAIR_RT)
    return NTI * NS - PAIR_RT * NTI * (NTI - 1) // 2, NTI * NS


def sk_cut(npad, P, nd, cap):
    """The stream-K cut of csrc/api.hip build_work for one rank: (waves, T, tdiag, toff); nd diagonal pairs stream iK."""
    tdiag, toff = sk_steps(npad)
    if nd == 0:
        tdiag = toff
    T = nd * tdiag + (P - nd) * toff
    waves = max(4, (T + 3) // 4 * 4) if cap > T else cap
    return waves, T, tdiag, toff


def small_col_splits(npad, NCH, NCHM, KP, PL, EL, rew=True, cus=CUS):
    """csrc/rollout.hip small_col_splits."""
    if npad // NCH != 64 or KP > 16:
        return 1
    spare = EL * NCHM + (1 if rew else 0)
    ncs = 1
    while ncs * 2 <= NCH and ncs * 2 <= 4 and PL * NCH * ncs * 2 + spare <= cus:
        ncs *= 2
    return ncs


def bwd_geometry(npad, Pg):
    """csrc/bwd.hip mm_bwd_geometry -> (njs, nrb); mm_jac_nt = njs * nrb."""
    nrb = (npad + 64 * BWD_RT - 1) // (64 * BWD_RT)
    q = 1
    while q < 4 and (npad // 16) % (2 * q) == 0 and nrb * Pg * q < 1536:
        q *= 2
    return q, nrb


def geometry(c, cus=CUS, cap=3072):
    """What the planner chooses for case c (one rank, default settings)."""
    E, D = c["E"], c["D"]
    n = c["M"] or c["N"]
    npad = round_up(n)
    P = E * (E + 1) // 2
    KP, vsep = mm_kp(D), mm_vsep(D)
    NCH, NCHM = prep_chunks(npad, P, E, cus)
    dt = prep_dt(D)
    same_kc = KP == mm_kp(dt) and vsep == mm_vsep(dt)
    if D > 16:
        fwd = "three"   # (the fused heads do not fit the LDS: helpers/dims_cases.py)
    elif npad <= 256 and same_kc:
        fwd = "small"
    else:
        fwd = "fused"
    jsmall = c["U"] > 0 and D <= 14 and npad <= 256 and npad // NCH == 64 and same_kc and KP <= 16
    nd = 0 if c.get("factors") == "user" else E
    waves, T, _, _ = sk_cut(npad, P, nd, cap)
    return dict(npad=npad, NCH=NCH, NCHM=NCHM, NCS=small_col_splits(npad, NCH, NCHM, KP, P, E, True, cus),
                NT=pair_nt(npad, 0, P), sk_waves=waves, sk_total=T, sk_nd=nd, bound="T" if cap > T else "cap",
                fwd=fwd, jsmall=bool(jsmall), half=npad % 128 == 64, KP=KP, vsep=vsep)


DECLARED = ("fwd", "jsmall", "npad", "NCH", "NCHM", "NCS", "bound", "half")


def _c(name, N, E, U, policy="linear", bf=0, reward="exp", M=0, H=3, grad=True, factors="device", lanes=False, **decl):
    c = dict(name=name, N=N, E=E, U=U, D=E + U, policy=policy, bf=bf, reward=reward, M=M, H=H, grad=grad and U > 0,
             factors=factors, lanes=lanes)
    c.update(decl)
    return c


F, S, T3 = "fused", "small", "three"
CASES = [
    # exact GP: every 64-row edge up to two 128-row blocks
    _c("n0001", 1, 1, 1, H=3, fwd=F, jsmall=False, npad=64, NCH=1, NCHM=1, NCS=1, bound='T', half=True),
    _c("n0002_comb", 2, 2, 1, reward="comb", fwd=F, jsmall=False, npad=64, NCH=1, NCHM=1, NCS=1, bound='T', half=True),
    _c("n0063_lin", 63, 3, 1, reward="lin", fwd=S, jsmall=True, npad=64, NCH=1, NCHM=1, NCS=1, bound='T', half=True),
    _c("n0064_rbf", 64, 4, 2, "rbf", bf=8, fwd=S, jsmall=True, npad=64, NCH=1, NCHM=1, NCS=1, bound='T', half=True, lanes=False),
    _c("n0065_comb", 65, 9, 1, reward="comb", fwd=S, jsmall=True, npad=128, NCH=2, NCHM=2, NCS=2, bound='T', half=False),
    _c("n0127_none", 127, 6, 0, "none", fwd=S, npad=128, NCH=2, NCHM=2, NCS=2, bound='T', half=False),
    _c("n0128", 128, 2, 1, fwd=F, jsmall=False, npad=128, NCH=2, NCHM=2, NCS=2, bound='T', half=False, lanes=True),
    _c("n0100_e8u2", 100, 8, 2, fwd=S, jsmall=True, npad=128, NCH=2, NCHM=2, NCS=2, bound='T', half=False),
    _c("n0129_lin", 129, 7, 1, reward="lin", fwd=S, jsmall=False, npad=192, NCH=1, NCHM=1, NCS=1, bound='T', half=True),
    _c("n0191", 191, 6, 2, fwd=S, jsmall=False, npad=192, NCH=1, NCHM=1, NCS=1, bound='T', half=True),
    _c("n0192_rbf", 192, 3, 1, "rbf", bf=10, fwd=S, jsmall=False, npad=192, NCH=1, NCHM=1, NCS=1, bound='T', half=True),
    _c("n0193_comb", 193, 5, 1, reward="comb", fwd=S, jsmall=True, npad=256, NCH=4, NCHM=4, NCS=2, bound='T', half=False, lanes=True),
    _c("n0255", 255, 10, 1, fwd=S, jsmall=True, npad=256, NCH=4, NCHM=2, NCS=1, bound='cap', half=False),
    _c("n0256", 256, 1, 1, fwd=F, jsmall=False, npad=256, NCH=4, NCHM=4, NCS=4, bound='T', half=False),
    _c("n0257", 257, 4, 1, jsmall=False, fwd=F, npad=320, NCH=1, NCHM=1, NCS=1, bound='T', half=True),
    # npad / 64 = 5, 6, 7: NCH = 1, 2, 1
    _c("n0320_lin", 320, 2, 1, reward="lin", jsmall=False, fwd=F, npad=320, NCH=1, NCHM=1, NCS=1, bound='T', half=True),
    _c("n0384", 384, 3, 1, jsmall=False, fwd=F, npad=384, NCH=2, NCHM=2, NCS=1, bound='T', half=False),
    _c("n0448_u3", 448, 2, 3, jsmall=False, fwd=F, npad=448, NCH=1, NCHM=1, NCS=1, bound='T', half=True),
    # larger models
    _c("n0513", 513, 5, 1, jsmall=False, fwd=F, npad=576, NCH=1, NCHM=1, NCS=1, bound='cap', half=True),
    _c("n1000", 1000, 6, 1, H=2, jsmall=False, fwd=F, npad=1024, NCH=8, NCHM=8, NCS=1, bound='cap', half=False, lanes=True),
    _c("n1024_e1", 1024, 1, 1, H=2, jsmall=False, fwd=F, npad=1024, NCH=16, NCHM=16, NCS=4, bound='T', half=False),
    _c("n1025_u2", 1025, 3, 2, H=2, jsmall=False, fwd=F, npad=1088, NCH=1, NCHM=1, NCS=1, bound='cap', half=True),
    _c("n4097_fwd", 4097, 1, 1, H=2, grad=False, jsmall=False, fwd=F, npad=4160, NCH=1, NCHM=1, NCS=1, bound='cap', half=True),
    # three-kernel step (D > 16)
    _c("n0300_d18", 300, 17, 1, H=2, jsmall=False, fwd=T3, npad=320, NCH=1, NCHM=1, NCS=1, bound='cap', half=True),
    # user-supplied factors without iK: no diagonal pair streams iK (nd = 0)
    _c("n0200_user", 200, 3, 1, factors="user", fwd=S, jsmall=True, npad=256, NCH=4, NCHM=4, NCS=4, bound='T', half=False),
    # FITC: M inducing points
    _c("f001_n50", 50, 2, 1, M=1, fwd=F, jsmall=False, npad=64, NCH=1, NCHM=1, NCS=1, bound='T', half=True),
    _c("f001_n700", 700, 1, 1, M=1, reward="lin", fwd=F, jsmall=False, npad=64, NCH=1, NCHM=1, NCS=1, bound='T', half=True),
    _c("f063_n300", 300, 3, 1, M=63, fwd=S, jsmall=True, npad=64, NCH=1, NCHM=1, NCS=1, bound='T', half=True),
    _c("f063_n1500", 1500, 2, 2, M=63, reward="lin", fwd=S, jsmall=True, npad=64, NCH=1, NCHM=1, NCS=1, bound='T', half=True),
    _c("f064_n64", 64, 2, 2, M=64, fwd=S, jsmall=True, npad=64, NCH=1, NCHM=1, NCS=1, bound='T', half=True, lanes=True),
    _c("f064_n2000", 2000, 4, 1, M=64, reward="comb", fwd=S, jsmall=True, npad=64, NCH=1, NCHM=1, NCS=1, bound='T', half=True),
    _c("f065_n400", 400, 4, 1, M=65, fwd=S, jsmall=True, npad=128, NCH=2, NCHM=2, NCS=2, bound='T', half=False),
    _c("f065_n66", 66, 3, 3, M=65, reward="comb", fwd=S, jsmall=True, npad=128, NCH=2, NCHM=2, NCS=2, bound='T', half=False),
    _c("f128_n129", 129, 1, 5, M=128, fwd=S, jsmall=True, npad=128, NCH=2, NCHM=2, NCS=2, bound='T', half=False),
    _c("f128_n3000", 3000, 6, 1, M=128, reward="lin", fwd=F, jsmall=False, npad=128, NCH=2, NCHM=2, NCS=2, bound='T', half=False),
    _c("f192_n1000", 1000, 3, 5, M=192, fwd=S, jsmall=False, npad=192, NCH=1, NCHM=1, NCS=1, bound='T', half=True),
    _c("f192_n200", 200, 2, 6, M=192, reward="lin", fwd=S, jsmall=False, npad=192, NCH=1, NCHM=1, NCS=1, bound='T', half=True),
    _c("f256_n700", 700, 2, 6, M=256, fwd=S, jsmall=True, npad=256, NCH=4, NCHM=4, NCS=4, bound='T', half=False),
    _c("f256_n300", 300, 3, 5, M=256, reward="comb", fwd=S, jsmall=True, npad=256, NCH=4, NCHM=4, NCS=4, bound='T', half=False),
    _c("f257_n300", 300, 3, 5, M=257, reward="comb", jsmall=False, fwd=F, npad=320, NCH=1, NCHM=1, NCS=1, bound='T', half=True),
    _c("f257_n2500", 2500, 2, 6, M=257, fwd=F, jsmall=False, npad=320, NCH=1, NCHM=1, NCS=1, bound='T', half=True),
    _c("f200_n5000", 5000, 2, 6, M=200, H=3, fwd=S, jsmall=True, npad=256, NCH=4, NCHM=4, NCS=4, bound='T', half=False),
]


def case_ids():
    return [c["name"] for c in CASES]


def classes_of(c, cus=CUS, cap=3072):
    """The geometry classes case c reaches (the coverage guard of test_npoints_cpu.py wants every one of REQUIRED)."""
    g = geometry(c, cus, cap)
    out = {"fwd=" + g["fwd"], "bound=" + g["bound"], "NCH=%d" % g["NCH"], "NCHM=%d" % g["NCHM"],
           "reward=" + c["reward"], "policy=" + c["policy"], "E=%d" % c["E"]}
    if g["fwd"] == "small" or g["jsmall"]:
        out.add("NCS=%d" % g["NCS"])
    out.add("U=0" if c["U"] == 0 else "U=1" if c["U"] == 1 else "U>1")
    if c["grad"]:
        out.add("grad jsmall" if g["jsmall"] else "grad tape")
        if g["half"]:
            out.add("grad half block" + (" jsmall" if g["jsmall"] else ""))
    if g["half"]:
        out.add("half block")
    if c["factors"] == "user":
        out.add("user factors nd=0")
    if c["M"]:
        out.add("M=%d" % c["M"])
        if c["N"] >= 5000:
            out.add("FITC N=5000")
    else:
        if c["N"] in EXACT_N:
            out.add("N=%d" % c["N"])
        if c["N"] > 4096:
            out.add("N>4096")
    return out


EXACT_N = (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 320, 384, 448, 513, 1000, 1024, 1025)
REQUIRED = ({"fwd=fused", "fwd=small", "fwd=three", "bound=T", "bound=cap", "grad jsmall", "grad tape", "half block",
             "grad half block", "user factors nd=0", "FITC N=5000", "N>4096", "U=0", "U=1", "U>1", "policy=linear",
             "policy=rbf", "reward=exp", "reward=lin", "reward=comb"}
            | {"NCH=%d" % k for k in (1, 2, 4, 8, 16)} | {"NCHM=%d" % k for k in (1, 2, 4)} | {"NCS=%d" % k for k in (1, 2, 4)}
            | {"N=%d" % n for n in EXACT_N} | {"M=%d" % m for m in (1, 63, 64, 65, 128, 192, 256, 257)}
            | {"E=%d" % e for e in range(1, 11)})


def missing_classes(cases, cus=CUS, cap=3072):
    have = set()
    for c in cases:
        have |= classes_of(c, cus, cap)
    return sorted(REQUIRED - have)
