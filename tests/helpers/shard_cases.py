"""Sharded rollout cases: one table for tests/test_shard_cases_cpu.py (mirror of the ownership layout and of the gathered
Jacobian records against the library and csrc/grad_layout.h, coverage guard, mutants, sensitivity) and
tests/test_gpu_sharding.py (every case at every listed rank count against the single-rank run, the oracle and autograd).

A case is a case of helpers/npoints_cases.py or helpers/dims_cases.py, named by its name there (same shape, same make_data,
so the same oracle and autograd reference), with the rank counts W it runs at and the extra horizons (besides its own) it
runs at.  Sharding deals pair kk of the dealing order (diagonal pairs (a, a) -> kk = a first, then (a, b), b < a ->
kk = E + a (a - 1) / 2 + b) to rank kk % W as its local pair kk / W, and output a to rank a % W (csrc/api.hip deal_pairs,
build_work; csrc/shard.hip pilco_shard_plan).

The mirror (`Mirror`) restates, for rank r of W: the owner of every pair and output, PL, EL, PLcap, ELcap, SEG, OUTOFF, the
local diagonal-pair count nd, the rank's row chunks and stream-K cut (the functions of helpers/npoints_cases.py with the local
counts), the block geometry of the gathered Jacobian records (csrc/grad_layout.h jac_gather) and the host assembly map
(csrc/grad_route.hip forward_sharded): (step, record of the whole model) -> (rank block, offset).  Its class attributes are the
places where a deliberate error can be put in (test_shard_cases_cpu.py: every such mutant must fail a named check).
"""
from __future__ import annotations

from helpers import dims_cases as dc
from helpers import npoints_cases as nc
from helpers.dims_cases import TOL_FWD, TOL_GRAD, TOL_ROUTES, make_data  # noqa: F401  (the same tolerances and data)

XQ_CAP = 4096   # csrc/shard.hip peer_alloc_local: doubles of a segment the peer exchange's slots hold


def pair_index(E, a, b):
    if a < b:
        a, b = b, a
    return a if a == b else E + a * (a - 1) // 2 + b


def pairs_in_order(E):
    """(a, b) of kk = 0 .. P - 1."""
    return [(a, a) for a in range(E)] + [(a, b) for a in range(E) for b in range(a)]


def rev_dims(E, U):
    """csrc/grad_layout.h rev_dims: doubles of a pair record and of an output record."""
    D = E + U
    NT2 = D * (D + 1) // 2
    NOUT = D + NT2
    return dict(P=E * (E + 1) // 2, recp=1 + NOUT, reco=NOUT + D * D + D * NT2)


class Mirror:
    """The layout of a model of E outputs and U controls sharded over W ranks, for a rollout of H steps."""
    plcap_floor = False       # mutants (test_shard_cases_cpu.py); the real layout has all four False
    outoff_from_P = False
    swap_mod_div = False
    gblk_from_H = False

    def __init__(self, E, U, W, H=3):
        self.E, self.U, self.D, self.W, self.H = E, U, E + U, W, H
        self.P = E * (E + 1) // 2
        d = rev_dims(E, U)
        self.recp, self.reco = d["recp"], d["reco"]

    # ---- ownership (pilco_shard_plan / _pair_slot / _output_slot)
    @property
    def PLcap(self):
        return self.P // self.W if self.plcap_floor else (self.P + self.W - 1) // self.W

    @property
    def ELcap(self):
        return (self.E + self.W - 1) // self.W

    @property
    def SEG(self):
        return self.PLcap + self.ELcap * (1 + self.D)

    @property
    def OUTOFF(self):
        return self.PLcap

    def owner_of_pair(self, kk):
        return kk % self.W

    def owner_of_output(self, a):
        return a % self.W

    def PL(self, r):
        return (self.P - r + self.W - 1) // self.W if r < self.P else 0

    def EL(self, r):
        return (self.E - r + self.W - 1) // self.W if r < self.E else 0

    def nd(self, r, iK=True):
        """Local diagonal pairs that stream iK (build_work): the rank's own outputs."""
        return sum(1 for pl in range(self.PL(r)) if pl * self.W + r < self.E) if iK else 0

    def plan(self, r):
        return dict(PL=self.PL(r), EL=self.EL(r), SEG=self.SEG, OUTOFF=self.OUTOFF, P=self.P)

    def pair_slot(self, a, b):
        kk = pair_index(self.E, a, b)
        return (kk % self.W) * self.SEG + kk // self.W

    def output_slot(self, a):
        return (a % self.W) * self.SEG + self.OUTOFF + (a // self.W) * (1 + self.D)

    def rank_class(self, r):
        if r >= self.P:
            return "none"
        if r >= self.E:
            return "offdiag"
        return "both" if self.PL(r) > self.EL(r) else "diag"

    # ---- a rank's launch geometry (build_work with the local counts)
    def rank_geometry(self, r, npad, variant=2, iK=True, cus=nc.CUS, cap=3072):
        PL, EL = self.PL(r), self.EL(r)
        NCH, NCHM = nc.prep_chunks(npad, max(PL, 1), EL, cus)
        if self.W > 1:   # the mean sums' chunks come from the whole model's counts: the same bits on any rank count
            NCHM = min(nc.prep_chunks(npad, self.P, self.E, cus)[1], NCH)
        g = dict(npad=npad, PL=PL, EL=EL, NCH=NCH, NCHM=NCHM, NT=nc.pair_nt(npad, variant, max(PL, 1)), sk_waves=0, sk_total=0, sk_nd=0)
        if variant == 0 and PL > 0:
            nd = self.nd(r, iK)
            waves, T, _, _ = nc.sk_cut(npad, PL, nd, cap)
            g.update(sk_waves=waves, sk_total=T, sk_nd=nd)
        return g

    # ---- the gathered Jacobian records (grad_layout.h jac_gather, grad_route.hip forward_sharded)
    def jac_gather(self):
        out_off = (self.P if self.outoff_from_P else self.PLcap) * self.recp
        gstep = self.PLcap * self.recp + self.E * self.reco
        gblk = (self.H if self.gblk_from_H else max(self.H, 1)) * gstep
        return dict(W=self.W, P=self.P, PLcap=self.PLcap, out_off=out_off, gstep=gstep, gblk=gblk, JSg=self.P * self.recp + self.E * self.reco)

    def assembly(self):
        """[(t, destination offset in the step's JSg records, length, rank block, offset in the block)]: what the host chain's
        assembly copies, in its order: per step the P pair records, then the E output records (rank 0's)."""
        g = self.jac_gather()
        out = []
        for t in range(self.H):
            for kk in range(self.P):
                blk, loc = (kk // self.W, kk % self.W) if self.swap_mod_div else (kk % self.W, kk // self.W)
                out.append((t, kk * self.recp, self.recp, blk, t * g["gstep"] + loc * self.recp))
            out.append((t, self.P * self.recp, self.E * self.reco, 0, t * g["gstep"] + g["out_off"]))
        return out


def check_layout(m):
    """The invariants of the layout mirror m; each failure names its check."""
    E, W, P = m.E, m.W, m.P
    # partition: every pair in exactly one (rank, local index) below the rank's pair count; every output likewise
    slots = {}
    for a, b in pairs_in_order(E):
        s = m.pair_slot(a, b)
        r, k = divmod(s, m.SEG)
        assert 0 <= r < W and 0 <= k < m.PL(r) and s not in slots, "partition: pair (%d, %d) -> rank %d, local %d of %d" % (a, b, r, k, m.PL(r) if 0 <= r < W else -1)
        slots[s] = (a, b)
    assert len(slots) == P and sum(m.PL(r) for r in range(W)) == P and sum(m.EL(r) for r in range(W)) == E, "partition: counts"
    for a in range(E):
        r, k = divmod(m.output_slot(a), m.SEG)
        assert r == m.pair_slot(a, a) // m.SEG and m.OUTOFF <= k and k + 1 + m.D <= m.SEG, "partition: output %d" % a
    g = m.jac_gather()
    assert g["gblk"] >= g["gstep"] > 0, "gblk: a rank's block must hold at least one step's records (gblk %d, gstep %d)" % (g["gblk"], g["gstep"])
    asm = m.assembly()
    for t in range(m.H):
        step = [x for x in asm if x[0] == t]
        # bijection: the copies of a step tile [0, JSg) exactly
        pos = 0
        for _, dst, ln, _, _ in sorted(step, key=lambda x: x[1]):
            assert dst == pos, "bijection: step %d, destination %d after %d" % (t, dst, pos)
            pos += ln
        assert pos == g["JSg"], "bijection: step %d covers %d of JSg %d" % (t, pos, g["JSg"])
        for kk, (_, dst, ln, blk, off) in enumerate(step[:P]):
            a, b = pairs_in_order(E)[kk]
            r, k = divmod(m.pair_slot(a, b), m.SEG)
            assert (blk, off) == (r, t * g["gstep"] + k * m.recp), "owner: pair %d read from block %d offset %d, its owner is rank %d (local %d)" % (kk, blk, off, r, k)
        oblk = step[P][3]
        assert 0 <= oblk < W and m.PL(oblk) > 0, "outputs: the output records come from rank %d, which has no pairs" % oblk
    # blocks: every source range inside its rank's block, inside its step, pair records below the output records, no overlap
    src = []
    for t, dst, ln, blk, off in asm:
        assert 0 <= blk < W, "overlap: block %d of %d" % (blk, W)
        assert t * g["gstep"] <= off and off + ln <= (t + 1) * g["gstep"] <= g["gblk"], "overlap: step %d source [%d, %d) leaves its step's records (gstep %d, gblk %d)" % (t, off, off + ln, g["gstep"], g["gblk"])
        src.append((blk * g["gblk"] + off, blk * g["gblk"] + off + ln))
    src.sort()
    for (a0, a1), (b0, b1) in zip(src, src[1:]):
        assert a1 <= b0, "overlap: sources [%d, %d) and [%d, %d)" % (a0, a1, b0, b1)
    # what every rank writes into its own block: PL(r) pair records, then (a rank with pairs) the E output records at out_off
    for r in range(W):
        assert m.PL(r) * m.recp <= g["out_off"] and g["out_off"] + E * m.reco <= g["gstep"], "overlap: rank %d's %d pair records reach its output records (out_off %d, gstep %d)" % (r, m.PL(r), g["out_off"], g["gstep"])


# ---------------------------------------------------------------------------------------------------------------- cases

_BY_NAME = {c["name"]: c for c in nc.CASES}
for _c in dc.CASES:
    _d = dict(_c, grad=_c["U"] > 0 and _c["D"] <= 14, factors="device")
    _d.setdefault("lanes", False)
    _d["npad"] = nc.round_up(_c["M"] or _c["N"])
    _BY_NAME.setdefault(_c["name"], _d)


def _s(name, ranks, horizons=()):
    """The case `name` of the single-rank tables at the rank counts `ranks`; `horizons`: further horizons (besides its own)."""
    base = _BY_NAME[name]
    c = dict(base, ranks=tuple(ranks), horizons=(base["H"],) + tuple(h for h in horizons if h != base["H"]))
    c["npad"] = nc.round_up(c["M"] or c["N"])
    c["grad"] = bool(base["grad"]) and c["D"] <= 14 and (c["M"] or c["N"]) <= 1025
    return c


CASES = [
    # npad 64; E = 1 with more ranks than pairs
    _s("n0001", (2, 3), (0, 1)),
    _s("n0063_lin", (2, 3, 4), (0, 1)),
    _s("n0064_rbf", (2, 4), (1,)),
    # npad 128 / 256: several row chunks per rank
    _s("n0128", (2, 4), (0, 1)),
    _s("n0065_comb", (4, 8)),
    _s("n0127_none", (3, 7), (0, 1)),
    _s("n0193_comb", (3, 5)),
    _s("n0255", (2, 8)),
    _s("n0256", (2, 3)),
    # npad 192 / 320: an empty half block in the reverse sweep
    _s("n0129_lin", (2, 8)),
    _s("n0192_rbf", (2, 3)),
    _s("n0257", (2, 4)),
    # larger models: several row chunks per rank, the stream-K cut at capacity on every rank, on none, and on some of a group
    _s("n0384", (3,)),
    _s("n0448_u3", (2,)),
    _s("n0513", (2, 8)),
    _s("n1000", (2, 8)),
    _s("n1025_u2", (2, 4, 6)),   # W = 4: two ranks' stream-K cut at capacity, two bound by their step count
    # user factors without iK
    _s("n0200_user", (2, 4)),
    # FITC
    _s("f001_n700", (2, 3), (0, 1)),
    _s("f063_n300", (2,), (1,)),
    _s("f064_n64", (4,), (0,)),
    _s("f065_n400", (3,)),
    _s("f257_n300", (2, 6)),
    # widths: D = 12, 14 (U = 4), 15 (no Jacobian tape: forward only, the gradient is refused), 19 (three-kernel step)
    _s("d12_e6u6_hostchain", (4,)),
    _s("d14_e10u4", (2, 8)),
    _s("d15_e14u1", (3,)),
    _s("d19_e18u1", (2, 8)),
]


def case_ids():
    return ["%s-W%d" % (c["name"], W) for c in CASES for W in c["ranks"]]


def case_runs():
    return [(c, W) for c in CASES for W in c["ranks"]]


def peer_step(c, W, H):
    """The step a rollout of H steps takes with the peer exchange attached: 5 (STEP_PEER) when the segments fit its slots and the
    fused heads fit the LDS (D <= 16: helpers/dims_cases.py), else the three-kernel step with the host-mediated exchange."""
    if H <= 0:
        return 0
    m = Mirror(c["E"], c["U"], W, H)
    return 5 if c["D"] <= 16 and m.SEG <= XQ_CAP else 3


def classes_of(c, cap=3072):
    """The classes case c reaches over its rank counts and horizons (the coverage guard wants every one of REQUIRED)."""
    E, U, D, npad = c["E"], c["U"], c["D"], c["npad"]
    P = E * (E + 1) // 2
    out = {"npad=%d" % npad, "dt=%d" % nc.prep_dt(D), "reward=" + c["reward"], "model=" + ("fitc" if c["M"] else "user" if c["factors"] == "user" else "exact")}
    out |= {"H=%d" % h for h in c["horizons"]}
    if c["M"]:
        out.add("M=%d" % c["M"])
    out.add("policy=none" if c["policy"] == "none" else "policy=rbf" if c["policy"] == "rbf" else "policy=linear U=%d" % U if U <= 4 else "policy=linear U>4")
    if D > 16:
        out.add("D>16 three-kernel step under the peer exchange")
    if c["grad"]:
        out.add("grad")
        if c["M"]:
            out.add("grad fitc")
        if c["factors"] == "user":
            out.add("grad user")
        out |= {"grad H=%d" % h for h in c["horizons"]}
        out.add("grad " + ("rbf" if c["policy"] == "rbf" else "linear host chain only" if U > 4 else "linear"))
    bounds = set()
    for W in c["ranks"]:
        m = Mirror(E, U, W)
        kinds = {m.rank_class(r) for r in range(W)}
        if P % W == 0 and E % W == 0:
            out.add("W divides P and E")
        if P % W and E % W:
            out.add("W divides neither P nor E")
        out |= {"rank " + k for k in kinds}
        if E == 1 and W in (2, 3):
            out.add("E=1 W=%d" % W)
        if E == 2 and W == 4:
            out.add("E=2 W=4")
        if P == 55 and W == 8:
            out.add("55 pairs over 8 ranks")
        if W == 8:
            out.add("W=8")
        group = set()
        for r in range(W):
            g = m.rank_geometry(r, npad, 0, c["factors"] != "user", cap=cap)
            if g["PL"] > 0:
                group.add("cap" if g["sk_waves"] == cap else "T")
            if g["NCH"] > 1:
                out.add("NCH>1 npad=%d" % npad)
        bounds |= group
        if npad > 256 and group == {"cap", "T"}:
            out.add("npad>256 stream-K cap and T in one group")
    if npad > 256:
        out |= {"npad>256 stream-K " + b for b in bounds}
    if (c["M"] or c["N"]) == 1000 and E >= 6 and "cap" in bounds:
        out.add("N=1000 E>=6 stream-K at capacity")
    return out


REQUIRED = ({"W divides P and E", "W divides neither P nor E", "rank both", "rank offdiag", "rank none", "E=1 W=2", "E=1 W=3", "E=2 W=4",
             "55 pairs over 8 ranks", "W=8", "NCH>1 npad=128", "NCH>1 npad=256", "npad>256 stream-K cap", "npad>256 stream-K T", "npad>256 stream-K cap and T in one group",
             "N=1000 E>=6 stream-K at capacity", "model=exact", "model=fitc", "model=user", "policy=none", "policy=rbf",
             "reward=exp", "reward=lin", "reward=comb", "D>16 three-kernel step under the peer exchange", "H=0", "H=1", "H=3",
             "grad", "grad fitc", "grad user", "grad H=0", "grad H=1", "grad H=3", "grad rbf", "grad linear", "grad linear host chain only"}
            | {"npad=%d" % n for n in (64, 128, 192, 256, 320, 576, 1024, 1088)} | {"M=%d" % m for m in (1, 63, 64, 65, 257)}
            | {"policy=linear U=%d" % u for u in (1, 2, 3, 4)} | {"dt=%d" % d for d in (4, 6, 8, 10, 11, 12, 14, 16)})


def missing_classes(cases, cap=3072):
    have = set()
    for c in cases:
        have |= classes_of(c, cap)
    return sorted(REQUIRED - have)
