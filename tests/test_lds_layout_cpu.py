"""The dynamic-LDS layouts of the reverse pass, the reverse chain and the serial link (csrc/lds_layout.h, glue_lds_carve in
csrc/glue_device.h, prep_head_lds in csrc/prep_device.h), checked on the CPU.

A host probe compiles the headers as they are (and glue_lds_doubles_for, cut out of csrc/glue.hip) and prints, per case, every
role's region offsets and total.  Cases: every case of helpers/dims_cases.py and helpers/npoints_cases.py, each rank count of
helpers/shard_cases.py, and npad in {6208, 6272, 6592, 6656} at D = 2 and D = 10 (the point counts around which k_mm_jac_rec
passes 64 KB).  Per role:
  * the regions ascend and do not overlap: offset + size <= next offset, the last one ends at or below the total.  The sizes are
    restated here from what the kernels keep in each region;
  * the regions read with 16-byte LDS accesses start at an even double: the sweep's scratch, cjl, the operand work's region
    behind the link in the fused head;
  * the launch total equals the formula of the launchers of commit e695f4f (cited at each formula) and is at most 160 KB.  The
    sweep's column split is mm_bwd_split's (cut out of csrc/bwd.hip into the probe and mirrored here): mm_bwd_geometry's, cut
    further only where that formula plus the kernel's static LDS is above 160 KB for it -- the four D = 10 edge shapes and
    (10, 1) at npad = 4224 and 4288 (55 pairs; 4160 is the last that fits), and no other case.
The link's hand-counted offsets (GlueLds::o_*) must equal the pointers' own.

Mutants (a copy of lds_layout.h with one line changed, compiled into the same probe): a region moved by one double, and the
npad term dropped from the record role: each must fail its named checks."""
import os
import shutil
import subprocess

import pytest

from helpers import dims_cases as dc
from helpers import link_cases as lc
from helpers import npoints_cases as nc
from helpers import shard_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pilco_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
LIMIT = 160 * 1024
GF_PACK, GF_ASSEMBLE, GF_PROPAGATE, GF_POLICY, GF_RBF_POST = 1, 2, 4, 32, 64   # csrc/moment.h


def _block(src, head):
    i = src.index(head)
    j = src.index("{", i)
    depth = 0
    for k in range(j, len(src)):
        depth += {"{": 1, "}": -1}.get(src[k], 0)
        if depth == 0:
            return src[i:k + 1]
    raise AssertionError("unbalanced braces after " + head)


def probe_source():
    doubles_for = _block(open(os.path.join(CSRC, "glue.hip")).read(), "size_t glue_lds_doubles_for(const GlueArgs& g) {")
    assert "glue_lds_carve(g, base, L)" in doubles_for
    bwd = open(os.path.join(CSRC, "bwd.hip")).read()
    split = _block(bwd, "void mm_bwd_geometry(int npad, int Pg, int* njs, int* nrb) {").replace("BWD_RT", "2") + "\n" + \
        _block(bwd, "void mm_bwd_split(int npad, int Pg, int kp, int* njs, int* nrb) {")
    return r'''#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "lds_layout.h"
#include "prep_device.h"
namespace pilco {
''' + doubles_for + "\n" + split + r'''
}
using namespace pilco;
int main(int argc, char** argv) {
    FILE* f = std::fopen(argv[1], "r");
    char kind[8], id[64];
    while (f && std::fscanf(f, "%7s %63s", kind, id) == 2) {
        if (!std::strcmp(kind, "R")) {
            int E, U, D, npad, kp, njs, nrb;
            if (std::fscanf(f, "%d %d %d %d %d", &E, &U, &D, &npad, &kp) != 5) return 2;
            mm_bwd_split(npad, E * (E + 1) / 2, kp, &njs, &nrb);   // (the split the launchers use)
            std::printf("%s split njs %d nrb %d\n", id, njs, nrb);
            const SweepLds s = sweep_lds(sweep_jws(npad, njs), kp);
            std::printf("%s sweep csl %d stg %d scr %d total %d launch %d\n", id, s.csl, s.stg, s.scr, s.total, lds_launch_sweep(npad, njs, kp, D));
            const HeadLds h = head_lds(D);
            std::printf("%s head G0 %d G1 %d lam %d total %d launch %d\n", id, h.G0, h.G1, h.lam, h.total, h.total);
            const PairPostLds pp = pair_post_lds((D + 16) / 16);
            std::printf("%s pair_post Gs %d Gc %d red %d total %d launch %d\n", id, pp.Gs, pp.Gc, pp.red, pp.total, lds_launch_bwd_post(D));
            const MeanPartialLds mp = mean_partial_lds(D);
            std::printf("%s mean_partial T %d zs %d lv %d lq %d u %d total %d launch %d\n", id, mp.T, mp.zs, mp.lv, mp.lq, mp.u, mp.total, lds_launch_bwd_post(D));
            const MeanFinalLds mf = mean_final_lds(D);
            std::printf("%s mean_final T %d u %d sc %d Th %d red %d TH %d total %d launch %d\n", id, mf.T, mf.u, mf.sc, mf.Th, mf.red, mf.TH, mf.total, lds_launch_bwd_fin(D));
            const FinPairsLds fp = fin_pairs_lds(D);
            std::printf("%s fin_pairs Pm %d lam %d Iv %d PI %d total %d launch %d\n", id, fp.Pm, fp.lam, fp.Iv, fp.PI, fp.total, lds_launch_bwd_fin(D));
            const JacRecLds jr = jac_rec_lds(D, npad);
            std::printf("%s jac_rec Gs %d Gc %d red %d Iv %d Pm %d lam %d PI %d cjl %d total %d launch %d\n", id, jr.post.Gs, jr.post.Gc, jr.post.red, jr.Iv, jr.Pm, jr.lam,
                        jr.PI, jr.cjl, jr.total, lds_launch_jac_rec(D, npad));
            const MeanMomentsLds mm = mean_moments_lds();
            std::printf("%s mean_moments T %d zs %d lv %d qp %d ptab %d total %d launch %d\n", id, mm.T, mm.zs, mm.lv, mm.qp, mm.ptab, mm.total, lds_launch_jac_rec(D, npad));
            const JacFinOutputLds jo = jac_fin_output_lds(D);
            std::printf("%s jac_fin_output T %d Hs %d Th %d TH %d THT %d W3 %d Z3 %d total %d launch %d\n", id, jo.T, jo.Hs, jo.Th, jo.TH, jo.THT, jo.W3, jo.Z3, jo.total,
                        lds_launch_jac_fin(D, true, E, U));
            const RevLocalLds rl = rev_local_lds(E, U);
            std::printf("%s rev_local mx %d sx %d dm %d dS %d v %d dTi %d d %d G0 %d G1 %d total %d launch %d\n", id, rl.mx, rl.sx, rl.dm, rl.dS, rl.v, rl.dTi, rl.d, rl.G0, rl.G1,
                        rl.total, lds_launch_jac_fin(D, true, E, U));
            std::printf("%s jac_fin_nolocal total %d launch %d\n", id, jo.total, lds_launch_jac_fin(D, false, E, U));
            const RevStepLds rs = rev_step_lds(E, U, D);
            std::printf("%s rev_step M1 %d s1 %d Mg %d Vg %d mx %d sx %d loc %d Wl %d gcol %d pab %d total %d launch %d\n", id, rs.M1, rs.s1, rs.Mg, rs.Vg, rs.mx, rs.sx, rs.loc,
                        rs.Wl, rs.gcol, rs.pab, rs.total, rs.total);
            const RevChainLds rc = rev_chain_lds(E, U, D);
            std::printf("%s rev_chain x %d part %d total %d launch %d\n", id, rc.x, rc.part, rc.total, rc.total);
            std::printf("%s rev_mat total %zu launch %zu\n", id, rev_mat_doubles(E, U, D), rev_mat_doubles(E, U, D));
        } else {
            GlueArgs g{};
            int DT, rewE;
            if (std::fscanf(f, "%d %d %d %d %d %d %d %d %d %d %d %d %d %d", &g.flags, &g.E, &g.D, &g.wk.SEG, &g.wk.nranks, &g.wk.EL, &g.wk.NCHM, &g.pwk.EL, &g.pwk.NCHM,
                            &g.pwk.SEG, &g.pol_inline, &g.pol_lds, &DT, &rewE) != 14) return 2;
            double* const base = reinterpret_cast<double*>(uintptr_t{1} << 20);
            GlueLds L;
            glue_lds_carve(g, base, L);
            const PrepHeadLds hd = prep_head_lds(DT, glue_lds_doubles_for(g), rewE);
            std::printf("%s link mx %td sx %td mu %td su %td cxu %td t1 %td t2 %td s1 %td jm %td js %td misc %td seg %td mp %td pol %td "
                        "o_sx %d o_s1 %d o_js %d o_seg %d o_mp %d o_misc %d total %zu work %zu gd %d bytes %zu\n", id, L.mx - base, L.sx - base, L.mu - base, L.su - base,
                        L.cxu - base, L.t1 - base, L.t2 - base, L.s1 - base, L.jm - base, L.js - base, L.misc - base, L.seg - base, L.mp - base, L.pol - base, L.o_sx, L.o_s1,
                        L.o_js, L.o_seg, L.o_mp, L.o_misc, glue_lds_doubles_for(g), (size_t)(prep_region_doubles(DT) + PREP_TAB_DOUBLES), hd.gd, hd.bytes);
        }
    }
    return 0;
}
'''


# ---------------------------------------------------------------------------------------------------------------- cases
def shapes():
    """{id: (E, U, D, npad)} of every case of the three tables and of the record role's 64 KB edge."""
    out = {}
    for c in list(dc.CASES) + list(nc.CASES) + list(sc.CASES):
        out[c["name"]] = (c["E"], c["U"], c["D"], nc.round_up(c["M"] or c["N"]))
    for E, U in ((1, 1), (9, 1)):
        for npad in (6208, 6272, 6592, 6656):
            out["edge_d%02d_npad%d" % (E + U, npad)] = (E, U, E + U, npad)
    for npad in (4160, 4224, 4288):   # 55 pairs, the columns left whole: the sweep's dynamic LDS below, at and above 160 KB
        out["edge_d11_npad%d" % npad] = (10, 1, 11, npad)
    return out


def link_runs():
    """{id: the link's arguments}: per case and rank count the links a rollout launches (csrc/rollout.hip): the whole link on one
    rank, the packing and the assembling link of a sharded step, the link behind an RbfController's own launches, the link with
    the controller evaluated inline, and the bare link of pilco_policy_action (glue_lds_bytes)."""
    out = {}
    runs = [(c, 1) for c in list(dc.CASES) + list(nc.CASES)] + list(sc.case_runs())
    for c, W in runs:
        E, U, D, npad = c["E"], c["U"], c["D"], nc.round_up(c["M"] or c["N"])
        m = sc.Mirror(E, U, W)
        g = m.rank_geometry(0, npad)
        base = dict(E=E, D=D, SEG=m.SEG, nranks=W, EL=g["EL"], NCHM=g["NCHM"], pEL=0, pNCHM=0, pSEG=0, inl=0, pol=0, DT=nc.prep_dt(D), rewE=E)
        name = "%s-W%d" % (c["name"], W)
        if W == 1:
            out[name + "-whole"] = dict(base, flags=GF_PACK | GF_ASSEMBLE | GF_PROPAGATE | GF_POLICY)
        else:
            out[name + "-pack"] = dict(base, flags=GF_PACK)
            out[name + "-assemble"] = dict(base, flags=GF_ASSEMBLE | GF_PROPAGATE | GF_POLICY)
        if c["policy"] == "rbf":
            Pu, bpad = U * (U + 1) // 2, nc.round_up(c["bf"])
            out[name + "-rbf_post"] = dict(base, flags=GF_RBF_POST | GF_POLICY, pEL=U, pNCHM=nc.prep_chunks(bpad, Pu, U)[1], pSEG=Pu + U * (1 + E))
            pol = lc.rbf_inline_lds_doubles(E, U, c["bf"])
            if pol:
                out[name + "-rbf_inline"] = dict(out[name + ("-whole" if W == 1 else "-assemble")], inl=1, pol=pol)
        out[name + "-bare"] = dict(base, flags=0)
    return out


LINK_FIELDS = ("flags", "E", "D", "SEG", "nranks", "EL", "NCHM", "pEL", "pNCHM", "pSEG", "inl", "pol", "DT", "rewE")


def run_probe(tmp, include_first=None):
    src = tmp / "lds_probe.hip"
    src.write_text(probe_source())
    exe = tmp / "lds_probe"
    inc = (["-I" + str(include_first)] if include_first else []) + ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-I/opt/rocm/include"]
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-std=c++17"] + inc + [str(src), "-o", str(exe)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = []
    for name, (E, U, D, npad) in shapes().items():
        lines.append("R %s %d %d %d %d %d" % (name, E, U, D, npad, nc.mm_kp(D)))
    for name, a in link_runs().items():
        lines.append("L %s " % name + " ".join(str(a[k]) for k in LINK_FIELDS))
    inp = tmp / "cases.txt"
    inp.write_text("\n".join(lines) + "\n")
    txt = subprocess.run([str(exe), str(inp)], capture_output=True, text=True, timeout=600, check=True).stdout
    rows = {}
    for ln in txt.split("\n"):
        w = ln.split()
        if w:
            rows[(w[0], w[1])] = {w[i]: int(w[i + 1]) for i in range(2, len(w), 2)}
    assert len(rows) == 15 * len(shapes()) + len(link_runs())
    return rows


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    return run_probe(tmp_path_factory.mktemp("lds_probe"))


# ---------------------------------------------------------------------------------------------------------------- checks
def sweep_doubles(npad, njs, kp):
    """The sweep role's LDS as the launchers of commit e695f4f computed it (bwd.hip:1312, 1378; bwd_tp: bwd.hip:42)."""
    return 4 * 16 * ((npad // 16 + njs - 1) // njs) + 2 * (64 * (17 if kp <= 16 else kp + 1) + 2 * 64) + 4 * 4 * 72


# static LDS of the role's kernel beside the dynamic (bytes; -Rpass-analysis=kernel-resource-usage, docs/lds_layouts.md): the sweep's
# exp table, k_mm_bwd_fin's flag, k_rev_step's and k_rev_chain's reduction buffers
STATIC = {"sweep": 2048, "mean_final": 16, "fin_pairs": 16, "rev_step": 256, "rev_chain": 4096}


def bwd_split(npad, Pg, kp):
    """csrc/bwd.hip mm_bwd_split -> (njs, nrb, njs of mm_bwd_geometry): the geometry's split, doubled (up to 4) while the parent's
    formula for that split, with the kernel's 2 048 static bytes, is above 160 KB -- a sweep that could not be launched.  A split that fits is the parent's."""
    njs0, nrb = nc.bwd_geometry(npad, Pg)
    njs = njs0
    while 2 * njs <= 4 and 8 * sweep_doubles(npad, njs, kp) + STATIC["sweep"] > LIMIT:
        njs *= 2
    return njs, nrb, njs0


def region_sizes(role, E, U, D, npad, njs, kp):
    """[(region, doubles)] in layout order: what the role's device function keeps there (csrc/bwd.hip, rev_local.h, rev.hip)."""
    nI, P = D * D, E * (E + 1) // 2
    NT2 = D * (D + 1) // 2
    NX, NOUT = E + P, D + NT2
    NR = NX + U * E + U
    nmt = (D + 16) // 16
    jws = 16 * ((npad // 16 + njs - 1) // njs)
    NS = (D + 1) * (D + 2) * (D + 3) // 6
    loc = E + E * E + 2 * U * E + 2 * U + 9 * U * U
    return {
        "sweep": [("csl", 4 * jws), ("stg", 2 * (64 * (17 if kp <= 16 else kp + 1) + 2 * 64)), ("scr", 4 * 4 * 72)],
        "head": [("G0", 2 * nI), ("G1", 2 * nI), ("lam", D)],
        "pair_post": [("Gs", 256 * nmt * nmt), ("Gc", 256 * nmt * nmt), ("red", 4 * 256)],
        "mean_partial": [("T", nI), ("zs", 64 * (D | 1)), ("lv", 64), ("lq", 64), ("u", D + 2)],
        "mean_final": [("T", nI), ("u", D + 2), ("sc", 2), ("Th", D), ("red", nI + 2 * D + 1), ("TH", nI)],
        "fin_pairs": [("Pm", nI), ("lam", D + 2), ("Iv", 1 + D + nI), ("PI", nI)],
        "jac_rec": [("Gs", 256), ("Gc", 256), ("red", 1024), ("Iv", 1 + D + nI), ("Pm", nI), ("lam", D + 2), ("PI", 2 * nI), ("cjl", npad)],
        "mean_moments": [("T", 256), ("zs", 64 * 17), ("lv", 64), ("qp", 4 * 256), ("ptab", 16 * 8 // 2)],
        "jac_fin_output": [("T", nI), ("Hs", NS), ("Th", D), ("TH", nI), ("THT", nI), ("W3", nI * D), ("Z3", nI * D)],
        "rev_local": [("mx", E), ("sx", E * E), ("dm", E), ("dS", E * E), ("v", E), ("dTi", E), ("d", E), ("G0", 2 * E * E), ("G1", max(2 * E * E, 2 * U * E + U - 2 * E * E))],   # (T1 | T2 | mu0 reuse G0 .. afterwards)
        "rev_step": [("M1", NX * NOUT), ("s1", E * D), ("Mg", E), ("Vg", E * D), ("mx", E), ("sx", E * E), ("loc", loc), ("Wl", U * E), ("gcol", NX * (U + U * U)),
                     ("pab", (P + 1) // 2)],
        "rev_chain": [("x", NX + 1), ("part", (512 // NR) * NR if NR <= 512 else 0)],
    }[role]


def parent_launch(role, E, U, D, npad, njs, kp):
    """The launch's LDS in doubles as the launchers of commit e695f4f computed it (file:line there)."""
    nI, P = D * D, E * (E + 1) // 2
    NX, NOUT, NR = E + P, D + D * (D + 1) // 2, E + P + U * E + U
    nmt, LD = (D + 16) // 16, D | 1
    NS = (D + 1) * (D + 2) * (D + 3) // 6
    rev_local = 2 * (E + E * E) + 3 * E + max(4 * E * E, 2 * U * E + U) + 8                                  # rev_local.h:136-139
    jac_fin = max(4 * nI + 4 * D + 8, 3 * nI + NS + D + 2 * nI * D)                                         # bwd.hip:1345
    sweep = max(sweep_doubles(npad, njs, kp), 4 * nI + D)                                                  # bwd.hip:1312, 1378
    post = max(2 * 256 * nmt * nmt + 4 * 256, nI + 64 * LD + 128 + D + 2)                                   # bwd.hip:1384
    fin = 3 * nI + 4 * D + 8                                                                                # bwd.hip:1394
    rec = max(6 * 256 + (1 + D + nI) + 3 * nI + D + 2 + 1 + npad, 256 + 64 * 17 + 64 + 4 * 256 + 8 * 8 + 2)   # bwd.hip:1353
    return {
        "sweep": sweep, "head": 4 * nI + D,                                                                 # bwd.hip:1343
        "pair_post": post, "mean_partial": post, "mean_final": fin, "fin_pairs": fin, "jac_rec": rec, "mean_moments": rec,
        "jac_fin_output": max(jac_fin, rev_local), "rev_local": max(jac_fin, rev_local), "jac_fin_nolocal": jac_fin,   # bwd.hip:1345-1346
        "rev_step": NX * NOUT + 2 * E * D + E + E + E * E + (E + E * E + 2 * U * E + 2 * U + 9 * U * U) + U * E + NX * (U + U * U) + (P + 1) // 2 + 2,   # rev.hip:49-53
        "rev_chain": NX + 1 + (512 // NR) * NR if NR <= 512 else None,                                      # rev.hip:360
        "rev_mat": NX * NR + NX + 4,                                                                        # rev.hip:34-37
    }[role]


EVEN = {"sweep": ("scr",), "jac_rec": ("cjl",)}


def applies(role, E, U, D):
    """Roles a shape can run: the Jacobian tape serves D <= 14 with controls, the device chain U <= 4 on top (NR <= 512)."""
    if role in ("jac_rec", "mean_moments", "jac_fin_output", "rev_local", "jac_fin_nolocal"):
        return U > 0 and D <= 14
    if role in ("rev_step", "rev_chain", "rev_mat"):
        return 0 < U <= 4 and D <= 14
    return True


def role_failures(rows, limit=False):
    """Failures of the layout checks; limit=True: the launches above 160 KB instead."""
    bad, over = [], []
    for name, (E, U, D, npad) in shapes().items():
        kp = nc.mm_kp(D)
        njs, nrb, njs0 = bwd_split(npad, E * (E + 1) // 2, kp)
        if rows[(name, "split")] != dict(njs=njs, nrb=nrb):
            bad.append("split: %s mm_bwd_split gives %s, the mirror (%d, %d)" % (name, rows[(name, "split")], njs, nrb))
        if njs != njs0 and 8 * sweep_doubles(npad, njs0, kp) + STATIC["sweep"] <= LIMIT:
            bad.append("split: %s a split that fitted (%d) was changed to %d" % (name, njs0, njs))
        for (rid, role), r in rows.items():
            if rid != name or role in ("link", "split") or not applies(role, E, U, D):
                continue
            if role not in ("jac_fin_nolocal", "rev_mat"):
                regs = region_sizes(role, E, U, D, npad, njs, kp)
                pos = 0
                for reg, size in regs:
                    if r[reg] < pos:
                        bad.append("overlap: %s %s.%s at %d, the region before it ends at %d" % (name, role, reg, r[reg], pos))
                    pos = r[reg] + size
                if pos > r["total"]:
                    bad.append("overlap: %s %s ends at %d, total %d" % (name, role, pos, r["total"]))
                if r["total"] > r["launch"]:
                    bad.append("launch: %s %s total %d above its launch's %d" % (name, role, r["total"], r["launch"]))
                for reg in EVEN.get(role, ()):
                    if r[reg] % 2:
                        bad.append("aligned: %s %s.%s at %d" % (name, role, reg, r[reg]))
            want = parent_launch(role, E, U, D, npad, njs, kp)
            if r["launch"] != want:
                bad.append("total: %s %s asks for %d doubles, the parent's launcher for %s" % (name, role, r["launch"], want))
            if role != "rev_mat" and 8 * r["launch"] + STATIC.get(role, 0) > LIMIT:
                over.append("limit: %s %s asks for %d bytes and %d static" % (name, role, 8 * r["launch"], STATIC.get(role, 0)))
    return over if limit else bad


def link_failures(rows):
    bad = []
    order = ("mx", "sx", "mu", "su", "cxu", "t1", "t2", "s1", "jm", "js", "misc", "seg", "mp", "pol")
    for name, a in link_runs().items():
        r = rows[(name, "link")]
        E, D = a["E"], a["D"]
        nm = max(E, D)
        seg_n = a["SEG"] * (1 if a["flags"] & GF_PACK else a["nranks"]) if a["flags"] & (GF_PACK | GF_ASSEMBLE) else 0
        mp_n = a["EL"] * a["NCHM"] * (1 + D) if a["flags"] & GF_PACK else 0
        if a["flags"] & GF_RBF_POST:
            seg_n, mp_n = a["pSEG"], a["pEL"] * a["pNCHM"] * (1 + E)
        sizes = dict(mx=nm, sx=nm * nm, mu=nm, su=nm * nm, cxu=nm * nm, t1=nm * nm, t2=nm * nm, s1=nm * nm, jm=nm, js=nm * nm, misc=256, seg=seg_n, mp=mp_n, pol=0)
        pos = 0
        for reg in order:
            if r[reg] < pos:
                bad.append("overlap: %s link.%s at %d, the region before it ends at %d" % (name, reg, r[reg], pos))
            pos = r[reg] + sizes[reg]
        for reg in ("sx", "s1", "js", "seg", "mp", "misc"):
            if r["o_" + reg] != r[reg]:
                bad.append("offset: %s link o_%s = %d, the pointer is at %d" % (name, reg, r["o_" + reg], r[reg]))
        rew = E + 4 * E * E + E * (E + 1) + E + 16                                                          # mm_device.h: reward_lds_doubles
        want = 3 * nm + 7 * nm * nm + 256 + max(seg_n + mp_n, rew) + (a["pol"] if (a["flags"] & GF_POLICY) and a["inl"] else 0)   # glue.hip:6-21
        if r["total"] != want:
            bad.append("total: %s link asks for %d doubles, the parent's launcher for %d" % (name, r["total"], want))
        if a["D"] <= 16 and 8 * r["total"] > LIMIT:
            bad.append("limit: %s link asks for %d bytes" % (name, 8 * r["total"]))
        # the fused head: prep.hip:39-41, 54, 57 and prep_kernel.h:121
        gd = (want + 1) & ~1
        lds_rw = 8 * (a["rewE"] + a["rewE"] ** 2 + (a["rewE"] + 4 * a["rewE"] ** 2 + a["rewE"] * (a["rewE"] + 1) + a["rewE"] + 16)) if a["rewE"] > 0 else 0
        if r["gd"] % 2 or r["gd"] < r["total"]:
            bad.append("aligned: %s fused head: the operand work's region at %d behind a link of %d" % (name, r["gd"], r["total"]))
        if r["gd"] != gd or r["bytes"] != max(8 * r["work"], lds_rw) + 8 * gd:
            bad.append("total: %s fused head asks for %d bytes (link region %d), the parent's launcher for %d (%d)" % (name, r["bytes"], r["gd"], max(8 * r["work"], lds_rw) + 8 * gd, gd))
        if a["D"] <= 16 and r["bytes"] > LIMIT:
            bad.append("limit: %s fused head asks for %d bytes" % (name, r["bytes"]))
    return bad


def test_every_role_s_regions_and_totals(probe):
    bad = role_failures(probe)
    assert not bad, "%d failures, first: %s" % (len(bad), bad[:5])


def test_no_launch_asks_for_more_than_160_kb(probe):
    """With mm_bwd_geometry's split alone the sweep would not fit at the D = 10 edge shapes (E = 9: 45 pairs, njs = 1 from
    npad = 4416 on, 227 328 .. 241 664 bytes at npad = 6208 .. 6656), nor with 55 pairs at npad = 4224 (163 840 dynamic bytes and
    the kernel's 2 048 static ones) and 4288; mm_bwd_split cuts the columns further there, and at no other shape of the tables.
    Every launch's dynamic and static bytes together are within 160 KB."""
    edge = [n for n, (E, U, D, npad) in shapes().items() if bwd_split(npad, E * (E + 1) // 2, nc.mm_kp(D))[0] != nc.bwd_geometry(npad, E * (E + 1) // 2)[0]]
    assert sorted(edge) == ["edge_d10_npad%d" % n for n in (6208, 6272, 6592, 6656)] + ["edge_d11_npad4224", "edge_d11_npad4288"], edge
    assert 8 * sweep_doubles(4224, 1, 12) == LIMIT   # (the dynamic part alone fits at npad = 4224: the exp table does not)
    over = role_failures(probe, limit=True)
    assert not over, "%d launches above 160 KB, first: %s" % (len(over), over[:4])


def test_the_link_s_regions_offsets_and_totals(probe):
    bad = link_failures(probe)
    assert not bad, "%d failures, first: %s" % (len(bad), bad[:5])


def test_the_record_role_passes_64_kb_where_the_issue_says(probe):
    """D = 2: 65 728 bytes at npad = 6656, below 64 KB at 6592; D = 10: above from npad = 6272."""
    b = lambda name: 8 * probe[(name, "jac_rec")]["launch"]
    assert b("edge_d02_npad6656") == 65728 and b("edge_d02_npad6592") <= 65536
    assert b("edge_d10_npad6272") > 65536 >= b("edge_d10_npad6208")


MUTANTS = {
    "a region moved by one double": ("    l.Th = l.sc + 2;\n", "    l.Th = l.sc + 1;\n", ("overlap:", "total:")),
    "the npad term dropped from the record role": ("    l.total = end + npad;\n", "    l.total = end;\n", ("overlap:", "total:")),
}


@pytest.mark.parametrize("name", list(MUTANTS))
def test_a_mutant_of_the_header_fails_its_named_checks(name, tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    old, new, checks = MUTANTS[name]
    text = open(os.path.join(CSRC, "lds_layout.h")).read()
    assert text.count(old) == 1, old
    (tmp_path / "lds_layout.h").write_text(text.replace(old, new))
    bad = role_failures(run_probe(tmp_path, include_first=tmp_path))
    for check in checks:
        assert any(b.startswith(check) for b in bad), "%s: no '%s' failure among %s" % (name, check, bad[:5])
