"""The case table of the input-width tests (helpers/dims_cases.py), checked on the CPU.

Coverage guard: the operand kernel's instantiations (the launch_prep_N dispatch in csrc/prep.hip) and the stream-K pair kernel's
contraction depths (the `case k:` list of its dispatch in csrc/pair.hip) are read from the source, KP(D) and vsep(D) from
csrc/moment.h (a host-only probe compiled against the header checks the mirror below).  Every DT bucket must be reached at both
of its edges and every (KC, vsep) that D = 1..32 produces by some case: a new instantiation without a case fails here.

Sensitivity: for every case, two errors a kernel could make -- the last point left out of the pair sums, the last input
dimension left out of the pair exponent -- must each move the H-step trajectory by at least 10 x the forward tolerance, so that
the GPU test's tolerance can see them on that case's data."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from helpers import dims_cases as dc
from helpers import widths_reference as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pilco_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def mm_vsep(D):   # mirror of csrc/moment.h mm_vsep / mm_kp (test_kp_mirror_matches_the_header)
    return (D + 2) % 4 == 1


def mm_kp(D):
    return D + 1 if mm_vsep(D) else (D + 2 + 3) // 4 * 4


def prep_dispatch():
    """D -> DT of launch_mm_prep, read from the if / else-if chain in csrc/prep.hip."""
    src = open(os.path.join(CSRC, "prep.hip")).read()
    body = src[src.index("void launch_mm_prep("):]
    rules = re.findall(r"if \(D (<=|==) (\d+)\) launch_prep_(\d+)\(a\);", body)
    last = re.search(r"\belse launch_prep_(\d+)\(a\);", body)
    assert rules and last, "launch_prep_N dispatch not found in prep.hip"
    out = {}
    for D in range(1, 33):
        for op, v, dt in rules:
            if (op == "<=" and D <= int(v)) or (op == "==" and D == int(v)):
                out[D] = int(dt)
                break
        else:
            out[D] = int(last.group(1))
    return out


def pair_sk_depths():
    """Contraction depths KC = KP / 4 instantiated for k_mm_pair_sk (the PS switch of launch_mm_pair) and the default's."""
    src = open(os.path.join(CSRC, "pair.hip")).read()
    cases = {int(k) for k, v in re.findall(r"case (\d+): PS\((\d+)\); break;", src) if k == v}
    dflt = re.search(r"default: PS\((\d+)\); break;", src)
    assert cases and dflt, "k_mm_pair_sk dispatch not found in pair.hip"
    return cases, int(dflt.group(1))


def test_kp_mirror_matches_the_header(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    probe = tmp_path / "kp_probe.hip"
    probe.write_text('#include <cstdio>\n#include "moment.h"\n'
                     'int main() { for (int D = 1; D <= 32; ++D) std::printf("%d %d %d\\n", D, pilco::mm_kp(D), (int)pilco::mm_vsep(D)); return 0; }\n')
    exe = tmp_path / "kp_probe"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-I/opt/rocm/include",
                        str(probe), "-o", str(exe)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, check=True).stdout.split("\n")
    got = {int(a): (int(b), bool(int(c))) for a, b, c in (ln.split() for ln in out if ln.strip())}
    assert got == {D: (mm_kp(D), mm_vsep(D)) for D in range(1, 33)}


def test_case_table_reaches_every_instantiation():
    widths = {c["D"] for c in dc.CASES}
    dt = prep_dispatch()
    missing = []
    for bucket in sorted(set(dt.values())):
        ds = [D for D in dt if dt[D] == bucket]
        for edge in (min(ds), max(ds)):
            if edge not in widths:
                missing.append("DT=%d edge D=%d" % (bucket, edge))
    cases, dflt = pair_sk_depths()
    reach = {(mm_kp(D) // 4, mm_vsep(D)) for D in range(1, 33)}
    assert len(reach) == 17
    for kc, _ in reach:
        assert kc in cases or kc == dflt, "KC=%d has no k_mm_pair_sk instantiation" % kc
    have = {(mm_kp(D) // 4, mm_vsep(D)) for D in widths}
    missing += ["KC=%d vsep=%d" % p for p in sorted(reach - have)]
    assert not missing, "instantiations no case of helpers/dims_cases.py reaches: %s" % missing


def test_case_table_covers_the_named_shapes():
    by = {(c["E"], c["U"]): c for c in dc.CASES}
    assert (32, 0) in by and (31, 1) in by and (28, 4) in by
    assert any(c["U"] in (5, 6) and c.get("chain") == "host" and c["D"] <= 14 for c in dc.CASES)
    rbf = [c for c in dc.CASES if c["policy"] == "rbf" and c["E"] >= 12]
    assert {c["policy_route"] for c in rbf} == {"inline", "own"}
    assert {c.get("rev") for c in dc.CASES if c.get("chain") == "device"} == {"above", "below"}
    assert sorted(c["M"] for c in dc.CASES if c["M"]) == [64, 65, 257]
    assert {16, 24, 32} <= {c["D"] for c in dc.CASES if not c["M"] and c["N"] > 256}
    assert len({c["name"] for c in dc.CASES}) == len(dc.CASES)


@pytest.mark.parametrize("case", dc.CASES, ids=dc.case_ids())
def test_forward_tolerance_sees_a_dropped_point_and_a_dropped_dimension(case):
    d = dc.make_data(case)
    ref, r_ref = wr.oracle_trajectory(case, d)
    same, r_same = wr.perturbed_trajectory(case, d)
    E = case["E"]
    assert wr.normwise_error(same, ref, E) < 0.1 * dc.TOL_FWD and abs(r_same - r_ref) <= 0.1 * dc.TOL_FWD * max(1.0, abs(r_ref))
    # an informative model: the states move, and not as prior-only outputs would
    assert np.abs(ref[-1, :E] - ref[0, :E]).max() > 1e-3
    for damage in ("drop_point", "drop_dim"):
        bad, _ = wr.perturbed_trajectory(case, d, **{damage: True})
        err = wr.normwise_error(bad, ref, E)
        assert err >= 10 * dc.TOL_FWD, "%s: %s moves the trajectory by %.2e only" % (case["name"], damage, err)
