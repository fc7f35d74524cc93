"""The hot loop of the headline pair kernel (k_mm_pair_sk<3, false>: N = 1000, D = 10) in the generated gfx950 code, checked
on the CPU: every 16-column step is one basic block with the step's 6 v_mfma_f64_16x16x4_f64, and the table exp there takes
the biased-table form (csrc/mm_device.h: fexp_scale) -- one v_lshl_add_u32 per exp inserts the exponent into the table
value, no v_and_b32 drops the index bits of n.  Off-diagonal step: 99 VALU operations (107 with the unbiased table)."""
import collections
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KERNEL = "_ZN5pilco12k_mm_pair_skILi3ELb0EEEvNS_7MMModelENS_6MMWorkE"
NE = 8   # exps per lane and step: PAIR_RT = 2 row tiles of 4 result registers


def _blocks(asm, name):
    body, on = [], False
    for line in open(asm).read().split("\n"):
        if line.startswith(name + ":"):
            on = True
            continue
        if on and (line.startswith(".Lfunc_end") or re.match(r"^\s*\.size", line)):
            break
        if on:
            body.append(line)
    blocks, cur = [], None
    for line in body:
        m = re.match(r"^(\.LBB\S+):", line)
        if m:
            cur = []
            blocks.append(cur)
            continue
        s = line.split(";")[0].strip()
        if cur is None or not s or s.startswith("."):
            continue
        cur.append(s.split()[0])
    return blocks


@pytest.fixture(scope="module")
def steps(tmp_path_factory):
    asm = str(tmp_path_factory.mktemp("pair_isa") / "pair.s")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include",
           "-mllvm", "-amdgpu-mfma-vgpr-form", "-S", "--cuda-device-only", "-o", asm, os.path.join(ROOT, "pilco_amd", "csrc", "pair.hip")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stderr[-2000:]
    out = []
    for ops in _blocks(asm, KERNEL):
        if sum(op.startswith("v_mfma") for op in ops) == 6:
            valu = collections.Counter(op for op in ops if op.startswith("v_") and not op.startswith("v_mfma"))
            if sum(valu.values()) > 20:   # (the prologue's blocks carry MFMAs with a couple of moves only)
                out.append(valu)
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_pair_step_exp_uses_the_biased_table(steps):
    assert len(steps) == 2, steps   # the diagonal and the off-diagonal step
    for valu in steps:
        assert not any(op.startswith("v_and_b32") for op in valu), valu
        assert valu["v_lshl_add_u32"] == NE, valu
        assert valu["v_max_f64"] == NE, valu                  # the -700 clamp
        assert valu["v_lshlrev_b32_sdwa"] == NE, valu         # the table address


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_pair_offdiagonal_step_valu_count(steps):
    assert min(sum(v.values()) for v in steps) == 99, steps
