"""The division-free forms of the stream-K cut (pair_device.h: sk_cut_make, sk_boundary_fast, sk_decode_fast, sk_wave_of_fast,
sk_row_tile, sk_pair_ab_fast) against the division forms they replace in the pair kernel's start-up, on the CPU.

A host probe compiles pair_device.h -- the very functions k_mm_pair_sk calls, they are __host__ __device__ -- and compares, for
every npad = 64 .. 8192, every pair count 1 .. 528, with and without diagonal pairs, the wave counts build_work chooses at
both capacities (3072, 2048) and the cost units 5:4, 10:8, 6:5, 9:8:
  per wave        begin and end with sk_boundary_of, the decode (pair, row tile, column step, steps left in the row) of every
                  segment start with the loop / division decode, the slot of the first touched pair with sk_pair_waves;
  per local pair  (a, b) with local_pair_ab (its text taken from mm_device.h) for 1, 2, 3, 4, 8 ranks;
  ranges          sk_cut_make must call every one of these shapes fast, and the probe recomputes in 64 / 128 bits that no
                  intermediate of the 32-bit forms (w cr, x + ud - 1, the fp32 integers of the two roots, (x + 1) m_inv in 64
                  bits) leaves its width.
The two closed forms with a square root are also run over ALL their arguments with the root off by two units in the last place
either way (the device takes v_sqrt_f32, good to one): the integer fix-up must absorb it.
Negative control: each divisor's multiplier lowered by one, and the inverse multiplier halved, must show up as mismatches."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pilco_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _function(text, head):
    """The text of the function that starts with `head` (up to its closing brace at column 0)."""
    i = text.index(head)
    j = text.index("\n}\n", i)
    return text[i:j + 3]


def probe_source():
    mm = open(os.path.join(CSRC, "mm_device.h")).read()
    lpab = _function(mm, "__device__ __forceinline__ void local_pair_ab(").replace("__device__ __forceinline__", "static")
    return r'''#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>
static float g_root_scale = 1.0f;   // the square root of the closed forms, off by a few ulp on request
#define SK_SQRTF(x_) (sqrtf(x_) * g_root_scale)
#include "pair_device.h"
namespace pilco {
''' + lpab + r'''
}
using namespace pilco;
static int e_of(int P) { int E = 1; while (E * (E + 1) / 2 < P) ++E; return E; }
struct Tot { long configs = 0, waves = 0, segs = 0, bad = 0, slow = 0, over = 0; };

// every intermediate of the 32-bit forms, recomputed wide
static bool ranges_ok(const SkCut& c) {
    const unsigned long long two31 = 1ull << 31;
    const unsigned long long C = (unsigned long long)c.cq * c.waves + c.cr;
    bool ok = c.cr < (unsigned)c.waves;
    ok = ok && (unsigned long long)c.waves * c.cr <= two31;                 // w cr: numerator of the waves multiplier
    ok = ok && C + (unsigned)c.ud + (unsigned)c.uo <= two31;                // x + ud - 1, x - Ud + uo - 1, cx + 1
    ok = ok && (unsigned long long)c.total <= two31 && c.Ud <= C;           // step, r, q: numerators of tdiag, toff, ns
    ok = ok && (unsigned long long)c.nd_steps * c.ud == c.Ud;
    const unsigned s = (c.sh1 >> 16) & 255u;
    ok = ok && s < 64 && (C >> s) == 0;                                     // the estimate is less than one below the quotient
    ok = ok && (((unsigned __int128)(C + 1) * c.m_inv) >> 64) == 0;         // (cx + 1) m_inv in 64 bits
    const double b = (double)c.ns + 0.5 * PAIR_RT;
    ok = ok && b * b <= 16777216.0 && 2.0 * PAIR_RT * (double)c.tdiag <= 16777216.0;   // fp32 holds the integers of the row-tile root
    return ok;
}

static void check_config(int npad, int P, int nd, int tdiag, int toff, int waves, int ud, int uo, int tamper, Tot& t) {
    const long T = (long)nd * tdiag + (long)(P - nd) * toff;
    const int nd_steps = nd * tdiag;
    SkCut c = sk_cut_make(waves, nd, tdiag, toff, (int)T, ud, uo, npad);
    ++t.configs;
    if (!c.fast) { ++t.slow; return; }
    if (!ranges_ok(c)) ++t.over;
    switch (tamper) {
        case 1: c.m_waves -= 1; break;
        case 2: c.m_ud -= 1; break;
        case 3: c.m_uo -= 1; break;
        case 4: c.m_tdiag -= 1; break;
        case 5: c.m_toff -= 1; break;
        case 6: c.m_ns -= 1; break;
        case 7: c.m_inv /= 2; break;
        default: break;
    }
    SkCut g = c;      // the same geometry through the division forms
    g.fast = 0;
    static thread_local std::vector<int> wlo;
    wlo.resize((size_t)P);
    for (int k = 0; k < P; ++k) {
        int fs, whi;
        sk_pair_waves(k, waves, nd, tdiag, toff, (int)T, ud, uo, wlo[(size_t)k], fs, whi);
    }
    int b0 = sk_boundary_of(0, waves, nd_steps, (int)T, ud, uo);
    for (int w = 0; w < waves; ++w) {
        const int b1 = sk_boundary_of(w + 1, waves, nd_steps, (int)T, ud, uo);
        ++t.waves;
        if (sk_boundary(c, w) != b0 || sk_boundary(c, w + 1) != b1) ++t.bad;
        int step = b0;
        bool first = true;
        while (step < b1) {
            int pl, ti, sidx, cnt, pl2, ti2, sidx2, cnt2;
            sk_decode(g, step, pl, ti, sidx, cnt);
            sk_decode(c, step, pl2, ti2, sidx2, cnt2);
            ++t.segs;
            if (pl != pl2 || ti != ti2 || sidx != sidx2 || cnt != cnt2) ++t.bad;
            if (first) {
                if (sk_first_slot(c, w, pl) != w - wlo[(size_t)pl] || sk_first_slot(g, w, pl) != w - wlo[(size_t)pl]) ++t.bad;
                first = false;
            }
            step += cnt < b1 - step ? cnt : b1 - step;
        }
        b0 = b1;
    }
}

static void sweep(int npad_lo, int npad_hi, int npad_step, bool all_units, bool both_caps, int tamper, Tot& tot) {
    const int units[4][2] = {{5, 4}, {10, 8}, {6, 5}, {9, 8}};
    const int caps[2] = {3072, 2048};
    std::vector<int> npads;
    for (int npad = npad_lo; npad <= npad_hi; npad += npad_step) npads.push_back(npad);
    std::atomic<size_t> next{0};
    unsigned nt = std::thread::hardware_concurrency();
    nt = nt < 1 ? 1 : nt > 16 ? 16 : nt;
    std::vector<Tot> part(nt);
    std::vector<std::thread> th;
    for (unsigned k = 0; k < nt; ++k)
        th.emplace_back([&, k] {
            Tot& t = part[k];
            for (size_t i = next++; i < npads.size(); i = next++) {
                const int npad = npads[npads.size() - 1 - i];   // (the long ones first)
                for (int P = 1; P <= 528; ++P)
                    for (int ndk = 0; ndk < 2; ++ndk) {
                        int tdiag, toff;
                        const int NS = npad / 16, NTI = npad / (16 * PAIR_RT);   // (mm_pair_sk_steps)
                        toff = NTI * NS;
                        tdiag = NTI * NS - PAIR_RT * NTI * (NTI - 1) / 2;
                        const int nd = ndk ? (e_of(P) < P ? e_of(P) : P) : 0;
                        if (nd == 0) tdiag = toff;
                        const long T = (long)nd * tdiag + (long)(P - nd) * toff;
                        for (int ci = 0; ci < (both_caps ? 2 : 1); ++ci) {
                            const int waves = (long)caps[ci] > T ? (int)std::max<long>(4, (T + 3) / 4 * 4) : caps[ci];   // (build_work)
                            for (int u = 0; u < (all_units ? 4 : 1); ++u) check_config(npad, P, nd, tdiag, toff, waves, units[u][0], units[u][1], tamper, t);
                        }
                    }
            }
        });
    for (auto& x : th) x.join();
    for (const Tot& t : part) {
        tot.configs += t.configs; tot.waves += t.waves; tot.segs += t.segs; tot.bad += t.bad; tot.slow += t.slow; tot.over += t.over;
    }
}

int main(int argc, char** argv) {
    const int mode = atoi(argv[1]);
    if (mode == 0) {   // the whole range
        Tot t;
        sweep(64, 8192, 64, true, true, 0, t);
        std::printf("summary %ld %ld %ld %ld %ld %ld\n", t.configs, t.waves, t.segs, t.bad, t.slow, t.over);
        return 0;
    }
    if (mode == 1) {   // negative control: one constant wrong, over a few point counts
        Tot t;
        sweep(256, 1280, 256, false, false, atoi(argv[2]), t);
        std::printf("summary %ld %ld %ld %ld %ld %ld\n", t.configs, t.waves, t.segs, t.bad, t.slow, t.over);
        return 0;
    }
    // mode 2: the two closed forms with a root, over all their arguments, the root exact and two ulp off either way
    long bad = 0, checked = 0;
    const float scales[3] = {1.0f, 1.0f + 2.4e-7f, 1.0f - 2.4e-7f};
    for (float sc : scales) {
        g_root_scale = sc;
        for (int ns = 4; ns <= 512; ns += 4) {
            const int NTI = ns / PAIR_RT, tdiag = NTI * ns - PAIR_RT * NTI * (NTI - 1) / 2;
            int ti = 0, start = 0, c = ns;
            for (int q = 0; q < tdiag; ++q) {
                if (q >= start + c) { start += c; ++ti; c -= PAIR_RT; }
                ++checked;
                if (sk_row_tile(q, ns) != ti) ++bad;
            }
        }
        SkCut f{};
        f.fast = 1;
        const int ranks[5] = {1, 2, 3, 4, 8};
        for (int E = 1; E <= 32; ++E)
            for (int W : ranks)
                for (int rank = 0; rank < W; ++rank) {
                    const int P = E * (E + 1) / 2, PL = rank < P ? (P - rank + W - 1) / W : 0;
                    MMWork wk{};
                    wk.nranks = W;
                    wk.rank = rank;
                    for (int pl = 0; pl < PL; ++pl) {
                        int a, b, a2, b2;
                        local_pair_ab(wk, E, pl, a, b);
                        sk_pair_ab_fast(pl * W + rank, E, a2, b2);
                        ++checked;
                        if (a != a2 || b != b2) ++bad;
                    }
                }
    }
    std::printf("summary %ld %ld\n", checked, bad);
    return 0;
}
'''


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    d = tmp_path_factory.mktemp("sk_cut_probe")
    src = d / "sk_cut_probe.hip"
    src.write_text(probe_source())
    exe = d / "sk_cut_probe"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-pthread", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                        "-I/opt/rocm/include", str(src), "-o", str(exe)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(exe)


def _summary(exe, *args, timeout=1200):
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout, check=True).stdout
    m = re.search(r"summary ([\d ]+)", out)
    assert m, out[-2000:]
    return [int(x) for x in m.group(1).split()]


def test_fast_forms_equal_the_division_forms_everywhere(probe):
    configs, waves, segs, bad, slow, over = _summary(probe, 0)
    assert configs == 128 * 528 * 2 * 2 * 4
    assert waves > 10 ** 9 and segs >= waves // 2
    assert slow == 0, "%d shapes of the range were refused by sk_cut_make (the 32-bit forms must cover all of them)" % slow
    assert over == 0, "%d shapes were called fast although an intermediate leaves its integer width" % over
    assert bad == 0, "%d boundaries / segment decodes / first slots differ from the division forms" % bad


def test_root_forms_over_all_arguments_with_an_inexact_root(probe):
    checked, bad = _summary(probe, 2)
    tiles = sum((ns // 2) * (ns // 2 + 1) for ns in range(4, 513, 4))   # column steps of a diagonal pair, every ns
    pairs = sum(5 * E * (E + 1) // 2 for E in range(1, 33))              # every local pair of every rank, five rank counts
    assert checked == 3 * (tiles + pairs)
    assert bad == 0, "%d row tiles / (a, b) differ from the loops" % bad


@pytest.mark.parametrize("tamper", [1, 2, 3, 4, 5, 6, 7], ids=["m_waves", "m_ud", "m_uo", "m_tdiag", "m_toff", "m_ns", "m_inv"])
def test_a_wrong_constant_is_caught(probe, tamper):
    configs, waves, segs, bad, slow, over = _summary(probe, 1, tamper)
    assert configs == 5 * 528 * 2 and slow == 0
    assert bad > 0, "the comparison did not notice a multiplier that is off"


def test_the_comparison_itself_is_clean_on_the_control_range(probe):
    configs, waves, segs, bad, slow, over = _summary(probe, 1, 0)
    assert bad == 0 and over == 0 and slow == 0
