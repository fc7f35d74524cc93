"""The stream-K cut as the DEVICE computes it, and the rollouts that run on it.

pilco_debug_sk_cut_probe launches a small kernel with the pair kernel's parameter list that calls the device functions
k_mm_pair_sk calls -- the division-free forms of pair_device.h, read from the kernel-argument segment -- for every wave of the
context's current cut.  Begin, end, the decode of the first segment, the slot of the first touched pair and its outputs must be
what the host's division forms say (pilco_debug_sk_boundary, pilco_debug_sk_pair_waves, and the loops restated below), at the
smallest shapes where the forms can go wrong (helpers/npoints_cases.py):
  n0001 more waves than steps (empty waves) | n0065_comb cut bound by T, empty waves | n0255 cut bound by the capacity |
  n1024_e1 no off-diagonal pair | n0300_d18 the 2048-wave capacity (KC = 5) | n1000 | n0513 split over two ranks (two contexts
  of this process).  The border between diagonal and off-diagonal pairs lies inside a wave at n1000 and n0300_d18 (at n0255 it
  falls on a wave's first step).
For the same shapes the stream-K rollout must be bitwise repeatable and agree with the MFMA tiled pair kernel to the route
tolerance of tests/test_gpu_npoints.py (TOL_ROUTES: all shapes here have npad <= 1088).
Rollout results through the pinned block: rollout against lane 0 of rollout_batch bitwise; a rollout after a horizon change
returns the reward of the new horizon (H = 1 and H = 2: both state copies), also after a larger model made the pinned block grow;
m_H and S_H against the trajectory's last row (a download), and m_H, S_H and the reward against the three-kernel step, whose
results come down by copies."""
import ctypes as C

import numpy as np
import pytest

from helpers import npoints_cases as nc
from helpers import widths_reference as wr

pytestmark = pytest.mark.gpu

SHAPES = ["n0001", "n0065_comb", "n0255", "n1024_e1", "n0300_d18", "n1000"]
_CASES = {c["name"]: c for c in nc.CASES}
_DATA = {}


def _data(name):
    if name not in _DATA:
        _DATA[name] = nc.make_data(_CASES[name])
    return _DATA[name]


def _load(cx, case, d):
    cx.gp_set_data(0, d["X"], d["Y"])
    cx.gp_set_hyp(0, d["ls"], d["var"], d["noise"])
    cx.gp_set_inducing(0, None)
    cx.gp_factorize(0)


def _policy(case, d):
    from pilco_amd import _lib
    return dict(kind=_lib.POLICY_LINEAR, state_dim=case["E"], control_dim=case["U"], W=d["W"], b=d["b"], max_action=d["maxact"], squash=True)


def _rewards(case, d):
    from pilco_amd import _lib
    ex = dict(kind=_lib.REWARD_EXPONENTIAL, W=d["Wr"], t=d["tr"].ravel())
    li = dict(kind=_lib.REWARD_LINEAR, W=d["Wl"].ravel())
    return {"exp": [dict(ex, coef=1.0)], "lin": [dict(li, coef=1.0)], "comb": [dict(ex, coef=0.7), dict(li, coef=-0.4)]}[case["reward"]]


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))


def _decode(step, h):
    """The division / loop decode of a step of the line (what sk_wave_range did before the closed forms)."""
    NS, nd, tdiag, toff = h["npad"] // 16, h["nd"], h["tdiag"], h["toff"]
    if step < nd * tdiag:
        pl, q = divmod(step, tdiag)
        ti, c = 0, NS
        while q >= c:
            q -= c
            ti += 1
            c -= nc.PAIR_RT
        return pl, ti, ti * nc.PAIR_RT + q, c - q
    k, q = divmod(step - nd * tdiag, toff)
    ti, sidx = divmod(q, NS)
    return nd + k, ti, sidx, NS - sidx


def _pair_ab(kk, E):
    if kk < E:
        return kk, kk
    q, a = kk - E, 1
    while a * (a + 1) // 2 <= q:
        a += 1
    return a, q - a * (a - 1) // 2


def _expected(lib, h, E, W, rank):
    g = (h["waves"], h["nd"], h["tdiag"], h["toff"], h["ud"], h["uo"], h["PL"])
    bnd = [lib.pilco_debug_sk_boundary(w, *g) for w in range(h["waves"] + 1)]
    wlo = []
    out3 = (C.c_int * 3)()
    for k in range(h["PL"]):
        assert lib.pilco_debug_sk_pair_waves(k, *g, out3) == 0
        wlo.append(out3[0])
    want = np.full((h["waves"], 9), -1, dtype=np.int64)
    for w in range(h["waves"]):
        want[w, 0], want[w, 1] = bnd[w], bnd[w + 1]
        if bnd[w] < bnd[w + 1]:
            pl, ti, sidx, cnt = _decode(bnd[w], h)
            want[w, 2:7] = pl, ti, sidx, cnt, w - wlo[pl]
            want[w, 7:9] = _pair_ab(pl * W + rank, E)
    return want, bnd


def _check_probe(cx, case, what, W=1, rank=0):
    geo = cx.geometry()
    head, got = cx.sk_cut_probe()
    assert head["fast"] == 1, "%s: the workspace did not take the division-free forms" % what
    assert (head["waves"], head["total"], head["nd"], head["npad"]) == (geo["sk_waves"], geo["sk_total"], geo["sk_nd"], geo["npad"]), what
    want, bnd = _expected(cx.lib, head, case["E"], W, rank)
    assert bnd[0] == 0 and bnd[-1] == head["total"], what
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, "%s: %d of %d waves differ from the host's division forms, first wave %d: device %s, host %s" % (
        what, bad.size, head["waves"], bad[0], got[bad[0]].tolist(), want[bad[0]].tolist())
    return head, want


@pytest.fixture(scope="module")
def runs():
    """Per shape, on a context of its own: the stream-K rollout twice, the device's view of its cut, the tiled rollout."""
    from pilco_amd import _lib
    out = {}
    for name in SHAPES:
        case, d = _CASES[name], _data(name)
        cx = _lib.Context()
        try:
            _load(cx, case, d)
            pol, rw = _policy(case, d), _rewards(case, d)
            cx.set_small_step(0)      # the pair sums in the stream-K kernel's own launch, whatever the size
            a = cx.rollout(pol, rw, d["m0"], d["S0"], case["H"], want_traj=True)
            route = cx.last_route()
            b = cx.rollout(pol, rw, d["m0"], d["S0"], case["H"], want_traj=True)
            head, got = cx.sk_cut_probe()
            geo = cx.geometry()
            want, bnd = _expected(cx.lib, head, case["E"], 1, 0)
            cx.set_pair_kernel(2)
            t = cx.rollout(pol, rw, d["m0"], d["S0"], case["H"], want_traj=True)
            out[name] = dict(a=a, b=b, t=t, route=route, head=head, got=got, want=want, bnd=bnd, geo=geo)
        finally:
            cx.close()
    return out


@pytest.mark.parametrize("name", SHAPES)
def test_device_cut_equals_the_host_forms(runs, name):
    r, case = runs[name], _CASES[name]
    head, got, want, geo = r["head"], r["got"], r["want"], r["geo"]
    assert r["route"]["pair"] == 0, "the rollout did not run the stream-K pair kernel"
    assert head["fast"] == 1, "the workspace did not take the division-free forms"
    assert (head["waves"], head["total"], head["nd"], head["npad"]) == (geo["sk_waves"], geo["sk_total"], geo["sk_nd"], geo["npad"])
    assert r["bnd"][0] == 0 and r["bnd"][-1] == head["total"]
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, "%d of %d waves differ from the host's division forms, first wave %d: device %s, host %s" % (
        bad.size, head["waves"], bad[0], got[bad[0]].tolist(), want[bad[0]].tolist())
    # the shape is the edge it was chosen for
    empty = int((want[:, 0] == want[:, 1]).sum())
    nd_steps = head["nd"] * head["tdiag"]
    if name == "n0001":
        assert empty > 0
    if name == "n0065_comb":
        assert head["waves"] < geo["sk_capacity"] and head["waves"] == max(4, (head["total"] + 3) // 4 * 4)
    if name in ("n0255", "n1000"):
        assert head["waves"] == geo["sk_capacity"] == 3072
    if name in ("n1000", "n0300_d18"):
        assert ((want[:, 0] < nd_steps) & (want[:, 1] > nd_steps)).any(), "no wave spans the diagonal / off-diagonal border"
    if name == "n1024_e1":
        assert head["PL"] == 1 and head["nd"] == 1
    if name == "n0300_d18":
        assert head["waves"] == geo["sk_capacity"] == 2048


@pytest.mark.parametrize("name", SHAPES)
def test_stream_k_rollout_repeats_and_agrees_with_the_tiled_kernel(runs, name):
    r, case = runs[name], _CASES[name]
    assert _same(r["a"], r["b"]), "the stream-K rollout is not bitwise repeatable"
    err = max(wr.normwise_error(r["a"][3], r["t"][3], case["E"]),
              abs(r["a"][2][0, 0] - r["t"][2][0, 0]) / max(abs(r["t"][2][0, 0]), 1e-300))
    assert case["npad"] <= 1088 and err <= nc.TOL_ROUTES, "stream-K against tiled: %.2e (tol %.0e)" % (err, nc.TOL_ROUTES)


def test_device_cut_of_a_two_rank_split():
    from pilco_amd import _lib
    case, d = _CASES["n0513"], _data("n0513")
    pol, rw = _policy(case, d), _rewards(case, d)
    grp = []
    try:
        for rnk in range(2):
            cx = _lib.Context()
            grp.append(cx)
            cx.shard_set(rnk, 2)
            _load(cx, case, d)
        _lib.group_sync_model(grp)
        for cx in grp:
            cx.set_pair_kernel(0)
        a = _lib.rollout_group(grp, pol, rw, d["m0"], d["S0"], case["H"], want_traj=True)
        b = _lib.rollout_group(grp, pol, rw, d["m0"], d["S0"], case["H"], want_traj=True)
        assert a[4] == 0 and b[4] == 0 and _same(a[:4], b[:4])
        pls = []
        for rnk, cx in enumerate(grp):
            head, want = _check_probe(cx, case, "rank %d of 2" % rnk, W=2, rank=rnk)
            pls.append(head["PL"])
            own = sorted({(int(x[7]), int(x[8])) for x in want if x[2] >= 0})
            assert all(nc_pair_owner(case["E"], ab) == rnk for ab in own), "rank %d decodes a pair it does not own" % rnk
        assert sum(pls) == case["E"] * (case["E"] + 1) // 2
    finally:
        for cx in grp:
            cx.close()


def nc_pair_owner(E, ab):
    a, b = ab
    kk = a if a == b else E + a * (a - 1) // 2 + b
    return kk % 2


def test_rollout_results_and_reward_through_the_pinned_block():
    from pilco_amd import _lib
    small, big = _CASES["n0065_comb"], _CASES["n0513"]
    cx = _lib.Context()
    try:
        for case in (_CASES["n0001"], small, big, small):   # E = 1, 9, 5, 9: the pinned block grows twice, then is reused
            d = _data(case["name"])
            _load(cx, case, d)
            pol, rw = _policy(case, d), _rewards(case, d)
            seen = {}
            for H in (3, 1, 2, 1, 0, 2, 3):
                one = cx.rollout(pol, rw, d["m0"], d["S0"], H)
                lane = cx.rollout_batch([pol], rw, d["m0"][None], d["S0"][None], H)
                what = "%s, H = %d" % (case["name"], H)
                assert np.array_equal(one[0].ravel(), lane[0][0].ravel()) and np.array_equal(one[1], lane[1][0]), what + ": state differs from lane 0 of a batch"
                assert one[2][0, 0] == lane[2][0], what + ": reward differs from lane 0 of a batch"
                if H in seen:
                    assert _same(one, seen[H]), what + ": not the result of the earlier call with this horizon"
                seen[H] = one
            tr = cx.rollout(pol, rw, d["m0"], d["S0"], 3, want_traj=True)
            E = case["E"]
            assert np.array_equal(tr[3][-1, :E], seen[3][0].ravel()), case["name"] + ": m_H differs from the downloaded trajectory"
            assert np.array_equal(tr[3][-1, E:].reshape(E, E), seen[3][1]), case["name"] + ": S_H differs from the downloaded trajectory"
            # an independent road for all three results: the three-kernel step computes the same bits as the fused heads
            # (include/pilco_hip_dev.h: pilco_set_fused_step) and its state and reward come down by copies, not through the block
            cx.set_small_step(0)
            for H in (1, 2, 3):
                cx.set_fused_step(1)
                pinned = cx.rollout(pol, rw, d["m0"], d["S0"], H)
                assert cx.last_route()["step"] == 1, "not the fused-head route"
                cx.set_fused_step(0)
                copied = cx.rollout(pol, rw, d["m0"], d["S0"], H)
                assert cx.last_route()["step"] == 3, "not the three-kernel route"
                assert _same(pinned, copied), "%s, H = %d: results through the pinned block differ from the downloaded ones" % (case["name"], H)
            cx.set_fused_step(1)
            cx.set_small_step(1)
            rews = [seen[H][2][0, 0] for H in (0, 1, 2, 3)]
            assert len(set(rews)) == 4, "%s: horizons 0..3 returned rewards %s" % (case["name"], rews)
    finally:
        cx.close()
