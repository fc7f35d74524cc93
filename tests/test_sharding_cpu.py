"""CPU tests of the multi-GPU exchange contract (no GPU needed).

The per-step exchange of the sharded rollout is one all-gather of fixed-size
segments; which pair / output lands where is defined by pure host functions of
libpilco_hip.so (pilco_shard_plan / _pair_slot / _output_slot).  Here two gloo
ranks each evaluate their share of one moment-matching step with the CPU oracle,
pack it with those functions, all-gather over torch.distributed (gloo) and
assemble -- the result must equal the single-process oracle.  This is the N>1
path of bench.py minus the device kernels (which test_gpu_parity.py covers with
two contexts on one GPU)."""
import os
import socket
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_declared_symbol_is_exported():
    """The C-ABI library loads and exports every symbol include/*.h declares (pilco_hip.h: the boundary; pilco_hip_dev.h: the
    measurement / developer entry points of the same library), and the boundary header is free of developer entry points."""
    import glob
    import re
    from pilco_amd import _lib
    lib = _lib.load_library()
    hdr = "".join(open(f).read() for f in sorted(glob.glob(os.path.join(ROOT, "include", "*.h"))))
    boundary = open(os.path.join(ROOT, "include", "pilco_hip.h")).read()
    assert not re.findall(r"\b(pilco_debug_[a-z0-9_]+|pilco_[a-z_]*_timed|pilco_[gs]et_pair_timing)\s*\(", boundary)
    declared = set(re.findall(r"\b(pilco_[a-z0-9_]+)\s*\(", hdr))
    declared -= {"pilco_ctx", "pilco_status"}
    assert declared, "no declarations parsed"
    missing = [n for n in sorted(declared) if not hasattr(lib, n)]
    assert not missing, f"symbols declared in the header but not exported: {missing}"
    unbound = [n for n in sorted(declared) if n not in _lib.SIGNATURES]
    assert not unbound, f"symbols without a ctypes signature: {unbound}"
    assert lib.pilco_abi_version() == 2


def test_no_cpu_fallback_without_gpu():
    """Compute calls fail loudly when no MI355X is visible (there is no CPU path)."""
    from pilco_amd import _lib
    import ctypes as C
    h = C.c_void_p()
    rc = _lib.load_library().pilco_ctx_create(0, C.byref(h))
    if rc == 0:
        pytest.skip("a GPU is visible here")
    with pytest.raises(_lib.PilcoError):
        _lib.Context(device=0)


@pytest.mark.parametrize("E,D,W", [(10, 10, 8), (10, 11, 4), (2, 3, 2), (3, 5, 5), (4, 4, 1)])
def test_shard_plan_is_a_partition(E, D, W):
    from pilco_amd import _lib
    P = E * (E + 1) // 2
    plans = [_lib.shard_plan(E, D, W, r) for r in range(W)]
    assert sum(p["PL"] for p in plans) == P and sum(p["EL"] for p in plans) == E
    assert len({p["SEG"] for p in plans}) == 1
    SEG = plans[0]["SEG"]
    slots = set()
    for a in range(E):
        for b in range(a + 1):
            s = _lib.shard_pair_slot(E, D, W, a, b)
            assert s == _lib.shard_pair_slot(E, D, W, b, a)
            r, k = divmod(s, SEG)
            assert 0 <= r < W and k < plans[r]["PL"]
            slots.add(s)
    assert len(slots) == P
    for a in range(E):
        s = _lib.shard_output_slot(E, D, W, a)
        r, k = divmod(s, SEG)
        # the owner of output a is the owner of pair (a,a)
        assert r == _lib.shard_pair_slot(E, D, W, a, a) // SEG
        assert plans[r]["OUTOFF"] <= k and k + 1 + D <= SEG
    assert max(p["PL"] for p in plans) - min(p["PL"] for p in plans) <= 1


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist
    from oracle import tf_path as tp
    from pilco_amd import _lib, synthetic
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group(backend="gloo", rank=rank, world_size=world)
    try:
        # the RCCL unique id travels as 128 opaque bytes: same broadcast as bench.py
        id_t = torch.zeros(_lib.COMM_ID_BYTES, dtype=torch.uint8)
        if rank == 0:
            id_t = torch.arange(_lib.COMM_ID_BYTES, dtype=torch.uint8)
        dist.broadcast(id_t, src=0)
        assert bytes(id_t.numpy().tobytes()) == bytes(range(_lib.COMM_ID_BYTES))
        c = synthetic.config_c2(N=60, D=5, E=4, noise=1e-2, seed=3, control_dim=1)
        E, D = 4, 5
        rs = np.random.RandomState(0)
        m = 0.2 * rs.randn(1, D)
        A = 0.3 * rs.randn(D, D)
        s = A @ A.T + 0.05 * np.eye(D)
        iK, beta = tp.calculate_factorizations(c["X"], c["Y"], c["lengthscales"], c["variance"], c["noise"])
        Mo, So, Vo = tp.predict_given_factorizations(c["X"], c["lengthscales"], c["variance"], m, s, iK, beta)
        plan = _lib.shard_plan(E, D, world, rank)
        seg = np.zeros(plan["SEG"])
        # a rank fills only what it owns; values before "+ var - M M^T": S_ab + M_a M_b - delta var_a
        for a in range(E):
            for b in range(a + 1):
                slot = _lib.shard_pair_slot(E, D, world, a, b)
                if slot // plan["SEG"] == rank:
                    seg[slot % plan["SEG"]] = So[a, b] + Mo[0, a] * Mo[0, b] - (c["variance"][a] if a == b else 0.0)
            slot = _lib.shard_output_slot(E, D, world, a)
            if slot // plan["SEG"] == rank:
                k = slot % plan["SEG"]
                seg[k] = Mo[0, a]
                seg[k + 1:k + 1 + D] = Vo[:, a]
        gathered = [torch.zeros(plan["SEG"], dtype=torch.float64) for _ in range(world)]
        dist.all_gather(gathered, torch.from_numpy(seg))
        g = torch.cat(gathered).numpy()
        M = np.array([[g[_lib.shard_output_slot(E, D, world, a)] for a in range(E)]])
        V = np.stack([g[_lib.shard_output_slot(E, D, world, a) + 1:_lib.shard_output_slot(E, D, world, a) + 1 + D] for a in range(E)], axis=1)
        S = np.empty((E, E))
        for a in range(E):
            for b in range(E):
                S[a, b] = g[_lib.shard_pair_slot(E, D, world, a, b)] + (c["variance"][a] if a == b else 0.0) - M[0, a] * M[0, b]
        ok = np.allclose(M, Mo, rtol=1e-13) and np.allclose(S, So, rtol=1e-11, atol=1e-14) and np.allclose(V, Vo, rtol=1e-13)
        # max-over-ranks timing reduction used by bench.py
        t = torch.tensor([float(rank + 1)], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        ok = ok and t.item() == float(world)
        dist.barrier()
        q.put((rank, bool(ok)))
    finally:
        dist.destroy_process_group()


def test_gloo_world_size_2_exchange():
    import torch.multiprocessing as mp
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = [q.get(timeout=180) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert sorted(results) == [(0, True), (1, True)]


def test_stream_k_closed_forms_match_enumeration():
    """The pair kernel's stream-K split (pair.hip: sk_boundary_of / sk_wave_of / sk_pair_waves) is closed form on both the
    writer (pair kernel) and reader (glue kernel) side; check it against a brute-force enumeration of the wave ranges."""
    import ctypes as C
    from pilco_amd import _lib
    lib = _lib.load_library()
    rs = np.random.RandomState(0)
    for _ in range(60):
        nd, noff = int(rs.randint(0, 7)), int(rs.randint(0, 30))
        if nd + noff == 0:
            continue
        tdiag, toff = int(rs.randint(3, 300)), int(rs.randint(3, 400))
        ud, uo = int(rs.randint(1, 6)), int(rs.randint(1, 6))
        total = nd * tdiag + noff * toff
        waves = int(rs.randint(1, max(2, total // 2)))
        n_pairs = nd + noff
        bnd = [lib.pilco_debug_sk_boundary(w, waves, nd, tdiag, toff, ud, uo, n_pairs) for w in range(waves + 1)]
        assert bnd[0] == 0 and bnd[-1] == total and all(b1 >= b0 for b0, b1 in zip(bnd, bnd[1:]))
        out = (C.c_int * 3)()
        for k in range(n_pairs):
            S0 = k * tdiag if k < nd else nd * tdiag + (k - nd) * toff
            S1 = S0 + (tdiag if k < nd else toff)
            touching = [w for w in range(waves) if bnd[w] < S1 and bnd[w + 1] > S0]   # non-empty ranges meeting the pair
            assert lib.pilco_debug_sk_pair_waves(k, waves, nd, tdiag, toff, ud, uo, n_pairs, out) == 0
            wlo, fslot, whi = out[0], out[1], out[2]
            assert wlo == touching[0] and whi == touching[-1]
            assert fslot == (1 if bnd[wlo] < S0 else 0)   # a wave that starts before the pair holds it in its second slot


@pytest.mark.parametrize("peer", ["ok", "rank1_fails", "first_rollout_fails"])
def test_bench_multi_rank_host_logic_under_torchrun(peer):
    """bench.py --gpus 2 --full exactly as the driver launches it (python -m torch.distributed.run, one process per rank), with
    the device replaced by a stand-in Context (tests/helpers/bench_fake_ranks.py): rendezvous over gloo on 127.0.0.1,
    broadcast of rank 0's RCCL id, barriers, MAX-over-ranks timing, the replica leg, verification against the fixture and
    ONE JSON line from rank 0 with the contract's keys.  The per-step exchange: peer exchange when every rank attaches and
    the first rollout over it succeeds, otherwise every rank detaches and the RCCL path is timed."""
    import json
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "helpers", "bench_fake_ranks.py"),
           "--gpus", "2", "--steps", "3", "--warmup", "1", "--full"]
    env = dict(os.environ, OMP_NUM_THREADS="1", FAKE_PEER=peer)
    pr = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=env, cwd=ROOT)
    assert pr.returncode == 0, pr.stderr[-2000:]
    lines = [l for l in pr.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, pr.stdout[-2000:]
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline"):
        assert k in d, k
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["scaling"] == "strong" and d["vs_baseline"] is None
    assert d["ms_per_step"] >= 4.0                      # the slower rank (2 x 2 ms sleep) sets the time
    assert abs(d["value"] - 1e3 / d["ms_per_step"]) < 1e-9
    assert d["verified"]["max_rel_err"]["S_H"] == 0.0
    assert "replica_rollouts_per_s" in d["secondary"] and "cpu_baseline" not in d
    assert ("peer stores" in d["config"]["exchange"]) == (peer == "ok"), d["config"]["exchange"]
    # one invocation reports BOTH exchanges: the other one timed and verified the same way (or why it could not run) ...
    oe = d["secondary"]["other_exchange"]
    if peer == "ok":
        assert "RCCL" in oe["exchange"] and oe["rollouts_per_s"] > 0 and oe["verified"]["max_rel_err"]["S_H"] == 0.0
    else:
        assert "peer" in oe["exchange"] and "error" in oe
    # ... what RCCL itself says about the communicator, every rank's own phase times, and the Amdahl model from this run's
    # 1-GPU phase times that the measured point is to be read against
    assert d["secondary"]["rccl_comm_count"] == 2 and d["secondary"]["ranks_on_distinct_gpus"] is True
    pr_ = d["secondary"]["per_rank"]
    assert [r["rank"] for r in pr_] == [0, 1] and all(r["pair_us_per_launch"] > 0 and r["other_us_per_step"] is not None for r in pr_)
    am = d["secondary"]["amdahl_model"]
    for k in ("one_gpu_ms_per_rollout", "one_gpu_pair_us_per_launch", "one_gpu_head_us_per_step", "slowest_rank_pair_us_per_launch",
              "predicted_rollouts_per_s_with_a_free_exchange", "measured_rollouts_per_s", "exchange_and_skew_us_per_step", "ideal_linear_rollouts_per_s"):
        assert k in am, k
    assert abs(am["measured_rollouts_per_s"] - d["value"]) < 1e-9


def test_bench_gpus_2_invoked_plainly_starts_its_own_ranks():
    """`python bench.py --gpus 2 ...` typed the way the driver types the 1-GPU line (no launcher, WORLD_SIZE unset): the
    script re-executes itself under torch.distributed.run with one process per rank, its options (--full here) go along, and
    rank 0 prints the ONE JSON line (round-3 review, missing #1: it used to exit with a usage message)."""
    import json
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(OMP_NUM_THREADS="1", FAKE_PEER="ok")
    cmd = [sys.executable, os.path.join(ROOT, "tests", "helpers", "bench_fake_ranks.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
           "--full"]
    pr = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=env, cwd=ROOT)
    assert pr.returncode == 0, pr.stderr[-2000:]
    lines = [l for l in pr.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, pr.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["secondary"]["rccl_comm_count"] == 2
    assert "peer stores" in d["config"]["exchange"] and "RCCL" in d["secondary"]["other_exchange"]["exchange"]


HEADLINE = ["metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "config"]


def _fake_bench(tmp_path, args, ranks=1, peer="ok"):
    """bench.py on the stand-in Context (one process, or `ranks` processes under torch.distributed.run): its ONE JSON line
    and, per rank, the stand-in calls in the order they were made."""
    import json
    import subprocess
    helper = os.path.join(ROOT, "tests", "helpers", "bench_fake_ranks.py")
    if ranks == 1:
        env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
        cmd = [sys.executable, helper, "--gpus", "1"] + args
    else:
        env = dict(os.environ)
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ranks), "--master-addr",
               "127.0.0.1", "--master-port", str(port), helper, "--gpus", str(ranks)] + args
    env.update(OMP_NUM_THREADS="1", FAKE_PEER=peer, FAKE_CALLS=str(tmp_path / "calls"))
    pr = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=env, cwd=ROOT)
    assert pr.returncode == 0, pr.stderr[-2000:]
    lines = [l for l in pr.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, pr.stdout[-2000:]
    calls = [[tuple(c) for c in json.load(open(str(tmp_path / "calls") + ".%d" % r))] for r in range(ranks)]
    return json.loads(lines[0]), calls


def _assert_headline(d, world, steps, warmup, min_ms):
    assert list(d)[:len(HEADLINE)] == HEADLINE
    assert d["metric"] == "moment-matching rollouts/sec (N=1000,D=10,E=10,H=40)" and d["unit"] == "rollouts/s"
    assert d["higher_is_better"] is True and d["dtype"] == "f64" and d["scaling"] == "strong" and d["vs_baseline"] is None
    assert d["n_gpus"] == world and d["steps"] == steps and d["warmup"] == warmup
    assert d["ms_per_step"] >= min_ms and abs(d["value"] - 1e3 / d["ms_per_step"]) < 1e-9
    assert d["config"]["parallelism"] == "pairs%d" % world


def test_bench_plain_run_times_the_steps_and_nothing_else(tmp_path):
    """A plain `bench.py --gpus 1` (no --full): one context, one factorisation, the warm-up and the timed rollouts, the last
    one's outputs written as they were returned, and the result line's own keys only -- no check against the reference, no
    roofline pass, no other configuration, no CPU baseline."""
    d, (calls,) = _fake_bench(tmp_path, ["--steps", "4", "--warmup", "2", "--dump-outputs", str(tmp_path / "out")])
    assert list(d) == HEADLINE
    _assert_headline(d, 1, 4, 2, min_ms=2.0)                 # the stand-in sleeps 2 ms per rollout
    assert d["config"]["exchange"] == "none (one rank)"
    assert calls == [("context", 0), ("factorize", 0, 1)] + [("rollout", 0)] * 6
    G = np.load(os.path.join(ROOT, "tests", "golden", "c2_rollout.npz"))
    for name, want in (("m_H", G["M_traj"][:, -1][None, :]), ("S_H", G["S_traj"][:, :, -1]), ("reward", np.array([[G["R_traj"][-1]]]))):
        got = np.load(str(tmp_path / "out" / (name + ".npy")))
        assert got.dtype == np.float64 and got.shape == want.shape and np.array_equal(got, want), name


def test_bench_full_run_adds_its_keys_after_the_timed_steps(tmp_path):
    """`bench.py --gpus 1 --full` (the other configurations and the CPU baseline left out, they need the device): the same
    headline from the same calls, then the check against the executed reference and the pair kernel's own timing pass."""
    d, (calls,) = _fake_bench(tmp_path, ["--steps", "3", "--warmup", "1", "--full", "--no-secondary", "--no-cpu-baseline",
                                         "--dump-outputs", str(tmp_path / "out")])
    assert list(d) == HEADLINE + ["verified", "roofline"]
    _assert_headline(d, 1, 3, 1, min_ms=2.0)
    assert d["verified"]["max_rel_err"]["S_H"] == 0.0 and d["verified"]["rtol"] == 1e-5
    assert abs(d["roofline"]["avg_launch_ms"] - 0.047) < 1e-12 and d["roofline"]["engine_clock_mhz_under_load"] == 2000.0
    assert calls == [("context", 0), ("factorize", 0, 1)] + [("rollout", 0)] * 4 + [("rollout_timed", 0)]
    assert os.path.exists(str(tmp_path / "out" / "S_H.npy"))


@pytest.mark.parametrize("peer", ["ok", "first_rollout_fails"])
def test_bench_plain_multi_rank_run_prints_the_headline_only(tmp_path, peer):
    """A plain `bench.py --gpus 2`: the exchange is still chosen before anything is timed (peer exchange, or RCCL after its
    first rollout failed), the time is still the slowest rank's, and nothing runs after the timed steps: no second
    exchange, no replica contexts, no timing pass, no verification."""
    d, calls = _fake_bench(tmp_path, ["--steps", "3", "--warmup", "1"], ranks=2, peer=peer)
    assert list(d) == HEADLINE
    _assert_headline(d, 2, 3, 1, min_ms=4.0)                 # the slower rank (2 x 2 ms sleep) sets the time
    assert ("peer stores" in d["config"]["exchange"]) == (peer == "ok"), d["config"]["exchange"]
    for r, c in enumerate(calls):
        # the first rollout over the peer exchange (rank 1's fails: every rank detaches), then warm-up + timed steps
        first = [("rollout", r)] if peer == "ok" else [("rollout", r)] * (r == 0) + [("peer_detach", r)]
        assert c == [("context", r), ("comm_init", r, 2), ("factorize", r, 2)] + first + [("rollout", r)] * 4, c
