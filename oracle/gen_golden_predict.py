"""Writes tests/golden/predict_edges.npz: the inputs, the 40-digit truth with units (oracle/mp_predict.py), the declared
zeros and the caps of every case in tests/helpers/predict_cases.py.

    python -m oracle.gen_golden_predict [-j WORKERS] [case names ...]     (named cases are merged into the file)

"_data/<set>/X", "/Y", "/Z": the data sets (Z (E, M, D): every output's inducing inputs; Z[0] is the shared set)
"<case>/xs" (Nt, D) the test points in the order of predict_cases.point_kinds; "<case>/zeros" (E, Nt, 4) the declared zeros
"<case>/t" (exact GP) or "<case>/ts", "<case>/to" (FITC on the shared Z, on every output's own): one vector,
  predict_cases.TRUTH_KEYS: mean, var (E, Nt), dmean, dvar (E, Nt, D) and their units
"_caps", "_caps_keys" ("<class>|<block>"): the caps of the device's K (helpers/predict_edges_reference.compute_caps)
The table's conditions are checked here: every truth value finite, every declared zero exactly zero (the variance: exactly sf2),
the float64 Cholesky of both restatements succeeds, the variance of the exact GP on a training point is below 10 sn2, and (in
predict_cases.make_points) the denormal point has denormal and zero k and the far point only zero k."""
from __future__ import annotations

import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from helpers import predict_cases as pc  # noqa: E402
from oracle import mp_predict  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "predict_edges.npz")
SUBSET = ("x24_ls_ard", "f10_var_tiny")   # recomputed by the CPU suite


def truth_of(args):
    """One output of one truth of a case."""
    c, d, tn, e = args
    t0 = time.time()
    a = (d["X"], d["Y"][:, e])
    b = (d["ls"][e], d["var"][e], d["noise"][e], d["xs"])
    if tn == "t":
        r = mp_predict.gpr(*a, *b)
    else:
        r = mp_predict.fitc(*a, d["Z"][0] if tn == "ts" else d["Z"][e], *b, jitter=pc.JITTER)
    return c["name"], tn, e, r, time.time() - t0


def check(c, d, truths):
    z = d["zeros"]
    on = pc.point_kinds(c).index("on")
    for tn, fx in truths.items():
        for k in pc.TRUTH_KEYS:
            assert np.all(np.isfinite(fx[k])), (c["name"], tn, k, "not finite")
            assert k[0] != "u" or np.all(fx[k] >= pc.TINY), (c["name"], tn, k)
        assert np.all(fx["mean"][z[:, :, 0]] == 0.0) and np.all(fx["dmean"][z[:, :, 2]] == 0.0) and np.all(fx["dvar"][z[:, :, 3]] == 0.0), (c["name"], tn)
        assert np.all((fx["var"] == d["var"][:, None])[z[:, :, 1]]), (c["name"], tn, "the far variance is not sf2")
        if tn == "t":
            assert np.all(fx["var"][:, on] < 10.0 * d["noise"]) and np.all(fx["var"][:, on] > 0.0), (c["name"], fx["var"][:, on], d["noise"])


def main(argv):
    workers = 1
    if argv[:1] == ["-j"]:
        workers, argv = int(argv[1]), argv[2:]
    t0 = time.time()
    have = dict(np.load(PATH)) if (argv and os.path.exists(PATH)) else {}
    for name in pc.DATA:
        if "_data/%s/X" % name not in have:
            for k, v in pc.make_base(name).items():
                have["_data/%s/%s" % (name, k)] = v
    cases = [c for c in pc.CASES if not argv or c["name"] in argv]
    jobs, datas = [], {}
    for c in cases:
        base = {k: have["_data/%s/%s" % (c["data"], k)] for k in (("X", "Y", "Z") if c["M"] else ("X", "Y"))}
        d = pc.make_data(c, base)
        d["xs"] = pc.make_points(c, d)
        d["zeros"] = pc.declared_zeros(c)
        datas[c["name"]] = d
        jobs += [(c, d, tn, e) for tn in pc.truth_names(c) for e in range(c["E"])]
    jobs.sort(key=lambda j: -max(j[0]["N"] if not j[0]["M"] else j[0]["M"], 1) ** 3 - j[0]["N"] * j[0]["M"] ** 2)
    if workers > 1:
        import multiprocessing as mpr
        with mpr.Pool(workers) as pool:
            results = list(_report(pool.imap_unordered(truth_of, jobs)))
    else:
        results = list(_report(map(truth_of, jobs)))
    for c in cases:
        d = datas[c["name"]]
        for k in [k for k in have if k.split("/")[0] == c["name"]]:
            del have[k]
        have[c["name"] + "/xs"] = d["xs"]
        have[c["name"] + "/zeros"] = d["zeros"].astype(np.uint8)
        truths = {}
        for tn in pc.truth_names(c):
            mine = sorted((r for r in results if r[0] == c["name"] and r[1] == tn), key=lambda r: r[2])
            t = {k: np.stack([r[3][k] for r in mine]) for k in pc.TRUTH_KEYS}
            have[c["name"] + "/" + tn] = pc.pack_truth(t)
            truths[tn] = pc.unpack_truth(c, have[c["name"] + "/" + tn])
        check(c, d, truths)
    known = set(pc.case_ids()) | {"_data"}
    have = {k: v for k, v in have.items() if k.split("/")[0] in known and not k.startswith("_caps")}
    np.savez_compressed(PATH, **have)
    from helpers import predict_edges_reference as pr
    pr._FX = None
    pr._CASE.clear()
    pr._KREF.clear()
    caps = sorted(pr.compute_caps().items())     # (a float64 Cholesky that fails in either restatement raises here)
    have["_caps_keys"] = np.array(["%s|%s" % k for k, _ in caps])
    have["_caps"] = np.array([v for _, v in caps])
    np.savez_compressed(PATH, **have)
    print("wrote", PATH, os.path.getsize(PATH), "bytes in %.0f s (sum of the jobs' own times: %.0f s)"
          % (time.time() - t0, sum(r[4] for r in results)))


def _report(results):
    for r in results:
        print("%-18s %-2s output %d %.1f s" % (r[0], r[1], r[2], r[4]), flush=True)
        yield r


if __name__ == "__main__":
    main(sys.argv[1:])
