"""Writes tests/golden/predict_cov.npz: the inputs, the 40-digit truth of the full posterior covariance with its units
(tests/helpers/predict_cov_truth.py on the primitives of oracle/mp_predict.py) and the cap of every case in
tests/helpers/predict_cov_cases.py.

    python tools/gen_golden_predict_cov.py [-j WORKERS]

"<case>/X", "/Y", "/Z" ((E, M, D): every output's inducing inputs; Z[0] is the shared set), "/ls", "/var", "/noise", "/xs"
"<case>/cov"   (E, Nt (Nt + 1) / 2) float64: the lower triangle of the truth, row by row (predict_cov_cases.tril_pack)
"<case>/lunit" the same entries' units as float32 log2, rounded down (predict_cov_cases.pack_unit)
"_caps", "_caps_keys": per case 8 x the larger K of the two float64 restatements against the truth, at least 4
"_provenance": how the file was made"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from helpers import predict_cov_cases as cc  # noqa: E402


def truth_of(args):
    from helpers import predict_cov_truth as ct
    c, d, e = args
    t0 = time.time()
    ls, sf2, sn2 = d["ls"][e], d["var"][e], d["noise"][e]
    if c["M"]:
        cov, unit = ct.fitc_cov(d["X"], cc.points_of(c, d, e), ls, sf2, sn2, d["xs"], jitter=cc.JITTER)
    else:
        cov, unit = ct.gpr_cov(d["X"], ls, sf2, sn2, d["xs"])
    return c["name"], e, cov, unit, time.time() - t0


def main(argv):
    workers = int(argv[1]) if argv[:1] == ["-j"] else 1
    assert not cc.missing(), cc.missing()
    t0 = time.time()
    datas, jobs = {}, []
    for c in cc.CASES:
        d = cc.make_data(c)
        d["xs"] = cc.make_points(c, d)
        datas[c["name"]] = d
        jobs += [(c, d, e) for e in range(c["E"])]
    jobs.sort(key=lambda j: -(j[0]["n"] ** 3 + j[0]["N"] * j[0]["M"] ** 2 + j[0]["n"] * j[0]["Nt"] ** 2))
    if workers > 1:
        import multiprocessing as mpr
        with mpr.Pool(workers) as pool:
            results = list(_report(pool.imap_unordered(truth_of, jobs, chunksize=1)))
    else:
        results = list(_report(map(truth_of, jobs)))
    have = {}
    for c in cc.CASES:
        d = datas[c["name"]]
        mine = sorted((r for r in results if r[0] == c["name"]), key=lambda r: r[1])
        cov, unit = np.stack([r[2] for r in mine]), np.stack([r[3] for r in mine])
        assert np.all(np.isfinite(cov)) and np.all(unit >= cc.TINY), c["name"]
        assert np.array_equal(cov, cov.transpose(0, 2, 1)) and np.array_equal(unit, unit.transpose(0, 2, 1)), c["name"]
        for k in ("X", "Y", "ls", "var", "noise", "xs"):
            have[c["name"] + "/" + k] = d[k]
        if c["M"]:
            have[c["name"] + "/Z"] = d["Z"]
        have[c["name"] + "/cov"] = cc.tril_pack(cov)
        have[c["name"] + "/lunit"] = cc.pack_unit(cc.tril_pack(unit))
    have["_provenance"] = np.array("tools/gen_golden_predict_cov.py; mpmath %s at %d digits; numpy %s" % (
        __import__("mpmath").__version__, __import__("oracle.mp_predict", fromlist=["DPS"]).DPS, np.__version__))
    np.savez_compressed(cc.PATH, **have)
    from helpers import predict_cov_restatement as cr
    cc._FX = None
    caps = []
    for c in cc.CASES:
        fx = dict(np.load(cc.PATH))
        cc._FX = fx
        d = {k: fx[c["name"] + "/" + k] for k in ("X", "Y", "ls", "var", "noise", "xs")}
        d["Z"] = fx[c["name"] + "/Z"] if c["M"] else None
        d["cov"] = cc.tril_unpack(fx[c["name"] + "/cov"], c["Nt"])
        d["unit"] = np.maximum(np.exp2(cc.tril_unpack(fx[c["name"] + "/lunit"], c["Nt"]).astype(np.float64)), cc.TINY)
        ka, kb = cr.k_of(cr.restate_a(c, d), d), cr.k_of(cr.restate_b(c, d), d)
        print("%-24s K_ref (a) %.3g (b) %.3g" % (c["name"], ka, kb), flush=True)
        caps.append(cr.cap_from(max(ka, kb)))
    have["_caps_keys"] = np.array(cc.case_ids())
    have["_caps"] = np.array(caps)
    np.savez_compressed(cc.PATH, **have)
    cc._FX = None
    print("wrote", cc.PATH, os.path.getsize(cc.PATH), "bytes in %.0f s" % (time.time() - t0))


def _report(results):
    for r in results:
        print("%-24s output %d %.1f s" % (r[0], r[1], r[4]), flush=True)
        yield r


if __name__ == "__main__":
    main(sys.argv[1:])
