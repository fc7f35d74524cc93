"""Writes tests/golden/particle_fn_edges.npz: the inputs, the draws and the caps of the function-sample edge table
(tests/helpers/particle_fn_edge_cases.py; docs/particle_fn_edges.md).  No truth is stored: the device's V depends on the
device's own iK, so the 40-digit truth is evaluated where the test runs (tests/helpers/particle_fn_edge_truth.py).

    python -m oracle.gen_golden_particle_fn_edges

"_data/<set>/X", "/Y"   the data sets x24 and x65 of helpers/predict_cases.make_base
"_draws/<shape>/z", "/phase", "/w", "/xi"   the normals and phases of the stream restatement (seed SEED), one set per shape
"<case>/x0" (P, E) the initial particles, "<case>/eps" (1, P, E) the step draws of an observation-noise case, "_bigL/x0"
"_caps", "_caps_keys" ("<class>|<block>")   the caps of the device's K (helpers/particle_fn_edge_reference.compute_caps)
The archive is written with fixed member times and in sorted order: a second run gives the same bytes.  The conditions on the
inputs (helpers/particle_fn_edge_reference.conditions) are asserted for every case."""
from __future__ import annotations

import io
import os
import sys
import time
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from helpers import particle_fn_edge_cases as ec  # noqa: E402
from helpers import predict_cases as pc  # noqa: E402


def save(path, arrays):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def inputs():
    fx = {}
    for name in ("x24", "x65"):
        for k, v in pc.make_base(name).items():
            fx["_data/%s/%s" % (name, k)] = v
    for c in ec.CASES:
        if c["kind"] != "table":
            continue
        base = {k: fx["_data/%s/%s" % (c["data"], k)] for k in ("X", "Y")}
        _, d = ec.table_model(c, base)
        fx[c["name"] + "/x0"] = ec.make_x0(c, d)
        if c["obs"]:
            fx[c["name"] + "/eps"] = np.random.RandomState(pc._seed("eps" + c["name"])).randn(1, c["P"], c["E"])
        if ec.draw_key(c) + "/z" not in fx:
            for k, v in ec.normals(c["E"], c["D"], c["L"], c["P"], c["N"]).items():
                fx["%s/%s" % (ec.draw_key(c), k)] = v
    std65 = pc._c("x65_std", "x65", "std")
    d = pc.make_data(std65, {k: fx["_data/x65/" + k] for k in ("X", "Y")})
    fx["_bigL/x0"] = pc.make_points(std65, d)[pc.POINT_KINDS.index("half")][None, :]
    return fx


def main():
    t0 = time.time()
    fx = inputs()
    save(ec.PATH, fx)
    from helpers import particle_fn_edge_reference as er
    ec._FX = None
    ec._CASE.clear()
    er._REF.clear()
    for c in ec.CASES:
        bad = er.conditions(c)
        assert not bad, (c["name"], bad)
    assert not ec.missing(ec.CASES), ec.missing(ec.CASES)
    caps = sorted(er.compute_caps().items())
    fx["_caps_keys"] = np.array(["%s|%s" % k for k, _ in caps])
    fx["_caps"] = np.array([v for _, v in caps])
    save(ec.PATH, fx)
    ec._FX = None
    print("wrote", ec.PATH, os.path.getsize(ec.PATH), "bytes in %.0f s" % (time.time() - t0))


if __name__ == "__main__":
    main()
