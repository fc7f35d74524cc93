"""End values of the executed reference for tests that run a whole script on both sides (the reference's own source on the
shim, the product on the CPU stand-in): where the reference tree exists the script is executed and checked against the
stored copy under tests/golden/; everywhere else the stored copy is what the product is held to.  Refresh a copy with
PILCO_REGEN_GOLDEN=1 where the reference tree exists."""
import os

import numpy as np

from oracle import ref_exec

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden")


def executed_or_stored(name, run, rtol=1e-5):
    """run() -> dict of arrays / floats (the reference's side of the script); name: tests/golden/<name>.npz."""
    path = os.path.join(GOLDEN, name + ".npz")
    if not ref_exec.available():
        with np.load(path) as g:
            return {k: (float(g[k]) if g[k].ndim == 0 else g[k]) for k in g.files}
    out = run()
    if os.environ.get("PILCO_REGEN_GOLDEN") == "1":
        np.savez(path, **{k: np.asarray(v, np.float64) for k, v in out.items()})
    with np.load(path) as g:
        assert sorted(g.files) == sorted(out), (path, sorted(g.files), sorted(out))
        for k in g.files:
            np.testing.assert_allclose(np.asarray(out[k], np.float64), g[k], rtol=rtol, atol=1e-12,
                                       err_msg="%s: %s moved away from the stored executed reference" % (path, k))
    return out
