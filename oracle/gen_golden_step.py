"""Writes tests/golden/step_edges.npz: the factors and the 40-digit truth with units (oracle/mp_step.py) of every case in
tests/helpers/step_cases.py.

    python -m oracle.gen_golden_step [-j WORKERS] [case names ...]     (named cases are merged into the file)

"_model/<model>" (shared by the model's cases; one vector, helpers/step_cases.factors_from): beta (E, N), then the inverse the
device is given:
  N <= 32  iK (E, N (N + 1) / 2): the upper triangle of the 40-digit (K + noise I)^-1 (oracle/mp_truth.factorize), rounded
  larger   d, g (E, N): iK_a = diag(d_a) - outer(g_a, g_a), d_a the diagonal of that inverse and g_a the dominant rank-one part
           of the rest -- the shape a real inverse has in both limits; numpy reproduces iK_a from d and g to the bit on any
           IEEE machine (a 257-point inverse takes minutes per output: they run in the worker pool)
"<case>/t" (one vector, helpers/step_cases.TRUTH_KEYS): M (1, E), S (E, E), V (D, E), their units uM, uS, uV, xr (E, 2) the range
  of the mean sums' exponents, ldetB (E), ldetR (E, E) log10 of the determinants; "<case>/beta" (E, N) where the case has its
  own; "<case>/g" = [gm (D) | gs (D, D)] for a gradient case
"<case>/wg" = [reward | dW (U, E) | db (U)] of a policy-gradient case (step_cases.WGRAD_CASES)
"_caps", "_caps_keys" ("<class>|<block>"): the caps of the device's K (helpers/step_reference.compute_caps)
The table's conditions are checked here: every truth value finite, det B and det R positive, a straddling case has exponents
on both sides of the clamp and a case below it has none above.
"""
from __future__ import annotations

import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from helpers import step_cases as sc  # noqa: E402
from oracle import mp_step, mp_truth  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "step_edges.npz")
SUBSET = ("cov_zero", "ls_ard_mixed", "e1_p3")   # recomputed by the CPU suite


def output_factors(args):
    """(model, output, 40-digit (K + noise I)^-1 rounded (N, N), beta (N)) of one output of a model (oracle/mp_truth.factorize)."""
    name, a = args
    d = sc.make_model(name)
    N = d["X"].shape[0]
    iKs, betas = mp_truth.factorize(d["X"], d["Y"][:, a:a + 1], d["ls"][a:a + 1], d["var"][a:a + 1], d["noise"][a:a + 1], mp_step.DPS)
    return name, a, np.array([[float(iKs[0][i, j]) for j in range(N)] for i in range(N)]), np.array([float(betas[0][i]) for i in range(N)])


def pack_factors(iK, beta):
    """The fixture's vector of a model from its rounded 40-digit inverse (E, N, N) and beta (E, N)."""
    E, N = beta.shape
    if N <= 32:
        iu = np.triu_indices(N)
        return np.concatenate([beta.ravel(), np.array([iK[a][iu] for a in range(E)]).ravel()])
    dd, g = np.empty((E, N)), np.zeros((E, N))
    for a in range(E):
        dd[a] = np.diag(iK[a])
        w, Q = np.linalg.eigh(-0.5 * ((iK[a] - np.diag(dd[a])) + (iK[a] - np.diag(dd[a])).T))
        if w[-1] > 0:
            g[a] = np.sqrt(w[-1]) * Q[:, -1]
    return np.concatenate([beta.ravel(), dd.ravel(), g.ravel()])


def cancelling_beta(c, d, beta):
    """Alternating signs over the mean sums' own factors: M cancels to 1e-10 of its absolute sum."""
    E, N = beta.shape
    out = np.empty_like(beta)
    zeta = d["X"] - d["m"]
    for a in range(E):
        iL = np.diag(1.0 / d["ls"][a])
        iN = zeta @ iL
        B = iL @ d["s"] @ iL + np.eye(c["D"])
        l = np.exp(-0.5 * np.sum(iN * np.linalg.solve(B.T, iN.T).T, 1))
        out[a] = np.where(np.arange(N) % 2 == 0, 1.0, -1.0) / l * np.abs(beta[a]).mean()
        out[a, 0] *= 1.0 + N * 1e-10
    return out


def wgrad_truth(c, have):
    """[R | dW | db] of the H = 3 rollout with the case's non-zero controller and ExponentialReward(W = I, t = 0): 50-digit central
    differences of the whole rollout (oracle/mp_link.gradient) on the factors the device gets."""
    import mpmath as mp
    from oracle import mp_link as ml
    d = sc.make_data(c)
    iK, beta, iKt = sc.factors_from(c, lambda k: have[k])
    E, N = beta.shape
    mp.mp.dps = ml.DPS
    fact = ([ml.mat(iKt[a], N, N) for a in range(E)], [ml.vec(beta[a]) for a in range(E)])
    gp = dict(X=d["X"], ls=d["ls"], var=d["var"])
    pd = dict(W=d["W"], b=d["b"], maxact=np.ones(c["U"]))
    terms = [dict(kind="exp", coef=1.0, W=np.eye(E), t=np.zeros(E))]
    R = float(ml.cascade(gp, ml.make_policy("linear", pd), ml.mp_terms(terms, E), d["m0"], d["S0"], sc.WGRAD_H, fact)[1][sc.WGRAD_H])
    dW, db = ml.gradient(gp, "linear", pd, terms, d["m0"], d["S0"], sc.WGRAD_H, ("W", "b"), fact=fact)
    out = np.concatenate([[R], dW.ravel(), db.ravel()])
    assert np.all(np.isfinite(out)) and np.abs(dW).max() > 0, c["name"]
    return out


def truth_of(args):
    c, have = args
    if c in sc.WGRAD_CASES:
        t0 = time.time()
        return c["name"], {"wg": wgrad_truth(c, have)}, time.time() - t0
    t0 = time.time()
    d = sc.make_data(c)
    out = {}
    get = lambda k: have[k]
    if c["beta"] == "cancel":
        base = dict(c, beta="stored")
        out["beta"] = cancelling_beta(c, d, sc.factors_from(base, get)[1])
        get = lambda k: out["beta"] if k == c["name"] + "/beta" else have[k]
    iK, beta, iKt = sc.factors_from(c, get)
    r = mp_step.step(d["X"], d["ls"], d["var"], d["m"], d["s"], iK, beta)
    out["t"] = sc.pack_truth(c, r)
    for k, v in out.items():
        assert np.all(np.isfinite(v)), (c["name"], k, "not finite")
    if c["mean"] == "straddle":
        assert np.any((r["xr"][:, 0] < sc.CLAMP) & (r["xr"][:, 1] > sc.CLAMP)), (c["name"], r["xr"], "does not straddle the clamp")
    if c["mean"] == "below":
        assert np.all(r["xr"][:, 1] < sc.CLAMP), (c["name"], r["xr"])
    if c["beta"] in ("zero", "zero0"):   # a block the case makes exactly zero is zero in the truth
        assert r["M"][0, 0] == 0.0 and np.all(r["V"][:, 0] == 0.0) and (c["beta"] == "zero0" or (np.all(r["M"] == 0.0) and np.all(r["V"] == 0.0))), c["name"]
    if c["beta"] == "cancel":
        assert np.all(np.abs(r["M"]) < 1e-8 * r["uM"] / sc.EPS), (c["name"], "M does not cancel")
    if c["grad"]:
        assert c["N"] <= 24 and c["D"] <= 4, c["name"]
        gm, gs = mp_step.gradient(d["X"], d["ls"], d["var"], d["m"], d["s"], iK, beta, d["Mbar"], d["Sbar"], d["Vbar"])
        out["g"] = np.concatenate([gm.ravel(), gs.ravel()])
        assert np.all(np.isfinite(out["g"])), c["name"]
    return c["name"], out, time.time() - t0


def main(argv):
    workers = 1
    if argv[:1] == ["-j"]:
        workers, argv = int(argv[1]), argv[2:]
    t0 = time.time()
    have = dict(np.load(PATH)) if (argv and os.path.exists(PATH)) else {}
    cases = [c for c in sc.CASES + sc.WGRAD_CASES if not argv or c["name"] in argv]
    need = [name for name in sorted({c["model"] for c in cases}) if "_model/" + name not in have]
    fjobs = [(name, a) for name in need for a in range(sc.MODELS[name][1])]
    fjobs.sort(key=lambda j: -sc.MODELS[j[0]][0])
    if workers > 1 and fjobs:
        import multiprocessing as mpr
        with mpr.Pool(workers) as pool:
            parts = list(pool.imap_unordered(output_factors, fjobs))
    else:
        parts = [output_factors(j) for j in fjobs]
    for name in need:
        mine = sorted((p for p in parts if p[0] == name), key=lambda p: p[1])
        have["_model/" + name] = pack_factors(np.stack([p[2] for p in mine]), np.stack([p[3] for p in mine]))
        print("model", name, flush=True)
    models = {k: v for k, v in have.items() if k.startswith("_model/")}
    jobs = [(c, {"_model/" + c["model"]: models["_model/" + c["model"]]}) for c in cases]
    jobs.sort(key=lambda j: -j[0]["N"] ** 2 * j[0]["E"] ** 2 * (30 if j[0]["grad"] else 1))
    if workers > 1:
        import multiprocessing as mpr
        with mpr.Pool(workers) as pool:
            results = pool.imap_unordered(truth_of, jobs)
            results = list(_report(results))
    else:
        results = list(_report(map(truth_of, jobs)))
    for name, out, _ in results:
        for k in [k for k in have if k.split("/")[0] == name]:
            del have[k]
        for k, v in out.items():
            have[name + "/" + k] = v
    known = set(sc.case_ids()) | set(sc.case_ids(sc.WGRAD_CASES)) | {"_model"}
    have = {k: v for k, v in have.items() if k.split("/")[0] in known and (k.split("/")[0] != "_model" or k.split("/")[1] in sc.MODELS)}
    have = {k: v for k, v in have.items() if not k.startswith("_caps")}
    np.savez_compressed(PATH, **have)
    from helpers import step_reference as sr
    sr._FX = None
    sr._CASE.clear()
    caps = sorted(sr.compute_caps().items())
    have["_caps_keys"] = np.array(["%s|%s" % k for k, _ in caps])
    have["_caps"] = np.array([v for _, v in caps])
    np.savez_compressed(PATH, **have)
    print("wrote", PATH, os.path.getsize(PATH), "bytes in %.0f s (sum of the cases' own times: %.0f s)"
          % (time.time() - t0, sum(r[2] for r in results)))


def _report(results):
    for r in results:
        print("%-16s %.1f s" % (r[0], r[2]), flush=True)
        yield r


if __name__ == "__main__":
    main(sys.argv[1:])
