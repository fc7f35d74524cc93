"""The GP factorisations at every block count, batch and conditioning (cases: helpers/fact_cases.py; truth: oracle/hp_factor.py).

Per case, on a context of its own (gp_factorize, then gp_get_factors):
- well-conditioned cases: iK (whole) and beta against the extended-precision truth, normwise per output, at TOL_WELL; the
  exact GP's objective (gp_nlml: the log-determinant from L's diagonal, k_logdet) at TOL_WELL relative.
- ill-conditioned cases (noise 1e-6, cond 1e8 .. 1e10): the forward errors of beta and of iK P (fixed probes) at most
  RATIO_ILL times those of float64 LAPACK (oracle.tf_path) on the same inputs.
- exact GP, every case: the backward error of beta within C_RES * N * eps.
- bit identity: every output of an E-batch against the same output alone (E = 1 model), the first call (graph capture)
  against the replay after gp_set_hyp to the same values, a fresh context; beta sharded over 2 and 3 contexts
  (group_sync_model) against the single-rank beta.
Each case prints one `FACTREPORT {json}` line with its measured errors (docs/factorisations.md is made of them).
Also: pilco_gp_gram at N1, N2 in {1, 255, 256, 257}, D in {1, 32} against the extended-precision Gram matrix, and the
not-positive-definite path with the failing pivot in block 0, block 1 and the last block, in outputs 0, 16 and 31 of E = 32."""
import json

import numpy as np
import pytest

from helpers import fact_cases as fc

pytestmark = pytest.mark.gpu

TOL_WELL = 1e-10      # normwise, per output, against the truth
RATIO_ILL = 8.0       # forward error against float64 LAPACK's on the same ill-conditioned case
C_RES = 1.0           # backward error of beta <= C_RES * N * eps
EPS = np.finfo(np.float64).eps
_REF = {}


def _ref(case):
    if case["name"] not in _REF:
        from oracle import hp_factor as hp
        d = fc.make_data(case)
        n = case["M"] or case["N"]
        P = fc.probes(n)
        if case["M"]:
            r = hp.fitc(d["X"], d["Y"], d["Z"], d["ls"], d["var"], d["noise"], P)
        else:
            r = hp.exact(d["X"], d["Y"], d["ls"], d["var"], d["noise"], P, full_iK=case["cls"] == "well")
        _REF[case["name"]] = (d, P, r)
    return _REF[case["name"]]


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _factorise(d, outs=None, M=0, cx=None, shard=None):
    """A context holding the case's model (outputs `outs` only, if given) factorised; -> (context, iK or None, beta)."""
    from pilco_amd import _lib
    sel = slice(None) if outs is None else outs
    cx = cx or _lib.Context()
    if shard:
        cx.shard_set(*shard)
    Y, ls, var, noise = d["Y"][:, sel], d["ls"][sel], d["var"][sel], d["noise"][sel]
    cx.gp_set_data(0, d["X"], Y)
    cx.gp_set_hyp(0, ls, var, noise)
    if M:
        cx.gp_set_inducing(0, d["Z"])
    cx.gp_factorize(0)
    if shard:
        return cx, None, None
    iK, beta = cx.gp_get_factors(0, Y.shape[1])
    return cx, iK, beta


@pytest.mark.parametrize("case", fc.CASES, ids=[c["name"] for c in fc.CASES])
def test_factorisation_case(case):
    from oracle import hp_factor as hp
    d, P, r = _ref(case)
    E, N = case["E"], case["N"]
    cx, iK, beta = _factorise(d, M=case["M"])
    try:
        rep = dict(name=case["name"], N=N, M=case["M"], E=E, D=case["D"], cls=case["cls"], nblk=-(-(case["M"] or N) // 64),
                   cond=float(np.max(r["cond"])))
        err_b = [_rel(beta[a], r["beta"][a]) for a in range(E)]
        err_p = [_rel(iK[a] @ P, r["iKP"][a]) for a in range(E)]
        rep.update(err_beta=max(err_b), err_iKP=max(err_p), lapack_beta=float(np.max(r["lapack_beta"])),
                   lapack_iKP=float(np.max(r["lapack_iKP"])))
        rep["ratio"] = max(max(eb / lb, ep / lp) for eb, ep, lb, lp in zip(err_b, err_p, r["lapack_beta"], r["lapack_iKP"]))
        if "iK" in r:
            rep["err_iK"] = max(_rel(iK[a], r["iK"][a]) for a in range(E))
        if not case["M"]:
            nl, _ = cx.gp_nlml(0, case["D"], E, want_grad=False)
            rep["err_nlml"] = float(np.max(np.abs(nl - r["nlml"]) / np.abs(r["nlml"])))
            res = [hp.residual(d["X"], d["Y"][:, a], d["ls"][a], d["var"][a], d["noise"][a], beta[a]) for a in range(E)]
            rep["backward"] = max(res)
            rep["backward_over_N_eps"] = max(res) / (N * EPS)
        # bit identity: replay of the captured chain after set_hyp to the same values; a fresh context; each output alone
        cx.gp_set_hyp(0, d["ls"], d["var"], d["noise"])
        cx.gp_factorize(0)
        iK2, beta2 = cx.gp_get_factors(0, E)
        rep["replay_bits"] = bool(np.array_equal(iK2, iK) and np.array_equal(beta2, beta))
        fresh, iK3, beta3 = _factorise(d, M=case["M"])
        fresh.close()
        rep["fresh_bits"] = bool(np.array_equal(iK3, iK) and np.array_equal(beta3, beta))
        alone = []
        for a in (range(E) if E <= 3 else (0, E // 2, E - 1)):
            one, iK1, beta1 = _factorise(d, outs=slice(a, a + 1), M=case["M"])
            one.close()
            alone.append(bool(np.array_equal(iK1[0], iK[a]) and np.array_equal(beta1[0], beta[a])))
        rep["alone_bits"] = all(alone)
        print("FACTREPORT " + json.dumps(rep))
    finally:
        cx.close()
    assert rep["replay_bits"] and rep["fresh_bits"] and rep["alone_bits"], rep
    if case["cls"] == "well":
        assert rep["err_beta"] < TOL_WELL and rep["err_iKP"] < TOL_WELL, rep
        if "err_iK" in rep:
            assert rep["err_iK"] < TOL_WELL, rep
        if "err_nlml" in rep:
            assert rep["err_nlml"] < TOL_WELL, rep
    else:
        assert rep["ratio"] <= RATIO_ILL, rep
    if "backward" in rep:
        assert rep["backward"] <= C_RES * N * EPS, rep


@pytest.mark.parametrize("name", ["e_n63", "e_n129_e32", "e_n448_ill", "e_n961_d32"])
def test_sharded_beta_is_the_single_rank_beta(name):
    """beta of every output after group_sync_model, on every rank of 2 and 3 contexts, bit for bit the single-rank beta (a
    third rank of a two-output model owns no output)."""
    from pilco_amd import _lib
    case = fc.BY_NAME[name]
    d = fc.make_data(case)
    one, _, beta = _factorise(d)
    one.close()
    for W in (2, 3):
        ctxs = []
        try:
            for rk in range(W):
                cx, _, _ = _factorise(d, shard=(rk, W))
                ctxs.append(cx)
            _lib.group_sync_model(ctxs)
            for rk, cx in enumerate(ctxs):
                _, b = cx.gp_get_factors(0, case["E"], want_iK=False)
                assert np.array_equal(b, beta), (name, W, rk, _rel(b, beta))
        finally:
            for cx in ctxs:
                cx.close()


@pytest.mark.parametrize("D", [1, 32])
def test_gram_against_extended_precision(D):
    from oracle import hp_factor as hp
    from pilco_amd import _lib
    rs = np.random.RandomState(D)
    E = 2
    ls = np.sqrt(D) * (0.7 + 0.6 * rs.rand(E, D))
    var = 0.5 + rs.rand(E)
    X = {n: 1.5 * np.sqrt(D) * rs.randn(n, D) / np.sqrt(D) ** 0.5 for n in (1, 255, 256, 257)}
    cx = _lib.Context()
    try:
        cx.gp_set_data(0, X[257], rs.randn(257, E))
        cx.gp_set_hyp(0, ls, var, 1e-2 * np.ones(E))
        worst = 0.0
        for n1 in X:
            for n2 in X:
                K = cx.gp_gram(0, X[n1], X[n2] if n2 != n1 else None, E)
                assert K.shape == (E, n1, n2)
                for a in range(E):
                    Kt = hp.gram(X[n1], X[n2], ls[a], var[a]).astype(np.float64)
                    err = _rel(K[a], Kt)
                    worst = max(worst, err)
                    assert err < 1e-14, (D, n1, n2, a, err)
        print("FACTREPORT " + json.dumps(dict(name=f"gram_d{D}", err_gram=worst)))
    finally:
        cx.close()


def _not_pd_data(N, copies):
    """N points in D = 2 whose Gram matrix is well-conditioned without noise (a line, three lengthscales apart), with three
    copies of one far-away point at the columns `copies`.  The far point's Gram entries against the others are exactly zero,
    so in an output of variance 1 its copies' pivots are 1, then exactly 0 at the second copy."""
    rs = np.random.RandomState(N)
    X = np.stack([3.0 * np.arange(N), 0.1 * rs.randn(N)], axis=1)
    X[list(copies)] = [-1e4, 0.0]
    return X


@pytest.mark.parametrize("copies,out", [((5, 40, 100), 0), ((10, 70, 150), 16), ((60, 195, 198), 31)],
                         ids=["block0_out0", "block1_out16", "lastblock_out31"])
def test_not_positive_definite_pivot_is_reported(copies, out):
    from pilco_amd import _lib
    N, E = 200, 32
    X = _not_pd_data(N, copies)
    rs = np.random.RandomState(7)
    Y = rs.randn(N, E)
    ls = 1.0 + 0.2 * rs.rand(E, 2)
    var = 0.5 + rs.rand(E)
    noise = 1e-2 * np.ones(E)
    var[out], noise[out] = 1.0, 0.0
    cx = _lib.Context()
    try:
        cx.gp_set_data(0, X, Y)
        cx.gp_set_hyp(0, ls, var, noise)
        with pytest.raises(_lib.NotPositiveDefiniteError) as ei:
            cx.gp_factorize(0)
        msg = str(ei.value)
        print("FACTREPORT " + json.dumps(dict(name=f"not_pd_{out}", copies=copies, output=ei.value.output, msg=msg)))
        assert ei.value.output == out, msg
        assert f"output {out} " in msg, msg
        pivot = int(msg.split("(pivot ")[1].split(")")[0])     # 1-based column of the first non-positive pivot
        assert copies[1] <= pivot - 1 <= copies[2], msg
        with pytest.raises(_lib.PilcoError) as e2:              # no usable factor afterwards
            cx.gp_get_factors(0, E)
        assert not isinstance(e2.value, _lib.NotPositiveDefiniteError)
        with pytest.raises(_lib.PilcoError) as e3:
            cx.gp_predict(0, np.zeros(2), 0.1 * np.eye(2), 2, E)
        assert not isinstance(e3.value, _lib.NotPositiveDefiniteError) and "factoris" in str(e3.value)
        noise[out] = 1e-2                                       # and a good factorisation after it is used as usual
        cx.gp_set_hyp(0, ls, var, noise)
        cx.gp_factorize(0)
        iK, beta = cx.gp_get_factors(0, E)
        assert np.all(np.isfinite(iK)) and np.all(np.isfinite(beta))
    finally:
        cx.close()
