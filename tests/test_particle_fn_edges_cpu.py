"""The yardstick of the function-sample edge table on the CPU (helpers/particle_fn_edge_cases.py, particle_fn_edge_truth.py,
particle_fn_edge_reference.py; docs/particle_fn_edges.md): the conditions on the stored inputs, the coverage guard and its
deletion test, the caps recomputed from both float64 restatements against the 40-digit truth, restatement (b) inside every
cap, and every mutant of (b) more than 100 caps out.  Figures are printed before they are asserted (pytest -s)."""
import numpy as np
import pytest

from helpers import particle_fn_edge_cases as ec
from helpers import particle_fn_edge_reference as er


@pytest.fixture(scope="module")
def krefs():
    return {c["name"]: er.k_ref(c) for c in ec.CASES}


@pytest.mark.parametrize("c", ec.CASES, ids=ec.case_ids())
def test_the_conditions_on_the_stored_inputs_hold(c):
    assert er.conditions(c) == [], c["name"]       # (a float64 Cholesky that fails raises inside)


def test_no_case_is_skipped_and_the_fixture_holds_inputs_and_caps_only():
    fx = ec.fixture()
    heads = {k.split("/")[0] for k in fx}
    assert heads <= {"_data", "_draws", "_bigL", "_caps", "_caps_keys"} | {c["name"] for c in ec.CASES if c["kind"] == "table"}
    assert {k.split("/")[-1] for k in fx if not k.startswith("_")} <= {"x0", "eps"}
    assert all("%s|%s" % (c["cls"], b) in set(fx["_caps_keys"]) for c in ec.CASES for b in c["blocks"])
    assert "noise_m10" not in {c["fam"] for c in ec.CASES}
    assert len(ec.case_ids()) == len(set(ec.case_ids()))


def test_the_stored_draws_are_the_stream_restatement():
    c = ec.by_name("x24_std")
    fx = ec.fixture()
    n = ec.normals(c["E"], c["D"], c["L"], c["P"], c["N"])
    for k, v in n.items():
        assert np.allclose(fx["%s/%s" % (ec.draw_key(c), k)], v, rtol=1e-13, atol=1e-15), k


def test_coverage_guard_and_its_deletions():
    assert ec.missing(ec.CASES) == []
    without = lambda pred: [c for c in ec.CASES if not pred(c)]
    assert "fam:ls_ard on matrix" in ec.missing(without(lambda c: c["fam"] == "ls_ard" and "matrix" in c["blocks"]))
    assert "fam:y0 on setup" in ec.missing(without(lambda c: c["fam"] == "y0"))
    assert any(m.startswith("pt:far40") for m in ec.missing(without(lambda c: c["kind"] == "table")))
    for D in ec.WIDTHS:
        assert ec.missing(without(lambda c: c["name"] == "w%d" % D)) == ["D:%d on value" % D]
    for L in ec.BIG_L:
        assert ec.missing(without(lambda c: c["L"] == L)) == ["L:%d on value" % L]
    assert set(ec.missing(without(lambda c: c["P"] == 65))) == {"P:65 on %s" % b for b in ec.BLOCKS}
    assert "L:1 on value" in ec.missing(without(lambda c: c["L"] == 1))
    for f in ec.ILL:
        assert "fam:%s at N:65 on matrix" % f in ec.missing(without(lambda c: c["name"] == "x65_" + f))
    for f in ("noise_floor", "noise_dom"):
        assert ec.missing(without(lambda c: c["obs"] and c["fam"] == f)) == ["obs:%s on value" % f]
    assert ec.missing(without(lambda c: c["name"] == "x24_ls_ard_lin0")) == ["policy:lin0:ls_ard on value"]
    assert ec.missing(without(lambda c: c["name"] == "x24_std_linW")) == ["policy:linW:std on value"]


def test_caps_recomputed_within_a_factor_of_two_and_b_inside_every_cap(krefs):
    caps = {}
    for c in ec.CASES:
        k = krefs[c["name"]]
        for b in c["blocks"]:
            print("FIGURE K_ref %-20s %-6s (a) %9.3g (b) %9.3g | cap of %-22s %9.3g" % (c["name"], b, k["a"][b], k["b"][b], c["cls"], er.cap_of(c, b)))
            assert np.isfinite(k["a"][b]) and np.isfinite(k["b"][b])
            assert k["b"][b] <= er.cap_of(c, b) and k["a"][b] <= er.cap_of(c, b), (c["name"], b)
            caps[(c["cls"], b)] = max(caps.get((c["cls"], b), 4.0), 8.0 * max(k["a"][b], k["b"][b]))
    for (cls, b), v in caps.items():
        stored = er.cap_of(dict(cls=cls), b)
        assert 0.5 * stored <= v <= 2.0 * stored, (cls, b, v, stored)


def test_declared_exact_results_are_exact_in_restatement_b():
    for name in ("x24_std", "x24_ls_ard", "x24_var_huge", "x24_y0"):
        c = ec.by_name(name)
        d, r = ec.case(c), er.reference(c)
        far, zero_out = ec.declared(c)
        xn, G = er.step_b(d["model"], d["draws"], r["v"], r["xt"])
        v0 = np.zeros_like(r["v"])                        # the feature half alone: the same operations on the same inputs
        xf, Gf = er.step_b(d["model"], d["draws"], v0, r["xt"])
        assert np.array_equal(xn[far], xf[far]) and np.array_equal(G[far], Gf[far]), name
        if zero_out:
            assert np.array_equal(xn[:, 0], d["x0"][:, 0]) and np.all(G[:, 0, :] == 2.0 * np.eye(3)[0]), name
            assert not er.setup_b(d["model"], d["draws"], r["iK"])[:, 0, :].any()


MUTANT_CASES = ("x24_std", "x24_ls_ard", "x65_dup", "x24_std_w0", "x24_std_L1")


def test_a_mutated_restatement_exceeds_the_cap_by_100():
    for mut in er.MUTANTS:
        best = (0.0, None, None)
        for name in MUTANT_CASES:
            c = ec.by_name(name)
            for b, k in er.mutant_ks(c, mut).items():
                if np.isfinite(k) and k / er.cap_of(c, b) > best[0]:
                    best = (k / er.cap_of(c, b), name, b)
        print("FIGURE mutant %-13s K / cap = %9.3g on %s, %s" % (mut, *best))
        assert best[0] > 100.0, (mut, best)
    # the second tile's only point (N = 65) left out is caught as well
    c = ec.by_name("x65_dup")
    k = er.mutant_ks(c, "drop_point")
    assert all(np.isfinite(v) and v > 100.0 * er.cap_of(c, b) for b, v in k.items()), k
