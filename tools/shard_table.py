"""The tables of docs/sharding.md from the JSON that tests/test_gpu_sharding.py writes with $SHARD_REPORT set:
    SHARD_REPORT=report.json python -m pytest tests/test_gpu_sharding.py -m gpu -s && python tools/shard_table.py report.json"""
import json
import sys

TOL = dict(fwd="1e-9", routes="1e-10", grad="1e-7")


def _e(v):
    return "-" if v is None else "%.1e" % v


def main(path):
    R = json.load(open(path))
    print("| case | model | E / U | npad | W | ranks by class | stream-K waves per rank (variant 0) | fwd err (tol %(fwd)s) | "
          "variant 0 vs single rank (tol %(routes)s) | grad err (tol %(grad)s) | bitwise comparisons |" % TOL)
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for tag in sorted(k for k in R if " W=" in k):
        r = R[tag]
        name, W = tag.split(" W=")
        kinds = r["ranks"]
        by = ", ".join("%d %s" % (kinds.count(k), k) for k in ("both", "diag", "offdiag", "none") if k in kinds)
        model = r["model"] if r["model"] != "exact" else "N=%d" % r["N"]
        if r["model"].startswith("FITC"):
            model += ", N=%d" % r["N"]
        print("| %s | %s | %d / %d | %d | %s | %s | %s | %s | %s | %s | %d |" % (
            name, model, r["E"], r["U"], r["npad"], W, by, " ".join(str(w) for w in r.get("waves", [])), _e(r.get("fwd")), _e(r.get("routes")),
            _e(r.get("grad")), r.get("bitwise", 0)))
    print()
    print("| once per file | worst fwd err | worst grad err | bitwise comparisons |")
    print("|---|---|---|---|")
    for tag in sorted(k for k in R if " W=" not in k and isinstance(R[k], dict)):
        r = R[tag]
        print("| %s | %s | %s | %d |" % (tag, _e(r.get("fwd")), _e(r.get("grad")), r.get("bitwise", 0)))
    print()
    print("run time of the file: %s s" % R.get("seconds"))


if __name__ == "__main__":
    main(sys.argv[1])
