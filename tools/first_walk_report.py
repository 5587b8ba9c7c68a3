#!/usr/bin/env python3
"""The raw walk over the LU factors, case by case (tests/first_walk_cases.py), one MI355X.

Every case of the shared table is factored and solved once with SPL_LU_IRSTEP=0 under its own switches.  Recorded per
case: the path before and after the solve, the walks, the chain span and bytes, the exact componentwise backward error
of the worst column (tests/helpers.py, exact_backward_error), the same figure of the reference's raw solution
(scipy.sparse.linalg.splu, no refinement), their worst ratio over the columns (the reference floored at 2^-53), the
backward error the product reports and its relative distance from the exact one.  Per family (band, tree, chain,
complex): the worst ratio, and R = the smallest power of two that is at least twice it — the constant
tests/test_gpu_first_walk.py reads from this file.  Nothing is asserted here: it is recorded.

python tools/first_walk_report.py [--only ID ...] [--out profiles/first_walk_omega.json]"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "first_walk_omega.json"))
    args = ap.parse_args()
    import first_walk_cases as F
    import __graft_entry__ as g
    import torch
    pkg = g.load_package()
    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    pkg._ffi.require_gpu()
    cases = [c for c in F.CASES if args.only is None or c.id in args.only]
    rows = []
    for c in cases:
        for name in F.SWITCHES:
            os.environ.pop(name, None)
        os.environ.update(c.env)
        os.environ["SPL_LU_IRSTEP"] = "0"
        t0 = time.time()
        fact, A, seen = F.run_case(pkg, c)
        seconds = time.time() - t0
        rep, st = seen["report"], seen["stats"]
        ref = F.reference_omega(c)
        worst = max(seen["omega"])
        row = {"id": c.id, "family": c.family, "matrix": "%s(%d)" % c.matrix, "n": st["n"], "k": c.k,
               "system": "A" if c.mode == F.NORMAL else "A^T", "env": c.env,
               "path": seen["path"], "path_after": seen["path_after"], "walks": rep["walks"],
               "ir_attempted": rep["ir_attempted"], "chain_span": rep["chain_span"], "chain_bytes": rep["chain_bytes"],
               "fronts": st["fronts"], "complex_fronts": st["complex_fronts"], "block_pivoting": st["block_pivoting"],
               "omega": worst, "omega_ref": max(ref), "ratio": F.ratio(c, seen["omega"]),
               "reported": rep["backward_error"],
               "reported_rel_diff": abs(rep["backward_error"] - worst) / worst if worst > 0 else rep["backward_error"],
               "seconds": round(seconds, 2)}
        rows.append(row)
        print("%-38s path %d->%d walks %d chain %4d fronts %5d  omega %.2e ref %.2e ratio %6.2f  reported %.2e (rel %.1e)  "
              "%.1f s" % (c.id, row["path"], row["path_after"], row["walks"], row["chain_span"], row["fronts"], worst,
                          row["omega_ref"], row["ratio"], row["reported"], row["reported_rel_diff"], seconds), flush=True)
        del fact, A
    worst_ratio = {f: max([r["ratio"] for r in rows if r["family"] == f] or [0.0]) for f in F.FAMILIES}
    R = {f: (2.0 ** math.ceil(math.log2(2.0 * w)) if w > 0 else 1.0) for f, w in worst_ratio.items()}
    out = {"what": "raw walk over the LU factors (SPL_LU_IRSTEP=0) against scipy splu without refinement: exact componentwise "
                   "backward errors, worst column; R = smallest power of two >= 2 x the family's worst ratio",
           "device": torch.cuda.get_device_name(0), "limit": F.R_LIMIT, "worst_ratio": worst_ratio, "R": R, "cases": rows}
    print(json.dumps({"worst_ratio": worst_ratio, "R": R}))
    if args.only is None:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:  # one case per line
            head = json.dumps({k: v for k, v in out.items() if k != "cases"}, indent=1)
            f.write(head[:-2] + ',\n "cases": [\n' + ",\n".join("  " + json.dumps(r) for r in rows) + "\n ]\n}\n")


if __name__ == "__main__":
    main()
