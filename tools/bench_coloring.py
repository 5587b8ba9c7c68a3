#!/usr/bin/env python3
"""Multicolour ordering on device handles (spl_matrix_color) and what it buys ILU(0) and the Krylov solvers, one MI355X.

  poisson3d(m)          m = 200 (8.0e6 rows) and m = 64: CG
  random(n, K) + 2 I    n = 1e6, K = 20, the generator's values scaled by 0.02: BiCGSTAB
  tridiagonal(n)        n = 1e6, 2 and -1: a chain, every row a level of its own in the natural order: CG

For every workload:
  * the colouring (colours, permutation and offsets) at SPL_COLOR_CHECK_EVERY = 1, 4, 8, 16 and 64, with colours, rounds
    and launches, beside one spl_matrix_spmv_dev, the select that makes P A P^T and the spl_trisolve_analyze it feeds;
  * ILU(0) in the natural and in the multicolour numbering: levels, one refactorisation, one application (two solves);
  * the whole solve to rtol with no preconditioner, natural ILU(0) and multicolour ILU(0) (Coloring.krylov: the
    permutations of b and x are inside the time, the set-up is beside it): iterations, time, time per iteration = time /
    iterations.  A solve that does not converge in --maxiter iterations says so.

Every case is warmed up unless it takes seconds (the chain in its natural order: one run); a time is a host clock around
a call that ends in a device synchronise; medians of --rounds with [min, max].  Nothing is asserted about a ratio: it is
recorded.  Prints one JSON line (and writes it to --out).
python tools/bench_coloring.py [--m3 200] [--m3-small 64] [--n 1000000] [--k 20] [--chain 1000000] [--rounds 3]
                               [--maxiter 5000] [--out profiles/coloring_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KNOBS = ("SPL_COLOR_CHECK_EVERY", "SPL_COLOR_GRID", "SPL_TRSV_SMALL_ROWS", "SPL_TRSV_SEGMENT_LEVELS", "SPL_KRYLOV_GRID")
INTERVALS = (1, 4, 8, 16, 64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m3", type=int, default=200)
    ap.add_argument("--m3-small", type=int, default=64)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--chain", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--maxiter", type=int, default=5000)
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    torch.cuda.set_device(0)
    DM = pkg.DeviceMatrix

    def clock(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def timed(f, rounds=None, warmup=1):
        for _ in range(warmup):
            clock(f)
        ts = [clock(f) for _ in range(rounds or args.rounds)]
        return {"ms": round(statistics.median(ts) * 1e3, 4), "ms_min_max": [round(min(ts) * 1e3, 4), round(max(ts) * 1e3, 4)]}

    def dominant_random(n):
        R = DM.synthetic("random", n, args.k)
        R0 = R.scale(0.02)
        R.free()
        D = R0.lin(1.0, DM.ident(n), 2.0)
        R0.free()
        return D

    def tridiagonal(n):
        rp = np.concatenate([[0], np.cumsum(np.concatenate([[2], np.full(n - 2, 3), [2]]))]).astype(np.int64)
        rows = np.repeat(np.arange(n), np.diff(rp))
        ci = (rows + np.arange(3 * n - 2) - rp[rows] - (rows > 0)).astype(np.int32)
        return DM.from_csr(n, n, rp, ci, np.where(ci == rows, 2.0, -1.0))

    def rhs(n):
        gen = torch.Generator(device="cuda").manual_seed(n)
        return torch.rand(n, dtype=torch.float64, device="cuda", generator=gen) - 0.5

    def ilu_numbers(ilu, A, b, y, slow):
        n = A.info()["nrows_global"]
        stream = torch.cuda.current_stream().cuda_stream
        kw = {"rounds": 1, "warmup": 0} if slow else {}
        return {"levels": ilu.info()["levels"], "launches_per_factorisation": ilu.info()["launches"],
                "launches_per_application": ilu.lower.info()["launches"] + ilu.upper.info()["launches"],
                "one_refactorisation": timed(lambda: ilu.refactor(A), **kw),
                "one_application": timed(lambda: ilu.apply_dev(b.data_ptr(), n, y.data_ptr(), n, 1, "N", stream), **kw)}

    def solve_numbers(solver, b, slow):
        got = {}

        def run():
            got["x"], got["res"] = solver.solve(b, rtol=args.rtol, maxiter=args.maxiter)
        t = timed(run, **({"rounds": 1, "warmup": 0} if slow else {}))
        its = got["res"]["iterations"]
        return {"iterations": its, "reason": got["res"]["reason_name"], "whole_solve": t,
                "ms_per_iteration": round(t["ms"] / max(its, 1), 4)}, got["x"]

    def note(what):
        print("[bench_coloring] %s" % what, file=sys.stderr, flush=True)

    def workload(name, H, method, natural_is_slow=False):
        note(name)
        inf = H.info()
        n = inf["nrows_global"]
        stream = torch.cuda.current_stream().cuda_stream
        b, y = rhs(n), torch.empty(n, dtype=torch.float64, device="cuda")
        out = {"workload": name, "n": n, "nnz": inf["nnz"], "method": method,
               "one_spmv": timed(lambda: H.spmv_dev(b.data_ptr(), y.data_ptr(), False, stream), 5)}
        # the colouring
        by_interval = {}
        for every in INTERVALS:
            os.environ["SPL_COLOR_CHECK_EVERY"] = str(every)
            by_interval[str(every)] = dict(timed(lambda: H.coloring(0)), launches=H.coloring(0).info()["launches"])
        os.environ.pop("SPL_COLOR_CHECK_EVERY", None)
        col = H.coloring(0)
        cinf = col.info()
        held = {}
        out["coloring"] = {"colors": cinf["colors"], "rounds": cinf["rounds"], "max_degree": cinf["max_degree"],
                           "largest_class": cinf["largest_class"], "smallest_class": cinf["smallest_class"],
                           "launches_at_the_default": cinf["launches"], "at_the_default": timed(lambda: H.coloring(0)),
                           "by_check_every": by_interval,
                           "select_P_A_Pt": timed(lambda: held.__setitem__("B", col.permute()))}
        B = held["B"]
        out["coloring"]["trisolve_analyze_of_its_lower_triangle"] = timed(lambda: held.__setitem__("T", B.triangular("lower")))
        out["coloring"]["levels_of_that_triangle"] = held["T"].info()["levels"]
        held["T"].free()
        note("coloured: %d colours in %d rounds; ILU(0)" % (cinf["colors"], cinf["rounds"]))
        # ILU(0), natural against multicolour.  A refactorisation replaces the two triangular solvers of an ILU0, and a
        # KrylovSolver borrows them: the objects that are refactored here are not the ones the solvers below are given
        setup = {}
        t0 = clock(lambda: held.__setitem__("nat", H.ilu0()))
        setup["natural_ilu0_ms"] = round(t0 * 1e3, 2)
        held["probe"] = pkg.ILU0(B)
        out["ilu0"] = {"natural": ilu_numbers(held["nat"], H, b, y, natural_is_slow),
                       "multicolour": ilu_numbers(held["probe"], B, b, y, False), "first_setup": setup}
        held["probe"].free()
        # the solves: the solvers are made after the last refactorisation
        nat = held["nat"]
        t0 = clock(lambda: held.__setitem__("mc", H.coloring(0).krylov(method, "ilu0")))
        setup["multicolour_colour_select_ilu0_solver_ms"] = round(t0 * 1e3, 2)
        mc = held["mc"]
        plain = H.krylov(method, None)
        pre = H.krylov(method, nat)
        solves = {}
        note("the solves")
        solves["none"], _ = solve_numbers(plain, b, False)
        solves["natural_ilu0"], x_nat = solve_numbers(pre, b, natural_is_slow)
        solves["multicolour_ilu0"], x_mc = solve_numbers(mc, b, False)
        r = torch.empty_like(b)
        H.spmv_dev(x_mc.data_ptr(), r.data_ptr(), False, stream)
        solves["multicolour_ilu0"]["true_relative_residual"] = float(torch.linalg.norm(b - r) / torch.linalg.norm(b))
        H.spmv_dev(x_nat.data_ptr(), r.data_ptr(), False, stream)
        solves["natural_ilu0"]["true_relative_residual"] = float(torch.linalg.norm(b - r) / torch.linalg.norm(b))
        out["solves_to_rtol"] = solves
        for part in (plain, pre, mc, nat, B):
            part.free()
        print("%r" % (out,), file=sys.stderr, flush=True)
        return out

    for key in KNOBS:
        os.environ.pop(key, None)
    results = []
    for name, make, method, slow in (
            ("poisson3d(%d)" % args.m3, lambda: DM.synthetic("poisson3d", args.m3), "cg", False),
            ("poisson3d(%d)" % args.m3_small, lambda: DM.synthetic("poisson3d", args.m3_small), "cg", False),
            ("random(%d, %d) 0.02 + 2 I" % (args.n, args.k), lambda: dominant_random(args.n), "bicgstab", False),
            ("tridiagonal(%d): a chain" % args.chain, lambda: tridiagonal(args.chain), "cg", True)):
        H = make()
        results.append(workload(name, H, method, slow))
        H.free()
        torch.cuda.empty_cache()
    line = json.dumps({"what": "tools/bench_coloring.py: multicolour ordering on device handles (spl_matrix_color) and ILU(0) / CG / "
                               "BiCGSTAB in the natural and in the multicolour numbering, one MI355X, host clock ending in a "
                               "synchronise, %d rounds after a warm-up (the chain in its natural order: one run), medians with "
                               "[min, max]; solves to rtol %g with at most %d iterations, time per iteration = time / iterations"
                               % (args.rounds, args.rtol, args.maxiter),
                       "device": torch.cuda.get_device_name(0), "workloads": results})
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
