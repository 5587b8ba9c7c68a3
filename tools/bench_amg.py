#!/usr/bin/env python3
"""Aggregation AMG on device handles (spl_matrix_aggregate, spl_amg_*), one MI355X.

  poisson3d(m)            m = 200: 8.0e6 rows, 5.6e7 entries, and m = 64; CG
  poisson3d(m), complex   the same matrix promoted (Hermitian positive definite); CG
  random(n, K) 0.02 + 2 I n = 1e6, K = 20: BiCGSTAB.  It converges in a handful of iterations without any help, and its
                          smoothed Galerkin product is out of proportion (a row of A P has K^2 entries: 4e8 entries and
                          about 9e9 products for R (A P)), so this case is measured with the PLAIN prolongator

For every case: the setup time (spl_amg_create, everything included), the level sizes and the operator complexity, the
time and the kernel launches of one application of the cycle with the tail kernel (the default) and without it
(SPL_AMG_TAIL_ROWS=0: a launch per step on every level), one SpMV of A beside it, and the whole solve to rtol 1e-8 with
no preconditioner, with Jacobi and with the cycle (setup not included: it is its own column).

Every case is warmed up; a time is a host clock around a call that ends in a device synchronise; medians of --rounds with
[min, max].  Nothing is asserted about a ratio: it is recorded.  Prints one JSON line (and writes it to --out).
python tools/bench_amg.py [--m3 200] [--small-m3 64] [--n 1000000] [--k 20] [--rounds 3] [--cases all]
                          [--out profiles/amg_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KNOBS = ("SPL_AMG_GRID", "SPL_AMG_CHECK_EVERY", "SPL_AMG_TAIL_ROWS", "SPL_KRYLOV_GRID")
CASES = ("poisson", "poisson_small", "poisson_complex", "random")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m3", type=int, default=200)
    ap.add_argument("--small-m3", type=int, default=64)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--cases", default="all")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    torch.cuda.set_device(0)
    DM = pkg.DeviceMatrix
    wanted = CASES if args.cases == "all" else tuple(args.cases.split(","))

    def clock(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def timed(f, rounds, warmup=1):
        for _ in range(warmup):
            clock(f)
        ts = [clock(f) for _ in range(rounds)]
        return statistics.median(ts), {"ms": round(statistics.median(ts) * 1e3, 4),
                                       "ms_min_max": [round(min(ts) * 1e3, 4), round(max(ts) * 1e3, 4)]}

    def poisson(m, cplx):
        P = DM.synthetic("poisson3d", m)
        if not cplx:
            return P
        Z = P.to_complex()
        P.free()
        return Z

    def dominant_random(n):
        R = DM.synthetic("random", n, args.k)
        R0 = R.scale(0.02)
        R.free()
        D = R0.lin(1.0, DM.ident(n), 2.0)
        R0.free()
        return D

    def rhs(n, cplx):
        gen = torch.Generator(device="cuda").manual_seed(n)
        b = torch.rand(n, dtype=torch.float64, device="cuda", generator=gen) - 0.5
        return b.to(torch.complex128) if cplx else b

    def case(name, H, method, **options):
        inf = H.info()
        n, cplx = inf["nrows_global"], H.is_complex
        stream = torch.cuda.current_stream().cuda_stream
        b = rhs(n, cplx)
        x = torch.empty_like(b)
        made = {}

        def setup():
            if "M" in made:
                made["M"].free()
            made["M"] = H.amg(**options)

        os.environ.pop("SPL_AMG_TAIL_ROWS", None)
        _, t_setup = timed(setup, min(args.rounds, 2), warmup=1)
        M = made["M"]
        info = M.info()
        sizes = [M.level(l)["dims"][0] for l in range(info["levels"])]
        m_spmv, t_spmv = timed(lambda: H.spmv_dev(b.data_ptr(), x.data_ptr(), False, stream), args.rounds)

        def application(obj):
            """the time of one application, and its launches: 5 + 2 (nu - 1) + 2 nu on a level with a coarser one, 1 +
            2 (coarse_sweeps - 1) on the coarsest, the SpMV counted as one, and 1 for all tail levels together"""
            nu, coarse = options.get("sweeps", 1), options.get("coarse_sweeps", 4)
            first = obj.info()["tail_first"]
            count = obj.info()["levels"]
            launches = 0
            for l in range(count):
                if l == first:
                    launches += 1
                    break
                launches += 1 + 2 * (coarse - 1) if l == count - 1 else 5 + 2 * (nu - 1) + 2 * nu
            m, t = timed(lambda: obj.apply_dev(b.data_ptr(), x.data_ptr(), stream), args.rounds)
            return m, t, launches

        m_app, t_app, l_app = application(M)
        os.environ["SPL_AMG_TAIL_ROWS"] = "0"
        flat = H.amg(**options)
        os.environ.pop("SPL_AMG_TAIL_ROWS", None)
        m_flat, t_flat, l_flat = application(flat)
        flat.free()
        solves = {}
        for kind, pre in (("none", None), ("jacobi", "jacobi"), ("amg", M)):
            solver = H.krylov(method, pre)
            got = {}

            def run():
                got["res"] = solver.solve_dev(b.data_ptr(), x.data_ptr(), False, 1e-8, 0.0, 20000, 0, False, stream)
            m, t = timed(run, args.rounds)
            solves[kind] = dict(t, iterations=got["res"]["iterations"], reason=got["res"]["reason_name"],
                                launches_per_iteration=solver.info()["launches_per_iteration"])
            solver.free()
        out = {"workload": name, "values": "complex" if cplx else "real", "method": method, "n": n, "nnz": inf["nnz"],
               "options": {k: (int(v) if not isinstance(v, bool) else v) for k, v in options.items()},
               "setup": t_setup, "levels": sizes, "operator_complexity": round(info["operator_complexity"], 3),
               "first_tail_level": info["tail_first"], "device_bytes": info["device_bytes"],
               "one_application": t_app, "one_application_launches": l_app,
               "one_application_without_tail": t_flat, "one_application_without_tail_launches": l_flat,
               "one_spmv": t_spmv, "application_over_spmv": round(m_app / m_spmv, 2),
               "solve_to_1e-8": solves,
               "amg_solve_over_plain_solve": round(solves["amg"]["ms"] / solves["none"]["ms"], 3),
               "amg_setup_and_solve_over_plain_solve": round((solves["amg"]["ms"] + t_setup["ms"]) / solves["none"]["ms"], 3)}
        M.free()
        print("%r" % (out,), file=sys.stderr, flush=True)
        return out

    for key in KNOBS:
        os.environ.pop(key, None)
    cases = []
    if "poisson" in wanted:
        P = poisson(args.m3, False)
        cases.append(case("poisson3d(%d)" % args.m3, P, "cg"))
        P.free()
        torch.cuda.empty_cache()
    if "poisson_small" in wanted:
        P = poisson(args.small_m3, False)
        cases.append(case("poisson3d(%d)" % args.small_m3, P, "cg"))
        P.free()
    if "poisson_complex" in wanted:
        Z = poisson(args.m3, True)
        cases.append(case("poisson3d(%d)" % args.m3, Z, "cg"))
        Z.free()
        torch.cuda.empty_cache()
    if "random" in wanted:
        R = dominant_random(args.n)
        cases.append(case("random(%d, %d) 0.02 + 2 I" % (args.n, args.k), R, "bicgstab", plain=True))
        R.free()
    line = json.dumps({"what": "tools/bench_amg.py: aggregation AMG on device handles (spl_amg_*), one MI355X, host clock "
                               "ending in a synchronise, %d rounds after a warm-up, medians with [min, max]; the solves "
                               "run to rtol 1e-8 from x = 0 and do not include the setup, which is its own column; the "
                               "launches of an application follow from the levels (csrc/amg.hip)" % args.rounds,
                       "device": torch.cuda.get_device_name(0),
                       "defaults": {"sweeps": 1, "coarse_size": 256, "coarse_sweeps": 4, "SPL_AMG_TAIL_ROWS": 1024},
                       "cases": cases})
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
