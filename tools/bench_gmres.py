#!/usr/bin/env python3
"""Restarted GMRES on device handles (spl_gmres_*) and its fused multi-vector inner product, one MI355X.

  (a) spl_vector_dots_dev, k = 4, 16, 32 columns of n = 8.0e6 entries, real and complex, at the batch widths 2, 4 and 8
      (SPL_GMRES_DOTS_BATCH; the default is the library's), against the loop of k spl_vector_dot_dev calls (the only way
      before) and against a device-to-device copy of the (k + 1) vectors' bytes (what any pass must at least read).
  (b) ms per GMRES step (a solve of `restart` steps that cannot converge, rtol = atol = 0, one cycle, divided by
      restart) for restart = 10, 30, 50 on poisson3d(200) and random(1e6, 20) 0.02 + 2 I with M = none, Jacobi and the
      AMG cycle, and beside it the sum of the step's parts timed alone: one SpMV, one M^-1, and copies of the vector
      bytes CGS2 must move (step j: two coefficient passes read j + 2 vectors each, two updates read j + 2 and write 1,
      the division reads and writes 1: 4 j + 12 vector passes, 2 restart + 10 on average; a copy of a vector is two).
  (c) whole solves to rtol 1e-8 of the unsymmetric 3-D upwind convection-diffusion operator L (x) I (x) I + I (x) L (x) I
      + I (x) I (x) L, L = tridiag(-1 - g, 2 + g, -1) (g = --gamma, the cell Peclet number), assembled handle to handle
      with kronecker / lin, on 64^3 and 200^3: GMRES(30) against BiCGSTAB with M = none, multicolour ILU(0) (both
      solvers on the permuted handle P A P^T of spl_matrix_color) and AMG.  Iterations, ms and the reason of each.

Every case is warmed up; a time is a host clock around a call that ends in a device synchronise; medians of --rounds with
[min, max].  Nothing is asserted about a ratio: it is recorded.  Prints one JSON line (and writes it to --out).
python tools/bench_gmres.py [--n 8000000] [--m3 200] [--nr 1000000] [--k 20] [--small-m3 64] [--gamma 1.0] [--rounds 5] [--maxiter 3000]
                            [--parts a,b,c] [--out profiles/gmres_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KNOBS = ("SPL_TRSV_SMALL_ROWS", "SPL_TRSV_SEGMENT_LEVELS", "SPL_KRYLOV_GRID", "SPL_GMRES_DOTS_BATCH", "SPL_AMG_TAIL_ROWS")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8_000_000)
    ap.add_argument("--m3", type=int, default=200)
    ap.add_argument("--nr", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--small-m3", type=int, default=64)
    ap.add_argument("--gamma", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--maxiter", type=int, default=3000)
    ap.add_argument("--parts", default="a,b,c")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    torch.cuda.set_device(0)
    DM = pkg.DeviceMatrix
    wanted = args.parts.split(",")

    def clock(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def timed(f, rounds, warmup=1, per=1):
        for _ in range(warmup):
            clock(f)
        ts = [clock(f) / per for _ in range(rounds)]
        return statistics.median(ts), {"ms": round(statistics.median(ts) * 1e3, 4),
                                       "ms_min_max": [round(min(ts) * 1e3, 4), round(max(ts) * 1e3, 4)]}

    def rhs(n, cplx):
        gen = torch.Generator(device="cuda").manual_seed(n)
        b = torch.rand(n, dtype=torch.float64, device="cuda", generator=gen) - 0.5
        return b.to(torch.complex128) if cplx else b

    # ---- (a) -----------------------------------------------------------------------------------------------------------
    def dots_cells():
        cells = []
        n = args.n
        stream = torch.cuda.current_stream().cuda_stream
        for cplx in (False, True):
            dtype = torch.complex128 if cplx else torch.float64
            step = 16 if cplx else 8
            for k in (4, 16, 32):
                V = torch.rand(k * n, dtype=torch.float64, device="cuda").to(dtype)
                w = rhs(n, cplx)
                out = torch.zeros(k, dtype=dtype, device="cuda")
                sink = torch.empty((k + 1) * n, dtype=dtype, device="cuda")
                src = torch.empty((k + 1) * n, dtype=dtype, device="cuda")

                def loop():
                    for i in range(k):
                        pkg.vector_dot_dev(n, V.data_ptr() + i * n * step, w.data_ptr(), out.data_ptr() + i * step, cplx, stream)
                m_loop, t_loop = timed(loop, args.rounds)
                by_width = {}
                for width in ("2", "4", "8"):
                    os.environ["SPL_GMRES_DOTS_BATCH"] = width
                    m, t = timed(lambda: pkg.vector_dots_dev(n, k, V.data_ptr(), n, w.data_ptr(), out.data_ptr(), cplx, stream),
                                 args.rounds)
                    by_width[width] = dict(t, loop_over_fused=round(m_loop / m, 2))
                os.environ.pop("SPL_GMRES_DOTS_BATCH", None)
                m_def, t_def = timed(lambda: pkg.vector_dots_dev(n, k, V.data_ptr(), n, w.data_ptr(), out.data_ptr(), cplx, stream),
                                     args.rounds)
                m_copy, t_copy = timed(lambda: sink.copy_(src), args.rounds)
                cell = {"values": "complex" if cplx else "real", "n": n, "k": k, "loop_of_k_single_dots": t_loop,
                        "fused_by_batch_width": by_width, "fused_default_width": t_def,
                        "copy_of_k_plus_1_vectors": t_copy, "loop_over_fused": round(m_loop / m_def, 2),
                        "fused_over_copy": round(m_def / m_copy, 2),
                        "read_GBps_fused": round((k + 1) * n * step / m_def / 1e9, 1)}
                print("%r" % (cell,), file=sys.stderr, flush=True)
                cells.append(cell)
                del V, w, sink, src
                torch.cuda.empty_cache()
        return cells

    # ---- (b) -----------------------------------------------------------------------------------------------------------
    def dominant_random(n):
        R = DM.synthetic("random", n, args.k)
        R0 = R.scale(0.02)
        R.free()
        D = R0.lin(1.0, DM.ident(n), 2.0)
        R0.free()
        return D

    def step_cells(name, H, amg_options):
        cells = []
        inf = H.info()
        n = inf["nrows_global"]
        stream = torch.cuda.current_stream().cuda_stream
        b = rhs(n, False)
        x = torch.empty_like(b)
        y = torch.empty_like(b)
        cycle = H.amg(**amg_options)
        m_spmv, t_spmv = timed(lambda: H.spmv_dev(b.data_ptr(), y.data_ptr(), False, stream), args.rounds)
        m_copy, t_copy = timed(lambda: y.copy_(b), args.rounds)
        for kind in (None, "jacobi", "amg"):
            m_pre, t_pre = 0.0, None
            if kind == "jacobi":
                d = torch.rand(n, dtype=torch.float64, device="cuda")
                m_pre, t_pre = timed(lambda: torch.mul(d, b, out=y), args.rounds)  # stands for the entry-wise kernel
            if kind == "amg":
                m_pre, t_pre = timed(lambda: cycle.apply_dev(b.data_ptr(), y.data_ptr(), stream), args.rounds)
            for restart in (10, 30, 50):
                S = H.gmres(restart, cycle if kind == "amg" else kind)

                def run():
                    S.solve_dev(b.data_ptr(), x.data_ptr(), False, 0.0, 0.0, restart, 0, False, stream)
                m_step, t_step = timed(run, args.rounds, per=restart)
                info = S.info()
                passes = 2 * restart + 10
                parts_ms = (m_spmv + m_pre + passes / 2.0 * m_copy) * 1e3
                cell = {"workload": name, "n": n, "nnz": inf["nnz"], "preconditioner": str(kind), "restart": restart,
                        "ms_per_step": t_step, "launches_of_the_solve": info["launches"], "device_bytes": info["device_bytes"],
                        "one_spmv": t_spmv, "one_preconditioner_application": t_pre, "copy_of_one_vector": t_copy,
                        "vector_passes_per_step_on_average": passes, "sum_of_parts_ms": round(parts_ms, 4),
                        "step_over_sum_of_parts": round(m_step * 1e3 / parts_ms, 2)}
                print("%r" % (cell,), file=sys.stderr, flush=True)
                cells.append(cell)
                S.free()
                torch.cuda.empty_cache()
        cycle.free()
        return cells

    # ---- (c) -----------------------------------------------------------------------------------------------------------
    def convection_diffusion(m, gamma):
        """L (x) I (x) I + I (x) L (x) I + I (x) I (x) L with the 1-D first-order upwind operator L, handle to handle"""
        rp = np.concatenate([[0], np.cumsum(np.concatenate([[2], np.full(m - 2, 3), [2]]))]).astype(np.int64)
        rows = np.repeat(np.arange(m), np.diff(rp))
        ci = (rows + (np.arange(3 * m - 2) - rp[rows]) - (rows > 0)).astype(np.int32)
        v = np.where(ci == rows, 2.0 + gamma, np.where(ci < rows, -1.0 - gamma, -1.0))
        L = DM.from_csr(m, m, rp, ci, v)
        I = DM.ident(m)
        II = I.kronecker(I)
        terms = [L.kronecker(II), I.kronecker(L).kronecker(I), II.kronecker(L)]
        two = terms[0].lin(1.0, terms[1], 1.0)
        A = two.lin(1.0, terms[2], 1.0)
        for h in terms + [two, II, I, L]:
            h.free()
        return A

    def whole_solves(m):
        out = []
        A = convection_diffusion(m, args.gamma)
        inf = A.info()
        n = inf["nrows_global"]
        stream = torch.cuda.current_stream().cuda_stream
        b = rhs(n, False)
        x = torch.empty_like(b)
        coloring = A.coloring()
        B = coloring.permute()
        ilu = B.ilu0()
        cycle = A.amg()
        for kind, H, M in (("none", A, None), ("multicolour ilu0", B, ilu), ("amg", A, cycle)):
            row = {"instance": "upwind convection-diffusion %d^3, cell Peclet %g" % (m, args.gamma), "n": n, "nnz": inf["nnz"],
                   "preconditioner": kind, "rtol": 1e-8, "max_iter": args.maxiter}
            for label, make in (("gmres(30)", lambda: H.gmres(30, M)), ("bicgstab", lambda: H.krylov("bicgstab", M))):
                S = make()
                got = {}

                def run():
                    got["res"] = S.solve_dev(b.data_ptr(), x.data_ptr(), False, 1e-8, 0.0, args.maxiter, 0, False, stream)
                m_s, t_s = timed(run, min(args.rounds, 2))
                res = got["res"]
                row[label] = dict(t_s, iterations=res["iterations"], reason=res["reason_name"], spmvs=res["spmvs"],
                                  preconditioner_applications=res["preconditioner_applications"])
                if "cycles" in res:
                    row[label].update(cycles=res["cycles"], true_residual=res["residual"])
                S.free()
            row["gmres_over_bicgstab"] = round(row["gmres(30)"]["ms"] / row["bicgstab"]["ms"], 2)
            print("%r" % (row,), file=sys.stderr, flush=True)
            out.append(row)
        cycle.free()
        ilu.free()
        B.free()
        A.free()
        torch.cuda.empty_cache()
        return out

    for key in KNOBS:
        os.environ.pop(key, None)
    result = {"what": "tools/bench_gmres.py: restarted GMRES on device handles (spl_gmres_*) and spl_vector_dots_dev, one "
                      "MI355X, host clock ending in a synchronise, %d rounds after a warm-up, medians with [min, max]; the "
                      "parts are timed alone and are yardsticks, not the code under test" % args.rounds,
              "device": torch.cuda.get_device_name(0)}
    if "a" in wanted:
        result["a_fused_inner_products"] = dots_cells()
    if "b" in wanted:
        cells = []
        P = DM.synthetic("poisson3d", args.m3)
        cells += step_cells("poisson3d(%d)" % args.m3, P, {})
        P.free()
        torch.cuda.empty_cache()
        R = dominant_random(args.nr)
        cells += step_cells("random(%d, %d) 0.02 + 2 I" % (args.nr, args.k), R, {"plain": True})
        R.free()
        torch.cuda.empty_cache()
        result["b_ms_per_step"] = cells
    if "c" in wanted:
        result["c_whole_solves"] = whole_solves(args.small_m3) + whole_solves(args.m3)
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
