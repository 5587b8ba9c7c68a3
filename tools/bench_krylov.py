#!/usr/bin/env python3
"""Preconditioned CG and BiCGSTAB on device handles (spl_krylov_*), one MI355X.

  poisson3d(m)            m = 200: 8.0e6 rows, 5.6e7 entries; CG with no preconditioner, Jacobi and ILU(0)
  random(n, K) + 2 I      n = 1e6, K = 20, the generator's values scaled by 0.02: BiCGSTAB with ILU(0)
  poisson3d(m), complex   the same matrix promoted (Hermitian positive definite): CG with none and ILU(0)

For every cell: the time per iteration (a solve of --iters iterations that cannot converge, rtol = atol = 0, divided
by --iters) at check_every = 1, 4, 16 and 64, the kernel launches per iteration, and beside it the sum of its parts
timed alone: one spl_matrix_spmv_dev, one application of the preconditioner, and device-to-device copies of as many
vector bytes as the fused kernels and the inner products of one iteration read and write (CG: 13 vector passes, 11 without a
preconditioner, BiCGSTAB: 23; a copy of one vector is two passes).  Then the whole solve to rtol against the host route a user had
before — export_csr, scipy.sparse.linalg.cg / bicgstab with the same start (zero) and tolerance and no preconditioner or
Jacobi, upload of x — on a SMALLER instance (--host-m3, --host-n: scipy is single-threaded), and on the chain
tridiagonal(--chain) with ILU(0) (on the host: its complete LU, which has no fill), where every row is a level of its
own and the host's serial substitution wins.

The last level of the fold is a launch of one workgroup that also does the scalar step; the other mechanism the design
names (every workgroup of the consuming kernel repeats the last fold) is not built, so there is one column.

Every case is warmed up; a time is a host clock around a call that ends in a device synchronise; medians of --rounds with
[min, max].  Nothing is asserted about a ratio: it is recorded.  Prints one JSON line (and writes it to --out).
python tools/bench_krylov.py [--m3 200] [--n 1000000] [--k 20] [--iters 40] [--rounds 5] [--host-m3 64] [--host-n 100000] [--chain 1000000]
                             [--out profiles/krylov_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KNOBS = ("SPL_TRSV_SMALL_ROWS", "SPL_TRSV_SEGMENT_LEVELS", "SPL_KRYLOV_GRID")
# vector reads and writes of the solver's own kernels per iteration; CG without a preconditioner does not compute
# <r,z> = <r,r> again: two passes less
PASSES = {"cg": 13, "cg_plain": 11, "bicgstab": 23}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m3", type=int, default=200)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-m3", type=int, default=64)
    ap.add_argument("--host-n", type=int, default=100_000)
    ap.add_argument("--chain", type=int, default=1_000_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    torch.cuda.set_device(0)
    DM = pkg.DeviceMatrix
    try:
        import scipy.sparse as sp
        import scipy.sparse.linalg as spla
    except ImportError:
        sp = None

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

    def tridiagonal(n):
        """2 on and -1 beside the diagonal: its ILU(0) is its LU, and every row is a level of its own"""
        rp = np.concatenate([[0], np.cumsum(np.concatenate([[2], np.full(n - 2, 3), [2]]))]).astype(np.int64)
        ci = np.empty(3 * n - 2, dtype=np.int32)
        v = np.empty(3 * n - 2)
        rows = np.repeat(np.arange(n), np.diff(rp))
        pos = np.arange(3 * n - 2) - rp[rows]
        ci[:] = rows + pos - (rows > 0)
        v[:] = np.where(ci == rows, 2.0, -1.0)
        return DM.from_csr(n, n, rp, ci, v)

    def rhs(n, cplx):
        gen = torch.Generator(device="cuda").manual_seed(n)
        b = torch.rand(n, dtype=torch.float64, device="cuda", generator=gen) - 0.5
        return b.to(torch.complex128) if cplx else b

    def cell(name, H, method, kind, iters):
        inf = H.info()
        n, cplx = inf["nrows_global"], H.is_complex
        stream = torch.cuda.current_stream().cuda_stream
        M = H.ilu0() if kind == "ilu0" else kind
        S = H.krylov(method, M)
        b = rhs(n, cplx)
        x = torch.empty_like(b)
        y = torch.empty_like(b)
        by_interval = {}
        launches = None
        for every in (1, 4, 16, 64):
            def run():
                S.solve_dev(b.data_ptr(), x.data_ptr(), False, 0.0, 0.0, iters, every, False, stream)
            m, t = timed(run, args.rounds, per=iters)
            by_interval[str(every)] = t
            launches = S.info()["launches_per_iteration"]
        m_it = by_interval["16"]["ms"]
        m_spmv, t_spmv = timed(lambda: H.spmv_dev(b.data_ptr(), y.data_ptr(), False, stream), args.rounds)
        t1, mid, t2 = S.parts
        m_pre, t_pre = 0.0, None
        if kind is not None:
            def apply():
                cur = b.data_ptr()
                if t1 is not None:
                    t1.solve_dev(cur, n, y.data_ptr(), n, 1, "N", stream)
                    cur = y.data_ptr()
                if mid is not None:
                    torch.mul(mid, b, out=y)  # stands for the entry-wise kernel: three vector passes
                    cur = y.data_ptr()
                if t2 is not None:
                    t2.solve_dev(cur, n, y.data_ptr(), n, 1, "N", stream)
            m_pre, t_pre = timed(apply, args.rounds)
        m_copy, t_copy = timed(lambda: y.copy_(b), args.rounds)
        per = {"cg": (1, 1), "bicgstab": (2, 2)}[method]
        passes = PASSES["cg_plain" if method == "cg" and kind is None else method]
        parts_ms = (per[0] * m_spmv + per[1] * m_pre + passes / 2.0 * m_copy) * 1e3
        out = {"workload": name, "values": "complex" if cplx else "real", "method": method, "preconditioner": str(kind),
               "n": n, "nnz": inf["nnz"], "iterations_timed": iters, "launches_per_iteration": launches, "vector_passes_per_iteration": passes,
               "ms_per_iteration_by_check_every": by_interval,
               "one_spmv": t_spmv, "one_preconditioner_application": t_pre, "copy_of_one_vector": t_copy,
               "sum_of_parts_ms": round(parts_ms, 4), "iteration_over_sum_of_parts": round(m_it / parts_ms, 2),
               "last_fold": "one-workgroup launch (the only mechanism built)"}
        S.free()
        if kind == "ilu0":
            M.free()
        print("%r" % (out,), file=sys.stderr, flush=True)
        return out

    def whole_solve(name, H, method, kind, rtol, check_every=0, rounds=3):
        """the device solve to rtol against export + scipy + upload on the same (smaller) instance"""
        inf = H.info()
        n, cplx = inf["nrows_global"], H.is_complex
        stream = torch.cuda.current_stream().cuda_stream
        b = rhs(n, cplx)
        x = torch.empty_like(b)
        got = {}

        def device():
            M = H.ilu0() if kind == "ilu0" else kind
            S = H.krylov(method, M)
            got["res"] = S.solve_dev(b.data_ptr(), x.data_ptr(), False, rtol, 0.0, 20000, check_every, False, stream)
            S.free()
            if kind == "ilu0":
                M.free()

        m_dev, t_dev = timed(device, min(args.rounds, rounds))
        out = {"instance": name, "n": n, "method": method, "preconditioner": str(kind), "rtol": rtol,
               "check_every": check_every or 16,
               "device_setup_and_solve": t_dev, "device_iterations": got["res"]["iterations"],
               "device_reason": got["res"]["reason_name"]}
        if sp is None:
            out["host"] = "scipy is not installed"
            return out
        count = [0]

        def host():
            rp, ci, v = H.export_csr()
            A = sp.csr_matrix((v, ci, rp), shape=(n, n))
            Mh = None
            if kind == "jacobi":
                d = 1.0 / A.diagonal()
                Mh = spla.LinearOperator((n, n), matvec=lambda r: d * r, dtype=A.dtype)
            if kind == "ilu0":  # only asked for the tridiagonal chain, whose complete LU without interchanges has no
                # fill: it IS the ILU(0).  (spilu is SuperLU's threshold ILU with secondary dropping: on this matrix it
                # drops a sixth of L, and scipy's cg then does not converge in 200 iterations.)
                f0 = spla.splu(A.tocsc(), permc_spec="NATURAL", diag_pivot_thresh=0)
                Mh = spla.LinearOperator((n, n), matvec=f0.solve, dtype=A.dtype)
            count[0] = 0

            def tick(_):
                count[0] += 1
            f = spla.cg if method == "cg" else spla.bicgstab
            xh, info = f(A, b.cpu().numpy(), rtol=rtol, atol=0.0, M=Mh, callback=tick, maxiter=20000)
            torch.from_numpy(xh).cuda()
            got["info"] = info

        m_host, t_host = timed(host, 1, warmup=0)
        out.update(host_export_scipy_upload=t_host, host_iterations=count[0], host_info=int(got["info"]),
                   host_over_device=round(m_host / m_dev, 2))
        print("%r" % (out,), file=sys.stderr, flush=True)
        return out

    for key in KNOBS:
        os.environ.pop(key, None)
    cells, solves = [], []
    P = poisson(args.m3, False)
    for kind in (None, "jacobi", "ilu0"):
        cells.append(cell("poisson3d(%d)" % args.m3, P, "cg", kind, args.iters))
    P.free()
    torch.cuda.empty_cache()
    R = dominant_random(args.n)
    cells.append(cell("random(%d, %d) 0.02 + 2 I" % (args.n, args.k), R, "bicgstab", "ilu0", max(args.iters // 8, 2)))
    R.free()
    torch.cuda.empty_cache()
    Z = poisson(args.m3, True)
    for kind in (None, "ilu0"):
        cells.append(cell("poisson3d(%d)" % args.m3, Z, "cg", kind, args.iters))
    Z.free()
    torch.cuda.empty_cache()
    Ps = poisson(args.host_m3, False)
    for kind in (None, "jacobi"):
        solves.append(whole_solve("poisson3d(%d)" % args.host_m3, Ps, "cg", kind, 1e-8))
    Ps.free()
    Rs = dominant_random(args.host_n)
    solves.append(whole_solve("random(%d, %d) 0.02 + 2 I" % (args.host_n, args.k), Rs, "bicgstab", None, 1e-8))
    Rs.free()
    Cs = tridiagonal(args.chain)
    solves.append(whole_solve("tridiagonal(%d): a chain, one row per level" % args.chain, Cs, "cg", "ilu0", 1e-8,
                              check_every=1, rounds=1))  # a look after every iteration: an application costs a second
    Cs.free()
    Zs = poisson(args.host_m3, True)
    solves.append(whole_solve("poisson3d(%d) complex" % args.host_m3, Zs, "cg", None, 1e-8))
    Zs.free()
    line = json.dumps({"what": "tools/bench_krylov.py: preconditioned CG and BiCGSTAB on device handles (spl_krylov_*), one MI355X, "
                               "host clock ending in a synchronise, %d rounds after a warm-up, medians with [min, max]; a time "
                               "per iteration is a solve of iterations_timed iterations that cannot converge divided by "
                               "that number; the parts are timed alone and are yardsticks, not the code under test" % args.rounds,
                       "device": torch.cuda.get_device_name(0),
                       "defaults": {"check_every": 16, "SPL_KRYLOV_GRID": 2048},
                       "cells": cells, "whole_solves_against_the_host_route": solves})
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
