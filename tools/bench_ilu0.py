#!/usr/bin/env python3
"""ILU(0) on device handles (spl_ilu0_*), one MI355X.

  poisson3d(m)            m = 200: 8.0e6 rows, 5.6e7 entries, 598 levels; real, and complex (promoted, times 0.6 + 0.8i)
  random(n, K) + 2 I      n = 1e6, K = 20, the generator's values scaled by 0.02: diagonally dominant
  bidiagonal(n)           n = 1e6: a chain, one row per level — the all-narrow worst case

For every workload: the analysis (spl_ilu0_analyze: download of the pattern, the level pass on the host, upload of the
tables), the one-shot factorisation (spl_matrix_ilu0 = analysis + factorisation), the refactorisation on a kept plan
(spl_ilu0_factor alone), ILU0.refactor (that plus the analyses of the two triangles for the solves), and the two-solve
apply U^-1 L^-1 b with k = 1 and k = 8.  Beside them, as yardsticks that are not the code under test:
  copy     a device-to-device copy of the values: the byte floor of anything that produces nnz values
  trisolve spl_trisolve_solve_dev (k = 1) on the unit lower triangle of the same handle: the SAME launch chain over the
           same levels — refactorisation over trisolve is the honest figure of merit
  host     the route a user had before: export_csr, scipy.sparse.linalg.spilu(drop_tol=0, fill_factor=1,
           permc_spec="NATURAL", diag_pivot_thresh=0), upload of L and U.  scipy has no ILU(0): this is SuperLU's
           threshold ILU with secondary dropping, a DIFFERENT incomplete factorisation of comparable fill

Every case is warmed up; a time is a host clock around a call that ends in a device synchronise; medians with [min, max].
The analysis, the one-shot call and ILU0.refactor take at most 3 rounds; the host route is timed once.
Nothing is asserted about a ratio: it is recorded.  Prints one JSON line (and writes it to --out).
The host route is single-threaded and far from linear in n (minutes at 10^6 rows of the Poisson matrix), so it is timed
on a SMALLER instance of every workload (--host-m3, --host-n; the chain at its full size), against the one-shot device
call on that same smaller instance.
python tools/bench_ilu0.py [--m3 200] [--n 1000000] [--k 20] [--chain 1000000] [--rounds 5] [--host-m3 50]
                           [--host-n 20000] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KNOBS = ("SPL_TRSV_SMALL_ROWS", "SPL_TRSV_SEGMENT_LEVELS")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m3", type=int, default=200)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--chain", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-m3", type=int, default=50, help="grid of the Poisson instance the host route is timed on")
    ap.add_argument("--host-n", type=int, default=20000, help="rows of the random instance the host route is timed on")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    torch.cuda.set_device(0)
    DM = pkg.DeviceMatrix
    F = pkg._ffi
    L = F.lib()
    try:
        import scipy.sparse as sp
        from scipy.sparse.linalg import spilu
    except ImportError:
        sp = None

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
        return statistics.median(ts), {"ms": round(statistics.median(ts) * 1e3, 3),
                                       "ms_min_max": [round(min(ts) * 1e3, 3), round(max(ts) * 1e3, 3)]}

    def chain(n):
        """the lower bidiagonal matrix with 2 on and -1 below the diagonal"""
        rp = np.concatenate([[0], np.cumsum(np.concatenate([[1], np.full(n - 1, 2)]))]).astype(np.int64)
        ci = np.empty(2 * n - 1, dtype=np.int32)
        v = np.empty(2 * n - 1)
        ci[0], v[0] = 0, 2.0
        ci[1::2], v[1::2] = np.arange(0, n - 1), -1.0
        ci[2::2], v[2::2] = np.arange(1, n), 2.0
        return DM.from_csr(n, n, rp, ci, v)

    def host_route(H):
        """export, SuperLU's incomplete factorisation, upload of its two factors as handles"""
        rp, ci, v = H.export_csr()
        n = len(rp) - 1
        A = sp.csr_matrix((v, ci, rp), shape=(n, n)).tocsc()
        f = spilu(A, drop_tol=0, fill_factor=1, permc_spec="NATURAL", diag_pivot_thresh=0)
        out = []
        for M in (f.L, f.U):
            M = sp.csc_matrix(M)
            M.sort_indices()
            m = pkg.Matrix(n, n, M.indptr, M.indices, M.data)
            out.append(DM.from_csc_complex(m) if np.iscomplexobj(M.data) else DM.from_csc(m))
        fill = int(f.L.nnz + f.U.nnz - n)
        for h in out:
            h.free()
        return fill

    def workload(name, H, rounds, host_instance):
        """H: a whole square handle (freed here); host_instance(): (name, handle) of the instance the host route takes"""
        inf = H.info()
        n, nnz, cplx = inf["nrows_global"], inf["nnz"], H.is_complex
        tdt = torch.complex128 if cplx else torch.float64
        holder = {}

        def analyse():
            p = C.c_void_p()
            F.check("spl_ilu0_analyze", L.spl_ilu0_analyze(H.handle, C.byref(p)))
            L.spl_ilu0_free(C.byref(p))

        def one_shot():
            f = C.c_void_p()
            F.check("spl_matrix_ilu0", L.spl_matrix_ilu0(H.handle, C.byref(f)))
            L.spl_matrix_free(C.byref(f))

        _, t_analysis = timed(analyse, min(rounds, 3))
        _, t_one_shot = timed(one_shot, min(rounds, 3))
        I = H.ilu0()
        iinf = I.info()

        def refactor():
            f = C.c_void_p()
            F.check("spl_ilu0_factor", L.spl_ilu0_factor(I.plan, H.handle, C.byref(f)))
            L.spl_matrix_free(C.byref(f))

        m_re, t_refactor = timed(refactor, rounds)
        _, t_object = timed(lambda: I.refactor(H), min(rounds, 3))
        src = torch.zeros(nnz, dtype=tdt, device="cuda")
        dst = torch.empty_like(src)
        m_copy, t_copy = timed(lambda: dst.copy_(src), rounds)
        del src, dst
        T = H.triangular("lower", unit=True)
        tinf = T.info()
        stream = torch.cuda.current_stream().cuda_stream
        gen = torch.Generator(device="cuda").manual_seed(n)
        B = (torch.rand((8, n), dtype=torch.float64, device="cuda", generator=gen) - 0.5).to(tdt).contiguous()
        X = torch.empty((8, n), dtype=tdt, device="cuda")
        m_tri, t_tri = timed(lambda: T.solve_dev(B.data_ptr(), n, X.data_ptr(), n, 1, "N", stream), rounds)
        T.free()
        applies = []
        for k in (1, 8):
            m_ap, t_ap = timed(lambda: I.apply_dev(B.data_ptr(), n, X.data_ptr(), n, k, "N", stream), rounds)
            applies.append({"k": k, "apply": t_ap})
        del B, X
        cell = {"workload": name, "values": "complex" if cplx else "real", "n": n, "nnz": nnz,
                "levels": iinf["levels"], "launches_per_factorisation": iinf["launches"],
                "longest_row": iinf["longest_row"], "plan_device_bytes": iinf["device_bytes"], "singular": I.singular,
                "analysis": t_analysis, "one_shot_analysis_and_factorisation": t_one_shot,
                "refactorisation_on_a_kept_plan": t_refactor,
                "ILU0.refactor_with_the_two_triangle_analyses": t_object, "apply_two_solves": applies,
                "copy_of_the_values": t_copy, "refactorisation_over_copy": round(m_re / m_copy, 1),
                "trisolve_unit_lower_k1": t_tri, "trisolve_launches": tinf["launches"],
                "refactorisation_over_trisolve": round(m_re / m_tri, 2),
                "us_per_level": round(m_re * 1e6 / max(iinf["levels"], 1), 3)}
        I.free()
        H.free()
        if sp is None:
            cell["host_route"] = "scipy is not installed"
        else:  # on the smaller instance, against the one-shot device call on that same instance
            hname, Hs = host_instance()
            sinf = Hs.info()

            def one_shot_small():
                f = C.c_void_p()
                F.check("spl_matrix_ilu0", L.spl_matrix_ilu0(Hs.handle, C.byref(f)))
                L.spl_matrix_free(C.byref(f))

            m_dev, t_dev = timed(one_shot_small, min(rounds, 3))
            m_host, t_host = timed(lambda: holder.__setitem__("fill", host_route(Hs)), 1, warmup=0)
            cell["host_route"] = {"instance": hname, "n": sinf["nrows_global"], "nnz": sinf["nnz"], "host": t_host,
                                  "entries_of_its_L_and_U": holder["fill"], "device_one_shot_on_the_same_instance": t_dev,
                                  "host_over_device": round(m_host / m_dev, 1)}
            Hs.free()
        print("%s %s: %r" % (name, cell["values"], cell), file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
        return cell

    def poisson(m, cplx):
        P = DM.synthetic("poisson3d", m)
        if not cplx:
            return P
        Z = P.to_complex()
        P.free()
        ZP = Z.scale(0.6 + 0.8j)
        Z.free()
        return ZP

    def dominant_random(n):
        R = DM.synthetic("random", n, args.k)
        R0 = R.scale(0.02)  # the generator's values lie in [0.5, 1.5): the rows' absolute sums stay below 0.6
        R.free()
        D = R0.lin(1.0, DM.ident(n), 2.0)  # and 2 on the diagonal dominates them
        R0.free()
        return D

    for key in KNOBS:
        os.environ.pop(key, None)
    cells = []
    for cplx in (False, True):
        cells.append(workload("poisson3d(%d)" % args.m3, poisson(args.m3, cplx), args.rounds,
                              lambda: ("poisson3d(%d)" % args.host_m3, poisson(args.host_m3, cplx))))
    cells.append(workload("random(%d, %d) + 2 I" % (args.n, args.k), dominant_random(args.n), args.rounds,
                          lambda: ("random(%d, %d) + 2 I" % (args.host_n, args.k), dominant_random(args.host_n))))
    cells.append(workload("bidiagonal(%d)" % args.chain, chain(args.chain), args.rounds,
                          lambda: ("bidiagonal(%d)" % args.chain, chain(args.chain))))
    line = json.dumps({"what": "tools/bench_ilu0.py: ILU(0) on device handles (spl_ilu0_analyze / _factor, spl_matrix_ilu0, "
                               "ILU0.apply_dev), one MI355X, host clock ending in a synchronise, %d rounds after a warm-up; "
                               "medians with [min, max]; at most 3 rounds for the analysis, the one-shot call (also on the host route's "
                               "instance) and ILU0.refactor.  Yardsticks, not the code under test: a device-to-device copy of the "
                               "values, spl_trisolve_solve_dev on the unit lower triangle of the same handle (the same launch "
                               "chain), and the host route" % args.rounds,
                       "host_route": "export_csr + scipy.sparse.linalg.spilu(drop_tol=0, fill_factor=1, "
                                     "permc_spec='NATURAL', diag_pivot_thresh=0) + upload of L and U, timed once, on a SMALLER "
                                     "instance of the workload (it is single-threaded and far from linear in n) and compared "
                                     "with the one-shot device call on that same instance.  scipy has "
                                     "no ILU(0): this is a DIFFERENT incomplete factorisation (SuperLU's threshold ILU with "
                                     "secondary dropping) of comparable fill, so only the times are comparable",
                       "device": torch.cuda.get_device_name(0),
                       "defaults": {"SPL_TRSV_SMALL_ROWS": 64, "SPL_TRSV_SEGMENT_LEVELS": 1024},
                       "cells": cells})
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
