#!/usr/bin/env python3
"""Sparse triangular solves on device handles (spl_trisolve_*), one MI355X.

  tril / triu of poisson3d(m)   m = 200: 8.0e6 rows, 3.2e7 entries, 598 levels of up to about 3e4 rows
  tril of random(n, K)          n = 1e6, K = 20, the strict triangle scaled by 0.02, unit diagonal
  bidiagonal(n)                 n = 1e6: a chain, one row per level — the all-narrow worst case
  tril of poisson3d(m), complex the real handle promoted and multiplied by 0.6 + 0.8i on the device

For every workload: the time of the analysis (download of the pattern, the level pass on the host, the permuted copy), and
of a solve with k = 1 and k = 8 right-hand sides, ops N and T, with info's levels and launches.  Beside them, as
yardsticks that are not the code under test:
  spmv     spl_matrix_spmv_many_dev on the same triangular handle: the same bytes without a dependency, the floor the
           launch chain is judged against
  host     the route a user had before: export_csr, scipy.sparse.linalg.spsolve_triangular, upload of x
  share    SURVEY §8d's SpTRSV bytes, 12 nnz + 16 n (20 nnz + 32 n complex; 8 or 16 more per row and further column),
           over the solve time, as a share of 8 TB/s
and a short sweep of the two knobs (SPL_TRSV_SMALL_ROWS, SPL_TRSV_SEGMENT_LEVELS) on the Poisson triangle and on a
shorter chain, with the chain also solved one launch per level (SMALL_ROWS = 1) to price the narrow kernel per level.

Every case is warmed up; a time is a host clock around a call that ends in a device synchronise; medians with [min, max].
The device and the host route are compared once per workload (largest relative difference).  Nothing is asserted about
a ratio: it is recorded.  Prints one JSON line (and writes it to --out).
python tools/bench_trisolve.py [--m3 200] [--n 1000000] [--k 20] [--chain 1000000] [--sweep-chain 100000] [--rounds 5]
                               [--out FILE]"""
import argparse
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
    ap.add_argument("--sweep-chain", type=int, default=100_000)
    ap.add_argument("--rounds", type=int, default=5)
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
        from scipy.sparse.linalg import spsolve_triangular
        host_label = "export_csr + scipy.sparse.linalg.spsolve_triangular + upload"
    except ImportError:
        sp = None
        host_label = "export_csr + a serial numpy loop + upload"

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

    def with_knobs(knobs, f):
        for key, value in knobs.items():
            os.environ[key] = str(value)
        try:
            return f()
        finally:
            for key in knobs:
                os.environ.pop(key, None)

    def host_solve(H, lower, unit, B):
        rp, ci, v = H.export_csr()
        n = len(rp) - 1
        if sp is not None:
            A = sp.csr_matrix((v, ci, rp), shape=(n, n))
            X = spsolve_triangular(A, B, lower=lower, unit_diagonal=unit)
        else:
            X = np.array(B, copy=True)
            rows = range(n) if lower else range(n - 1, -1, -1)
            for i in rows:
                d = 1.0
                for q in range(rp[i], rp[i + 1]):
                    if ci[q] == i:
                        d = v[q]
                    else:
                        X[i] = X[i] - v[q] * X[ci[q]]
                if not unit:
                    X[i] = X[i] / d
        return torch.from_numpy(np.ascontiguousarray(X.T)).cuda()

    def workload(name, H, uplo, unit, rounds):
        """H: a triangular handle (freed here)"""
        inf = H.info()
        n, cplx = inf["nrows_global"], H.is_complex
        tdt = torch.complex128 if cplx else torch.float64
        holder = {}

        def analyse():
            if "T" in holder:
                holder.pop("T").free()
            holder["T"] = H.triangular(uplo, unit)

        _, t_analysis = timed(analyse, min(rounds, 3), warmup=1)
        T = holder["T"]
        tinf = T.info()
        nnz = tinf["stored"]
        cell = {"workload": name, "values": "complex" if cplx else "real", "uplo": uplo, "unit_diagonal": unit, "n": n,
                "stored": nnz, "levels": tinf["levels"], "launches_per_solve": tinf["launches"],
                "longest_row": tinf["longest_row"], "device_bytes": tinf["device_bytes"], "analysis": t_analysis,
                "solves": []}
        gen = torch.Generator(device="cuda").manual_seed(n)
        stream = torch.cuda.current_stream().cuda_stream
        for k in (1, 8):
            B = torch.rand((k, n), dtype=torch.float64, device="cuda", generator=gen) - 0.5
            if cplx:
                B = torch.complex(B, torch.rand((k, n), dtype=torch.float64, device="cuda", generator=gen) - 0.5)
            B = B.contiguous()
            X = torch.empty((k, n), dtype=tdt, device="cuda")
            Y = torch.empty((k, n), dtype=tdt, device="cuda")
            per_entry, per_row = (20, 32) if cplx else (12, 16)
            nbytes = per_entry * nnz + per_row * n * k
            for op in ("N", "T"):
                md, t = timed(lambda: T.solve_dev(B.data_ptr(), n, X.data_ptr(), n, k, op, stream), rounds)
                out = {"k": k, "op": op, "solve": t, "sptrsv_bytes": nbytes,
                       "share_of_8TBps": round(nbytes / md / 8e12, 5),
                       "us_per_level": round(md * 1e6 / max(tinf["levels"], 1), 3)}
                if op == "N":
                    ms, ts = timed(lambda: H.spmv_many_dev(B.data_ptr(), n, Y.data_ptr(), n, k, stream=stream), rounds)
                    out.update({"spmv_many_on_the_same_handle": ts, "solve_over_spmv": round(md / ms, 1)})
                    lower = uplo == "lower"
                    Bh = B.cpu().numpy().T
                    Bh = Bh[:, 0] if k == 1 else Bh
                    mh, th = timed(lambda: holder.__setitem__("xh", host_solve(H, lower, unit, Bh)), min(rounds, 2),
                                   warmup=0)
                    diff = (X - holder.pop("xh")).abs().max().item() / max(X.abs().max().item(), 1e-300)
                    out.update({"host_route": th, "host_over_device": round(mh / md, 1),
                                "largest_difference_to_host_relative": diff})
                cell["solves"].append(out)
                print("%s %s k=%d %s: %r" % (name, cell["values"], k, op, out), file=sys.stderr, flush=True)
            del B, X, Y
        T.free()
        H.free()
        torch.cuda.empty_cache()
        return cell

    def sweep(name, make, uplo, settings, rounds):
        """the k = 1, op N solve under other knob settings (read by the analysis)"""
        H = make()
        n = H.info()["nrows_global"]
        B = torch.rand(n, dtype=torch.float64, device="cuda") - 0.5
        X = torch.empty(n, dtype=torch.float64, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        rows = []
        for knobs in settings:
            T = with_knobs(knobs, lambda: H.triangular(uplo))
            inf = T.info()
            md, t = timed(lambda: T.solve_dev(B.data_ptr(), n, X.data_ptr(), n, 1, "N", stream), rounds)
            rows.append({"knobs": knobs or "defaults", "levels": inf["levels"], "launches": inf["launches"], "solve": t,
                         "us_per_level": round(md * 1e6 / max(inf["levels"], 1), 3)})
            print("sweep %s %r: %r" % (name, knobs, rows[-1]), file=sys.stderr, flush=True)
            T.free()
        H.free()
        return {"workload": name, "n": n, "k": 1, "op": "N", "settings": rows}

    for key in KNOBS:
        os.environ.pop(key, None)
    cells = []
    P = DM.synthetic("poisson3d", args.m3)
    L, U = P.tril(), P.triu()
    P.free()
    cells.append(workload("tril(poisson3d(%d))" % args.m3, L, "lower", False, args.rounds))
    cells.append(workload("triu(poisson3d(%d))" % args.m3, U, "upper", False, args.rounds))
    R = DM.synthetic("random", args.n, args.k)
    L0 = R.tril(-1)
    R.free()
    L = L0.scale(0.02)  # the generator's values lie in [0.5, 1.5): the rows' sums stay below 1 and the solution bounded
    L0.free()
    cells.append(workload("tril(random(%d, %d))" % (args.n, args.k), L, "lower", True, args.rounds))
    cells.append(workload("bidiagonal(%d)" % args.chain, chain(args.chain), "lower", False, min(args.rounds, 3)))
    P = DM.synthetic("poisson3d", args.m3)
    L = P.tril()
    P.free()
    Z = L.to_complex()
    L.free()
    ZL = Z.scale(0.6 + 0.8j)
    Z.free()
    cells.append(workload("tril(poisson3d(%d))" % args.m3, ZL, "lower", False, args.rounds))

    def poisson_tril():
        P = DM.synthetic("poisson3d", args.m3)
        L = P.tril()
        P.free()
        return L

    sweeps = [
        sweep("tril(poisson3d(%d))" % args.m3, poisson_tril, "lower",
              [{}] + [{"SPL_TRSV_SMALL_ROWS": s} for s in (1, 16, 32, 64, 128, 256, 1024, 4096, 2 ** 30)], min(args.rounds, 3)),
        sweep("bidiagonal(%d)" % args.sweep_chain, lambda: chain(args.sweep_chain), "lower",
              [{}] + [{"SPL_TRSV_SEGMENT_LEVELS": s} for s in (64, 256, 4096, 65536)] + [{"SPL_TRSV_SMALL_ROWS": 1}],
              min(args.rounds, 3)),
    ]
    line = json.dumps({"what": "tools/bench_trisolve.py: sparse triangular solves on device handles (spl_trisolve_analyze / "
                               "_solve_dev), one MI355X, host clock ending in a synchronise, %d rounds after a warm-up; medians "
                               "with [min, max].  Yardsticks, not the code under test: spl_matrix_spmv_many_dev on the same "
                               "handle, the host route (%s), and the share of 8 TB/s of SURVEY 8d's SpTRSV bytes"
                               % (args.rounds, host_label),
                       "device": torch.cuda.get_device_name(0),
                       "defaults": {"SPL_TRSV_SMALL_ROWS": 64, "SPL_TRSV_SEGMENT_LEVELS": 1024},
                       "cells": cells, "knob_sweeps": sweeps,
                       "note": "analysis = download of the pattern + level pass on the host + permuted copy, per call; the "
                               "first transposed solve (which builds its image) is in the warm-up, not in the figures; "
                               "SMALL_ROWS = 1 makes every level one launch: on the chain that prices the narrow kernel "
                               "per level against a launch per level"})
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
