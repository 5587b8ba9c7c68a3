#!/usr/bin/env python3
"""Cost of a condition estimate next to the solves it is made of: the 3-D 7-point Poisson matrix on an m^3 grid (real,
multifrontal L D L^T) and the shifted complex operator (3 + 0.5i) I - A on the same grid, each factored once; then one
single-column solve, one 2-column batched device solve and repeated conditionEstimate calls with t = 2 (seconds,
median).  Prints one JSON line per workload with the iterations, the batched solve calls and the estimate."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_seconds(fn, reps):
    import numpy as np
    import torch
    fn()  # warm-up (the chain matrices of each direction are built by its first solve)
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--workloads", default="real,complex")
    args = ap.parse_args()
    import numpy as np
    import scipy.sparse as sp
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    torch.cuda.set_device(0)
    U = pkg.umfpack
    m = args.grid
    n = m ** 3
    H = pkg.DeviceMatrix.synthetic("poisson3d", m)
    rp, ci, v = H.export_csr()  # symmetric: CSR arrays == CSC arrays
    H.free()
    for kind in args.workloads.split(","):
        if kind == "real":
            A = pkg.Matrix(n, n, rp, ci, v)
            dt = torch.float64
        else:
            S = (3.0 + 0.5j) * sp.identity(n, format="csc") - sp.csc_matrix((v, ci, rp), shape=(n, n)).astype(np.complex128)
            S.sort_indices()
            A = pkg.Matrix(n, n, S.indptr, S.indices, S.data)
            dt = torch.complex128
        fact = U.factor(A, U.analyze(A))
        b = np.ones(n, dtype=np.complex128 if kind != "real" else np.float64)
        B2 = torch.ones((2, n), dtype=dt, device="cuda")
        solve_s = median_seconds(lambda: U.linearSolve_(fact, U.UmfpackNormal, A, b), args.reps)
        solve2_s = median_seconds(lambda: U.linearSolveManyDevice_(fact, U.UmfpackNormal, A, B2), args.reps)
        r = {}

        def estimate():
            r.update(U.conditionEstimate(fact, A, norm=1, t=2))
        cond_s = median_seconds(estimate, args.reps)
        print(json.dumps({"workload": "%s %d^3" % (kind, m), "n": n, "path": fact.path, "condest_s": round(cond_s, 5),
                          "solve_1col_s": round(solve_s, 5), "solve_2col_dev_s": round(solve2_s, 5),
                          "iterations": r["iterations"], "solve_calls": r["solves"], "cond_1": r["cond"],
                          "norm_A": r["norm_A"], "norm_inv": r["norm_inv"]}), flush=True)
        del fact, A


if __name__ == "__main__":
    main()
