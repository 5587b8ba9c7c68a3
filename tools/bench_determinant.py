#!/usr/bin/env python3
"""Cost of the determinant next to one solve with the same factors: the 3-D 7-point Poisson matrix on an m^3 grid
(multifrontal L D L^T), factored once; then one solve of A x = b and repeated spl_umfpack_di_log_determinant calls
(the pivot reduction plus the host bookkeeping of the path; the factors are not speculative, so no check runs).
Grids above 100^3 run only where the device has the memory (as tests/test_gpu_large.py gates config C5).
Prints one JSON line per grid."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NEEDS_GB = {200: 260}  # free HBM a factorisation of the grid needs (200^3: config C5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", default="100,200")
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import numpy as np
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    torch.cuda.set_device(0)
    U = pkg.umfpack
    for m in [int(t) for t in args.grid.split(",")]:
        pkg._ffi.release_cached_memory()
        torch.cuda.empty_cache()
        free, _ = torch.cuda.mem_get_info()
        need = NEEDS_GB.get(m, 0) * 1e9
        if free < need:
            print(json.dumps({"grid": m, "skipped": "needs %.0f GB of free HBM, %.0f GB free" % (need / 1e9, free / 1e9)}))
            continue
        H = pkg.DeviceMatrix.synthetic("poisson3d", m)
        rp, ci, v = H.export_csr()  # symmetric: CSR arrays == CSC arrays
        H.free()
        n = m ** 3
        A = pkg.Matrix(n, n, rp, ci, v)
        fact = U.factor(A, U.analyze(A))
        b = np.ones(n)
        U.linearSolve_(fact, U.UmfpackNormal, A, b)  # warm-up (chain matrices are built by the first solve)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        U.linearSolve_(fact, U.UmfpackNormal, A, b)
        solve_ms = (time.perf_counter() - t0) * 1e3
        U.logDeterminant(fact)  # warm-up
        times = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            sign, logabs = U.logDeterminant(fact)
            times.append((time.perf_counter() - t0) * 1e3)
        det_ms = float(np.median(times))
        print(json.dumps({"grid": m, "n": n, "path": fact.path, "solve_ms": round(solve_ms, 3),
                          "determinant_ms_median": round(det_ms, 4), "determinant_ms_min": round(min(times), 4),
                          "ratio_to_solve": round(det_ms / solve_ms, 5), "sign": sign, "log_abs_det": logabs}),
              flush=True)
        del fact, A


if __name__ == "__main__":
    main()
