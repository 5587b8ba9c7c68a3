#!/usr/bin/env python3
"""The handle-level complex operations against the routes they replace, on the complex shift  ze I - A  of
poisson3d(m) (what FEAST factors at a contour point), device-resident operands, one MI355X:

  H.hermitian()        against  sparse.hermitian(mat) on the host Matrix (two uploads and device transposes of the
                                parts, a download, the comparison in numpy); also the kernel's model bytes
                                4 (n + 1) + 20 nnz over the call's time, as a share of 8 TB/s
  H.ctrans()           against  transpose() of the REAL handle with the same pattern: the ratio (the complex call moves
                                20 instead of 12 bytes per entry, plus the 8-byte position payload)
  A.spgemm(A) complex  against  spl_spgemm_z on host tuples (sparse.mm)

Every shape is warmed up; a time is a host clock around one call that ends in a device synchronise (result handles
are freed outside the window); the new and the existing route alternate round by round in this process, and the
existing route's round-to-round spread stands next to each result.  `meets_bar`: the new route's median is below the
existing one's by more than that spread.  Prints one JSON line (and writes it to --out).
python tools/bench_complex_handles.py [--sizes 100,200] [--spgemm-sizes 100] [--rounds 5] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8.0e12  # bytes per second
ZE = 1.5 + 0.3j


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100,200")
    ap.add_argument("--spgemm-sizes", default=None, help="sizes at which the product is timed too (default: all)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    torch.cuda.set_device(0)
    sizes = [int(s) for s in args.sizes.split(",")]
    mm_sizes = sizes if args.spgemm_sizes is None else [int(s) for s in args.spgemm_sizes.split(",") if s]

    def clock(f):
        """seconds of f() up to the device's idle; f returns what is to be freed afterwards"""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        keep = f()
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        for h in keep if isinstance(keep, (list, tuple)) else [keep]:
            if isinstance(h, pkg.DeviceMatrix):
                h.free()
        return t

    def contest(new, old):
        for _ in range(args.warmup):
            clock(new)
            clock(old)
        tn, to = [], []
        for _ in range(args.rounds):
            tn.append(clock(new))
            to.append(clock(old))
        mn, mo = statistics.median(tn), statistics.median(to)
        spread = max(to) - min(to)
        return {"new_ms": round(mn * 1e3, 4), "new_ms_min_max": [round(min(tn) * 1e3, 4), round(max(tn) * 1e3, 4)],
                "existing_ms": round(mo * 1e3, 4),
                "existing_ms_min_max": [round(min(to) * 1e3, 4), round(max(to) * 1e3, 4)],
                "existing_spread_ms": round(spread * 1e3, 4), "existing_over_new": round(mo / mn, 3),
                "meets_bar": bool(mo - mn > spread)}, mn

    cells = []
    for m in sizes:
        Hr = pkg.DeviceMatrix.synthetic("poisson3d", m)
        inf = Hr.info()
        n, nnz = inf["nrows_local"], inf["nnz"]
        rp, ci, v = Hr.export_csr()
        rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
        z = -v.astype(np.complex128)
        z[ci == rows] += ZE                      # ze I - A; the matrix is symmetric: its CSR arrays are its CSC arrays
        del rows
        mat = pkg.Matrix(n, n, rp, ci.astype(np.int64), z)
        Hz = pkg.DeviceMatrix.from_csc_complex(mat)
        assert Hz.info()["nnz"] == nnz
        cell = {"matrix": "ze I - poisson3d(%d)" % m, "n": n, "nnz": nnz}

        verdicts = []
        r, tnew = contest(lambda: verdicts.append(Hz.hermitian()), lambda: verdicts.append(pkg.hermitian(mat)))
        model = 4 * (n + 1) + 20 * nnz
        r.update({"verdicts_agree": len(set(verdicts)) == 1, "verdict": bool(verdicts[0]), "model_bytes": model,
                  "model_share_of_8TBps": round(model / tnew / PEAK, 4)})
        cell["hermitian"] = r

        r, _ = contest(lambda: Hz.ctrans(), lambda: Hr.transpose())
        r["new_over_existing"] = round(r["new_ms"] / r["existing_ms"], 3)
        cell["ctrans_vs_real_transpose"] = r

        if m in mm_sizes:
            counts = []

            def new_mm():
                P, _ = Hz.spgemm(Hz)
                counts.append(P.info()["nnz"])
                return P

            def old_mm():
                counts.append(len(pkg.mm(mat, mat).indices))

            r, _ = contest(new_mm, old_mm)
            r.update({"nnz_of_product": counts[0], "nnz_agree": len(set(counts)) == 1})
            cell["spgemm_vs_spl_spgemm_z"] = r
        cells.append(cell)
        Hr.free()
        Hz.free()
        del mat, rp, ci, v, z
    line = json.dumps({"what": "tools/bench_complex_handles.py: handle-level hermitian / ctrans / complex spgemm against "
                               "the existing routes, one MI355X, host clock ending in a synchronise, %d rounds alternating"
                               % args.rounds,
                       "device": torch.cuda.get_device_name(0), "cells": cells})
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
