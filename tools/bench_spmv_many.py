#!/usr/bin/env python3
"""The multi-vector SpMV (spl_matrix_spmv_many_dev, csrc/spmv_many.hip) against what it replaces: k calls of
spl_matrix_spmv_dev on the same handle (for a real handle after optimize(), as Matrix.device_handle() does, so the loop
runs on whatever image that chose; a complex handle has the one native kernel).  Operands stay on the device, times
are HIP events around `reps` calls, the two contenders alternate round by round in this process, and the loop's
round-to-round spread is reported next to the result: `separated` says that the slowest round of the fused call beat
the fastest round of the loop.  Bytes are the model's, one pass over A for all k vectors:
real 12 nnz + 4 (nrows + 1) + 8 k (ncols + nrows), complex 20 nnz + 4 (nrows + 1) + 16 k (ncols + nrows),
divided by each contender's time and given as a share of 8 TB/s.  Prints one JSON line.
python tools/bench_spmv_many.py [--shapes poisson3d:100,poisson3d:200,random:2000000] [--ks 1,4,16,32]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8.0e12  # bytes per second


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="poisson3d:100,poisson3d:200,random:2000000")
    ap.add_argument("--ks", default="1,4,16,32")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=4, help="calls per timed window; rounds * reps >= 20")
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import numpy as np
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    torch.cuda.set_device(0)
    assert args.rounds * args.reps >= 20
    ks = [int(k) for k in args.ks.split(",")]
    kmax = max(ks)
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    rng = np.random.default_rng(1)
    cells = []
    for shape in args.shapes.split(","):
        kind, size = shape.split(":")
        H = pkg.DeviceMatrix.synthetic(kind, int(size), 20)
        inf = H.info()
        nrows, ncols, nnz = inf["nrows_local"], inf["ncols"], inf["nnz"]
        # the complex matrix: the same pattern and real parts, imaginary parts drawn from a seeded stream
        rp, ci, _ = H.export_csr()
        G = pkg.DeviceMatrix.from_csr(nrows, ncols, rp, ci, rng.uniform(0.5, 1.5, nnz))
        Hr, Gz = H.to_complex(), G.to_complex()
        Hz = Hr.lin(1.0, Gz, 1j)
        for h in (G, Hr, Gz):
            h.free()
        del rp, ci
        assert Hz.info()["nnz"] == nnz
        H.optimize()
        for field, h in (("real", H), ("complex", Hz)):
            tdt, entry, per_nz = (torch.float64, 8, 12) if field == "real" else (torch.complex128, 16, 20)
            X = torch.randn((kmax, ncols), generator=gen, device="cuda", dtype=torch.float64).to(tdt)
            if field == "complex":
                X = X + 1j * torch.randn((kmax, ncols), generator=gen, device="cuda", dtype=torch.float64)
            Yf = torch.zeros((kmax, nrows), device="cuda", dtype=tdt)
            Yl = torch.zeros((kmax, nrows), device="cuda", dtype=tdt)
            xp = [X[j].data_ptr() for j in range(kmax)]
            yp = [Yl[j].data_ptr() for j in range(kmax)]

            for k in ks:
                def fused():
                    h.spmv_many_dev(X.data_ptr(), ncols, Yf.data_ptr(), nrows, k, False, s)

                def loop():
                    for j in range(k):
                        h.spmv_dev(xp[j], yp[j], False, s)

                def timed(f):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    for _ in range(args.reps):
                        f()
                    e1.record(stream)
                    e1.synchronize()
                    return e0.elapsed_time(e1) / args.reps

                for _ in range(args.warmup):
                    fused()
                    loop()
                torch.cuda.synchronize()
                tf, tl = [], []
                for _ in range(args.rounds):
                    tf.append(timed(fused))
                    tl.append(timed(loop))
                same = bool(torch.equal(Yf[:k], Yl[:k]))
                model = per_nz * nnz + 4 * (nrows + 1) + entry * k * (ncols + nrows)
                mf, ml = statistics.median(tf), statistics.median(tl)
                cells.append({
                    "matrix": shape, "field": field, "k": k, "nrows": nrows, "nnz": nnz,
                    "spmv_kernel_of_loop": h.spmv_kernel(),
                    "fused_ms": round(mf, 4), "fused_ms_min_max": [round(min(tf), 4), round(max(tf), 4)],
                    "loop_ms": round(ml, 4), "loop_ms_min_max": [round(min(tl), 4), round(max(tl), 4)],
                    "loop_spread_ms": round(max(tl) - min(tl), 4),
                    "speedup": round(ml / mf, 3), "separated": bool(max(tf) < min(tl)),
                    "model_bytes": model,
                    "fused_share_of_8TBps": round(model / (mf * 1e-3) / PEAK, 4),
                    "loop_share_of_8TBps": round(model / (ml * 1e-3) / PEAK, 4),
                    "bit_identical": same})
            del X, Yf, Yl
        H.free()
        Hz.free()
    print(json.dumps({"what": "tools/bench_spmv_many.py: spl_matrix_spmv_many_dev with k vectors against k calls of "
                              "spl_matrix_spmv_dev, one MI355X, HIP events, %d rounds of %d calls alternating"
                              % (args.rounds, args.reps),
                      "device": torch.cuda.get_device_name(0), "cells": cells}), flush=True)


if __name__ == "__main__":
    main()
