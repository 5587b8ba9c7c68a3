#!/usr/bin/env python3
"""A sparse torch tensor on the GPU into a handle and back, by the device route against the host route, one MI355X.

  poisson3d(m)      m = 200: 8.0e6 rows, 5.6e7 entries
  random(n, K)      n = 1e6, K = 20: 2.0e7 entries

Both come from the synthetic constructors and are exported once to torch.sparse_csr tensors with int64 indices.

  device route   DeviceMatrix.from_torch(t), then H.to_torch(): check-and-narrow, copies and widening on the device
                 (spl_matrix_create_csr_dev, spl_matrix_export_csr_dev); nothing crosses PCIe
  host route     what the library offered before: the three arrays to the host with .cpu(), the indices narrowed there,
                 DeviceMatrix.from_csr, export_csr, and the tensors rebuilt with .cuda()

and the import call's moved bytes per second — pointers read and written as 8 bytes, indices read as 8 and written as 4,
values read and written as 8: 16 (n + 1) + 28 nnz — next to a device-to-device hipMemcpy that moves as many bytes (half of
them read, half written) in this process.  The call time is a CALL time: allocation of the handle's arrays, the
kernels, the read-backs between them and the pass that finishes a handle.

Every shape is warmed up; a time is a host clock around one route that ends in a device synchronise (handles are freed
outside the window); the two routes alternate round by round in this process.  `meets_bar`: the device route's median
is below the host route's by more than the host route's own min-max spread.  Prints one JSON line (and writes it to
--out).
python tools/bench_device_arrays.py [--m3 200] [--n 1000000] [--k 20] [--rounds 7] [--warmup 1] [--out FILE]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m3", type=int, default=200)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
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
        """seconds of f() up to the device's idle; the handles f returns are freed afterwards"""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        keep = f()
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        for h in keep:
            if isinstance(h, DM):
                h.free()
        return t

    def device_route(t):
        H = DM.from_torch(t)
        return H, H.to_torch()

    def host_route(t):
        n, nc = t.shape
        rp = t.crow_indices().cpu().numpy().astype(np.int32)
        ci = t.col_indices().cpu().numpy().astype(np.int32)
        v = t.values().cpu().numpy()
        H = DM.from_csr(n, nc, rp, ci, v)
        rp2, ci2, v2 = H.export_csr()
        back = torch.sparse_csr_tensor(torch.from_numpy(rp2).cuda(), torch.from_numpy(ci2.astype(np.int64)).cuda(),
                                       torch.from_numpy(v2).cuda(), size=(n, nc))
        return H, back

    def spread(ts):
        return [round(min(ts) * 1e3, 3), round(max(ts) * 1e3, 3)]

    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.restype = ctypes.c_int
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]

    cells = []
    for name, make in (("poisson3d(%d)" % args.m3, lambda: DM.synthetic("poisson3d", args.m3)),
                       ("random(%d, %d)" % (args.n, args.k), lambda: DM.synthetic("random", args.n, args.k))):
        src = make()
        t = src.to_torch()  # int64 indices
        src.free()
        n, nnz = int(t.shape[0]), int(t.values().shape[0])
        # both routes once: the first warm-up, and the check that they give the same tensor
        (Hd, td), (Hh, th) = device_route(t), host_route(t)
        same = bool(torch.equal(td.crow_indices(), th.crow_indices()) and torch.equal(td.col_indices(), th.col_indices())
                    and torch.equal(td.values().clone().view(torch.int64), th.values().clone().view(torch.int64))
                    and torch.equal(td.col_indices(), t.col_indices()))
        Hd.free()
        Hh.free()
        del td, th
        for _ in range(args.warmup):
            clock(lambda: device_route(t))
            clock(lambda: host_route(t))
        tn, to = [], []
        for _ in range(args.rounds):
            tn.append(clock(lambda: device_route(t)))
            to.append(clock(lambda: host_route(t)))
        mn, mo = statistics.median(tn), statistics.median(to)
        cell = {"matrix": name, "n": n, "nnz": nnz, "routes_agree_bit_for_bit": same,
                "device_ms": round(mn * 1e3, 3), "device_ms_min_max": spread(tn),
                "host_ms": round(mo * 1e3, 3), "host_ms_min_max": spread(to),
                "host_spread_ms": round((max(to) - min(to)) * 1e3, 3), "host_over_device": round(mo / mn, 2),
                "meets_bar": bool(mo - mn > max(to) - min(to))}
        # the import alone next to a device-to-device copy that moves as many bytes
        moved = 16 * (n + 1) + 28 * nnz
        a = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
        b = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
        a.zero_()

        def copy():
            st = hip.hipMemcpy(b.data_ptr(), a.data_ptr(), moved // 2, 3)  # hipMemcpyDeviceToDevice
            assert st == 0, st
            return ()

        for _ in range(args.warmup + 1):
            clock(lambda: (DM.from_torch(t),))
            clock(copy)
        ti, tc = [], []
        for _ in range(args.rounds):
            ti.append(clock(lambda: (DM.from_torch(t),)))
            tc.append(clock(copy))
        mi, mc = statistics.median(ti), statistics.median(tc)
        cell["import"] = {"moved_bytes": moved, "from_torch_call_ms": round(mi * 1e3, 3), "from_torch_call_ms_min_max": spread(ti),
                          "from_torch_call_GBps_moved": round(moved / mi / 1e9, 1),
                          "memcpy_d2d_ms": round(mc * 1e3, 3), "memcpy_d2d_ms_min_max": spread(tc),
                          "memcpy_d2d_GBps_moved": round(moved / mc / 1e9, 1), "call_share_of_copy_rate": round(mc / mi, 3)}
        del a, b, t
        torch.cuda.empty_cache()
        cells.append(cell)

    line = json.dumps({"what": "tools/bench_device_arrays.py: torch.sparse_csr tensor (int64 indices) -> handle -> tensor on the "
                               "device against the host route (.cpu(), narrow, from_csr, export_csr, .cuda()), one MI355X, "
                               "host clock ending in a synchronise, %d rounds alternating after %d warm-up"
                               % (args.rounds, args.warmup + 1),
                       "device": torch.cuda.get_device_name(0), "cells": cells,
                       "note": "call times: allocation + kernels + read-backs + the pass that finishes a handle"})
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
