#!/usr/bin/env python3
"""Assembling the model problems on device handles against the host-tuple route, one MI355X.

  laplacian2d(m) = kron(I, T) + kron(T, I)                                   (m = 3000: 9.0e6 rows, 4.5e7 entries)
  laplacian3d(m) = kron(I2, T) + kron(kron(I, T), I) + kron(T, I2), I2 = ident(m^2)   (m = 200: 8.0e6 rows, 5.6e7 entries)

  handle route   DeviceMatrix.ident, DeviceMatrix.kronecker, DeviceMatrix.lin: T is uploaded (3m - 2 entries), nothing
                 else crosses PCIe, the result is a handle
  host route     sparse.kronecker, sparse.lin on host Matrix values (every call uploads its operands and downloads its
                 result), then DeviceMatrix.from_csc of the sum: the same handle by the route the library had before

and the Kronecker call's written bytes per second — 8 (nrows + 1) + (4 + 8) nnz over the time of
`ident(m^2).kronecker(T)` — next to a device-to-device hipMemcpy of the same byte count in this process.  The call
time is a CALL time: it holds the allocation of the result, the kernel and the pass that finishes a handle (int32
pointers, longest row); the kernel alone is what `--kron-only N` under `rocprofv3 --kernel-trace --stats` shows.

Every shape is warmed up; a time is a host clock around one route that ends in a device synchronise (handles are
freed outside the window); the two routes alternate round by round in this process.  `meets_bar`: the handle route's
median is below the host route's by more than the host route's own min-max spread.  Prints one JSON line (and writes
it to --out).
python tools/bench_handle_assembly.py [--m2 3000] [--m3 200] [--rounds 7] [--warmup 1] [--out FILE] [--kron-only N]"""
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
    ap.add_argument("--m2", type=int, default=3000)
    ap.add_argument("--m3", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kron-only", type=int, default=0,
                    help="only run ident(m3^2).kronecker(T) this many times (for a kernel trace) and exit")
    args = ap.parse_args()
    import numpy as np
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    torch.cuda.set_device(0)
    DM = pkg.DeviceMatrix

    def tridiag(m):
        ptr = np.concatenate([[0], np.cumsum(np.r_[2, np.full(m - 2, 3), 2])]).astype(np.int64)
        idx = np.concatenate([np.arange(max(c - 1, 0), min(c + 2, m)) for c in range(m)]).astype(np.int64)
        cols = np.repeat(np.arange(m), np.diff(ptr))
        return pkg.Matrix(m, m, ptr, idx, np.where(idx == cols, 2.0, -1.0))

    def free(hs):
        for h in hs if isinstance(hs, (list, tuple)) else [hs]:
            if isinstance(h, DM):
                h.free()

    def clock(f):
        """seconds of f() up to the device's idle; what f returns is freed afterwards"""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        keep = f()
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        free(keep)
        return t

    def dev2(m, T):
        HT, I = DM.from_csc(T), DM.ident(m)
        a, b = I.kronecker(HT), HT.kronecker(I)
        out = a.lin(1, b, 1)
        free([HT, I, a, b])
        return out

    def host2(m, T):
        I = pkg.ident(m)
        return DM.from_csc(pkg.lin(1.0, pkg.kronecker(I, T), 1.0, pkg.kronecker(T, I)))

    def dev3(m, T):
        HT, I, I2 = DM.from_csc(T), DM.ident(m), DM.ident(m * m)
        a, it, c = I2.kronecker(HT), I.kronecker(HT), HT.kronecker(I2)
        b = it.kronecker(I)
        ab = a.lin(1, b, 1)
        out = ab.lin(1, c, 1)
        free([HT, I, I2, a, it, b, c, ab])
        return out

    def host3(m, T):
        I, I2 = pkg.ident(m), pkg.ident(m * m)
        a, b, c = pkg.kronecker(I2, T), pkg.kronecker(pkg.kronecker(I, T), I), pkg.kronecker(T, I2)
        return DM.from_csc(pkg.lin(1.0, pkg.lin(1.0, a, 1.0, b), 1.0, c))

    if args.kron_only:
        HT, I2 = DM.from_csc(tridiag(args.m3)), DM.ident(args.m3 ** 2)
        for _ in range(args.kron_only):
            free(I2.kronecker(HT))
        torch.cuda.synchronize()
        return

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
        return {"handle_ms": round(mn * 1e3, 3), "handle_ms_min_max": [round(min(tn) * 1e3, 3), round(max(tn) * 1e3, 3)],
                "host_ms": round(mo * 1e3, 3), "host_ms_min_max": [round(min(to) * 1e3, 3), round(max(to) * 1e3, 3)],
                "host_spread_ms": round(spread * 1e3, 3), "host_over_handle": round(mo / mn, 2),
                "meets_bar": bool(mo - mn > spread)}

    cells = []
    for name, m, dev, host in (("laplacian2d", args.m2, dev2, host2), ("laplacian3d", args.m3, dev3, host3)):
        T = tridiag(m)
        probe_d, probe_h = dev(m, T), host(m, T)  # also the first warm-up: code objects, pools
        inf_d, inf_h = probe_d.info(), probe_h.info()
        same = False
        if inf_d["nnz"] == inf_h["nnz"] and inf_d["nrows_global"] == inf_h["nrows_global"]:
            d, h = probe_d.export_csr(), probe_h.export_csr()
            same = all(np.array_equal(x.view(np.uint64) if x.dtype == np.float64 else x,
                                      y.view(np.uint64) if y.dtype == np.float64 else y) for x, y in zip(d, h))
            del d, h
        free([probe_d, probe_h])
        cell = {"matrix": "%s(%d)" % (name, m), "n": inf_d["nrows_global"], "nnz": inf_d["nnz"],
                "routes_agree_bit_for_bit": bool(same)}
        cell.update(contest(lambda: dev(m, T), lambda: host(m, T)))
        cells.append(cell)

    # the Kronecker call's store stream next to a device-to-device copy of as many bytes
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.restype = ctypes.c_int
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    m = args.m3
    HT, I2 = DM.from_csc(tridiag(m)), DM.ident(m * m)
    probe = I2.kronecker(HT)
    inf = probe.info()
    free(probe)
    nbytes = 8 * (inf["nrows_global"] + 1) + 12 * inf["nnz"]
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    src.zero_()

    def copy():
        st = hip.hipMemcpy(dst.data_ptr(), src.data_ptr(), nbytes, 3)  # hipMemcpyDeviceToDevice
        assert st == 0, st

    for _ in range(args.warmup + 1):
        clock(lambda: I2.kronecker(HT))
        clock(copy)
    tk, tc = [], []
    for _ in range(args.rounds):
        tk.append(clock(lambda: I2.kronecker(HT)))
        tc.append(clock(copy))
    mk, mc = statistics.median(tk), statistics.median(tc)
    stream = {"product": "ident(%d) (x) tridiag(%d)" % (m * m, m), "nrows": inf["nrows_global"], "nnz": inf["nnz"],
              "written_bytes": nbytes,
              "kronecker_call_ms": round(mk * 1e3, 3), "kronecker_call_ms_min_max": [round(min(tk) * 1e3, 3), round(max(tk) * 1e3, 3)],
              "kronecker_call_GBps": round(nbytes / mk / 1e9, 1),
              "memcpy_d2d_ms": round(mc * 1e3, 3), "memcpy_d2d_ms_min_max": [round(min(tc) * 1e3, 3), round(max(tc) * 1e3, 3)],
              "memcpy_d2d_GBps_written": round(nbytes / mc / 1e9, 1),
              "call_share_of_copy_rate": round(mc / mk, 3),
              "note": "call time: result allocation + kernel + the pass that finishes a handle, not the kernel alone"}
    line = json.dumps({"what": "tools/bench_handle_assembly.py: model problems assembled handle to handle against the "
                               "host-tuple route (kronecker, lin, from_csc), one MI355X, host clock ending in a "
                               "synchronise, %d rounds alternating after %d warm-up" % (args.rounds, args.warmup + 1),
                       "device": torch.cuda.get_device_name(0), "cells": cells, "kronecker_store_stream": stream})
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
