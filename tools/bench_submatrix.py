#!/usr/bin/env python3
"""Taking a device handle apart on the device against the host route, one MI355X.

  poisson3d(m)      m = 200: 8.0e6 rows, 5.6e7 entries
  random(n, K)      n = 1e6, K = 20: 2.0e7 entries

  (a) window        the middle half of the rows and of the columns: H.submatrix(n/4, n/4, n/2, n/2)
  (b) row block     the middle half of the rows, all columns: H.select(rows, None) with rows = n/4 .. 3n/4 on the device
  (c) permutation   a random symmetric permutation: H.select(p, p), p on the device

  device route   the handle call alone (spl_matrix_submatrix / spl_matrix_select): nothing crosses PCIe
  host route     what the library offered before: export_csr to the host, the same cut in numpy, from_csr

and, for (a) and (b), a device-to-device hipMemcpy of the bytes the RESULT occupies — 8 (nr + 1) of pointers and 12 nnz
of indices and values — as the bound a cut that only had to move its result could reach.  The call time is a CALL time:
allocation of the result's arrays, the kernels, the read-back of nnz and the pass that finishes a handle.

Every shape is warmed up; a time is a host clock around one route that ends in a device synchronise (handles are freed
outside the window); the routes alternate round by round in this process.  The two routes' results are compared bit for
bit once per cell.  Nothing is asserted about the ratio: it is recorded.  Prints one JSON line (and writes it to --out).
python tools/bench_submatrix.py [--m3 200] [--n 1000000] [--k 20] [--rounds 5] [--host-rounds 3] [--warmup 1] [--out FILE]"""
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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-rounds", type=int, default=3)
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
        """seconds of f() up to the device's idle; the handle f returns is freed afterwards"""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h = f()
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        if isinstance(h, DM):
            h.free()
        return t

    def spread(ts):
        return [round(min(ts) * 1e3, 3), round(max(ts) * 1e3, 3)]

    # the same cuts in numpy on exported CSR arrays (ascending columns inside every row)
    def host_window(rp, ci, v, r0, c0, nr, nc, ncols):
        a, b = int(rp[r0]), int(rp[r0 + nr])
        ci, v = ci[a:b], v[a:b]
        keep = (ci >= c0) & (ci < c0 + nc)
        rows = np.repeat(np.arange(nr, dtype=np.int64), np.diff(rp[r0:r0 + nr + 1]))
        out = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=nr))])
        return nr, nc, out, ci[keep] - c0, v[keep]

    def host_rows(rp, ci, v, r0, nr, ncols):
        a, b = int(rp[r0]), int(rp[r0 + nr])
        return nr, ncols, rp[r0:r0 + nr + 1] - a, ci[a:b], v[a:b]

    def host_permutation(rp, ci, v, p, ncols):
        n = len(p)
        inv = np.empty(n, dtype=np.int64)
        inv[p] = np.arange(n)
        lens = np.diff(rp)[p]
        out = np.concatenate([[0], np.cumsum(lens)])
        src = np.repeat(rp[p] - out[:-1], lens) + np.arange(int(out[-1]), dtype=np.int64)
        key = np.repeat(np.arange(n, dtype=np.int64), lens) * n + inv[ci[src]]
        order = np.argsort(key, kind="stable")
        return n, n, out, (key[order] % n), v[src][order]

    def host_route(H, cut):
        rp, ci, v = H.export_csr()
        nr, nc, rp2, ci2, v2 = cut(rp, ci, v)
        return DM.from_csr(nr, nc, rp2, ci2, v2)

    def same(Ha, Hb):
        a, b = Ha.export_csr(), Hb.export_csr()
        return bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
                    and np.array_equal(a[2].view(np.uint64), b[2].view(np.uint64)))

    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.restype = ctypes.c_int
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]

    cells = []
    for name, make in (("poisson3d(%d)" % args.m3, lambda: DM.synthetic("poisson3d", args.m3)),
                       ("random(%d, %d)" % (args.n, args.k), lambda: DM.synthetic("random", args.n, args.k))):
        H = make()
        inf = H.info()
        n, ncols, nnz = inf["nrows_global"], inf["ncols"], inf["nnz"]
        q, h = n // 4, n // 2
        rows_dev = torch.arange(q, q + h, dtype=torch.int32, device="cuda")
        p_host = np.random.default_rng(n).permutation(n)
        p_dev = torch.from_numpy(p_host.astype(np.int32)).cuda()
        cases = (
            ("window_middle_half", lambda: H.submatrix(q, q, h, h),
             lambda rp, ci, v: host_window(rp, ci, v, q, q, h, h, ncols), True),
            ("row_block_all_columns", lambda: H.select(rows_dev, None),
             lambda rp, ci, v: host_rows(rp, ci, v, q, h, ncols), True),
            ("symmetric_permutation", lambda: H.select(p_dev, p_dev),
             lambda rp, ci, v: host_permutation(rp, ci, v, p_host, ncols), False),
        )
        cell = {"matrix": name, "n": n, "nnz": nnz, "cases": []}
        for label, device_route, cut, with_copy in cases:
            # both routes once: the first warm-up, and the check that they give the same matrix
            Hd, Hh = device_route(), host_route(H, cut)
            out = {"case": label, "result_nnz": Hd.info()["nnz"], "routes_agree_bit_for_bit": same(Hd, Hh)}
            result_bytes = 8 * (Hd.info()["nrows_global"] + 1) + 12 * Hd.info()["nnz"]
            Hd.free()
            Hh.free()
            for _ in range(args.warmup):
                clock(device_route)
            td, th = [], []
            for r in range(args.rounds):
                td.append(clock(device_route))
                if r < args.host_rounds:
                    th.append(clock(lambda: host_route(H, cut)))
            md, mh = statistics.median(td), statistics.median(th)
            out.update({"device_ms": round(md * 1e3, 3), "device_ms_min_max": spread(td),
                        "host_ms": round(mh * 1e3, 3), "host_ms_min_max": spread(th),
                        "host_over_device": round(mh / md, 1), "result_bytes": result_bytes,
                        "device_GBps_of_result": round(result_bytes / md / 1e9, 1)})
            if with_copy:
                a = torch.empty(result_bytes, dtype=torch.uint8, device="cuda")
                b = torch.empty(result_bytes, dtype=torch.uint8, device="cuda")
                a.zero_()

                def copy():
                    st = hip.hipMemcpy(b.data_ptr(), a.data_ptr(), result_bytes, 3)  # hipMemcpyDeviceToDevice
                    assert st == 0, st

                for _ in range(args.warmup + 1):
                    clock(copy)
                tc = []
                for _ in range(args.rounds):
                    tc.append(clock(copy))
                mc = statistics.median(tc)
                out.update({"memcpy_d2d_ms": round(mc * 1e3, 3), "memcpy_d2d_ms_min_max": spread(tc),
                            "call_over_copy": round(md / mc, 2)})
                del a, b
            cell["cases"].append(out)
            print("%s %s: %r" % (name, label, out), file=sys.stderr, flush=True)
        H.free()
        del rows_dev, p_dev
        torch.cuda.empty_cache()
        cells.append(cell)

    line = json.dumps({"what": "tools/bench_submatrix.py: a window, a row block and a symmetric permutation of a device handle "
                               "(spl_matrix_submatrix / spl_matrix_select) against the host route (export_csr, numpy, "
                               "from_csr), one MI355X, host clock ending in a synchronise, %d device rounds and %d host "
                               "rounds alternating after %d warm-up" % (args.rounds, args.host_rounds, args.warmup + 1),
                       "device": torch.cuda.get_device_name(0), "cells": cells,
                       "note": "call times: allocation + kernels + read-backs + the pass that finishes a handle; the copy "
                               "moves the bytes the result occupies, 8 (nr + 1) + 12 nnz"})
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
