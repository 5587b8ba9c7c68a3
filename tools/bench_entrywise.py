#!/usr/bin/env python3
"""The entry-wise layer on device handles against the host route, one MI355X.

  poisson3d(m)      m = 200: 8.0e6 rows, 5.6e7 entries
  random(n, K)      n = 1e6, K = 20: 2.0e7 entries
  each real, and complex (the real handle promoted and multiplied by 0.6 + 0.8i on the device)

  maps              negate, abs (the magnitude on complex handles), scale
  scaling           diag(r) A diag(c), r and c on the device
  filters           drop_small(tol) (about the off-diagonal part of poisson3d, half of random), tril(0)
  reductions        abs_sums per row and per column, abs_max per column, the Frobenius norm and the 1-norm

  device route   the handle call alone: nothing crosses PCIe
  host route     what the library offered before: export_csr to the host, the same step in numpy, and for the calls that
                 give a matrix the upload of the result (from_csr, or the device-array import for complex values)

and, for the calls that give a matrix, a device-to-device hipMemcpy of the bytes the RESULT occupies — 8 (nr + 1) of
pointers and 12 (real) or 20 (complex) nnz of indices and values — as the bound a call that only had to move its result
could reach.  The column sums are the row sums of the order-preserving transpose of the moduli (no floating-point atomic
add): `abs_sums_cols` beside `abs_sums_rows` is what that fixed order costs.  A call time is a CALL time: allocation of
the result's arrays, the kernels, the read-back of nnz and the pass that finishes a handle.

Every case is warmed up; a time is a host clock around one route that ends in a device synchronise (handles are freed
outside the window).  The two routes' results are compared once per case: matrices bit for bit, sums to 1e-12 relative.
Nothing is asserted about a ratio: it is recorded.  Prints one JSON line (and writes it to --out).
python tools/bench_entrywise.py [--m3 200] [--n 1000000] [--k 20] [--rounds 5] [--host-rounds 2] [--warmup 1] [--out FILE]"""
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
    ap.add_argument("--host-rounds", type=int, default=2)
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

    def upload(nr, nc, rp, ci, v):
        if v.dtype != np.complex128:
            return DM.from_csr(nr, nc, rp, ci, v)
        drp, dci, dv = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (rp.astype(np.int64), ci.astype(np.int64), v))
        torch.cuda.synchronize()
        return DM.from_csr_dev(nr, nc, drp.data_ptr(), dci.data_ptr(), dv.data_ptr(), index_width=8, complex=True)

    def rows_of(rp):
        return np.repeat(np.arange(len(rp) - 1, dtype=np.int64), np.diff(rp))

    def keep_entries(rp, ci, v, keep):
        out = np.concatenate([[0], np.cumsum(np.bincount(rows_of(rp)[keep], minlength=len(rp) - 1))])
        return out, ci[keep], v[keep]

    def same_matrix(Ha, Hb):
        a, b = Ha.export_csr(), Hb.export_csr()
        return bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
                    and np.array_equal(np.ascontiguousarray(a[2]).view(np.uint64), np.ascontiguousarray(b[2]).view(np.uint64)))

    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.restype = ctypes.c_int
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]

    cells = []
    for name, make in (("poisson3d(%d)" % args.m3, lambda: DM.synthetic("poisson3d", args.m3)),
                       ("random(%d, %d)" % (args.n, args.k), lambda: DM.synthetic("random", args.n, args.k))):
        for kind in ("real", "complex"):
            H = make()
            if kind == "complex":
                R = H
                H = R.to_complex().scale(0.6 + 0.8j)
                R.free()
            inf = H.info()
            n, ncols, nnz = inf["nrows_global"], inf["ncols"], inf["nnz"]
            vb = 16 if kind == "complex" else 8
            rng = np.random.default_rng(n)
            r_host, c_host = rng.uniform(0.5, 2.0, n), rng.uniform(0.5, 2.0, ncols)
            r_dev, c_dev = torch.from_numpy(r_host).cuda(), torch.from_numpy(c_host).cuda()
            if kind == "complex":  # packed pairs, as the call takes them: the promotion is not part of the timed call
                r_dev, c_dev = r_dev.to(torch.complex128), c_dev.to(torch.complex128)
            tol = 1.0 if name.startswith("poisson") else float(torch.median(H.abs_max(1)).item()) / 2
            s = 2.5

            def host_matrix(step):
                rp, ci, v = H.export_csr()
                rp2, ci2, v2 = step(rp, ci, v)
                return upload(n, ncols, rp2, ci2, v2)

            def host_vector(step):
                rp, ci, v = H.export_csr()
                return step(rp, ci, v)

            def col_sums(rp, ci, v):
                return np.bincount(ci, weights=np.abs(v), minlength=ncols)

            def col_max(rp, ci, v):
                order = np.argsort(ci, kind="stable")  # the columns' entries one behind the other
                cp = np.concatenate([[0], np.cumsum(np.bincount(ci, minlength=ncols))])
                m = np.abs(v)[order]
                out = np.zeros(ncols)
                full = np.diff(cp) > 0
                out[full] = np.maximum.reduceat(m, cp[:-1][full])
                return out

            matrix_cases = (
                ("negate", lambda: H.negate(), lambda rp, ci, v: (rp, ci, -v)),
                ("abs", lambda: H.abs(), lambda rp, ci, v: (rp, ci, np.abs(v) + (0j if kind == "complex" else 0.0))),
                ("scale", lambda: H.scale(s), lambda rp, ci, v: (rp, ci, v * s)),
                ("scale_rows_cols", lambda: H.scale_rows_cols(r_dev, c_dev),
                 lambda rp, ci, v: (rp, ci, (r_host[rows_of(rp)] * v) * c_host[ci])),
                ("drop_small", lambda: H.drop_small(tol), lambda rp, ci, v: keep_entries(rp, ci, v, ~(np.abs(v) <= tol))),
                ("tril", lambda: H.tril(0), lambda rp, ci, v: keep_entries(rp, ci, v, ci <= rows_of(rp))),
            )
            vector_cases = (
                ("abs_sums_rows", lambda: H.abs_sums(1), lambda rp, ci, v: np.add.reduceat(np.abs(v), rp[:-1])),
                ("abs_sums_cols", lambda: H.abs_sums(0), col_sums),
                ("abs_max_cols", lambda: H.abs_max(0), col_max),
                ("norm_fro", lambda: H.norm("fro"), lambda rp, ci, v: float(np.linalg.norm(v))),
                ("norm_one", lambda: H.norm(1), lambda rp, ci, v: float(col_sums(rp, ci, v).max())),
            )
            cell = {"matrix": name, "values": kind, "n": n, "nnz": nnz, "cases": []}

            def timed(device_route, host_route):
                for _ in range(args.warmup):
                    clock(device_route)
                td, th = [], []
                for r in range(args.rounds):
                    td.append(clock(device_route))
                    if r < args.host_rounds:
                        th.append(clock(host_route))
                md, mh = statistics.median(td), statistics.median(th)
                return md, {"device_ms": round(md * 1e3, 3), "device_ms_min_max": spread(td),
                            "host_ms": round(mh * 1e3, 3), "host_ms_min_max": spread(th),
                            "host_over_device": round(mh / md, 1)}

            for label, device_route, step in matrix_cases:
                Hd, Hh = device_route(), host_matrix(step)
                # abs and scale of complex values: numpy's hypot and its own product order differ in the last bit
                out = {"case": label, "result_nnz": Hd.info()["nnz"], "routes_agree_bit_for_bit": same_matrix(Hd, Hh)}
                rb = 8 * (n + 1) + (4 + (16 if Hd.is_complex else 8)) * Hd.info()["nnz"]
                Hd.free()
                Hh.free()
                md, times = timed(device_route, lambda: host_matrix(step))
                out.update(times)
                out.update({"result_bytes": rb, "device_GBps_of_result": round(rb / md / 1e9, 1)})
                a = torch.empty(rb, dtype=torch.uint8, device="cuda")
                b = torch.empty(rb, dtype=torch.uint8, device="cuda")
                a.zero_()

                def copy():
                    st = hip.hipMemcpy(b.data_ptr(), a.data_ptr(), rb, 3)  # hipMemcpyDeviceToDevice
                    assert st == 0, st

                for _ in range(args.warmup + 1):
                    clock(copy)
                tc = [clock(copy) for _ in range(args.rounds)]
                mc = statistics.median(tc)
                out.update({"memcpy_d2d_ms": round(mc * 1e3, 3), "memcpy_d2d_ms_min_max": spread(tc),
                            "call_over_copy": round(md / mc, 2)})
                del a, b
                cell["cases"].append(out)
                print("%s %s %s: %r" % (name, kind, label, out), file=sys.stderr, flush=True)

            for label, device_route, step in vector_cases:
                got, want = device_route(), host_vector(step)
                got = got.cpu().numpy() if hasattr(got, "cpu") else got
                err = float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300)))
                out = {"case": label, "routes_agree_to_1e-12": bool(err <= 1e-12), "largest_relative_difference": err}
                md, times = timed(device_route, lambda: host_vector(step))
                out.update(times)
                read = (4 + vb) * nnz + 8 * (n + 1)
                out.update({"bytes_read_once": read, "device_GBps_of_input": round(read / md / 1e9, 1)})
                cell["cases"].append(out)
                print("%s %s %s: %r" % (name, kind, label, out), file=sys.stderr, flush=True)
            H.free()
            del r_dev, c_dev
            torch.cuda.empty_cache()
            cells.append(cell)

    line = json.dumps({"what": "tools/bench_entrywise.py: maps, scaling, filters and reductions of a device handle "
                               "(spl_matrix_map / _scale_rows_cols / _filter / _band / _reduce_dev / _norm) against the host "
                               "route (export_csr, numpy, upload), one MI355X, host clock ending in a synchronise, %d device "
                               "rounds and %d host rounds after %d warm-up; medians, with [min, max]"
                               % (args.rounds, args.host_rounds, args.warmup + 1),
                       "device": torch.cuda.get_device_name(0), "cells": cells,
                       "note": "call times: allocation + kernels + read-backs + the pass that finishes a handle; the copy "
                               "moves the bytes the result occupies; abs_sums_cols and norm_one pay for a fixed order of "
                               "the column sums with a transpose of the moduli (no floating-point atomic add)"})
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
