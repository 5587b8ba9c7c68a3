#!/usr/bin/env python3
"""A numeric factorisation from host arrays (`factor`) against one from a device-resident handle (`factorDevice`), same
matrix, same analysis, same process: the FEAST pattern of one symbolic analysis and many same-pattern factorisations.

Workloads: zi3d:<m> the contour point (3 + 0.5i) I - A of the 3-D 7-point Laplacian on an m^3 grid (complex symmetric;
native complex fronts where the tree has the work), zi2d:<m> the same of the 2-D 5-point Laplacian on an m^2 grid (below
the native threshold: the real embedding, where the host's share is largest), real3d:<m> 3-D Poisson itself.

Per workload one JSON line: after one warm-up factorisation of each route (so that the device pool serves the large
blocks) the median and the min - max of --reps steady-state factorisations per route, the seconds spent inside hipMalloc
meanwhile (spl_device_alloc_seconds: a wait for the driver's wipe would show there), and the SPL_MF_TIMING phase split of
one further call of each route.  --routes host runs on a commit that has no handle route (the baseline)."""
import argparse
import json
import os
import re
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build(pkg, spec):
    """(host Matrix, DeviceMatrix, description) of a workload, assembled on the device: A from the synthetic generator,
    z I - A by to_complex and lin on handles; the host copy is the export of that handle (symmetric: CSR == CSC)"""
    kind, m = spec.split(":")
    m = int(m)
    dim = 2 if kind == "zi2d" else 3
    n = m ** dim
    H = pkg.DeviceMatrix.synthetic("poisson2d" if dim == 2 else "poisson3d", m)
    if kind == "real3d":
        what = "3-D Poisson %d^3" % m
    else:
        I = pkg.DeviceMatrix.from_csc(pkg.ident(n)).to_complex()
        Hz = H.to_complex()
        H.free()
        H = I.lin(3.0 + 0.5j, Hz, -1.0)
        I.free()
        Hz.free()
        what = "(3 + 0.5i) I - A, %d-D Laplacian %d^%d" % (dim, m, dim)
    rp, ci, v = H.export_csr()
    return pkg.Matrix(n, n, rp, ci, v), H, what


def timed(pkg, torch, fn, reps):
    """fn() reps times, its result released before the next call; seconds of each, and of hipMalloc over all"""
    a0 = pkg._ffi.device_alloc_seconds()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f = fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
        del f
    times_sorted = sorted(times)
    mid = len(times) // 2
    median = times_sorted[mid] if len(times) % 2 else 0.5 * (times_sorted[mid - 1] + times_sorted[mid])
    return {"median_s": round(median, 5), "min_s": round(times_sorted[0], 5), "max_s": round(times_sorted[-1], 5),
            "times_s": [round(t, 5) for t in times], "hipMalloc_s": round(pkg._ffi.device_alloc_seconds() - a0, 5)}


def phases(fn):
    """the SPL_MF_TIMING lines one call writes to stderr: {phase: milliseconds}"""
    sys.stderr.flush()
    saved = os.dup(2)
    out = {}
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.environ["SPL_MF_TIMING"] = "1"
        os.dup2(tmp.fileno(), 2)
        try:
            f = fn()
            del f
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            del os.environ["SPL_MF_TIMING"]
        tmp.seek(0)
        for line in tmp.read().decode(errors="replace").splitlines():
            hit = re.match(r"\[(zi numeric|numeric)\]\s+(.*?)\s+([0-9.]+) ms\s*$", line)
            if hit:
                key = hit.group(2).strip() if hit.group(1) == "numeric" else "zi: " + hit.group(2).strip()
                out[key] = out.get(key, 0.0) + float(hit.group(3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="zi3d:100,zi3d:64,zi2d:1000,real3d:100")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--routes", default="host,handle")
    ap.add_argument("--label", default="", help="copied into every line (e.g. the commit measured)")
    args = ap.parse_args()
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    torch.cuda.set_device(0)
    U = pkg.umfpack
    routes = args.routes.split(",")
    for spec in args.workloads.split(","):
        A, H, what = build(pkg, spec)
        t0 = time.perf_counter()
        an = U.analyzeDevice(H) if "handle" in routes else U.analyze(A)
        analysis_s = time.perf_counter() - t0
        calls = {"host": lambda: U.factor(A, an), "handle": lambda: U.factorDevice(H, an)}
        line = {"workload": spec, "matrix": what, "n": A.ncols, "nnz": int(A.pointers[-1]), "label": args.label,
                "analysis_s": round(analysis_s, 3), "reps": args.reps}
        for r in routes:  # warm-up: first-use costs, and the large blocks enter the pool
            f = calls[r]()
            line.update(path=f.path, complex_fronts=f.stats["complex_fronts"])
            del f
        for r in routes:
            line[r] = timed(pkg, torch, calls[r], args.reps)
        for r in routes:
            line[r]["phases_ms"] = phases(calls[r])
        if "host" in routes and "handle" in routes:
            line["host_over_handle"] = round(line["host"]["median_s"] / line["handle"]["median_s"], 3)
        print(json.dumps(line), flush=True)
        del an, A
        H.free()


if __name__ == "__main__":
    main()
