#!/usr/bin/env python3
"""LOBPCG for A x = lambda B x on device handles (spl_lobpcg_set_mass) and the paired update it is built on
(spl_vector_update_pair_dev), one MI355X.

  (a) the paired update at --rows rows for k = 10, 30, 60, 125 columns, real and complex, with Re<w, bw>: ms, and the
      bytes it has to move ((2 k + 4) n entries: the columns of V and BV once, w and bw in and out) per second; beside it
      a device-to-device copy that moves the same bytes ((k + 2) n entries read and as many written).
  (b) ms per LOBPCG iteration on poisson3d(--m3) with the 27-point mass matrix kron(T, T, T), T = tridiag(1, 4, 1), for
      block = 10 and 20, beside the standard iteration of the same object from the same run: solves that cannot converge
      (tol = atol = 0) of 1 and of 3 iterations, the difference halved; beside it one product of `block` columns with B.
  (c) the 10 smallest pairs of (7-point Laplacian, 27-point mass) at --small-m3 to tol 1e-8 by LOBPCG with AMG on A
      (block 10 + --guard columns), beside feast.geigSH with the same B on a window that holds exactly those 10, and
      beside scipy's eigsh(A, k = 10, M = B, sigma = 0) in a process of its own on the host's threads, given
      --scipy-limit seconds; errors against the closed form (A and B share the sine modes).

Every case is warmed up; a time is a host clock around a call that ends in a device synchronise; medians of --rounds with
[min, max].  Nothing is asserted about a ratio: it is recorded.  Prints one JSON line (and writes it to --out).
python tools/bench_globpcg.py [--rows 8000000] [--m3 200] [--small-m3 80] [--parts a,b,c] [--out profiles/globpcg_bench.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KNOBS = ("SPL_KRYLOV_GRID", "SPL_GMRES_DOTS_BATCH", "SPL_EIGSH_ROTATE_ROWS", "SPL_GRAM_TILE", "SPL_GRAM_SCRATCH",
         "SPL_AMG_TAIL_ROWS")


def tridiagonal_arrays(m, diagonal, off):
    import numpy as np
    rp = np.concatenate([[0], np.cumsum(np.concatenate([[2], np.full(m - 2, 3), [2]]))]).astype(np.int64)
    rows = np.repeat(np.arange(m), np.diff(rp))
    ci = (rows + (np.arange(3 * m - 2) - rp[rows]) - (rows > 0)).astype(np.int32)
    return rp, ci, np.where(ci == rows, diagonal, off)


def closed_form(m, count):
    """the smallest `count` values (a_i + a_j + a_k) / (t_i t_j t_k), a = 2 - 2 cos, t = 4 + 2 cos of k pi / (m + 1)"""
    import numpy as np
    c = np.cos(np.arange(1, min(m, 12) + 1) * np.pi / (m + 1))  # the smallest values use small indices only
    a, t = 2.0 - 2.0 * c, 4.0 + 2.0 * c
    num = a[:, None, None] + a[None, :, None] + a[None, None, :]
    den = t[:, None, None] * t[None, :, None] * t[None, None, :]
    return np.sort((num / den).ravel())[:count]


def scipy_child(m, nev):
    """eigsh(A, M=B, sigma=0) on the host, no GPU: prints one JSON line"""
    import numpy as np
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla

    def tri(diagonal, off):
        return sp.diags([np.full(m - 1, off), np.full(m, diagonal), np.full(m - 1, off)], [-1, 0, 1], format="csr")
    L, T, I = tri(2.0, -1.0), tri(4.0, 1.0), sp.identity(m, format="csr")
    A = (sp.kron(sp.kron(L, I), I) + sp.kron(sp.kron(I, L), I) + sp.kron(sp.kron(I, I), L)).tocsc()
    B = sp.kron(sp.kron(T, T), T).tocsc()
    t0 = time.perf_counter()
    values, X = spla.eigsh(A, k=nev, M=B, sigma=0.0, which="LM", tol=1e-8)
    seconds = time.perf_counter() - t0
    exact = closed_form(m, nev)
    R = A @ X - (B @ X) * values
    print(json.dumps({"seconds": round(seconds, 3), "worst_residual": float(np.linalg.norm(R, axis=0).max()),
                      "worst_error_against_the_closed_form": float(np.abs(np.sort(values) - exact).max())}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=8000000)
    ap.add_argument("--m3", type=int, default=200)
    ap.add_argument("--small-m3", type=int, default=80)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--nev", type=int, default=10)
    ap.add_argument("--guard", type=int, default=4)
    ap.add_argument("--scipy-limit", type=int, default=300)
    ap.add_argument("--parts", default="a,b,c")
    ap.add_argument("--out", default=None)
    ap.add_argument("--scipy-child", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.scipy_child:
        return scipy_child(args.scipy_child, args.nev)
    import numpy as np
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    torch.cuda.set_device(0)
    DM = pkg.DeviceMatrix
    wanted = args.parts.split(",")
    for key in KNOBS:
        os.environ.pop(key, None)
    stream = torch.cuda.current_stream().cuda_stream

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

    result = {"what": "tools/bench_globpcg.py: LOBPCG with a mass matrix (spl_lobpcg_set_mass) and the paired update "
                      "(spl_vector_update_pair_dev), one MI355X, host clock ending in a synchronise, %d rounds after a "
                      "warm-up, medians with [min, max]" % args.rounds,
              "device": torch.cuda.get_device_name(0)}

    def save():
        line = json.dumps(result)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(result, indent=1) + "\n")
        return line

    # ---- (a) -----------------------------------------------------------------------------------------------------------
    def update_cells():
        cells = []
        n, kmax = args.rows, 125
        pool = torch.rand((2 * (kmax + 2), 2 * n), dtype=torch.float64, device="cuda") - 0.5  # rows of 2 n doubles
        V, BV = pool[:kmax + 2], pool[kmax + 2:]
        coef = (torch.rand(2 * kmax, dtype=torch.float64, device="cuda") - 0.5) / 64.0
        q = torch.zeros(1, dtype=torch.float64, device="cuda")
        for cplx in (False, True):
            entry = 16 if cplx else 8
            ld = n if cplx else 2 * n  # a row of the pool holds n packed pairs or 2 n doubles
            for k in (10, 30, 60, 125):
                w, bw = V[kmax], BV[kmax]
                m_up, t_up = timed(lambda: pkg.vector_update_pair_dev(n, k, V.data_ptr(), ld, BV.data_ptr(), ld, coef.data_ptr(),
                                                                      w.data_ptr(), bw.data_ptr(), q.data_ptr(), cplx, stream),
                                   args.rounds)
                width = n * entry // 8  # doubles of a column
                src, dst = V[:k + 2, :width], BV[:k + 2, :width]
                m_copy, t_copy = timed(lambda: dst.copy_(src), args.rounds)
                moved = (2 * k + 4) * n * entry
                cell = {"rows": n, "k": k, "values": "complex" if cplx else "real", "bytes_moved": moved,
                        "update_pair_with_q": t_up, "update_pair_TB_per_s": round(moved / m_up / 1e12, 3),
                        "copy_of_the_same_bytes": t_copy, "copy_TB_per_s": round(moved / m_copy / 1e12, 3),
                        "update_over_copy": round(m_up / m_copy, 3)}
                print("%r" % (cell,), file=sys.stderr, flush=True)
                cells.append(cell)
        del pool, V, BV
        torch.cuda.empty_cache()
        return cells

    # ---- the matrices ------------------------------------------------------------------------------------------------------
    def kron3(m, diagonal, off):
        T = DM.from_csr(m, m, *tridiagonal_arrays(m, diagonal, off))
        TT = T.kronecker(T)
        B = TT.kronecker(T)
        TT.free()
        T.free()
        return B

    def laplacian3(m):
        L = DM.from_csr(m, m, *tridiagonal_arrays(m, 2.0, -1.0))
        I = DM.ident(m)
        II = I.kronecker(I)
        terms = [L.kronecker(II), I.kronecker(L).kronecker(I), II.kronecker(L)]
        two = terms[0].lin(1.0, terms[1], 1.0)
        A = two.lin(1.0, terms[2], 1.0)
        for h in terms + [two, II, I, L]:
            h.free()
        return A

    def start_block(n, block):
        gen = torch.Generator(device="cuda").manual_seed(n + block)
        return torch.rand((n, block), dtype=torch.float64, device="cuda", generator=gen) - 0.5

    # ---- (b) -----------------------------------------------------------------------------------------------------------
    def iteration_cells():
        cells = []
        H = DM.synthetic("poisson3d", args.m3)
        B = kron3(args.m3, 4.0, 1.0)
        n = H.info()["nrows_global"]
        for block in (10, 20):
            X0 = start_block(n, block).T.contiguous()
            out = torch.empty((block, n), dtype=torch.float64, device="cuda")
            BX = torch.empty((block, n), dtype=torch.float64, device="cuda")
            _, t_mass = timed(lambda: B.spmv_many_dev(X0.data_ptr(), n, BX.data_ptr(), n, block, False, stream), args.rounds)
            del BX
            L = pkg.LOBPCGSolver(H, block)
            cell = {"workload": "poisson3d(%d), 27-point mass" % args.m3, "n": n, "block": block, "preconditioner": "none",
                    "product_of_block_columns_with_B": t_mass, "nnz_of_B": B.info()["nnz"]}
            for name, mass in (("standard", None), ("generalized", B)):
                L.set_mass(mass)
                got = {}

                def solve(iterations):
                    got[iterations] = L.solve_dev(block, X0.data_ptr(), n, out.data_ptr(), n, False, 0.0, 0.0, iterations,
                                                  False, stream)[1]
                m1, t1 = timed(lambda: solve(1), args.rounds)
                m3, t3 = timed(lambda: solve(3), args.rounds)
                inf = L.info()
                cell[name] = {"solve_of_1_iteration": t1, "solve_of_3_iterations": t3,
                              "ms_per_iteration": round((m3 - m1) / 2.0 * 1e3, 3),
                              "launches_of_the_3_iteration_solve": inf["launches"],
                              "synchronisations_per_iteration": (got[3]["synchronisations"] - got[1]["synchronisations"]) / 2.0,
                              "columns_dropped": got[3]["columns_dropped"], "mass_columns": inf["mass_columns"],
                              "device_bytes": inf["device_bytes"]}
            cell["generalized_over_standard"] = round(cell["generalized"]["ms_per_iteration"]
                                                      / cell["standard"]["ms_per_iteration"], 3)
            print("%r" % (cell,), file=sys.stderr, flush=True)
            cells.append(cell)
            L.free()
            torch.cuda.empty_cache()
        B.free()
        H.free()
        return cells

    # ---- (c) -----------------------------------------------------------------------------------------------------------
    def whole_solves():
        m, nev, block = args.small_m3, args.nev, args.nev + args.guard
        A, B = laplacian3(m), kron3(m, 4.0, 1.0)
        n = A.info()["nrows_global"]
        exact = closed_form(m, nev + 1)
        row = {"instance": "7-point Laplacian and 27-point mass, %d^3" % m, "n": n, "nev": nev, "block": block, "tol": 1e-8,
               "relative_gap_behind_the_last": float((exact[nev] - exact[nev - 1]) / exact[nev - 1])}
        X0 = start_block(n, block)
        setup, got = {}, {}

        def make():
            setup["L"] = pkg.LOBPCGSolver(A, block, "amg", B)
        row["lobpcg_setup_amg_and_object"] = {"ms": round(clock(make) * 1e3, 3)}
        L = setup["L"]

        def solve():
            got["g"] = L.solve(X0, nev, False, 1e-8, 0.0, 200)
        _, t = timed(solve, args.rounds)
        values, _, res = got["g"]
        keys = ("reason_name", "iterations", "spmv_columns", "preconditioner_applications", "columns_dropped", "pairs")
        row["lobpcg_amg_generalized"] = dict(t, worst_residual=float(res["residuals"].max()) if res["pairs"] else None,
                                             worst_error_against_the_closed_form=float(
                                                 np.abs(np.sort(values) - exact[:len(values)]).max()) if len(values) else None,
                                             mass_columns=L.info()["mass_columns"], device_bytes=L.info()["device_bytes"],
                                             **{k: res[k] for k in keys})
        print("%r" % (row["lobpcg_amg_generalized"],), file=sys.stderr, flush=True)
        L.free()
        result["c_whole_solves"] = row
        save()

        def host(H):
            rp, ci, v = H.export_csr()
            return pkg.Matrix(n, n, rp, ci, v)  # symmetric: the CSR arrays are the CSC arrays
        hA, hB = host(A), host(B)
        A.free()
        B.free()
        torch.cuda.empty_cache()
        window = (0.0, float(0.5 * (exact[nev - 1] + exact[nev])))

        def feast():
            got["f"] = pkg.feast.geigSH(16, window, hA, hB)
        _, t = timed(feast, 1, warmup=1)
        lam = np.sort(np.asarray(got["f"][0]))
        row["feast_geigSH_m0_16"] = dict(t, runs=1, found=int(len(lam)), window=list(window),
                                         worst_error_against_the_closed_form=float(np.abs(lam - exact[:len(lam)]).max())
                                         if len(lam) == nev else None)
        print("%r" % (row["feast_geigSH_m0_16"],), file=sys.stderr, flush=True)
        save()
        try:
            child = subprocess.run([sys.executable, os.path.abspath(__file__), "--scipy-child", str(m), "--nev", str(nev)],
                                   capture_output=True, text=True, timeout=args.scipy_limit)
            row["scipy_eigsh_M_B_sigma_0"] = (json.loads(child.stdout.strip().splitlines()[-1]) if child.returncode == 0
                                              else {"failed": child.stderr.strip().splitlines()[-1:]})
        except subprocess.TimeoutExpired:
            row["scipy_eigsh_M_B_sigma_0"] = {"did_not_finish_within_seconds": args.scipy_limit}
        row["scipy_eigsh_M_B_sigma_0"]["threads"] = os.environ.get("OMP_NUM_THREADS")
        print("%r" % (row["scipy_eigsh_M_B_sigma_0"],), file=sys.stderr, flush=True)

    if "a" in wanted:
        result["a_paired_update"] = update_cells()
        save()
    if "b" in wanted:
        result["b_ms_per_iteration"] = iteration_cells()
        save()
    if "c" in wanted:
        whole_solves()
    print(save(), flush=True)


if __name__ == "__main__":
    main()
