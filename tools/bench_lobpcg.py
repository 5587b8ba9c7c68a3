#!/usr/bin/env python3
"""LOBPCG on device handles (spl_lobpcg_*), one MI355X.  (The Gram kernel it is built on has its own table:
tools/bench_gram.py, profiles/gram_bench.json.)

  (b) ms per LOBPCG iteration on poisson3d(--m3) for block = 10 and 20, without a preconditioner and with the AMG cycle:
      solves that cannot converge (tol = atol = 0) of 1 and of 3 iterations, the difference halved; beside it the parts
      timed alone on arrays of the same shape: one product of 2 block columns, block AMG cycles, the Gram matrix of
      3 block columns (upper), the two rotations 3 block -> 2 block; what is left is the orthogonalisation (5 block
      columns of classical Gram-Schmidt done twice), the residuals and the host's close.  Launches, synchronisations
      and device memory of the 3-iteration solve.
  (c) the case of DESIGN.md 4.14 (c): the 10 smallest eigenpairs of 1.0 L(x)I(x)I + 1.3 I(x)L(x)I + 1.7 I(x)I(x)L at
      --small-m3 and --m3 to tol 1e-8 by LOBPCG with AMG (block 10 + --guard columns) and without a preconditioner (capped
      at --plain-maxiter iterations), against inverse-mode Lanczos (sigma = 0, CG + AMG to 1e-10) from the same run;
      errors against the closed form.
  (d) the isotropic poisson3d(--small-m3): the --iso-nev smallest values with LOBPCG + AMG, and the multiplicities found
      against those of the closed form (a single-vector Lanczos returns one copy of each).

Every case is warmed up; a time is a host clock around a call that ends in a device synchronise; medians of --rounds with
[min, max].  Nothing is asserted about a ratio: it is recorded.  Prints one JSON line (and writes it to --out).
python tools/bench_lobpcg.py [--m3 200] [--small-m3 80] [--rounds 3] [--parts b,c,d] [--out profiles/lobpcg_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KNOBS = ("SPL_KRYLOV_GRID", "SPL_GMRES_DOTS_BATCH", "SPL_EIGSH_ROTATE_ROWS", "SPL_GRAM_TILE", "SPL_GRAM_SCRATCH",
         "SPL_AMG_TAIL_ROWS")
WEIGHTS = (1.0, 1.3, 1.7)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m3", type=int, default=200)
    ap.add_argument("--small-m3", type=int, default=80)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--nev", type=int, default=10)
    ap.add_argument("--guard", type=int, default=4)
    ap.add_argument("--iso-nev", type=int, default=20)
    ap.add_argument("--plain-maxiter", type=int, default=300)
    ap.add_argument("--parts", default="b,c,d")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
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

    result = {"what": "tools/bench_lobpcg.py: LOBPCG on device handles (spl_lobpcg_*), one MI355X, host clock ending in a "
                      "synchronise, %d rounds after a warm-up, medians with [min, max]" % args.rounds,
              "device": torch.cuda.get_device_name(0)}

    def save():
        line = json.dumps(result)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(result, indent=1) + "\n")
        return line

    def start_block(n, block):
        gen = torch.Generator(device="cuda").manual_seed(n + block)
        return torch.rand((n, block), dtype=torch.float64, device="cuda", generator=gen) - 0.5

    # ---- (b) -----------------------------------------------------------------------------------------------------------
    def iteration_cells():
        cells = []
        H = DM.synthetic("poisson3d", args.m3)
        n = H.info()["nrows_global"]
        amg = H.amg()
        for block in (10, 20):
            X0 = start_block(n, block).T.contiguous()
            out = torch.empty((block, n), dtype=torch.float64, device="cuda")
            S = torch.rand((3 * block, n), dtype=torch.float64, device="cuda") - 0.5
            AS = torch.rand((3 * block, n), dtype=torch.float64, device="cuda") - 0.5
            G = torch.zeros(9 * block * block, dtype=torch.float64, device="cuda")
            Y = torch.linalg.qr(torch.rand(3 * block, 3 * block, dtype=torch.float64, device="cuda") - 0.5)[0][:, :2 * block]
            Y = Y.T.contiguous()
            m_spmv, t_spmv = timed(lambda: H.spmv_many_dev(S.data_ptr(), n, AS.data_ptr(), n, 2 * block, False, stream),
                                   args.rounds)

            def cycles():
                for j in range(block):
                    amg.apply_dev(S[j].data_ptr(), AS[j].data_ptr(), stream)
            m_amg, t_amg = timed(cycles, args.rounds)
            m_gram, t_gram = timed(lambda: pkg.vector_gram_dev(n, 3 * block, 3 * block, S.data_ptr(), n, AS.data_ptr(), n,
                                                               G.data_ptr(), 3 * block, True, False, stream), args.rounds)

            def rotations():
                for V in (S, AS):
                    pkg.sparse.vector_rotate_dev(n, 3 * block, 2 * block, V.data_ptr(), n, Y.data_ptr(), 3 * block, None, 0,
                                                 False, stream)
            m_rot, t_rot = timed(rotations, args.rounds)
            del S, AS
            torch.cuda.empty_cache()
            for M, name in ((None, "none"), (amg, "amg")):
                L = pkg.LOBPCGSolver(H, block, M)
                got = {}

                def solve(iterations):
                    got[iterations] = L.solve_dev(block, X0.data_ptr(), n, out.data_ptr(), n, False, 0.0, 0.0, iterations,
                                                  False, stream)[1]
                m1, t1 = timed(lambda: solve(1), args.rounds)
                m3, t3 = timed(lambda: solve(3), args.rounds)
                per = (m3 - m1) / 2.0
                inf, res1, res3 = L.info(), got[1], got[3]
                parts = m_spmv + m_gram + m_rot + (m_amg if M is not None else 0.0)
                cell = {"workload": "poisson3d(%d)" % args.m3, "n": n, "block": block, "preconditioner": name,
                        "solve_of_1_iteration": t1, "solve_of_3_iterations": t3, "ms_per_iteration": round(per * 1e3, 3),
                        "product_of_2_block_columns": t_spmv, "block_amg_cycles": t_amg if M is not None else None,
                        "gram_of_3_block_columns_upper": t_gram, "two_rotations_3_block_to_2_block": t_rot,
                        "orthogonalisation_residuals_and_host_close_ms": round((per - parts) * 1e3, 3),
                        "launches_of_the_3_iteration_solve": inf["launches"],
                        "synchronisations_per_iteration": (res3["synchronisations"] - res1["synchronisations"]) / 2.0,
                        "columns_dropped": res3["columns_dropped"], "device_bytes": inf["device_bytes"]}
                print("%r" % (cell,), file=sys.stderr, flush=True)
                cells.append(cell)
                L.free()
                torch.cuda.empty_cache()
        amg.free()
        H.free()
        return cells

    # ---- (c), (d) --------------------------------------------------------------------------------------------------------
    def laplacian_arrays(m):
        rp = np.concatenate([[0], np.cumsum(np.concatenate([[2], np.full(m - 2, 3), [2]]))]).astype(np.int64)
        rows = np.repeat(np.arange(m), np.diff(rp))
        ci = (rows + (np.arange(3 * m - 2) - rp[rows]) - (rows > 0)).astype(np.int32)
        v = np.where(ci == rows, 2.0, -1.0)
        return rp, ci, v

    def laplacian3(m, weights):
        rp, ci, v = laplacian_arrays(m)
        L = DM.from_csr(m, m, rp, ci, v)
        I = DM.ident(m)
        II = I.kronecker(I)
        terms = [L.kronecker(II), I.kronecker(L).kronecker(I), II.kronecker(L)]
        two = terms[0].lin(weights[0], terms[1], weights[1])
        A = two.lin(1.0, terms[2], weights[2])
        for h in terms + [two, II, I, L]:
            h.free()
        return A

    def closed_form(m, count, weights):
        a = 2.0 - 2.0 * np.cos(np.arange(1, m + 1) * np.pi / (m + 1))
        low = a[:min(m, 12)]  # the smallest values use small indices only
        all_ = (weights[0] * low[:, None, None] + weights[1] * low[None, :, None] + weights[2] * low[None, None, :]).ravel()
        return np.sort(all_)[:count]

    def report(t, values, res, exact):
        values = np.sort(np.asarray(values))
        keys = ("reason_name", "iterations", "cycles", "applications", "inner_iterations", "spmv_columns",
                "preconditioner_applications", "columns_dropped", "synchronisations", "pairs")
        return dict(t, worst_residual=float(res["residuals"].max()) if res["pairs"] else None,
                    worst_error_against_the_closed_form=float(np.max(np.abs(values - exact[:len(values)]))) if len(values) else None,
                    **{k: res[k] for k in keys if k in res})

    def whole_solves(m):
        A = laplacian3(m, WEIGHTS)
        n = A.info()["nrows_global"]
        nev, block = args.nev, args.nev + args.guard
        exact = closed_form(m, nev + 1, WEIGHTS)
        row = {"instance": "anisotropic Laplacian %d^3 (weights %s)" % (m, list(WEIGHTS)), "n": n, "nev": nev, "block": block,
               "tol": 1e-8, "relative_gap_behind_the_last": float((exact[nev] - exact[nev - 1]) / exact[nev - 1])}
        X0 = start_block(n, block)
        got = {}
        setup = {}

        def make():
            setup["L"] = pkg.LOBPCGSolver(A, block, "amg")
        row["lobpcg_setup_amg_and_object"] = {"ms": round(clock(make) * 1e3, 3)}
        L = setup["L"]

        def with_amg():
            got["a"] = L.solve(X0, nev, False, 1e-8, 0.0, 200)
        _, t = timed(with_amg, args.rounds)
        row["lobpcg_amg"] = dict(report(t, got["a"][0], got["a"][2], exact), device_bytes=L.info()["device_bytes"])
        print("%r" % (row["lobpcg_amg"],), file=sys.stderr, flush=True)
        L.set_preconditioner(None)

        def plain():
            got["p"] = L.solve(X0, nev, False, 1e-8, 0.0, args.plain_maxiter)
        _, t = timed(plain, 1, warmup=0)
        row["lobpcg_no_preconditioner"] = dict(report(t, got["p"][0], got["p"][2], exact), max_iter=args.plain_maxiter, runs=1)
        print("%r" % (row["lobpcg_no_preconditioner"],), file=sys.stderr, flush=True)
        L.free()
        torch.cuda.empty_cache()
        v0 = torch.from_numpy(np.random.default_rng(0).standard_normal(n)).cuda()
        E = pkg.EigenSolver(A, pkg.sparse.default_ncv(n, nev), sigma=0.0, M="amg", inner_rtol=1e-10, inner_maxiter=2000)

        def inverse():
            got["i"] = E.solve(nev, "LM", 1e-8, 0.0, 100, v0)
        _, t = timed(inverse, args.rounds)
        row["lanczos_inverse_LM_sigma_0_cg_amg"] = report(t, got["i"][0], got["i"][2], exact)
        print("%r" % (row["lanczos_inverse_LM_sigma_0_cg_amg"],), file=sys.stderr, flush=True)
        E.free()
        A.free()
        torch.cuda.empty_cache()
        result.setdefault("c_whole_solves", []).append(row)
        save()

    def multiplicities():
        m, nev = args.small_m3, args.iso_nev
        A = laplacian3(m, (1.0, 1.0, 1.0))
        n = A.info()["nrows_global"]
        exact = closed_form(m, nev + args.guard + 1, (1.0, 1.0, 1.0))
        block = nev + args.guard
        X0 = start_block(n, block)
        L = pkg.LOBPCGSolver(A, block, "amg")
        got = {}

        def solve():
            got["v"] = L.solve(X0, nev, False, 1e-8, 0.0, 200)
        _, t = timed(solve, args.rounds)
        values, _, res = got["v"]
        values = np.sort(values)

        def groups(v):
            out, i = [], 0
            while i < len(v):
                j = i
                while j + 1 < len(v) and abs(v[j + 1] - v[i]) <= 1e-6 * abs(v[i]):
                    j += 1
                out.append(j - i + 1)
                i = j + 1
            return out
        cell = dict(report(t, values, res, exact), instance="isotropic poisson3d(%d)" % m, n=n, nev=nev, block=block,
                    multiplicities_found=groups(values), multiplicities_of_the_closed_form=groups(exact[:nev]),
                    distinct_values_a_single_vector_method_returns=len(groups(exact[:nev])))
        print("%r" % (cell,), file=sys.stderr, flush=True)
        L.free()
        A.free()
        result["d_isotropic_multiplicities"] = cell

    if "b" in wanted:
        result["b_ms_per_iteration"] = iteration_cells()
        save()
    if "c" in wanted:
        whole_solves(args.small_m3)
        whole_solves(args.m3)
    if "d" in wanted:
        multiplicities()
    print(save(), flush=True)


if __name__ == "__main__":
    main()
