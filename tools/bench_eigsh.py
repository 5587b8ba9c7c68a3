#!/usr/bin/env python3
"""Thick-restart Lanczos on device handles (spl_eigsh_*) and its in-place basis rotation, one MI355X.

  (a) spl_vector_rotate_dev in place at n = 8.0e6 for (m, k) = (20, 10), (64, 32), (128, 64), real and complex, at the
      tile heights SPL_EIGSH_ROTATE_ROWS = 16, 32, 64 and at the library's default, against a device-to-device copy of
      n (m + k) entries (what any pass must at least move) and against the arithmetic: 2 n m k products and sums per
      part, none of them fused.
  (b) ms per Lanczos step (a solve of one cycle that cannot converge, tol = atol = 0, max_restarts = 1, nev = 1, divided
      by ncv: the start, the close and the finish of one pair are in it) for ncv = 10, 30, 50 on poisson3d(200), and the
      GMRES step of the same basis length measured the same way in the same run.
  (c) the 10 smallest eigenpairs of the anisotropic Laplacian 1.0 L (x) I (x) I + 1.3 I (x) L (x) I + 1.7 I (x) I (x) L,
      assembled handle to handle with kronecker / lin, at 80^3 and 200^3 to tol 1e-8: direct `SA`; inverse `LM` at
      sigma = 0 with CG + AMG (the setup apart); at 80^3 the FEAST driver over an interval that holds those 10 and, if
      scipy imports, scipy.sparse.linalg.eigsh (ARPACK, `SA`, once).  Every value is compared with the closed form.

Every case is warmed up; a time is a host clock around a call that ends in a device synchronise; medians of --rounds with
[min, max].  Nothing is asserted about a ratio: it is recorded.  Prints one JSON line (and writes it to --out).
python tools/bench_eigsh.py [--n 8000000] [--m3 200] [--small-m3 80] [--rounds 3] [--parts a,b,c] [--direct-restarts 300]
                            [--no-scipy] [--scipy-maxiter 300] [--out profiles/eigsh_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KNOBS = ("SPL_KRYLOV_GRID", "SPL_GMRES_DOTS_BATCH", "SPL_EIGSH_ROTATE_ROWS", "SPL_AMG_TAIL_ROWS")
WEIGHTS = (1.0, 1.3, 1.7)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8_000_000)
    ap.add_argument("--m3", type=int, default=200)
    ap.add_argument("--small-m3", type=int, default=80)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parts", default="a,b,c")
    ap.add_argument("--nev", type=int, default=10)
    ap.add_argument("--direct-restarts", type=int, default=300)
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--scipy-maxiter", type=int, default=300, help="ARPACK's restarts at most")
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

    def clock(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def timed(f, rounds, warmup=1, per=1):
        for _ in range(warmup):
            clock(f)
        ts = [clock(f) / per for _ in range(rounds)]
        return statistics.median(ts), {"ms": round(statistics.median(ts) * 1e3, 4),
                                       "ms_min_max": [round(min(ts) * 1e3, 4), round(max(ts) * 1e3, 4)]}

    result = {"what": "tools/bench_eigsh.py: thick-restart Lanczos on device handles (spl_eigsh_*) and spl_vector_rotate_dev, "
                      "one MI355X, host clock ending in a synchronise, %d rounds after a warm-up, medians with [min, max]"
                      % args.rounds,
              "device": torch.cuda.get_device_name(0)}

    def save():
        line = json.dumps(result)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(line + "\n")
        return line

    # ---- (a) -----------------------------------------------------------------------------------------------------------
    def rotation_cells():
        cells = []
        n = args.n
        stream = torch.cuda.current_stream().cuda_stream
        for cplx in (False, True):
            dtype = torch.complex128 if cplx else torch.float64
            step = 16 if cplx else 8
            for m, k in ((20, 10), (64, 32), (128, 64)):
                V = (torch.rand(m * n, dtype=torch.float64, device="cuda") - 0.5).to(dtype)
                # an orthogonal-like Y keeps the columns bounded over the repeated in-place calls
                Y = torch.linalg.qr(torch.rand(m, m, dtype=torch.float64, device="cuda") - 0.5)[0][:, :k].T.contiguous()
                src = torch.empty((m + k) * n // 2, dtype=dtype, device="cuda")
                sink = torch.empty_like(src)

                def run():
                    pkg.sparse.vector_rotate_dev(n, m, k, V.data_ptr(), n, Y.data_ptr(), m, None, 0, cplx, stream)
                by_rows = {}
                for rows in ("16", "32", "64"):
                    os.environ["SPL_EIGSH_ROTATE_ROWS"] = rows
                    by_rows[rows] = timed(run, args.rounds)[1]
                os.environ.pop("SPL_EIGSH_ROTATE_ROWS", None)
                m_def, t_def = timed(run, args.rounds)
                m_copy, t_copy = timed(lambda: sink.copy_(src), args.rounds)  # reads and writes n (m + k) / 2 entries each
                flops = 2.0 * n * m * k * (2 if cplx else 1)
                cell = {"values": "complex" if cplx else "real", "n": n, "m": m, "k": k, "in_place_by_tile_rows": by_rows,
                        "in_place_default_rows": t_def, "copy_moving_n_times_m_plus_k_entries": t_copy,
                        "rotate_over_copy": round(m_def / m_copy, 2),
                        "moved_GBps": round((m + k) * n * step / m_def / 1e9, 1),
                        "unfused_GFLOPs": round(flops / m_def / 1e9, 1)}
                print("%r" % (cell,), file=sys.stderr, flush=True)
                cells.append(cell)
                del V, src, sink
                torch.cuda.empty_cache()
        return cells

    # ---- (b) -----------------------------------------------------------------------------------------------------------
    def step_cells():
        cells = []
        H = DM.synthetic("poisson3d", args.m3)
        inf = H.info()
        n = inf["nrows_global"]
        stream = torch.cuda.current_stream().cuda_stream
        gen = torch.Generator(device="cuda").manual_seed(n)
        b = torch.rand(n, dtype=torch.float64, device="cuda", generator=gen) - 0.5
        x = torch.empty_like(b)
        X = torch.empty(n, dtype=torch.float64, device="cuda")
        m_spmv, t_spmv = timed(lambda: H.spmv_dev(b.data_ptr(), x.data_ptr(), False, stream), args.rounds)
        for ncv in (10, 30, 50):
            E = pkg.EigenSolver(H, ncv)
            m_l, t_l = timed(lambda: E.solve_dev(1, b.data_ptr(), X.data_ptr(), n, "LA", 0.0, 0.0, 1, False, stream),
                             args.rounds, per=ncv)
            e_info = E.info()
            E.free()
            S = H.gmres(ncv, None)
            m_g, t_g = timed(lambda: S.solve_dev(b.data_ptr(), x.data_ptr(), False, 0.0, 0.0, ncv, 0, False, stream),
                             args.rounds, per=ncv)
            g_info = S.info()
            S.free()
            cell = {"workload": "poisson3d(%d)" % args.m3, "n": n, "nnz": inf["nnz"], "basis": ncv,
                    "lanczos_ms_per_step": t_l, "gmres_ms_per_step": t_g, "lanczos_over_gmres": round(m_l / m_g, 3),
                    "lanczos_launches": e_info["launches"], "gmres_launches": g_info["launches"],
                    "lanczos_device_bytes": e_info["device_bytes"], "gmres_device_bytes": g_info["device_bytes"],
                    "one_spmv": t_spmv}
            print("%r" % (cell,), file=sys.stderr, flush=True)
            cells.append(cell)
            torch.cuda.empty_cache()
        H.free()
        return cells

    # ---- (c) -----------------------------------------------------------------------------------------------------------
    def laplacian_arrays(m):
        rp = np.concatenate([[0], np.cumsum(np.concatenate([[2], np.full(m - 2, 3), [2]]))]).astype(np.int64)
        rows = np.repeat(np.arange(m), np.diff(rp))
        ci = (rows + (np.arange(3 * m - 2) - rp[rows]) - (rows > 0)).astype(np.int32)
        v = np.where(ci == rows, 2.0, -1.0)
        return rp, ci, v

    def anisotropic(m):
        rp, ci, v = laplacian_arrays(m)
        L = DM.from_csr(m, m, rp, ci, v)
        I = DM.ident(m)
        II = I.kronecker(I)
        terms = [L.kronecker(II), I.kronecker(L).kronecker(I), II.kronecker(L)]
        two = terms[0].lin(WEIGHTS[0], terms[1], WEIGHTS[1])
        A = two.lin(1.0, terms[2], WEIGHTS[2])
        for h in terms + [two, II, I, L]:
            h.free()
        return A

    def closed_form(m, count):
        a = 2.0 - 2.0 * np.cos(np.arange(1, m + 1) * np.pi / (m + 1))
        low = a[:min(m, 12)]  # the smallest values use small indices only
        all_ = (WEIGHTS[0] * low[:, None, None] + WEIGHTS[1] * low[None, :, None] + WEIGHTS[2] * low[None, None, :]).ravel()
        return np.sort(all_)[:count + 1]

    deferred = []  # the CPU's turn comes last: the GPU's numbers are on disk by then

    def scipy_cell(row, S, n, nev, exact):
        try:
            import scipy.sparse.linalg as spl
        except ImportError:
            row["scipy_eigsh_arpack_on_the_cpu"] = None
            return
        t0 = time.perf_counter()
        try:
            lam = spl.eigsh(S, k=nev, which="SA", tol=1e-8, ncv=4 * nev, maxiter=args.scipy_maxiter,
                            v0=np.random.default_rng(0).standard_normal(n), return_eigenvectors=False)
            cell = {"worst_error_against_the_closed_form": float(np.max(np.abs(np.sort(lam) - exact[:nev])))}
        except spl.ArpackNoConvergence as err:
            cell = {"no_convergence": str(err)[:120]}
        cell.update(seconds=round(time.perf_counter() - t0, 2), runs=1, which="SA", ncv=4 * nev,
                    maxiter=args.scipy_maxiter, threads=os.environ.get("OMP_NUM_THREADS"))
        row["scipy_eigsh_arpack_on_the_cpu"] = cell
        print("%r" % (cell,), file=sys.stderr, flush=True)

    def whole_solves(m, with_feast):
        A = anisotropic(m)
        inf = A.info()
        n = inf["nrows_global"]
        nev = args.nev
        exact = closed_form(m, nev)
        ncv = pkg.sparse.default_ncv(n, nev)
        v0 = torch.from_numpy(np.random.default_rng(0).standard_normal(n)).cuda()
        row = {"instance": "anisotropic Laplacian %d^3 (weights %s)" % (m, list(WEIGHTS)), "n": n, "nnz": inf["nnz"],
               "nev": nev, "ncv": ncv, "tol": 1e-8, "smallest_exact": exact[:nev].tolist(),
               "relative_gap_behind_the_last": float((exact[nev] - exact[nev - 1]) / exact[nev - 1])}

        def report(t, values, res):
            values = np.sort(np.asarray(values))
            err = float(np.max(np.abs(values - exact[:len(values)]))) if len(values) else None
            return dict(t, reason=res["reason_name"], cycles=res["cycles"], applications=res["applications"],
                        pairs=res["pairs"], inner_iterations=res["inner_iterations"],
                        worst_residual=float(res["residuals"].max()) if res["pairs"] else None,
                        worst_error_against_the_closed_form=err)

        got = {}
        E = pkg.EigenSolver(A, ncv)

        def direct():
            got["d"] = E.solve(nev, "SA", 1e-8, 0.0, args.direct_restarts, v0)
        _, t = timed(direct, args.rounds)
        row["direct_SA"] = dict(report(t, got["d"][0], got["d"][2]), max_restarts=args.direct_restarts,
                                device_bytes=E.info()["device_bytes"])
        E.free()
        print("%r" % (row["direct_SA"],), file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
        setup = {}

        def make():
            setup["E"] = pkg.EigenSolver(A, ncv, sigma=0.0, M="amg", inner_rtol=1e-10, inner_maxiter=2000)
        row["inverse_setup_shift_amg_objects"] = {"ms": round(clock(make) * 1e3, 3)}
        E = setup["E"]

        def inverse():
            got["i"] = E.solve(nev, "LM", 1e-8, 0.0, 100, v0)
        _, t = timed(inverse, args.rounds)
        row["inverse_LM_sigma_0_cg_amg"] = dict(report(t, got["i"][0], got["i"][2]), inner_rtol=1e-10,
                                                amg_levels=E.inner.amg.levels)
        E.free()
        print("%r" % (row["inverse_LM_sigma_0_cg_amg"],), file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
        result.setdefault("c_whole_solves", []).append(row)
        save()
        if with_feast:
            import scipy.sparse as sp
            rp, ci, v = A.export_csr()
            S = sp.csr_matrix((v, ci, rp), shape=(n, n))
            C = sp.csc_matrix(S)
            C.sort_indices()
            host = pkg.Matrix(n, n, C.indptr, C.indices, C.data)
            interval = (0.0, float(0.5 * (exact[nev - 1] + exact[nev])))

            def feast():
                got["f"] = pkg.feast.eigSH(2 * nev, interval, host)
            _, t = timed(feast, args.rounds)
            lam = np.sort(np.asarray(got["f"][0]).real)
            row["feast_m0_%d" % (2 * nev)] = dict(t, interval=list(interval), found=int(len(lam)),
                                                  worst_error_against_the_closed_form=float(
                                                      np.max(np.abs(lam[:nev] - exact[:len(lam[:nev])]))) if len(lam) else None)
            print("%r" % (row["feast_m0_%d" % (2 * nev)],), file=sys.stderr, flush=True)
            save()
            if not args.no_scipy:
                deferred.append(lambda: scipy_cell(row, S, n, nev, exact))
        A.free()
        torch.cuda.empty_cache()

    for key in KNOBS:
        os.environ.pop(key, None)

    def part(key, run):
        """a part that is refused is recorded as such, and the others still run; a device error ends the run"""
        try:
            run()
        except (ValueError, AssertionError, pkg.SparseLinearError) as err:
            if getattr(err, "status", 0) == pkg._ffi.SPL_ERROR_device:
                raise
            result[key + "_failed"] = "%s: %s" % (type(err).__name__, err)
            print("%s failed: %r" % (key, err), file=sys.stderr, flush=True)
        save()

    if "a" in wanted:
        part("a_rotation_in_place", lambda: result.update(a_rotation_in_place=rotation_cells()))
    if "b" in wanted:
        part("b_ms_per_step", lambda: result.update(b_ms_per_step=step_cells()))
    if "c" in wanted:
        part("c_whole_solves_%d" % args.small_m3, lambda: whole_solves(args.small_m3, True))
        part("c_whole_solves_%d" % args.m3, lambda: whole_solves(args.m3, False))
        for cpu_turn in deferred:
            part("c_scipy", cpu_turn)
    print(save(), flush=True)


if __name__ == "__main__":
    main()
