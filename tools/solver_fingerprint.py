#!/usr/bin/env python3
"""One sha256 per case over the raw bytes the iterative solvers on device handles return, for comparing two builds of
the library bit for bit (a refactor of the host side must not move one).

  CG               2-D Poisson 12 x 12: no preconditioner, jacobi, sgs, ILU(0), amg
  BiCGSTAB         convection-diffusion 12 x 12 (not symmetric): no preconditioner, ILU(0)
  GMRES(5), (30)   the same: no preconditioner, ILU(0), amg
  eigsh            2-D Poisson 12 x 12: 'LA', 'SA', and shift-invert about sigma (with and without jacobi inside)
  lobpcg           the same matrix: block 4, 3 pairs, smallest and largest: no preconditioner, jacobi, amg; and the
                   smallest pairs with the 9-point mass matrix (a build without spl_lobpcg_set_mass has no such case)

Every case real and complex (the Poisson matrix with Hermitian imaginary off-diagonals, the other with complex
convection), right-hand sides and starts from a fixed seed.  A linear case hashes x, the history and the integer
results, the reason among them (GMRES: its two residuals too); an eigsh case the values, the vectors, the residuals,
the history and the integer results; its "+launches" twin and every lobpcg case also info()["launches"] after the
solve.  The "dev" cases go through solve_dev with torch tensors.

python tools/solver_fingerprint.py [--lib path/to/libsparse_linear_hip.so] [--out file.json]
Prints one JSON object {case: sha256}; two builds agree when the two objects are equal."""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

M = 12
SEED = 20240607


def grid_matrix(np, sp, cplx, convection):
    """5-point stencil on an M x M grid; convection: upwind first-order terms that break the symmetry"""
    n = M * M
    rows, cols, vals = [], [], []
    wx, wy = (0.75, 0.4) if convection else (0.0, 0.0)
    twist = 0.1j if cplx else 0.0
    for i in range(M):
        for j in range(M):
            r = i * M + j
            rows.append(r), cols.append(r), vals.append(4.0 + wx + wy + (0.0j if cplx else 0.0))
            for di, dj, w in ((-1, 0, -1.0 - wx), (1, 0, -1.0), (0, -1, -1.0 - wy), (0, 1, -1.0)):
                a, b = i + di, j + dj
                if 0 <= a < M and 0 <= b < M:
                    c = a * M + b
                    v = w + (twist if c > r else -twist)  # Hermitian when there is no convection
                    if convection and cplx:
                        v = v + 0.1j * (di + dj)
                    rows.append(r), cols.append(c), vals.append(v)
    S = sp.csc_matrix((np.array(vals), (rows, cols)), shape=(n, n))
    S.sort_indices()
    return S


def handle_of(pkg, np, S):
    Mx = pkg.Matrix(S.shape[1], S.shape[0], S.indptr, S.indices, S.data)
    return pkg.DeviceMatrix.from_csc_complex(Mx) if np.iscomplexobj(S.data) else pkg.DeviceMatrix.from_csc(Mx)


def digest(np, *arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="the shared library to load instead of the package's own")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import scipy.sparse as sp
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    if args.lib:
        pkg._ffi.LIB_PATH = os.path.abspath(args.lib)
    assert torch.cuda.is_available(), "the fingerprint needs the GPU"
    torch.cuda.set_device(0)
    I64 = np.int64
    out = {}
    for cplx in (False, True):
        kind = "complex" if cplx else "real"
        rng = np.random.default_rng(SEED)
        n = M * M
        b = rng.standard_normal(n) + (1j * rng.standard_normal(n) if cplx else 0.0)
        x0 = rng.standard_normal(n) + (1j * rng.standard_normal(n) if cplx else 0.0)
        spd = handle_of(pkg, np, grid_matrix(np, sp, cplx, False))
        uns = handle_of(pkg, np, grid_matrix(np, sp, cplx, True))

        def linear(label, solver, start=None):
            x, res = solver.solve(b, start, rtol=1e-10, maxiter=400)
            ints = [res[k] for k in ("iterations", "reason", "spmvs", "preconditioner_applications")]
            floats = []
            if "cycles" in res:
                ints.append(res["cycles"])
                floats = [res["residual"], res["estimate"]]
            out["%s %s" % (label, kind)] = digest(np, x, res["history"], np.array(ints, dtype=I64), np.array(floats))
            solver.free()

        def preconditioner(H, name):  # amg: three levels on 144 rows
            return H.ilu0() if name == "ilu0" else H.amg(coarse_size=16) if name == "amg" else name

        for name in (None, "jacobi", "sgs", "ilu0", "amg"):
            linear("cg %s" % name, spd.krylov("cg", preconditioner(spd, name)))
        linear("cg None x0", spd.krylov("cg", None), x0)
        for name in (None, "ilu0"):
            linear("bicgstab %s" % name, uns.krylov("bicgstab", preconditioner(uns, name)))
        for restart in (5, 30):
            for name in (None, "ilu0", "amg"):
                linear("gmres(%d) %s" % (restart, name), uns.gmres(restart, preconditioner(uns, name)))
        linear("gmres(5) None x0", uns.gmres(5, None), x0)

        def eigen_digest(res, values, vectors, *more):
            ints = [res[k] for k in res if isinstance(res[k], int) and not isinstance(res[k], bool)] + list(more)
            return digest(np, values, vectors, res["residuals"], res["history"], np.array(ints, dtype=I64))

        def eigen(label, which, sigma=None, M=None):
            E = pkg.EigenSolver(spd, 12, sigma, M)
            values, vectors, res = E.solve(3, which, 1e-10, 0.0, 200)
            out["%s %s" % (label, kind)] = eigen_digest(res, values, vectors)
            out["%s +launches %s" % (label, kind)] = eigen_digest(res, values, vectors, E.info()["launches"])
            E.free()

        eigen("eigsh LA", "LA")
        eigen("eigsh SA", "SA")
        eigen("eigsh sigma=0.05 LM", "LM", 0.05)  # below the spectrum: the inner CG stays positive definite
        eigen("eigsh sigma=0.05 LM jacobi", "LM", 0.05, "jacobi")

        X0 = rng.standard_normal((n, 4)) + (1j * rng.standard_normal((n, 4)) if cplx else 0.0)
        for name in (None, "jacobi", "amg"):
            for largest in (False, True):
                L = pkg.LOBPCGSolver(spd, 4, preconditioner(spd, name))
                values, vectors, res = L.solve(X0, 3, largest, 1e-8, 0.0, 200)
                out["lobpcg %s %s %s" % (name, "largest" if largest else "smallest", kind)] = eigen_digest(
                    res, values, vectors, L.info()["launches"])
                L.free()

        # the generalized problem: the 9-point mass matrix kron(T, T), T = tridiag(1, 4, 1), beside the same operator
        if hasattr(pkg._ffi.lib(), "spl_lobpcg_set_mass"):  # --lib may name an older build
            T = sp.diags([np.ones(M - 1), 4.0 * np.ones(M), np.ones(M - 1)], [-1, 0, 1])
            mass = sp.csc_matrix(sp.kron(T, T)).astype(np.complex128 if cplx else np.float64)
            mass.sort_indices()
            L = pkg.LOBPCGSolver(spd, 4, None, handle_of(pkg, np, mass))
            values, vectors, res = L.solve(X0, 3, False, 1e-8, 0.0, 200)
            out["lobpcg None smallest mass %s" % kind] = eigen_digest(res, values, vectors, L.info()["launches"],
                                                                      L.info()["mass_columns"])
            L.free()

        # the same two solvers through solve_dev, on torch tensors and torch's current stream
        stream = torch.cuda.current_stream().cuda_stream
        dX0 = torch.from_numpy(np.ascontiguousarray(X0.T)).cuda()
        dX = torch.zeros((3, n), dtype=dX0.dtype, device="cuda")
        E = pkg.EigenSolver(spd, 12)
        values, res = E.solve_dev(3, dX0.data_ptr(), dX.data_ptr(), n, "SA", 1e-10, 0.0, 200, True, stream)
        out["eigsh SA dev %s" % kind] = eigen_digest(res, values, dX.cpu().numpy(), E.info()["launches"])
        E.free()
        L = pkg.LOBPCGSolver(spd, 4, "jacobi")
        values, res = L.solve_dev(3, dX0.data_ptr(), n, dX.data_ptr(), n, False, 1e-8, 0.0, 200, True, stream)
        out["lobpcg jacobi smallest dev %s" % kind] = eigen_digest(res, values, dX.cpu().numpy(), L.info()["launches"])
        L.free()
    text = json.dumps(out, indent=1, sort_keys=True)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
