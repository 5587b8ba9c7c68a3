#!/usr/bin/env python3
"""A/B record of the LU ladder (csrc/umfpack.hip: next_factors): one case per rung, `di` and `zi`, under the
environment switches that steer it.  One process per library; every observable of every call is written as one JSON
line — statuses, spl_umfpack_path before and after, spl_umfpack_stats, spl_umfpack_solve_report (without the build time
of the chains), Info[80..83], determinant / log-determinant / inertia, condest out[0..5], SHA-1 of every solution and
witness.  Floats are written with float.hex(): equal means the same bits.

  python tools/lu_ladder_ab.py record LIBRARY.so OUT.jsonl
  python tools/lu_ladder_ab.py compare PARENT_RUN1.jsonl PARENT_RUN2.jsonl CANDIDATE.jsonl

compare: what differs between the two parent runs is not bit-stable on the parent itself; there the candidate has to
lie inside the parent's spread (numbers) — everything else has to be equal.  Prints every difference; exit status 1
when there is one.  The matrices are those of tests/test_gpu_lu_from_handles.py, tests/test_gpu_umfpack.py and
tests/test_gpu_complex.py."""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SWITCHES = ("SPL_LU_METHOD", "SPL_LU_FORCE_PIVOT", "SPL_LU_BLOCK_PIVOT", "SPL_LU_STATIC_PIVOT", "SPL_LU_GMRES",
            "SPL_LU_TEST_SPECULATION_OOM", "SPL_ZI_NATIVE", "SPL_ZI_SYMMETRIC")


def _symmetric_tiny_blocks(m):
    import scipy.sparse as sp
    rng = np.random.default_rng(77)
    n = m * m
    off = np.zeros(n - 1)
    off[0::2] = 3.0
    far = rng.uniform(-0.1, 0.1, n - m)
    return sp.diags([far, off, np.full(n, 1e-14), off, far], (-m, -1, 0, 1, m), format="csc")


def _rows_in_random_order(m):
    import scipy.sparse as sp
    rng = np.random.default_rng(12)
    T = sp.diags([np.ones(m - 1), np.ones(m), np.ones(m - 1)], (-1, 0, 1))
    P = (sp.kron(sp.identity(m), T) + sp.kron(T, sp.identity(m))).tocoo()
    v = 10.0 ** rng.uniform(-3, 3, P.nnz) * rng.choice([-1.0, 1.0], P.nnz)
    perm = rng.permutation(m * m)
    return sp.csc_matrix((v, (perm[P.row], P.col)), shape=(m * m, m * m))


def _singular_mesh(H):
    import scipy.sparse as sp
    S = sp.lil_matrix(H._dominant_unsymmetric_grid(30))
    S[:, 17] = 0.0
    S[17, :] = 0.0
    S = sp.csc_matrix(S)
    S.eliminate_zeros()
    return S


def _complex_tiny_blocks(m):
    import scipy.sparse as sp
    rng = np.random.default_rng(12)
    n = m * m
    lo = np.zeros(n - 1, dtype=np.complex128)
    up = np.zeros(n - 1, dtype=np.complex128)
    lo[0::2] = 3.0
    up[0::2] = 3.0j
    d = np.where(np.arange(n) % 2 == 0, 1e-14, 1e-14j)
    far = rng.uniform(-0.1, 0.1, n - m) + 1j * rng.uniform(-0.1, 0.1, n - m)
    return sp.diags([lo, d, up, far], (-1, 0, 1, m), format="csc")


def _complex_tiny_diagonal_mesh(m):
    import scipy.sparse as sp
    rng = np.random.default_rng(31)
    T = sp.diags([np.ones(m - 1), np.ones(m), np.ones(m - 1)], (-1, 0, 1))
    S = sp.csc_matrix(sp.kron(sp.identity(m), T) + sp.kron(T, sp.identity(m)), dtype=np.complex128)
    S.data = rng.uniform(-1, 1, S.nnz) + 1j * rng.uniform(-1, 1, S.nnz)
    S.setdiag(1e-12 * (rng.uniform(0.5, 1.0, S.shape[0]) + 0j))
    return sp.csc_matrix(S)


def cases():
    import test_gpu_lu_from_handles as H
    mf = {"SPL_LU_METHOD": "mf"}
    band = {"SPL_LU_METHOD": "band"}
    real = [
        ("di_forced_pivoting", {"SPL_LU_FORCE_PIVOT": "1"}, lambda: H._dominant_unsymmetric_grid(30)),
        ("di_force0_not_dominant", dict(mf, SPL_LU_FORCE_PIVOT="0"), lambda: H._tiny_blocks(40)),
        ("di_force0_dominant", dict(mf, SPL_LU_FORCE_PIVOT="0"), lambda: H._dominant_unsymmetric_grid(45)),
        ("di_band_dominant", band, lambda: H._dominant_unsymmetric_grid(30)),
        ("di_band_speculation_holds", band, lambda: H._btb(600)),
        ("di_band_speculation_to_static", band, lambda: H._tiny_blocks(30)),
        ("di_band_speculation_to_pivoted_band", dict(band, SPL_LU_STATIC_PIVOT="0"), lambda: H._tiny_blocks(30)),
        ("di_tree_dominant", mf, lambda: H._dominant_unsymmetric_grid(45)),
        ("di_tree_ldlt_holds", mf, lambda: H._btb(600)),
        ("di_tree_block_pivoting_holds", mf, lambda: H._tiny_blocks(40)),
        ("di_tree_ldlt_block_pivot_retry", mf, lambda: _symmetric_tiny_blocks(48)),
        ("di_tree_ldlt_no_retry_to_static", dict(mf, SPL_LU_BLOCK_PIVOT="0"), lambda: _symmetric_tiny_blocks(48)),
        ("di_tree_no_block_pivot_to_static", dict(mf, SPL_LU_BLOCK_PIVOT="0"), lambda: H._tiny_blocks(40)),
        ("di_tree_block_pivot_to_static", mf, lambda: H._tiny_diagonal_mesh(300)),
        ("di_tree_to_pivoted_band", dict(mf, SPL_LU_STATIC_PIVOT="0"), lambda: H._tiny_diagonal_mesh(60)),
        ("di_speculation_oom_static_polish", dict(mf, SPL_LU_TEST_SPECULATION_OOM="1"), lambda: _rows_in_random_order(280)),
        ("di_speculation_oom_no_gmres", dict(mf, SPL_LU_TEST_SPECULATION_OOM="1", SPL_LU_GMRES="0"),
         lambda: _rows_in_random_order(40)),
        ("di_speculation_oom_no_static", dict(mf, SPL_LU_TEST_SPECULATION_OOM="1", SPL_LU_STATIC_PIVOT="0"),
         lambda: _rows_in_random_order(40)),
        ("di_singular", mf, lambda: _singular_mesh(H)),
    ]
    native = dict(mf, SPL_ZI_NATIVE="1")
    cplx = [("zi_" + name, env, build) for name, env, build in H._COMPLEX_CASES]
    cplx += [
        ("zi_plain_embedding_tree", dict(mf, SPL_ZI_NATIVE="0", SPL_ZI_SYMMETRIC="0"), lambda: H._complex_shift(13)),
        ("zi_native_block_pivoting", native, lambda: _complex_tiny_blocks(40)),
        ("zi_native_to_static", native, lambda: _complex_tiny_diagonal_mesh(44)),
        ("zi_native_no_block_pivot_to_static", dict(native, SPL_LU_BLOCK_PIVOT="0"), lambda: _complex_tiny_diagonal_mesh(44)),
        ("zi_embedding_to_static", dict(mf, SPL_ZI_NATIVE="0"), lambda: _complex_tiny_diagonal_mesh(44)),
        ("zi_native_to_pivoted_band", dict(native, SPL_LU_STATIC_PIVOT="0"), lambda: _complex_tiny_diagonal_mesh(30)),
    ]
    return real + cplx


def _hex(v):
    if isinstance(v, float):
        return v.hex()
    if isinstance(v, dict):
        return {k: _hex(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_hex(x) for x in v]
    if isinstance(v, (np.floating,)):
        return float(v).hex()
    if isinstance(v, (np.integer,)):
        return int(v)
    return v


def _sha(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


def record(lib_path, out_path):
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    pkg._ffi.LIB_PATH = os.path.abspath(lib_path)
    torch.cuda.set_device(0)
    U = pkg.umfpack
    L = U._declare()
    out = open(out_path, "w")

    def state(f):
        rep = dict(f.solve_report)
        rep.pop("chain_build_ms")  # a time
        return {"path": f.path, "stats": f.stats, "report": rep}

    def emit(case, obj, step, f, **kw):
        row = {"case": case, "object": obj, "step": step}
        row.update(_hex(kw))
        row.update(_hex(state(f)))
        out.write(json.dumps(row, sort_keys=True) + "\n")
        out.flush()

    def solve1(f, M, mode, b):
        """one column through umfpack_{di,zi}_solve with Info"""
        nr, nc, ap, ai, ax = M._tuple32()
        info = (C.c_double * 90)()
        if M.is_complex:
            b = np.ascontiguousarray(b, dtype=np.complex128)
            x = np.zeros(nc, dtype=np.complex128)
            st = L.umfpack_zi_solve(int(mode), U.p_i32(ap), U.p_i32(ai), U.p_f64(ax), None, U.p_f64(x.view(np.float64)), None,
                                    U.p_f64(b.view(np.float64)), None, f.value, None, info)
        else:
            b = np.ascontiguousarray(b, dtype=np.float64)
            x = np.zeros(nc)
            st = L.umfpack_di_solve(int(mode), U.p_i32(ap), U.p_i32(ai), U.p_f64(ax), U.p_f64(x), U.p_f64(b), f.value, None, info)
        return {"status": st, "info": [info[0], info[80], info[81], info[82], info[83]], "sha1": _sha(x)}

    def solve_many(f, M, mode, Bs):
        try:
            X = U.linearSolveMany_(f, mode, M, list(Bs))
            return {"status": "ok", "sha1": [_sha(x) for x in X]}
        except U.UmfpackError as e:
            return {"status": str(e)}

    def determinants(f):
        res = {}
        for name, fn in (("determinant", U.determinant), ("logDeterminant", U.logDeterminant), ("inertia", U.inertia)):
            try:
                res[name] = list(fn(f))
            except U.UmfpackError as e:
                res[name] = "error: %s" % e
        return res

    def condest(f, M, norm):
        try:
            r = U.conditionEstimate(f, M, norm=norm, t=2)
        except U.UmfpackError as e:
            return {"status": str(e)}
        w = r.pop("witness")
        r["witness_sha1"] = _sha(w) if w is not None else None
        return r

    for name, env, build in cases():
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(env)
        S = build().tocsc()
        S.sort_indices()
        n = S.shape[0]
        M = pkg.Matrix(n, n, S.indptr.astype(np.int32), S.indices.astype(np.int32), S.data)
        cplx = bool(M.is_complex)
        rng = np.random.default_rng(3)

        def rhs():
            return rng.normal(size=n) + (1j * rng.normal(size=n) if cplx else 0.0)
        b1, bt = rhs(), rhs()
        # five columns of which only some need refinement: two random ones, one with a single entry, A times ones (an
        # exactly representable solution), one scaled by 1e8
        e7 = np.zeros(n, dtype=S.dtype)
        e7[7 % n] = 1.0
        B5 = [rhs(), np.asarray(S @ np.ones(n)).ravel(), e7, rhs(), 1e8 * rhs()]
        an = U.analyze(M)
        # object 1: the determinant (its acceptance check) meets the fresh factors, then a solve
        f = U.factor(M, an)
        emit(name, 1, "factor", f, status=f.status)
        if not cplx:
            emit(name, 1, "determinant_fresh", f, **determinants(f))
        emit(name, 1, "solve_A", f, **solve1(f, M, U.UmfpackNormal, b1))
        del f
        # object 2: solves first
        f = U.factor(M, an)
        emit(name, 2, "factor", f, status=f.status)
        emit(name, 2, "solve_A", f, **solve1(f, M, U.UmfpackNormal, b1))
        emit(name, 2, "solve_many_At_5", f, **solve_many(f, M, U.UmfpackTrans, B5))
        emit(name, 2, "solve_many_A_5", f, **solve_many(f, M, U.UmfpackNormal, B5))
        emit(name, 2, "condest_1", f, **condest(f, M, 1))
        emit(name, 2, "condest_inf", f, **condest(f, M, np.inf))
        if not cplx:
            emit(name, 2, "determinant_after", f, **determinants(f))
        emit(name, 2, "solve_At", f, **solve1(f, M, U.UmfpackTrans, bt))
        del f
        # object 3: the transposed system is the first to check the factors
        f = U.factor(M, an)
        emit(name, 3, "solve_At", f, **solve1(f, M, U.UmfpackTrans, bt))
        emit(name, 3, "solve_A", f, **solve1(f, M, U.UmfpackNormal, b1))
        del f
        print("recorded", name, flush=True)
    out.close()


def _load(path):
    rows = {}
    for line in open(path):
        r = json.loads(line)
        rows[(r["case"], r["object"], r["step"])] = r
    return rows


def _flat(v, prefix=""):
    if isinstance(v, dict):
        for k, x in v.items():
            yield from _flat(x, prefix + "." + k if prefix else k)
    elif isinstance(v, list):
        for i, x in enumerate(v):
            yield from _flat(x, "%s[%d]" % (prefix, i))
    else:
        yield prefix, v


def _num(v):
    try:
        return float.fromhex(v) if isinstance(v, str) else float(v)
    except (ValueError, TypeError):
        return None


def compare(p1, p2, cand):
    A, B, Cn = _load(p1), _load(p2), _load(cand)
    differences = unstable = 0
    for key in sorted(set(A) | set(Cn)):
        if key not in A or key not in Cn or key not in B:
            print("MISSING", key)
            differences += 1
            continue
        a, b, c = dict(_flat(A[key])), dict(_flat(B[key])), dict(_flat(Cn[key]))
        for field in sorted(set(a) | set(c)):
            va, vb, vc = a.get(field), b.get(field), c.get(field)
            if va == vb:
                if vc != va:
                    print("DIFFERENT %s %s: parent %r candidate %r" % (key, field, va, vc))
                    differences += 1
                continue
            unstable += 1
            na, nb, nc = _num(va), _num(vb), _num(vc)
            inside = None not in (na, nb, nc) and min(na, nb) <= nc <= max(na, nb)
            print("parent not bit-stable %s %s: %r / %r, candidate %r%s" % (key, field, va, vb, vc, "" if inside or vc in (va, vb) else "  OUTSIDE"))
            if not (inside or vc in (va, vb)):
                differences += 1
    print("%d records, %d fields the parent does not reproduce itself, %d differences" % (len(A), unstable, differences))
    return 1 if differences else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "record":
        record(sys.argv[2], sys.argv[3])
    elif len(sys.argv) == 5 and sys.argv[1] == "compare":
        sys.exit(compare(*sys.argv[2:]))
    else:
        sys.exit(__doc__)
