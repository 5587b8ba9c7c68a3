"""The yardstick of tests/test_gpu_globpcg.py and tests/test_globpcg_cpu.py: a serial restatement of "The generalized
problem A x = lambda B x" in the section "LOBPCG on handles" of include/sparse_linear_hip.h, in the style of
tests/lobpcg_cases.py and built from its pieces: the method of that file in the inner product <u,v>_B = <u, B v>, with
B S kept beside S and A S.  It never runs code of the library under test.

Every product, sum, quotient and root is one separately rounded IEEE operation.  With B an identity every quantity is
lobpcg_cases.lobpcg's bit for bit (but for the sign of a zero).  `python tests/globpcg_cases.py` prints reason,
iterations, drops and sweeps of every committed case and the B-orthonormality figures, without a GPU."""
import functools
import math

import numpy as np
import scipy.sparse as sp

import eigsh_cases as EK
import gmres_cases as G
import gram_cases as GK
import krylov_cases as K
import lobpcg_cases as LK

REASONS, LARGEST, SMALLEST, DROP_RATIO = LK.REASONS, LK.LARGEST, LK.SMALLEST, LK.DROP_RATIO
_root = EK._root


class Outcome(LK.Outcome):
    """lobpcg_cases.Outcome with the columns multiplied by B"""
    mass_columns = 0


def update_pair(V, BV, coef, w, bw, A):
    """(w, bw, Re<w, bw>) of spl_vector_update_pair_dev: w = ((w - c_0 v_0) - c_1 v_1) - ... and the same on bw with the
    columns of BV, a product and a difference per term; V, BV: lists of columns"""
    for i in range(len(coef)):
        w = w - A.scaled(coef[i], V[i])
        bw = bw - A.scaled(coef[i], BV[i])
    return w, bw, A.real(A.dot(w, bw))


def lobpcg(S, Bm, X0, nev, which=SMALLEST, tol=1e-8, atol=0.0, max_iter=200, M=None):
    """the header's sequence for S x = lambda Bm x (scipy matrices or callable operators) from the start block X0
    (n x block); M: None or a callable r -> M^-1 r"""
    A_op = S if callable(S) else K.RowSerial(S)
    B_op = Bm if callable(Bm) else K.RowSerial(Bm)
    X0 = np.asarray(X0)
    cplx = np.iscomplexobj(X0)
    Z = G._Complex if cplx else G._Real
    with np.errstate(all="ignore"):
        return _lobpcg(A_op, B_op, X0.astype(Z.A.dtype), nev, which, tol, atol, max_iter, M, Z, Z.A, cplx)


def _lobpcg(A_op, B_op, X0, nev, which, tol, atol, max_iter, M, Z, A, cplx):
    n, b = X0.shape
    st = {"it": 0, "spmv": 0, "mass": 0, "apps": 0, "sweeps": 0, "dropped": 0, "syncs": 0}
    history = []
    zero = np.zeros(n, dtype=A.dtype)
    cols = [np.ascontiguousarray(X0[:, j]) for j in range(b)] + [zero.copy() for _ in range(2 * b)]
    image = [zero.copy() for _ in range(3 * b)]
    mass = [zero.copy() for _ in range(3 * b)]  # B S
    flags = [0] * (3 * b)
    theta = [0.0] * b

    def done(reason, values=(), vectors=None, residuals=()):
        vectors = np.zeros((n, 0), dtype=A.dtype) if vectors is None else vectors
        out = Outcome(reason, st["it"], st["spmv"], st["apps"], st["sweeps"], st["dropped"], st["syncs"], values, vectors,
                      residuals, history)
        out.mass_columns = st["mass"]
        return out

    def norm(v):
        return _root(A.real(A.dot(v, v)))

    def settle(c, with_image=False):
        w, bw = cols[c], mass[c]
        q0 = A.real(A.dot(w, bw))
        q2 = None
        passes = []
        if c > 0:
            for _ in range(2):
                coef = [A.dot(mass[i], w) for i in range(c)]
                passes.append(coef)
                w, bw, q2 = update_pair(cols[:c], mass[:c], coef, w, bw, A)
        else:
            q2 = A.real(A.dot(w, bw))
        eta2 = float("nan")
        if not (math.isfinite(q0) and math.isfinite(q2)):
            flags[c] = 2
        elif q0 < 0.0 or q2 < 0.0:
            flags[c] = 1
        else:
            eta0, eta2 = _root(q0), _root(q2)
            flags[c] = 1 if (eta2 == 0.0 or eta2 <= DROP_RATIO * eta0) else 0
        cols[c] = zero.copy() if flags[c] else Z.vector_over(w, eta2)
        mass[c] = zero.copy() if flags[c] else Z.vector_over(bw, eta2)
        if with_image:  # A x_c receives the same coefficients, the same division and the same zeros
            v = image[c]
            for coef in passes:
                for i in range(c):
                    v = v - A.scaled(coef[i], image[i])
            image[c] = zero.copy() if flags[c] else Z.vector_over(v, eta2)

    def close(mc, kout, count_from):
        """None: go on; else the reason that ends the solve"""
        st["syncs"] += 1
        kept = []
        for j in range(mc):
            if flags[j] == 2 or (j < b and flags[j] != 0):
                return 3
            if flags[j] == 0:
                kept.append(j)
            elif j >= count_from:
                st["dropped"] += 1
        mp = len(kept)
        Tr = [[0.0] * mp for _ in range(mp)]
        Ti = [[0.0] * mp for _ in range(mp)]
        for a in range(mp):
            for c in range(a, mp):
                g = A.dot(cols[kept[a]], image[kept[c]])
                gr, gi = (g[0], 0.0 if a == c else g[1]) if cplx else (g, 0.0)
                if not (math.isfinite(gr) and math.isfinite(gi)):
                    return 3
                Tr[a][c] = Tr[c][a] = gr
                Ti[a][c] = gi
                Ti[c][a] = 0.0 if a == c else -gi
        if cplx:
            solved = LK.jacobi_hermitian(Tr, Ti)
            if solved is None:
                return 3
            values, Yr, Yi, sweeps = solved
        else:
            solved = EK.jacobi(Tr)
            if solved is None:
                return 3
            values, Yr, sweeps = solved
            Yi = [[0.0] * mp for _ in range(mp)]
        if not LK._finite(values) or not all(LK._finite(row) for row in Yr) or not all(LK._finite(row) for row in Yi):
            return 3
        st["sweeps"] = max(st["sweeps"], sweeps)
        order = EK.ordered(values, which)
        Zm = np.zeros((mc, kout), dtype=A.dtype)
        for i in range(kout):
            col = order[i if i < b else i - b]
            for a in range(mp):
                if i >= b and kept[a] < b:
                    continue
                Zm[kept[a], i] = complex(Yr[a][col], Yi[a][col]) if cplx else Yr[a][col]
        rotate = GK.rotate_z if cplx else EK.rotate
        new_s = rotate(np.stack(cols[:mc], axis=1), Zm)
        new_i = rotate(np.stack(image[:mc], axis=1), Zm)
        new_m = rotate(np.stack(mass[:mc], axis=1), Zm)
        for i in range(kout):
            cols[i] = np.ascontiguousarray(new_s[:, i])
            image[i] = np.ascontiguousarray(new_i[:, i])
            mass[i] = np.ascontiguousarray(new_m[:, i])
        for i in range(b):
            theta[i] = values[order[i]]
        for j in range(b):  # X' is settled again, A X' and B X' with it
            settle(j, True)
        return None

    def finish(reason):
        values, residuals = [], []
        for i in range(nev):
            r = A_op(cols[i]) - EK.real_times(theta[i], B_op(cols[i]))
            st["spmv"] += 1
            st["mass"] += 1
            values.append(theta[i])
            residuals.append(norm(r))
        st["syncs"] += 1
        return done(reason, values, np.stack(cols[:nev], axis=1), residuals)

    # ---- start
    for j in range(b):
        mass[j] = B_op(cols[j])
    st["mass"] += b
    for j in range(b):
        settle(j)
    st["syncs"] += 1
    if any(flags[j] == 2 for j in range(b)):
        return done(3)
    if any(flags[j] == 1 for j in range(b)):
        return done(2)
    for j in range(b):
        image[j] = A_op(cols[j])
    st["spmv"] += b
    reason = close(b, b, b)
    if reason is not None:
        return done(reason)
    it = 0
    while True:
        st["it"] = it
        R = [image[i] - EK.real_times(theta[i], mass[i]) for i in range(b)]
        rho = [norm(r) for r in R]
        st["syncs"] += 1
        if not LK._finite(rho):
            return done(3)
        worst = 0.0
        for i in range(nev):
            if rho[i] > worst:
                worst = rho[i]
        history.append(worst)
        if all(rho[i] <= max(tol * abs(theta[i]), atol) for i in range(nev)):
            return finish(0)
        if it >= max_iter:
            return finish(1)
        for i in range(b):
            if M is None:
                cols[2 * b + i] = R[i]
            else:
                cols[2 * b + i] = np.ascontiguousarray(M(R[i]))
                st["apps"] += 1
        for i in range(b):
            mass[2 * b + i] = B_op(cols[2 * b + i])
        st["mass"] += b
        for c in range(b, 3 * b):
            settle(c)
        for c in range(b, 3 * b):
            image[c] = A_op(cols[c])
        st["spmv"] += 2 * b
        reason = close(3 * b, 2 * b, 2 * b if it == 0 else b)
        st["it"] = it + 1
        if reason is not None:
            return done(reason)
        it += 1


# ---- the committed cases ---------------------------------------------------------------------------------------------------
def _tri141(m):
    return sp.diags([np.ones(m - 1), 4.0 * np.ones(m), np.ones(m - 1)], [-1, 0, 1], format="csr")


def mass2d(m):
    """kron(T, T), T = tridiag(1, 4, 1): the entries 16, 4 and 1 are exact and every eigenvalue lies in (4, 36)"""
    return LK._csr(sp.kron(_tri141(m), _tri141(m)))


def mass3d(m):
    return LK._csr(sp.kron(sp.kron(_tri141(m), _tri141(m)), _tri141(m)))


@functools.lru_cache(maxsize=None)
def mass(name):
    if name == "mass12":
        return mass2d(12)
    if name == "phased_mass12":  # complex Hermitian, with phases of its own
        return LK.phased(mass2d(12), seed=23)
    if name == "mass70":
        return mass2d(70)
    if name == "mass8_3d":  # to go with poisson8
        return mass3d(8)
    if name == "diag21":  # to go with "two"
        return LK._csr(np.array([[2.0, 0.0], [0.0, 1.0]]))
    raise KeyError(name)


def identity(n, cplx=False):
    return LK._csr(sp.identity(n, dtype=np.complex128 if cplx else np.float64, format="csr"))


# (A, B, block, nev, which, tol, max_iter): every one a bit test on the device; all but grid70 reach reason 0
CASES = (("poisson12", "mass12", 6, 4, SMALLEST, 1e-9, 200), ("phased12", "phased_mass12", 6, 4, SMALLEST, 1e-9, 200),
         ("poisson12", "mass12", 4, 2, LARGEST, 1e-9, 200), ("two", "diag21", 1, 1, SMALLEST, 1e-10, 50),
         ("grid70", "mass70", 4, 2, SMALLEST, 1e-9, 3))
# (preconditioner of A, block, nev, tol, max_iter) on (poisson8, mass8_3d), smallest; "amg" is restated on the levels the
# device exports
PRECONDITIONED = (("jacobi", 4, 3, 1e-8, 200), ("amg", 4, 3, 1e-8, 200))


@functools.lru_cache(maxsize=None)
def reference(name, bname, block, nev, which, tol, max_iter, kind=None):
    S = LK.matrix(name)
    M = None if kind is None else K.preconditioner(S, kind)
    out = lobpcg(S, mass(bname), LK.start_of(name, block), nev, which, tol, 0.0, max_iter, M)
    for a in (out.values, out.vectors, out.residuals, out.history):
        a.setflags(write=False)
    return out


def b_orthonormality(out, Bm):
    """max |X^H B X - I| of the vectors returned"""
    X = out.vectors
    return float(np.abs(X.conj().T @ (Bm @ X) - np.eye(out.pairs)).max()) if out.pairs else float("nan")


if __name__ == "__main__":  # what every committed case does: checked here, without a GPU
    import time

    def show(label, out, Bm, t0):
        print("%-34s reason %-10s iterations %3d  drops %3d  sweeps %2d  spmv columns %4d  mass columns %4d  applications"
              " %4d  residual %.2e  |X^H B X - I| %.1e  %.2f s"
              % (label, REASONS[out.reason], out.iterations, out.dropped, out.sweeps, out.spmv_columns, out.mass_columns,
                 out.applications, out.residuals.max() if out.pairs else float("nan"), b_orthonormality(out, Bm),
                 time.time() - t0))

    for case in CASES:
        t0 = time.time()
        show("%s %s b%d nev%d w%d" % case[:5], reference(*case), mass(case[1]), t0)
    for kind, block, nev, tol, max_iter in PRECONDITIONED:
        if kind == "amg":
            continue
        t0 = time.time()
        show("poisson8 mass8_3d %s" % kind, reference("poisson8", "mass8_3d", block, nev, SMALLEST, tol, max_iter, kind),
             mass("mass8_3d"), t0)
    # B-orthonormality beside the orthonormality of the standard restatement on the same A, block and start
    for name, bname, block, nev, which, tol, max_iter in CASES:
        if name == "grid70":
            continue
        std = LK.reference(name, block, nev, which, tol, max_iter)
        gen = reference(name, bname, block, nev, which, tol, max_iter)
        plain = float(np.abs(std.vectors.conj().T @ std.vectors - np.eye(std.pairs)).max())
        kappa = float(np.linalg.cond(mass(bname).toarray()))
        print("%-10s %-14s block %d: |X^H B X - I| %.3e   standard |X^H X - I| %.3e   kappa_2(B) %.3f   bound %.3e"
              % (name, bname, block, b_orthonormality(gen, mass(bname)), plain, kappa, 16.0 * kappa * plain))
