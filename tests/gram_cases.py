"""Inputs and the yardstick of tests/test_gpu_gram.py and tests/test_gram_cpu.py: serial restatements of
spl_vector_gram_dev and spl_vector_rotate_z_dev as include/sparse_linear_hip.h states them, built from the fold and the
two arithmetics of tests/krylov_cases.py.  They never run code of the library under test.

  * gram: every entry is krylov_cases.dot of its two columns.  The fold is done for all columns of V at once (the same
    sums row by row: numpy rounds each row's operations on their own), which is checked against krylov_cases.fold in
    tests/test_gram_cpu.py;
  * rotate_z: column i is x = Y[0][i] v_0; x = x + Y[l][i] v_l ascending with Data.Complex's product, four products, a
    difference and a sum per term, then one sum per part.

`python tests/gram_cases.py` prints what the committed shapes are, without a GPU."""
import numpy as np

import krylov_cases as K

LENGTHS = (0, 1, 255, 256, 257, 4095, 4096, 4097, 3 * 4096 + 5)
WIDTHS = ((1, 1), (2, 1), (3, 2), (5, 127), (30, 30), (128, 128))
WIDE_UP_TO = 4097  # the last two widths run at n <= 4097 only
TILES = ("1", "2", "4")


def fold_many(P):
    """krylov_cases.fold of every row of P (rows x length): one value per row"""
    P = np.ascontiguousarray(P, dtype=np.float64)
    rows = P.shape[0]
    if P.shape[1] == 0:
        return np.zeros(rows)
    with np.errstate(all="ignore"):
        while True:
            length = P.shape[1]
            nchunks = -(-length // K.CHUNK)
            padded = np.zeros((rows, nchunks * K.CHUNK))
            padded[:, :length] = P
            steps = padded.reshape(rows, nchunks, K.CHUNK // K.LANES, K.LANES)
            s = np.zeros((rows, nchunks, K.LANES))
            for k in range(K.CHUNK // K.LANES):
                s = s + steps[:, :, k, :]
            h = K.LANES // 2
            while h >= 1:
                s[:, :, :h] = s[:, :, :h] + s[:, :, h:2 * h]
                h //= 2
            P = np.ascontiguousarray(s[:, :, 0])
            if P.shape[1] == 1:
                return P[:, 0].copy()


def gram(V, W):
    """G[i][j] = <V[:, i], W[:, j]> as the device computes it: V n x k, W n x l, float64 or complex128"""
    V, W = np.asarray(V), np.asarray(W)
    k, l = V.shape[1], W.shape[1]
    cplx = np.iscomplexobj(V)
    G = np.zeros((k, l), dtype=np.complex128 if cplx else np.float64)
    Vt = np.ascontiguousarray(V.T)
    with np.errstate(all="ignore"):
        for j in range(l):
            w = W[:, j][None, :]
            if cplx:
                ar, ai, br, bi = Vt.real, -Vt.imag, w.real, w.imag  # Data.Complex's product on conj(v) and w
                G[:, j].real = fold_many(ar * br - ai * bi)
                G[:, j].imag = fold_many(ar * bi + ai * br)
            else:
                G[:, j] = fold_many(Vt * w)
    return G


def rotate_z(V, Y):
    """V Y: V an n x m complex128 array, Y a COMPLEX m x k array; all columns at once, term by term"""
    V, Y = np.asarray(V, dtype=np.complex128), np.asarray(Y, dtype=np.complex128)
    m = V.shape[1]
    c, d = np.ascontiguousarray(V.real), np.ascontiguousarray(V.imag)
    a, b = np.ascontiguousarray(Y.real), np.ascontiguousarray(Y.imag)
    with np.errstate(all="ignore"):
        xr = c[:, 0:1] * a[0:1, :] - d[:, 0:1] * b[0:1, :]
        xi = d[:, 0:1] * a[0:1, :] + c[:, 0:1] * b[0:1, :]
        for l in range(1, m):
            xr = xr + (a[l:l + 1, :] * c[:, l:l + 1] - b[l:l + 1, :] * d[:, l:l + 1])
            xi = xi + (a[l:l + 1, :] * d[:, l:l + 1] + b[l:l + 1, :] * c[:, l:l + 1])
    out = np.empty(xr.shape, dtype=np.complex128)
    out.real, out.imag = xr, xi
    return out


def blocks(n, k, l, cplx):
    """V (n x k) and W (n x l) of krylov_cases.dot_inputs data: column i of W is the cancelling partner of column i of V,
    and -0.0, the smallest subnormal and 1e300 stand among ordinary numbers.  Narrower blocks are the first columns of
    wider ones"""
    cols_v, cols_w = [], []
    for i in range(max(k, l)):
        a, b = K.dot_inputs(n, cplx, seed=1 + i)
        if i < k:
            cols_v.append(a)
        if i < l:
            cols_w.append(b)
    dtype = np.complex128 if cplx else np.float64
    V = np.stack(cols_v, axis=1).astype(dtype) if n else np.zeros((0, k), dtype=dtype)
    W = np.stack(cols_w, axis=1).astype(dtype) if n else np.zeros((0, l), dtype=dtype)
    if n > 0:
        V[0, 0] = -0.0
    if n > 2:
        V[1, 0], W[1, 0] = 5e-324, 1e-3
        V[2, 0], W[2, 0] = 1e300, 1e-300
    return V, W


if __name__ == "__main__":
    import time
    for cplx in (False, True):
        for n in LENGTHS:
            for k, l in WIDTHS:
                if (k, l) in WIDTHS[-2:] and n > WIDE_UP_TO:
                    continue
                t0 = time.time()
                V, W = blocks(n, k, l, cplx)
                G = gram(V, W)
                print("%-7s n %6d  k %3d  l %3d  |G|_max %.3e  finite %s  %.2f s"
                      % ("complex" if cplx else "real", n, k, l, np.abs(G).max() if G.size else 0.0,
                         bool(np.isfinite(G.view(np.float64)).all()), time.time() - t0))
