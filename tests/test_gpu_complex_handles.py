"""Complex device handles through the structural half of the handle family: spl_matrix_transpose and
spl_matrix_spgemm on complex handles, and the new spl_matrix_ctrans / spl_matrix_hermitian on real and complex ones.

Inputs and truths come from tests/complex_handle_cases.py (their properties: tests/test_complex_handle_cases.py): every
expected value is the CPU oracle's (O.transpose on the two parts, O.mm_z, O.lin_z, O.mulV_z, O.axpy_z, O.compress) or
numpy on oracle output, none the library's.  Structure is compared with np.array_equal, values bit for bit.

One comparison is not bit for bit over all rows, and not because of anything the calls above do: mulv / gaxpy on the
5003 x 1201 input's ctrans() run the complex CSR-stream SpMV, which sums a row that fills one of its 256-entry chunks
with a wavefront tree (csrc/spmv_z.hip; include/sparse_linear_hip.h, spl_matrix_set_spmv_order).  That handle has rows
of 300 and 4 200 entries.  Rows of at most 255 entries never fill a chunk and are compared bit for bit; on the longer
ones both orders add the SAME rounded products p (and the same y when accumulating), N <= len + 1 terms, so each part
of the result differs from the oracle's by at most twice the summation error  (N - 1) u sum |terms| / (1 - (N - 1) u),
u = eps / 2,  with  |p| <= (1 + u)^2 |a| |x|  per part:  the test allows  (len + 1) eps (sum |a| |x| + |y|),  whose
one extra eps per row covers the (1 + O(len u)) factors and the rounding of the bound's own sum.  spmv_many_dev, which
keeps the order for rows of any length, is compared bit for bit on every row of the same handle, as are mulv / gaxpy
on the 37 x 129 input's ctrans()."""
import ctypes as C

import numpy as np
import pytest

import complex_handle_cases as K
from complex_handle_cases import same_bits

pytestmark = pytest.mark.gpu

ARG, INVALID = -5, -3  # SPL_ERROR_argument_missing, SPL_ERROR_invalid_handle
EPS = np.finfo(float).eps
STREAM_CHUNK_Z = 256   # entries per chunk of the complex CSR-stream SpMV (csrc/spmv_z.hip)


@pytest.fixture(scope="module")
def L(pkg, gpu):
    return pkg._ffi.lib()


def zhandle(pkg, m):
    """whole complex (or real) handle of an oracle CSC tuple"""
    M = pkg.Matrix(m[1], m[0], m[2], m[3], m[4])
    return pkg.DeviceMatrix.from_csc_complex(M) if np.iscomplexobj(m[4]) else pkg.DeviceMatrix.from_csc(M)


def csr_handle(pkg, t):
    return pkg.DeviceMatrix.from_csr(t.nrows_global, t.ncols, t.rp, t.ci, t.v, row0=t.row0)


def assert_holds(H, t):
    inf = H.info()
    assert (inf["nrows_global"], inf["ncols"], inf["row0"], inf["nrows_local"], inf["nnz"]) == \
        (t.nrows_global, t.ncols, t.row0, len(t.rp) - 1, len(t.ci))
    assert H.is_complex == np.iscomplexobj(t.v)
    rp, ci, v = H.export_csr()
    assert np.array_equal(rp, t.rp) and np.array_equal(ci, t.ci)
    assert v.dtype == t.v.dtype and same_bits(v, t.v)


def same_arrays(H1, H2):
    """the derived Eq on the device's own arrays: dimensions, pointers, indices, values with IEEE =="""
    a, b = H1.info(), H2.info()
    if (a["nrows_global"], a["ncols"]) != (b["nrows_global"], b["ncols"]):
        return False
    return all(np.array_equal(x, y) for x, y in zip(H1.export_csr(), H2.export_csr()))


# ---- transpose / ctrans ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tcase(O):
    inputs = dict(K.small_inputs(O), big=K.transpose_input(O))
    return {name: (m, K.transpose(O, m), K.ctrans(O, m)) for name, m in inputs.items()}


@pytest.mark.parametrize("name", ["big", "37x129", "1x1"])
def test_transpose_and_ctrans_of_a_complex_handle(gpu, pkg, O, tcase, name):
    m, mt, mh = tcase[name]
    H = zhandle(pkg, m)
    assert_holds(H, K.csr_truth(O, m))
    T, CT = H.transpose(), H.ctrans()
    assert_holds(T, K.csr_truth(O, mt))
    assert_holds(CT, K.csr_truth(O, mh))   # np.conj's sign bits, those of zeros included
    # back again: the input's arrays bit for bit
    assert_holds(T.transpose(), K.csr_truth(O, m))
    assert_holds(CT.ctrans(), K.csr_truth(O, m))
    assert_holds(T.ctrans(), K.csr_truth(O, K.ctrans(O, mt)))
    # the input is untouched
    assert_holds(H, K.csr_truth(O, m))


def test_ctrans_of_a_real_handle_is_its_transpose(gpu, pkg, O, tcase):
    m = K.real_part(tcase["big"][0])
    H = zhandle(pkg, m)
    want = K.csr_truth(O, O.transpose(m))
    assert not H.is_complex
    assert_holds(H.transpose(), want)
    assert_holds(H.ctrans(), want)


def spmv_many(torch, H, X, Y0=None):
    """the k columns of X through spmv_many_dev; Y0 given: accumulate"""
    k, nrows = X.shape[1], H.info()["nrows_local"]
    dX = torch.from_numpy(np.ascontiguousarray(X.T)).cuda()
    dY = (torch.from_numpy(np.ascontiguousarray(Y0.T)).cuda() if Y0 is not None
          else torch.full((k, nrows), 12345.0, dtype=torch.complex128, device="cuda"))
    H.spmv_many_dev(dX.data_ptr(), X.shape[0], dY.data_ptr(), nrows, k, accumulate=Y0 is not None,
                    stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return dY.cpu().numpy().T


@pytest.mark.parametrize("name", ["big", "37x129"])
def test_the_ctrans_handle_is_consumed(gpu, pkg, O, tcase, name):
    """mulv, gaxpy and spmv_many_dev (k = 5) on the ctrans() handle against O.mulV_z / O.axpy_z on the expected tuple"""
    m, _, mh = tcase[name]
    CT = zhandle(pkg, m).ctrans()
    nr, nc = mh[0], mh[1]
    rng = np.random.default_rng(11)
    X = rng.standard_normal((nc, 5)) + 1j * rng.standard_normal((nc, 5))
    Y0 = rng.standard_normal((nr, 5)) + 1j * rng.standard_normal((nr, 5))
    want = np.stack([O.mulV_z(mh, np.ascontiguousarray(X[:, j])) for j in range(5)], axis=1)
    want_acc = np.empty_like(want)
    for j in range(5):
        y = np.ascontiguousarray(Y0[:, j])
        O.axpy_z(mh, np.ascontiguousarray(X[:, j]), y)
        want_acc[:, j] = y
    # every row, whatever its length
    assert same_bits(spmv_many(gpu, CT, X), want)
    assert same_bits(spmv_many(gpu, CT, X, Y0), want_acc)
    # the CSR-stream kernel: bit for bit where a row cannot fill a chunk, the summation bound of the docstring beyond
    x = np.ascontiguousarray(X[:, 0])
    got = CT.mulv(x)
    got_acc = CT.gaxpy(x, np.ascontiguousarray(Y0[:, 0]))
    lens = np.diff(K.csr_truth(O, mh).rp)
    short = lens < STREAM_CHUNK_Z
    assert same_bits(got[short], want[short, 0]) and same_bits(got_acc[short], want_acc[short, 0])
    if name == "37x129":
        assert short.all()
    else:
        assert np.count_nonzero(~short) == 2
    absm = mh[:4] + (np.abs(mh[4]) + 0j,)
    sabs = O.mulV_z(absm, np.abs(x) + 0j).real   # sum |a| |x| per row
    for y, w, y0 in ((got, want[:, 0], np.zeros(nr, dtype=complex)), (got_acc, want_acc[:, 0], Y0[:, 0])):
        assert np.all(np.abs(y.real - w.real) <= (lens + 1) * EPS * (sabs + np.abs(y0.real)))
        assert np.all(np.abs(y.imag - w.imag) <= (lens + 1) * EPS * (sabs + np.abs(y0.imag)))


# ---- hermitian ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def hcases(O):
    return K.hermitian_cases(O)


@pytest.mark.parametrize("name", sorted(K.H_EXPECTED))
def test_hermitian_verdicts(gpu, pkg, L, O, hcases, name):
    m = hcases[name]
    want = K.hermitian_by_definition(O, m)
    assert want == K.H_EXPECTED[name]
    H = zhandle(pkg, m)
    r = C.c_int(-7)
    assert L.spl_matrix_hermitian(H.handle, C.byref(r)) == 0 and r.value == int(want)   # SPL_OK also when not square
    assert H.hermitian() is want
    if H.is_complex:
        assert same_arrays(H.ctrans(), H) is want     # the definition, on the device's own arrays
    else:
        assert same_arrays(H.transpose(), H) is want
        Z = H.to_complex()
        assert Z.hermitian() is want and same_arrays(Z.ctrans(), Z) is want
    assert H.hermitian() is want                      # read-only: the same answer again


def test_hermitian_of_a_promoted_real_symmetric_handle(gpu, pkg, hcases):
    """to_complex() gives +0.0 imaginary parts, ctrans() makes them -0.0, and == does not mind"""
    Z = zhandle(pkg, hcases["real_symmetric"]).to_complex()
    assert Z.is_complex and Z.hermitian() is True
    im, im_h = Z.export_csr()[2].imag, Z.ctrans().export_csr()[2].imag
    assert not np.signbit(im).any() and np.signbit(im_h).all()
    assert zhandle(pkg, hcases["real_asymmetric"]).to_complex().hermitian() is False


# ---- spgemm ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gcase(O):
    inp = K.spgemm_inputs(O)
    return inp, K.spgemm_truths(O, inp)


def test_complex_product_of_whole_handles(gpu, pkg, O, gcase):
    inp, t = gcase
    HA, HB = zhandle(pkg, inp["A"]), zhandle(pkg, inp["B"])
    P, products = HA.spgemm(HB)
    assert_holds(P, K.csr_truth(O, t["AB"]))          # b * a in the kernel, a * b in the oracle: the same bits
    # the products counted are those of the two patterns
    assert products == zhandle(pkg, K.real_part(inp["A"])).spgemm(zhandle(pkg, K.real_part(inp["B"])))[1] > 0
    assert_holds(P.ctrans(), K.csr_truth(O, K.ctrans(O, t["AB"])))
    assert_holds(HA, K.csr_truth(O, inp["A"]))        # operands untouched
    assert_holds(HB, K.csr_truth(O, inp["B"]))


def test_complex_product_with_a_row_block_on_the_left(gpu, pkg, O, gcase):
    """the left factor made on the device as R1 + 0.5j R2 from two real row-block handles"""
    inp, t = gcase
    r0, r1 = K.G_BLOCK
    R1, R2 = (csr_handle(pkg, K.rows_of(K.csr_truth(O, inp[n]), r0, r1)) for n in ("R1", "R2"))
    A2 = R1.to_complex().lin(1.0, R2.to_complex(), 0.5j)
    assert_holds(A2, K.rows_of(K.csr_truth(O, t["A2"]), r0, r1))
    P, products = A2.spgemm(zhandle(pkg, inp["B"]))
    assert_holds(P, K.rows_of(K.csr_truth(O, t["A2B"]), r0, r1))
    assert products >= P.info()["nnz"]


def test_lin_of_two_complex_products(gpu, pkg, O, gcase):
    """a second generation: alpha (A B) + beta (A2 B) with complex scalars"""
    inp, t = gcase
    HB = zhandle(pkg, inp["B"])
    P1 = zhandle(pkg, inp["A"]).spgemm(HB)[0]
    P2 = zhandle(pkg, t["A2"]).spgemm(HB)[0]
    assert_holds(P2, K.csr_truth(O, t["A2B"]))
    assert_holds(P1.lin(K.G_ALPHA, P2, K.G_BETA), K.csr_truth(O, t["lin"]))


# ---- refusals and statuses ---------------------------------------------------------------------------------------

def refused(call, status=ARG):
    """call(out) passes `out` as the entry point's output handle: the status, and the handle left NULL"""
    h = C.c_void_p(1)
    return call(C.byref(h)) == status and not h.value


def test_refusals_and_statuses(gpu, pkg, L, O, gcase):
    inp, _ = gcase
    Ar, Br = zhandle(pkg, K.real_part(inp["A"])), zhandle(pkg, K.real_part(inp["B"]))
    Az, Bz = zhandle(pkg, inp["A"]), zhandle(pkg, inp["B"])
    # one real and one complex operand, both ways round
    assert refused(lambda out: L.spl_matrix_spgemm(Ar.handle, Bz.handle, out, None))
    assert refused(lambda out: L.spl_matrix_spgemm(Az.handle, Br.handle, out, None))
    # ctrans / hermitian of a row block, real and complex
    blk = csr_handle(pkg, K.rows_of(K.csr_truth(O, inp["R1"]), *K.G_BLOCK))
    r = C.c_int(-7)
    for H in (blk, blk.to_complex()):
        assert refused(lambda out: L.spl_matrix_ctrans(H.handle, out))
        assert refused(lambda out: L.spl_matrix_transpose(H.handle, out))
        assert L.spl_matrix_hermitian(H.handle, C.byref(r)) == ARG and r.value == -7
    # missing out pointers
    assert L.spl_matrix_hermitian(Az.handle, None) == ARG
    assert L.spl_matrix_transpose(Az.handle, None) == ARG and L.spl_matrix_ctrans(Az.handle, None) == ARG
    # no handle at all
    zeros = (C.c_char * 512)()
    for bad in (None, C.cast(zeros, C.c_void_p)):
        assert L.spl_matrix_hermitian(bad, C.byref(r)) == INVALID and r.value == -7
        h = C.c_void_p(1)
        assert L.spl_matrix_ctrans(bad, C.byref(h)) == INVALID
        assert L.spl_matrix_spgemm(bad, Bz.handle, C.byref(h), None) == INVALID
    # the neighbouring legal calls go through
    assert Az.spgemm(Bz)[0].is_complex and not Ar.spgemm(Br)[0].is_complex
    assert Ar.to_complex().spgemm(Bz)[0].is_complex
    assert Az.ctrans().info()["nrows_global"] == K.G_NK and blk.to_complex().info()["row0"] == K.G_BLOCK[0]
    assert Az.hermitian() is False
