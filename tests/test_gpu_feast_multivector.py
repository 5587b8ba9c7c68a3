"""FEAST's products A Q, B Q, B Y as ONE multi-vector call each (spl_matrix_spmv_many_dev) instead of one
spl_matrix_spmv_dev per subspace vector (SPL_FEAST_MULTIVECTOR=0, the reference's `multiplyWork`, Feast.hs:203-208):
the same bits either way on the short rows FEAST's matrices have, and 3 product calls per iteration instead of 3 m0."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def both_ways(pkg, monkeypatch, solve):
    monkeypatch.delenv("SPL_FEAST_MULTIVECTOR", raising=False)
    lam1, X1 = solve()
    fused = dict(pkg.feast.geigSH_.last_clock)
    monkeypatch.setenv("SPL_FEAST_MULTIVECTOR", "0")
    lam0, X0 = solve()
    loop = dict(pkg.feast.geigSH_.last_clock)
    assert len(lam1) > 0
    assert np.array_equal(lam1, lam0) and np.array_equal(X1, X0)
    assert fused["iterations"] == loop["iterations"]
    return lam1, fused, loop


def test_real_poisson3d_same_bits_and_call_counts(gpu, pkg, monkeypatch):
    """the setting of the resident-factors test: poisson3d m = 12, four contour points, m0 = 12"""
    m, m0 = 12, 12
    H = pkg.DeviceMatrix.synthetic("poisson3d", m)
    rp, ci, v = H.export_csr()
    H.free()
    n = m ** 3
    A = pkg.Matrix(n, n, rp, ci, v)  # symmetric: its CSR arrays are its CSC arrays
    ref = np.linalg.eigvalsh(pkg.pack(A))
    uniq = np.unique(np.round(ref, 9))
    lo, hi = 0.5 * (uniq[0] + uniq[1]), 0.5 * (uniq[2] + uniq[3])
    params = pkg.feast.FeastParams(feastContourPoints=4)
    lam, fused, loop = both_ways(pkg, monkeypatch, lambda: pkg.feast.eigSHParams(params, m0, (lo, hi), A))
    assert len(lam) == 6
    assert fused["iterations"] >= 2
    assert fused["spmv_calls"] == 3 * fused["iterations"]
    assert loop["spmv_calls"] == 3 * m0 * loop["iterations"]


def test_complex_hermitian_same_bits_and_call_counts(gpu, pkg, monkeypatch):
    """the complex Hermitian tridiagonal of tests/test_gpu_feast.py: a complex subspace through the complex kernel"""
    rng = np.random.default_rng(12)
    n, m0 = 50, 8
    tri = [(i, i, float(i + 1)) for i in range(n)]
    for i in range(n - 1):
        z = complex(0.3 * rng.normal(), 0.3 * rng.normal())
        tri += [(i, i + 1, z), (i + 1, i, z.conjugate())]
    A = pkg.fromTriples(n, n, [(r, c, complex(v)) for r, c, v in tri])
    assert A.is_complex
    ref = np.linalg.eigvalsh(pkg.pack(A))
    lo, hi = 0.5 * (ref[11] + ref[12]), 0.5 * (ref[16] + ref[17])
    lam, fused, loop = both_ways(pkg, monkeypatch, lambda: pkg.feast.eigSH(m0, (lo, hi), A))
    assert len(lam) == 5
    assert fused["spmv_calls"] == 3 * fused["iterations"]
    assert loop["spmv_calls"] == 3 * m0 * loop["iterations"]
