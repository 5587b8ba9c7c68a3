"""The rounds form of the order-free panel SpMV (csrc/spmv_panel.hip, form 11): a panel's paired stream is cut
into rounds of exactly 16 * unroll units (pairs of 64-entry chunks) whatever the index blocks are, and the block
of a unit comes from a per-unit table.  Same contract and the same three checks as tests/test_gpu_spmv_panel.py
— 1e-10 relative against the oracle's CSR product with the reference's closeness predicate, the rounding bound
2 * len(row) * eps * sum |a x| per row, bit equality on integer data — for y = A x and y <- A x + y, on shapes
that exercise what is new: panels shorter than a round, streams that are an exact multiple of a round, segments
far shorter and far longer than a round, empty segments, one index block, ragged edges, 3 to 6 register sets;
and repeated launches on one handle without a synchronise in between (the kernel itself puts the rendezvous
word between generations back to zero: there is no memset in front of a launch)."""
import numpy as np
import pytest

from helpers import panel_check as _check, panel_run as _run, panel_stream as _stream

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n,K,P,w,unroll", [
    # panels with fewer units than one round (at most 63 one-pair segments against 80), many blocks per round
    (1000, 3, 64, 4, 5), (1000, 3, 64, 4, 3),
    # segments far shorter than a round: 49 blocks of about two units each, ragged last panel
    (50_003, 3, 3000, 10, 5), (50_003, 3, 3000, 10, 6),
    # segments far longer than a round: about 170 units against rounds of 48 and 64
    (70_001, 40, 5000, 13, 3), (70_001, 40, 5000, 13, 4),
    # one index block
    (4096, 7, 512, 12, 4), (100_000, 20, 20479, 17, 5),
    # the flagship's shape in small: full-height panels, w = 17 and 14, every unroll, the default unroll (0)
    (131_072, 7, 8192, 17, 3), (200_000, 20, 20479, 14, 6), (300_000, 20, 19000, 13, 4), (200_000, 20, 19700, 14, 0),
    # one row, one entry
    (64, 1, 64, 4, 5)])
def test_rounds_match_oracle(gpu, pkg, O, n, K, P, w, unroll):
    torch = gpu
    H = pkg.DeviceMatrix.synthetic("random", n, K)
    H.build_panel(P, w, unroll, pkg.DeviceMatrix.PANEL_FORM_ROUNDS)
    H.set_variant(16)
    assert H.spmv_kernel() == 16 and H.info()["blocked_rows"] == P
    _check(torch, O, H, n)


@pytest.mark.parametrize("unroll", [3, 4, 5, 6])
@pytest.mark.parametrize("nib", [1, 4])
def test_rounds_exact_multiple_of_a_round(gpu, pkg, O, unroll, nib):
    """every full panel holds exactly 96 units — 1024 rows with 12 entries, each (panel, block) segment whole pairs —
    which is two rounds for 3 register sets and one for 6 (1.5 and 1.2 for 4 and 5); the last panel is ragged"""
    torch = gpu
    P, nc = 1024, 1024
    nr = 2 * P + 100
    wb = nc // nib                    # columns per index block
    r = np.repeat(np.arange(nr), 12)
    j = np.tile(np.arange(12), nr)
    per = 12 // nib                   # entries of a row in one block: distinct columns
    c = (j // per) * wb + (r * 7 + (j % per) * 13) % wb
    rng = np.random.default_rng(11)
    A = O.compress(nr, nc, r, c, rng.uniform(0.5, 1.5, len(r)))
    H = pkg.DeviceMatrix.from_csc(pkg.Matrix(nc, nr, A[2], A[3], A[4]))
    assert H.info()["nnz"] == 12 * nr
    H.build_panel(P, int(np.log2(wb)), unroll, pkg.DeviceMatrix.PANEL_FORM_ROUNDS)
    H.set_variant(16)
    _check(torch, O, H, nc)


def test_rounds_exact_on_integers(gpu, pkg, O):
    """integer-valued entries and vector: every partial sum is exact, so any order gives the same bits"""
    torch = gpu
    rng = np.random.default_rng(5)
    n, k = 40_000, 700_000
    A = O.compress(n, n, rng.integers(0, n, k), rng.integers(0, n, k), rng.integers(-9, 10, k).astype(float))
    xh = rng.integers(-5, 6, n).astype(float)
    yo = O.mulV(A, xh)
    for P, w, unroll in [(2500, 11, 5), (2500, 8, 3), (20479, 16, 6), (700, 13, 4)]:
        H = pkg.DeviceMatrix.from_csc(pkg.Matrix(n, n, A[2], A[3], A[4]))
        H.build_panel(P, w, unroll, pkg.DeviceMatrix.PANEL_FORM_ROUNDS)
        H.set_variant(16)
        assert np.array_equal(_run(torch, H, torch.from_numpy(xh).cuda()), yo)
        H.free()


@pytest.mark.parametrize("unroll", [3, 5])
def test_rounds_empty_rows_segments_and_ragged_edges(gpu, pkg, O, unroll):
    """rows without entries, index blocks without entries (empty segments in the middle of a panel's stream),
    a last panel with a few rows, a last index block with a few columns, an all-empty matrix"""
    torch = gpu
    rng = np.random.default_rng(3)
    nr, nc = 10_007, 4_099
    rows = rng.integers(0, nr, 30_000)
    rows = rows[(rows % 7 != 0) & (rows < nr - 5)]  # every 7th row and the last rows stay empty
    cols = rng.integers(0, nc, len(rows))
    keep = (cols >> 10) != 2                         # nobody has an entry in index block 2 of 5 (w = 10)
    rows, cols = rows[keep], cols[keep]
    A = O.compress(nr, nc, rows, cols, rng.uniform(0.5, 1.5, len(rows)))
    H = pkg.DeviceMatrix.from_csc(pkg.Matrix(nc, nr, A[2], A[3], A[4]))
    H.build_panel(1000, 10, unroll, pkg.DeviceMatrix.PANEL_FORM_ROUNDS)
    H.set_variant(16)
    xh = rng.uniform(0.5, 1.5, nc)
    y = _run(torch, H, torch.from_numpy(xh).cuda())
    yo = O.mulV(A, xh)
    assert O.count_not_close(y, yo, 1e-10) == 0 and np.all(y[::7] == 0.0)
    _check(torch, O, H, nc)
    # w = 4: 257 index blocks, most of them empty in any one panel of 64 rows
    H.build_panel(64, 4, unroll, pkg.DeviceMatrix.PANEL_FORM_ROUNDS)
    _check(torch, O, H, nc)
    Z = pkg.DeviceMatrix.from_csc(pkg.zeros(300, 200))
    Z.build_panel(64, 4, unroll, pkg.DeviceMatrix.PANEL_FORM_ROUNDS)
    Z.set_variant(16)
    assert np.array_equal(_run(torch, Z, torch.ones(200, dtype=torch.float64, device="cuda")), np.zeros(300))


@pytest.mark.parametrize("P,w,unroll", [(8192, 12, 5), (20479, 17, 4), (1024, 9, 3)])
def test_rounds_rmat(gpu, pkg, O, P, w, unroll):
    """the skewed matrix of the existing synthetic generator: segment sizes from empty to many rounds"""
    torch = gpu
    H = pkg.DeviceMatrix.rmat(17, 16, (0.57, 0.19, 0.19))
    H.build_panel(P, w, unroll, pkg.DeviceMatrix.PANEL_FORM_ROUNDS)
    H.set_variant(16)
    _check(torch, O, H, 1 << 17)


@pytest.mark.parametrize("unroll", [3, 6])
def test_rounds_repeated_launches_without_synchronise(gpu, pkg, O, unroll):
    """40 000 rows in panels of 64 are 625 panels, at least two generations on any device: the workgroups meet at
    the rendezvous word between generations, and the last one to leave the kernel resets it.  Launches queued back to
    back on one handle (plain and accumulate mixed) must each meet the contract."""
    torch = gpu
    n = 40_000
    H = pkg.DeviceMatrix.synthetic("random", n, 20)
    H.build_panel(64, 12, unroll, pkg.DeviceMatrix.PANEL_FORM_ROUNDS)
    H.set_variant(16)
    rp, ci, v = H.export_csr()
    xh = O.gen_vector(n)
    x = torch.from_numpy(xh).cuda()
    yo = np.zeros(n)
    O.csr_gaxpy32(rp.astype(np.int32), ci, v, xh, yo)
    reps = 12
    ys = [torch.full((n,), float(i), dtype=torch.float64, device="cuda") for i in range(reps)]
    s = _stream(torch)
    for i in range(reps):  # no synchronise in between
        H.spmv_dev(x.data_ptr(), ys[i].data_ptr(), accumulate=bool(i % 2), stream=s)
    torch.cuda.synchronize()
    for i in range(reps):
        want = yo + float(i) if i % 2 else yo
        assert O.count_not_close(ys[i].cpu().numpy(), want, 1e-10) == 0, "launch %d" % i
    assert H.panel_errors() == 0


def test_rounds_arguments(gpu, pkg):
    """unroll outside 3 ... 6 is refused for this form; the default (0) is accepted"""
    H = pkg.DeviceMatrix.synthetic("random", 5000, 5)
    for bad in (1, 2, 7, 12):
        with pytest.raises(Exception):
            H.build_panel(512, 10, bad, pkg.DeviceMatrix.PANEL_FORM_ROUNDS)
    H.build_panel(512, 10, 0, pkg.DeviceMatrix.PANEL_FORM_ROUNDS)
    H.set_variant(16)
    assert H.spmv_kernel() == 16
