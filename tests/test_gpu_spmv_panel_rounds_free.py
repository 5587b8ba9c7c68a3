"""The rounds form of the panel SpMV without the rendezvous between a workgroup's panels (csrc/spmv_panel.hip,
PanelPlan::meet = 0).  The build's one-time timing chooses this on large matrices where it pays; here
SPL_PANEL_RENDEZVOUS=0 asks for it on small ones with many more panels than CUs, so that every workgroup walks several
panels and the workgroups drift apart.  The rendezvous is pacing only: integer-valued data must give the oracle's
bits, random data the order-free contract, for y = A x and y <- A x + y, over launches queued back to back (the last
workgroup to leave still resets the words of the image)."""
import numpy as np
import pytest

from helpers import panel_check as _check, panel_stream as _stream

pytestmark = pytest.mark.gpu


def _build(pkg, monkeypatch, H, P, w, unroll):
    monkeypatch.setenv("SPL_PANEL_RENDEZVOUS", "0")
    H.build_panel(P, w, unroll, pkg.DeviceMatrix.PANEL_FORM_ROUNDS)
    H.set_variant(16)
    assert H.spmv_kernel() == 16


@pytest.mark.parametrize("P,w,unroll", [(64, 12, 3), (100, 9, 4), (64, 4, 6)])
def test_rounds_without_rendezvous_exact_on_integers(gpu, pkg, O, monkeypatch, P, w, unroll):
    """40 000 rows in panels of 64 or 100 rows: 625 or 400 panels, several per workgroup on any device"""
    torch = gpu
    rng = np.random.default_rng(21)
    n, k = 40_000, 700_000
    A = O.compress(n, n, rng.integers(0, n, k), rng.integers(0, n, k), rng.integers(-9, 10, k).astype(float))
    xh = rng.integers(-5, 6, n).astype(float)
    yo = O.mulV(A, xh)
    H = pkg.DeviceMatrix.from_csc(pkg.Matrix(n, n, A[2], A[3], A[4]))
    _build(pkg, monkeypatch, H, P, w, unroll)
    x = torch.from_numpy(xh).cuda()
    y0 = rng.integers(-100, 101, n).astype(float)
    ys = [torch.from_numpy(y0.copy()).cuda() for _ in range(6)]
    for i, y in enumerate(ys):  # no synchronise in between; plain and accumulate mixed
        H.spmv_dev(x.data_ptr(), y.data_ptr(), accumulate=bool(i % 2), stream=_stream(torch))
    torch.cuda.synchronize()
    for i, y in enumerate(ys):
        assert np.array_equal(y.cpu().numpy(), yo + y0 if i % 2 else yo), "launch %d" % i
    assert H.panel_errors() == 0
    H.free()


@pytest.mark.parametrize("n,K,P,w,unroll", [(50_003, 3, 128, 10, 5), (200_000, 20, 700, 14, 4)])
def test_rounds_without_rendezvous_contract(gpu, pkg, O, monkeypatch, n, K, P, w, unroll):
    """the three-part contract of tests/test_gpu_spmv_panel.py on random doubles, ragged last panel"""
    H = pkg.DeviceMatrix.synthetic("random", n, K)
    _build(pkg, monkeypatch, H, P, w, unroll)
    _check(gpu, O, H, n)
    H.free()
