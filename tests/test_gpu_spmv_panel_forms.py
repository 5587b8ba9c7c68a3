"""Every form of the order-free panel SpMV (csrc/spmv_panel.hip) through the public API only: each kernel the
dispatch table holds runs once on a matrix whose panels are shorter than one phase or round and once on one whose
phases outgrow the register pipeline; requests between the instantiated register counts are served by the nearest
one, not refused; every form family crosses the rendezvous between generations, also in launches queued back to
back; and what is refused is refused where it always was (shape and form at build, an unknown ring shape at the
first launch).  The contract is helpers.panel_check: 1e-10 against the oracle with the reference's closeness
predicate, the rounding bound 2 len eps sum |a x| per row, the accumulate form, panel_errors() == 0."""
import numpy as np
import pytest

from helpers import panel_check, panel_stream

pytestmark = pytest.mark.gpu

ARGUMENT_MISSING = -5

# (form family, index blocks per phase, register sets): what the dispatch instantiates
CHUNK = [("chunk", K, U) for K in (1, 2) for U in (4, 6, 8, 10, 12)]
PAIRED = [("paired", 1, U) for U in (2, 3, 4)] + [("paired", 2, U) for U in (3, 4, 5, 6)]
ROUNDS = [("rounds", 0, U) for U in (3, 4, 5, 6)]
# ring shapes (loaders, loader depth, gatherer depth, index blocks per phase, slots per loader)
RING = [(4, 4, 4, 2, 1), (4, 6, 4, 2, 1), (4, 8, 4, 2, 1), (4, 6, 3, 2, 1), (4, 6, 4, 1, 1), (4, 6, 4, 2, 3),
        (4, 4, 3, 2, 1), (4, 5, 4, 2, 1), (2, 8, 2, 2, 1), (8, 3, 4, 2, 1), (8, 4, 4, 2, 1), (4, 6, 4, 3, 1),
        (4, 6, 4, 4, 1), (4, 6, 4, 3, 3), (4, 6, 4, 4, 3), (4, 4, 4, 2, 3), (4, 6, 3, 2, 3), (4, 6, 4, 1, 3),
        (4, 4, 4, 4, 1), (4, 4, 4, 3, 1), (8, 4, 4, 4, 1), (8, 4, 4, 2, 2), (4, 4, 4, 8, 1), (4, 6, 4, 8, 1)]

# panels shorter than one phase or round, 63 index blocks, dummy units in every register set / phases longer than
# the pipeline, the tail loop, a ragged last panel
MATRICES = {"short": (1000, 3, 64, 4), "long": (50_003, 20, 3000, 12)}

_handles = {}


def _matrix(pkg, name):
    """one handle per matrix for the whole module: build_panel replaces the image, the CSR arrays stay"""
    if name not in _handles:
        n, K, _, _ = MATRICES[name]
        _handles[name] = pkg.DeviceMatrix.synthetic("random", n, K)
    return _handles[name]


def _form_code(D, family, K):
    if family == "chunk":
        return {1: D.PANEL_FORM_CHUNK_K1, 2: D.PANEL_FORM_CHUNK_K2}[K]
    if family == "paired":
        return {1: D.PANEL_FORM_PAIRED_K1, 2: D.PANEL_FORM_PAIRED_K2}[K]
    if family == "ring":
        return {1: D.PANEL_FORM_RING_K1, 2: D.PANEL_FORM_RING_K2, 3: D.PANEL_FORM_RING_K3, 4: D.PANEL_FORM_RING_K4,
                8: D.PANEL_FORM_RING_K8}[K]
    return D.PANEL_FORM_ROUNDS


def _ring_env(monkeypatch, nl, gd, slots):
    monkeypatch.setenv("SPL_PANEL_RING_NL", str(nl))
    monkeypatch.setenv("SPL_PANEL_RING_GD", str(gd))
    monkeypatch.setenv("SPL_PANEL_RING_SLOTS", str(slots))


@pytest.mark.parametrize("matrix", sorted(MATRICES))
@pytest.mark.parametrize("family,K,U", CHUNK + PAIRED + ROUNDS)
def test_every_instantiation(gpu, pkg, O, matrix, family, K, U):
    n, _, P, w = MATRICES[matrix]
    H = _matrix(pkg, matrix)
    H.build_panel(P, w, U, _form_code(pkg.DeviceMatrix, family, K))
    H.set_variant(16)
    assert H.spmv_kernel() == 16 and H.info()["blocked_rows"] == P
    panel_check(gpu, O, H, n)


@pytest.mark.parametrize("matrix", sorted(MATRICES))
@pytest.mark.parametrize("nl,D,GD,K,S", RING)
def test_every_ring_shape(gpu, pkg, O, monkeypatch, matrix, nl, D, GD, K, S):
    _ring_env(monkeypatch, nl, GD, S)
    n, _, P, w = MATRICES[matrix]
    H = _matrix(pkg, matrix)
    H.build_panel(P, w, D, _form_code(pkg.DeviceMatrix, "ring", K))
    H.set_variant(16)
    assert H.spmv_kernel() == 16 and H.info()["blocked_rows"] == P
    panel_check(gpu, O, H, n)


@pytest.mark.parametrize("family,K", [("chunk", 1), ("chunk", 2), ("paired", 1)])
def test_request_between_instantiations_is_served(gpu, pkg, O, family, K):
    """5 register sets are instantiated for neither: the launch takes the nearest kernel that is"""
    n, _, P, w = MATRICES["short"]
    H = _matrix(pkg, "short")
    H.build_panel(P, w, 5, _form_code(pkg.DeviceMatrix, family, K))
    H.set_variant(16)
    panel_check(gpu, O, H, n)


@pytest.mark.parametrize("family,K,slices", [("chunk", 2, 0), ("paired", 2, 0), ("paired", 2, 4), ("ring", 2, 0)])
def test_generations_and_rendezvous(gpu, pkg, O, monkeypatch, family, K, slices):
    """40 000 rows in panels of 64 are 625 panels — at least two generations on any device, ten 2-chunk segments per
    panel: the workgroups meet at the rendezvous word between generations, which the launcher clears in front of
    every launch.  Then four launches queued back to back on one stream, plain and accumulate alternating, against
    the oracle applied the same four times."""
    torch = gpu
    if slices:
        monkeypatch.setenv("SPL_PANEL_SLICES", str(slices))
    n = 40_000
    H = pkg.DeviceMatrix.synthetic("random", n, 20)
    H.build_panel(64, 12, 0, _form_code(pkg.DeviceMatrix, family, K))
    H.set_variant(16)
    panel_check(torch, O, H, n)
    rp, ci, v = H.export_csr()
    rp32 = rp.astype(np.int32)
    xh = O.gen_vector(n)
    x = torch.from_numpy(xh).cuda()
    y0 = O.gen_vector(n, seed=9)
    y = torch.from_numpy(y0.copy()).cuda()
    s = panel_stream(torch)
    for i in range(4):  # no synchronise in between
        H.spmv_dev(x.data_ptr(), y.data_ptr(), accumulate=bool(i % 2), stream=s)
    torch.cuda.synchronize()
    yo = y0.copy()
    for i in range(4):
        if not i % 2:
            yo[:] = 0.0
        O.csr_gaxpy32(rp32, ci, v, xh, yo)
    assert O.count_not_close(y.cpu().numpy(), yo, 1e-10) == 0
    assert H.panel_errors() == 0
    H.free()


def test_refusals_keep_their_place(gpu, pkg, monkeypatch):
    torch = gpu
    D = pkg.DeviceMatrix
    n, _, P, w = MATRICES["short"]
    H = _matrix(pkg, "short")
    with pytest.raises(pkg.SparseLinearError) as e:  # rounds of 7 register sets: at build
        H.build_panel(512, 10, 7, D.PANEL_FORM_ROUNDS)
    assert e.value.status == ARGUMENT_MISSING
    with pytest.raises(pkg.SparseLinearError) as e:  # no form 3
        H.build_panel(P, w, 0, 3)
    assert e.value.status == ARGUMENT_MISSING
    _ring_env(monkeypatch, 4, 7, 1)  # a ring shape that is not instantiated: builds, the launch refuses
    H.build_panel(P, w, 6, D.PANEL_FORM_RING_K2)
    H.set_variant(16)
    x = torch.ones(n, dtype=torch.float64, device="cuda")
    y = torch.zeros(n, dtype=torch.float64, device="cuda")
    with pytest.raises(pkg.SparseLinearError) as e:
        H.spmv_dev(x.data_ptr(), y.data_ptr(), stream=panel_stream(torch))
    assert e.value.status == ARGUMENT_MISSING
    torch.cuda.synchronize()
