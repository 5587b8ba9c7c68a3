"""The N > 1 flow of bench.py (the driver's multi-GPU scaling run) rehearsed on ONE GPU: two ranks
share cuda:0 and exchange y over gloo (SPL_BENCH_REHEARSAL=1).  Checks that the launch contract
holds end to end — row blocks, all-gather, max over ranks, one JSON line from rank 0 — and that the
gathered y equals the single-rank y."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(nproc, extra, chunks=None, exchange=None, plain=False, env_extra=None, want_stderr=False, drop_env=(), full=True):
    env = dict(os.environ, SPL_BENCH_REHEARSAL="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.update(env_extra or {})
    for k in drop_env:
        env.pop(k, None)
    if chunks is not None:
        env["SPL_BENCH_CHUNKS"] = str(chunks)
    if exchange is not None:
        env["SPL_BENCH_EXCHANGE"] = exchange
    if nproc == 1 or plain:  # plain: bench.py starts the launcher itself (no WORLD_SIZE in the environment)
        for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
            env.pop(k, None)
        cmd = [sys.executable, os.path.join(ROOT, "bench.py")]
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc),
               "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py")]
    cmd += ["--gpus", str(nproc), "--steps", "3", "--warmup", "1"]
    if full:  # roofline and the fingerprint of y; the CPU baseline and the secondary block are not wanted here
        cmd += ["--full", "--no-cpu-baseline", "--no-secondary"]
    if "--order" not in extra:
        cmd += ["--order", "reference"]  # bit-identical sums: the SHA-1 of y must not depend on the rank count
    cmd += extra
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout  # exactly one JSON line, from rank 0
    if want_stderr:
        return json.loads(lines[0]), r.stderr
    return json.loads(lines[0])


@pytest.mark.parametrize("matrix", ["random", "banded"])
def test_two_ranks_on_one_gpu(gpu, matrix):
    args = ["--rows", "400000", "--matrix", matrix]
    one = _run(1, args)
    two = _run(2, args)
    for out, n in ((one, 1), (two, 2)):
        assert out["n_gpus"] == n and out["steps"] == 3 and out["warmup"] == 1
        assert out["metric"] == "fp64 CSR SpMV effective GB/s" and out["unit"] == "GB/s"
        assert out["scaling"] == "strong" and out["dtype"] == "f64" and out["vs_baseline"] is None
        assert out["value"] > 0 and out["roofline"]["frac"] > 0
    # the same matrix: identical nnz, hence identical algorithmic bytes, whatever the rank count
    assert one["config"]["algorithmic_bytes"] == two["config"]["algorithmic_bytes"]
    assert one["y_sha1"] == two["y_sha1"]  # the gathered y is the single-rank y, bit for bit
    assert set(two["config"]["exchange_ms_per_step_by_chunks"]) == {"rccl1", "rccl2", "rccl4", "peer1", "peer2", "peer4"}  # all candidates were measured


def test_pipelined_exchange_forced(gpu):
    """the chunked, overlapped exchange (one asynchronous all-gather per chunk) forced on: 2 ranks x 4
    chunks and 3 ranks x 2 chunks give the y of one rank"""
    args = ["--rows", "480000"]
    one = _run(1, args)
    for nproc, chunks in ((2, 4), (3, 2), (2, 1)):
        out = _run(nproc, args, chunks=chunks, exchange="rccl")
        assert out["y_sha1"] == one["y_sha1"], (nproc, chunks)
        assert out["config"]["algorithmic_bytes"] == one["config"]["algorithmic_bytes"]
        if chunks > 1:
            assert "%d chunks per rank" % chunks in out["config"]["workload"]
            assert out["roofline"]["launches_per_step"] == chunks
        else:
            assert "one RCCL all-gather of y after the kernel" in out["config"]["workload"]


def test_two_ranks_order_free(gpu):
    """--order free (the default of bench.py): sums may differ at rounding level between launches, so y is
    compared through its sum and 2-norm instead of its SHA-1"""
    args = ["--rows", "400000", "--order", "free"]
    one, two = _run(1, args), _run(2, args)
    assert one["config"]["sum_order"] == two["config"]["sum_order"] == "free"
    for k in ("y_sum", "y_norm2"):
        assert abs(one[k] - two[k]) <= 1e-12 * abs(one[k])


@pytest.mark.parametrize("nproc,chunks", [(2, 1), (3, 1), (2, 4), (3, 2)])
def test_peer_store_exchange_forced(gpu, nproc, chunks):
    """the one-sided exchange (csrc/peer.hip: device-to-device copies into the peers' buffers through IPC
    handles, step flags, a wait kernel) forced on, in one piece and pipelined over chunks: N = 2 and 3 give
    the y of one rank, bit for bit"""
    args = ["--rows", "480000"]
    one = _run(1, args)
    out = _run(nproc, args, chunks=chunks, exchange="peer")
    assert "one-sided peer stores" in out["config"]["workload"]
    if chunks > 1:
        assert "%d chunks per rank" % chunks in out["config"]["workload"]
        assert out["roofline"]["launches_per_step"] == chunks
    assert out["y_sha1"] == one["y_sha1"]
    assert out["config"]["algorithmic_bytes"] == one["config"]["algorithmic_bytes"]


def test_plain_launch_starts_its_own_ranks(gpu):
    """`python bench.py --gpus 2` without torchrun (the shape of the driver's 1-GPU command): the script starts
    the launcher as a child before touching a GPU and hands its status on; same y as one rank"""
    args = ["--rows", "400000"]
    one = _run(1, args)
    two = _run(2, args, plain=True)
    assert two["n_gpus"] == 2 and two["y_sha1"] == one["y_sha1"]


def test_four_ranks_all_schedules(gpu):
    """the widest rehearsal a one-GPU box admits (its process guard allows 6 processes on the card: this test
    runner and 4 ranks use it, the launcher's agent does not initialise it): 3 IPC peers and 3 copy streams per rank,
    4-way all-gather, all six schedules measured and each equal to the single-rank y.  Unattended since round 5
    (rounds 3 - 4: opt-in).  The 8-rank shape of config C3 is rehearsed on CPU ranks (tests/test_dist_gloo.py)."""
    args = ["--rows", "240000"]
    one = _run(1, args)
    four, err = _run(4, args, want_stderr=True)
    assert four["n_gpus"] == 4 and four["y_sha1"] == one["y_sha1"]
    assert set(four["config"]["exchange_ms_per_step_by_chunks"]) == {"rccl1", "rccl2", "rccl4", "peer1", "peer2", "peer4"}
    # rank 0's last stderr line: a <= 500-byte summary a failed scaling run can be diagnosed from
    last = [l for l in err.strip().splitlines() if l.startswith("{")][-1]
    brief = json.loads(last)
    assert len(last) <= 500 and brief["n_gpus"] == 4 and brief["value"] == four["value"] and set(brief["tournament"]) == set(four["config"]["exchange_ms_per_step_by_chunks"])


@pytest.mark.parametrize("exchange", ["peer", "rccl"])
def test_bench_sets_the_ipc_mode_itself(gpu, exchange):
    """bench.py:88 `os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")`: this platform's host driver supports dmabuf
    IPC only, and without the variable hipIpcGetMemHandle fails.  The pool's boxes export it; here it is REMOVED from the
    ranks' environment, so the one-sided exchange (IPC handles of the peers' buffers) only works if bench.py put it back
    before HIP initialised — what a bare 8-GPU box gets."""
    args = ["--rows", "240000"]
    one = _run(1, args)
    two = _run(2, args, chunks=1, exchange=exchange, drop_env=("HSA_ENABLE_IPC_MODE_LEGACY",))
    assert two["n_gpus"] == 2 and two["y_sha1"] == one["y_sha1"]
    if exchange == "peer":
        assert "one-sided peer stores" in two["config"]["workload"]


def test_secondary_block_rides_on_the_headline_line(gpu):
    """the C5 / banded / C4 / SpMV block bench.py appends at N = 1 (tools/bench_secondary.py, one child process per
    item), on small instances of the same code: every entry carries value, unit, roofline and parity — the LU entries
    the roofline of their triangular solves too —, an item that fails costs only itself, the headline fields are untouched"""
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--rows", "400000", "--steps", "3", "--warmup", "1",
           "--cpu-reps", "1", "--secondary", "c5:16:cpu8,banded,no-such-item,c4:12,zi:14,spmv:poisson3d:16,spmv:rmat:12,feast:10"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][0]
    # the driver keeps 8 KB of stdout (round 4's 13.9 KB line lost three secondary entries): same number of items as the
    # default list, every key present, and the whole stdout — not only the line — under 7 500 bytes
    assert len(line) <= 7500 and r.stdout.rstrip().endswith(line), (len(line), len(r.stdout))
    out = json.loads(line)
    assert out["metric"] == "fp64 CSR SpMV effective GB/s" and out["n_gpus"] == 1 and out["parity"]["not_close_1e-10"] == 0
    assert out["cpu_baseline"]["cores"] == 1 and out["cpu_baseline"]["kind"] == "port"
    sec = out["secondary"]
    assert set(sec) == {"c2_banded_spmv", "c5_lu_poisson3d_16", "c4_spgemm_rmat12", "f3_zi_lu_shifted_poisson3d_14",
                        "spmv_poisson3d_16", "spmv_rmat_12", "no-such-item", "f4_feast_laplacian3d_10"}
    assert "error" in sec["no-such-item"]
    assert sec["f3_zi_lu_shifted_poisson3d_14"]["parity"]["within_1e-10"] and sec["f3_zi_lu_shifted_poisson3d_14"]["unit"] == "s"
    assert sec["c2_banded_spmv"]["parity"]["bit_identical"] and sec["c2_banded_spmv"]["roofline"]["bound"] == "hbm"
    lu = sec["c5_lu_poisson3d_16"]
    assert lu["parity"]["within_1e-10"] and lu["unit"] == "s" and lu["parity"]["second_solve_bit_identical"]
    assert lu["value"] >= lu["analyze_s"] + lu["first_factor_s"]  # the one-shot figure: analysis + FIRST factorisation + first solve
    sr = lu["solve_roofline"]
    assert sr["bound"] == "hbm" and sr["walks"] >= 1 and sr["bytes_per_walk"] > 16 * 4096 and 0 < sr["frac"] < 1
    assert sr["backward_error"] < 2.3e-16 and 0 < sr["host_buffers"]["frac"] < 1 and sr["host_buffers"]["s"] > 0
    assert lu["cpu_baseline"]["same_workload"] is False and isinstance(lu["memory_was_clean"], bool)
    assert "traffic" in sr and "traffic" in lu["roofline"]
    assert sec["f3_zi_lu_shifted_poisson3d_14"]["solve_roofline"]["walks"] >= 1
    for k in ("spmv_poisson3d_16", "spmv_rmat_12"):
        assert sec[k]["parity"]["bit_identical"] and sec[k]["roofline"]["bound"] == "hbm" and sec[k]["unit"] == "GB/s"
    assert sec["c4_spgemm_rmat12"]["parity"]["structure_and_values_bit_identical"]
    assert sec["c4_spgemm_rmat12"]["cpu_baseline"]["kind"] == "port" and sec["c4_spgemm_rmat12"]["unit"] == "Gproducts/s"
    fe = sec["f4_feast_laplacian3d_10"]
    assert fe["within_1e-10"] and fe["found"] == fe["eigenvalues_exact_in_window"] > 0 and fe["unit"] == "s"
    assert fe["stage_seconds"]["factorisations"] == 8 and fe["stage_seconds"]["iterations"] >= 1


@pytest.mark.parametrize("nproc,chunks", [(2, 1), (3, 2)])
def test_one_sided_exchange_that_gives_up_in_the_timed_region_falls_back_to_the_collective(gpu, nproc, chunks):
    """the fallback of bench.py after a one-sided exchange that timed out DURING the timed region had never
    run.  SPL_PEER_TEST_FAIL_AT_STEP makes the wait kernel of csrc/peer.hip give up at a chosen step (here: inside the
    timed steps, after the 14 steps the start-up tournament spends on the candidate and the warm-up step): every rank
    must agree on the failure, release the exchange (IPC mappings, copy streams, the pieces' matrices), rebuild the
    plain row-block step, time the region again and deliver the y of a single rank — exit status 0, and the line says
    what happened.  Twice in a row from this process: nothing is left behind that the second run would trip over."""
    args = ["--rows", "480000"]
    one = _run(1, args)
    for attempt in range(2):
        out, err = _run(nproc, args, chunks=chunks, exchange="peer", env_extra={"SPL_PEER_TEST_FAIL_AT_STEP": "16"},
                        want_stderr=True)
        assert out["n_gpus"] == nproc and out["y_sha1"] == one["y_sha1"]
        assert "fallback" in out["config"]["workload"] and "exchange_fallback" in out["config"]
        assert "invalid" not in out
        assert "falling back to the RCCL all-gather" in err and "exchange of y, ms per step before the timed region" in err
    # only ONE rank's wait gives up (a single late link): the others must follow it into the fallback all the same
    out = _run(nproc, args, chunks=chunks, exchange="peer", env_extra={"SPL_PEER_TEST_FAIL_AT_STEP": "17:%d" % (nproc - 1)})
    assert out["y_sha1"] == one["y_sha1"] and "exchange_fallback" in out["config"]
    # the switch off: the forced one-sided exchange is what the line reports, no fallback
    out = _run(nproc, args, chunks=chunks, exchange="peer")
    assert out["y_sha1"] == one["y_sha1"] and "exchange_fallback" not in out["config"] and "one-sided" in out["config"]["workload"]


def test_three_ranks_all_schedules(gpu):
    """3 ranks on one GPU, nothing forced: the start-up tournament measures all six schedules (2 IPC peers and copy
    streams per rank, 3-way all-gather, 1 / 2 / 4 chunks) and whichever wins reproduces the single-rank y"""
    args = ["--rows", "480000"]
    one = _run(1, args)
    three = _run(3, args)
    assert three["n_gpus"] == 3 and three["y_sha1"] == one["y_sha1"]
    assert set(three["config"]["exchange_ms_per_step_by_chunks"]) == {"rccl1", "rccl2", "rccl4", "peer1", "peer2", "peer4"}


def test_plain_run_prints_the_headline_only(gpu, tmp_path):
    """without --full a run sets up, warms up, times its steps, dumps y and prints the line: the headline and its
    configuration, no roofline, fingerprint, CPU baseline, parity or secondary block (none of them is run).  The dumped
    y is the y a --full run fingerprints, for one rank and for two"""
    import hashlib

    import numpy as np
    args = ["--rows", "400000"]
    full = _run(1, args)
    for nproc in (1, 2):
        d = tmp_path / ("plain%d" % nproc)
        out, err = _run(nproc, args + ["--dump-outputs", str(d)], full=False, want_stderr=True)
        assert out["metric"] == "fp64 CSR SpMV effective GB/s" and out["unit"] == "GB/s" and out["dtype"] == "f64"
        assert out["higher_is_better"] is True and out["value"] > 0 and out["ms_per_step"] > 0
        assert out["n_gpus"] == nproc and out["steps"] == 3 and out["warmup"] == 1
        assert out["config"]["algorithmic_bytes"] == full["config"]["algorithmic_bytes"]
        for k in ("roofline", "y_sha1", "y_sum", "y_norm2", "cpu_baseline", "cpu_fair_openmp", "parity", "secondary"):
            assert k not in out, k
        assert hashlib.sha1(np.load(d / "y.npy").tobytes()).hexdigest() == full["y_sha1"]
        if nproc > 1:
            brief = json.loads([l for l in err.strip().splitlines() if l.startswith("{")][-1])
            assert brief["value"] == out["value"] and brief["kernel_ms"] is None


def test_dump_outputs(gpu, tmp_path):
    """--dump-outputs DIR: the y of the last timed step as DIR/y.npy (float64), from rank 0.  Under the reference
    order it is the y the line fingerprints, the same for one rank and for two (over either exchange), and the same
    from run to run; past 2^21 rows a fixed, seeded sample of it, with its row numbers in DIR/y_rows.npy"""
    import hashlib

    import numpy as np
    args = ["--rows", "400000"]
    one = _run(1, args + ["--dump-outputs", str(tmp_path / "one")])
    y = np.load(tmp_path / "one" / "y.npy")
    assert y.dtype == np.float64 and y.shape == (400000,) and not (tmp_path / "one" / "y_rows.npy").exists()
    assert hashlib.sha1(y.tobytes()).hexdigest() == one["y_sha1"]
    for exchange in ("rccl", "peer"):
        d = tmp_path / ("two_" + exchange)
        _run(2, args + ["--dump-outputs", str(d)], chunks=1, exchange=exchange)
        assert np.array_equal(np.load(d / "y.npy"), y), exchange
    # a larger y: a sample of 2^21 rows, drawn the same way every run
    args = ["--rows", "2400000"]
    runs = []
    for name in ("a", "b"):
        _run(1, args + ["--dump-outputs", str(tmp_path / name)])
        runs.append((np.load(tmp_path / name / "y.npy"), np.load(tmp_path / name / "y_rows.npy")))
    (ya, ra), (yb, rb) = runs
    assert ya.dtype == ra.dtype == np.float64 and ya.shape == ra.shape == (1 << 21,)
    assert ra[0] >= 0 and ra[-1] < 2400000 and np.all(np.diff(ra) > 0) and np.all(ra == np.floor(ra))
    assert np.array_equal(ra, rb) and np.array_equal(ya, yb)
