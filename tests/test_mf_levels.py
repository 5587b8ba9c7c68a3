"""Host tables of the multifrontal LU (csrc/mf_levels.hpp): which fronts of a tree level go to which kernel, the
prefix sums that turn a level into flat grids (factorisation and solves), the scratch of the chunked products and the
transient memory plan are plain C++, so they are checked on the CPU with a small native driver
(tests/native/levels_check.cpp) that restates every table from the tree alone.  Grids: Poisson 2-D m = 60 and 3-D m = 24;
at m = 24 and the shrunken limits one level holds all three classes and the top levels have fronts above 256 rows.  No
grid of this size has a level of 4096 row blocks, where a solve workgroup takes four: the driver checks that case on a
level written down by hand, in every run."""
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# limits small enough that the grids used here hold fronts of all three factor classes, levels of more than one
# super-block step in the solves and fronts solved by many workgroups from 64 rows
SHRUNK = {"SPL_MF_SMALL": "64", "SPL_MF_MIDMAX": "256", "SPL_MF_BIGSOLVE": "64"}
SWITCHES = ("SPL_MF_SMALL", "SPL_MF_MID", "SPL_MF_MIDMAX", "SPL_MF_MIDPAIR", "SPL_MF_BIGSOLVE", "SPL_MF_OVERLAP",
            "SPL_MF_CUT", "SPL_MF_TIMING")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("levels") / "levels_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-Wall", "-I", os.path.join(ROOT, "sparse-linear_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "levels_check.cpp"), "-o", exe], check=True)
    return exe


def poisson(m, dim):
    T = sp.diags([-np.ones(m - 1), 2 * np.ones(m), -np.ones(m - 1)], (-1, 0, 1))
    I = sp.identity(m)
    if dim == 2:
        return sp.kron(I, T) + sp.kron(T, I)
    return sp.kron(sp.kron(I, I), T) + sp.kron(sp.kron(I, T), I) + sp.kron(sp.kron(T, I), I)


@pytest.fixture(scope="module")
def grids():
    return {2: poisson(60, 2), 3: poisson(24, 3)}


def check(checker, S, switches, require_all=False):
    S = sp.csc_matrix(S)
    S.sort_indices()
    text = "%d %d\n%s\n%s\n" % (S.shape[0], S.nnz, " ".join(map(str, S.indptr)), " ".join(map(str, S.indices)))
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(switches)
    r = subprocess.run([checker, "256", str(int(require_all))], input=text, capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = {k: int(v) for k, v in (kv.split("=") for kv in r.stdout.split())}
    assert out["bad"] == 0 and out["fronts"] > 1 and out["plans"] >= 5
    return out


@pytest.mark.parametrize("dim", [2, 3])
def test_tables_with_default_limits(checker, grids, dim):
    out = check(checker, grids[dim], {})
    assert out["small"] > 0 and out["small"] + out["mid"] + out["large"] <= out["fronts"]


@pytest.mark.parametrize("dim", [2, 3])
def test_tables_with_shrunken_limits(checker, grids, dim):
    # 3-D, m = 24: one level holds small, medium and many-workgroup fronts at once, the upper levels fronts above 256
    # rows and pivot blocks of two super-block steps — the driver fails unless all of that is there
    out = check(checker, grids[dim], SHRUNK, require_all=dim == 3)
    assert out["small"] > 0 and out["mid"] > 0 and out["big"] > 0
    if dim == 3:
        assert out["large"] > 0 and out["all_three_levels"] > 0 and out["multi_step_levels"] > 0 and out["gemv_scratch"] > 0


def test_tables_without_paired_steps(checker, grids):
    out = check(checker, grids[3], dict(SHRUNK, SPL_MF_MIDPAIR="0"), require_all=True)
    assert out["mid"] > 0


def test_tables_without_medium_fronts(checker, grids):
    out = check(checker, grids[3], dict(SHRUNK, SPL_MF_MID="0"))
    assert out["mid"] == 0 and out["small"] > 0 and out["large"] > 0


def test_switches_keep_their_clamping(checker, grids):
    knobs = ("small_limit", "mid_limit", "big_solve", "mid_paired", "overlap", "forced_cut", "timing")

    def read(**switches):
        out = check(checker, grids[2], switches)
        return tuple(out[k] for k in knobs)

    assert read() == (128, 4096, 128, 1, 1, -1, 0)
    assert read(SPL_MF_SMALL="10", SPL_MF_BIGSOLVE="1") == (64, 4096, 64, 1, 1, -1, 0)  # at least 64
    assert read(SPL_MF_SMALL="500", SPL_MF_MIDMAX="300") == (500, 500, 128, 1, 1, -1, 0)  # mid_limit >= small_limit
    assert read(SPL_MF_SMALL="96", SPL_MF_MID="0", SPL_MF_MIDMAX="300") == (96, 96, 128, 1, 1, -1, 0)  # no medium class
    assert read(SPL_MF_MIDPAIR="0", SPL_MF_OVERLAP="0", SPL_MF_CUT="3", SPL_MF_TIMING="") == (128, 4096, 128, 0, 0, 3, 1)
    assert read(SPL_MF_MIDPAIR="2", SPL_MF_OVERLAP="1", SPL_MF_CUT="-4") == (128, 4096, 128, 1, 1, 0, 0)  # forced, from 0 up
