"""The growth rule of a solve's device history (csrc/history_room.hpp: room_for, shared by CG, BiCGSTAB and GMRES) is
plain C++ over a store, so it is checked on the CPU: a small native driver (tests/native/history_room_check.cpp) with a
stub store replays the calls of the solvers for max_iter in {0, 1, 63, 64, 65, 1000}, check intervals {1, 16, 100} and
restarts {1, 5, 128}, writes what the batches write, and compares every capacity with the rule the two solvers had
before it was folded.  Built with the address and undefined-behaviour sanitizers: the stub's array has exactly the
capacity, so a batch that writes past it is reported."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_history_room_rule(tmp_path):
    exe = str(tmp_path / "history_room_check")
    # the sanitizer's runtime is linked into the program: nothing has to be preloaded to run it
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-I", os.path.join(ROOT, "sparse-linear_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "history_room_check.cpp"), "-o", exe], check=True)
    # the leak checker needs ptrace, which a container may refuse; the stub frees what it allocates
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = {k: int(v) for k, v in (kv.split("=") for kv in r.stdout.split())}
    assert out["bad"] == 0 and out["runs"] == 6 * 3 * 3 * 7 and out["grows"] > out["runs"] and out["calls"] > out["grows"]
