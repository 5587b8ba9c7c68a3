"""The two cyclic Jacobi rules of csrc/ritz_jacobi.hpp (real symmetric, complex Hermitian) are plain C++ on the host, so
they are checked on the CPU: a stand-alone program (tests/native/ritz_jacobi_check.cpp) runs both on fixed matrices of
the orders 1, 2, 3, 17 and 60 under the address and undefined-behaviour sanitizers, checks what they leave, and prints
every value and every entry of Y; here the same matrices go through the restatements (eigsh_cases.jacobi,
lobpcg_cases.jacobi_hermitian) and the two must agree BIT FOR BIT.  The same program runs the Ritz step both
eigensolvers call (ritz_step) for each of the three orders: its values are the restatement's, its order is
``sorted(range(m), key=...)`` on them (Python's sort is stable too), and a NaN or an infinity is refused.  No sanitizer
goes near code loaded into Python."""
import os
import subprocess

import eigsh_cases as EK
import lobpcg_cases as LK

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDERS = (1, 2, 3, 17, 60)


class Draws(object):
    """the generator of the native program"""

    def __init__(self):
        self.state = 0x243F6A8885A308D3

    def __call__(self):
        self.state = (self.state * 6364136223846793005 + 1442695040888963407) % 2 ** 64
        return float(self.state >> 11) * 2.0 ** -53 - 0.5


def restated():
    draw = Draws()
    lines = []
    for m in ORDERS:
        T = [[0.0] * m for _ in range(m)]
        for r in range(m):
            for c in range(r, m):
                T[r][c] = T[c][r] = draw()
        theta, Y, sweeps = EK.jacobi(T)
        lines.append(("real", m, sweeps, theta + [Y[r][c] for r in range(m) for c in range(m)]))
    for m in ORDERS:
        Tr = [[0.0] * m for _ in range(m)]
        Ti = [[0.0] * m for _ in range(m)]
        for r in range(m):
            for c in range(r, m):
                re = draw()
                im = 0.0 if r == c else draw()
                Tr[r][c] = Tr[c][r] = re
                Ti[r][c] = im
                Ti[c][r] = 0.0 if r == c else -im
        theta, Yr, Yi, sweeps = LK.jacobi_hermitian(Tr, Ti)
        lines.append(("hermitian", m, sweeps, theta + [v for r in range(m) for c in range(m) for v in (Yr[r][c], Yi[r][c])]))
    for which in range(3):
        lines.extend(restated_steps(draw, which))
    return lines


STEP_ORDERS = (1, 2, 3, 17)
KEYS = (lambda v: -v, lambda v: v, lambda v: -abs(v))  # SPL_EIGSH_largest_algebraic, smallest_algebraic, largest_magnitude


def restated_steps(draw, which):
    """the lines of run_steps(which) of the native program: the values and, as floats, the stable order"""
    def line(name, theta, sweeps):
        order = sorted(range(len(theta)), key=lambda i: KEYS[which](theta[i]))
        return ("step-%s-%d" % (name, which), len(theta), sweeps, theta + [float(i) for i in order])

    lines = []
    for m in STEP_ORDERS:
        T = [[0.0] * m for _ in range(m)]
        for r in range(m):
            for c in range(r, m):
                T[r][c] = T[c][r] = draw()
        theta, _, sweeps = EK.jacobi(T)
        lines.append(line("real", theta, sweeps))
    for m in STEP_ORDERS:
        Tr = [[0.0] * m for _ in range(m)]
        Ti = [[0.0] * m for _ in range(m)]
        for r in range(m):
            for c in range(r, m):
                Tr[r][c] = Tr[c][r] = draw()
                Ti[r][c] = 0.0 if r == c else draw()
                Ti[c][r] = 0.0 if r == c else -Ti[r][c]
        theta, _, _, sweeps = LK.jacobi_hermitian(Tr, Ti)
        lines.append(line("hermitian", theta, sweeps))
    for name, T in (("pairs", [[2.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 2.0, 0.0], [0.0, 0.0, 0.0, 1.0]]),
                    ("planted", [[2.0, 0.0, 0.0], [0.0, 1.0, 1.0], [0.0, 1.0, 1.0]]),
                    ("signs", [[-1.5, 0.0, 0.0], [0.0, 0.25, 0.0], [0.0, 0.0, 1.5]])):
        theta, _, sweeps = EK.jacobi(T)
        lines.append(line(name, theta, sweeps))
    assert lines[-3][3] == [2.0, 1.0, 2.0, 1.0] + [float(i) for i in ((0, 2, 1, 3), (1, 3, 0, 2), (0, 2, 1, 3))[which]]
    assert lines[-2][3][:3] == [2.0, 0.0, 2.0]  # the planted pair is exact, so its two copies tie
    lines.extend(("step-%s-%d" % (name, which), 2, -1, []) for name in ("nan", "inf", "nan"))  # refused: no numbers
    return lines


def test_both_rules_under_the_sanitizers_are_the_restatements(tmp_path):
    exe = str(tmp_path / "ritz_jacobi_check")
    # the sanitizer's runtime is linked into the program: nothing has to be preloaded to run it
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-I", os.path.join(ROOT, "sparse-linear_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "ritz_jacobi_check.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")  # the leak checker needs ptrace, which a container may refuse
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    got = r.stdout.strip().split("\n")
    assert got[-1] == "bad 0"
    want = restated()
    assert len(got) == len(want) + 1
    for line, (kind, m, sweeps, numbers) in zip(got, want):
        words = line.split()
        assert words[0] == kind and int(words[1]) == m and int(words[2]) == sweeps, (kind, m, words[:3], sweeps)
        native = [float.fromhex(w) for w in words[3:]]
        assert len(native) == len(numbers)
        assert [v.hex() for v in native] == [v.hex() for v in numbers], (kind, m)
