#!/usr/bin/env python3
"""spl_vector_gram_dev (csrc/gram.hip) on one MI355X: G = V^H W of (k, l) = (10, 10), (30, 30), (60, 60), (128, 128)
columns of n = 8.0e6 entries, real and complex, at the register tiles 1, 2 and 4 (SPL_GRAM_TILE; the default is the
library's), against

  * the loop of l spl_vector_dots_dev calls that produces the same bits (what the library offered before), and
  * a device-to-device copy of the n (k + l) entries any pass must at least read.

Per cell: the ratios, the rate of the bytes that must move (n (k + l) entries over the time) and the unfused arithmetic
rate (2 k l n real operations, 8 k l n complex).  Every case is warmed up; a time is a host clock around a call that ends
in a device synchronise; medians of --rounds with [min, max].  Nothing is asserted about a ratio: it is recorded.
Prints one JSON line (and writes it to --out).
python tools/bench_gram.py [--n 8000000] [--rounds 3] [--shapes 10,30,60,128] [--out profiles/gram_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KNOBS = ("SPL_KRYLOV_GRID", "SPL_GMRES_DOTS_BATCH", "SPL_GRAM_TILE", "SPL_GRAM_SCRATCH")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8_000_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", default="10,30,60,128")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    torch.cuda.set_device(0)
    for name in KNOBS:
        os.environ.pop(name, None)

    def clock(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def timed(f, rounds, warmup=1):
        for _ in range(warmup):
            clock(f)
        ts = [clock(f) for _ in range(rounds)]
        return statistics.median(ts), {"ms": round(statistics.median(ts) * 1e3, 4),
                                       "ms_min_max": [round(min(ts) * 1e3, 4), round(max(ts) * 1e3, 4)]}

    n = args.n
    stream = torch.cuda.current_stream().cuda_stream
    cells = []
    for cplx in (False, True):
        dtype = torch.complex128 if cplx else torch.float64
        step = 16 if cplx else 8
        for k in (int(v) for v in args.shapes.split(",")):
            l = k
            V = (torch.rand(k * n, dtype=torch.float64, device="cuda") - 0.5).to(dtype)
            W = (torch.rand(l * n, dtype=torch.float64, device="cuda") - 0.5).to(dtype)
            G = torch.zeros(k * l, dtype=dtype, device="cuda")
            G2 = torch.zeros(k * l, dtype=dtype, device="cuda")

            def loop():
                for j in range(l):
                    pkg.vector_dots_dev(n, k, V.data_ptr(), n, W.data_ptr() + j * n * step, G2.data_ptr() + j * k * step,
                                        cplx, stream)

            def gram(upper=False):
                pkg.vector_gram_dev(n, k, l, V.data_ptr(), n, W.data_ptr(), n, G.data_ptr(), k, upper, cplx, stream)

            m_loop, t_loop = timed(loop, args.rounds)
            by_tile = {}
            for tile in ("1", "2", "4"):
                os.environ["SPL_GRAM_TILE"] = tile
                m, t = timed(gram, args.rounds)
                by_tile[tile] = dict(t, loop_over_gram=round(m_loop / m, 2))
            os.environ.pop("SPL_GRAM_TILE", None)
            m_def, t_def = timed(gram, args.rounds)
            same = bool((G.view(torch.int64) == G2.view(torch.int64)).all())
            m_up, t_up = timed(lambda: gram(True), args.rounds)
            m_copy, t_copy = timed(lambda: W.copy_(V), args.rounds)  # reads n k entries and writes n l: k == l
            cell = {"values": "complex" if cplx else "real", "n": n, "k": k, "l": l, "loop_of_l_dots_calls": t_loop,
                    "gram_by_tile": by_tile, "gram_default_tile": t_def, "gram_upper_default_tile": t_up,
                    "copy_of_k_plus_l_columns": t_copy, "same_bits_as_the_loop": same,
                    "loop_over_gram": round(m_loop / m_def, 2), "gram_over_copy": round(m_def / m_copy, 2),
                    "must_move_GBps": round((k + l) * n * step / m_def / 1e9, 1),
                    "unfused_Gflops": round((8 if cplx else 2) * k * l * n / m_def / 1e9, 1)}
            print("%r" % (cell,), file=sys.stderr, flush=True)
            cells.append(cell)
            del V, W, G, G2
            torch.cuda.empty_cache()
    result = {"what": "tools/bench_gram.py: spl_vector_gram_dev against the loop of spl_vector_dots_dev calls and a copy, "
                      "one MI355X; host clock ending in a synchronise, medians of %d after a warm-up" % args.rounds,
              "device": torch.cuda.get_device_name(0), "cells": cells}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(os.path.join(ROOT, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
