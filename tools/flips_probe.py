#!/usr/bin/env python3
"""Per-turn cost of the CellFlipped paths on one engine (DESIGN.md "K5 flip lists").

On a W x H board (default 5120^2) from fill_random(3) after 100 turns, per turn, host wall
clock from before step(1) to the result on the host (both calls synchronise):
  step(1) + flipped_cells()   the device flip list (libraries that have gol_flipped_cells)
  step(1) + read_board()      the transfer half of the host comparison it replaces
Median of --turns turns (>= 20) after 5 warm-up turns each, and the flip count and density of
the measured turns.  --pkg selects another checkout's package directory (the parent commit's, to
time its read_board path with its own library).

The measurement runs in a child process under a time limit; the first error ends it, and nothing
touches the GPU after that.
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def measure(a):
    sys.path.insert(0, os.path.abspath(a.pkg))
    import gol
    from gol import _native as N
    print(f"library {N.LIB_PATH} source {N.lib().gol_source_id().decode()}", flush=True)
    have = hasattr(gol.Engine, "flipped_cells")
    with gol.Engine(a.width, a.height, device=0) as e:
        e.fill_random(3)
        e.step(100)
        e.sync()
        cells = a.width * a.height
        if have:
            t, flips = [], []
            for i in range(5 + a.turns):
                t0 = time.perf_counter()
                e.step(1)
                f = e.flipped_cells()
                t.append((time.perf_counter() - t0) * 1e3)
                flips.append(len(f))
            t, flips = t[5:], flips[5:]
            fl = statistics.median(flips)
            print(f"step(1) + flipped_cells(): median {statistics.median(t):.3f} ms "
                  f"(min {min(t):.3f}, max {max(t):.3f}) over {len(t)} turns; "
                  f"flips per turn median {fl:.0f} = {fl / cells:.4%} of {a.width} x {a.height} "
                  f"cells, list {fl * 16 / 1e6:.2f} MB vs board bytes {cells / 1e6:.2f} MB",
                  flush=True)
        else:
            print("step(1) + flipped_cells(): not in this library", flush=True)
        t = []
        for i in range(5 + a.turns):
            t0 = time.perf_counter()
            e.step(1)
            b = e.read_board()
            t.append((time.perf_counter() - t0) * 1e3)
        t = t[5:]
        assert b.shape == (a.height, a.width)
        print(f"step(1) + read_board():    median {statistics.median(t):.3f} ms "
              f"(min {min(t):.3f}, max {max(t):.3f}) over {len(t)} turns", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--width", type=int, default=5120)
    ap.add_argument("--height", type=int, default=5120)
    ap.add_argument("--turns", type=int, default=30)
    ap.add_argument("--pkg", default=os.path.join(ROOT, "conway-s-gol-distributed_amd"))
    ap.add_argument("--timeout", type=int, default=120, help="seconds for the whole measurement")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.turns < 20:
        ap.error("--turns must be at least 20")
    if a.child:
        measure(a)
        return 0
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + sys.argv[1:],
                       timeout=a.timeout)
    return r.returncode


if __name__ == "__main__":
    sys.exit(main())
