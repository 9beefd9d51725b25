#!/usr/bin/env python3
"""Cost of the per-turn alive series (count_every_turn) on one engine (DESIGN.md "K1t per-turn
counts").

On a W x H torus from fill_random(3): an engine with count_every_turn and one without, each
warmed up with one step of --turns turns, then --reps steps of --turns turns in one call each,
host wall clock around step() + sync().  Prints the best us per turn of both, the launch plan
of the counted step (turns per launch x kernel) and turn_counts(turns done, 1).
GOL_COUNT_BLOCKING=0 in the environment times the one-turn launches of a library that has the
fused multi-turn counts.  Public Python API only: --pkg selects another checkout's package
directory (the parent commit's, to time its library with the same file).

The measurement runs in a child process under a time limit; the first error ends it, and nothing
touches the GPU after that.
"""
import argparse
import collections
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed(e, turns, reps):
    e.fill_random(3)
    e.step(turns)                                          # warm-up (clock, first launches)
    e.sync()
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        e.step(turns)
        e.sync()
        dt = (time.perf_counter() - t0) * 1e6 / turns
        best = dt if best is None or dt < best else best
    return best


def measure(a):
    sys.path.insert(0, os.path.abspath(a.pkg))
    import gol
    from gol import _native as N
    print(f"library {N.LIB_PATH} source {N.lib().gol_source_id().decode()}", flush=True)
    with gol.Engine(a.width, a.height, device=0, count_every_turn=True) as e:
        us_cnt = timed(e, a.turns, a.reps)
        plan = collections.Counter((k, kern) for k, kern, _ in e.last_launches())
        tiles = sorted({(tw, seg) for tw, seg, _ in e.last_launch_tiles() if seg})
        info = e.info()
        last = int(e.turn_counts(e.turn, 1)[0])
        print(f"counted   {a.width} x {a.height}: {us_cnt:.3f} us per turn over {a.turns} turns; "
              f"launches " + ", ".join(f"{n} x {k} turns (kernel {kern})"
                                       for (k, kern), n in sorted(plan.items(), reverse=True)) +
              f"; tiles {tiles}; turns_per_launch {info.turns_per_launch} band {info.band_rows} "
              f"shape_source {info.shape_source}", flush=True)
        print(f"turn_counts({e.turn}, 1) = {last}", flush=True)
    with gol.Engine(a.width, a.height, device=0) as e:
        us_plain = timed(e, a.turns, a.reps)
        print(f"uncounted {a.width} x {a.height}: {us_plain:.3f} us per turn over {a.turns} turns",
              flush=True)
    print(f"RESULT width={a.width} height={a.height} turns={a.turns} counted_us={us_cnt:.4f} "
          f"uncounted_us={us_plain:.4f} ratio={us_cnt / us_plain:.3f}", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--turns", type=int, default=10000, help="turns per step() call")
    ap.add_argument("--reps", type=int, default=3, help="timed steps (the best counts)")
    ap.add_argument("--pkg", default=os.path.join(ROOT, "conway-s-gol-distributed_amd"))
    ap.add_argument("--timeout", type=int, default=240, help="seconds for the whole measurement")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.turns < 1 or a.reps < 1:
        ap.error("--turns and --reps must be positive")
    if a.child:
        measure(a)
        return 0
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + sys.argv[1:],
                       timeout=a.timeout)
    return r.returncode


if __name__ == "__main__":
    sys.exit(main())
