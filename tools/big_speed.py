#!/usr/bin/env python3
"""Time per turn of gol_step on boards of 2 GiB and more per buffer, two libraries side by side,
and the cost of k_step_tile's big form itself at 65536^2 ("K1t on boards of 2 GiB and
more").

    python tools/big_speed.py --base exp_build/parent/libgolamd.so [--new build/libgolamd.so]
                              [--repeats 3] [--log profiles/NAME.log]

Boards (131072^2, 262144^2): the two libraries alternate in child processes (one engine per
process, so no tune cache or clock state is shared): gol_fill_random(seed), 60 turns whose alive
count is compared between the sides (the boards are too large to read back and hash), a warm-up,
then at least 0.5 s of gol_step calls ended by one gol_sync.  A board's spread is the range of
its repeats.

The form's cost: the new library at 65536^2 on its pinned shape (30 lanes x 452 rows, code 516,
30 turns per launch), with and without GOL_TILE_BIG=1 in the child's environment, alternating.

The child binds the handful of calls it needs by hand: a base library from before this tool
lacks the newer symbols of gol/_native.py.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "conway-s-gol-distributed_amd"))

BOARDS = [(131072, 131072), (262144, 262144)]
FORM_BOARD = (65536, 65536)
NEEDED = ("gol_create", "gol_destroy", "gol_get_info", "gol_sync", "gol_fill_random", "gol_step",
          "gol_last_launches", "gol_last_launch_tiles", "gol_snapshot")


def child(lib_path, w, h, seed, min_s):
    from gol import _native as N          # (the structures and signatures; the library is ours)
    L = C.CDLL(lib_path)
    for name in NEEDED:
        res, args = N.SIGNATURES[name]
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    ctx = C.c_void_p()

    def ok(rc):
        if rc < 0:
            raise SystemExit(f"gol call failed: {rc}")

    t0 = time.perf_counter()
    ok(L.gol_create(w, h, 0, C.byref(ctx)))
    create_s = time.perf_counter() - t0
    info = N.gol_info()
    ok(L.gol_get_info(ctx, C.byref(info)))
    ok(L.gol_fill_random(ctx, seed))
    ok(L.gol_step(ctx, 60))
    turn, alive = C.c_int64(), C.c_int64()
    ok(L.gol_snapshot(ctx, C.byref(turn), C.byref(alive)))
    cap = 8
    arr = [(C.c_int32 * cap)() for _ in range(7)]
    L.gol_last_launches(ctx, arr[0], arr[1], arr[2], cap)
    L.gol_last_launch_tiles(ctx, arr[3], arr[4], arr[5], arr[6], cap)
    first = dict(k=arr[0][0], kernel=arr[1][0], band=arr[2][0], tw=arr[3][0], code=arr[4][0],
                 waves=arr[5][0])
    block = 240                            # (whole launches at 20, 24 and 30 turns per launch)
    for _ in range(2):                     # warm-up, and the time of one block of turns
        t0 = time.perf_counter()
        ok(L.gol_step(ctx, block))
        ok(L.gol_sync(ctx))
        t1 = time.perf_counter() - t0
    n = max(1, int(min_s * 1.2 / t1) + 1)
    t0 = time.perf_counter()
    for _ in range(n):
        ok(L.gol_step(ctx, block))
    ok(L.gol_sync(ctx))
    dt = time.perf_counter() - t0
    L.gol_destroy(ctx)
    print(json.dumps(dict(w=w, h=h, lib=os.path.basename(os.path.dirname(lib_path)) or lib_path,
                          big_env=os.environ.get("GOL_TILE_BIG", ""),
                          tpl=info.turns_per_launch, blocking_limited=info.blocking_limited,
                          first=first, create_s=round(create_s, 2), turns=n * block,
                          seconds=round(dt, 4), us_per_turn=round(dt / (n * block) * 1e6, 3),
                          gcups=round(w * h * n * block / dt / 1e9, 1), alive60=alive.value)))


def run_child(lib_path, w, h, seed, min_s, env=None):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib_path, str(w),
                          str(h), str(seed), str(min_s)], capture_output=True, text=True,
                         timeout=300, env=dict(os.environ, **(env or {})))
    if out.returncode != 0:
        raise SystemExit(f"child failed ({lib_path}, {w}x{h}): {out.stdout}{out.stderr}")
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs=5)
    ap.add_argument("--base")
    ap.add_argument("--new", default=os.path.join(ROOT, "conway-s-gol-distributed_amd", "build",
                                                  "libgolamd.so"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--boards", default="all", help="all, or WxH[,WxH...]")
    ap.add_argument("--log")
    a = ap.parse_args()
    if a.child:
        lib_path, w, h, seed, min_s = a.child
        return child(lib_path, int(w), int(h), int(seed), float(min_s))
    log = open(a.log, "w") if a.log else None

    def emit(s):
        print(s, flush=True)
        if log:
            log.write(s + "\n")
            log.flush()

    new = os.path.abspath(a.new)
    boards = BOARDS if a.boards == "all" else [tuple(int(v) for v in b.split("x"))
                                               for b in a.boards.split(",")]
    # (side, library, environment): the two libraries on the big boards, the two forms at 65536^2
    runs = [(b, [("base", os.path.abspath(a.base), {})] if a.base else []) for b in boards]
    for _, sides in runs:
        sides.append(("new", new, {}))
    runs.append((FORM_BOARD, [("plain", new, {}), ("big", new, {"GOL_TILE_BIG": "1"})]))
    rows = []
    for (w, h), sides in runs:
        res = {name: [] for name, _, _ in sides}
        for rep in range(a.repeats):
            for name, path, env in sides:
                r = run_child(path, w, h, 1000 + w, a.min_seconds, env)
                r["side"] = name
                res[name].append(r)
                emit(json.dumps(r))
        counts = {r["alive60"] for rs in res.values() for r in rs}
        if len(counts) != 1:
            raise SystemExit(f"{w}x{h}: the alive counts after 60 turns differ: {counts}")
        rows.append((w, h, res))
    emit("")
    emit("board          side   us/turn (min .. max)        GCUPS (best)  turns/launch  first launch")
    for w, h, res in rows:
        for name, rs in res.items():
            us = sorted(r["us_per_turn"] for r in rs)
            f = rs[0]["first"]
            emit(f"{w}x{h:<7} {name:<6} {us[0]:9.3f} .. {us[-1]:9.3f}   {max(r['gcups'] for r in rs):12.1f}"
                 f"  {rs[0]['tpl']:12d}  k={f['k']} kernel={f['kernel']} tile={f['tw']}x{f['band']}"
                 f" code={f['code']} waves={f['waves']} blocking_limited={rs[0]['blocking_limited']}")
        names = list(res)
        if len(names) == 2:
            b = [r["us_per_turn"] for r in res[names[0]]]
            n = [r["us_per_turn"] for r in res[names[1]]]
            spread = max(max(b) - min(b), max(n) - min(n))
            emit(f"{w}x{h:<7} {names[1]} below {names[0]} by {min(b) - max(n):.3f} us at least "
                 f"(spread {spread:.3f}): {'yes' if min(b) - max(n) > spread else 'NO'}; ratio of the "
                 f"medians {sorted(b)[len(b) // 2] / sorted(n)[len(n) // 2]:.3f}x")


if __name__ == "__main__":
    main()
