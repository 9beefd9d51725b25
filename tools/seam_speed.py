#!/usr/bin/env python3
"""Time per turn of gol_step on boards whose width is no multiple of 128, two libraries side by
side ("K1t across the row seam").

    python tools/seam_speed.py --base exp_build/parent/libgolamd.so [--new build/libgolamd.so]
                               [--repeats 3] [--log profiles/NAME.log]

For every board the two libraries alternate in child processes (one engine per process, so no
tune cache or clock state is shared): gol_fill_random(seed), 100 turns whose board is hashed,
a warm-up, then at least 0.5 s of gol_step calls ended by one gol_sync.  The boards of the two
sides must hash alike.  A board's spread is the range of its repeats; the boards listed as
neighbours (a fast-path width beside a seam width) run on the new library only.

The child binds the handful of calls it needs by hand: a base library from before this tool
lacks the newer symbols of gol/_native.py.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "conway-s-gol-distributed_amd"))

BOARDS = [(1000, 1000), (1920, 1080), (5000, 5000), (10000, 10000), (4160, 4160)]
NEIGHBOURS = [(5120, 5120), (9984, 9984)]
NEEDED = ("gol_create", "gol_destroy", "gol_get_info", "gol_sync", "gol_fill_random", "gol_step",
          "gol_last_launches", "gol_last_launch_tiles", "gol_read_packed")


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

    ok(L.gol_create(w, h, 0, C.byref(ctx)))
    info = N.gol_info()
    ok(L.gol_get_info(ctx, C.byref(info)))
    ok(L.gol_fill_random(ctx, seed))
    ok(L.gol_step(ctx, 100))
    ok(L.gol_sync(ctx))
    words = (C.c_uint64 * (h * info.words_per_row))()
    ok(L.gol_read_packed(ctx, words))
    digest = hashlib.sha256(bytes(words)).hexdigest()[:16]
    cap = 8
    arr = [(C.c_int32 * cap)() for _ in range(7)]
    L.gol_last_launches(ctx, arr[0], arr[1], arr[2], cap)
    L.gol_last_launch_tiles(ctx, arr[3], arr[4], arr[5], arr[6], cap)
    first = dict(k=arr[0][0], kernel=arr[1][0], band=arr[2][0], tw=arr[3][0], code=arr[4][0],
                 waves=arr[5][0])
    block = 256
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
                          tpl=info.turns_per_launch, fast_path=info.fast_path, first=first,
                          turns=n * block, seconds=round(dt, 4),
                          us_per_turn=round(dt / (n * block) * 1e6, 4),
                          gcups=round(w * h * n * block / dt / 1e9, 1), sha=digest)))


def run_child(lib_path, w, h, seed, min_s):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib_path, str(w),
                          str(h), str(seed), str(min_s)], capture_output=True, text=True,
                         timeout=120)
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

    sides = ([("base", os.path.abspath(a.base))] if a.base else []) + [("new", os.path.abspath(a.new))]
    rows = []
    for (w, h) in BOARDS + NEIGHBOURS:
        res = {name: [] for name, _ in sides}
        for rep in range(a.repeats):
            for name, path in sides:
                if name == "base" and (w, h) in NEIGHBOURS:
                    continue
                r = run_child(path, w, h, 1000 + w, a.min_seconds)
                r["side"] = name
                res[name].append(r)
                emit(json.dumps(r))
        shas = {r["sha"] for rs in res.values() for r in rs}
        if len(shas) != 1:
            raise SystemExit(f"{w}x{h}: the boards differ: {shas}")
        rows.append((w, h, res))
    emit("")
    emit("board        side  us/turn (min .. max)        GCUPS (best)  turns/launch  first launch")
    for w, h, res in rows:
        for name, rs in res.items():
            if not rs:
                continue
            us = sorted(r["us_per_turn"] for r in rs)
            f = rs[0]["first"]
            emit(f"{w}x{h:<6} {name:<5} {us[0]:9.3f} .. {us[-1]:9.3f}   {max(r['gcups'] for r in rs):12.1f}"
                 f"  {rs[0]['tpl']:12d}  k={f['k']} kernel={f['kernel']} tile={f['tw']}x{f['band']}"
                 f" code={f['code']} waves={f['waves']}")
        if "base" in res and res["base"] and res["new"]:
            b = [r["us_per_turn"] for r in res["base"]]
            n = [r["us_per_turn"] for r in res["new"]]
            spread = max(max(b) - min(b), max(n) - min(n))
            emit(f"{w}x{h:<6} new below base by {min(b) - max(n):.3f} us at least (spread {spread:.3f}):"
                 f" {'yes' if min(b) - max(n) > spread else 'NO'}; ratio of the medians "
                 f"{sorted(b)[len(b) // 2] / sorted(n)[len(n) // 2]:.2f}x")


if __name__ == "__main__":
    main()
