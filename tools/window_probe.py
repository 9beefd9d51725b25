#!/usr/bin/env python3
"""What looking at a running board costs: step(K); <read>; step(K) with the window calls, and
with the cheapest whole-board route of a library that lacks them ("Windows").

    python tools/window_probe.py [--base exp_build/parent/libgolamd.so] [--new build/libgolamd.so]
                                 [--boards 16384,65536] [--runs 10] [--log profiles/NAME.log]

Boards 16384^2 and 65536^2, gol_fill_random(3), K = the engine's own turns per launch.  After one
warm-up of every call, each figure is the median (and the range) of `runs` timings, host wall
clock, of

    gol_step(K); <read>; gol_step(K); gol_sync

    floor     no read at all: the two steps alone
    window    gol_read_window(x, y, 1024, 1024) in the board's middle
    density   gol_window_density(0, 0, W, H, W // 1024): a 1024 x 1024 thumbnail of the board
    packed    gol_read_packed, the cheapest whole-board route (W x H / 8 host bytes)

and of one gol_write_window of 1024 x 1024 cells alone (write).  The new library runs all of
them, the base library floor and packed; the libraries alternate in child processes (one engine
per process).  The new side also reports gol_board_layout before and after its reads: the
structural criterion is that a window read leaves it alone, so the second step converts nothing.

The child binds the calls it needs by hand: a base library from before this tool lacks the newer
symbols of gol/_native.py.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "conway-s-gol-distributed_amd"))

COMMON = ("gol_create", "gol_destroy", "gol_get_info", "gol_sync", "gol_fill_random", "gol_step",
          "gol_read_packed", "gol_snapshot")
WINDOW = ("gol_read_window", "gol_window_density", "gol_write_window", "gol_board_layout")
WIN = 1024


def child(lib_path, size, runs, has_windows):
    import numpy as np
    from gol import _native as N          # (the structures and signatures; the library is ours)
    L = C.CDLL(lib_path)
    for name in COMMON + (WINDOW if has_windows else ()):
        res, args = N.SIGNATURES[name]
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    ctx = C.c_void_p()

    def ok(rc):
        if rc < 0:
            raise SystemExit(f"gol call failed: {rc}")
        return rc

    w = h = size
    ok(L.gol_create(w, h, 0, C.byref(ctx)))
    info = N.gol_info()
    ok(L.gol_get_info(ctx, C.byref(info)))
    K = info.turns_per_launch
    ok(L.gol_fill_random(ctx, 3))
    packed = np.zeros((h, w // 64), np.uint64)
    win = np.zeros((WIN, WIN), np.uint8)
    block = w // 1024
    dens = np.zeros((1024, 1024), np.uint32)
    turn = C.c_int64()
    x0 = y0 = size // 2 - WIN // 2 + 37   # (no multiple of 64)
    u32p = C.POINTER(C.c_uint32)
    reads = {
        "floor": lambda: 0,
        "packed": lambda: L.gol_read_packed(ctx, packed.ctypes.data_as(N._u64p)),
    }
    if has_windows:
        reads["window"] = lambda: L.gol_read_window(ctx, x0, y0, WIN, WIN,
                                                    win.ctypes.data_as(N._u8p), C.byref(turn))
        reads["density"] = lambda: L.gol_window_density(ctx, 0, 0, w, h, block,
                                                        dens.ctypes.data_as(u32p), C.byref(turn))
    out = dict(size=size, lib=os.path.basename(os.path.dirname(lib_path)) or lib_path, K=K, ms={})
    layouts = {}
    for name, read in reads.items():
        ts = []
        for i in range(runs + 1):         # (the first one is the warm-up)
            t0 = time.perf_counter()
            ok(L.gol_step(ctx, K))
            if has_windows and i == runs:
                before = L.gol_board_layout(ctx)
            ok(read())
            if has_windows and i == runs:
                layouts[name] = (before, L.gol_board_layout(ctx))
            ok(L.gol_step(ctx, K))
            ok(L.gol_sync(ctx))
            ts.append((time.perf_counter() - t0) * 1e3)
        out["ms"][name] = ts[1:]
    if has_windows:
        out["layout_before_after"] = layouts
        alive = C.c_int64()
        ok(reads["density"]())             # (the same board as the snapshot below)
        ok(L.gol_snapshot(ctx, C.byref(turn), C.byref(alive)))
        out["density_sum_matches_snapshot"] = bool(int(dens.sum()) == alive.value)
        out["window_alive"] = int((win == 255).sum())
        patch = np.where(np.random.default_rng(1).integers(0, 2, (WIN, WIN)) > 0, 255, 0)
        patch = np.ascontiguousarray(patch, np.uint8)
        ts = []
        for i in range(runs + 1):
            t0 = time.perf_counter()
            ok(L.gol_write_window(ctx, x0, y0, WIN, WIN, patch.ctypes.data_as(N._u8p)))
            ts.append((time.perf_counter() - t0) * 1e3)
        out["ms"]["write"] = ts[1:]
    L.gol_destroy(ctx)
    print(json.dumps(out))


def run_child(lib_path, size, runs, has_windows):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib_path, str(size),
                          str(runs), str(int(has_windows))], capture_output=True, text=True,
                         timeout=600)
    if out.returncode != 0:
        raise SystemExit(f"child failed ({lib_path}, {size}): {out.stdout}{out.stderr}")
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs=4)
    ap.add_argument("--base")
    ap.add_argument("--new", default=os.path.join(ROOT, "conway-s-gol-distributed_amd", "build",
                                                  "libgolamd.so"))
    ap.add_argument("--boards", default="16384,65536")
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--log")
    a = ap.parse_args()
    if a.child:
        lib_path, size, runs, hw = a.child
        return child(lib_path, int(size), int(runs), bool(int(hw)))
    log = open(a.log, "w") if a.log else None

    def emit(s):
        print(s, flush=True)
        if log:
            log.write(s + "\n")
            log.flush()

    rows = []
    for size in (int(s) for s in a.boards.split(",")):
        sides = ([("base", os.path.abspath(a.base), False)] if a.base else []) + \
                [("new", os.path.abspath(a.new), True)]
        for name, path, hw in sides:
            r = run_child(path, size, a.runs, hw)
            r["side"] = name
            emit(json.dumps(r))
            rows.append(r)
    emit("")
    emit("board   side  K   call      median ms   (min .. max)        over the floor")
    for r in rows:
        floor = statistics.median(r["ms"]["floor"])
        for call, ts in r["ms"].items():
            med = statistics.median(ts)
            over = "" if call in ("floor", "write") else f"{med - floor:10.3f}"
            emit(f"{r['size']:<7d} {r['side']:<5} {r['K']:<3d} {call:<9} {med:10.3f}   "
                 f"({min(ts):.3f} .. {max(ts):.3f})   {over}")
        if "layout_before_after" in r:
            emit(f"{r['size']:<7d} {r['side']:<5} layout before / after each read: "
                 f"{r['layout_before_after']}; density sums to the snapshot: "
                 f"{r['density_sum_matches_snapshot']}")


if __name__ == "__main__":
    main()
