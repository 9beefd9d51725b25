#!/usr/bin/env python3
"""Time per turn of gol_step on boards narrower than 256 cells: k_step_resident
(GOL_FLAG_RESIDENT) against the same library without the flag and against a base library
("K1r2: resident boards").

    python tools/resident_speed.py [--base exp_build/parent/libgolamd.so] [--new build/libgolamd.so]
                                   [--rounds 3] [--turns 100000] [--log profiles/NAME.log]

Configurations: "on" (the flag, the partition rule's rows per lane R), "on_x2" / "on_x4" (the
flag with GOL_RESIDENT_ROWS = 2 R / 4 R on the boards where the kernel is built for that and
the board fits: fewer lanes, fewer wavefronts), "off" (the new library without the flag) and
"base" (the base library, which knows no flag).  They alternate, one child process at a time,
`rounds` times; a child runs every board: gol_fill_random(seed), a warm-up step of 1000 turns
whose board is hashed, then `turns` turns between two HIP events on the engine's stream, and the
board is hashed again.  All configurations must hash alike.  A board's spread is the largest
range any configuration's rounds show on it.

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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "conway-s-gol-distributed_amd"))

BOARDS = [(16, 16), (64, 64), (128, 128), (200, 77), (255, 1024), (64, 4096)]
NEEDED = ("gol_create", "gol_destroy", "gol_get_info", "gol_get_stream", "gol_sync",
          "gol_fill_random", "gol_step", "gol_last_launches", "gol_read_packed")
FLAG_RESIDENT = 0x8
WARMUP = 1000


def hip_runtime():
    """The HIP runtime the engine library brought in (already loaded: no second copy)."""
    for name in ("libamdhip64.so.7", "libamdhip64.so.6", "libamdhip64.so"):
        try:
            return C.CDLL(name, mode=os.RTLD_NOW | os.RTLD_NOLOAD)
        except OSError:
            pass
    raise SystemExit("no loaded libamdhip64 found")


def alt_rows(w, h, rows, mult):
    """mult x rows where k_step_resident is built for it and the board fits 256 lanes, else 0."""
    nw, r = (w + 63) // 64, rows * mult
    built = r * nw <= 16 and (r & (r - 1) == 0 or r == 16 // nw)
    return r if built and -(-h // r) <= 256 else 0


def child(lib_path, config, turns):
    from gol import _native as N          # (the structures and signatures; the library is ours)
    L = C.CDLL(lib_path)
    for name in NEEDED:
        res, args = N.SIGNATURES[name]
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    hip = hip_runtime()
    for fn in (hip.hipEventCreate, hip.hipEventRecord, hip.hipEventSynchronize,
               hip.hipEventElapsedTime, hip.hipEventDestroy):
        fn.restype = C.c_int
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipEventDestroy.argtypes = [C.c_void_p]

    def ok(rc):
        if rc != 0:
            raise SystemExit(f"call failed: {rc}")

    mult = {"on_x2": 2, "on_x4": 4}.get(config, 0)
    flags = FLAG_RESIDENT if config.startswith("on") else 0
    for (w, h) in BOARDS:
        os.environ.pop("GOL_RESIDENT_ROWS", None)
        rows = 0
        if flags:
            L.gol_resident_plan.restype = C.c_int32
            a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
            ok(L.gol_resident_plan(w, h, C.byref(a), C.byref(b), C.byref(c)))
            rows = b.value
            if mult:
                rows = alt_rows(w, h, rows, mult)
                if not rows:
                    continue                   # (no such partition of this board)
                os.environ["GOL_RESIDENT_ROWS"] = str(rows)
        ctx = C.c_void_p()
        ok(L.gol_create(w, h, flags, C.byref(ctx)))
        info = N.gol_info()
        ok(L.gol_get_info(ctx, C.byref(info)))
        stream = L.gol_get_stream(ctx)
        words = (C.c_uint64 * (h * info.words_per_row))()

        def digest():
            ok(L.gol_read_packed(ctx, words))
            return hashlib.sha256(bytes(words)).hexdigest()[:16]

        ok(L.gol_fill_random(ctx, 1000 + w))
        ok(L.gol_step(ctx, WARMUP))
        sha_warm = digest()
        cap = 4
        arr = [(C.c_int32 * cap)() for _ in range(3)]
        L.gol_last_launches(ctx, arr[0], arr[1], arr[2], cap)
        e0, e1 = C.c_void_p(), C.c_void_p()
        ok(hip.hipEventCreate(C.byref(e0)))
        ok(hip.hipEventCreate(C.byref(e1)))
        ok(hip.hipEventRecord(e0, stream))
        ok(L.gol_step(ctx, turns))
        ok(hip.hipEventRecord(e1, stream))
        ok(hip.hipEventSynchronize(e1))
        ms = C.c_float()
        ok(hip.hipEventElapsedTime(C.byref(ms), e0, e1))
        ok(L.gol_sync(ctx))
        sha_end = digest()
        ok(hip.hipEventDestroy(e0))
        ok(hip.hipEventDestroy(e1))
        L.gol_destroy(ctx)
        print(json.dumps(dict(w=w, h=h, config=config, tpl=info.turns_per_launch, rows=rows,
                              k=arr[0][0], kernel=arr[1][0], turns=turns,
                              us_per_turn=round(ms.value * 1e3 / turns, 4),
                              sha=sha_warm + sha_end)), flush=True)


def run_child(lib_path, config, turns):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib_path, config,
                          str(turns)], capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        raise SystemExit(f"child failed ({lib_path}, {config}): {out.stdout}{out.stderr}")
    return [json.loads(line) for line in out.stdout.strip().splitlines() if line.startswith("{")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs=3)
    ap.add_argument("--base")
    ap.add_argument("--new", default=os.path.join(ROOT, "conway-s-gol-distributed_amd", "build",
                                                  "libgolamd.so"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--turns", type=int, default=100000)
    ap.add_argument("--log")
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1], int(a.child[2]))
    log = open(a.log, "w") if a.log else None

    def emit(s):
        print(s, flush=True)
        if log:
            log.write(s + "\n")
            log.flush()

    new = os.path.abspath(a.new)
    sides = [("on", new), ("on_x2", new), ("on_x4", new), ("off", new)]
    if a.base:
        sides.append(("base", os.path.abspath(a.base)))
    res = {}
    for rnd in range(a.rounds):
        for config, path in sides:
            for r in run_child(path, config, a.turns):
                r["round"] = rnd
                res.setdefault((r["w"], r["h"]), {}).setdefault(config, []).append(r)
                emit(json.dumps(r))
    emit("")
    emit(f"us per turn, {a.turns} turns per sample, {a.rounds} rounds (min .. max)")
    emit("board      config  rows/lane  turns/launch  kernel   us/turn min ..      max")
    failed = []
    for (w, h) in BOARDS:
        by = res.get((w, h), {})
        shas = {r["sha"] for rs in by.values() for r in rs}
        if len(shas) != 1:
            raise SystemExit(f"{w}x{h}: the boards differ: {shas}")
        for config, _ in sides:
            rs = by.get(config)
            if not rs:
                continue
            us = sorted(r["us_per_turn"] for r in rs)
            emit(f"{w}x{h:<6} {config:<7} {rs[0]['rows']:9d}  {rs[0]['tpl']:12d}  {rs[0]['kernel']:6d}"
                 f"  {us[0]:10.4f} .. {us[-1]:10.4f}")
        spread = max(max(r["us_per_turn"] for r in rs) - min(r["us_per_turn"] for r in rs)
                     for rs in by.values())
        if "base" in by:
            on = [r["us_per_turn"] for r in by["on"]]
            off = [r["us_per_turn"] for r in by["off"]]
            base = [r["us_per_turn"] for r in by["base"]]
            med = lambda v: sorted(v)[len(v) // 2]
            faster = min(base) - max(on) > spread
            level = abs(med(off) - med(base)) <= spread
            emit(f"{w}x{h:<6} spread {spread:.4f}; on below base by more than the spread: "
                 f"{'yes' if faster else 'NO'} ({med(base) / med(on):.1f}x at the medians); "
                 f"off within the spread of base: {'yes' if level else 'NO'} "
                 f"({med(off):.4f} against {med(base):.4f})")
            if not faster or not level:
                failed.append((w, h))
    if a.base:
        emit("")
        emit("acceptance: " + ("every board passes" if not failed else f"FAILED on {failed}"))


if __name__ == "__main__":
    main()
