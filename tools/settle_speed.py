#!/usr/bin/env python3
"""What watching a batch costs and what skipping settled turns saves (k_settle_resident_batch,
gol_settle_step) against gol_batch_step of a base library ("K1r2s: periods of a batch").

    python tools/settle_speed.py --base exp_build/parent/libgolamd.so [--new build/libgolamd.so]
                                 [--rounds 3] [--launches 10] [--log profiles/NAME.log]

Configurations: "settle" (the new library: gol_settle_step) and "plain" (the base library, the
parent commit's: gol_batch_step).  They alternate, one child process at a time, `rounds` times.
Both sides hold the same boards (gol_batch_fill_random of the same seed) and every time is taken
between two HIP events on the batch's stream.

(1) The price of watching: one launch of 256 turns of fresh soups, too few turns for a soup to
settle but for the odd one (the settle side counts the boards whose period it knows afterwards
and the table shows the count beside the boards run), 64 x 64 and
255 x 1024 boards, B = 256 and B = the co-resident limit of k_step_resident_batch
(gol_batch_occupancy of the new library, handed to both sides).  A sample: `launches` times a
fresh fill (a new seed each), on the settle side the start of the watch (gol_settle_step of 0
turns: a copy of the boards and 32 bytes per board, once per watch and not per launch), then the
timed 256 turns; one untimed sample first.  Reported as us per launch.

(2) The gain: 8192 turns of B = 5120 soups of 64 x 64 and of B = 1024 of 128 x 128 in one call,
the start of the watch included.  Reported as ms per call and as the count of boards whose period
was found.  The boards of both sides hash alike at the end.

"Faster" stands only where the settle range lies wholly below the base's range.

The children bind the calls they need by hand: the base library lacks the gol_settle_* symbols.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "conway-s-gol-distributed_amd"))

PRICE_BOARDS = [(64, 64), (255, 1024)]
GAIN = [(64, 64, 5120), (128, 128, 1024)]
GAIN_TURNS = 8192
DEPTH = 256
NEEDED = ("gol_batch_create", "gol_batch_destroy", "gol_batch_occupancy", "gol_batch_get_stream",
          "gol_batch_sync", "gol_batch_fill_random", "gol_batch_step", "gol_batch_read_packed")
SETTLE_NEEDED = ("gol_settle_step", "gol_settle_read")


def hip_runtime():
    """The HIP runtime the engine library brought in (already loaded: no second copy)."""
    for name in ("libamdhip64.so.7", "libamdhip64.so.6", "libamdhip64.so"):
        try:
            hip = C.CDLL(name, mode=os.RTLD_NOW | os.RTLD_NOLOAD)
            break
        except OSError:
            pass
    else:
        raise SystemExit("no loaded libamdhip64 found")
    for fn in (hip.hipEventCreate, hip.hipEventRecord, hip.hipEventSynchronize,
               hip.hipEventElapsedTime, hip.hipEventDestroy):
        fn.restype = C.c_int
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipEventDestroy.argtypes = [C.c_void_p]
    return hip


def bind(lib_path, names):
    from gol import _native as N          # (the signatures; the library is the caller's)
    L = C.CDLL(lib_path)
    for name in names:
        res, args = N.SIGNATURES[name]
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    return L


def ok(rc):
    if rc != 0:
        raise SystemExit(f"call failed: {rc}")


def probe(lib_path):
    """{board: [workgroups per CU, CUs]} from the new library."""
    L = bind(lib_path, NEEDED)
    out = {}
    for (w, h) in PRICE_BOARDS:
        b = C.c_void_p()
        ok(L.gol_batch_create(w, h, 1, -1, 0, C.byref(b)))
        per, cus = C.c_int32(), C.c_int32()
        ok(L.gol_batch_occupancy(b, C.byref(per), C.byref(cus)))
        L.gol_batch_destroy(b)
        out[f"{w}x{h}"] = [per.value, cus.value]
    print(json.dumps(out), flush=True)


def child(config, lib_path, launches, caps):
    settle = config == "settle"
    L = bind(lib_path, NEEDED + (SETTLE_NEEDED if settle else ()))
    hip = hip_runtime()
    step = L.gol_settle_step if settle else L.gol_batch_step
    e0, e1 = C.c_void_p(), C.c_void_p()
    ok(hip.hipEventCreate(C.byref(e0)))
    ok(hip.hipEventCreate(C.byref(e1)))

    def timed(b, turns, with_watch_start):
        """ms between two events around one step call."""
        stream = L.gol_batch_get_stream(b)
        if settle and not with_watch_start:
            ok(L.gol_settle_step(b, 0))
        ok(hip.hipEventRecord(e0, stream))
        ok(step(b, turns))
        ok(hip.hipEventRecord(e1, stream))
        ok(L.gol_batch_sync(b))
        ms = C.c_float()
        ok(hip.hipEventElapsedTime(C.byref(ms), e0, e1))
        return ms.value

    def known(b, B):
        """boards whose period is known (the settle side)."""
        if not settle:
            return None
        period = np.zeros(B, dtype=np.int64)
        ok(L.gol_settle_read(b, 0, B, None, period.ctypes.data_as(C.POINTER(C.c_int64))))
        return int((period != 0).sum())

    for (w, h) in PRICE_BOARDS:
        per, cus = caps[f"{w}x{h}"]
        for B in dict.fromkeys((256, per * cus)):
            b = C.c_void_p()
            ok(L.gol_batch_create(w, h, B, -1, 0, C.byref(b)))
            total, found = 0.0, 0
            for i in range(launches + 1):
                ok(L.gol_batch_fill_random(b, 2000 + i))
                ms = timed(b, DEPTH, False)
                if i:
                    total += ms
                    found += known(b, B) or 0
            got = np.zeros((B, h, (w + 63) // 64), dtype=np.uint64)
            ok(L.gol_batch_read_packed(b, 0, B, got.ctypes.data_as(C.POINTER(C.c_uint64))))
            L.gol_batch_destroy(b)
            print(json.dumps(dict(part="price", w=w, h=h, B=B, config=config,
                                  us=round(total * 1e3 / launches, 3),
                                  found=found if settle else None, board_launches=B * launches,
                                  sha=hashlib.sha256(got.tobytes()).hexdigest()[:16])), flush=True)
    for (w, h, B) in GAIN:
        b = C.c_void_p()
        ok(L.gol_batch_create(w, h, B, -1, 0, C.byref(b)))
        ok(L.gol_batch_fill_random(b, 3000))
        timed(b, DEPTH, True)                                # (untimed: the first launches)
        ok(L.gol_batch_fill_random(b, 3001))
        ms = timed(b, GAIN_TURNS, True)
        found = known(b, B)
        got = np.zeros((B, h, (w + 63) // 64), dtype=np.uint64)
        ok(L.gol_batch_read_packed(b, 0, B, got.ctypes.data_as(C.POINTER(C.c_uint64))))
        L.gol_batch_destroy(b)
        print(json.dumps(dict(part="gain", w=w, h=h, B=B, config=config, ms=round(ms, 3),
                              found=found, sha=hashlib.sha256(got.tobytes()).hexdigest()[:16])),
              flush=True)
    ok(hip.hipEventDestroy(e0))
    ok(hip.hipEventDestroy(e1))


def run_child(args):
    out = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True,
                         text=True, timeout=300)
    if out.returncode != 0:
        raise SystemExit(f"child failed ({args}): {out.stdout}{out.stderr}")
    return [json.loads(line) for line in out.stdout.strip().splitlines() if line.startswith("{")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs="+")
    ap.add_argument("--base", help="the parent commit's libgolamd.so (the reference)")
    ap.add_argument("--new", default=os.path.join(ROOT, "conway-s-gol-distributed_amd", "build",
                                                  "libgolamd.so"))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--log")
    a = ap.parse_args()
    if a.child:
        kind, path = a.child[0], a.child[1]
        if kind == "probe":
            return probe(path)
        return child(kind, path, int(a.child[2]), json.loads(a.child[3]))
    if not a.base:
        raise SystemExit("--base: the reference is the parent commit's library, never this one")
    log = open(a.log, "w") if a.log else None

    def emit(s):
        print(s, flush=True)
        if log:
            log.write(s + "\n")
            log.flush()

    new, base = os.path.abspath(a.new), os.path.abspath(a.base)
    caps = run_child(["--child", "probe", new])[0]
    emit("co-resident limit of k_step_resident_batch (workgroups per CU x CUs, gol_batch_occupancy): " +
         ", ".join(f"{k}: {v[0]} x {v[1]} = {v[0] * v[1]}" for k, v in caps.items()))
    res = {}
    for rnd in range(a.rounds):
        for config, path in (("settle", new), ("plain", base)):
            for r in run_child(["--child", config, path, str(a.launches), json.dumps(caps)]):
                r["round"] = rnd
                res.setdefault((r["part"], r["w"], r["h"], r["B"]), {}).setdefault(config, []).append(r)
                emit(json.dumps(r))
    for key, by in res.items():
        shas = {r["sha"] for rs in by.values() for r in rs}
        if len(shas) != 1:
            raise SystemExit(f"{key}: the boards differ: {shas}")

    def verdict(s, p):
        return "settle faster" if s[-1] < p[0] else "settle slower" if s[0] > p[-1] else "ranges overlap"

    emit("")
    emit(f"(1) the price of watching: us per launch of {DEPTH} turns of fresh soups "
         f"({a.launches} launches per sample, {a.rounds} rounds, min .. max)")
    emit("board      B      gol_settle_step         base gol_batch_step     settle / base (medians)")
    for (part, w, h, B), by in res.items():
        if part != "price":
            continue
        s = sorted(r["us"] for r in by["settle"])
        p = sorted(r["us"] for r in by["plain"])
        found = sum(r["found"] for r in by["settle"])
        ran = sum(r["board_launches"] for r in by["settle"])
        emit(f"{w}x{h:<6} {B:<6d} {s[0]:9.2f} .. {s[-1]:9.2f}  {p[0]:9.2f} .. {p[-1]:9.2f}  "
             f"{s[len(s) // 2] / p[len(p) // 2]:6.3f}   {verdict(s, p)}   "
             f"({found} of {ran} boards settled within the launch)")
    emit("")
    emit(f"(2) the gain: ms per call of {GAIN_TURNS} turns of soups ({a.rounds} rounds, min .. max)")
    emit("board      B      gol_settle_step         base gol_batch_step     base / settle (medians)  "
         "periods found")
    for (part, w, h, B), by in res.items():
        if part != "gain":
            continue
        s = sorted(r["ms"] for r in by["settle"])
        p = sorted(r["ms"] for r in by["plain"])
        found = sorted({r["found"] for r in by["settle"]})
        emit(f"{w}x{h:<6} {B:<6d} {s[0]:9.3f} .. {s[-1]:9.3f}  {p[0]:9.3f} .. {p[-1]:9.3f}  "
             f"{p[len(p) // 2] / s[len(s) // 2]:6.2f}x  {verdict(s, p)}   {found} of {B}")
    emit("")
    emit("the boards of both sides hash alike in every case")


if __name__ == "__main__":
    main()
