#!/usr/bin/env python3
"""Time of one 256-turn launch of a batch of resident boards (k_step_resident_batch, gol_batch_*)
against the same boards as that many single-board resident engines of a base library
("K1r2b: batches of resident boards").

    python tools/batch_speed.py --base exp_build/parent/libgolamd.so [--new build/libgolamd.so]
                                [--rounds 3] [--launches 20] [--ref-max-boards 1024]
                                [--log profiles/NAME.log]

Configurations: "batch" (the new library: one gol_batch of B boards) and "ref" (the base
library, the parent commit's: B engines with GOL_FLAG_RESIDENT, each on its own stream, stepped
one after the other, one sync of all at the end).  They alternate, one child process at a time,
`rounds` times; a child runs every board at every batch size B = 1, 256, 1024 and the largest B
whose workgroups are all co-resident, CUs x the occupancy gol_batch_occupancy reports (the
parent process asks the new library once and hands the numbers to both sides).  The reference
runs the sizes up to --ref-max-boards: every engine owns two streams, three events and five
allocations, and thousands of them in one process are not what this tool is about.

Both sides hold the same boards: board i, row y = row i x height + y of gol_fill_random(seed) on
a width x (B x height) board, computed here on the host (splitmix64) and loaded packed; the batch
side checks that gol_batch_fill_random gives the same words.  A sample: a warm-up of one 256-turn
launch, then `launches` x 256 turns.  The batch is timed between two HIP events on its stream and
by the host clock from the first call to the end of the sync; the reference by the host clock
alone (its engines run on B streams, which no event pair brackets).  The acceptance compares
the host-clock ranges of both sides, the same clock on both.  The boards of both sides hash alike
at the end.

The children bind the handful of calls they need by hand: the base library lacks the batch
symbols of gol/_native.py.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "conway-s-gol-distributed_amd"))

BOARDS = [(16, 16), (64, 64), (128, 128), (200, 77), (255, 1024)]
SIZES = (1, 256, 1024)
FLAG_RESIDENT = 0x8
DEPTH = 256
REF_NEEDED = ("gol_create", "gol_destroy", "gol_get_info", "gol_sync", "gol_load_packed",
              "gol_step", "gol_read_packed")
BATCH_NEEDED = ("gol_batch_create", "gol_batch_destroy", "gol_batch_occupancy",
                "gol_batch_get_stream", "gol_batch_sync", "gol_batch_load_packed",
                "gol_batch_fill_random", "gol_batch_step", "gol_batch_read_packed")


def hip_runtime():
    """The HIP runtime the engine library brought in (already loaded: no second copy)."""
    for name in ("libamdhip64.so.7", "libamdhip64.so.6", "libamdhip64.so"):
        try:
            return C.CDLL(name, mode=os.RTLD_NOW | os.RTLD_NOLOAD)
        except OSError:
            pass
    raise SystemExit("no loaded libamdhip64 found")


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


def splitmix64(x):
    z = x + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def start_boards(seed, w, h, boards):
    """gol_fill_random(seed) of a w x (boards x h) board, as (boards, h, nw) words."""
    nw = (w + 63) // 64
    with np.errstate(over="ignore"):
        idx = np.arange(boards * h * nw, dtype=np.uint64)
        words = splitmix64((np.uint64(seed) << np.uint64(40)) + idx).reshape(boards * h, nw)
    nb = w - 64 * (nw - 1)
    if nb < 64:
        words[:, nw - 1] &= np.uint64((1 << nb) - 1)
    return np.ascontiguousarray(words.reshape(boards, h, nw))


def sizes_for(cap, limit=None):
    out = [b for b in dict.fromkeys(SIZES + (cap,))]
    return [b for b in out if limit is None or b <= limit]


def probe(lib_path):
    """{board: [workgroups per CU, CUs]} from the new library."""
    L = bind(lib_path, BATCH_NEEDED)
    out = {}
    for (w, h) in BOARDS:
        b = C.c_void_p()
        ok(L.gol_batch_create(w, h, 1, -1, 0, C.byref(b)))
        per, cus = C.c_int32(), C.c_int32()
        ok(L.gol_batch_occupancy(b, C.byref(per), C.byref(cus)))
        L.gol_batch_destroy(b)
        out[f"{w}x{h}"] = [per.value, cus.value]
    print(json.dumps(out), flush=True)


def child_batch(lib_path, launches, caps):
    L = bind(lib_path, BATCH_NEEDED)
    hip = hip_runtime()
    for fn in (hip.hipEventCreate, hip.hipEventRecord, hip.hipEventSynchronize,
               hip.hipEventElapsedTime, hip.hipEventDestroy):
        fn.restype = C.c_int
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
    hip.hipEventDestroy.argtypes = [C.c_void_p]
    for (w, h) in BOARDS:
        per, cus = caps[f"{w}x{h}"]
        for B in sizes_for(per * cus):
            start = start_boards(1000 + w, w, h, B)
            got = np.zeros_like(start)
            b = C.c_void_p()
            ok(L.gol_batch_create(w, h, B, -1, 0, C.byref(b)))
            ok(L.gol_batch_fill_random(b, 1000 + w))
            ok(L.gol_batch_read_packed(b, 0, B, got.ctypes.data_as(C.POINTER(C.c_uint64))))
            if not np.array_equal(got, start):
                raise SystemExit(f"{w}x{h} B={B}: gol_batch_fill_random is not the host's board")
            stream = L.gol_batch_get_stream(b)
            ok(L.gol_batch_step(b, DEPTH))
            ok(L.gol_batch_sync(b))
            e0, e1 = C.c_void_p(), C.c_void_p()
            ok(hip.hipEventCreate(C.byref(e0)))
            ok(hip.hipEventCreate(C.byref(e1)))
            t0 = time.perf_counter()
            ok(hip.hipEventRecord(e0, stream))
            ok(L.gol_batch_step(b, DEPTH * launches))
            ok(hip.hipEventRecord(e1, stream))
            ok(L.gol_batch_sync(b))
            wall = time.perf_counter() - t0
            ms = C.c_float()
            ok(hip.hipEventElapsedTime(C.byref(ms), e0, e1))
            ok(L.gol_batch_read_packed(b, 0, B, got.ctypes.data_as(C.POINTER(C.c_uint64))))
            ok(hip.hipEventDestroy(e0))
            ok(hip.hipEventDestroy(e1))
            L.gol_batch_destroy(b)
            print(json.dumps(dict(w=w, h=h, B=B, config="batch", launches=launches,
                                  us_event=round(ms.value * 1e3 / launches, 3),
                                  us_wall=round(wall * 1e6 / launches, 3),
                                  sha=hashlib.sha256(got.tobytes()).hexdigest()[:16])), flush=True)


def child_ref(lib_path, launches, caps, limit):
    from gol import _native as N
    L = bind(lib_path, REF_NEEDED)
    u64p = C.POINTER(C.c_uint64)
    for (w, h) in BOARDS:
        per, cus = caps[f"{w}x{h}"]
        for B in sizes_for(per * cus, limit):
            start = start_boards(1000 + w, w, h, B)
            got = np.zeros_like(start)
            engines = []
            for i in range(B):
                ctx = C.c_void_p()
                ok(L.gol_create(w, h, FLAG_RESIDENT, C.byref(ctx)))
                ok(L.gol_load_packed(ctx, start[i].ctypes.data_as(u64p)))
                engines.append(ctx)
            info = N.gol_info()
            ok(L.gol_get_info(engines[0], C.byref(info)))
            if info.turns_per_launch != DEPTH:
                raise SystemExit(f"{w}x{h}: the base engine is not resident")
            for ctx in engines:
                ok(L.gol_step(ctx, DEPTH))
            for ctx in engines:
                ok(L.gol_sync(ctx))
            t0 = time.perf_counter()
            for ctx in engines:                          # one after the other ...
                ok(L.gol_step(ctx, DEPTH * launches))
            for ctx in engines:                          # ... one sync at the end
                ok(L.gol_sync(ctx))
            wall = time.perf_counter() - t0
            for i, ctx in enumerate(engines):
                ok(L.gol_read_packed(ctx, got[i].ctypes.data_as(u64p)))
                L.gol_destroy(ctx)
            print(json.dumps(dict(w=w, h=h, B=B, config="ref", launches=launches,
                                  us_event=None, us_wall=round(wall * 1e6 / launches, 3),
                                  sha=hashlib.sha256(got.tobytes()).hexdigest()[:16])), flush=True)


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
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--ref-max-boards", type=int, default=1024)
    ap.add_argument("--log")
    a = ap.parse_args()
    if a.child:
        kind, path = a.child[0], a.child[1]
        if kind == "probe":
            return probe(path)
        launches, caps = int(a.child[2]), json.loads(a.child[3])
        if kind == "batch":
            return child_batch(path, launches, caps)
        return child_ref(path, launches, caps, int(a.child[4]))
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
    emit("co-resident capacity (workgroups per CU x CUs, gol_batch_occupancy): " +
         ", ".join(f"{k}: {v[0]} x {v[1]} = {v[0] * v[1]}" for k, v in caps.items()))
    res = {}
    for rnd in range(a.rounds):
        for config, path in (("batch", new), ("ref", base)):
            extra = [str(a.ref_max_boards)] if config == "ref" else []
            for r in run_child(["--child", config, path, str(a.launches), json.dumps(caps)] + extra):
                r["round"] = rnd
                res.setdefault((r["w"], r["h"], r["B"]), {}).setdefault(config, []).append(r)
                emit(json.dumps(r))
    emit("")
    emit(f"us per launch of {DEPTH} turns ({a.launches} launches per sample, {a.rounds} rounds, "
         f"min .. max) and board-turns per second at the median")
    emit("board      B      batch events          batch host clock      ref host clock        "
         "batch bt/s   ref bt/s   ref / batch")
    failed = []
    for (w, h) in BOARDS:
        per, cus = caps[f"{w}x{h}"]
        for B in sizes_for(per * cus):
            by = res.get((w, h, B), {})
            shas = {r["sha"] for rs in by.values() for r in rs}
            if len(shas) != 1:
                raise SystemExit(f"{w}x{h} B={B}: the boards differ: {shas}")
            ev = sorted(r["us_event"] for r in by["batch"])
            bw = sorted(r["us_wall"] for r in by["batch"])
            med = lambda v: v[len(v) // 2]
            rate = lambda us: B * DEPTH / (us * 1e-6)
            line = (f"{w}x{h:<6} {B:<6d} {ev[0]:9.2f} .. {ev[-1]:9.2f}  {bw[0]:9.2f} .. {bw[-1]:9.2f}")
            if "ref" in by:
                rw = sorted(r["us_wall"] for r in by["ref"])
                line += (f"  {rw[0]:9.2f} .. {rw[-1]:9.2f}  {rate(med(bw)):10.3e}  {rate(med(rw)):10.3e}"
                         f"  {med(rw) / med(bw):8.1f}x")
                if B == 256 and not bw[-1] < rw[0]:
                    failed.append((w, h))
            else:
                line += f"  {'(not run)':>22}  {rate(med(bw)):10.3e}"
            emit(line)
    emit("")
    emit("acceptance (B = 256: the batch's min .. max range lies wholly below the reference's): " +
         ("every board passes" if not failed else f"FAILED on {failed}"))


if __name__ == "__main__":
    main()
