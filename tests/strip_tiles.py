"""Shapes for the strip and split-launch tests of k_step_tile (test_gpu_strip_tiles.py).

A pure-Python mirror of golk::tile_waves / golk::tile_shape_ok (csrc/gol_tile.hip) and the
parameter tables built with it, so that a table can be checked where there is no GPU
(test_strip_tiles_cpu.py) and no case is skipped at run time: a combination the engine would
refuse at create is never generated.
"""
from __future__ import annotations

MAX_WAVES = 16          # golk::kTileMaxWaves
MAX_TILE_TURNS = 64     # golk::kMaxTileTurns
OVERLAP_BAND = 16       # golk::kOverlapBand: tile height of a split launch's boundary launches


def seg_words(code: int) -> int:
    """Words per lane of a segment code (SEG + 100 * ORD + 1000 * (words - 1))."""
    return code // 1000 + 1


def tile_waves(K: int, th: int, tw: int, code: int) -> int:
    """Waves per workgroup of a K-turn launch on th-row tiles of tw lanes (golk::tile_waves)."""
    C = tw + 2
    G = 64 // C
    seg = code % 100
    nseg = -(-(th + 2 * K) // seg)
    return -(-nseg // G)


def tile_shape_ok(nw: int, K: int, th: int, tw: int, code: int) -> bool:
    """golk::tile_shape_ok but for the list of instantiated codes (the callers pass only
    codes the library under test has)."""
    if K < 2 or K > MAX_TILE_TURNS or th < 1 or tw < 1 or tw + 2 > 64:
        return False
    if nw % seg_words(code):
        return False
    G = 64 // (tw + 2)
    seg = code % 100
    nseg = -(-(th + 2 * K) // seg)
    if code // 100 % 10 == 7 and (G != 2 or nseg < 3):
        return False
    return 1 <= tile_waves(K, th, tw, code) <= MAX_WAVES


def even_split(room: int, tpl: int) -> list[int]:
    """The launch depths of `room` turns at `tpl` turns per launch (plan_launch's rule for an
    engine without a measured plan: ceil(room / tpl) launches of near-equal depth)."""
    out = []
    while room > 0:
        nl = -(-room // tpl)
        k = -(-room // nl)
        out.append(k)
        room -= k
    return out


def strip_split(height: int, n: int):
    base, slack = divmod(height, n)
    out, off = [], 0
    for i in range(n):
        r = base + (1 if i < slack else 0)
        out.append((off, r))
        off += r
    return out


def launch_rows(rows: int, halo: int, tpl: int, windows) -> set[tuple[int, int]]:
    """{(depth, computed rows)} of every launch of a strip of `rows` owned rows that runs
    `windows` (turns per halo window, each <= halo): a k-turn launch that starts s0 turns
    into its window computes buffer rows [s0 + k, rows + 2 halo - s0 - k)."""
    out = set()
    for m in windows:
        s0 = 0
        for k in even_split(m, tpl):
            out.add((k, rows + 2 * halo - 2 * (s0 + k)))
            s0 += k
    return out


# ------------------------------------------------- part 1: every code on ragged strips
CODE_W, CODE_H, CODE_N = 4224, 157, 3          # 66 words; strips of 53 / 52 / 52 rows
CODE_HALO, CODE_TPL = 11, 8                    # a full window: a 6-turn then a 5-turn launch
CODE_WINDOWS = (11, 11, 7)                     # 29 turns
TOOLS_CODES = (724, 824, 812, 806, 924, 912, 906)


def code_tile_w(code: int) -> int:
    """Tile width in lanes on the 66-word board, each with a partial last tile column (as
    test_gpu_engine._pinned_shape): 66 = 4 x 14 + 10 = 2 x 30 + 6; 33 lane pairs = 4 x 7 + 5."""
    if seg_words(code) == 2:
        return 7
    return 14 if code % 100 <= 8 else 30


def code_launches() -> set[tuple[int, int]]:
    out = set()
    for _, r in strip_split(CODE_H, CODE_N):
        out |= launch_rows(r, CODE_HALO, CODE_TPL, CODE_WINDOWS)
    return out


def code_tile_h(code: int) -> int:
    """The smallest tile height >= 7 at which no launch of the run computes a whole number of
    tile rows (a short last tile row every time), every launch's workgroup has more than one
    wave, and the engine accepts the shape at create (depth CODE_TPL).  Large segments need
    tiles taller than a strip for a second wave: then the one tile row is the short one."""
    tw = code_tile_w(code)
    nw = CODE_W // 64
    launches = code_launches()
    for th in range(7, 200):
        if any(rows % th == 0 for _, rows in launches):
            continue
        if not tile_shape_ok(nw, CODE_TPL, th, tw, code):
            continue
        if all(tile_shape_ok(nw, k, th, tw, code) and tile_waves(k, th, tw, code) > 1
               for k, _ in launches):
            return th
    raise AssertionError(f"no tile height for code {code}")


# ------------------------------------------------- part 2: strip edge shapes
EDGE_CODES = (8, 108, 208, 408, 516, 612, 1004, 1104, 1204)

# name -> width, height, strips, halo, turns per launch, tile height, gol_step calls (turns
# each; a call runs on across exchanges), and optionally the tile width in lanes for one /
# two words per lane (default: code_tile_w's 14 / 30 / 7)
EDGE_SHAPES = {
    # nothing but boundary: every owned row is somebody's halo
    "rows_eq_halo": dict(w=1024, h=36, n=3, halo=12, tpl=8, th=10, steps=(12, 17)),
    # the strip is its own upper and lower neighbour: a torus run through the halo path
    "one_strip": dict(w=1024, h=60, n=1, halo=9, tpl=8, th=13, steps=(9, 14)),
    # 100 rows over 7 strips: 15, 15, 14, 14, 14, 14, 14
    "ragged_split": dict(w=1024, h=100, n=7, halo=10, tpl=8, th=9, steps=(23,)),
    # halo deeper than the tile: 24 halo rows around 10-row tiles, launches of 12 turns
    "halo_gt_tile": dict(w=1024, h=90, n=2, halo=24, tpl=12, th=10, steps=(24, 19)),
    # one 40-turn launch per window (the planner's tables end at 32)
    "deep_window": dict(w=1024, h=100, n=2, halo=40, tpl=40, th=21, steps=(40, 13)),
    # kMaxTileTurns: one 64-turn launch on 70-row strips
    "halo_64": dict(w=1024, h=140, n=2, halo=64, tpl=64, th=24, steps=(64, 9)),
    # one tile column (6 words): the halo words wrap onto the tile itself
    "one_column": dict(w=384, h=60, n=2, halo=8, tpl=8, th=11, steps=(8, 13), tw=(6, 3)),
    # 130 words: one lane group per wave (G = 1), a short last tile column
    "wide_tile": dict(w=8320, h=60, n=2, halo=6, tpl=6, th=13, steps=(6, 10), tw=(62, 31)),
    # a call that ends mid-window; the next one finishes the window before it exchanges
    "mid_window": dict(w=1024, h=75, n=3, halo=12, tpl=8, th=9, steps=(5, 21)),
}


def edge_tile_w(shape: dict, code: int) -> int:
    if "tw" in shape:
        return shape["tw"][seg_words(code) - 1]
    return code_tile_w(code)


def edge_windows(shape: dict) -> list[int]:
    """Turns per halo window of a shape's calls (a window is halo turns, cut where a call ends)."""
    out, valid = [], 0
    for turns in shape["steps"]:
        while turns:
            if valid == 0:
                valid = shape["halo"]
            m = min(turns, valid)
            out.append(m)
            turns -= m
            valid -= m
    return out


def edge_ok(shape: dict, code: int) -> bool:
    """Whether the engine accepts the shape for this code, at create and at every launch."""
    nw = (shape["w"] + 63) // 64
    tw = edge_tile_w(shape, code)
    depths = {k for m in edge_windows(shape) for k in even_split(m, shape["tpl"])}
    return all(tile_shape_ok(nw, k, shape["th"], tw, code) for k in depths | {shape["tpl"]})


def edge_cases() -> list[tuple[str, int]]:
    return [(name, code) for name, s in EDGE_SHAPES.items() for code in EDGE_CODES
            if edge_ok(s, code)]


# ------------------------------------------------- part 3: the split launch
# (kernel id, k_step_tile code or 0)
SPLIT_KERNELS = ((7, 0), (8, 0), (9, 0), (13, 0), (12, 0), (14, 0),
                 (15, 516), (15, 112), (15, 512), (15, 203), (15, 624), (15, 2), (15, 1008))
SPLIT_TILE_H = 40       # k_step_tile's tile height (boundary launches: OVERLAP_BAND)

# window forms: halo, turns per launch, board height by number of strips, turns of each
# overlapped window (every window starts with an exchange, also a partial one)
SPLIT_FORMS = {
    # only the first of three launches (7 + 7 + 6) is split
    "first_of_three": dict(halo=20, tpl=8, h={1: 96, 2: 130, 3: 200}, windows=(20, 20)),
    # the bench's halo on 150-row strips
    "bench_halo": dict(halo=128, tpl=32, h={1: 150, 2: 300, 3: 450}, windows=(128, 40)),
    # rows <= 2k: no interior, the whole launch goes to the side stream
    "no_interior": dict(halo=8, tpl=8, h={1: 12, 2: 24, 3: 36}, windows=(8, 8, 5)),
    # a partial window, then another overlapped window
    "partial": dict(halo=20, tpl=8, h={1: 100, 2: 131, 3: 203}, windows=(9, 20, 5, 20)),
}
# kMultiWgPg / kMultiWgPgS run parallelogram bands only alone on their device (one strip) at
# depths and bands golk::pg_ok accepts: 8-turn launches on bands of 37 (mv 12) / 48 (mv 14)
# rows.  The split first launch must run them as helix; the second launch runs them whole.
SPLIT_PG = dict(halo=16, tpl=8, h={1: 150}, windows=(16, 16, 8), band={12: 37, 14: 48})
# one-turn launches (also on the generic path, width 100) and per-turn counts (no split: the
# launch waits whole)
SPLIT_ONE_TURN = dict(halo=3, tpl=1, h={1: 96, 2: 101, 3: 130}, windows=(3, 3, 2))
SPLIT_ONE_TURN_THIN = dict(halo=2, tpl=1, h={1: 2, 2: 4, 3: 6}, windows=(2, 2, 1))   # no interior
SPLIT_COUNTS = dict(halo=6, tpl=8, h={1: 96, 2: 101, 3: 130}, windows=(6, 6, 4))
# a one-turn window on an engine of multi-turn launches: the board is in the multi-turn
# kernels' interleaved layout when the receives are queued, and the one-turn launch converts
# it back first -- rows the receives have yet to write
SPLIT_ONE_TURN_WINDOW = dict(halo=20, tpl=8, h={1: 96, 2: 130, 3: 200}, windows=(20, 1, 20))


def split_tile_w(code: int) -> int:
    return code_tile_w(code)


def split_cases():
    """[(id, dict)] of the split-launch cases: every kernel in every window form, the widths
    and strip counts rotated so that each (width, strips) pair meets each form and kernel
    family."""
    out = []
    widths, strips = (1024, 4224), (1, 2, 3)
    for fi, (fname, form) in enumerate(SPLIT_FORMS.items()):
        for ki, (mv, code) in enumerate(SPLIT_KERNELS):
            w = widths[(ki + fi) % 2]
            n = strips[(ki // 2 + fi) % 3]
            out.append((f"{fname}-mv{mv}" + (f"-c{code}" if code else "") + f"-w{w}-n{n}",
                        dict(form, mv=mv, code=code, w=w, n=n, band=16)))
    for mv in (12, 14):
        out.append((f"pg-mv{mv}-w1024-n1",
                    dict(SPLIT_PG, mv=mv, code=0, w=1024, n=1, band=SPLIT_PG["band"][mv])))
    for w in (1024, 4224, 100):
        for n in strips:
            out.append((f"one_turn-w{w}-n{n}",
                        dict(SPLIT_ONE_TURN, mv=0, code=0, w=w, n=n, band=16)))
    for w, n in ((1024, 3), (100, 2), (4224, 1)):
        out.append((f"one_turn_thin-w{w}-n{n}",
                    dict(SPLIT_ONE_TURN_THIN, mv=0, code=0, w=w, n=n, band=16)))
    for (mv, code), w, n in (((7, 0), 4224, 1), ((9, 0), 1024, 3), ((15, 516), 4224, 2),
                             ((15, 1008), 1024, 1)):
        out.append((f"one_turn_window-mv{mv}" + (f"-c{code}" if code else "") + f"-w{w}-n{n}",
                    dict(SPLIT_ONE_TURN_WINDOW, mv=mv, code=code, w=w, n=n, band=16)))
    for (mv, code), w, n in (((7, 0), 1024, 2), ((15, 516), 4224, 3), ((0, 0), 100, 3),
                             ((9, 0), 4224, 1)):
        out.append((f"counts-mv{mv}-w{w}-n{n}",
                    dict(SPLIT_COUNTS, mv=mv, code=code, w=w, n=n, band=16, counts=True)))
    return out


def split_ok(case: dict) -> bool:
    """k_step_tile cases: the engine accepts the shape at create, at every launch depth, and
    on the OVERLAP_BAND-row tiles of the boundary launches."""
    if case["mv"] != 15 or case["tpl"] == 1:
        return True
    nw, tw, code = case["w"] // 64, split_tile_w(case["code"]), case["code"]
    depths = {k for m in case["windows"] for k in even_split(m, case["tpl"])} | {case["tpl"]}
    depths.discard(1)                       # (a one-turn launch is not k_step_tile's)
    return all(tile_shape_ok(nw, k, th, tw, code)
               for k in depths for th in (SPLIT_TILE_H, min(SPLIT_TILE_H, OVERLAP_BAND)))
