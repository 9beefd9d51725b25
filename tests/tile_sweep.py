"""The case table of the tile-shape sweep (test_gpu_tile_sweep.py; checked without a GPU by
test_tile_sweep_cpu.py).

The create-time search of an unpinned engine (tile_search, csrc/gol_tune.cpp) only times its
candidates: any shipped segment code, a tile width of 1..62 lanes, a workgroup of 4, 6, 8, 12 or
16 waves, a depth K of 8, 12, 16, 20, 24 or 32 turns, and the tile height that exactly fills the
workgroup, th = wv G SEG - 2 K with G = 64 // (tw + 2) lane groups per wave.  This table samples
that space so that every code meets every lane-grouping class on an exactly full tile:

part 1  every code of the library's lists (gol_tile_codes for plain launches,
        gol_tile_count_codes for counted ones, gol_tile_seam_codes across the row seam) at the
        tile widths SWEEP_WIDTHS -- G = 21, 16, 8, 3, 2, 1, 1 with 1, 0, 0, 1, 20, 31, 0 idle
        lanes -- in two shapes each: case A, K = 8 in the smallest workgroup that holds a tile of
        MIN_TILE_H rows (the search's floor), and case B, 16 waves at the deepest K that leaves
        such a tile (waves that hold nothing but halo rows and leave the trapezoid early);
part 2  one code per family (strip_tiles.EDGE_CODES) at every tile width 1..62, case A.

A case's board is the smallest with two tile columns and two tile rows, ragged both ways; its
seed is a function of (code, tw, K).  Nothing here is skipped at run time: a shape the library
would refuse is not generated, and test_tile_sweep_cpu.py checks every case against the library.
"""
from __future__ import annotations

import ctypes
from collections import namedtuple

import strip_tiles as S

SWEEP_WIDTHS = (1, 2, 6, 19, 20, 31, 62)
SEARCH_WAVES = (4, 6, 8, 12, 16)          # tile_search's workgroups
SEARCH_DEPTHS = (8, 12, 16, 20, 24, 32)   # and its depths
MIN_TILE_H = 8
KINDS = ("plain", "count", "seam")

# kind: plain / count / seam; part: 1 or 2; case: "A" or "B"; tw in lanes; wv waves; K turns;
# th tile rows; nw words per row; w, h the board; r the lanes of the ragged last tile column
Case = namedtuple("Case", "kind part case code tw wv K th nw w h r seed")


def _code_list(fn_name: str) -> tuple[int, ...]:
    from gol import _native as N
    fn = getattr(N.lib(), fn_name)
    n = fn(None, 0)
    buf = (ctypes.c_int32 * n)()
    assert fn(buf, n) == n
    return tuple(buf)


def library_codes() -> dict[str, tuple[int, ...]]:
    """The library's own code lists by kind (no device needed)."""
    return {"plain": _code_list("gol_tile_codes"),
            "count": _code_list("gol_tile_count_codes"),
            "seam": _code_list("gol_tile_seam_codes")}


def lane_groups(tw: int) -> int:
    return 64 // (tw + 2)


def full_tile_h(code: int, tw: int, wv: int, K: int) -> int:
    """The tile height that exactly fills wv waves at depth K."""
    return wv * lane_groups(tw) * (code % 100) - 2 * K


def case_a(code: int, tw: int):
    """(wv, K, th): K = 8 in the smallest searched workgroup with th >= MIN_TILE_H, or None."""
    for wv in SEARCH_WAVES:
        th = full_tile_h(code, tw, wv, 8)
        if th >= MIN_TILE_H:
            return wv, 8, th
    return None


def case_b(code: int, tw: int):
    """(wv, K, th): 16 waves at the deepest searched K > 8 with th >= MIN_TILE_H, or None."""
    for K in sorted(SEARCH_DEPTHS, reverse=True):
        if K == 8:
            break
        th = full_tile_h(code, tw, S.MAX_WAVES, K)
        if th >= MIN_TILE_H:
            return S.MAX_WAVES, K, th
    return None


def ragged_lanes(tw: int, words: int, min_words: int, large: bool) -> int:
    """r, the lanes of the last tile column of a row of 2 tw + r lanes: 1 <= r < tw where a
    tile is wide enough for that, the row an even number of words (two-word lanes, counted
    engines) and at least min_words; the smallest such r, or the largest."""
    ok = [r for r in range(1, max(tw, 64))
          if (2 * tw + r) * words % 2 == 0 and (2 * tw + r) * words >= min_words]
    if tw >= 3:
        ok = [r for r in ok if r < tw]
        return ok[-1] if large else ok[0]
    return ok[0]


def make_case(kind: str, part: int, case: str, code: int, tw: int, shape, i: int) -> Case:
    """The board of a case; i (the case's index in its kind) alternates the ragged column
    between narrow and nearly whole, and a seam board's last word between 1 and 40 cells (at
    rates of their own, so that cases A and B of a code each meet both)."""
    wv, K, th = shape
    words = S.seg_words(code)
    # (across the seam the engine blocks widths of at least 256 cells: five words)
    r = ragged_lanes(tw, words, 5 if kind == "seam" else 4, large=bool((i + i // 2) % 2))
    nw = (2 * tw + r) * words
    w = 64 * nw if kind != "seam" else 64 * (nw - 1) + (1, 40)[i // 3 % 2]
    h = th + max(1, th // 3)
    return Case(kind, part, case, code, tw, wv, K, th, nw, w, h, r,
                seed=code * 10000 + tw * 100 + K)


def build_cases(codes: dict[str, tuple[int, ...]] | None = None) -> list[Case]:
    codes = codes or library_codes()
    out, seen = [], set()
    count = dict.fromkeys(KINDS, 0)

    def add(kind, part, case, code, tw, shape):
        key = (kind, code, tw, shape)
        if shape is None or key in seen:
            return
        seen.add(key)
        out.append(make_case(kind, part, case, code, tw, shape, count[kind]))
        count[kind] += 1

    for kind in KINDS:
        for code in codes[kind]:
            for tw in SWEEP_WIDTHS:
                add(kind, 1, "A", code, tw, case_a(code, tw))
                add(kind, 1, "B", code, tw, case_b(code, tw))
    for code in S.EDGE_CODES:
        if code not in codes["plain"]:
            continue
        for tw in range(1, 63):
            add("plain", 2, "A", code, tw, case_a(code, tw))
    return out


def case_id(c: Case) -> str:
    return f"c{c.code}-tw{c.tw}-wv{c.wv}-K{c.K}"


def cases_of(kind: str, cases: list[Case] | None = None) -> list[Case]:
    return [c for c in (cases if cases is not None else CASES) if c.kind == kind]


def leaving(c: Case) -> bool:
    """The top wave holds halo rows only (G SEG <= K): it leaves the trapezoid before the
    launch's last turn, and so does the bottom one."""
    return lane_groups(c.tw) * (c.code % 100) <= c.K


CASES = build_cases()
