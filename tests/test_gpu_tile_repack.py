"""k_step_tile with the ragged last tile column repacked into narrow tiles (golk::tile_grid),
and the two load and two store paths of a wave, against the CPU oracle at small shapes.

One code per turn order and word count.  Every case asserts through gol_tile_grid that its
launches have narrow tiles, so none passes by never taking the path; the reference is
oracle.bit_run from oracle.gen_random, compared bit for bit.  Boards:
  * 42 lanes at tile width 13: r = 3 lanes left, C' = 5, G' = 12 segments per wave;
  * 40 lanes: r = 1, C' = 3, G' = 21;
    (the multi-turn kernels need an even word count, so no board has 31 or 29 words)
  * 40 rows: shorter than one narrow tile with its halos, whose rows wrap the torus;
  * 203 rows: no multiple of any tile height used, main or narrow;
  * 4 lanes at tile width 14: no full-width column at all, the row narrower than the tile with its halo lanes.
The waves of these launches take both load paths (a segment that wraps past the buffer's last
row or none) and both store paths (a wave of whole segments, a wave at the tile's edge).
"""
import ctypes

import numpy as np
import pytest

import strip_tiles as S
from test_gpu_strip_tiles import _Strips, _run_split, delay_buffers, torch  # noqa: F401

pytestmark = pytest.mark.gpu

CODES = (8, 112, 203, 416, 516, 616, 1104)
TW, K = 13, 8
# tile heights by rows per segment: several tile rows on a 200-row board, more than one wave
# where the segment allows it; the short board's give two tile rows of 40
TILE_H = {3: 5, 4: 5, 8: 19, 12: 35, 16: 51}
TILE_H_SHORT = {3: 5, 4: 5, 8: 19, 12: 35, 16: 20}


@pytest.fixture(scope="module")
def gol():
    import gol as g
    return g


def _grid(nw, rows, k, th, tw, code):
    from gol import _native as N
    buf = (ctypes.c_int32 * 5)()
    assert N.lib().gol_tile_grid(nw, rows, k, th, tw, code, buf) == 0
    return tuple(buf)


def _pin_tile(monkeypatch, tw, code):
    monkeypatch.setenv("GOL_MULTI_VARIANT", "15")
    monkeypatch.setenv("GOL_TILE", f"{tw},{code}")


_RUNS = {}


def _oracle_run(oracle, seed, w, h, turns_list):
    """(start, boards after each cumulative turn count) of gen_random(seed), computed once per
    key and shared; callers do not modify them."""
    key = (seed, w, h, tuple(turns_list))
    if key not in _RUNS:
        start = oracle.gen_random(seed, w, h)
        boards, cur = [], start
        for t in turns_list:
            cur = oracle.bit_run(cur, w, t)
            boards.append(cur)
        for a in [start] + boards:
            a.setflags(write=False)
        _RUNS[key] = (start, boards)
    return _RUNS[key]


def _run_torus(gol, oracle, monkeypatch, lanes, h, th, code, narrow=True, tw=TW):
    """One launch of 8 turns, then launches of 8 and 7; the board after each call."""
    w = lanes * 64 * S.seg_words(code)
    nw = w // 64
    _pin_tile(monkeypatch, tw, code)
    grids = [_grid(nw, h, k, th, tw, code) for k in (K, K - 1)]
    assert all((g[2] > 0) == narrow for g in grids), grids
    start, (want_mid, want) = _oracle_run(oracle, code + lanes + h, w, h, (K, 2 * K - 1))
    with gol.Engine(w, h, device=0, band_rows=th, turns_per_launch=K) as e:
        e.load_packed(start)
        e.step(K)
        assert [(k, v) for k, v, _ in e.last_launches()] == [(K, 15)]
        mid = e.read_packed()
        e.step(2 * K - 1)
        assert sorted(k for k, _, _ in e.last_launches()) == [K - 1, K]
        assert {(a, b) for a, b, _ in e.last_launch_tiles()} == {(tw, code)}
        got = e.read_packed()
    assert np.array_equal(mid, want_mid)
    assert np.array_equal(got, want)
    return grids


@pytest.mark.parametrize("code", CODES)
@pytest.mark.parametrize("lanes", [42, 40])
def test_narrow_column(gol, oracle, monkeypatch, code, lanes):
    """r = 3 (C' = 5, G' = 12) and r = 1 (C' = 3, G' = 21) on 200 rows: three full-width columns
    and the narrow one, the narrow tiles taller than the main ones."""
    th = TILE_H[code % 100]
    grids = _run_torus(gol, oracle, monkeypatch, lanes, 200, th, code)
    assert all(g[0] == 3 and g[3] == lanes - 39 and g[4] > th for g in grids), grids


@pytest.mark.parametrize("code", CODES)
def test_short_board(gol, oracle, monkeypatch, code):
    """40 rows: the one narrow tile is the whole column, and its halo rows (and those of the
    main tiles) wrap the torus -- the load path that wraps row by row."""
    grids = _run_torus(gol, oracle, monkeypatch, 42, 40, TILE_H_SHORT[code % 100], code)
    assert all(g[2] == 1 and g[4] == 40 for g in grids), grids


@pytest.mark.parametrize("code,th", [(516, 40), (203, 5), (8, 19), (1104, 5)])
def test_ragged_height(gol, oracle, monkeypatch, code, th):
    """203 rows: the last main tile row and the last narrow tile are short (the store path of
    a wave whose segments the board's end cuts); 516 on 40-row tiles runs one-wave workgroups
    and two narrow tiles."""
    grids = _run_torus(gol, oracle, monkeypatch, 42, 203, th, code)
    assert all(203 % g[4] and 203 % th for g in grids), grids
    if code == 516:
        assert [g[2] for g in grids] == [2, 2]


@pytest.mark.parametrize("code", [108, 516])
def test_narrow_column_only(gol, oracle, monkeypatch, code):
    """4 lanes at tile width 14: no full-width column, every tile is narrow (C' = 6, the row
    narrower than the tile with its halo lanes: they wrap onto the tile itself)."""
    grids = _run_torus(gol, oracle, monkeypatch, 4, 300, 19, code, tw=14)
    assert all(g[0] == 0 and g[2] >= 2 and g[3] == 4 for g in grids), grids


def test_repack_switch(gol, oracle, monkeypatch):
    """GOL_TILE_REPACK=0: the rectangular grid, the same board."""
    monkeypatch.setenv("GOL_TILE_REPACK", "0")
    grids = _run_torus(gol, oracle, monkeypatch, 42, 200, TILE_H[16], 516, narrow=False)
    assert all(g == (4, 4, 0, 0, 0) for g in grids), grids


# ------------------------------------------------------------------ row strips
STRIP_H, STRIP_N, STRIP_HALO, STRIP_TPL = 157, 3, 11, 8
STRIP_WINDOWS = (11, 11, 7)       # 6 + 5 (the second launch starts 6 turns in), 6 + 5, 7
STRIP_TILE_H = {3: 5, 4: 5, 8: 19, 12: 20, 16: 20}


@pytest.mark.parametrize("code", CODES)
def test_narrow_column_on_strips(gol, oracle, monkeypatch, code):
    """Three strips of 53 / 52 / 52 rows with 11-row halos (row_lo > 0, no torus wrap, a
    computed range that shrinks per launch, a launch that starts mid-window); in some launch
    of every code row_hi cuts a tile row and a segment short."""
    lanes, th = 42, STRIP_TILE_H[code % 100]
    w = lanes * 64 * S.seg_words(code)
    nw = w // 64
    _pin_tile(monkeypatch, TW, code)
    cut = False
    for _, r in S.strip_split(STRIP_H, STRIP_N):
        for k, rows in S.launch_rows(r, STRIP_HALO, STRIP_TPL, STRIP_WINDOWS):
            g = _grid(nw, rows, k, th, TW, code)
            assert g[2] > 0, (k, rows, g)
            cut |= rows % th != 0 and rows % (code % 100) != 0
    assert cut
    turns = (STRIP_WINDOWS[0], sum(STRIP_WINDOWS[1:]))
    start, (want_mid, want) = _oracle_run(oracle, code + 157, w, STRIP_H, turns)

    def check(e, m):
        plan = e.last_launches()
        assert [v for _, v, _ in plan] == [15] * len(plan), plan
        assert [k for k, _, _ in plan] == S.even_split(m, STRIP_TPL), plan
        assert {(a, b) for a, b, _ in e.last_launch_tiles()} == {(TW, code)}

    with _Strips(gol, start, w, STRIP_N, STRIP_HALO, band_rows=th,
                 turns_per_launch=STRIP_TPL) as s:
        s.step(turns[0], check)
        assert [k for k, _, _ in s.engs[0].last_launches()] == [6, 5]
        mid = s.read()
        s.step(turns[1], check)
        got = s.read()
    assert np.array_equal(mid, want_mid)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("code", [516, 112])
def test_narrow_column_split_launch(gol, oracle, torch, monkeypatch, delay_buffers, code):  # noqa: F811
    """gol_step_overlap's split first launch (interior rows, then the rows next to the halos on
    16-row tiles behind the delayed receives) and the whole launches after it, two strips of a
    4224 x 130 board: 66 lanes = 2 x 30 + 6, the 6 as narrow tiles (C' = 8, G' = 8)."""
    case = dict(S.SPLIT_FORMS["first_of_three"], mv=15, code=code, w=4224, n=2, band=16)
    assert S.split_ok(case)
    rows, s0 = case["h"][2] // 2 + 2 * case["halo"], 0
    for k in S.even_split(case["windows"][0], case["tpl"]):
        s0 += k
        g = _grid(66, rows - 2 * s0, k, S.SPLIT_TILE_H, 30, code)
        assert g[0] == 2 and g[2] > 0 and g[3] == 6, g
    got, start, _ = _run_split(gol, oracle, torch, monkeypatch, case, delay_buffers)
    assert np.array_equal(got, oracle.bit_run(start, case["w"], sum(case["windows"])))


# ------------------------------------------------------------------ counted launches
@pytest.mark.parametrize("lanes,h,th", [(42, 200, 51), (42, 203, 40)])
def test_narrow_column_counted(gol, oracle, monkeypatch, lanes, h, th):
    """A GOL_FLAG_COUNT_EVERY_TURN engine at code 516 (k_step_tile_cnt): the per-turn counts of
    launches of 8, 8 and 7 turns with the narrow column present -- every board word is counted
    by exactly one tile, main or narrow."""
    w, code = lanes * 64, 516
    _pin_tile(monkeypatch, TW, code)
    assert all(_grid(lanes, h, k, th, TW, code)[2] > 0 for k in (K, K - 1))
    start = oracle.gen_random(516 + h, w, h)
    want, wc = oracle.bit_run(start, w, 3 * K - 1, counts=True)
    with gol.Engine(w, h, device=0, band_rows=th, turns_per_launch=K, count_every_turn=True) as e:
        e.load_packed(start)
        e.step(K)
        assert [(k, v) for k, v, _ in e.last_launches()] == [(K, 15)]
        e.step(2 * K - 1)
        assert sorted(k for k, _, _ in e.last_launches()) == [K - 1, K]
        got, counts = e.read_packed(), e.turn_counts(1, 3 * K - 1)
    assert counts.tolist() == wc.astype(np.int64).tolist()
    assert np.array_equal(got, want)
