"""The tile grid of a k_step_tile launch (golk::tile_grid through gol_tile_grid; no device).

A ragged last tile column that packs more row segments into a wave at its own width is cut into
a few tall narrow tiles instead of one full-price tile per tile row.  These tests pin the
geometry of the pinned launch shapes, the cases that must not repack, and -- by brute force on
small boards -- that every board row and lane column belongs to exactly one tile's stored region.
"""
import ctypes

import pytest

import strip_tiles as S


@pytest.fixture(scope="module")
def L():
    from gol import _native as N
    return N.lib()


def _grid(L, nw, rows, K, th, tw, code):
    buf = (ctypes.c_int32 * 5)()
    assert L.gol_tile_grid(nw, rows, K, th, tw, code, buf) == 0, (nw, rows, K, th, tw, code)
    return tuple(buf)


def _narrow_rows_max(K, th, tw, narrow_w, code):
    """Rows a narrow tile can hold: the main tiles' waves x G' x SEG - 2 K."""
    return S.tile_waves(K, th, tw, code) * (64 // (narrow_w + 2)) * (code % 100) - 2 * K


def test_headline_pin(L):
    """65536^2 at K = 20 on 30 x 472 tiles, code 516: 1024 lanes = 34 x 30 + 4."""
    g = _grid(L, 1024, 65536, 20, 472, 30, 516)
    assert g[:4] == (34, 139, 27, 4)
    assert S.tile_waves(20, 472, 30, 516) == 16
    assert _narrow_rows_max(20, 472, 30, 4, 516) == 2520
    assert 27 * g[4] >= 65536 > 26 * g[4] and g[4] <= 2520
    assert 34 * 139 + 27 == 4753


def test_long_step_pin(L):
    """65536^2 at K = 30 on 30 x 452 tiles."""
    g = _grid(L, 1024, 65536, 30, 452, 30, 516)
    assert g[:4] == (34, 145, 27, 4)
    assert g[4] <= _narrow_rows_max(30, 452, 30, 4, 516) == 2500
    assert 34 * 145 + 27 == 4957


@pytest.mark.parametrize("nl,why", [(28, "r = 0: the last column is whole"),
                                    (27, "r = 13 of 14: G' = 64 / 15 = 4 = G"),
                                    (14, "one whole column")])
def test_no_repack(L, nl, why):
    g = _grid(L, nl, 200, 8, 19, 14, 8)
    assert g == (-(-nl // 14), -(-200 // 19), 0, 0, 0), why


def test_no_repack_without_fewer_workgroups(L):
    """31 lanes at 14: r = 3 packs 12 groups, but with a single tile row the narrow column
    would take as many workgroups as it saves."""
    assert _grid(L, 31, 40, 8, 40, 14, 516) == (3, 1, 0, 0, 0)
    assert _grid(L, 31, 200, 8, 51, 14, 516) == (2, 4, 1, 3, 200)


def test_switch_and_errors(L, monkeypatch):
    """GOL_TILE_REPACK=0 keeps the rectangular grid; a shape the library does not run and a
    null result are GOL_EINVAL."""
    from gol import _native as N
    assert _grid(L, 31, 200, 8, 19, 14, 8)[2] > 0
    monkeypatch.setenv("GOL_TILE_REPACK", "0")
    assert _grid(L, 31, 200, 8, 19, 14, 8) == (3, 11, 0, 0, 0)
    monkeypatch.setenv("GOL_TILE_REPACK", "1")
    assert _grid(L, 31, 200, 8, 19, 14, 8)[2] > 0
    buf = (ctypes.c_int32 * 5)()
    assert L.gol_tile_grid(31, 200, 8, 19, 14, 9, buf) == N.GOL_EINVAL      # no such code
    assert L.gol_tile_grid(31, 200, 8, 4000, 14, 8, buf) == N.GOL_EINVAL    # > 16 waves
    assert L.gol_tile_grid(31, 200, 8, 19, 14, 8, None) == N.GOL_EINVAL


# (lanes per row, rows, K, tile height, tile width, code)
COVER_SHAPES = [
    (31, 200, 8, 19, 14, 8), (31, 200, 7, 19, 14, 8), (29, 200, 8, 35, 14, 112),
    (31, 203, 8, 5, 14, 203), (31, 40, 8, 20, 14, 516), (31, 203, 8, 40, 14, 516),
    (31, 200, 8, 51, 14, 616), (31, 157, 6, 20, 14, 416), (31, 200, 8, 5, 14, 1104),
    (66, 157, 8, 100, 30, 516), (66, 157, 8, 100, 14, 8), (33, 157, 8, 100, 7, 1004),
    (27, 200, 8, 19, 14, 8), (28, 90, 8, 19, 14, 8), (4, 300, 8, 19, 14, 108),
    (1024, 1500, 20, 472, 30, 516),
]


@pytest.mark.parametrize("nl,rows,K,th,tw,code", COVER_SHAPES)
def test_every_cell_in_one_tile(L, nl, rows, K, th, tw, code):
    """The stored regions of the launch's tiles -- main tile (tx, ty): lanes [tx tw, (tx + 1)
    tw) below nl, rows [ty th, (ty + 1) th) below `rows`; narrow tile j: the last narrow_w
    lanes, rows [j narrow_h, (j + 1) narrow_h) -- cover the board exactly once, and a narrow
    tile fits the main tiles' workgroup."""
    nw = nl * S.seg_words(code)
    assert S.tile_shape_ok(nw, K, th, tw, code)
    ntx, nty, nn, nw_, nh = _grid(L, nw, rows, K, th, tw, code)
    seen = [[0] * nl for _ in range(rows)]
    for ty in range(nty):
        for tx in range(ntx):
            for y in range(ty * th, min(rows, (ty + 1) * th)):
                for x in range(tx * tw, min(nl, (tx + 1) * tw)):
                    seen[y][x] += 1
    if nn:
        assert 0 < nw_ < tw and ntx * tw + nw_ == nl
        assert 64 // (nw_ + 2) > 64 // (tw + 2) and nn < nty
        assert 1 <= nh <= min(rows, _narrow_rows_max(K, th, tw, nw_, code))
        assert (nn - 1) * nh < rows <= nn * nh
    for j in range(nn):
        for y in range(j * nh, min(rows, (j + 1) * nh)):
            for x in range(ntx * tw, ntx * tw + nw_):
                seen[y][x] += 1
    assert all(c == 1 for row in seen for c in row)
