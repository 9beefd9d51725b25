"""The tile-shape sweep's case table (tile_sweep.py) against the library, without a GPU: every
case is a shape the engine accepts, exactly fills its workgroup and has the wave count the GPU
test will assert; and the table as a whole covers what it is there for.  The totals below are
conditions on the table, not measurements of it.
"""
import ctypes
from collections import Counter

import pytest

import strip_tiles as S
import tile_sweep as T


@pytest.fixture(scope="module")
def N():
    from gol import _native
    return _native


def _grid(N, c, K, th=None):
    """(return code, grid) of gol_tile_grid on the case's board at depth K."""
    buf = (ctypes.c_int32 * 5)()
    rc = N.lib().gol_tile_grid(c.nw, c.h, K, c.th if th is None else th, c.tw, c.code, buf)
    return rc, tuple(buf)


def test_table_sizes():
    """Two cases for every code of every library list at every sweep width; every width for
    the edge codes the library has."""
    codes = T.library_codes()
    part1 = Counter((c.kind, c.code, c.tw, c.case) for c in T.CASES if c.part == 1)
    for kind in T.KINDS:
        assert codes[kind], kind
        for code in codes[kind]:
            for tw in T.SWEEP_WIDTHS:
                assert part1[(kind, code, tw, "A")] == 1, (kind, code, tw)
                assert part1[(kind, code, tw, "B")] == 1, (kind, code, tw)
    assert sum(part1.values()) == 14 * sum(len(codes[k]) for k in T.KINDS)
    edge = [code for code in S.EDGE_CODES if code in codes["plain"]]
    assert edge
    have = {(c.code, c.tw) for c in T.cases_of("plain") if c.case == "A"}
    assert all((code, tw) in have for code in edge for tw in range(1, 63))
    ids = [(c.kind, T.case_id(c)) for c in T.CASES]
    assert len(set(ids)) == len(ids)
    print({k: len(T.cases_of(k)) for k in T.KINDS}, "leaving:", sum(map(T.leaving, T.CASES)))


@pytest.mark.parametrize("kind", T.KINDS)
def test_every_case_is_a_full_legal_shape(N, kind):
    codes = T.library_codes()[kind]
    cases = T.cases_of(kind)
    assert cases
    for c in cases:
        assert c.code in codes, c
        G, seg = T.lane_groups(c.tw), c.code % 100
        assert 1 <= c.tw <= 62 and c.wv in T.SEARCH_WAVES and c.K in T.SEARCH_DEPTHS, c
        assert c.th >= T.MIN_TILE_H, c
        assert c.th + 2 * c.K == c.wv * G * seg, c                    # exactly full
        assert S.tile_waves(c.K, c.th, c.tw, c.code) == c.wv, c
        assert S.tile_shape_ok(c.nw, c.K, c.th, c.tw, c.code), c
        assert S.tile_shape_ok(c.nw, c.K - 1, c.th, c.tw, c.code), c
        assert _grid(N, c, c.K)[0] == 0, c
        assert _grid(N, c, c.K - 1)[0] == 0, c
        if c.case == "A":
            # the smallest searched workgroup: the next smaller one holds no MIN_TILE_H rows
            i = T.SEARCH_WAVES.index(c.wv)
            assert c.K == 8 and (i == 0 or T.full_tile_h(c.code, c.tw, T.SEARCH_WAVES[i - 1], 8)
                                 < T.MIN_TILE_H), c
        else:
            deeper = [K for K in T.SEARCH_DEPTHS if K > c.K]
            assert c.wv == S.MAX_WAVES and c.K > 8, c
            assert all(T.full_tile_h(c.code, c.tw, c.wv, K) < T.MIN_TILE_H for K in deeper), c
        if c.wv == S.MAX_WAVES:
            # one row more than 16 waves hold is refused, not silently left uncomputed
            assert not S.tile_shape_ok(c.nw, c.K, c.th + 1, c.tw, c.code), c
            assert _grid(N, c, c.K, c.th + 1)[0] == N.GOL_EINVAL, c


@pytest.mark.parametrize("kind", T.KINDS)
def test_every_board_is_ragged_and_legal(kind):
    """Two tile columns and a ragged third (the narrowest tiles: whole columns), one full tile
    row and a short one; an even word count of at least four; across the seam a last word of 1
    or 40 cells, a width of at least 256 and tiles no wider than the row."""
    seen_rb = set()
    for c in T.cases_of(kind):
        words = S.seg_words(c.code)
        assert c.nw == (2 * c.tw + c.r) * words and c.nw >= 4 and c.nw % 2 == 0, c
        assert (1 <= c.r < c.tw) if c.tw >= 3 else c.r >= 1, c
        assert c.th < c.h < 2 * c.th and c.h == c.th + max(1, c.th // 3), c
        assert c.seed == c.code * 10000 + c.tw * 100 + c.K, c
        if kind == "seam":
            assert c.w // 64 == c.nw - 1 and c.w % 64 in (1, 40), c
            assert c.w >= 256 and c.tw <= c.nw and words == 1, c
            seen_rb.add((c.case, c.w % 64))
        else:
            assert c.w == 64 * c.nw, c
            assert kind != "count" or (c.w % 128 == 0 and words == 1), c
    if kind == "seam":
        assert seen_rb == {(ab, rb) for ab in "AB" for rb in (1, 40)}


def test_leaving_waves_are_covered():
    """At least 400 cases whose outermost waves hold only halo rows (G SEG <= K) and leave the
    trapezoid early; among them every turn order of every kind that has one."""
    gone = [c for c in T.CASES if T.leaving(c)]
    assert len(gone) >= 400, len(gone)
    for kind in T.KINDS:
        orders = {c.code // 100 for c in T.cases_of(kind)}
        assert {c.code // 100 for c in gone if c.kind == kind} == orders, kind


def test_both_grids_per_code_family(N):
    """Every code family (turn order and words per lane) of every kind meets a repacked narrow
    last column (gol_tile_grid: n_narrow > 0) and a rectangular grid, at depth K."""
    packed, plain = set(), set()
    for c in T.CASES:
        rc, g = _grid(N, c, c.K)
        assert rc == 0
        (packed if g[2] > 0 else plain).add((c.kind, c.code // 100))
    families = {(c.kind, c.code // 100) for c in T.CASES}
    assert packed == families and plain == families
