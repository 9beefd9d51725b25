"""The parameter tables of test_gpu_strip_tiles.py, checked without a GPU: the Python mirror of
golk::tile_waves / tile_shape_ok (strip_tiles.py) against worked numbers, and every generated
case against the mirror."""
import pytest

import strip_tiles as S
from conftest import TILE_CODES

ALL_CODES = tuple(TILE_CODES) + S.TOOLS_CODES


def test_mirror_worked_numbers():
    # C = tw + 2, G = 64 // C, nseg = ceil((th + 2K) / SEG), waves = ceil(nseg / G)
    assert S.tile_waves(20, 472, 30, 516) == 16      # the 65536^2 pinned shape: 512 rows / 16 / 2
    assert S.tile_waves(30, 452, 30, 516) == 16
    assert S.tile_waves(51, 410, 14, 516) == 8       # 16384^2: 512 rows, G = 4
    assert S.tile_waves(40, 160, 10, 203) == 16      # 5120^2: 240 rows / 3 = 80 segments, G = 5
    assert S.tile_waves(8, 100, 14, 2) == 15         # 116 rows / 2 = 58 segments, G = 4
    assert S.tile_waves(8, 100, 7, 1002) == 9        # C = 9, G = 7
    assert S.tile_waves(6, 13, 62, 8) == 4           # G = 1: one segment per wave
    assert S.tile_shape_ok(66, 8, 100, 14, 2)
    assert not S.tile_shape_ok(66, 8, 113, 14, 2)    # 129 rows: 65 segments, 17 waves
    assert not S.tile_shape_ok(66, 1, 10, 14, 8)     # depth < 2
    assert not S.tile_shape_ok(66, 65, 10, 14, 8)    # depth > kMaxTileTurns
    assert not S.tile_shape_ok(66, 8, 10, 63, 8)     # tile wider than a wave
    assert not S.tile_shape_ok(65, 8, 10, 7, 1004)   # odd words, two words per lane
    assert S.tile_shape_ok(66, 8, 87, 30, 724)       # ORD 7: G = 2, >= 3 segments
    assert not S.tile_shape_ok(66, 8, 87, 14, 724)   # ORD 7 at G = 4
    assert not S.tile_shape_ok(66, 8, 20, 30, 724)   # ORD 7 with 2 segments


def test_even_split_and_launch_rows():
    assert S.even_split(11, 8) == [6, 5]
    assert S.even_split(7, 8) == [7]
    assert S.even_split(128, 6) == [6] * 18 + [5] * 4
    assert S.even_split(20, 8) == [7, 7, 6]
    assert S.strip_split(157, 3) == [(0, 53), (53, 52), (105, 52)]
    # 53 owned rows, halo 11: a 6-turn launch computes 75 - 12 rows, the 5-turn launch that
    # follows it (s0 = 6) the owned rows, a 7-turn window's launch 75 - 14
    assert S.launch_rows(53, 11, 8, (11, 7)) == {(6, 63), (5, 53), (7, 61)}
    assert S.code_launches() == {(6, 63), (5, 53), (7, 61), (6, 62), (5, 52), (7, 60)}


@pytest.mark.parametrize("code", ALL_CODES)
def test_code_table(code):
    """Part 1: 1 < waves <= 16 at every launch, a short last tile row at every launch, a
    partial last tile column, and a shape the engine accepts at create."""
    tw, th = S.code_tile_w(code), S.code_tile_h(code)
    nw = S.CODE_W // 64
    assert S.tile_shape_ok(nw, S.CODE_TPL, th, tw, code)
    assert 1 <= S.tile_waves(S.CODE_TPL, th, tw, code) <= S.MAX_WAVES
    assert (nw // S.seg_words(code)) % tw != 0 and nw // S.seg_words(code) > tw
    for k, rows in S.code_launches():
        assert 2 <= S.tile_waves(k, th, tw, code) <= S.MAX_WAVES, (k, th)
        assert rows % th != 0, (rows, th)


def test_code_table_heights():
    """The derived heights at a glance (a change of the rule shows here)."""
    got = {c: S.code_tile_h(c) for c in (2, 8, 16, 48, 516, 1002, 1208, 724)}
    assert got == {2: 8, 8: 23, 16: 23, 48: 87, 516: 23, 1002: 8, 1208: 47, 724: 39}


def test_edge_table():
    """Part 2: every shape keeps all nine code families but where tile_shape_ok refuses, every
    kept case passes the mirror at create and at each launch depth, and no call leaves a
    one-turn launch (the launch assertions expect kernel 15 only)."""
    cases = S.edge_cases()
    assert len(cases) >= 9 * len(S.EDGE_SHAPES) - 9
    for name in S.EDGE_SHAPES:
        assert {c // 100 for n, c in cases if n == name} >= {0, 1, 2, 4, 5, 6, 10, 11, 12} - \
            {c // 100 for c in S.EDGE_CODES if not S.edge_ok(S.EDGE_SHAPES[name], c)}
        assert any(n == name for n, _ in cases)
    for name, code in cases:
        s = S.EDGE_SHAPES[name]
        tw, nw = S.edge_tile_w(s, code), (s["w"] + 63) // 64
        assert sum(S.edge_windows(s)) == sum(s["steps"])
        assert min(r for _, r in S.strip_split(s["h"], s["n"])) >= s["halo"]
        for m in S.edge_windows(s):
            for k in S.even_split(m, s["tpl"]):
                assert k >= 2 and 1 <= S.tile_waves(k, s["th"], tw, code) <= S.MAX_WAVES
                assert S.tile_shape_ok(nw, k, s["th"], tw, code)
    assert S.edge_windows(S.EDGE_SHAPES["mid_window"]) == [5, 7, 12, 2]
    assert S.edge_windows(S.EDGE_SHAPES["deep_window"]) == [40, 13]


def test_split_table():
    """Part 3: the cases cover every kernel, the one-turn split, no interior rows, counts and a
    partial window; every k_step_tile case passes the mirror, also on the boundary launches'
    16-row tiles; every (width, strips) pair occurs."""
    cases = S.split_cases()
    assert len({i for i, _ in cases}) == len(cases)
    assert all(S.split_ok(c) for _, c in cases)
    assert {c["mv"] for _, c in cases} >= {7, 8, 9, 12, 13, 14, 15}
    assert {c["code"] for _, c in cases if c["mv"] == 15} == {516, 112, 512, 203, 624, 2, 1008}
    assert {(c["w"], c["n"]) for _, c in cases} >= {(w, n) for w in (1024, 4224) for n in (1, 2, 3)}
    assert any(c["tpl"] == 1 and c["w"] == 100 for _, c in cases)
    assert any(c.get("counts") for _, c in cases)
    for _, c in cases:
        rows = [r for _, r in S.strip_split(c["h"][c["n"]], c["n"])]
        assert min(rows) >= c["halo"] and all(1 <= m <= c["halo"] for m in c["windows"])
    # no interior: rows <= 2k at the first launch of a window
    thin = [c for i, c in cases if i.startswith(("no_interior", "one_turn_thin"))]
    for c in thin:
        k = S.even_split(c["windows"][0], c["tpl"])[0]
        assert max(r for _, r in S.strip_split(c["h"][c["n"]], c["n"])) <= 2 * k
    assert any(m < c["halo"] for i, c in cases if i.startswith("partial") for m in c["windows"][:-1])
