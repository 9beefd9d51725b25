"""k_step_tile_duo (csrc/gol_tile.h, tile_pass DUO: code 516 with the interior rows of a segment
ruled in pairs on shared row-pair sums) against the oracle and against the plain kernel.

Code 516 is pinned through GOL_MULTI_VARIANT=15 / GOL_TILE and run twice on every board: with
GOL_TILE_DUO unset (plain launches take the pair form) and with GOL_TILE_DUO=0 (the plain kernel).
Both must equal oracle.bit_run bit for bit, hence each other.  The launch records are the same
for both forms (variant 15, code 516) and are asserted for every launch of two turns or more.

Shapes (K = 20 turns per launch, so 33 turns are a 17- and a 16-turn launch):
  groups   1024 x 203, tiles 16 words x 56 rows: three lane groups per wave, two waves -- a
           segment's edge sums go to another lane group of its wave or to the other wave
  waves    2048 x 270, tiles 32 words x 135 rows: one segment per wave, 11 waves; wave 0 and
           the last waves leave the trapezoid from turn 17 on
  wrap     1024 x 50, one tile of 50 rows: it wraps past the buffer's first and last row, the
           wrap falling inside a segment
  repack   1152 x 130, tiles 14 words wide: the last tile column is 4 words, repacked at 10
           groups per wave
  strip    two strip engines (60 rows each, 33 halo rows) of a 1024 x 120 torus
Turns 1, 2, 16, 17, 20 and 33 from the same start; boards of density 0.05, 0.37 and 0.9 and an
all-alive board.  The oracle runs once per (shape, board) and is shared by both forms.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CODE, K = 516, 20
TURNS = (1, 2, 16, 17, 20, 33)
SHAPES = {
    "groups": dict(w=1024, h=203, tw=16, th=56, waves=2),
    "waves": dict(w=2048, h=270, tw=32, th=135, waves=11),
    "wrap": dict(w=1024, h=50, tw=16, th=50, waves=2),
    "repack": dict(w=1152, h=130, tw=14, th=88, waves=2),
    "strip": dict(w=1024, h=120, tw=16, th=40, waves=0, n=2, halo=33),
}
BOARDS = ("d05", "d37", "d90", "full")


@pytest.fixture(scope="module")
def gol():
    import gol as g
    return g


def _start(oracle, board, w, h, seed):
    if board == "full":
        return np.full((h, w // 64), ~np.uint64(0), dtype=np.uint64)
    p = {"d05": 0.05, "d37": 0.37, "d90": 0.9}[board]
    cells = (np.random.RandomState(seed).random_sample((h, w)) < p).astype(np.uint8) * 255
    return oracle.pack(cells)[0]


@pytest.fixture(scope="module")
def refs(oracle):
    """(shape, board) -> (start, {turns: board}), computed on first use, then read-only."""
    cache = {}

    def get(shape, board):
        key = (shape, board)
        if key not in cache:
            s = SHAPES[shape]
            start = _start(oracle, board, s["w"], s["h"], 516 + len(cache))
            want, cur, done = {}, start, 0
            for t in TURNS:
                cur = oracle.bit_run(cur, s["w"], t - done)
                done = t
                cur.setflags(write=False)
                want[t] = cur
            start.setflags(write=False)
            cache[key] = (start, want)
        return cache[key]
    return get


def _check_launches(e, s, turns):
    plan = e.last_launches()
    assert sum(k for k, _, _ in plan) == turns, plan
    if turns < 2:
        return
    assert [v for _, v, _ in plan] == [15] * len(plan), plan
    assert max(k for k, _, _ in plan) <= K
    tiles = e.last_launch_tiles()
    assert [(a, b) for a, b, _ in tiles] == [(s["tw"], CODE)] * len(plan), tiles
    if s["waves"] and turns >= 16:                      # (shallow launches need fewer segments)
        assert {v for _, _, v in tiles} == {s["waves"]}, tiles


def _run_torus(gol, s, start):
    got = {}
    with gol.Engine(s["w"], s["h"], device=0, band_rows=s["th"], turns_per_launch=K) as e:
        assert e.info().turns_per_launch == K and e.info().band_rows == s["th"]
        for t in TURNS:
            e.load_packed(start)
            e.step(t)
            _check_launches(e, s, t)
            got[t] = e.read_packed()
    return got


def _run_strips(gol, s, start):
    n, halo, h = s["n"], s["halo"], s["h"]
    parts = gol.strip_split(h, n)
    engs, got = [], {}
    try:
        for o, r in parts:
            engs.append(gol.Engine(s["w"], h, device=0, row_offset=o, rows=r, halo=halo,
                                   band_rows=s["th"], turns_per_launch=K))
        for t in TURNS:
            for e, (o, r) in zip(engs, parts):
                e.load_packed(np.ascontiguousarray(start[np.arange(o - halo, o + r + halo) % h]))
            for e in engs:
                assert e.halo_valid >= t
                e.step(t)
                _check_launches(e, s, t)
            got[t] = np.concatenate([e.read_packed() for e in engs])
    finally:
        for e in engs:
            e.close()
    return got


@pytest.mark.parametrize("board", BOARDS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_duo_matches_oracle_and_plain(gol, refs, monkeypatch, shape, board):
    s = SHAPES[shape]
    start, want = refs(shape, board)
    monkeypatch.setenv("GOL_MULTI_VARIANT", "15")
    monkeypatch.setenv("GOL_TILE", f"{s['tw']},{CODE}")
    run = _run_strips if shape == "strip" else _run_torus
    monkeypatch.delenv("GOL_TILE_DUO", raising=False)
    duo = run(gol, s, start)
    monkeypatch.setenv("GOL_TILE_DUO", "0")
    plain = run(gol, s, start)
    for t in TURNS:
        assert np.array_equal(duo[t], want[t]), ("duo", t)
        assert np.array_equal(plain[t], want[t]), ("plain", t)
        assert np.array_equal(duo[t], plain[t]), t
