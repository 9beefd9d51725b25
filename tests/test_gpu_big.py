"""k_step_tile's big form (k_step_tile_big: the buffer resources rebased per tile, for board buffers
of 2 GiB and more), forced on small boards against the CPU oracle, and on a real board of more
than 2^32 bytes.

Forced (GOL_TILE_BIG=1 with GOL_MULTI_VARIANT=15 and GOL_TILE): the reference is oracle.bit_run
from oracle.gen_random, compared bit for bit; every case asserts its launches through
last_launches / last_launch_tiles, so none passes on one-turn launches.  The shapes are the
smallest at which the rebasing, the torus wrap of a tile's window and the store base can go wrong.

The real board (131072 x 262400: 16 KiB rows, 4 299 161 600 bytes per buffer) is dead except
four 64 x 64 soups laid across the rows at byte offsets 2^31 and 2^32, across the y wrap and
across the x wrap; each soup's future comes from the oracle on a small torus of its own.
"""
import ctypes

import numpy as np
import pytest

import strip_tiles as S
from gol import _native
from test_gpu_seam import TILE_H, _oracle_run
from test_gpu_strip_tiles import _Strips, _run_split, delay_buffers, torch  # noqa: F401

pytestmark = pytest.mark.gpu

K = 16


@pytest.fixture(scope="module")
def gol():
    import gol as g
    return g


def _big_codes():
    n = _native.lib().gol_tile_big_codes(None, 0)
    buf = (ctypes.c_int32 * n)()
    assert _native.lib().gol_tile_big_codes(buf, n) == n
    return tuple(buf)


BIG_CODES = _big_codes()
assert all(TILE_H[c % 100] + 2 * 8 <= 77 for c in BIG_CODES)


def _force_big(monkeypatch, tw, code):
    monkeypatch.setenv("GOL_TILE_BIG", "1")
    monkeypatch.setenv("GOL_MULTI_VARIANT", "15")
    monkeypatch.setenv("GOL_TILE", f"{tw},{code}")


# ------------------------------------------------------------------ forced small shapes
# width, tile width: 5 words as columns of 3 + 2; 5 words as one column with both x-halo columns
# in the same tile; 16 words as 13 + a repacked narrow column of 3; 33 words: interior columns
BIG_SHAPES = [(320, 3), (320, 5), (1024, 13), (2112, 13)]


@pytest.mark.parametrize("h", [77, 200])
@pytest.mark.parametrize("code", BIG_CODES)
@pytest.mark.parametrize("w,tw", BIG_SHAPES)
def test_big_code_forced(gol, oracle, monkeypatch, w, tw, code, h):
    """Every big code on every shape: step(8) then step(15) (8 + 7), on 200 rows and on 77, where
    the first and last tile rows' windows wrap the torus once and the last tile row is short."""
    k, th = 8, TILE_H[code % 100]
    _force_big(monkeypatch, tw, code)
    start, (want_mid, want) = _oracle_run(oracle, w + h, w, h, (k, 2 * k - 1))
    with gol.Engine(w, h, device=0, band_rows=th, turns_per_launch=k) as e:
        assert e.info().turns_per_launch == k and e.info().blocking_limited == 0
        e.load_packed(start)
        e.step(k)
        assert [(a, v) for a, v, _ in e.last_launches()] == [(k, 15)]
        assert {(a, b) for a, b, _ in e.last_launch_tiles()} == {(tw, code)}
        mid = e.read_packed()
        e.step(2 * k - 1)
        assert sorted(a for a, _, _ in e.last_launches()) == [k - 1, k]
        assert {(a, b) for a, b, _ in e.last_launch_tiles()} == {(tw, code)}
        got = e.read_packed()
    assert np.array_equal(mid, want_mid)
    assert np.array_equal(got, want)


def test_big_deepest_launch(gol, oracle, monkeypatch):
    """One launch of 64 turns, then one of 63: 64 halo rows above and below 51-row tiles on 200
    rows, windows of 179 rows that wrap in the first, the third and the last tile row."""
    w, h, tw, code, th = 320, 200, 5, 16, 51
    _force_big(monkeypatch, tw, code)
    start, (want_mid, want) = _oracle_run(oracle, 64, w, h, (64, 63))
    with gol.Engine(w, h, device=0, band_rows=th, turns_per_launch=64) as e:
        e.load_packed(start)
        e.step(64)
        assert [(a, v) for a, v, _ in e.last_launches()] == [(64, 15)]
        mid = e.read_packed()
        e.step(63)
        assert [(a, v) for a, v, _ in e.last_launches()] == [(63, 15)]
        assert {(a, b) for a, b, _ in e.last_launch_tiles()} == {(tw, code)}
        got = e.read_packed()
    assert np.array_equal(mid, want_mid)
    assert np.array_equal(got, want)


def test_big_chunked_launches(gol, oracle, monkeypatch):
    """GOL_STEP_CHUNKS=2 on 1024 x 200 over two consecutive launches: each launch runs as two
    kernels cut by row_lo / row_hi, the second launch's chunks ordered after the first's."""
    w, h, tw, code, th = 1024, 200, 13, 516, 35
    _force_big(monkeypatch, tw, code)
    monkeypatch.setenv("GOL_STEP_CHUNKS", "2")
    start, (want,) = _oracle_run(oracle, 2024, w, h, (2 * K,))
    with gol.Engine(w, h, device=0, band_rows=th, turns_per_launch=K) as e:
        e.load_packed(start)
        e.step(2 * K)
        assert [(a, v) for a, v, _ in e.last_launches()] == [(K, 15), (K, 15)]
        assert {(a, b) for a, b, _ in e.last_launch_tiles()} == {(tw, code)}
        assert e.last_step_chunks() == 4
        got = e.read_packed()
    assert np.array_equal(got, want)


def test_big_on_strips(gol, oracle, monkeypatch):
    """Three strips of 53 / 52 / 52 rows of a 1024 x 157 board with 11-row halos at code 516: no
    y wrap, row_lo > 0, a computed range that shrinks per launch."""
    w, h, n, halo, tpl, tw, code, th = 1024, 157, 3, 11, 8, 13, 516, 20
    _force_big(monkeypatch, tw, code)
    turns = (11, 18)
    start, (want_mid, want) = _oracle_run(oracle, code + 157, w, h, turns)

    def check(e, m):
        plan = e.last_launches()
        assert [v for _, v, _ in plan] == [15] * len(plan), plan
        assert [k for k, _, _ in plan] == S.even_split(m, tpl), plan
        assert {(a, b) for a, b, _ in e.last_launch_tiles()} == {(tw, code)}

    with _Strips(gol, start, w, n, halo, band_rows=th, turns_per_launch=tpl) as s:
        s.step(turns[0], check)
        assert [k for k, _, _ in s.engs[0].last_launches()] == [6, 5]
        mid = s.read()
        s.step(turns[1], check)
        got = s.read()
    assert np.array_equal(mid, want_mid)
    assert np.array_equal(got, want)


def test_big_split_launch(gol, oracle, torch, monkeypatch, delay_buffers):  # noqa: F811
    """One gol_step_overlap window per call on two strips of a 1024 x 130 board: the split first
    launch (interior rows, then the rows next to the halos on 16-row tiles behind the delayed
    receives) and the whole launches after it all go through the big form."""
    monkeypatch.setenv("GOL_TILE_BIG", "1")
    monkeypatch.setattr(S, "split_tile_w", lambda c: 13)
    case = dict(S.SPLIT_FORMS["first_of_three"], mv=15, code=516, w=1024, n=2, band=16)
    got, start, _ = _run_split(gol, oracle, torch, monkeypatch, case, delay_buffers)
    assert np.array_equal(got, oracle.bit_run(start, case["w"], sum(case["windows"])))


@pytest.mark.parametrize("what", ["count_engine", "width_1000", "code_outside_the_set",
                                  "window_wraps_twice"])
def test_big_refusals(gol, monkeypatch, what):
    """Under GOL_TILE_BIG=1 an engine or shape the form does not run fails at create."""
    from conftest import TILE_CODES
    w, h, th, tw, kw = 1024, 77, 19, 13, {}
    code = 108
    if what == "count_engine":
        kw = dict(count_every_turn=True)
    elif what == "width_1000":
        w = 1000
    elif what == "code_outside_the_set":
        code = next(c for c in TILE_CODES if c < 1000 and c % 100 == 8 and c not in BIG_CODES)
    else:
        code, th = 524, 60                               # 60 + 2 x 16 rows on a buffer of 77
    _force_big(monkeypatch, tw, code)
    with pytest.raises(_native.GolError):
        gol.Engine(w, h, device=0, band_rows=th, turns_per_launch=K, **kw).close()
    if what == "window_wraps_twice":                     # (45 + 32 = 77 rows: it just fits)
        gol.Engine(w, h, device=0, band_rows=45, turns_per_launch=K).close()


# ------------------------------------------------------------------ the real thing
W, H = 131072, 262400
assert W // 8 * H == 4_299_161_600 > 1 << 32
SOUP, PAD, TORUS = 64, 96, 256                          # PAD dead cells round a soup > 59 turns
# (x, y) of each soup's first cell: across row 131072 (byte offset 2^31), across row 262144
# (2^32), across the y wrap (rows 262380 .. 262399, 0 .. 43), across the x wrap (columns
# 131040 .. 131071, 0 .. 31); more than 200 cells apart in x and in y
SOUPS = [(20007, 131072 - 32), (50013, 262144 - 32), (80001, 262380), (131040, 60000)]
TURNS = (20, 39)


def _cells(packed, width):
    """(xs, ys) of the alive cells of a packed board (standard layout: bit b of word v is cell
    64 v + b)."""
    bits = np.unpackbits(packed.view(np.uint8), axis=1, bitorder="little")[:, :width]
    ys, xs = np.nonzero(bits)
    return xs.astype(np.int64), ys.astype(np.int64)


@pytest.fixture(scope="module")
def board(oracle):
    """The start board (one shared host array, read-only) and the expected row-major alive lists
    after TURNS[0] and after TURNS[0] + TURNS[1] turns."""
    start = np.zeros((H, W // 64), np.uint64)
    want = [[], []]
    for i, (x0, y0) in enumerate(SOUPS):
        soup = oracle.gen_random(100 + i, SOUP, SOUP)
        xs, ys = _cells(soup, SOUP)
        gx, gy = (x0 + xs) % W, (y0 + ys) % H
        np.bitwise_or.at(start, (gy, gx // 64), np.uint64(1) << (gx % 64).astype(np.uint64))
        small = np.zeros((TORUS, TORUS // 64), np.uint64)
        np.bitwise_or.at(small, (PAD + ys, (PAD + xs) // 64),
                         np.uint64(1) << ((PAD + xs) % 64).astype(np.uint64))
        cur = small
        for j, t in enumerate(TURNS):
            cur = oracle.bit_run(cur, TORUS, t)
            sx, sy = _cells(cur, TORUS)
            assert len(sx) > 0                            # (an empty answer cannot pass)
            # (the soup cannot have reached the small torus's edge: PAD > the turns run)
            assert sx.min() > 0 and sx.max() < TORUS - 1 and sy.min() > 0 and sy.max() < TORUS - 1
            want[j].append(np.stack([(x0 - PAD + sx) % W, (y0 - PAD + sy) % H], axis=1))
    out = []
    for lists in want:
        xy = np.concatenate(lists)
        out.append(xy[np.lexsort((xy[:, 0], xy[:, 1]))])
    start.setflags(write=False)
    return start, out


def _run_real(gol, board, tpl, check_plan):
    start, want = board
    with gol.Engine(W, H, device=0, band_rows=472 if tpl > 1 else 0, turns_per_launch=tpl,
                    autotune=False) as e:
        info = e.info()
        assert info.blocking_limited == 0 and info.turns_per_launch == tpl
        e.load_packed(start)
        done = 0
        for j, t in enumerate(TURNS):
            e.step(t)
            done += t
            check_plan(e, j)
            assert np.array_equal(e.alive_cells(), want[j]), (tpl, done)
            assert e.snapshot() == (done, len(want[j]))


def test_real_board_blocked(gol, board, monkeypatch):
    """The pinned 65536^2 shape (30 lanes x 472 rows, code 516) at 20 turns per launch: step(20)
    is one launch of 20, step(39) a 20 and a 19, all on k_step_tile."""
    monkeypatch.setenv("GOL_TILE", "30,516")

    def check_plan(e, j):
        plan = [(k, v) for k, v, _ in e.last_launches()]
        assert plan == ([(20, 15)] if j == 0 else [(20, 15), (19, 15)]), plan
        assert {(a, b) for a, b, _ in e.last_launch_tiles()} == {(30, 516)}

    _run_real(gol, board, 20, check_plan)


def test_real_board_one_turn_control(gol, board):
    """The same board and turns at turns_per_launch = 1: the one-turn path at this size, against
    the same lists."""
    def check_plan(e, j):
        assert [k for k, _, _ in e.last_launches()] == [1] * TURNS[j]

    _run_real(gol, board, 1, check_plan)


def test_unpinned_engine_blocks(gol):
    """gol.Engine(131072, 131072) with no overrides (a buffer of exactly 2 GiB) plans multi-turn
    launches at a big code, and after fill_random(1) and step(40) has the alive count of a
    turns_per_launch = 1 engine on the same seed.  (A count comparison, not a bit-exact one: two
    boards of 2 GiB are not read back and compared on the host here; the bit-exact checks are
    the ones above.)"""
    with gol.Engine(131072, 131072, device=0) as e:
        info = e.info()
        assert info.blocking_limited == 0 and info.turns_per_launch > 1
        e.fill_random(1)
        e.step(40)
        plan, tiles = e.last_launches(), e.last_launch_tiles()
        print(f"131072^2: turns_per_launch {info.turns_per_launch} band {info.band_rows} "
              f"plan {plan} tiles {tiles}")
        assert sum(k for k, _, _ in plan) == 40 and min(k for k, _, _ in plan) > 1
        assert all(v == 15 and code in BIG_CODES for (_, v, _), (_, code, _) in zip(plan, tiles))
        got = e.snapshot()
    with gol.Engine(131072, 131072, device=0, turns_per_launch=1) as e:
        assert e.info().blocking_limited == 0
        e.fill_random(1)
        e.step(40)
        assert [k for k, _, _ in e.last_launches()] == [1] * 40
        assert e.snapshot() == got and got[1] > 0
    with gol.Engine(131072, 131072, device=0, count_every_turn=True) as e:
        assert e.info().blocking_limited == 1 and e.info().turns_per_launch == 1
