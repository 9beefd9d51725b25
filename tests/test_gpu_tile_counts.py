"""Per-turn alive counts fused into k_step_tile (K1t): a GOL_FLAG_COUNT_EVERY_TURN engine whose
multi-turn kernel is k_step_tile at a gol_tile_count_codes code keeps its temporal blocking, and
every turn of every launch has its true count (the reference's AliveCellsCount series,
Local/count_test.go).  Expected boards and series come from the CPU oracle
(oracle.bit_run(..., counts=True)), never from the engine.
"""
import ctypes
import threading
import time

import numpy as np
import pytest

import strip_tiles as S

pytestmark = pytest.mark.gpu


def _count_codes():
    """golk::kTileCountCodes through gol_tile_count_codes (needs no device)."""
    from gol import _native as N
    L = N.lib()
    n = L.gol_tile_count_codes(None, 0)
    buf = (ctypes.c_int32 * n)()
    assert L.gol_tile_count_codes(buf, n) == n
    return tuple(buf)


COUNT_CODES = _count_codes()


@pytest.fixture(scope="module")
def gol():
    import gol as g
    return g


_SERIES = {}


def _oracle_series(oracle, seed, w, h, turns):
    """(start, board after `turns`, counts of turns 1..turns) of gen_random(seed), computed once
    per (seed, shape, turns) and shared; callers do not modify it."""
    key = (seed, w, h, turns)
    if key not in _SERIES:
        start = oracle.gen_random(seed, w, h)
        board, counts = oracle.bit_run(start, w, turns, counts=True)
        for a in (start, board, counts):
            a.setflags(write=False)
        _SERIES[key] = (start, board, counts.astype(np.int64))
    return _SERIES[key]


def _pin_tile(monkeypatch, tw, code):
    monkeypatch.setenv("GOL_MULTI_VARIANT", "15")
    monkeypatch.setenv("GOL_TILE", f"{tw},{code}")


# ------------------------------------------------------------------ 1. default engine
def test_count_engine_keeps_temporal_blocking(gol, oracle, monkeypatch):
    """A plain 512 x 512 count engine: step(100) fuses turns into k_step_tile launches (kernel
    15) and the 100 counts and the board are the oracle's; GOL_COUNT_BLOCKING=0 restores one
    turn per launch with the same series."""
    w = h = 512
    start, want, wc = _oracle_series(oracle, 5, w, h, 100)
    with gol.Engine(w, h, device=0, count_every_turn=True) as e:
        e.fill_random(5)
        e.step(100)
        launches = e.last_launches()
        got, counts = e.read_packed(), e.turn_counts(1, 100)
    assert sum(k for k, _, _ in launches) == 100
    fused = [(k, kern) for k, kern, _ in launches if k > 1]
    assert fused, launches
    assert all(kern == 15 for _, kern in fused), launches
    assert counts.tolist() == wc.tolist()
    assert np.array_equal(got, want)
    monkeypatch.setenv("GOL_COUNT_BLOCKING", "0")
    with gol.Engine(w, h, device=0, count_every_turn=True) as e:
        e.fill_random(5)
        e.step(100)
        launches = e.last_launches()
        got, counts = e.read_packed(), e.turn_counts(1, 100)
    assert [k for k, _, _ in launches] == [1] * 100
    assert counts.tolist() == wc.tolist()
    assert np.array_equal(got, want)


# ------------------------------------------------------------------ 2. every counted code
@pytest.mark.parametrize("code", COUNT_CODES)
def test_count_code_pinned(gol, oracle, monkeypatch, code):
    """Every k_step_tile_cnt instantiation on test_tile_code_pinned's ragged shape (4224 x 157,
    100-row tiles of 14 or 30 lanes with a partial last column): a launch of 8 turns, then 8 and
    7 (an odd depth ends the paired turn loop on a single turn); all 23 counts and the board."""
    w, h, K, th = 4224, 157, 8, 100
    tw = 14 if code % 100 <= 8 else 30
    _pin_tile(monkeypatch, tw, code)
    start, want, wc = _oracle_series(oracle, 77, w, h, 3 * K - 1)
    with gol.Engine(w, h, device=0, band_rows=th, turns_per_launch=K, count_every_turn=True) as e:
        e.load_packed(start)
        e.step(K)
        assert [(k, kern) for k, kern, _ in e.last_launches()] == [(K, 15)]
        e.step(2 * K - 1)
        assert sorted(k for k, _, _ in e.last_launches()) == [K - 1, K]
        assert {(a, b) for a, b, _ in e.last_launch_tiles()} == {(tw, code)}
        got, counts = e.read_packed(), e.turn_counts(1, 3 * K - 1)
    assert counts.tolist() == wc.tolist()
    assert np.array_equal(got, want)


# ------------------------------------------------------------------ 3. degenerate boards
# boards shorter than a tile plus its halos (the loads wrap the torus several times), one tile
# column whose halo words wrap onto itself, a one-row board, and a ragged wide one; a short
# segment (turn pairs) and a long one (one turn body) each, at the shallowest depths and a deep
# one.  (width, height, tile width in lanes, tile height)
DEGENERATE_BOARDS = ((256, 64, 2, 25), (384, 3, 6, 2), (1024, 1, 14, 1), (8320, 41, 30, 13))
DEGENERATE = [(w, h, tw, th, code, K) for (w, h, tw, th) in DEGENERATE_BOARDS
              for code in (203, 516) for K in (2, 3, 32)]
_DEGENERATE_OK = [c for c in DEGENERATE
                  if all(S.tile_shape_ok(c[0] // 64, k, c[3], c[2], c[4])
                         for k in {c[5]} | set(S.even_split(2 * c[5] - 1, c[5])) - {1})]
assert 4 * len(_DEGENERATE_OK) >= 3 * len(DEGENERATE)   # at most a quarter may skip


@pytest.mark.parametrize("w,h,tw,th,code,K", DEGENERATE)
def test_counts_on_degenerate_boards(gol, oracle, monkeypatch, w, h, tw, th, code, K):
    """K turns, then 2K - 1 (K and K - 1; at K = 2 a fused launch and a one-turn launch): every
    board row and word is counted by exactly one tile, however often the loads wrap."""
    if (w, h, tw, th, code, K) not in _DEGENERATE_OK:
        pytest.skip("the tile shape check rejects this shape")
    _pin_tile(monkeypatch, tw, code)
    turns = 3 * K - 1
    start, want, wc = _oracle_series(oracle, 31 + h, w, h, turns)
    with gol.Engine(w, h, device=0, band_rows=th, turns_per_launch=K, count_every_turn=True) as e:
        e.load_packed(start)
        e.step(K)
        assert [(k, kern) for k, kern, _ in e.last_launches()] == [(K, 15)]
        e.step(2 * K - 1)
        assert [k for k, _, _ in e.last_launches()] == S.even_split(2 * K - 1, K)
        got, counts = e.read_packed(), e.turn_counts(1, turns)
    assert counts.tolist() == wc.tolist()
    assert np.array_equal(got, want)


def test_counts_deep_launch(gol, oracle, monkeypatch):
    """One launch of kMaxTileTurns = 64 turns (code 516, 30 x 120 tiles on 4224 x 600: a partial
    last tile column, 5 tile rows): 64 count slots from one launch."""
    w, h, K = 4224, 600, 64
    _pin_tile(monkeypatch, 30, 516)
    start, want, wc = _oracle_series(oracle, 64, w, h, K)
    with gol.Engine(w, h, device=0, band_rows=120, turns_per_launch=K, count_every_turn=True) as e:
        e.load_packed(start)
        e.step(K)
        assert [(k, kern) for k, kern, _ in e.last_launches()] == [(K, 15)]
        got, counts = e.read_packed(), e.turn_counts(1, K)
    assert counts.tolist() == wc.tolist()
    assert np.array_equal(got, want)


# ------------------------------------------------------------------ 4. strips
STRIP_ROWS = (96, 101, 130)
STRIP_W, STRIP_HALO, STRIP_WINDOWS = 4224, 8, (8, 8, 5)


@pytest.mark.parametrize("code,overlap", [(516, False), (103, False), (516, True)])
def test_counts_on_strips(gol, oracle, monkeypatch, code, overlap):
    """Three strip engines of 96 / 101 / 130 owned rows (halo 8, windows of 8, 8 and 5 turns, one
    counted launch each) with in-process halo copies: an engine counts its owned rows only
    (cnt_lo / cnt_hi), so the engines' series add up to the oracle's and each engine's count is
    the alive count of its own rows.  overlap: the windows go through gol_step_overlap on a side
    stream (no split on a count engine: the counted launch waits whole)."""
    import torch
    w, H, K = STRIP_W, sum(STRIP_ROWS), STRIP_HALO
    tw = 14 if code % 100 <= 8 else 30
    _pin_tile(monkeypatch, tw, code)
    turns = sum(STRIP_WINDOWS)
    start, _, wc = _oracle_series(oracle, 9, w, H, turns)
    offs = [sum(STRIP_ROWS[:i]) for i in range(len(STRIP_ROWS))]
    engs = [gol.Engine(w, H, device=0, row_offset=o, rows=r, halo=K, band_rows=40,
                       turns_per_launch=8, count_every_turn=True)
            for o, r in zip(offs, STRIP_ROWS)]
    xs = torch.cuda.Stream(device=0) if overlap else None
    try:
        for e, o, r in zip(engs, offs, STRIP_ROWS):
            rows = [(o - K + i) % H for i in range(r + 2 * K)]
            e.load_packed(start[rows])
        n = len(engs)
        for wi, m in enumerate(STRIP_WINDOWS):
            if wi:
                for i, e in enumerate(engs):
                    e.copy_halo_from_upper(engs[(i - 1) % n])
                    e.copy_halo_from_lower(engs[(i + 1) % n])
            for e in engs:
                if overlap:
                    e.step_overlap(m, xs.cuda_stream)
                else:
                    if wi:
                        e.halo_done()
                    e.step(m)
                assert [(k, kern) for k, kern, _ in e.last_launches()] == [(m, 15)]
        series = [e.turn_counts(1, turns) for e in engs]
        assert sum(series).tolist() == wc.tolist()
        for t in (1, turns):
            full = oracle.unpack(oracle.bit_run(start, w, t), w)
            for s, o, r in zip(series, offs, STRIP_ROWS):
                assert int(s[t - 1]) == int((full[o:o + r] == 255).sum())
    finally:
        for e in engs:
            e.close()


# ------------------------------------------------------------------ 5. the count ring
def test_count_ring_batches_and_wrap(gol, oracle, monkeypatch):
    """256 x 64 at code 506, launches of 19 / 18 turns (step(37)) past turn 4500: the launches
    straddle the ring's zeroing batches (256 slots) and its wrap (4352 slots); then 4400 turns
    in one call.  The whole 4096-turn window is true each time, and one turn further back is
    still refused."""
    from gol import _native as N
    w, h = 256, 64
    _pin_tile(monkeypatch, 2, 506)
    n37 = 4500 // 37 + 1
    total = 37 * n37 + 4400
    start, _, wc = _oracle_series(oracle, 13, w, h, total)
    with gol.Engine(w, h, device=0, band_rows=25, turns_per_launch=32, count_every_turn=True) as e:
        e.load_packed(start)
        for _ in range(n37):
            e.step(37)
        assert sorted(k for k, _, _ in e.last_launches()) == [18, 19]
        t = e.turn
        assert t == 37 * n37 > 4500
        assert e.turn_counts(t - 4095, 4096).tolist() == wc[t - 4096:t].tolist()
        e.step(4400)
        assert max(k for k, _, _ in e.last_launches()) > 1
        t = e.turn
        assert t == total
        assert e.turn_counts(t - 4095, 4096).tolist() == wc[t - 4096:t].tolist()
        with pytest.raises(N.GolError) as ei:
            e.turn_counts(t - 4096, 1)
        assert ei.value.code == N.GOL_EINVAL


# ------------------------------------------------------------------ 6. readers and control
def _wait_for(cond, what, seconds=20.0):
    end = time.monotonic() + seconds
    while not cond():
        assert time.monotonic() < end, what
    return True


def test_counts_for_readers_pause_and_stop(gol, oracle):
    """A long step on a worker thread, turn advancing a launch (many turns) at a time: while
    parked on PAUSE the last 64 counts up to the progress turn are true (read from this thread),
    and after RUN then STOP every count up to info().turn is."""
    from gol import _native as N
    w = h = 512
    with gol.Engine(w, h, device=0, count_every_turn=True) as e:
        e.fill_random(21)
        e.set_control(N.GOL_CONTROL_RUN)
        res = {}
        th = threading.Thread(target=lambda: res.update(done=e.step(10 ** 9)), daemon=True)
        th.start()
        try:
            _wait_for(lambda: e.progress()[0] >= 200, "the step never started")
            e.set_control(N.GOL_CONTROL_PAUSE)
            _wait_for(lambda: e.progress()[1], "the step never parked")
            t_paused, parked = e.progress()
            assert parked and t_paused >= 200
            paused_counts = e.turn_counts(t_paused - 63, 64)
            assert e.progress() == (t_paused, True)
            e.set_control(N.GOL_CONTROL_RUN)
            _wait_for(lambda: e.progress()[0] >= t_paused + 200, "the step never resumed")
        finally:
            e.set_control(N.GOL_CONTROL_STOP)
            th.join(20)
        assert not th.is_alive() and res["done"] is False
        e.sync()
        t_end = e.turn
        assert t_end >= t_paused + 200
        n = min(t_end, 4096)
        tail = e.turn_counts(t_end - n + 1, n)
        got = e.read_packed()
    want, wc = oracle.bit_run(oracle.gen_random(21, w, h), w, t_end, counts=True)
    wc = wc.astype(np.int64)
    assert paused_counts.tolist() == wc[t_paused - 64:t_paused].tolist()
    assert tail.tolist() == wc[t_end - n:t_end].tolist()
    assert np.array_equal(got, want)


# ------------------------------------------------------------------ 7. non-binary first turn
def test_counts_nonbinary_first_turn(gol, oracle):
    """512 x 130 bytes with a few values outside {0, 255}: turn 1 applies the reference's
    non-binary rule in a one-turn launch, the turns after it are fused."""
    w, h, turns = 512, 130, 20
    rng = np.random.default_rng(130)
    board = np.where(rng.random((h, w)) < 0.4, 255, 0).astype(np.uint8)
    for y, x, v in ((0, 0, 1), (5, 17, 128), (64, 511, 254), (129, 300, 7), (77, 64, 200)):
        board[y, x] = v
    words, blocked, nb = oracle.pack(board)
    assert nb == 5
    want, wc = oracle.bit_run(words, w, turns, blocked=blocked, counts=True)
    with gol.Engine(w, h, device=0, count_every_turn=True) as e:
        e.load(board)
        e.step(turns)
        launches = e.last_launches()
        got, counts = e.read_packed(), e.turn_counts(1, turns)
    assert launches[0][0] == 1
    fused = [(k, kern) for k, kern, _ in launches[1:] if k > 1]
    assert fused and all(kern == 15 for _, kern in fused), launches
    assert counts.tolist() == wc.astype(np.int64).tolist()
    assert np.array_equal(got, want)


# ------------------------------------------------------------------ 8. fallback unchanged
@pytest.mark.parametrize("how", ["band_rows", "mv7", "uncounted_code"])
def test_count_engines_without_a_counted_kernel(gol, oracle, monkeypatch, how):
    """Count engines whose multi-turn kernel has no counted form run one turn per launch as
    before: a caller-given band with no tile variant, k_step_skew (GOL_MULTI_VARIANT=7), and a
    GOL_TILE code outside gol_tile_count_codes (which must not fail the create)."""
    w, h = 1024, 203
    kw = {}
    if how == "band_rows":
        kw["band_rows"] = 7
    elif how == "mv7":
        monkeypatch.setenv("GOL_MULTI_VARIANT", "7")
    else:
        code = 1004
        assert code not in COUNT_CODES
        _pin_tile(monkeypatch, 7, code)
        kw.update(band_rows=40, turns_per_launch=8)
    start, want, wc = _oracle_series(oracle, 8, w, h, 9)
    with gol.Engine(w, h, device=0, count_every_turn=True, **kw) as e:
        e.load_packed(start)
        e.step(9)
        assert [k for k, _, _ in e.last_launches()] == [1] * 9
        got, counts = e.read_packed(), e.turn_counts(1, 9)
    assert counts.tolist() == wc.tolist()
    assert np.array_equal(got, want)
