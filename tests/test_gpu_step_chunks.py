"""gol_step's chunked pipeline (consecutive k_step_tile launches cut into row chunks on two
streams, GOL_STEP_CHUNKS) against the CPU oracle at small shapes.

The board is a 2688-wide torus: 42 lanes at tile width 13 leave a narrow last column, which
every chunk of two or more tile rows repacks into narrow tiles of its own.  Tiles are 40 rows
tall; 203 rows are 5 tile rows and a 3-row one, 270 rows are 6 and a 30-row one.  A step of 23
turns at 6 turns per launch runs launches of 6, 6, 6 and 5 turns, so the last pair of launches
has two depths.  Every case asserts Engine.last_step_chunks(), so none passes by never taking
the path, and compares the whole board with oracle.bit_run bit for bit.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, TW, TH, K, TURNS = 2688, 13, 40, 6, 23
LAUNCHES = [6, 6, 6, 5]
CODES = (104, 516)
HEIGHTS = (203, 270)
ALL = 64                      # "as many as fit": more than any of these boards has tile rows


@pytest.fixture(scope="module")
def gol():
    import gol as g
    return g


def _pin(monkeypatch, code, chunks):
    monkeypatch.setenv("GOL_MULTI_VARIANT", "15")
    monkeypatch.setenv("GOL_TILE", f"{TW},{code}")
    monkeypatch.setenv("GOL_STEP_CHUNKS", str(chunks))


def _fit(h, want, k=K, th=TH):
    """The chunks a launch gets when `want` are asked for (gol_step_chunk_plan)."""
    from gol import _native as N
    counts = (ctypes.c_int32 * 2)()
    b0, b1 = (ctypes.c_int32 * (ALL + 1))(), (ctypes.c_int32 * (ALL + 1))()
    deps = (ctypes.c_uint8 * (ALL * ALL))()
    assert N.lib().gol_step_chunk_plan(h, k, th, want, k, th, want, counts, b0, b1, deps, ALL) == 0
    assert counts[0] == counts[1]
    return counts[0]


_RUNS = {}


def _boards(oracle, h, turns_list, w=W):
    """(start, boards after each cumulative turn count): computed once per key and shared;
    callers do not modify them."""
    key = (w, h, tuple(turns_list))
    if key not in _RUNS:
        start = oracle.gen_random(900 + h + (w if w != W else 0), w, h)
        boards, cur = [], start
        for t in turns_list:
            cur = oracle.bit_run(cur, w, t)
            boards.append(cur)
        for a in [start] + boards:
            a.setflags(write=False)
        _RUNS[key] = (start, boards)
    return _RUNS[key]


def _engine(gol, h, k=K, th=TH, w=W, **kw):
    return gol.Engine(w, h, device=0, band_rows=th, turns_per_launch=k, **kw)


def _expect(n):
    return len(LAUNCHES) * n if n > 1 else 0


@pytest.mark.parametrize("chunks", [1, 2, 3, 4, 5, ALL])
@pytest.mark.parametrize("h", HEIGHTS)
@pytest.mark.parametrize("code", CODES)
def test_chunk_counts(gol, oracle, monkeypatch, code, h, chunks):
    """1 (off), 2 and 3 (every chunk follows every chunk), 4, 5 and as many as fit (5 of the
    203 rows' 6 tile rows: the 3-row one is shorter than a launch is deep; 7 of 270's 7)."""
    _pin(monkeypatch, code, chunks)
    n = _fit(h, chunks)
    assert n == (min(chunks, 5 if h == 203 else 7))
    start, (want,) = _boards(oracle, h, (TURNS,))
    with _engine(gol, h) as e:
        e.load_packed(start)
        e.step(TURNS)
        assert [(k, v, b) for k, v, b in e.last_launches()] == [(k, 15, TH) for k in LAUNCHES]
        assert {(a, b) for a, b, _ in e.last_launch_tiles()} == {(TW, code)}
        assert e.last_step_chunks() == _expect(n)
        assert e.info().launches == len(LAUNCHES) and e.info().turn == TURNS
        got = e.read_packed()
    assert np.array_equal(got, want)


@pytest.mark.parametrize("code", CODES)
def test_steps_back_to_back(gol, oracle, monkeypatch, code):
    """Two steps with different chunk counts and a read between them: the first step's side
    chunks are joined before the read and before the second step's first chunks."""
    h = 270
    start, (mid_want, want) = _boards(oracle, h, (TURNS, 2 * K))
    _pin(monkeypatch, code, 3)
    with _engine(gol, h) as e:
        e.load_packed(start)
        e.step(TURNS)
        assert e.last_step_chunks() == 4 * 3
        mid = e.read_packed()
        monkeypatch.setenv("GOL_STEP_CHUNKS", "5")
        e.step(2 * K)
        assert [k for k, _, _ in e.last_launches()] == [K, K]
        assert e.last_step_chunks() == 2 * 5
        got = e.read_packed()
    assert np.array_equal(mid, mid_want)
    assert np.array_equal(got, want)


def test_lone_launch_stays_whole(gol, oracle, monkeypatch):
    """A step of one launch is one kernel, whatever GOL_STEP_CHUNKS asks for."""
    h = 203
    start, (want,) = _boards(oracle, h, (K,))
    _pin(monkeypatch, 516, 4)
    with _engine(gol, h) as e:
        e.load_packed(start)
        e.step(K)
        assert [k for k, _, _ in e.last_launches()] == [K]
        assert e.last_step_chunks() == 0
        got = e.read_packed()
    assert np.array_equal(got, want)


@pytest.mark.parametrize("chunks", [4, 5])
@pytest.mark.parametrize("code", CODES)
def test_step_ends_in_one_turn_launch(gol, oracle, monkeypatch, code, chunks):
    """5 turns at 2 turns per launch run as 2, 2 and 1: the one-turn launch and the layout
    conversion in front of it meet a live pipeline inside the step, and the engine stream
    joins the side chunks before them."""
    h = 203
    start, (want,) = _boards(oracle, h, (5,))
    _pin(monkeypatch, code, chunks)
    n = _fit(h, chunks, k=2)
    assert n == chunks
    with _engine(gol, h, k=2) as e:
        e.load_packed(start)
        e.step(5)
        assert [(k, v) for k, v, _ in e.last_launches()] == [(2, 15), (2, 15), (1, 0)]
        assert e.last_step_chunks() == 2 * n
        got = e.read_packed()
    assert np.array_equal(got, want)


# 4013 rows on 400-row tiles at 30 turns per launch, the headline's depth: chunks of 400 to
# 1213 rows in 8-wave workgroups, long enough to be in flight together on the two streams
TALL_H, TALL_TH, TALL_K = 4013, 400, 30


@pytest.mark.parametrize("chunks", [4, 5, 10])
def test_chunks_in_flight(gol, oracle, monkeypatch, chunks):
    """Four, five and ten chunks of deep launches on tall tiles, where a chunk follows only its
    neighbours in the launch before.  (This checks the board at that shape; it does not by
    itself prove the waits: with the cross-stream waits dropped only the cases where every
    chunk follows every chunk fail, because two in-order streams running chunks of equal length
    keep a chunk's neighbours ahead of it anyway.  DESIGN.md, "Negative controls".)"""
    start, (want,) = _boards(oracle, TALL_H, (3 * TALL_K,))
    _pin(monkeypatch, 516, chunks)
    n = _fit(TALL_H, chunks, k=TALL_K, th=TALL_TH)
    assert n == chunks
    with _engine(gol, TALL_H, k=TALL_K, th=TALL_TH) as e:
        e.load_packed(start)
        e.step(3 * TALL_K)
        assert [(k, v, b) for k, v, b in e.last_launches()] == [(TALL_K, 15, TALL_TH)] * 3
        assert e.last_step_chunks() == 3 * n
        got = e.read_packed()
    assert np.array_equal(got, want)


@pytest.mark.parametrize("code", CODES)
def test_one_turn_step_after_chunks(gol, oracle, monkeypatch, code):
    """A chunked step, then a step of one turn: the layout conversion in front of it reads the
    whole board on the engine stream, after every side chunk (joined when the first step
    returned)."""
    h = 203
    start, (prev, want) = _boards(oracle, h, (TURNS, 1))
    _pin(monkeypatch, code, 4)
    with _engine(gol, h) as e:
        e.load_packed(start)
        e.step(TURNS)
        assert e.last_step_chunks() == 4 * 4
        e.step(1)
        assert [k for k, _, _ in e.last_launches()] == [1]
        assert e.last_step_chunks() == 0
        flips = e.flipped_cells()
        got = e.read_packed()
    assert np.array_equal(got, want)
    # the other half of the double buffer is the board exactly one turn back, after the join
    # and the conversion: the flip list is the oracle's for this turn
    yx = np.argwhere(oracle.unpack(prev, W) != oracle.unpack(want, W))
    want_flips = np.ascontiguousarray(yx[:, ::-1].astype(np.int64))
    assert len(want_flips) > 0
    assert flips.shape == want_flips.shape and np.array_equal(flips, want_flips)


SEAM_W = 1000                 # 15 words and 40 cells: the torus seam in x lies inside the last word


@pytest.mark.parametrize("chunks", [2, 4, ALL])
@pytest.mark.parametrize("h", HEIGHTS)
@pytest.mark.parametrize("code", CODES)
def test_seam_kernel_chunked(gol, oracle, monkeypatch, code, h, chunks):
    """k_step_tile_seam under chunking (chunk_eligible does not exclude it, and large boards of
    such widths reach it in automatic mode): 16 lane columns at tile width 13 leave a narrow
    last column, repacked per chunk, and the chunks run the seam kernel with row_lo > 0 on a
    torus that wraps.  Both codes are seam codes (gol_tile_seam_codes)."""
    _pin(monkeypatch, code, chunks)
    n = _fit(h, chunks)
    assert n == (min(chunks, 5 if h == 203 else 7))
    start, (want,) = _boards(oracle, h, (TURNS,), w=SEAM_W)
    with _engine(gol, h, w=SEAM_W) as e:
        assert e.info().fast_path == 0
        e.load_packed(start)
        e.step(TURNS)
        assert [(k, v, b) for k, v, b in e.last_launches()] == [(k, 15, TH) for k in LAUNCHES]
        assert {(a, b) for a, b, _ in e.last_launch_tiles()} == {(TW, code)}
        assert e.last_step_chunks() == _expect(n)
        assert e.info().launches == len(LAUNCHES) and e.info().turn == TURNS
        got = e.read_packed()
    assert np.array_equal(got, want)


def test_two_words_per_lane_chunked(gol, oracle, monkeypatch):
    """One two-words-per-lane code (1106) under chunking, at the tile shape test_tile_code_pinned
    runs that family at (7 lanes x 100 rows): 21 lane columns are 3 tile columns; 430 rows are 4
    tile rows and a 30-row one, so 4 chunks of 100, 100, 100 and 130 rows."""
    code, tw, th, h = 1106, 7, 100, 430
    monkeypatch.setenv("GOL_MULTI_VARIANT", "15")
    monkeypatch.setenv("GOL_TILE", f"{tw},{code}")
    monkeypatch.setenv("GOL_STEP_CHUNKS", "4")
    assert _fit(h, 4, th=th) == 4
    start, (want,) = _boards(oracle, h, (TURNS,))
    with _engine(gol, h, th=th) as e:
        e.load_packed(start)
        e.step(TURNS)
        assert [(k, v, b) for k, v, b in e.last_launches()] == [(k, 15, th) for k in LAUNCHES]
        assert {(a, b) for a, b, _ in e.last_launch_tiles()} == {(tw, code)}
        assert e.last_step_chunks() == 4 * 4
        got = e.read_packed()
    assert np.array_equal(got, want)


@pytest.mark.parametrize("code", CODES)
def test_nonbinary_load_then_chunked_step(gol, oracle, monkeypatch, code):
    """A board loaded with a few bytes outside {0, 255}, then one chunked step: the first launch
    is the one-turn masked launch, the pipeline starts behind it and behind the layout
    conversion, and the mask is released after the join.  The 22 turns after the first spread
    evenly over 4 launches: 6, 6, 5, 5."""
    h = 203
    start = _boards(oracle, h, (TURNS,))[0]
    board = oracle.unpack(start, W).copy()
    for y, x, v in ((0, 0, 1), (5, 17, 128), (39, 2687, 254), (40, 832, 7), (202, 1300, 200),
                    (120, 63, 100), (121, 64, 3)):
        board[y, x] = v
    words, blocked, nb = oracle.pack(board)
    assert nb == 7
    want = oracle.bit_run(words, W, TURNS, blocked=blocked)
    assert not np.array_equal(want, oracle.bit_run(words, W, TURNS))     # (the mask matters)
    _pin(monkeypatch, code, 4)
    with _engine(gol, h) as e:
        e.load(board)
        assert e.info().nonbinary_cells == 7
        e.step(TURNS)
        assert [(k, v) for k, v, _ in e.last_launches()] == [(1, 0), (6, 15), (6, 15), (5, 15),
                                                             (5, 15)]
        assert e.last_step_chunks() == 4 * 4
        got = e.read_packed()
        # (the mask is gone: a further one-turn step is an ordinary one)
        e.step(1)
        after = e.read_packed()
    assert np.array_equal(got, want)
    assert np.array_equal(after, oracle.bit_run(want, W, 1))


def test_control_word_engine_is_not_chunked(gol, oracle, monkeypatch):
    from gol import _native as N
    h = 203
    start, (want,) = _boards(oracle, h, (TURNS,))
    _pin(monkeypatch, 516, 4)
    with _engine(gol, h) as e:
        e.load_packed(start)
        e.set_control(N.GOL_CONTROL_RUN)
        assert e.step(TURNS)
        assert [k for k, _, _ in e.last_launches()] == LAUNCHES
        assert e.last_step_chunks() == 0
        got = e.read_packed()
    assert np.array_equal(got, want)


def test_count_engine_is_not_chunked(gol, oracle, monkeypatch):
    h = 203
    start = _boards(oracle, h, (TURNS,))[0]
    want, wc = oracle.bit_run(start, W, TURNS, counts=True)
    _pin(monkeypatch, 516, 4)
    with _engine(gol, h, count_every_turn=True) as e:
        e.load_packed(start)
        e.step(TURNS)
        assert sorted(k for k, _, _ in e.last_launches()) == sorted(LAUNCHES)
        assert e.last_step_chunks() == 0
        got, counts = e.read_packed(), e.turn_counts(1, TURNS)
    assert counts.tolist() == wc.astype(np.int64).tolist()
    assert np.array_equal(got, want)


def test_strip_engine_is_not_chunked(gol, oracle, monkeypatch):
    """Two strips of the 270-row board with 12-row halos: launches of 6 and 6 turns each."""
    from test_gpu_strip_tiles import _Strips
    h, halo = 270, 2 * K
    start, (want,) = _boards(oracle, h, (2 * K,))
    _pin(monkeypatch, 516, 4)

    def check(e, m):
        assert [(k, v) for k, v, _ in e.last_launches()] == [(K, 15), (K, 15)]
        assert e.last_step_chunks() == 0

    with _Strips(gol, start, W, 2, halo, band_rows=TH, turns_per_launch=K) as s:
        s.step(2 * K, check)
        got = s.read()
    assert np.array_equal(got, want)


def test_on_a_torch_stream(gol, oracle, monkeypatch):
    """The engine on a non-default torch stream, as the benchmark sets it: work queued on that
    stream after step() follows every chunk."""
    import torch
    h = 270
    start, (want,) = _boards(oracle, h, (TURNS,))
    _pin(monkeypatch, 516, 3)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream), _engine(gol, h) as e:
        e.set_stream(stream.cuda_stream)
        e.load_packed(start)
        e.step(TURNS)
        assert e.last_step_chunks() == 4 * 3
        done = torch.cuda.Event()
        done.record(stream)
        done.synchronize()
        got = e.read_packed()
    assert np.array_equal(got, want)
