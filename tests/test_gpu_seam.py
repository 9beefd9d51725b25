"""k_step_tile on boards whose width is no multiple of 128: across the row seam (width % 64 != 0,
the torus wraps in x inside the row's last word -- tile_pass SEAM, k_step_tile_seam) and on odd
word counts (width % 64 == 0), against the CPU oracle at small shapes.

The reference everywhere is oracle.bit_run from oracle.gen_random, compared bit for bit.  The
pinned cases assert their launches through last_launches / last_launch_tiles, so none passes by
running one turn per launch; the unpinned ones assert that the engine's own plan runs multi-turn
launches of k_step_tile at a gol_tile_seam_codes code.
"""
import ctypes

import numpy as np
import pytest

import strip_tiles as S
from gol import _native
from test_gpu_strip_tiles import _Strips, _run_split, delay_buffers, torch  # noqa: F401

pytestmark = pytest.mark.gpu

K = 8
# tile heights by rows per segment: several tile rows on a 200-row board, none that divides 77
# or 200 (a short last tile row), and on 77 rows tiles whose halo rows wrap the torus
TILE_H = {2: 3, 4: 6, 6: 12, 8: 19, 12: 35, 16: 51, 24: 60}
assert all(77 % th and 200 % th for th in TILE_H.values())


@pytest.fixture(scope="module")
def gol():
    import gol as g
    return g


def _seam_codes():
    from gol import _native as N
    n = N.lib().gol_tile_seam_codes(None, 0)
    buf = (ctypes.c_int32 * n)()
    assert N.lib().gol_tile_seam_codes(buf, n) == n
    return tuple(buf)


SEAM_CODES = _seam_codes()


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


def _run_pinned(gol, oracle, monkeypatch, w, h, tw, code, th, k=K):
    """One launch of k turns, then launches of k and k - 1; the board after each call."""
    _pin_tile(monkeypatch, tw, code)
    start, (want_mid, want) = _oracle_run(oracle, w + h, w, h, (k, 2 * k - 1))
    with gol.Engine(w, h, device=0, band_rows=th, turns_per_launch=k) as e:
        assert e.info().turns_per_launch == k and e.info().fast_path == 0
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


# ------------------------------------------------------------------ pinned shapes
# width, tile width: 257 (r = 1) as two columns 3 + 2 and as one column with both halo columns
# stitched in the same tile; 319 (r = 63); 1000 (r = 40, even) as 13 + a narrow column of 3;
# 1055 (r = 31, odd, and 17 words); 2113 (r = 1, 34 words): interior columns with no stitch
# beside the two that have it
SEAM_SHAPES = [(257, 3), (257, 5), (319, 3), (1000, 13), (1055, 13), (2113, 13)]


@pytest.mark.parametrize("h", [77, 200])
@pytest.mark.parametrize("code", SEAM_CODES)
@pytest.mark.parametrize("w,tw", SEAM_SHAPES)
def test_seam_code_pinned(gol, oracle, monkeypatch, w, tw, code, h):
    """Every seam code on every seam shape: step(8) then step(15) (8 + 7), on 200 rows and on
    77 (tile rows that wrap the torus, a short last tile row)."""
    _run_pinned(gol, oracle, monkeypatch, w, h, tw, code, TILE_H[code % 100])


@pytest.mark.parametrize("code", [108, 516])
@pytest.mark.parametrize("w,tw", [(320, 3), (4160, 13)])
def test_odd_word_count_whole_words(gol, oracle, monkeypatch, w, tw, code):
    """r = 0 with an odd word count (5 and 65 words): the plain one-word-per-lane kernels."""
    _run_pinned(gol, oracle, monkeypatch, w, 77, tw, code, TILE_H[code % 100])


@pytest.mark.parametrize("w", [320, 4160, 1000])
def test_two_word_code_refused(gol, monkeypatch, w):
    """A two-words-per-lane code on an odd word count, or across the seam, is refused at create,
    not run."""
    _pin_tile(monkeypatch, 2, 1104)
    with pytest.raises(_native.GolError):
        gol.Engine(w, 77, device=0, band_rows=5, turns_per_launch=K).close()


def test_code_outside_the_seam_set_refused(gol, monkeypatch):
    """A one-word code without a seam instantiation is refused across the seam."""
    from conftest import TILE_CODES
    code = next(c for c in TILE_CODES if c < 1000 and c not in SEAM_CODES)
    _pin_tile(monkeypatch, 13, code)
    with pytest.raises(_native.GolError):
        gol.Engine(1000, 77, device=0, band_rows=19, turns_per_launch=K).close()


# ------------------------------------------------------------------ the deepest launch
@pytest.mark.parametrize("w", [257, 319])
def test_seam_deepest_launch(gol, oracle, monkeypatch, w):
    """One launch of 64 turns and one of 63 on one tile column at code 16: the x-halo is exactly
    64 cells, so a stitch that is short by one cell shows only here."""
    tw, code, th = 5, 16, 77
    _pin_tile(monkeypatch, tw, code)
    start, (want_mid, want) = _oracle_run(oracle, w, w, 77, (64, 63))
    with gol.Engine(w, 77, device=0, band_rows=th, turns_per_launch=64) as e:
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


# ------------------------------------------------------------------ the padding invariant
def test_seam_padding_stays_zero(gol, oracle, monkeypatch):
    """1000 x 77: after a multi-turn launch the popcount and the alive list (both read every bit
    of the last word) are the oracle's, and a one-turn step after it -- the layout round trip
    with a partial word, the one-turn kernel on the stored board -- flips the oracle's cells."""
    w, h, tw, code = 1000, 77, 13, 108
    _pin_tile(monkeypatch, tw, code)
    start, (b8, b9) = _oracle_run(oracle, 4321, w, h, (K, 1))
    with gol.Engine(w, h, device=0, band_rows=TILE_H[8], turns_per_launch=K) as e:
        e.load_packed(start)
        e.step(K)
        assert [(a, v) for a, v, _ in e.last_launches()] == [(K, 15)]
        assert e.snapshot() == (K, oracle.popcount(b8, w))
        bytes8 = oracle.unpack(b8, w)
        assert np.array_equal(e.alive_cells(), oracle.ref_alive_cells(bytes8))
        e.step(1)
        assert [a for a, _, _ in e.last_launches()] == [1]
        flips = e.flipped_cells()
        got = e.read_packed()
    assert np.array_equal(got, b9)
    ys, xs = np.nonzero(bytes8 != oracle.unpack(b9, w))
    assert np.array_equal(flips, np.stack([xs, ys], axis=1).astype(np.int64))


# ------------------------------------------------------------------ unpinned engines
@pytest.mark.parametrize("w,h,turns", [(1000, 600, 100), (1920, 1080, 100), (8200, 8200, 20)])
def test_seam_engine_plans_tile_launches(gol, oracle, w, h, turns):
    """No environment overrides: the engine's own plan at these widths is multi-turn launches of
    k_step_tile at a seam code -- also at 8200^2 (1.06 M words: the large-board planner's
    size) -- and the board is the oracle's.

    1920 = 15 x 128 is a fast-path width: its engine ran multi-turn k_step_tile launches before
    the seam kernel and searches every shipped code, not the seam set alone.  Its pick on an
    MI355X is code 2 (4 x 25 turns on 6 x 64, 10 x 16 or 6 x 32 tiles, every run seen), which
    the seam set holds because boards of this size run fastest on it: with it a 1000^2 board
    runs 0.369 us per turn, without it 0.460."""
    start = oracle.gen_random(w + turns, w, h)
    with gol.Engine(w, h, device=0) as e:
        info = e.info()
        assert info.turns_per_launch > 1 and info.blocking_limited == 0
        assert info.fast_path == int(w % 128 == 0)       # (its meaning stays: the one-turn stencil)
        e.load_packed(start)
        e.step(turns)
        plan, tiles = e.last_launches(), e.last_launch_tiles()
        got = e.read_packed()
    print(f"{w}x{h}: plan {plan} tiles {tiles}")
    assert sum(k for k, _, _ in plan) == turns and max(k for k, _, _ in plan) > 1
    for (k, v, _), (_, code, _) in zip(plan, tiles):
        assert k == 1 or (v == 15 and code in SEAM_CODES), (plan, tiles)
    assert np.array_equal(got, oracle.bit_run(start, w, turns))


# ------------------------------------------------------------------ unchanged paths
@pytest.mark.parametrize("kw", [dict(force_generic=True), dict(turns_per_launch=1),
                                dict(count_every_turn=True)], ids=lambda kw: next(iter(kw)))
def test_one_turn_paths_unchanged(gol, oracle, kw):
    """Forced-generic engines, turns_per_launch = 1 and count engines keep one-turn launches at
    these widths, with the oracle's board and counts."""
    w, h, turns = 1000, 77, 9
    start = oracle.gen_random(99, w, h)
    want, wc = oracle.bit_run(start, w, turns, counts=True)
    with gol.Engine(w, h, device=0, **kw) as e:
        assert e.info().turns_per_launch == 1
        e.load_packed(start)
        e.step(turns)
        assert [k for k, _, _ in e.last_launches()] == [1] * turns
        assert e.snapshot() == (turns, int(wc[-1]))
        if "count_every_turn" in kw:
            assert e.turn_counts(1, turns).tolist() == wc.astype(np.int64).tolist()
        got = e.read_packed()
    assert np.array_equal(got, want)


def test_narrow_board_keeps_one_turn_launches(gol, oracle):
    """Widths below 256 do not block."""
    start = oracle.gen_random(5, 200, 77)
    with gol.Engine(200, 77, device=0) as e:
        assert e.info().turns_per_launch == 1
        e.load_packed(start)
        e.step(9)
        assert [k for k, _, _ in e.last_launches()] == [1] * 9
        got = e.read_packed()
    assert np.array_equal(got, oracle.bit_run(start, 200, 9))


# ------------------------------------------------------------------ row strips
STRIP_W, STRIP_H, STRIP_N, STRIP_HALO, STRIP_TPL = 1000, 157, 3, 11, 8
STRIP_WINDOWS = (11, 11, 7)       # 6 + 5 (the second launch starts 6 turns in), 6 + 5, 7
STRIP_TILE_H = {8: 19, 16: 20}


@pytest.mark.parametrize("code", [108, 516])
def test_seam_on_strips(gol, oracle, monkeypatch, code):
    """Three strips of 53 / 52 / 52 rows of a 1000 x 157 board with 11-row halos (row_lo > 0, no
    torus wrap in y, a computed range that shrinks per launch, a launch that starts mid-window):
    the halo rows cross between the engines in the standard layout, partial word included."""
    tw, th = 13, STRIP_TILE_H[code % 100]
    _pin_tile(monkeypatch, tw, code)
    turns = (STRIP_WINDOWS[0], sum(STRIP_WINDOWS[1:]))
    start, (want_mid, want) = _oracle_run(oracle, code + 157, STRIP_W, STRIP_H, turns)

    def check(e, m):
        plan = e.last_launches()
        assert [v for _, v, _ in plan] == [15] * len(plan), plan
        assert [k for k, _, _ in plan] == S.even_split(m, STRIP_TPL), plan
        assert {(a, b) for a, b, _ in e.last_launch_tiles()} == {(tw, code)}

    with _Strips(gol, start, STRIP_W, STRIP_N, STRIP_HALO, band_rows=th,
                 turns_per_launch=STRIP_TPL) as s:
        s.step(turns[0], check)
        assert [k for k, _, _ in s.engs[0].last_launches()] == [6, 5]
        mid = s.read()
        s.step(turns[1], check)
        got = s.read()
    assert np.array_equal(mid, want_mid)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("code", [108, 516])
def test_seam_split_launch(gol, oracle, torch, monkeypatch, delay_buffers, code):  # noqa: F811
    """gol_step_overlap's split first launch (interior rows, then the rows next to the halos on
    16-row tiles behind the delayed receives) and the whole launches after it, two strips of a
    1000 x 130 board on 13-lane tiles; the halo buffers are handed out in the interleaved
    layout."""
    monkeypatch.setattr(S, "split_tile_w", lambda c: 13)     # (the helper's widths exceed 16 words)
    case = dict(S.SPLIT_FORMS["first_of_three"], mv=15, code=code, w=1000, n=2, band=16)
    got, start, _ = _run_split(gol, oracle, torch, monkeypatch, case, delay_buffers)
    assert np.array_equal(got, oracle.bit_run(start, case["w"], sum(case["windows"])))


# ------------------------------------------------------------------ the run driver
@pytest.mark.parametrize("ngpus", [1, 3])
def test_seam_through_run(gol, oracle, tmp_path, ngpus):
    """gol.Run on a 300 x 200 random PGM for 100 turns, on one engine and on three strips of
    device 0: the output PGM and FinalTurnComplete.Alive are the reference restatement's."""
    w, h, turns = 300, 200, 100
    (tmp_path / "images").mkdir()
    start = oracle.unpack(oracle.gen_random(31, w, h), w)
    (tmp_path / "images" / f"{w}x{h}.pgm").write_bytes(f"P5\n{w} {h}\n255\n".encode() +
                                                      start.tobytes())
    want = oracle.ref_run(start, turns)
    p = gol.Params(Turns=turns, Threads=4, ImageWidth=w, ImageHeight=h)
    kw = dict(ngpus=ngpus, devices=[0] * ngpus) if ngpus > 1 else {}
    events = gol.Channel()
    run = gol.Run(p, events, None, image_dir=str(tmp_path / "images"),
                  out_dir=str(tmp_path / "out"), **kw)
    evs = list(events)
    run.wait(5)
    assert run.error is None, run.error
    final = [e for e in evs if isinstance(e, gol.FinalTurnComplete)]
    assert len(final) == 1 and final[0].CompletedTurns == turns
    got = np.array([(c.X, c.Y) for c in final[0].Alive], dtype=np.int64).reshape(-1, 2)
    alive = oracle.ref_alive_cells(want)
    assert got.shape == alive.shape
    assert np.array_equal(got[np.lexsort((got[:, 0], got[:, 1]))], alive)
    out = (tmp_path / "out" / f"{w}x{h}x{turns}.pgm").read_bytes()
    assert out == f"P5\n{w} {h}\n255\n".encode() + want.tobytes()
