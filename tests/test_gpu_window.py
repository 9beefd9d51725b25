"""The window calls (gol_read_window, gol_window_density, gol_write_window, gol_clear,
gol_board_layout; kernels k_window_unpack / k_window_density / k_window_pack) against the CPU
oracle, on the board in both layouts.

No expected value comes from the engine: boards are oracle.gen_random stepped by oracle.bit_run
and unpacked by oracle.unpack, windows are numpy slices of them (indices taken mod the board),
patches are applied in numpy and packed by oracle.pack.  Every window taken from a random board
is asserted to hold alive and dead cells both, so an all-zero answer cannot pass (the four 1 x 1
corner windows are asserted as a group).

The multi-turn engines are pinned the way test_gpu_seam.py pins them (k_step_tile, 13-lane
tiles, code 108, 8 turns per launch), so that after step(8) the board IS in the interleaved
layout -- asserted, not assumed.
"""
import os
import subprocess
import sys
import threading
import time

import numpy as np
import pytest

from gol import _native
from test_gpu_big import H as BIG_H, PAD, SOUP, SOUPS, TORUS, W as BIG_W
from test_gpu_seam import TILE_H, _oracle_run, _pin_tile
from test_gpu_strip_tiles import _Strips

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGE_LIB = os.path.join(ROOT, "conway-s-gol-distributed_amd", "build", "libgolamd_stage64k.so")

K = 8
BH = 77
BOARDS = (1000, 1024)                 # r = 40 (a row seam) and whole words


@pytest.fixture(scope="module")
def gol():
    import gol as g
    return g


def _windows(W, H):
    """(x, y, w, h): the whole board; one crossing the x wrap, the y wrap, both corners; x and w
    no multiples of 64; two that start inside the row's last word (one of them wraps); rows of
    whole 16-byte units at an aligned and at an odd start (the 16-byte byte side); a window as
    wide as the board that starts mid-row (its two ends share a word)."""
    return [(0, 0, W, H), (W - 30, 5, 100, 20), (100, H - 10, 200, 25), (W - 37, H - 7, 90, 15),
            (37, 11, 333, 9), (W - 30, 3, 114, 5), (W - 10, 0, 10, 4), (64, 2, 128, 6),
            (5, 1, 256, 3), (500, 70, W, 3)]


def _corners(W, H):
    return [(0, 0, 1, 1), (W - 1, 0, 1, 1), (0, H - 1, 1, 1), (W - 1, H - 1, 1, 1)]


def _win(board, x, y, w, h):
    """The window of a (H, W) array, indices mod the board."""
    H, W = board.shape
    return board[np.ix_((y + np.arange(h)) % H, (x + np.arange(w)) % W)]


def _both(a, what=None):
    assert (a == 255).any() and (a == 0).any(), what


def _engine(gol, monkeypatch, w, h=BH, **kw):
    _pin_tile(monkeypatch, 13, 108)
    return gol.Engine(w, h, device=0, band_rows=TILE_H[8], turns_per_launch=K, **kw)


def _boards(oracle, W):
    """start, after 8 and after 16 turns (packed), shared and read-only.  (Seeds at which the
    four corner cells hold both states at turn 0 and at turn 8.)"""
    start, (b8, b16) = _oracle_run(oracle, {1000: 2, 1024: 1}[W], W, BH, (K, K))
    return start, b8, b16


def _check_windows(oracle, e, packed, W, turn):
    want_board = oracle.unpack(packed, W)
    for (x, y, w, h) in _windows(W, BH):
        got, t = e.read_window(x, y, w, h)
        want = _win(want_board, x, y, w, h)
        _both(want, (x, y, w, h))
        assert t == turn
        assert got.shape == (h, w) and np.array_equal(got, want), (W, turn, x, y, w, h)
    corner = []
    for (x, y, w, h) in _corners(W, BH):
        got, t = e.read_window(x, y, w, h)
        want = _win(want_board, x, y, w, h)
        corner.append(int(want[0, 0]))
        assert t == turn and np.array_equal(got, want), (W, turn, x, y)
    assert 0 in corner and 255 in corner


# ------------------------------------------------------------------ 1. read, both layouts
@pytest.mark.parametrize("W", BOARDS)
def test_read_window_both_layouts(gol, oracle, monkeypatch, W):
    start, b8, b16 = _boards(oracle, W)
    with _engine(gol, monkeypatch, W) as e:
        e.load_packed(start)
        assert e.board_layout() == 0
        _check_windows(oracle, e, start, W, 0)
        assert e.board_layout() == 0
        e.step(K)
        assert [(a, v) for a, v, _ in e.last_launches()] == [(K, 15)]
        assert e.board_layout() == 1
        _check_windows(oracle, e, b8, W, K)
        assert e.board_layout() == 1                      # no read converted the buffer
        e.step(K)
        assert [(a, v) for a, v, _ in e.last_launches()] == [(K, 15)]
        got = e.read_packed()
        assert e.board_layout() == 0                      # (the whole-board read-out does)
    assert np.array_equal(got, b16)


@pytest.mark.parametrize("what", ["x", "y", "w0", "h0", "w_big", "h_big", "x_neg", "y_neg"])
def test_window_arguments_refused(gol, oracle, what):
    W, H = 320, 40
    bad = {"x": (W, 0, 1, 1), "y": (0, H, 1, 1), "w0": (0, 0, 0, 1), "h0": (0, 0, 1, 0),
           "w_big": (0, 0, W + 1, 1), "h_big": (0, 0, 1, H + 1), "x_neg": (-1, 0, 1, 1),
           "y_neg": (0, -1, 1, 1)}[what]
    start = oracle.gen_random(3, W, H)
    with gol.Engine(W, H, device=0) as e:
        e.load_packed(start)
        x, y, w, h = bad
        with pytest.raises(_native.GolError) as ei:
            e.read_window(x, y, w, h)
        assert ei.value.code == _native.GOL_EINVAL
        with pytest.raises(_native.GolError) as ei:
            e.window_density(x, y, w, h, 4)
        assert ei.value.code == _native.GOL_EINVAL
        buf = np.zeros((max(h, 1), max(w, 1)), np.uint8)
        rc = _native.lib().gol_write_window(e.handle, x, y, w, h,
                                            buf.ctypes.data_as(_native._u8p))
        assert rc == _native.GOL_EINVAL
        for block in (0, 4097):
            with pytest.raises(_native.GolError) as ei:
                e.window_density(0, 0, 8, 8, block)
            assert ei.value.code == _native.GOL_EINVAL
        assert np.array_equal(e.read_packed(), start)      # the engine untouched
        assert e.turn == 0


# ------------------------------------------------------------------ 2. narrow boards
@pytest.mark.parametrize("W,H,turns,seed", [(200, 77, 3, 3), (16, 16, 2, 12), (2, 1, 0, 1),
                                            (64, 1, 0, 14)])
def test_narrow_and_degenerate_boards(gol, oracle, W, H, turns, seed):
    """One-turn engines in the standard layout; rows of less than one word, of one word, of one
    cell row: a window as wide as the board and windows wrapping x (and y)."""
    start = oracle.gen_random(seed, W, H)
    want_packed = oracle.bit_run(start, W, turns) if turns else start
    want_board = oracle.unpack(want_packed, W)
    rng = np.random.default_rng(seed)
    with gol.Engine(W, H, device=0) as e:
        assert e.info().turns_per_launch == 1
        e.load_packed(start)
        e.step(turns)
        assert e.board_layout() == 0
        wins = [(0, 0, W, H), (W // 2, 0, W, H), (W - 1, H - 1, W, H), (W - 1, 0, 2, 1)]
        for (x, y, w, h) in wins:
            got, t = e.read_window(x, y, w, h)
            want = _win(want_board, x, y, w, h)
            _both(want, (W, H, x, y, w, h))
            assert t == turns and np.array_equal(got, want), (W, H, x, y, w, h)
            d, _ = e.window_density(x, y, w, h, 1)
            assert np.array_equal(d, want // 255)
            d, _ = e.window_density(x, y, w, h, max(w, h))
            assert d.shape == (1, 1) and int(d[0, 0]) == int((want == 255).sum())
        # a write on the same shapes: the window's two ends meet in one word
        exp = want_board.copy()
        for (x, y, w, h) in wins[1:]:
            patch = rng.choice(np.array([0, 255], np.uint8), size=(h, w))
            exp[np.ix_((y + np.arange(h)) % H, (x + np.arange(w)) % W)] = patch
            e.write_window(x, y, patch)
            assert np.array_equal(e.read_packed(), oracle.pack(exp)[0]), (W, H, x, y, w, h)
            assert e.snapshot() == (turns, int((exp == 255).sum()))


# ------------------------------------------------------------------ 3. density
def _block_sums(win, block):
    a = (win == 255).astype(np.int64)
    h, w = a.shape
    a = np.add.reduceat(a, np.arange(0, h, block), axis=0)
    return np.add.reduceat(a, np.arange(0, w, block), axis=1)


@pytest.mark.parametrize("layout", [0, 1], ids=["standard", "interleaved"])
@pytest.mark.parametrize("W", BOARDS)
def test_window_density(gol, oracle, monkeypatch, W, layout):
    start, b8, _ = _boards(oracle, W)
    packed, turn = (b8, K) if layout else (start, 0)
    board = oracle.unpack(packed, W)
    with _engine(gol, monkeypatch, W) as e:
        e.load_packed(start)
        if layout:
            e.step(K)
        assert e.board_layout() == layout
        for (x, y, w, h) in _windows(W, BH):
            want = _win(board, x, y, w, h)
            _both(want)
            for block in (1, 3, 64, 100, max(w, h)):
                got, t = e.window_density(x, y, w, h, block)
                ws = _block_sums(want, block)
                assert t == turn and got.dtype == np.uint32 and got.shape == ws.shape
                assert np.array_equal(got.astype(np.int64), ws), (W, layout, x, y, w, h, block)
            one, _ = e.window_density(x, y, w, h, 1)
            rd, _ = e.read_window(x, y, w, h)
            assert np.array_equal(one, rd // 255)
        whole, _ = e.window_density(0, 0, W, BH, W)       # one block over the whole torus
        assert whole.shape == (1, 1)
        assert (turn, int(whole[0, 0])) == e.snapshot() == (turn, oracle.popcount(packed, W))
        assert e.board_layout() == layout


# ------------------------------------------------------------------ 4. write
def _patch(rng, h, w):
    """(bytes to write, the bytes they mean): 255 = alive, every other value dead."""
    raw = rng.choice(np.array([0, 255, 255, 0, 7, 254], np.uint8), size=(h, w))
    return raw, np.where(raw == 255, 255, 0).astype(np.uint8)


@pytest.mark.parametrize("layout", [0, 1], ids=["standard", "interleaved"])
@pytest.mark.parametrize("W", BOARDS)
def test_write_window(gol, oracle, monkeypatch, W, layout):
    start, b8, _ = _boards(oracle, W)
    packed, turn = (b8, K) if layout else (start, 0)
    board = oracle.unpack(packed, W)
    rng = np.random.default_rng(100 * W + layout)
    with _engine(gol, monkeypatch, W) as e:
        for (x, y, w, h) in _windows(W, BH) + _corners(W, BH):
            e.load_packed(start)
            if layout:
                e.step(K)
            assert e.board_layout() == layout
            launches = e.info().launches
            raw, cells = _patch(rng, h, w)
            if w * h > 1:
                _both(cells)
                assert not np.array_equal(cells, _win(board, x, y, w, h))
            else:
                raw = cells = 255 - _win(board, x, y, 1, 1)  # (flip the corner cell)
            exp = board.copy()
            exp[np.ix_((y + np.arange(h)) % BH, (x + np.arange(w)) % W)] = cells
            exp_packed = oracle.pack(exp)[0]
            e.write_window(x, y, raw)
            assert e.board_layout() == layout
            assert e.turn == turn and e.info().launches == launches
            assert e.snapshot() == (turn, oracle.popcount(exp_packed, W))
            back, _ = e.read_window(x, y, w, h)
            assert np.array_equal(back, cells)
            got = e.read_packed()
            assert np.array_equal(got, exp_packed), (W, layout, x, y, w, h)
            # every bit of every word: the padding past `width` is zero
            assert int(np.unpackbits(got.view(np.uint8)).sum()) == oracle.popcount(exp_packed, W)
            if layout:                                      # written in the interleaved layout,
                e.load_packed(start)                        # then stepped from it
                e.step(K)
                e.write_window(x, y, raw)
                assert e.board_layout() == 1
            e.step(K + 1)
            assert e.turn == turn + K + 1
            assert np.array_equal(e.read_packed(), oracle.bit_run(exp_packed, W, K + 1))


def test_write_invalidates_the_flip_list(gol, oracle):
    W = 1000
    start = oracle.gen_random(5, W, BH)
    with gol.Engine(W, BH, device=0) as e:
        e.load_packed(start)
        e.step(1)
        assert len(e.flipped_cells()) > 0
        e.write_window(10, 10, np.full((3, 3), 255, np.uint8))
        with pytest.raises(_native.GolError) as ei:
            e.flipped_cells()
        assert ei.value.code == _native.GOL_ESTATE
        e.step(1)
        e.flipped_cells()


def test_nonbinary_turn0_board(gol, oracle):
    """A non-binary load: write_window is refused while the engine holds the raw turn-0 bytes,
    and read_window returns those bytes' window."""
    W = 1000
    rng = np.random.default_rng(9)
    board = rng.choice(np.array([0, 255, 255, 0, 1, 128, 254], np.uint8), size=(BH, W))
    with gol.Engine(W, BH, device=0) as e:
        e.load(board)
        assert e.info().nonbinary_cells > 0
        with pytest.raises(_native.GolError) as ei:
            e.write_window(0, 0, np.zeros((2, 2), np.uint8))
        assert ei.value.code == _native.GOL_ESTATE
        for (x, y, w, h) in _windows(W, BH):
            got, t = e.read_window(x, y, w, h)
            assert t == 0 and np.array_equal(got, _win(board, x, y, w, h)), (x, y, w, h)
        assert np.array_equal(e.read_board(), board)
        e.step(1)
        e.write_window(0, 0, np.zeros((2, 2), np.uint8))   # (turn 1: an ordinary board)


# ------------------------------------------------------------------ 5. clear then stamp
def test_clear_then_stamp(gol, monkeypatch):
    W = 1000
    glider = np.array([[0, 255, 0], [0, 0, 255], [255, 255, 255]], np.uint8)
    with _engine(gol, monkeypatch, W) as e:
        e.fill_random(3)
        e.step(3)
        assert e.snapshot()[1] > 0
        e.clear()
        assert e.snapshot() == (0, 0)
        assert e.board_layout() == 0 and e.turn == 0
        e.write_window(W - 2, BH - 2, glider)              # across both wraps
        assert e.snapshot() == (0, 5)
        e.step(4)
        got, t = e.read_window(W - 1, BH - 1, 3, 3)
        assert t == 4 and np.array_equal(got, glider)      # moved by (1, 1)
        assert e.snapshot() == (4, 5)


# ------------------------------------------------------------------ 6. strips
def test_windows_on_strips(gol, oracle, monkeypatch):
    """Three strips of 53 / 52 / 52 rows of a 1000 x 157 board with 11-row halos."""
    W, H, n, halo = 1000, 157, 3, 11
    _pin_tile(monkeypatch, 13, 108)
    start, (b11,) = _oracle_run(oracle, 108 + 157, W, H, (halo,))
    board = oracle.unpack(b11, W)
    rng = np.random.default_rng(6)
    with _Strips(gol, start, W, n, halo, band_rows=19, turns_per_launch=K) as s:
        s.step(halo)
        for e, (o, r) in zip(s.engs, s.parts):
            assert e.board_layout() == 1
            for (x, y, w, h) in ((0, o, W, r), (W - 20, o + 2, 50, r - 4), (o, o + r - 1, 65, 1)):
                got, t = e.read_window(x, y, w, h)
                want = _win(board, x, y, w, h)
                _both(want)
                assert t == halo and np.array_equal(got, want), (o, x, y, w, h)
                d, _ = e.window_density(x, y, w, h, 7)
                assert np.array_equal(d.astype(np.int64), _block_sums(want, 7))
            # a window that reaches a halo row, above or below the owned rows
            for (y, h) in ((o + r - 3, 4), ((o - 1) % H, 2)):
                with pytest.raises(_native.GolError) as ei:
                    e.read_window(0, y, 8, h)
                assert ei.value.code == _native.GOL_EINVAL
                with pytest.raises(_native.GolError) as ei:
                    e.window_density(0, y, 8, h, 2)
                assert ei.value.code == _native.GOL_EINVAL
        # one write across the boundary of strips 0 and 1 (rows 45 .. 64) and the x wrap, one
        # across the y wrap (rows 150 .. 156, 0 .. 6): strip 2 holds none of the first window's
        # rows, every strip's halo rows hold some of one of them
        s.exchange()
        exp = board.copy()
        for (x, y, w, h) in ((W - 15, 45, 30, 20), (300, 150, 100, 14)):
            raw, cells = _patch(rng, h, w)
            exp[np.ix_((y + np.arange(h)) % H, (x + np.arange(w)) % W)] = cells
            for e in s.engs:
                e.write_window(x, y, raw)
                assert e.turn == halo and e.halo_valid == halo
        exp_packed = oracle.pack(exp)[0]
        assert not np.array_equal(exp_packed, b11)
        assert np.array_equal(s.read(), exp_packed)
        s.step(halo)                                       # (no exchange first: the halos are fresh)
        assert np.array_equal(s.read(), oracle.bit_run(exp_packed, W, halo))


def test_write_reaches_both_copies_of_a_row(gol, oracle):
    """One strip engine that owns every row and has halos: its buffer holds global rows
    66 .. 76, 0 .. 76, 0 .. 10, so rows 70 .. 76 and 0 .. 4 are there twice.  Stepping `halo`
    turns from the halo copies gives the oracle's board only if both copies were written."""
    W, halo = 1000, 11
    start = oracle.gen_random(8, W, BH)
    rng = np.random.default_rng(8)
    with gol.Engine(W, BH, device=0, row_offset=0, rows=BH, halo=halo) as e:
        idx = np.arange(-halo, BH + halo) % BH
        e.load_packed(np.ascontiguousarray(start[idx]))
        raw, cells = _patch(rng, 12, 200)
        exp = oracle.unpack(start, W)
        exp[np.ix_((70 + np.arange(12)) % BH, (900 + np.arange(200)) % W)] = cells
        exp_packed = oracle.pack(exp)[0]
        e.write_window(900, 70, raw)
        assert np.array_equal(e.read_packed(), exp_packed)
        e.step(halo)
        assert np.array_equal(e.read_packed(), oracle.bit_run(exp_packed, W, halo))


# ------------------------------------------------------------------ 7. staging chunks
_CHILD = r"""
import sys
sys.path[:0] = [sys.argv[1], sys.argv[2], sys.argv[3]]
import numpy as np
import gol
from gol import _native as N
from oracle import oracle as O

assert N.LIB_PATH.endswith("libgolamd_stage64k.so"), N.LIB_PATH

def win(board, x, y, w, h):
    H, W = board.shape
    return board[np.ix_((y + np.arange(h)) % H, (x + np.arange(w)) % W)]

W, H = 1000, 333
start = O.gen_random(77, W, H)
b8 = O.bit_run(start, W, 8)
board = O.unpack(b8, W)
with gol.Engine(W, H, device=0, autotune=False) as e:
    e.load_packed(start)
    e.step(8)
    lay = e.board_layout()
    # 300 x 300 bytes = 90 000: two chunks of 218 and 82 rows, across both wraps
    got, t = e.read_window(900, 200, 300, 300)
    want = win(board, 900, 200, 300, 300)
    assert (want == 255).any() and (want == 0).any()
    assert t == 8 and np.array_equal(got, want)
    print("OK read")
    # 300 x 300 counts = 360 000 bytes: six chunks of 54 block rows
    d, t = e.window_density(900, 200, 300, 300, 1)
    assert t == 8 and np.array_equal(d, want // 255)
    d, t = e.window_density(900, 200, 300, 300, 7)
    a = (want == 255).astype(np.int64)
    a = np.add.reduceat(np.add.reduceat(a, np.arange(0, 300, 7), axis=0), np.arange(0, 300, 7), axis=1)
    assert np.array_equal(d.astype(np.int64), a)
    assert e.board_layout() == lay
    print("OK density")
    # 1000 x 77 bytes = 77 000: two chunks of 65 and 12 rows, across the y wrap
    rng = np.random.default_rng(7)
    raw = rng.choice(np.array([0, 255, 255, 0, 9], np.uint8), size=(77, W))
    exp = board.copy()
    exp[np.ix_((300 + np.arange(77)) % H, (500 + np.arange(W)) % W)] = np.where(raw == 255, 255, 0)
    e.write_window(500, 300, raw)
    assert e.board_layout() == lay and e.turn == 8
    assert np.array_equal(e.read_packed(), O.pack(exp)[0])
    print("OK write")
"""


def test_chunked_staging():
    """libgolamd_stage64k.so (64 KiB staging chunks): a read, a density and a write that take
    several chunks.  In a child process (the test library is a second copy of the engine)."""
    assert os.path.exists(STAGE_LIB), "build it: make -C conway-s-gol-distributed_amd/csrc smallstage"
    env = dict(os.environ, GOL_AMD_LIB=STAGE_LIB)
    r = subprocess.run([sys.executable, "-c", _CHILD, os.path.join(ROOT, "tests"),
                        os.path.join(ROOT, "conway-s-gol-distributed_amd"), ROOT],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert [l for l in lines if l.startswith("OK")] == ["OK read", "OK density", "OK write"]


# ------------------------------------------------------------------ 8. from another thread
def test_read_window_from_another_thread(gol, oracle):
    """read_window from a second thread while step(4000) runs on 512^2: served at a launch
    boundary, the bytes are the oracle's board at the turn the call returns."""
    W = H = 512
    total = 4000
    start = oracle.gen_random(41, W, H)
    with gol.Engine(W, H, device=0) as e:
        e.load_packed(start)
        res = {}

        def reader():
            end = time.monotonic() + 10
            while e.progress()[0] == 0 and time.monotonic() < end:
                pass
            res["win"] = e.read_window(400, 450, 200, 100)
            res["dens"] = e.window_density(400, 450, 200, 100, 50)

        th = threading.Thread(target=reader, daemon=True)
        th.start()
        e.step(total)
        th.join(20)
        assert not th.is_alive()
        assert e.turn == total
        for key in ("win", "dens"):
            got, t = res[key]
            assert 0 <= t <= total
            want = _win(oracle.unpack(oracle.bit_run(start, W, t), W), 400, 450, 200, 100)
            _both(want)
            if key == "win":
                assert np.array_equal(got, want), t
            else:
                assert np.array_equal(got.astype(np.int64), _block_sums(want, 50)), t
        print("served at turns", res["win"][1], res["dens"][1])


# ------------------------------------------------------------------ 9. the real size
def test_real_board_windows(gol, oracle, monkeypatch):
    """test_gpu_big.py's board (131072 x 262400, 4.3 GB per buffer) without a host board: clear,
    four write_window calls of its 64 x 64 soups (across byte offsets 2^31 and 2^32 of the
    buffer, the y wrap and the x wrap), step(20) on the pinned big-form shape, then a 256 x 256
    read_window round each soup against the soup's own 256^2 torus run (PAD dead cells round a
    soup outlast the turns run, as in that file), and the whole board's density in blocks of
    4096.  The largest host array here is the density's 65 x 32 counts."""
    monkeypatch.setenv("GOL_TILE", "30,516")
    turns, block = 20, 4096
    nby, nbx = -(-BIG_H // block), BIG_W // block
    want_d = np.zeros((nby, nbx), np.int64)
    with gol.Engine(BIG_W, BIG_H, device=0, band_rows=472, turns_per_launch=turns,
                    autotune=False) as e:
        e.clear()
        wants = []
        for i, (x0, y0) in enumerate(SOUPS):
            soup = oracle.unpack(oracle.gen_random(100 + i, SOUP, SOUP), SOUP)
            _both(soup)
            e.write_window(x0, y0, soup)
            small = np.zeros((TORUS, TORUS), np.uint8)
            small[PAD:PAD + SOUP, PAD:PAD + SOUP] = soup
            after = oracle.unpack(oracle.bit_run(oracle.pack(small)[0], TORUS, turns), TORUS)
            _both(after)
            assert not after[0].any() and not after[-1].any()      # (it stayed inside its torus)
            assert not after[:, 0].any() and not after[:, -1].any()
            wants.append(after)
            ys, xs = np.nonzero(after)
            np.add.at(want_d, (((y0 - PAD + ys) % BIG_H) // block, ((x0 - PAD + xs) % BIG_W) // block), 1)
        assert e.snapshot() == (0, sum(int((oracle.unpack(oracle.gen_random(100 + i, SOUP, SOUP),
                                                           SOUP) == 255).sum()) for i in range(4)))
        e.step(turns)
        assert [(k, v) for k, v, _ in e.last_launches()] == [(turns, 15)]
        assert {(a, b) for a, b, _ in e.last_launch_tiles()} == {(30, 516)}
        assert e.board_layout() == 1
        for (x0, y0), after in zip(SOUPS, wants):
            got, t = e.read_window((x0 - PAD) % BIG_W, (y0 - PAD) % BIG_H, TORUS, TORUS)
            assert t == turns and np.array_equal(got, after), (x0, y0)
        dens, t = e.window_density(0, 0, BIG_W, BIG_H, block)
        assert t == turns and dens.shape == (nby, nbx)
        assert e.board_layout() == 1
        assert (turns, int(dens.sum())) == e.snapshot()
        assert int(dens.sum()) == int(want_d.sum()) > 0
        assert np.array_equal(dens.astype(np.int64), want_d)
