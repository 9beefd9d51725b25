"""gol_flipped_cells / Engine.flipped_cells (K5: k_row_flipcount, k_row_scan, k_flip_scatter)
and the run driver's CellFlipped stream that is built on it.

Bit-exact.  Every expected list comes from the oracle on the host: prev = board,
cur = oracle.np_step(prev), want = argwhere((prev == 255) != (cur == 255)) in row-major order
as (x, y).  Every parity case asserts a non-empty list, so a call that always reports nothing
cannot pass.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import golden_data as G
import io_boards as B

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGE_LIB = os.path.join(ROOT, "conway-s-gol-distributed_amd", "build", "libgolamd_stage64k.so")


@pytest.fixture(scope="module")
def gol():
    import gol as g
    return g


def want_flips(prev, cur, row_offset=0):
    """Row-major (n, 2) int64 {x, y} of the cells whose packed bit (byte == 255) differs."""
    yx = np.argwhere((np.asarray(prev) == 255) != (np.asarray(cur) == 255))
    out = yx[:, ::-1].astype(np.int64)
    out[:, 1] += row_offset
    return np.ascontiguousarray(out)


def random_board(oracle, w, h, seed=None):
    return oracle.unpack(oracle.gen_random(w + h if seed is None else seed, w, h), w)


def flips_capped(e, cap, canary=-7777, slack=8):
    """gol_flipped_cells through the raw ABI into a canary-filled array `slack` pairs longer
    than `cap`.  Returns (rc, total, the whole array)."""
    from gol import _native as N
    buf = np.full((cap + slack, 2), canary, dtype=np.int64)
    n = ctypes.c_int64(-1)
    rc = N.lib().gol_flipped_cells(e.handle, buf.ctypes.data_as(N._i64p), int(cap),
                                   ctypes.byref(n))
    return rc, int(n.value), buf


def assert_estate(gol, e):
    from gol import _native as N
    with pytest.raises(N.GolError) as ei:
        e.flipped_cells()
    assert ei.value.code == N.GOL_ESTATE, ei.value
    assert b"gol_flipped_cells" in N.lib().gol_last_error(e.handle)


# ------------------------------------------------------------ 1. parity per shape
# 16x16: generic stencil, one word.  70x5: a partial last word (no padding bit may be
# reported) and 5 rows = one full block of 4 rows + 1.  130x3: three words, partial last.
# 64x1, 64x2: degenerate torus heights.  256x8: the smallest fast-path width.  8330x6: 131
# words > 64 lanes, so the scatter's second pass with a carried base, plus a partial word.
# 512x512: a full-size fixture board.  (k_row_scan's second slice: test_scan_past_one_slice.)
SHAPES = [(16, 16), (70, 5), (130, 3), (64, 1), (64, 2), (256, 8), (8330, 6), (512, 512)]


@pytest.mark.parametrize("w,h", SHAPES)
def test_parity(gol, oracle, w, h):
    board = G.input_board(512) if (w, h) == (512, 512) else random_board(oracle, w, h)
    assert board.shape == (h, w)
    with gol.Engine(w, h, device=0) as e:
        e.load(board)
        acc = board == 255                       # XOR-accumulated from the turn-0 board
        prev = board
        for turn in range(1, 5):
            cur = oracle.np_step(prev)
            e.step(1)
            got = e.flipped_cells()
            want = want_flips(prev, cur)
            assert len(want) > 0, (w, h, turn)
            assert got.dtype == np.int64 and got.shape == want.shape, (turn, got.shape, want.shape)
            assert np.array_equal(got, want), (w, h, turn)
            assert got[:, 0].max() < w and got[:, 1].max() < h     # no padding bit, no halo row
            acc[got[:, 1], got[:, 0]] ^= True
            assert np.array_equal(acc, e.read_board() == 255), (w, h, turn)
            prev = cur


def test_scan_past_one_slice(gol, oracle):
    """2500 rows: k_row_scan's workgroup takes three slices of 1024 rows, the last one partial,
    and carries the running total between them."""
    w, h = 64, 2500
    board = random_board(oracle, w, h)
    with gol.Engine(w, h, device=0) as e:
        e.load(board)
        e.step(1)
        want = want_flips(board, oracle.np_step(board))
        assert len(want) > 0 and want[:, 1].max() > 2048
        assert np.array_equal(e.flipped_cells(), want)


# ------------------------------------------------------------ 2. strips
def test_strips_match_torus(gol, oracle):
    """256 x 64 as 3 strip engines with halo 2, 5 turns: the concatenated lists equal the torus
    engine's and the oracle's, with global y."""
    w, h, K = 256, 64, 2
    board = random_board(oracle, w, h)
    split = gol.strip_split(h, 3)
    engs = [gol.Engine(w, h, device=0, row_offset=o, rows=r, halo=K) for o, r in split]
    torus = gol.Engine(w, h, device=0)
    try:
        for e, (o, r) in zip(engs, split):
            e.load(gol.haloed_rows(board, o, r, K))
        torus.load(board)
        prev = board
        for turn in range(1, 6):
            if engs[0].halo_valid == 0:
                for i, e in enumerate(engs):
                    e.copy_halo_from_upper(engs[(i - 1) % 3])
                    e.copy_halo_from_lower(engs[(i + 1) % 3])
                for e in engs:
                    e.halo_done()
            for e in engs:
                e.step(1)
            torus.step(1)
            cur = oracle.np_step(prev)
            want = want_flips(prev, cur)
            assert len(want) > 0
            parts = [e.flipped_cells() for e in engs]
            for p, (o, r) in zip(parts, split):
                assert len(p) == 0 or (p[:, 1].min() >= o and p[:, 1].max() < o + r), turn
            got = np.concatenate(parts)
            assert np.array_equal(got, want), turn
            assert np.array_equal(torus.flipped_cells(), want), turn
            prev = cur
    finally:
        for e in engs + [torus]:
            e.close()


# ------------------------------------------------------------ 3. layout
def test_after_multi_turn_launch(gol, oracle):
    """512 x 512, turns_per_launch 8: step(8) may leave the board in the interleaved layout;
    the step(1) after it converts back, and the list has standard x."""
    board = G.input_board(512)
    with gol.Engine(512, 512, device=0, turns_per_launch=8) as e:
        e.load(board)
        e.step(8)
        assert_estate(gol, e)
        e.step(1)
        prev = oracle.np_run(board, 8)
        want = want_flips(prev, oracle.np_step(prev))
        assert len(want) > 0
        assert np.array_equal(e.flipped_cells(), want)


# ------------------------------------------------------------ 4. cap
def test_cap(gol, oracle):
    from gol import _native as N
    board = random_board(oracle, 130, 3)
    want = want_flips(board, oracle.np_step(board))
    assert len(want) > 10
    with gol.Engine(130, 3, device=0) as e:
        e.load(board)
        e.step(1)
        rc, n, buf = flips_capped(e, 0)
        assert (rc, n) == (N.GOL_OK, len(want)) and (buf == -7777).all()
        for cap in (1, 7, len(want) - 1):
            rc, n, buf = flips_capped(e, cap)
            assert (rc, n) == (N.GOL_OK, len(want)), cap
            assert np.array_equal(buf[:cap], want[:cap]), cap
            assert (buf[cap:] == -7777).all(), cap
        rc, n, buf = flips_capped(e, len(want) + 5)
        assert (rc, n) == (N.GOL_OK, len(want))
        assert np.array_equal(buf[:n], want) and (buf[n:] == -7777).all()


def test_still_life_is_empty(gol):
    from gol import _native as N
    board = np.zeros((16, 16), dtype=np.uint8)
    board[4:6, 7:9] = 255                                  # a 2 x 2 block
    with gol.Engine(16, 16, device=0) as e:
        e.load(board)
        e.step(1)
        assert np.array_equal(e.read_board(), board)
        rc, n, buf = flips_capped(e, 4)
        assert (rc, n) == (N.GOL_OK, 0) and (buf == -7777).all()
        assert e.flipped_cells().shape == (0, 2)


# ------------------------------------------------------------ 5. state
def test_state(gol, oracle):
    board = random_board(oracle, 70, 5)
    with gol.Engine(70, 5, device=0) as e:
        e.load(board)
        assert_estate(gol, e)                               # a load, no step yet
        e.step(1)
        want1 = want_flips(board, oracle.np_step(board))
        assert len(want1) > 0 and np.array_equal(e.flipped_cells(), want1)
        e.step(0)                                           # no launch: still valid
        assert np.array_equal(e.flipped_cells(), want1)
        e.step(2)
        assert_estate(gol, e)
        e.step(1)                                           # valid again
        b3 = oracle.np_run(board, 3)
        want4 = want_flips(b3, oracle.np_step(b3))
        assert len(want4) > 0 and np.array_equal(e.flipped_cells(), want4)
        e.fill_random(5)
        assert_estate(gol, e)
        e.step(1)
        r = oracle.unpack(oracle.gen_random(5, 70, 5), 70)
        wantr = want_flips(r, oracle.np_step(r))
        assert len(wantr) > 0 and np.array_equal(e.flipped_cells(), wantr)
        e.load_packed(oracle.pack(board)[0])
        assert_estate(gol, e)


def test_state_halo_buffers_conversion(gol, oracle):
    """A strip engine whose stepping layout is interleaved: gol_halo_buffers converts the board
    into the other half of the double buffer, so the previous board is gone."""
    w, h, K = 1536, 300, 16
    with gol.Engine(w, h, device=0, row_offset=0, rows=h, halo=K, turns_per_launch=8) as e:
        e.fill_random(11)
        e.step(1)
        r = oracle.unpack(oracle.gen_random(11, w, h), w)
        cur = oracle.np_step(r)
        want = want_flips(r, cur)
        assert len(want) > 0 and np.array_equal(e.flipped_cells(), want)
        _, layout = e.halo_buffers()
        if layout != 1:
            pytest.skip("no interleaved stepping layout at this size")
        assert_estate(gol, e)
        e.step(1)                                           # back in the standard layout
        want = want_flips(cur, oracle.np_step(cur))
        assert len(want) > 0 and np.array_equal(e.flipped_cells(), want)


# ------------------------------------------------------------ 6. per-turn counts
def test_count_every_turn_unaffected(gol, oracle):
    board = random_board(oracle, 256, 8)
    with gol.Engine(256, 8, device=0, count_every_turn=True) as e:
        e.load(board)
        prev, counts = board, []
        for _ in range(6):
            cur = oracle.np_step(prev)
            e.step(1)
            want = want_flips(prev, cur)
            assert len(want) > 0 and np.array_equal(e.flipped_cells(), want)
            counts.append(int((cur == 255).sum()))
            prev = cur
        assert e.turn_counts(1, 6).tolist() == counts


# ------------------------------------------------------------ 7. non-binary input
def test_nonbinary_first_turn_is_the_bit_xor(gol, oracle):
    """A flip is a change of the packed bit (bit = byte == 255): a non-binary cell is 0 before
    and dead after the first turn, so it is not listed (include/gol_amd.h)."""
    board = B.nonbinary_board(100, 30)
    assert ((board != 0) & (board != 255)).any()
    cur = oracle.np_step(board)
    assert np.array_equal(cur, oracle.ref_run(board, 1, nsub=3, threads=2))
    want = want_flips(board, cur)
    assert 0 < len(want) < int((board != cur).sum())       # fewer than the byte changes
    with gol.Engine(100, 30, device=0) as e:
        e.load(board)
        e.step(1)
        assert np.array_equal(e.flipped_cells(), want)
        e.step(1)
        want2 = want_flips(cur, oracle.np_step(cur))
        assert len(want2) > 0 and np.array_equal(e.flipped_cells(), want2)


# ------------------------------------------------------------ 8. chunked staging
_CHILD = r"""
import ctypes, sys
sys.path[:0] = [sys.argv[1], sys.argv[2], sys.argv[3]]
import numpy as np
import gol
from gol import _native as N
from oracle import oracle as O

assert N.LIB_PATH.endswith("libgolamd_stage64k.so"), N.LIB_PATH
CHUNK = 65536 // 16           # flips per staging chunk

def want_flips(prev, cur):
    yx = np.argwhere((prev == 255) != (cur == 255))
    return np.ascontiguousarray(yx[:, ::-1].astype(np.int64))

def capped(e, cap):
    buf = np.full((cap + 8, 2), -7777, dtype=np.int64)
    n = ctypes.c_int64(-1)
    N.check(N.lib().gol_flipped_cells(e.handle, buf.ctypes.data_as(N._i64p), cap,
                                      ctypes.byref(n)), e.handle)
    return int(n.value), buf

# 8330 x 40 random: ~4000 flips per row, about one staging chunk each, ~40 chunks in all
w, h = 8330, 40
board = O.unpack(O.gen_random(w + h, w, h), w)
cur = O.np_step(board)
want = want_flips(board, cur)
assert len(want) > 4 * CHUNK, len(want)
per_row = np.bincount(want[:, 1], minlength=h)
with gol.Engine(w, h, device=0, autotune=False) as e:
    e.load(board)
    e.step(1)
    got = e.flipped_cells()
    assert got.shape == want.shape and np.array_equal(got, want), "full list"
    print("OK full", len(want))
    # caps inside the first chunk (row 0), at a chunk's size, inside the second chunk (row 1)
    # and a later one
    first = int(per_row[0])
    assert first <= CHUNK < first + per_row[1], per_row[:2]
    for cap in sorted({1, CHUNK - 1, CHUNK, first + 17, first + CHUNK // 2, 3 * CHUNK + 1,
                       len(want) - 1}):
        n, buf = capped(e, cap)
        assert n == len(want), (cap, n)
        assert np.array_equal(buf[:cap], want[:cap]), (cap, "head")
        assert (buf[cap:] == -7777).all(), (cap, "wrote past cap")
    print("OK caps")
    assert np.array_equal(e.read_board(), cur)              # the board is untouched

# one row larger than a chunk: the rows above and below a full 8320-cell row are born whole
# (8320 flips each > 4096), after rows that hold a few flips
w, h = 8320, 12
board = np.zeros((h, w), dtype=np.uint8)
board[5] = 255
board[1, 10:13] = 255                                       # a blinker
cur = O.np_step(board)
want = want_flips(board, cur)
per_row = np.bincount(want[:, 1], minlength=h)
assert per_row.max() > CHUNK and len(want) > per_row.max(), per_row
with gol.Engine(w, h, device=0, autotune=False) as e:
    e.load(board)
    e.step(1)
    got = e.flipped_cells()
    assert got.shape == want.shape and np.array_equal(got, want), "big row"
    cap = int(per_row[:4].sum()) + CHUNK + 3                # ends inside the first big row
    n, buf = capped(e, cap)
    assert n == len(want) and np.array_equal(buf[:cap], want[:cap]) and (buf[cap:] == -7777).all()
print("OK big row")
"""


def test_chunked_staging():
    """libgolamd_stage64k.so (64 KiB staging chunks): a list of several chunks takes the row
    chunk path -- offsets rebased per chunk, caps that end inside a chunk, a single row larger
    than a chunk.  In a child process (the test library is a second copy of the engine), which
    ends at its first failure."""
    assert os.path.exists(STAGE_LIB), "build it: make -C conway-s-gol-distributed_amd/csrc smallstage"
    env = dict(os.environ, GOL_AMD_LIB=STAGE_LIB)
    r = subprocess.run([sys.executable, "-c", _CHILD, os.path.join(ROOT, "tests"),
                        os.path.join(ROOT, "conway-s-gol-distributed_amd"), ROOT],
                       capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert any(l.startswith("OK full") for l in lines), r.stdout
    assert "OK caps" in lines and "OK big row" in lines, r.stdout


# ------------------------------------------------------------ 9. run driver
def _pgm(board):
    h, w = board.shape
    return b"P5\n%d %d\n255\n" % (w, h) + np.ascontiguousarray(board, dtype=np.uint8).tobytes()


def _run_events(gol, tmp_path, w, h, turns, **kw):
    """(type, turn, x, y) of the CellFlipped and TurnComplete events of one run, in order."""
    events = gol.Channel()
    hdl = gol.Run(gol.Params(Turns=turns, Threads=1, ImageWidth=w, ImageHeight=h), events, None,
                  image_dir=str(tmp_path / "images"), out_dir=str(tmp_path / "out"),
                  emit_cell_flipped=True, emit_turn_complete=True, **kw)
    evs = list(events)
    hdl.wait(5)
    assert hdl.error is None, hdl.error
    out = []
    for e in evs:
        if isinstance(e, gol.CellFlipped):
            out.append(("flip", e.CompletedTurns, e.Cell.X, e.Cell.Y))
        elif isinstance(e, gol.TurnComplete):
            out.append(("turn", e.CompletedTurns, -1, -1))
    return out


def _want_events(oracle, image, first, last, start=None):
    """Initial alive cells of `image` row-major, then for turns first..last the flips row-major
    before the turn's TurnComplete.  `start` (default: the image) is the board at turn
    first - 1; the first turn's flips are byte changes against the image (the driver starts
    from the image's bytes), the later ones changes of the board."""
    out = [("flip", 0, int(x), int(y)) for x, y in B.np_alive_cells(image)]
    shown = np.asarray(image)
    board = np.asarray(image if start is None else start)
    for t in range(first, last + 1):
        nxt = oracle.np_step(board)
        yx = np.argwhere(shown != nxt)
        out += [("flip", t, int(x), int(y)) for y, x in yx]
        out.append(("turn", t, -1, -1))
        shown = board = nxt
    return out


def _images(tmp_path, boards):
    img = tmp_path / "images"
    img.mkdir()
    for b in boards:
        (img / f"{b.shape[1]}x{b.shape[0]}.pgm").write_bytes(_pgm(b))


@pytest.mark.parametrize("case", ["16x16", "64x64-strips", "70x5", "nonbinary"])
def test_driver_event_stream(gol, oracle, tmp_path, case):
    kw = {}
    if case == "16x16":
        board = G.input_board(16)
    elif case == "64x64-strips":
        board = G.input_board(64)
        kw = dict(ngpus=4, devices=[0] * 4, halo=2)
    elif case == "70x5":
        board = random_board(oracle, 70, 5)
    else:
        board = B.nonbinary_board(100, 30)
        assert ((board != 0) & (board != 255)).any()
    _images(tmp_path, [board])
    h, w = board.shape
    got = _run_events(gol, tmp_path, w, h, 3, **kw)
    want = _want_events(oracle, board, 1, 3)
    assert sum(1 for e in want if e[0] == "flip" and e[1] > 0) > 0
    assert len(got) == len(want), (len(got), len(want))
    assert got == want


def test_driver_event_stream_resume(gol, oracle, tmp_path):
    """resume=1 after a plain run: the events start from the image, the board from the retained
    one, so the first turn's flips are the image against turn 3 (the kept host comparison)."""
    board = G.input_board(16)
    _images(tmp_path, [board])
    events = gol.Channel()
    hdl = gol.Run(gol.Params(Turns=2, Threads=1, ImageWidth=16, ImageHeight=16), events, None,
                  image_dir=str(tmp_path / "images"), out_dir=str(tmp_path / "out"),
                  resume=False)
    list(events)
    hdl.wait(5)
    assert hdl.error is None, hdl.error
    got = _run_events(gol, tmp_path, 16, 16, 5, resume=True)
    want = _want_events(oracle, board, 3, 5, start=oracle.np_run(board, 2))
    assert sum(1 for e in want if e[0] == "flip" and e[1] > 0) > 0
    assert got == want
