"""The load, read-out and count paths around the stencils, at their edge shapes: k_pack /
k_unpack (K4), k_popcount (K2), k_row_popcount / k_alive_scatter (K3), k_il_convert, the
per-turn count ring and the host loops that feed them through the staging buffer -- what a
user sees as PGM in and out (Local/gol/io.go:42-143), AliveCellsCount
(Server/gol/distributor.go:173-183) and FinalTurnComplete.Alive
(Local/gol/distributor.go:229-239).

Bit-exact throughout.  No expected value comes from the engine: packed boards are
oracle.pack, stepped boards oracle.bit_run / ref_run, alive lists the numpy restatement in
io_boards.py (cross-checked against oracle.ref_alive_cells on the CPU, tests/test_oracle.py::
test_structured_boards_alive_list_and_pack).
"""
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


def _stepped(oracle, board, turns):
    """`board` (0 / 255 bytes) after `turns` turns, by the bit oracle."""
    w = board.shape[1]
    return oracle.unpack(oracle.bit_run(oracle.pack(board)[0], w, turns), w)


# ------------------------------------------------------------ 1. round trip and read-outs
# The smallest widths at which each path changes: one partial word; 63 / 64 / 65 around one
# word; 80 = 16-byte rows with a partial only word; 100 and 208 = scalar and mixed
# vector / scalar rows of 2 and 4 words; 4096 = 64 words (one k_alive_scatter pass); 4112 = 64
# full words + a 16-bit tail (k_pack / k_unpack take the uint4 path for the full words and
# the scalar path for the last word of the same row); 4160 = 65 words and 8320 = 130 words
# (second and third scatter pass).  Heights are no multiples of 4 (k_row_popcount and the
# scatter run 4 rows per block): a partial block alone, and 8 full blocks + 1 row.
WIDTHS = (2, 63, 64, 65, 80, 100, 208, 4096, 4112, 4160, 8320)
HEIGHTS = (1, 3, 5, 33)
# every (width, board) pair once, the heights rotating so that every width meets each of them
ROUND_TRIP = [(name, w, HEIGHTS[(i + k) % 4])
              for i, w in enumerate(WIDTHS) for k, name in enumerate(B.MAKERS)]
# and the dense random board at every height of the widths past one scatter pass / one word
ROUND_TRIP += [("random50", w, h) for w in (100, 4160, 8320) for h in HEIGHTS
               if ("random50", w, h) not in ROUND_TRIP]
assert len(ROUND_TRIP) <= 120


@pytest.mark.parametrize("name,w,h", ROUND_TRIP)
def test_round_trip_and_readouts(gol, oracle, name, w, h):
    """load(bytes) and load_packed(words) of the same board, then one turn: read_packed,
    read_board, snapshot and alive_cells each time."""
    board = B.MAKERS[name](w, h)
    with gol.Engine(w, h, device=0, autotune=False) as e:
        e.load(board)
        assert e.info().nonbinary_cells == 0
        B.check_readouts(oracle, e, board, 0, tag="load")
        e.fill_random(1)                       # another board in between
        e.load_packed(oracle.pack(board)[0])
        B.check_readouts(oracle, e, board, 0, tag="load_packed")
        e.step(1)
        B.check_readouts(oracle, e, _stepped(oracle, board, 1), 1, tag="step")


# ------------------------------------------------------------ 2. truncated alive list
@pytest.mark.parametrize("name,w,h", [("random16", 4160, 5), ("alt_rows", 100, 33),
                                      ("last_bit", 65, 33), ("full", 80, 3),
                                      ("random50", 8320, 3), ("first_cell", 64, 1)])
def test_alive_cells_truncated(gol, name, w, h):
    """gol_alive_cells writes min(n, cap) pairs and sets *n to the total: cap in
    {1, n-1, n, n+5} with a canary behind the array."""
    board = B.MAKERS[name](w, h)
    n = int((board == 255).sum())
    with gol.Engine(w, h, device=0, autotune=False) as e:
        e.load(board)
        for cap in sorted({1, n - 1, n, n + 5} - {-1}):
            B.check_capped(e, board, cap, tag=name)


# ------------------------------------------------------------ 3. interleaved layout
@pytest.mark.parametrize("w,h,tpl,mv", [(2048, 300, 8, 7), (8320, 41, 8, 7), (1024, 96, 0, None)])
def test_readouts_on_interleaved_layout(gol, oracle, monkeypatch, w, h, tpl, mv):
    """read_board, alive_cells and snapshot after multi-turn launches (k_step_skew<IL> leaves
    the device board in the interleaved word layout; 1024 x 96 runs the default tile kernel):
    the reads convert, and do not disturb the run that goes on."""
    if mv is not None:
        monkeypatch.setenv("GOL_MULTI_VARIANT", str(mv))
    start = oracle.unpack(oracle.gen_random(w + h, w, h), w)
    with gol.Engine(w, h, device=0, turns_per_launch=tpl) as e:
        e.load(start)
        e.step(16)
        plan = e.last_launches()
        assert sum(k for k, _, _ in plan) == 16, plan
        if mv is not None:                     # multi-turn launches: interleaved when read
            assert all(k >= 2 for k, _, _ in plan), plan
        want = _stepped(oracle, start, 16)
        assert np.array_equal(e.read_board(), want)
        assert np.array_equal(e.alive_cells(), B.np_alive_cells(want))
        assert e.snapshot() == (16, int((want == 255).sum()))
        e.step(9)
        assert np.array_equal(e.read_packed(), oracle.pack(_stepped(oracle, want, 9))[0])


# ------------------------------------------------------------ 4. non-binary input
def _run_strips(engs, turns):
    """Advance in-process strip engines `turns` turns, exchanging halos when they run out."""
    n = len(engs)
    left = turns
    while left:
        if engs[0].halo_valid == 0:
            for i, e in enumerate(engs):
                e.copy_halo_from_upper(engs[(i - 1) % n])
                e.copy_halo_from_lower(engs[(i + 1) % n])
            for e in engs:
                e.halo_done()
        m = min(left, engs[0].halo_valid)
        for e in engs:
            e.step(m)
        left -= m


def test_nonbinary_strips(gol, oracle):
    """Bytes other than 0 / 255 on strip engines (n = 3, K = 2, 130 x 33): at turn 0 each
    strip returns its own raw rows; later the strips together are the reference's board.
    gol_info.nonbinary_cells of a strip counts the rows it LOADED, rows + 2 * halo: the owned
    rows and both halos (the halo rows' mask is needed for turn 1 as well)."""
    w, h, n, K = 130, 33, 3, 2
    board = B.nonbinary_board(w, h)
    parts = gol.strip_split(h, n)
    engs = [gol.Engine(w, h, device=0, row_offset=o, rows=r, halo=K) for o, r in parts]
    try:
        for e, (o, r) in zip(engs, parts):
            loaded = gol.haloed_rows(board, o, r, K)
            e.load(loaded)
            assert e.info().nonbinary_cells == int(((loaded != 0) & (loaded != 255)).sum())
            assert np.array_equal(e.read_board(), board[o:o + r])
        for t in (1, 2, 5):
            _run_strips(engs, t - engs[0].turn)
            got = np.concatenate([e.read_board() for e in engs])
            assert np.array_equal(got, oracle.ref_run(board, t, nsub=3, threads=2)), t
    finally:
        for e in engs:
            e.close()


def test_nonbinary_default_multiturn_engine(gol, oracle):
    """Non-binary bytes on a board whose default kernel is multi-turn (1024 x 96, k_step_tile):
    turn 1 runs alone with the mask, then the planner takes over, all inside one step(5)."""
    w, h = 1024, 96
    board = B.nonbinary_board(w, h)
    with gol.Engine(w, h, device=0) as e:
        e.load(board)
        assert e.info().nonbinary_cells == int(((board != 0) & (board != 255)).sum())
        assert np.array_equal(e.read_board(), board)
        e.step(5)
        plan = e.last_launches()
        assert plan[0][0] == 1 and sum(k for k, _, _ in plan) == 5
        want = oracle.ref_run(board, 5, nsub=2, threads=3)
        assert np.array_equal(e.read_board(), want)
        assert np.array_equal(e.alive_cells(), B.np_alive_cells(want))


# ------------------------------------------------------------ 5. chunked staging
_CHILD = r"""
import sys
sys.path[:0] = [sys.argv[1], sys.argv[2], sys.argv[3]]
import numpy as np
import gol
import io_boards as B
from gol import _native as N
from oracle import oracle as O

assert N.LIB_PATH.endswith("libgolamd_stage64k.so"), N.LIB_PATH

def stepped(board, turns):
    w = board.shape[1]
    return O.unpack(O.bit_run(O.pack(board)[0], w, turns), w)

CHUNK = 65536 // 16           # alive cells per staging chunk

# torus boards: 100 x 1500 = 3 chunks of 655 rows; 4160 x 50 = 15 rows per chunk; 8320 x 12
# full = 8320 cells per row against a 4096-cell chunk (the single-row-over-budget branch,
# which grows the staging buffer in the middle of the call)
for name, w, h in (("random50", 100, 1500), ("random16", 100, 1500), ("alt_rows", 100, 1500),
                   ("random50", 4160, 50), ("last_cell", 4160, 50), ("full", 8320, 12)):
    board = B.MAKERS[name](w, h)
    with gol.Engine(w, h, device=0, autotune=False) as e:
        e.load(board)
        B.check_readouts(O, e, board, 0, tag=(name, w, h, "load"))
        n = int((board == 255).sum())
        # caps inside the first chunk, on a chunk edge, inside a later chunk, and past the end
        for cap in sorted({1, CHUNK - 1, CHUNK, CHUNK + 17, 2 * CHUNK + 1, 8320 + 100,
                           n - 1, n, n + 5}):
            if cap >= 0:
                B.check_capped(e, board, cap, tag=(name, w, h))
        e.step(3)
        B.check_readouts(O, e, stepped(board, 3), 3, tag=(name, w, h, "step"))
    print("OK torus", name, w, h)

# a strip engine (rows < buffer_rows, row_offset > 0): own_lo + r0 and the global y in later
# chunks.  1408 buffer rows load in 3 chunks, 1400 owned rows read in 3 chunks.
w, H, off, rows, K = 100, 3000, 1000, 1400, 4
board = B.MAKERS["random50"](w, H)
with gol.Engine(w, H, device=0, row_offset=off, rows=rows, halo=K, autotune=False) as e:
    assert e.buffer_rows == rows + 2 * K
    e.load(gol.haloed_rows(board, off, rows, K))
    B.check_readouts(O, e, board[off:off + rows], 0, row_offset=off, tag="strip load")
    for cap in (CHUNK + 17, 3 * CHUNK):
        B.check_capped(e, board[off:off + rows], cap, row_offset=off, tag="strip")
    e.step(3)
    B.check_readouts(O, e, stepped(board, 3)[off:off + rows], 3, row_offset=off, tag="strip step")
print("OK strip")

# non-binary bytes through several pack launches: the mask rows and the count add up
w, h = 100, 1500
board = B.nonbinary_board(w, h)
with gol.Engine(w, h, device=0, autotune=False) as e:
    e.load(board)
    assert e.info().nonbinary_cells == int(((board != 0) & (board != 255)).sum())
    assert np.array_equal(e.read_board(), board)
    e.step(1)
    assert np.array_equal(e.read_board(), O.ref_run(board, 1, nsub=3, threads=2))
print("OK nonbinary")
"""


def test_chunked_staging():
    """libgolamd_stage64k.so (make smallstage: the engine with 64 KiB staging chunks instead of
    256 MiB) makes gol_load, the byte read-out and gol_alive_cells take a second and a third
    chunk on small boards: the r0 > 0 rows of k_pack / k_unpack, the alive list's offsets
    rebased per chunk, caps that end inside a chunk, and a single row larger than a chunk.
    Runs in a child process (the test library is a second copy of the engine)."""
    assert os.path.exists(STAGE_LIB), "build it: make -C conway-s-gol-distributed_amd/csrc smallstage"
    env = dict(os.environ, GOL_AMD_LIB=STAGE_LIB)
    r = subprocess.run([sys.executable, "-c", _CHILD, os.path.join(ROOT, "tests"),
                        os.path.join(ROOT, "conway-s-gol-distributed_amd"), ROOT],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert sum(l.startswith("OK torus") for l in lines) == 6, r.stdout
    assert "OK strip" in lines and "OK nonbinary" in lines, r.stdout


# ------------------------------------------------------------ 6. count ring
def _series64(oracle, upto):
    """Alive counts of the 64 x 64 fixture board for turns 1..upto as {turn: count}: the
    reference's CSV (Local/check/alive/64x64.csv) for turns <= 10000, the bit oracle (which
    reproduces that CSV, tests/test_oracle.py::test_bitref_alive_series) beyond it."""
    series = dict(G.alive_series(64))
    if upto > 10000:
        w, _, _ = oracle.pack(G.input_board(64))
        _, counts = oracle.bit_run(w, 64, upto, counts=True)
        assert [int(c) for c in counts[:10000]] == [series[t] for t in range(1, 10001)]
        series.update({t: int(counts[t - 1]) for t in range(10001, upto + 1)})
    return series


def _check_window(e, series, turn):
    """Every turn gol_turn_counts accepts at `turn` (turn-4095 .. turn) has its true count, and
    the turns on either side of the window are GOL_EINVAL."""
    from gol import _native as N
    first = max(1, turn - 4095)
    got = e.turn_counts(first, turn - first + 1).tolist()
    want = [series[t] for t in range(first, turn + 1)]
    bad = [(first + i, g, x) for i, (g, x) in enumerate(zip(got, want)) if g != x]
    assert not bad, (turn, len(bad), bad[:5])
    for t in (first - 1, turn + 1):
        with pytest.raises(N.GolError) as ei:
            e.turn_counts(t, 1)
        assert ei.value.code == N.GOL_EINVAL
    assert e.turn_counts(turn, 0).tolist() == []


def test_count_ring_window_and_stop(gol, oracle):
    """One gol_step of more than 4096 turns, the window's two edges, and a step that
    GOL_CONTROL_STOP ends before its first launch: the counts already recorded stay."""
    from gol import _native as N
    series = _series64(oracle, 0)
    with gol.Engine(64, 64, device=0, count_every_turn=True) as e:
        e.load(G.input_board(64))
        e.step(5000)
        assert e.turn_counts(905, 4096).tolist() == [series[t] for t in range(905, 5001)]
        _check_window(e, series, 5000)
        e.set_control(N.GOL_CONTROL_STOP)
        assert e.step(3000) is False and e.turn == 5000
        _check_window(e, series, 5000)
        e.set_control(N.GOL_CONTROL_RUN)
        assert e.step(100) is True
        _check_window(e, series, 5100)


def test_count_ring_read_mid_step(gol, oracle):
    """gol_turn_counts from a second thread while a long gol_step is parked on PAUSE in its
    middle, and after STOP has ended that step early: every turn of the window has its true
    count (the step clears ring slots ahead of itself; none of them may be a turn the window
    still accepts).  The step asks for more turns than it could run, so it is parked, not
    finished, when the reads happen; get_progress says at which turn."""
    import threading
    import time
    from gol import _native as N
    with gol.Engine(64, 64, device=0, count_every_turn=True) as e:
        e.load(G.input_board(64))
        e.step(5000)
        e.set_control(N.GOL_CONTROL_RUN)
        res = {}
        th = threading.Thread(target=lambda: res.update(done=e.step(10 ** 9)), daemon=True)
        th.start()
        t_end = time.time() + 10
        while e.progress()[0] <= 5000 and time.time() < t_end:
            pass
        e.set_control(N.GOL_CONTROL_PAUSE)
        while not e.progress()[1] and time.time() < t_end:
            time.sleep(0.001)
        t_paused, parked = e.progress()
        try:
            assert parked and t_paused > 5000
            series = _series64(oracle, t_paused)
            _check_window(e, series, t_paused)
        finally:
            e.set_control(N.GOL_CONTROL_STOP)
            th.join(30)
        assert not th.is_alive() and res["done"] is False
        assert e.turn == t_paused
        _check_window(e, series, t_paused)


def test_count_every_turn_on_strips(gol, oracle):
    """Per-turn counts on strip engines (n = 3, K = 4, 100 x 37, 23 turns): each engine counts
    its owned rows, so the engines' series add up to the oracle's."""
    w, h, n, K, turns = 100, 37, 3, 4, 23
    board = B.MAKERS["random50"](w, h)
    parts = gol.strip_split(h, n)
    engs = [gol.Engine(w, h, device=0, row_offset=o, rows=r, halo=K, count_every_turn=True)
            for o, r in parts]
    try:
        for e, (o, r) in zip(engs, parts):
            e.load(gol.haloed_rows(board, o, r, K))
        _run_strips(engs, turns)
        got = sum(e.turn_counts(1, turns) for e in engs)
        _, want = oracle.bit_run(oracle.pack(board)[0], w, turns, counts=True)
        assert got.tolist() == want.astype(np.int64).tolist()
        # and each engine alone against its rows of the oracle's boards
        for t in (1, turns):
            full = _stepped(oracle, board, t)
            for e, (o, r) in zip(engs, parts):
                assert int(e.turn_counts(t, 1)[0]) == int((full[o:o + r] == 255).sum())
    finally:
        for e in engs:
            e.close()


# ------------------------------------------------------------ packed loads: padding bits
def test_load_packed_rejects_dirty_padding(gol, oracle):
    """gol_load_packed at 100 x 8 (36 valid bits in each row's last word): clean words load;
    one set padding bit is GOL_EINVAL with the row named, and the engine keeps the board and
    the turn it had."""
    from gol import _native as N
    w, h = 100, 8
    first = B.MAKERS["random50"](w, h)
    other = B.MAKERS["random16"](w, h)
    clean = oracle.pack(other)[0]
    with gol.Engine(w, h, device=0, autotune=False) as e:
        e.load_packed(clean)
        B.check_readouts(oracle, e, other, 0, tag="clean")
        e.load(first)
        e.step(2)
        kept = _stepped(oracle, first, 2)
        for row, bit in ((3, 36), (7, 63), (0, 37)):
            dirty = clean.copy()
            dirty[row, 1] |= np.uint64(1) << np.uint64(bit)
            with pytest.raises(N.GolError) as ei:
                e.load_packed(dirty)
            assert ei.value.code == N.GOL_EINVAL
            assert f"row {row} " in str(ei.value), str(ei.value)
            B.check_readouts(oracle, e, kept, 2, tag=("kept", row, bit))
        # the last valid bit is not padding
        edge = clean.copy()
        edge[5, 1] |= np.uint64(1) << np.uint64(35)
        e.load_packed(edge)
        want = other.copy()
        want[5, 99] = 255
        B.check_readouts(oracle, e, want, 0, tag="edge")
        e.step(1)
        B.check_readouts(oracle, e, _stepped(oracle, want, 1), 1, tag="edge step")
