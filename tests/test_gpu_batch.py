"""k_step_resident_batch on the device (gol.BatchEngine, gol_batch_*): many torus boards narrower
than 256 cells in one buffer, one workgroup per board, stepped in place.  The expected board of
batch member i is oracle.bit_run of that member's start rows alone; the shapes, the partition and
the liveness guard are resident_cases'."""
import numpy as np
import pytest

import resident_cases as RC

pytestmark = pytest.mark.gpu

STEPS = (1, 2, 7, 256, 257)                      # cumulative; 257 = two launches, 1 = new ground
TINY = RC.TINY + ((2, 3), (3, 3))


@pytest.fixture(scope="module")
def gol():
    import gol as g
    return g


def _err(gol):
    from gol import _native as N
    return N


def sweep_heights(width):
    """RC.heights_for, the heights that change the wave count (64, 65 and 256 lanes), and one
    ragged height for every rows-per-lane count R the kernel is built for at this width."""
    extra = tuple(RC.height_with_lanes(width, n) for n in (64, 65, 256))
    nw = RC.nwords(width)
    per_r = tuple(256 * r - 3 for r in range(1, 17)
                  if r * nw <= 16 and (r & (r - 1) == 0 or r == 16 // nw))
    return tuple(dict.fromkeys(RC.heights_for(width) + extra + per_r))


def live_seeds(width, height, turns_list, n):
    """The first n seeds of RC.SEEDS that are live (alive and changing) at one of those turns;
    the guard fails the test where fewer are."""
    out = [s for s in RC.SEEDS if any(RC.is_live(s, width, height, t) for t in turns_list)]
    assert len(out) >= n, f"{width}x{height}: live seeds {out} among {RC.SEEDS} at {turns_list}"
    return out[:n]


def popcounts(boards):
    return np.array([sum(bin(int(w)).count("1") for w in b.ravel()) for b in boards], dtype=np.int64)


def run_each(oracle, boards, width, turns):
    """Every member stepped alone by the oracle."""
    return np.stack([oracle.bit_run(b, width, turns) for b in boards])


# ------------------------------------------------------------------ 1. parity per (nw, R) class
@pytest.mark.parametrize("width", (64, 128, 191, 255, 63, 65))
def test_parity_per_class(gol, oracle, width):
    classes = set()
    for height in sweep_heights(width):
        lanes, rows, waves = RC.plan(width, height)
        classes.add((RC.nwords(width), rows))
        seeds = live_seeds(width, height, (1, 3, 10), 3)
        start = np.stack([RC.oracle_run(s, width, height, 0)[0] for s in seeds])
        with gol.BatchEngine(width, height, 3, device=0) as b:
            i = b.info
            assert (i.width, i.height, i.boards, i.words_per_row) == (width, height, 3, RC.nwords(width))
            assert (i.lanes, i.rows_per_lane, i.waves, i.turn) == (lanes, rows, waves, 0)
            assert not b.read_packed().any()                      # (a new batch: dead boards)
            b.load_packed(start)
            done = 0
            for turns in STEPS:
                b.step(turns)
                done += turns
                want = np.stack([RC.oracle_run(s, width, height, done)[0] for s in seeds])
                got = b.read_packed()
                assert np.array_equal(got, want), (width, height, done)
                assert b.turn == done
                cells = b.read()
                assert cells.shape == (3, height, width)
                for k in range(3):
                    assert np.array_equal(cells[k], oracle.unpack(want[k], width)), (width, height, done, k)
                assert np.array_equal(b.alive(), popcounts(want)), (width, height, done)
    # every rows-per-lane class of this nw was run
    nw = RC.nwords(width)
    built = {r for r in range(1, 17) if r * nw <= 16 and (r & (r - 1) == 0 or r == 16 // nw)}
    assert {r for n, r in classes if n == nw} == built, classes


# ------------------------------------------------------------------ 2. every start board at once
@pytest.mark.parametrize("shape", TINY, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_start_board_at_once(gol, oracle, shape):
    width, height = shape
    start = RC.tiny_boards(width, height)
    t1 = run_each(oracle, start, width, 1)
    t2 = run_each(oracle, t1, width, 1)
    # (on the oracle's side, unlike at the two turns the single-board test must use: at turn 1
    # some members are alive and some have changed.  On 2 x 1 and 2 x 2 no single member does
    # both -- a cell's one x neighbour counts twice in each of three rows, so a board either
    # stands still or dies at once; on the other four shapes some member is alive at turn 1 and
    # unlike its start.)
    alive = {k for k in range(len(start)) if t1[k].any()}
    changed = {k for k in range(len(start)) if not np.array_equal(t1[k], start[k])}
    assert alive and changed, shape
    assert bool(alive & changed) == (shape not in ((2, 1), (2, 2))), shape
    if shape != (3, 1):                          # (all 8 boards of 3 x 1 are empty by turn 2)
        assert any(t2[k].any() for k in range(len(start))), shape
    with gol.BatchEngine(width, height, len(start), device=0) as b:
        b.load_packed(start)
        want = start
        for done in (1, 2, 3):
            b.step(1)
            want = run_each(oracle, want, width, 1)
            got = b.read_packed()
            bad = [k for k in range(len(start)) if not np.array_equal(got[k], want[k])]
            assert not bad, (shape, done, bad[:8])
            assert b.turn == done


# ------------------------------------------------------------------ 3. boards do not see each other
@pytest.mark.parametrize("alive_members", ((0, 2, 4), (1, 3)), ids=("even", "odd"))
def test_boards_do_not_see_each_other(gol, oracle, alive_members):
    w = h = 64
    seeds = live_seeds(w, h, (9,), 3)
    start = np.zeros((5, h, 1), dtype=np.uint64)
    for k, s in zip(alive_members, seeds):
        start[k] = RC.oracle_run(s, w, h, 0)[0]
    with gol.BatchEngine(w, h, 5, device=0) as b:
        b.load_packed(start)
        b.step(9)
        got = b.read_packed()
    for k in range(5):
        if k in alive_members:
            want = RC.oracle_run(seeds[alive_members.index(k)], w, h, 9)[0]
            assert want.any() and np.array_equal(got[k], want), k
        else:
            assert not got[k].any(), k


# ------------------------------------------------------------------ 4. partial ranges
def test_partial_ranges(gol, oracle):
    N = _err(gol)
    w, h, B = 200, 77, 6
    seeds = live_seeds(w, h, (5, 9), 8)
    start = np.stack([RC.oracle_run(s, w, h, 0)[0] for s in seeds[:B]])
    fresh = np.stack([RC.oracle_run(s, w, h, 0)[0] for s in seeds[6:8]])
    with gol.BatchEngine(w, h, B, device=0) as b:
        b.load_packed(start)
        b.step(5)
        at5 = run_each(oracle, start, w, 5)
        assert np.array_equal(b.read_packed(), at5)
        b.load_packed(fresh, first=2)            # members 2 and 3, mid-run
        assert b.turn == 5
        mixed = at5.copy()
        mixed[2:4] = fresh
        assert np.array_equal(b.read_packed(), mixed)
        for first, n in ((0, 1), (2, 2), (5, 1), (1, 4), (0, 6)):
            got = b.read_packed(first, n)
            assert got.shape == (n, h, RC.nwords(w))
            assert np.array_equal(got, mixed[first:first + n]), (first, n)
            assert np.array_equal(b.alive(first, n), popcounts(mixed[first:first + n]))
            assert np.array_equal(b.read(first, n),
                                  np.stack([oracle.unpack(m, w) for m in mixed[first:first + n]]))
        assert np.array_equal(b.read_packed(4), mixed[4:])        # (n = None: to the end)
        # out-of-range ranges: GOL_EINVAL, nothing changed
        for first, n in ((5, 2), (6, 1), (-1, 2), (0, 7), (0, 0), (3, -1)):
            with pytest.raises(N.GolError) as e:
                b.read_packed(first, n)
            assert e.value.code == N.GOL_EINVAL, (first, n)
            with pytest.raises(N.GolError) as e:
                b.alive(first, n)
            assert e.value.code == N.GOL_EINVAL, (first, n)
            with pytest.raises(N.GolError) as e:
                b.read(first, n)
            assert e.value.code == N.GOL_EINVAL, (first, n)
        for first in (5, 6, -1):
            with pytest.raises(N.GolError) as e:
                b.load_packed(fresh, first=first)
            assert e.value.code == N.GOL_EINVAL, first
            with pytest.raises(N.GolError) as e:
                b.load(np.zeros((2, h, w), dtype=np.uint8), first=first)
            assert e.value.code == N.GOL_EINVAL, first
        assert b.turn == 5 and np.array_equal(b.read_packed(), mixed)
        b.step(4)
        assert b.turn == 9
        assert np.array_equal(b.read_packed(), run_each(oracle, mixed, w, 4))
        # a byte load of a part keeps the turn too; a whole-range load resets it
        cells = np.stack([oracle.unpack(m, w) for m in fresh])
        cells[cells == 0] = 7                    # (anything but 255 is dead)
        b.load(cells, first=0)
        assert b.turn == 9 and np.array_equal(b.read_packed(0, 2), fresh)
        b.load_packed(start)
        assert b.turn == 0 and np.array_equal(b.read_packed(), start)
        b.step(3)
        b.load(np.stack([oracle.unpack(m, w) for m in start]))
        assert b.turn == 0 and np.array_equal(b.read_packed(), start)


# ------------------------------------------------------------------ 5. more workgroups than fit at once
def test_more_workgroups_than_fit_at_once(gol, oracle):
    """16 x 16, 7 turns, more boards than one launch keeps resident: the co-resident capacity is
    CUs x the occupancy the runtime reports for this kernel (gol_batch_occupancy).  B = 8200
    unless the capacity reaches it, then capacity + 1.
    (The MI355X run this test was written on reported 20 workgroups per CU x 256 CUs = 5120 --
    the 8 KiB exchange area is what caps it -- and so used B = 8200: two rounds.)"""
    w = h = 16
    with gol.BatchEngine(w, h, 1, device=0) as probe:
        per_cu, cus = probe.occupancy()
    assert per_cu >= 1 and cus >= 1
    capacity = per_cu * cus
    B = 8200 if capacity < 8200 else capacity + 1
    print(f"occupancy {per_cu} workgroups per CU x {cus} CUs = {capacity}; B = {B}")
    assert B > capacity
    start = oracle.gen_random(5, w, B * h).reshape(B, h, 1)
    want = run_each(oracle, start, w, 7)
    changed = sum(1 for k in range(B) if want[k].any() and not np.array_equal(want[k], start[k]))
    assert changed > B // 2
    with gol.BatchEngine(w, h, B, device=0) as b:
        b.load_packed(start)
        b.step(7)
        got = b.read_packed()
    bad = [k for k in range(B) if not np.array_equal(got[k], want[k])]
    assert not bad, bad[:8]


# ------------------------------------------------------------------ 6. fill
@pytest.mark.parametrize("width,height,B", ((64, 64, 5), (200, 77, 4)))
def test_fill_random(gol, oracle, width, height, B):
    seed = 21
    whole = oracle.gen_random(seed, width, B * height)
    start = whole.reshape(B, height, RC.nwords(width))
    with gol.BatchEngine(width, height, B, device=0) as b, \
            gol.Engine(width, B * height, device=0) as e:
        b.load_packed(start[::-1].copy())
        b.step(2)
        b.fill_random(seed)
        assert b.turn == 0
        assert np.array_equal(b.read_packed(), start)
        e.fill_random(seed)                      # (the definition: one board of B x height rows)
        assert np.array_equal(e.read_packed(), whole)
        b.step(9)
        want = run_each(oracle, start, width, 9)
        assert all(want[k].any() and not np.array_equal(want[k], start[k]) for k in range(B))
        assert np.array_equal(b.read_packed(), want)


# ------------------------------------------------------------------ 7. against the single-board engine
@pytest.mark.parametrize("width,height", ((200, 77), (64, 4096)))
def test_against_the_single_board_engine(gol, oracle, width, height):
    B = 3
    start = oracle.gen_random(31, width, B * height).reshape(B, height, RC.nwords(width))
    with gol.BatchEngine(width, height, B, device=0) as b:
        b.load_packed(start)
        b.step(300)
        got = b.read_packed()
        assert b.turn == 300
    for k in range(B):
        with gol.Engine(width, height, device=0, resident=True) as e:
            assert e.info().turns_per_launch == 256
            e.load_packed(start[k])
            e.step(300)
            want = e.read_packed()
        assert want.any() and not np.array_equal(want, start[k])
        assert np.array_equal(got[k], want), k


# ------------------------------------------------------------------ 8. counts
@pytest.mark.parametrize("width,height", ((64, 64), (200, 77), (255, 1024)))
def test_counts(gol, oracle, width, height):
    N = _err(gol)
    seeds = live_seeds(width, height, (307,), 3)
    start = np.stack([RC.oracle_run(s, width, height, 0)[0] for s in seeds])
    series = np.stack([RC.oracle_run(s, width, height, 307)[1] for s in seeds], axis=1)  # (307, 3)
    with gol.BatchEngine(width, height, 3, device=0, count_every_turn=True) as b:
        b.load_packed(start)
        b.step(7)
        assert np.array_equal(b.turn_counts(1, 7), series[:7])
        with pytest.raises(N.GolError) as e:
            b.turn_counts(8, 1)                  # (not stepped yet)
        assert e.value.code == N.GOL_EINVAL
        b.step(300)
        turn = b.turn
        assert turn == 307
        got = b.turn_counts(turn - 255, 256)
        assert got.shape == (256, 3) and got.dtype == np.int64
        assert np.array_equal(got, series[turn - 256:turn])
        assert np.array_equal(b.turn_counts(turn, 1), series[-1:])
        assert np.array_equal(b.alive(), series[-1])
        for first, n in ((turn - 256, 1), (turn - 256, 257), (turn, 2), (turn + 1, 1), (0, 1)):
            with pytest.raises(N.GolError) as e:
                b.turn_counts(first, n)
            assert e.value.code == N.GOL_EINVAL, (first, n)
        want = np.stack([RC.oracle_run(s, width, height, 307)[0] for s in seeds])
        assert np.array_equal(b.read_packed(), want)
        # after a whole-batch load, turns before it are refused
        b.load_packed(start)
        assert b.turn == 0
        with pytest.raises(N.GolError) as e:
            b.turn_counts(1, 1)
        assert e.value.code == N.GOL_EINVAL
        b.step(2)
        assert np.array_equal(b.turn_counts(1, 2), series[:2])
        with pytest.raises(N.GolError) as e:
            b.turn_counts(3, 1)
        assert e.value.code == N.GOL_EINVAL


def test_counts_store_zeros(gol, oracle):
    """A member that dies out has stored zeros: its ring slots held another board's non-zero
    counts 256 turns earlier."""
    w = h = 16
    seeds = live_seeds(w, h, (261,), 2)
    start = np.stack([RC.oracle_run(s, w, h, 0)[0] for s in seeds])
    series = np.stack([RC.oracle_run(s, w, h, 261)[1] for s in seeds], axis=1)
    lone = np.zeros((1, h, 1), dtype=np.uint64)
    lone[0, 8, 0] = 1 << 8                       # one cell: the oracle empties it in one turn
    after, lone_series = oracle.bit_run(lone[0], w, 5, counts=True)
    assert not after.any() and [int(c) for c in lone_series] == [0] * 5
    assert (series[:5, 1] > 0).all()             # (what the slots of turns 257 .. 261 held)
    with gol.BatchEngine(w, h, 2, device=0, count_every_turn=True) as b:
        b.load_packed(start)
        b.step(256)
        assert np.array_equal(b.turn_counts(1, 256), series[:256])
        b.load_packed(lone, first=1)
        assert b.turn == 256
        b.step(5)
        got = b.turn_counts(257, 5)
        assert np.array_equal(got[:, 0], series[256:261, 0])
        assert np.array_equal(got[:, 1], np.zeros(5, dtype=np.int64))
        assert np.array_equal(b.alive(), np.array([series[260, 0], 0]))


def test_counts_need_the_flag(gol):
    N = _err(gol)
    with gol.BatchEngine(64, 64, 2, device=0) as b:
        b.fill_random(3)
        b.step(4)
        with pytest.raises(N.GolError) as e:
            b.turn_counts(1, 1)
        assert e.value.code == N.GOL_ESTATE


# ------------------------------------------------------------------ 9. padding rule
def test_padding_rule(gol, oracle):
    N = _err(gol)
    w, h, B = 200, 77, 3
    start = oracle.gen_random(41, w, B * h).reshape(B, h, RC.nwords(w))
    with gol.BatchEngine(w, h, B, device=0) as b:
        b.load_packed(start)
        b.step(3)
        before = b.read_packed()
        bad = start.copy()
        bad[1, 3, 3] |= np.uint64(1) << np.uint64(200 - 192)     # the first padding bit
        for first, member in ((0, 1), (1, 0)):
            with pytest.raises(N.GolError) as e:
                b.load_packed(bad[first:], first=first)
            assert e.value.code == N.GOL_EINVAL
            assert "board 1" in str(e.value) and "row 3" in str(e.value), str(e.value)
            assert b.turn == 3 and np.array_equal(b.read_packed(), before)
        bad[1, 3, 3] = start[1, 3, 3]
        bad[2, 76, 3] |= np.uint64(1) << np.uint64(63)
        with pytest.raises(N.GolError) as e:
            b.load_packed(bad)
        assert "board 2" in str(e.value) and "row 76" in str(e.value), str(e.value)
        assert b.turn == 3 and np.array_equal(b.read_packed(), before)


# ------------------------------------------------------------------ 10. limits
@pytest.mark.parametrize("width,height", ((64, 4096), (128, 2048), (192, 1280), (255, 1024)))
def test_limits(gol, oracle, width, height):
    N = _err(gol)
    assert RC.limit(width) == height
    start = oracle.gen_random(11, width, 2 * height).reshape(2, height, RC.nwords(width))
    with gol.BatchEngine(width, height, 2, device=0) as b:
        assert b.info.lanes == 256
        b.load_packed(start)
        b.step(9)
        want = run_each(oracle, start, width, 9)
        assert all(want[k].any() and not np.array_equal(want[k], start[k]) for k in range(2))
        assert np.array_equal(b.read_packed(), want)
    with pytest.raises(N.GolError) as e:
        gol.BatchEngine(width, height + 1, 2, device=0)
    assert e.value.code == N.GOL_EINVAL
