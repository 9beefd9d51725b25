"""k_settle_resident_batch on the device (gol.BatchEngine.step_settle / settled, gol_settle_*):
every board ends where the plain step puts it, and the (settled_turn, period) entries are the
oracle's (settle_cases: the orbit of every start board from oracle.bit_run, the contract's formula
for the turn of the match), whatever the launch depth and however many boards are resident."""
import numpy as np
import pytest

import resident_cases as RC
import settle_cases as SC

pytestmark = pytest.mark.gpu

STOPS = (1, 2, 7, 256, 257, 1024, 4200)          # cumulative turns


@pytest.fixture(scope="module")
def gol():
    import gol as g
    return g


@pytest.fixture(scope="module")
def N():
    from gol import _native
    return _native


def popcounts(boards):
    return np.array([sum(bin(int(w)).count("1") for w in b.ravel()) for b in boards], dtype=np.int64)


def run_each(oracle, boards, width, turns):
    return np.stack([oracle.bit_run(b, width, turns) for b in boards])


def entries(exps, now):
    """The (settled_turn, period) arrays gol_settle_read must give at turn `now`."""
    e = [SC.entry(x, now) for x in exps]
    return (np.array([t for t, _ in e], dtype=np.int64), np.array([p for _, p in e], dtype=np.int64))


def assert_entries(b, exps, now, what):
    turn, period = b.settled()
    want_turn, want_period = entries(exps, now)
    assert np.array_equal(period, want_period), (what, now, period, want_period)
    assert np.array_equal(turn, want_turn), (what, now, turn, want_turn)


# ------------------------------------------------------------------ 1. parity with the plain step
@pytest.fixture(scope="module")
def parity_case(oracle):
    """Per shape: the start boards (8 soups, a glider, a dead board, a block), the oracle's boards
    at every stop and every board's expected entry; computed once."""
    out = {}
    for width, height in ((64, 64), (65, 37)):
        start = [SC.soup(s, width, height) for s in RC.SEEDS]
        exps = [SC.soup_expected(s, width, height) for s in RC.SEEDS]
        for extra in (SC.glider(width, height), np.zeros_like(start[0]), SC.block(width, height, 9, 62)):
            start.append(extra)
            exps.append(SC.expected(extra, width, 4 * width * height + 1))
        assert all(e is not None for e in exps)
        start = np.stack(start)
        at = {}
        now, cur = 0, start
        for stop in STOPS:
            cur = run_each(oracle, cur, width, stop - now)
            now = stop
            at[stop] = cur
        # the stops see boards before their match, after it, and soups that are live and moving
        assert any(e[0] > 257 for e in exps) and any(e[0] <= 7 for e in exps)
        assert sum(e[0] <= 4200 for e in exps) >= 8, exps
        out[(width, height)] = (start, at, exps)
    return out


@pytest.mark.parametrize("depth", (None, 7, 1), ids=("unset", "depth7", "depth1"))
@pytest.mark.parametrize("shape", ((64, 64), (65, 37)), ids=("64x64", "65x37"))
def test_parity_with_the_plain_step(gol, oracle, parity_case, monkeypatch, shape, depth):
    width, height = shape
    start, at, exps = parity_case[shape]
    if depth is None:
        monkeypatch.delenv("GOL_SETTLE_DEPTH", raising=False)
    else:
        monkeypatch.setenv("GOL_SETTLE_DEPTH", str(depth))
    stops = tuple(s for s in STOPS if depth != 1 or s <= 300)
    B = len(start)
    with gol.BatchEngine(width, height, B, device=0) as a, \
            gol.BatchEngine(width, height, B, device=0) as plain:
        a.load_packed(start)
        plain.load_packed(start)
        now = 0
        for stop in stops:
            a.step_settle(stop - now)
            plain.step(stop - now)
            now = stop
            got = a.read_packed()
            assert a.turn == now and plain.turn == now
            assert np.array_equal(got, at[stop]), (shape, depth, now)
            assert np.array_equal(got, plain.read_packed()), (shape, depth, now)
            assert np.array_equal(a.alive(), popcounts(at[stop])), (shape, depth, now)
            assert np.array_equal(a.alive(), plain.alive()), (shape, depth, now)
            assert_entries(a, exps, now, (shape, depth))


# ------------------------------------------------------------------ 2. the compare, per class
@pytest.mark.parametrize("shape", SC.class_shapes(extra=((64, 4096), (255, 1024))),
                         ids=lambda s: f"{s[0]}x{s[1]}")
def test_compare_covers_every_lane_row_and_word(gol, oracle, shape):
    width, height = shape
    cases = SC.class_boards(width, height)
    start = np.stack([c[1] for c in cases])
    exps = [SC.expected(c[1], width, 16) for c in cases]
    assert exps == [(3, 2) if c[2] == 2 else (1, 1) for c in cases]
    want = run_each(oracle, start, width, 8)
    with gol.BatchEngine(width, height, len(cases), device=0) as b:
        assert b.info.waves == 4
        b.load_packed(start)
        b.step_settle(8)
        got = b.read_packed()
        turn, period = b.settled()
    for k, (name, _, _) in enumerate(cases):
        assert (int(turn[k]), int(period[k])) == exps[k], (shape, name)
        assert np.array_equal(got[k], want[k]), (shape, name)


# ------------------------------------------------------------------ 3. a period longer than a launch
def test_period_longer_than_a_launch(gol, oracle):
    width, height = 64, 48
    start = SC.glider(width, height)
    exp = SC.expected(start, width, 2048)
    assert exp == (1791, 768)
    with gol.BatchEngine(width, height, 2, device=0) as b:
        b.load_packed(np.stack([start, start]))
        b.step_settle(1790)
        assert_entries(b, [exp, exp], 1790, "before")
        b.step_settle(1)
        assert_entries(b, [exp, exp], 1791, "at the match")
        assert np.array_equal(b.read_packed()[0], oracle.bit_run(start, width, 1791))
        b.step_settle(1000)                      # the skip path: 1000 mod 768 turns
        assert b.turn == 2791
        want = oracle.bit_run(start, width, 2791)
        got = b.read_packed()
        assert np.array_equal(got[0], want) and np.array_equal(got[1], want)
        assert_entries(b, [exp, exp], 2791, "after")


# ------------------------------------------------------------------ 4. boards do not share state
def test_boards_do_not_share_state(gol, oracle):
    """16 x 16, 600 turns, more boards than one launch keeps resident (test_gpu_batch's rule with
    5200 boards), soups of 8 seeds cycled: by the oracle (the guard below) some of them have
    their match by turn 600 and some have not, so settled and unsettled members alternate."""
    w = h = 16
    turns = 600
    with gol.BatchEngine(w, h, 1, device=0) as probe:
        per_cu, cus = probe.occupancy()
    capacity = per_cu * cus
    B = 5200 if capacity < 5200 else capacity + 1
    exps8 = [SC.soup_expected(s, w, h) for s in RC.SEEDS]
    assert any(e[0] <= turns for e in exps8) and any(e[0] > turns for e in exps8), exps8
    want8 = [oracle.bit_run(SC.soup(s, w, h), w, turns) for s in RC.SEEDS]
    start = np.stack([SC.soup(RC.SEEDS[k % 8], w, h) for k in range(B)])
    with gol.BatchEngine(w, h, B, device=0) as b:
        b.load_packed(start)
        b.step_settle(turns)
        got = b.read_packed()
        turn, period = b.settled()
    bad = [k for k in range(B) if not np.array_equal(got[k], want8[k % 8])]
    assert not bad, bad[:8]
    want_turn, want_period = entries([exps8[k % 8] for k in range(B)], turns)
    assert np.array_equal(period, want_period), np.flatnonzero(period != want_period)[:8]
    assert np.array_equal(turn, want_turn), np.flatnonzero(turn != want_turn)[:8]


# ------------------------------------------------------------------ 5. resets
def test_a_plain_step_restarts_the_watch(gol, oracle):
    width, height = 16, 16
    start = np.stack([SC.glider(width, height), SC.blinker(width, height, 4, 4),
                      SC.soup(1, width, height)])
    with gol.BatchEngine(width, height, 3, device=0) as b:
        b.load_packed(start)
        b.step_settle(200)
        exps = [SC.expected(s, width, 1024) for s in start]
        assert exps[0] == (127, 64) and exps[1] == (3, 2)
        assert_entries(b, exps, 200, "first watch")
        b.step(5)                                # forgets the periods
        at205 = run_each(oracle, start, width, 205)
        assert np.array_equal(b.read_packed(), at205)
        b.step_settle(0)                         # the watch restarts at turn 205
        exps = [SC.expected(s, width, 1024, start_turn=205) for s in at205]
        assert exps[0] == (205 + 127, 64) and exps[1] == (205 + 3, 2)
        assert_entries(b, exps, 205, "restart")
        b.step_settle(100)
        assert_entries(b, exps, 305, "restart")
        b.step_settle(100)
        assert_entries(b, exps, 405, "restart")
        assert np.array_equal(b.read_packed(), run_each(oracle, start, width, 405))


def test_a_partial_load_restarts_its_boards_only(gol, oracle):
    width, height = 16, 16
    start = np.stack([SC.glider(width, height)] * 4)
    fresh = np.stack([SC.blinker(width, height, 4, 4), SC.glider(width, height)])
    exp = SC.expected(start[0], width, 1024)
    with gol.BatchEngine(width, height, 4, device=0) as b:
        b.load_packed(start)
        b.step_settle(50)
        b.load_packed(fresh, first=1)            # members 1 and 2, mid-watch, at turn 50
        assert b.turn == 50
        exps = [exp, SC.expected(fresh[0], width, 1024, start_turn=50),
                SC.expected(fresh[1], width, 1024, start_turn=50), exp]
        assert exps == [(127, 64), (53, 2), (177, 64), (127, 64)]
        assert_entries(b, exps, 50, "after the load")
        for now in (52, 53, 130, 177, 400):
            b.step_settle(now - b.turn)
            assert_entries(b, exps, now, "partial")
        want = run_each(oracle, start, width, 400)
        want[1:3] = run_each(oracle, fresh, width, 350)
        assert np.array_equal(b.read_packed(), want)


def test_fill_and_whole_load_end_the_watch(gol, oracle, N):
    width, height = 64, 64
    with gol.BatchEngine(width, height, 3, device=0) as b:
        with pytest.raises(N.GolError) as e:     # (no watch yet)
            b.settled()
        assert e.value.code == N.GOL_ESTATE
        for reset in ("fill", "load", "step"):
            b.step_settle(3)
            b.settled()
            for first, n in ((3, 1), (-1, 1), (0, 0), (2, 2)):
                with pytest.raises(N.GolError) as e:
                    b.settled(first, n)
                assert e.value.code == N.GOL_EINVAL, (first, n)
            assert len(b.settled(1)[0]) == 2 and len(b.settled(2, 1)[1]) == 1
            if reset == "fill":
                b.fill_random(5)
            elif reset == "load":
                b.load_packed(oracle.gen_random(5, width, 3 * height).reshape(3, height, 1))
            else:
                b.step(1)
            with pytest.raises(N.GolError) as e:
                b.settled()
            assert e.value.code == N.GOL_ESTATE, reset
        b.fill_random(5)
        b.step_settle(9)
        turn, period = b.settled()
        assert b.turn == 9 and (turn == -1).all() and (period == 0).all()
        want = run_each(oracle, oracle.gen_random(5, width, 3 * height).reshape(3, height, 1), width, 9)
        assert np.array_equal(b.read_packed(), want)


# ------------------------------------------------------------------ 6. a counted batch
def test_counted_batch_refuses(gol, oracle, N):
    width, height = 64, 64
    start = np.stack([SC.soup(s, width, height) for s in RC.SEEDS[:2]])
    with gol.BatchEngine(width, height, 2, device=0, count_every_turn=True) as b:
        b.load_packed(start)
        b.step(3)
        before = b.read_packed()
        with pytest.raises(N.GolError) as e:
            b.step_settle(5)
        assert e.value.code == N.GOL_ESTATE
        assert b.turn == 3 and np.array_equal(b.read_packed(), before)
        with pytest.raises(N.GolError) as e:
            b.settled()
        assert e.value.code == N.GOL_ESTATE
        b.step(4)
        series = np.stack([RC.oracle_run(s, width, height, 7)[1] for s in RC.SEEDS[:2]], axis=1)
        assert np.array_equal(b.turn_counts(1, 7), series)
        assert np.array_equal(b.read_packed(), run_each(oracle, start, width, 7))
