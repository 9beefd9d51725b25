"""k_step_resident on the device (GOL_FLAG_RESIDENT, Engine(resident=True)): a torus board
narrower than 256 cells held in the registers of one workgroup, up to 256 turns per launch
(launch kind 18).  Boards, counts and every service call against oracle.bit_run and against an
engine without the flag; the partition is read through gol_resident_plan."""
import ctypes
import threading
import time

import numpy as np
import pytest

import golden_data as G
import resident_cases as RC

pytestmark = pytest.mark.gpu

KIND = 18                                           # golk::kMultiResident
STEPS = (2, 7, 256, 600)
# Shapes whose every start board is run instead of a guarded random one.  A resident launch has
# at least 2 turns, and no board of 2 x 3 or 3 x 3 cells is live there (alive and unlike the
# turn before, at turn 2, 3 or 9: all 64 and all 512 start boards checked with the oracle), as
# none of the CPU file's four shapes is: a random case of these six would compare dead or
# frozen boards.
TINY = RC.TINY + ((2, 3), (3, 3))


@pytest.fixture(scope="module")
def gol():
    import gol as g
    return g


def _resident_launches(e, turns):
    """The last step's launches: all of kind 18, 2 .. 256 turns each, `turns` in all."""
    ls = e.last_launches()
    assert ls and all(kern == KIND and 2 <= k <= 256 for k, kern, _ in ls), ls
    assert sum(k for k, _, _ in ls) == turns, ls
    assert all(t == (0, 0, 0) for t in e.last_launch_tiles()), e.last_launch_tiles()
    return [k for k, _, _ in ls]


def _sweep_heights(width):
    """The CPU sweep's heights and the ones that change the wave count: 64, 65 and 256 lanes."""
    extra = tuple(RC.height_with_lanes(width, n) for n in (64, 65, 256))
    for h, n in zip(extra, (64, 65, 256)):
        lanes, _, waves = RC.plan(width, h)
        assert lanes == n and waves == -(-n // 64)
    return tuple(dict.fromkeys(RC.heights_for(width) + extra))


# ------------------------------------------------------------------ 1. parity sweep
@pytest.mark.parametrize("width", RC.WIDTHS)
def test_parity_sweep(gol, width):
    for height in _sweep_heights(width):
        seed = 1 if (width, height) in TINY else RC.live_seed(width, height, (2, 9))
        start, _ = RC.oracle_run(seed, width, height, 0)
        with gol.Engine(width, height, device=0, resident=True) as e, \
                gol.Engine(width, height, device=0) as plain:
            assert e.info().turns_per_launch == 256
            assert plain.info().turns_per_launch == 1
            e.load_packed(start)
            plain.load_packed(start)
            done = 0
            for turns in STEPS:
                e.step(turns)
                plain.step(turns)
                done += turns
                ks = _resident_launches(e, turns)
                if turns == 600:
                    assert ks == [200, 200, 200]
                assert all(k == 1 for k, _, _ in plain.last_launches())
                got = e.read_packed()
                want, _ = RC.oracle_run(seed, width, height, done)
                assert np.array_equal(got, want), (width, height, done)
                assert np.array_equal(got, plain.read_packed()), (width, height, done)
                assert e.board_layout() == 0
                assert e.info().turns_per_launch == 256
                assert e.turn == done


# ------------------------------------------------------------------ 2. exhaustive tiny boards
@pytest.mark.parametrize("shape", TINY, ids=lambda s: f"{s[0]}x{s[1]}")
def test_exhaustive_tiny_boards(gol, oracle, shape):
    width, height = shape
    alive = 0
    with gol.Engine(width, height, device=0, resident=True) as e:
        assert e.info().turns_per_launch == 256
        for start in RC.tiny_boards(width, height):
            for turns in (2, 3):
                e.load_packed(start)
                e.step(turns)
                assert _resident_launches(e, turns) == [turns]
                want = oracle.bit_run(start, width, turns)
                assert np.array_equal(e.read_packed(), want), (shape, start.tolist(), turns)
                alive += int(want.any())
    # (on the oracle's side: every shape but 3 x 1 has start boards still alive after 2 and 3
    # turns; all 8 boards of 3 x 1 are empty by turn 2, and the kernel has to empty them too)
    assert (alive > 0) == (shape != (3, 1))


# ------------------------------------------------------------------ 3. limits
@pytest.mark.parametrize("width,height", ((64, 4096), (128, 2048), (192, 1280), (255, 1024)))
def test_limits(gol, oracle, width, height):
    assert RC.limit(width) == height
    start = oracle.gen_random(11, width, height)
    with gol.Engine(width, height, device=0, resident=True) as e:
        assert e.info().turns_per_launch == 256
        e.load_packed(start)
        e.step(9)
        assert _resident_launches(e, 9) == [9]
        assert np.array_equal(e.read_packed(), oracle.bit_run(start, width, 9))
    start = oracle.gen_random(11, width, height + 1)
    with gol.Engine(width, height + 1, device=0, resident=True) as e:
        assert e.info().turns_per_launch == 1
        e.load_packed(start)
        e.step(9)
        assert [k for k, _, _ in e.last_launches()] == [1] * 9
        assert np.array_equal(e.read_packed(), oracle.bit_run(start, width, 9))


# ------------------------------------------------------------------ 4. requests that switch it off
@pytest.mark.parametrize("kw", ({"turns_per_launch": 1}, {"force_generic": True}),
                         ids=("depth1", "forced_generic"))
def test_switched_off_by_request(gol, oracle, kw):
    start = oracle.gen_random(4, 200, 77)
    with gol.Engine(200, 77, device=0, resident=True, **kw) as e:
        assert e.info().turns_per_launch == 1
        e.load_packed(start)
        e.step(9)
        assert [k for k, _, _ in e.last_launches()] == [1] * 9
        assert np.array_equal(e.read_packed(), oracle.bit_run(start, 200, 9))


def test_switched_off_on_a_strip(gol, oracle):
    """A strip engine (halo > 0) with the flag runs as without it: one turn per launch."""
    w, h, off, rows, halo = 200, 77, 20, 30, 4
    start = oracle.gen_random(4, w, h)
    buf = start[np.arange(off - halo, off + rows + halo) % h]
    want = oracle.bit_run(start, w, halo)[off:off + rows]
    boards = []
    for flag in (True, False):
        with gol.Engine(w, h, device=0, row_offset=off, rows=rows, halo=halo, resident=flag) as e:
            assert e.info().turns_per_launch == 1
            e.load_packed(buf)
            e.step(halo)
            assert [k for k, _, _ in e.last_launches()] == [1] * halo
            boards.append(e.read_packed())
    assert np.array_equal(boards[0], want) and np.array_equal(boards[1], want)


def test_switched_off_at_width_256(gol, oracle):
    """Width 256 has k_step_tile: the flag changes nothing, launch for launch."""
    start = oracle.gen_random(4, 256, 77)
    seen = []
    for flag in (True, False):
        with gol.Engine(256, 77, device=0, resident=flag, autotune=False) as e:
            tpl = e.info().turns_per_launch
            e.load_packed(start)
            e.step(9)
            ls = e.last_launches()
            assert all(kern != KIND for _, kern, _ in ls)
            seen.append((tpl, ls))
            assert np.array_equal(e.read_packed(), oracle.bit_run(start, 256, 9))
    assert seen[0] == seen[1]


def test_requested_depth(gol, oracle):
    start = oracle.gen_random(4, 200, 77)
    with gol.Engine(200, 77, device=0, resident=True, turns_per_launch=5) as e:
        assert e.info().turns_per_launch == 5
        e.load_packed(start)
        e.step(23)
        ks = _resident_launches(e, 23)
        assert len(ks) == 5 and max(ks) <= 5
        assert np.array_equal(e.read_packed(), oracle.bit_run(start, 200, 23))


# ------------------------------------------------------------------ 5. counts
@pytest.mark.parametrize("width,height", ((64, 64), (200, 77), (255, 64), (16, 16)))
def test_counts(gol, width, height):
    seed = RC.live_seed(width, height, (600,))
    start, _ = RC.oracle_run(seed, width, height, 0)
    want, series = RC.oracle_run(seed, width, height, 600)
    with gol.Engine(width, height, device=0, resident=True, count_every_turn=True) as e:
        assert e.info().turns_per_launch == 256
        e.load_packed(start)
        e.step(600)
        assert _resident_launches(e, 600) == [200, 200, 200]
        assert np.array_equal(e.turn_counts(1, 600), series)
        assert e.snapshot() == (600, int(series[-1]))
        assert np.array_equal(e.read_packed(), want)


# ------------------------------------------------------------------ 6. counts across the ring end
def test_counts_across_the_ring_end(gol, oracle):
    """192 x 200: turn 4352 takes slot 0 of the count ring (4096 + 256 slots), so the launch
    before it ends exactly at turn 4351."""
    w, h = 192, 200
    start = oracle.gen_random(7, w, h)
    want, series = oracle.bit_run(start, w, 4600, counts=True)
    series = np.asarray(series, dtype=np.int64)
    assert len(set(series[4200:4600].tolist())) >= 100
    with gol.Engine(w, h, device=0, resident=True, count_every_turn=True) as e:
        e.load_packed(start)
        e.step(4200)
        _resident_launches(e, 4200)
        e.step(400)
        ks = _resident_launches(e, 400)
        ends = (4200 + np.cumsum(ks)).tolist()
        assert 4351 in ends, ends
        assert np.array_equal(e.turn_counts(4201, 400), series[4200:4600])
        assert e.snapshot() == (4600, int(series[-1]))
        assert np.array_equal(e.read_packed(), want)


# ------------------------------------------------------------------ 7. non-binary load
def test_nonbinary_load(gol, oracle):
    w, h, turns = 200, 77, 50
    rng = np.random.default_rng(77)
    board = np.where(rng.random((h, w)) < 0.4, 255, 0).astype(np.uint8)
    for y, x, v in ((0, 0, 1), (5, 17, 128), (64, 199, 254), (76, 100, 7), (33, 64, 200)):
        board[y, x] = v
    words, blocked, nb = oracle.pack(board)
    assert nb == 5
    want = oracle.bit_run(words, w, turns, blocked=blocked)
    assert not np.array_equal(want, oracle.bit_run(words, w, turns))     # (the mask matters)
    boards = []
    for flag in (True, False):
        with gol.Engine(w, h, device=0, resident=flag) as e:
            e.load(board)
            e.step(turns)
            ls = e.last_launches()
            if flag:
                assert ls[0][:2] == (1, 0)
                assert all(kern == KIND and k >= 2 for k, kern, _ in ls[1:]) and len(ls) >= 2
                assert sum(k for k, _, _ in ls) == turns
            boards.append(e.read_packed())
    assert np.array_equal(boards[0], boards[1])
    assert np.array_equal(boards[0], want)


# ------------------------------------------------------------------ 8. one-turn services
def test_one_turn_services_after_a_resident_step(gol, oracle):
    w, h = 200, 77
    start = oracle.gen_random(9, w, h)
    b64 = oracle.bit_run(start, w, 64)
    b65 = oracle.bit_run(b64, w, 1)
    with gol.Engine(w, h, device=0, resident=True) as e:
        e.load_packed(start)
        e.step(64)
        assert _resident_launches(e, 64) == [64]
        e.step(1)
        assert [k for k, _, _ in e.last_launches()] == [1]
        now, before = oracle.unpack(b65, w), oracle.unpack(b64, w)
        ys, xs = np.nonzero(now != before)
        assert len(xs) > 0
        assert np.array_equal(e.flipped_cells(), np.stack([xs, ys], axis=1).astype(np.int64))
        assert np.array_equal(e.alive_cells(), oracle.ref_alive_cells(now))
        x0, y0, ww, wh = 190, 70, 30, 20                 # across both wraps
        win = now[(y0 + np.arange(wh)) % h][:, (x0 + np.arange(ww)) % w]
        got, turn = e.read_window(x0, y0, ww, wh)
        assert turn == 65 and np.array_equal(got, win)
        block = 8
        dens, turn = e.window_density(x0, y0, ww, wh, block)
        want = np.zeros((-(-wh // block), -(-ww // block)), dtype=np.uint32)
        for by in range(want.shape[0]):
            for bx in range(want.shape[1]):
                want[by, bx] = (win[by * block:(by + 1) * block, bx * block:(bx + 1) * block] == 255).sum()
        assert turn == 65 and np.array_equal(dens, want)
        assert e.board_layout() == 0


# ------------------------------------------------------------------ 9. readers and control
def _wait_parked(e):
    t_end = time.time() + 10
    while not e.progress()[1] and time.time() < t_end:
        time.sleep(0.001)
    return e.progress()


def test_pause_before_the_step(gol, oracle):
    from gol import _native as N
    w, h = 200, 77
    start = oracle.gen_random(12, w, h)
    with gol.Engine(w, h, device=0, resident=True) as e:
        e.load_packed(start)
        e.set_control(N.GOL_CONTROL_PAUSE)
        res = {}
        th = threading.Thread(target=lambda: res.update(done=e.step(1000)), daemon=True)
        th.start()
        assert _wait_parked(e) == (0, True)
        board, turn = e.get_world()
        assert turn == 0 and np.array_equal(board, oracle.unpack(start, w))
        e.set_control(N.GOL_CONTROL_RUN)
        th.join(60)
        assert not th.is_alive() and res["done"] is True
        assert e.turn == 1000
        _resident_launches(e, 1000)
        assert np.array_equal(e.read_packed(), oracle.bit_run(start, w, 1000))


def test_get_world_during_a_step(gol, oracle):
    w = h = 64
    start = oracle.gen_random(13, w, h)
    with gol.Engine(w, h, device=0, resident=True) as e:
        e.load_packed(start)
        res = {}
        th = threading.Thread(target=lambda: res.update(done=e.step(200_000)), daemon=True)
        th.start()
        board, turn = e.get_world()
        th.join(60)
        assert not th.is_alive() and res["done"] is True
        assert 0 <= turn <= 200_000
        assert np.array_equal(board, oracle.unpack(oracle.bit_run(start, w, turn), w)), turn
        assert e.turn == 200_000
        assert np.array_equal(e.read_packed(), oracle.bit_run(start, w, 200_000))


def test_stop_ends_on_a_whole_launch(gol, oracle):
    from gol import _native as N
    w = h = 64
    start = oracle.gen_random(14, w, h)
    with gol.Engine(w, h, device=0, resident=True) as e:
        e.load_packed(start)
        e.set_control(N.GOL_CONTROL_RUN)
        res = {}
        th = threading.Thread(target=lambda: res.update(rc=e._L.gol_step(e.handle, 10 ** 8)),
                              daemon=True)
        th.start()
        t_end = time.time() + 10
        while e.progress()[0] == 0 and time.time() < t_end:
            time.sleep(0.0005)
        e.set_control(N.GOL_CONTROL_STOP)
        th.join(60)
        assert not th.is_alive() and res["rc"] == N.GOL_STOPPED
        turn = int(e.info().turn)
        cap = 4096
        arrs = [(ctypes.c_int32 * cap)() for _ in range(3)]
        n = e._L.gol_last_launches(e.handle, *arrs, cap)
        assert n >= 1 and turn < 10 ** 8
        assert all(arrs[0][i] == 256 and arrs[1][i] == KIND for i in range(min(n, cap)))
        assert turn == 256 * n                       # whole launches, nothing else
        assert np.array_equal(e.read_packed(), oracle.bit_run(start, w, turn))


# ------------------------------------------------------------------ 10. driver
@pytest.mark.parametrize("size", (64, 16))
@pytest.mark.parametrize("per_turn", (False, True), ids=("deep", "per_turn"))
def test_driver(gol, tmp_path, size, per_turn):
    """gol.Run(..., resident=True): FinalTurnComplete.Alive and the written PGM are the
    reference's check image after 100 turns (with TurnComplete events the driver steps turn by
    turn; without them the engine takes the turns in resident launches)."""
    img = tmp_path / "images"
    img.mkdir()
    (img / f"{size}x{size}.pgm").write_bytes(G.input_pgm_bytes(size))
    events = gol.Channel()
    p = gol.Params(Turns=100, Threads=8, ImageWidth=size, ImageHeight=size)
    hnd = gol.Run(p, events, None, image_dir=str(img), out_dir=str(tmp_path / "out"),
                  resident=True, emit_turn_complete=per_turn)
    evs = list(events)
    hnd.wait(5)
    assert hnd.error is None, hnd.error
    final = [ev for ev in evs if isinstance(ev, gol.FinalTurnComplete)]
    assert len(final) == 1
    ys, xs = np.nonzero(G.check_board(size, 100))
    assert set((c.X, c.Y) for c in final[0].Alive) == set(zip(xs.tolist(), ys.tolist()))
    out = tmp_path / "out" / f"{size}x{size}x100.pgm"
    assert out.read_bytes() == G.check_pgm_bytes(size, 100)
