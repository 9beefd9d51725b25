"""k_step_resident (GOL_FLAG_RESIDENT), the parts that need no device: gol_resident_plan (how a
board narrower than 256 cells is partitioned over the lanes of one workgroup) and
gol_resident_host_run (the host build of the kernel's own turn: the same partition, in-lane
west / east words, row sums, rule and tail mask, run lane by lane over arrays indexed like the
kernel's LDS exchange area) against oracle.bit_run, boards and per-turn counts."""
import ctypes as C

import numpy as np
import pytest

import resident_cases as RC

TURNS = (1, 2, 7)


def _native():
    from gol import _native as N
    return N


def _host_run(board, width, turns, counts=True):
    N = _native()
    b = np.ascontiguousarray(board, dtype=np.uint64)
    out = np.zeros_like(b)
    cnt = np.full(max(turns, 1), -1, dtype=np.int64)
    rc = N.lib().gol_resident_host_run(b.ctypes.data_as(N._u64p), width, b.shape[0], turns,
                                       out.ctypes.data_as(N._u64p),
                                       cnt.ctypes.data_as(N._i64p) if counts else None)
    assert rc == N.GOL_OK
    return out, cnt[:turns]


def test_exports_declared():
    N = _native()
    for name in ("gol_resident_plan", "gol_resident_host_run"):
        assert name in N.header_functions()
        assert name in N.SIGNATURES
    assert N.GOL_FLAG_RESIDENT == 0x8


# ------------------------------------------------------------------ gol_resident_plan
def test_plan_invariants():
    """Every width 2 .. 255 x the heights around the wave and lane counts and each word count's
    limit: at most 256 lanes of at most 16 words, the last lane owns a row, no lane lies wholly
    past the board, waves = ceil(lanes / 64); GOL_EINVAL exactly past the limits."""
    limits = sorted({256 * (16 // nw) for nw in (1, 2, 3, 4)})
    assert limits == [1024, 1280, 2048, 4096]
    heights = [1, 2, 3, 63, 64, 65, 255, 256, 257] + limits + [h + 1 for h in limits]
    for width in range(2, 256):
        nw = RC.nwords(width)
        for h in heights:
            p = RC.plan(width, h)
            if h > RC.limit(width):
                assert p is None, (width, h)
                continue
            assert p is not None, (width, h)
            lanes, rows, waves = p
            assert 1 <= lanes <= 256, (width, h, p)
            assert rows >= 1 and rows * nw <= 16, (width, h, p)
            assert (lanes - 1) * rows < h <= lanes * rows, (width, h, p)
            assert waves == -(-lanes // 64), (width, h, p)
    for width, h in ((256, 64), (257, 1), (4096, 4096), (1, 16), (0, 16), (-5, 16), (64, 0), (64, -1)):
        assert RC.plan(width, h) is None, (width, h)
    for width in (64, 128, 192, 255):
        assert RC.plan(width, RC.limit(width)) is not None
        assert RC.plan(width, RC.limit(width) + 1) is None


def test_plan_rejects_null_pointers():
    N = _native()
    a = C.c_int32()
    assert N.lib().gol_resident_plan(64, 64, None, C.byref(a), C.byref(a)) == N.GOL_EINVAL
    assert N.lib().gol_resident_plan(64, 64, C.byref(a), None, C.byref(a)) == N.GOL_EINVAL
    assert N.lib().gol_resident_plan(64, 64, C.byref(a), C.byref(a), None) == N.GOL_EINVAL


def test_host_run_rejects_ineligible_boards():
    N = _native()
    b = np.zeros((4, 5), dtype=np.uint64)
    p = b.ctypes.data_as(N._u64p)
    f = N.lib().gol_resident_host_run
    assert f(p, 256, 4, 1, p, None) == N.GOL_EINVAL
    assert f(p, 1, 4, 1, p, None) == N.GOL_EINVAL
    assert f(p, 64, 4097, 1, p, None) == N.GOL_EINVAL
    assert f(None, 64, 4, 1, p, None) == N.GOL_EINVAL
    assert f(p, 64, 4, -1, p, None) == N.GOL_EINVAL


# ------------------------------------------------------------------ gol_resident_host_run
@pytest.mark.parametrize("width", RC.WIDTHS)
def test_host_run_matches_oracle(width):
    """Boards and per-turn counts at every height of the list, the width's limit and a height
    with a ragged last lane, 1, 2 and 7 turns.  Seeds: 1, and on to the first seed with a live
    case (the guard: checked on the oracle's side for every shape but the exhaustive ones)."""
    for height in RC.heights_for(width):
        seeds = [1]
        if (width, height) not in RC.TINY:
            s = RC.live_seed(width, height, TURNS)
            seeds = sorted({1, s})
        for seed in seeds:
            start, _ = RC.oracle_run(seed, width, height, 0)
            for turns in TURNS:
                want, want_counts = RC.oracle_run(seed, width, height, turns)
                got, got_counts = _host_run(start, width, turns)
                assert np.array_equal(got, want), (width, height, seed, turns)
                assert np.array_equal(got_counts, want_counts), (width, height, seed, turns)


def test_host_run_ragged_last_lane_is_exercised():
    """The ragged heights of the sweep really leave the last lane short (from the plan)."""
    for width in (64, 128, 192, 255):
        h = RC.ragged_height(width)
        lanes, rows, _ = RC.plan(width, h)
        assert 0 < h - (lanes - 1) * rows < rows


def test_host_run_zero_turns_and_no_counts():
    from oracle import oracle as O
    start = O.gen_random(3, 200, 77)
    got, _ = _host_run(start, 200, 0, counts=False)
    assert np.array_equal(got, start)
    got, _ = _host_run(start, 200, 5, counts=False)
    assert np.array_equal(got, O.bit_run(start, 200, 5))


@pytest.mark.parametrize("shape", RC.TINY, ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_run_exhaustive_tiny_boards(shape, oracle):
    """Every start board of 2x1, 3x1, 2x2 and 3x2 for 1, 2 and 3 turns (random boards of these
    shapes die within three turns): width 2 counts its one x neighbour twice, height 1 is its own
    north and south row, height 2 has one row as both."""
    width, height = shape
    alive = 0
    for start in RC.tiny_boards(width, height):
        for turns in (1, 2, 3):
            want, want_counts = oracle.bit_run(start, width, turns, counts=True)
            got, got_counts = _host_run(start, width, turns)
            assert np.array_equal(got, want), (shape, start.tolist(), turns)
            assert np.array_equal(got_counts, np.asarray(want_counts, dtype=np.int64))
            alive += int(want.any())
    assert alive > 0
