"""Shapes and helpers shared by test_resident_cpu.py and test_gpu_resident.py (k_step_resident,
GOL_FLAG_RESIDENT): the width and height lists, the partition read through gol_resident_plan,
the oracle's boards with the liveness guard, and the exhaustive tiny boards."""
import ctypes as C
import functools

import numpy as np

WIDTHS = (2, 3, 5, 16, 63, 64, 65, 127, 128, 129, 191, 192, 193, 200, 255)
HEIGHTS = (1, 2, 3, 5, 63, 64, 65, 77, 130, 257)
TINY = ((2, 1), (3, 1), (2, 2), (3, 2))          # (width, height): every start board is run
SEEDS = tuple(range(1, 9))


def nwords(width):
    return (width + 63) // 64


def limit(width):
    """The tallest resident board of that width: 256 lanes x floor(16 / words per row) rows."""
    return 256 * (16 // nwords(width))


def plan(width, height):
    """(lanes, rows per lane, waves) from gol_resident_plan, or None where it says GOL_EINVAL."""
    from gol import _native as N
    a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
    rc = N.lib().gol_resident_plan(width, height, C.byref(a), C.byref(b), C.byref(c))
    if rc == N.GOL_EINVAL:
        return None
    assert rc == N.GOL_OK
    return a.value, b.value, c.value


def ragged_height(width):
    """A height whose last lane owns fewer rows than the others (asserted from the plan)."""
    h = limit(width) - 1
    lanes, rows, _ = plan(width, h)
    assert rows > 1 and h % rows != 0 and lanes * rows > h
    return h


def heights_for(width):
    """HEIGHTS, the width's limit and one height with a ragged last lane."""
    return tuple(dict.fromkeys(HEIGHTS + (limit(width), ragged_height(width))))


def height_with_lanes(width, lanes):
    """The smallest height gol_resident_plan partitions into exactly `lanes` lanes."""
    for h in range(1, limit(width) + 1):
        if plan(width, h)[0] == lanes:
            return h
    raise AssertionError(f"no height of width {width} has {lanes} lanes")


@functools.lru_cache(maxsize=None)
def _oracle_run(seed, width, height, turns):
    from oracle import oracle as O
    board, counts = O.bit_run(O.gen_random(seed, width, height), width, turns, counts=True)
    board.setflags(write=False)
    counts = np.asarray(counts[:turns], dtype=np.int64)
    counts.setflags(write=False)
    return board, counts


def oracle_run(seed, width, height, turns):
    """(board, per-turn counts) of gen_random(seed) after `turns` turns; shared and read-only."""
    if turns == 0:
        from oracle import oracle as O
        return O.gen_random(seed, width, height), np.zeros(0, dtype=np.int64)
    return _oracle_run(seed, width, height, turns)


def is_live(seed, width, height, turns):
    """The oracle's board after `turns` turns has live cells and differs from the turn before."""
    now, _ = oracle_run(seed, width, height, turns)
    before, _ = oracle_run(seed, width, height, turns - 1)
    return bool(now.any()) and not np.array_equal(now, before)


def live_seed(width, height, turns_list):
    """The first seed of SEEDS with a live (seed, turns) case for that shape; the guard fails the
    test where no seed has one, so an empty or frozen board cannot pass a case."""
    for seed in SEEDS:
        if any(is_live(seed, width, height, t) for t in turns_list):
            return seed
    raise AssertionError(f"{width}x{height}: no live case among seeds {SEEDS}, turns {turns_list}")


def tiny_boards(width, height):
    """Every start board of a tiny shape, packed: (2^(W H), H, 1) uint64."""
    n = 1 << (width * height)
    out = np.zeros((n, height, 1), dtype=np.uint64)
    mask = (1 << width) - 1
    for b in range(n):
        for y in range(height):
            out[b, y, 0] = (b >> (y * width)) & mask
    return out
