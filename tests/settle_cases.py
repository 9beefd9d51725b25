"""Boards and expected values shared by test_settle_cpu.py and test_gpu_settle.py (K1r2s:
gol_settle_*, k_settle_resident_batch).  Every expected value comes from the oracle: a start board
is stepped by oracle.bit_run one turn at a time with each board's bytes keyed in a dict, which
gives mu (the first turn of the cycle) and the period; settled_turn follows from the contract's
formula; the expected board at turn T is oracle.bit_run(start, width, T)."""
import functools

import numpy as np

import resident_cases as RC

GLIDERS = ((16, 16), (20, 12), (64, 48))         # period 4 lcm(W, H): 64, 240, 768
SOUP_SHAPES = ((16, 16), (64, 64), (65, 37), (130, 9), (200, 77))
SOUP_TURNS = 8192


def soup_seeds(shape):
    return RC.SEEDS[:2] if shape == (200, 77) else RC.SEEDS


def place(width, height, cells):
    """A packed board (height, nw) with the (row, col) cells alive, both taken modulo the board."""
    from oracle import oracle as O
    b = np.zeros((height, width), dtype=np.uint8)
    for r, c in cells:
        b[r % height, c % width] = 255
    words, _, nonbinary = O.pack(b)
    assert nonbinary == 0
    return words


def glider(width, height):
    return place(width, height, ((1, 2), (2, 3), (3, 1), (3, 2), (3, 3)))


def blinker(width, height, row, col, vertical=False):
    """Three cells around (row, col), in a row or in a column."""
    return place(width, height, [(row + d, col) if vertical else (row, col + d) for d in (-1, 0, 1)])


def block(width, height, row, col):
    return place(width, height, ((row, col), (row, col + 1), (row + 1, col), (row + 1, col + 1)))


def cycle(start, width, cap):
    """(mu, period) of the oracle's orbit of `start`, or None if no board repeats within `cap`
    turns."""
    from oracle import oracle as O
    seen = {}
    b = np.ascontiguousarray(start, dtype=np.uint64)
    for t in range(cap + 1):
        key = b.tobytes()
        if key in seen:
            return seen[key], t - seen[key]
        seen[key] = t
        b = O.bit_run(b, width, 1)
    return None


def brent(start_turn, mu, period):
    """settled_turn of a watch begun at start_turn on an orbit whose cycle begins mu turns after
    it: s_k + period for the least k with s_k >= mu and 2^k >= period (s_k = 2^k - 1 after the
    start)."""
    k = 0
    while not ((1 << k) - 1 >= mu and (1 << k) >= period):
        k += 1
    return start_turn + (1 << k) - 1 + period


def expected(start, width, cap, start_turn=0):
    """(settled_turn, period) the contract gives a watch of `start` begun at start_turn, or None
    if the oracle finds no cycle within `cap` turns."""
    c = cycle(start, width, cap)
    if c is None:
        return None
    return brent(start_turn, c[0], c[1]), c[1]


def entry(exp, now):
    """What gol_settle_read reports at turn `now` for a board whose expected() is exp."""
    if exp is None or exp[0] > now:
        return -1, 0
    return exp


@functools.lru_cache(maxsize=None)
def soup(seed, width, height):
    from oracle import oracle as O
    b = O.gen_random(seed, width, height)
    b.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def soup_expected(seed, width, height):
    """expected() of the soup within SOUP_TURNS; the guard: it must settle within the run."""
    exp = expected(soup(seed, width, height), width, SOUP_TURNS)
    assert exp is not None and exp[0] <= SOUP_TURNS, (seed, width, height, exp)
    return exp


# ------------------------------------------------------------------ the (nw, R) class sweep
CLASS_WIDTHS = {1: 64, 2: 128, 3: 191, 4: 255}


def class_shapes(extra=()):
    """(width, height) for every (nw, R) class the kernels are built for: height 256 R - 3 (256
    lanes or 255, the last lane short where R > 1), and the `extra` shapes."""
    out = []
    for nw, width in CLASS_WIDTHS.items():
        for r in range(1, 17):
            if r * nw <= 16 and (r & (r - 1) == 0 or r == 16 // nw):
                height = 256 * r - 3
                lanes, rows, waves = RC.plan(width, height)
                assert rows == r and waves == 4 and (r == 1 or height % r != 0), (width, height)
                out.append((width, height))
    return tuple(out) + tuple(extra)


def class_boards(width, height):
    """[(name, start board, expected period)]: a dead board but for one blinker -- in lane 0,
    across the boundary of waves 0 and 1, in the last (short) lane, in the row's last word and
    over the seam -- the same with a block, and the dead board."""
    lanes, rows, waves = RC.plan(width, height)
    assert waves >= 2
    inner = 1 if rows >= 3 else 0                # a row with both neighbours in the lane
    spots = (("lane0", inner, 5, False),
             ("waves01", 64 * rows - 1, 7, True),          # rows 64R - 2 .. 64R: lanes 63 and 64
             ("lastlane", height - 1, 9, False),
             ("seam", height // 2, width - 1, False))      # columns width - 2, width - 1, 0
    out = []
    for name, row, col, vertical in spots:
        out.append(("blinker-" + name, blinker(width, height, row, col, vertical), 2))
    for name, row, col, vertical in spots:
        out.append(("block-" + name, block(width, height, row - (1 if name == "lastlane" else 0), col), 1))
    out.append(("dead", np.zeros((height, RC.nwords(width)), dtype=np.uint64), 1))
    return out
