"""K1r2s where it needs no device: the argument checks of gol_settle_*, and gol_settle_host_run --
the host build of k_settle_resident_batch, the waves' compare words, the reload of the state at
every launch and the skip of settled turns included -- against the oracle: the period, the turn
it is found at and the board at the end (settle_cases)."""
import ctypes as C

import numpy as np
import pytest

import resident_cases as RC
import settle_cases as SC


@pytest.fixture(scope="module")
def lib():
    from gol import _native as N
    return N.lib(), N


def host_run(lib, start, width, turns, depth):
    """(board, settled_turn, period) of gol_settle_host_run."""
    L, N = lib
    start = np.ascontiguousarray(start, dtype=np.uint64)
    out = np.zeros_like(start)
    t, p = C.c_int64(-7), C.c_int64(-7)
    rc = L.gol_settle_host_run(start.ctypes.data_as(N._u64p), width, start.shape[0], turns, depth,
                               out.ctypes.data_as(N._u64p), C.byref(t), C.byref(p))
    assert rc == N.GOL_OK, (width, start.shape, turns, depth)
    return out, t.value, p.value


# ------------------------------------------------------------------ 1. argument checks
def test_null_handles(lib):
    L, N = lib
    a, b = (C.c_int64 * 4)(), (C.c_int64 * 4)()
    assert L.gol_settle_step(None, 1) == N.GOL_EINVAL
    assert L.gol_settle_step(None, -1) == N.GOL_EINVAL
    assert L.gol_settle_read(None, 0, 1, a, b) == N.GOL_EINVAL
    assert L.gol_settle_read(None, 0, 1, None, None) == N.GOL_EINVAL
    # (the names tests/test_batch_cpu.py pins keep their prefix to themselves)
    assert not [n for n in N.header_functions() if n.startswith("gol_batch_settle")]


def test_host_run_argument_checks(lib):
    L, N = lib
    words = (C.c_uint64 * 64)()
    out = (C.c_uint64 * 64)()
    t, p = C.c_int64(), C.c_int64()

    def run(width=16, height=16, turns=4, depth=256, src=words, dst=out):
        return L.gol_settle_host_run(src, width, height, turns, depth, dst, C.byref(t), C.byref(p))

    assert run() == N.GOL_OK
    assert L.gol_settle_host_run(words, 16, 16, 4, 256, out, None, None) == N.GOL_OK
    assert run(src=None) == N.GOL_EINVAL
    assert run(dst=None) == N.GOL_EINVAL
    assert run(turns=-1) == N.GOL_EINVAL
    assert run(turns=0) == N.GOL_OK
    for depth in (0, -1, 257, 1 << 20):
        assert run(depth=depth) == N.GOL_EINVAL, depth
    for depth in (1, 255, 256):
        assert run(depth=depth) == N.GOL_OK, depth
    for width, height in ((1, 16), (256, 16), (0, 16), (16, 0), (16, -1)):   # gol_resident_plan's
        assert run(width=width, height=height) == N.GOL_EINVAL, (width, height)
    assert RC.plan(64, RC.limit(64) + 1) is None
    big = (C.c_uint64 * (RC.limit(64) + 1))()
    assert L.gol_settle_host_run(big, 64, RC.limit(64) + 1, 1, 256, big, None, None) == N.GOL_EINVAL


# ------------------------------------------------------------------ 2. gliders
@pytest.mark.parametrize("depth", (1, 7, 256))
@pytest.mark.parametrize("shape,period,settled", zip(SC.GLIDERS, (64, 240, 768), (127, 495, 1791)),
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_gliders(lib, oracle, shape, period, settled, depth):
    width, height = shape
    start = SC.glider(width, height)
    lcm = width * height // np.gcd(width, height)
    assert period == 4 * lcm
    assert SC.cycle(start, width, 2048) == (0, period)           # the oracle: mu = 0
    assert SC.expected(start, width, 2048) == (settled, period)  # the formula
    got, t, p = host_run(lib, start, width, 2048, depth)
    print(f"{width}x{height} depth {depth}: settled_turn {t}, period {p}")
    assert (t, p) == (settled, period)
    assert np.array_equal(got, oracle.bit_run(start, width, 2048))
    # a run that ends at the match reports it; one turn less does not
    got, t, p = host_run(lib, start, width, settled, depth)
    assert (t, p) == (settled, period)
    assert np.array_equal(got, oracle.bit_run(start, width, settled))
    got, t, p = host_run(lib, start, width, settled - 1, depth)
    assert (t, p) == (-1, 0)
    assert np.array_equal(got, oracle.bit_run(start, width, settled - 1))


# ------------------------------------------------------------------ 3. soups
@pytest.mark.parametrize("depth", (256, 37))
@pytest.mark.parametrize("shape", SC.SOUP_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_soups(lib, oracle, shape, depth):
    width, height = shape
    for seed in SC.soup_seeds(shape):
        start = SC.soup(seed, width, height)
        exp = SC.soup_expected(seed, width, height)              # (the guard: it settles)
        assert exp[0] <= 4097 and exp[1] >= 1, (shape, seed, exp)
        got, t, p = host_run(lib, start, width, SC.SOUP_TURNS, depth)
        print(f"{width}x{height} seed {seed} depth {depth}: settled_turn {t}, period {p}; oracle {exp}")
        assert (t, p) == exp, (shape, seed)
        assert np.array_equal(got, oracle.bit_run(start, width, SC.SOUP_TURNS)), (shape, seed)


def test_not_settled_within_the_run(lib, oracle):
    width = height = 64
    for seed in RC.SEEDS:
        exp = SC.soup_expected(seed, width, height)
        turns = exp[0] - 1                                       # one turn short of the match
        assert turns >= 256
        got, t, p = host_run(lib, SC.soup(seed, width, height), width, turns, 256)
        assert (t, p) == (-1, 0), seed
        assert np.array_equal(got, oracle.bit_run(SC.soup(seed, width, height), width, turns)), seed


# ------------------------------------------------------------------ 4. the compare, per class
@pytest.mark.parametrize("shape", SC.class_shapes(), ids=lambda s: f"{s[0]}x{s[1]}")
def test_compare_covers_every_lane_row_and_word(lib, oracle, shape):
    width, height = shape
    for name, start, period in SC.class_boards(width, height):
        exp = SC.expected(start, width, 16)
        assert exp == ((3, 2) if period == 2 else (1, 1)), name  # the oracle and the formula
        for depth in (256, 3):
            got, t, p = host_run(lib, start, width, 8, depth)
            assert (t, p) == exp, (shape, name, depth)
            assert np.array_equal(got, oracle.bit_run(start, width, 8)), (shape, name, depth)
