"""The host side of k_step_tile's big form (board buffers of 2 GiB and more; no device): the
code list gol_tile_big_codes and the window arithmetic golk::tile_window through gol_tile_window,
the same function the kernel calls to base its buffer resources.

A tile at buffer row y0, th rows high, run K turns deep touches rows (y0 - K + j) mod modrows,
j = 0 .. th + 2K - 1.  The model below lists them one by one; the library must describe the same
rows as a first part from row0 and a second part from row 0, and the first part's base as a
64-bit byte count -- compared here as Python integers, which have no width to overflow."""
import ctypes
import random

import pytest


@pytest.fixture(scope="module")
def N():
    from gol import _native
    return _native


def _codes(N, fn):
    n = fn(None, 0)
    buf = (ctypes.c_int32 * n)()
    assert fn(buf, n) == n
    return tuple(buf)


def _window(N, modrows, pitch, y0, k, th):
    out = [ctypes.c_int64(-1) for _ in range(3)]
    base = ctypes.c_uint64(0xdeadbeef)
    rc = N.lib().gol_tile_window(modrows, pitch, y0, k, th, *(ctypes.byref(o) for o in out),
                                 ctypes.byref(base))
    return rc, tuple(o.value for o in out), base.value


def _model(modrows, y0, k, th):
    """(row0, rows_a, rows_b) from the listed rows: the run that starts at the window's first row
    and the run that starts at row 0 after the wrap."""
    rows = [(y0 - k + j) % modrows for j in range(th + 2 * k)]
    a = 1
    while a < len(rows) and rows[a] == rows[a - 1] + 1:
        a += 1
    assert rows[a:] == list(range(len(rows) - a))        # (the rest starts at row 0: one wrap)
    return rows[0], a, len(rows) - a


def test_big_codes_are_shipped_one_word_codes(N):
    big = _codes(N, N.lib().gol_tile_big_codes)
    assert set(big) <= set(_codes(N, N.lib().gol_tile_codes))
    assert all(c < 1000 for c in big) and len(set(big)) == len(big)
    assert {516, 524, 112, 16} <= set(big)
    assert N.lib().gol_tile_big_codes(None, -1) == N.GOL_EINVAL
    assert N.lib().gol_tile_big_codes(None, 1) == N.GOL_EINVAL


def _cases():
    rng = random.Random(20260)
    out = []
    # pitches (words) and row counts whose byte offsets pass 2^31, 2^32 and 2^40
    big = [(2048, 131072), (2048, 262400), (4096, 262144), (1 << 20, 1 << 17 | 5), (1 << 24, 70000),
           (3, 1 << 28), (1030, 1 << 30)]
    small = [(5, 77), (16, 200), (33, 77), (1, 3), (7, 1000)]
    for pitch, modrows in big + small:
        fit = min(modrows, ((1 << 31) - 1) // (pitch * 8))   # rows a window may span
        for _ in range(260):
            k = rng.randint(1, min(64, (fit - 1) // 2))
            th = rng.randint(1, min(fit - 2 * k, 4000))
            span = th + 2 * k
            y0 = rng.choice([0, rng.randint(0, k - 1) if k > 1 else 0,      # y0 - K < 0
                             (modrows - span + k) % modrows,               # ends exactly at modrows
                             (modrows - span + k + 1) % modrows,           # one row past it
                             modrows - 1, rng.randrange(modrows)])
            out.append((modrows, pitch, y0, k, th))
    return out


def test_window_matches_the_row_list(N):
    cases = _cases()
    assert len(cases) > 2500
    seen = dict(neg=0, exact=0, past=0, b31=0, b32=0, b40=0, wrap=0)
    for modrows, pitch, y0, k, th in cases:
        rc, (row0, ra, rb), base = _window(N, modrows, pitch, y0, k, th)
        assert rc == 0, (modrows, pitch, y0, k, th)
        assert (row0, ra, rb) == _model(modrows, y0, k, th), (modrows, pitch, y0, k, th)
        assert base == row0 * pitch * 8
        assert ra + rb == th + 2 * k and (ra + rb) * pitch * 8 < 1 << 31
        seen["neg"] += y0 - k < 0
        seen["exact"] += rb == 0 and row0 + ra == modrows
        seen["past"] += rb == 1
        seen["wrap"] += rb > 0
        seen["b31"] += base >= 1 << 31
        seen["b32"] += base >= 1 << 32
        seen["b40"] += base >= 1 << 40
    assert all(v > 20 for v in seen.values()), seen


def test_window_refusals(N):
    E = N.GOL_EINVAL
    ok = (262400, 2048, 1000, 20, 472)
    assert _window(N, *ok)[0] == 0
    # a window of 2 GiB or more: 131072 rows of 16 KiB are exactly 2^31 bytes
    assert _window(N, 1 << 20, 2048, 0, 20, 131072 - 40)[0] == E
    assert _window(N, 1 << 20, 2048, 0, 20, 131072 - 41)[0] == 0
    assert _window(N, 1 << 20, 1 << 28, 0, 2, 1)[0] == E              # one row of 2 GiB
    assert _window(N, 1 << 20, (1 << 60) + 1, 0, 2, 1)[0] == E        # (no overflow into "fits")
    # modrows < tile_h + 2 turns: the window would wrap twice
    assert _window(N, 77, 5, 0, 16, 46)[0] == E
    assert _window(N, 77, 5, 0, 16, 45)[0] == 0
    # arguments out of range
    for bad in [(262400, 2048, -1, 20, 472), (262400, 2048, 262400, 20, 472),
                (262400, 2048, 0, 0, 472), (262400, 2048, 0, 20, 0), (262400, 0, 0, 20, 472)]:
        rc, parts, base = _window(N, *bad)
        assert rc == E and parts == (0, 0, 0) and base == 0, bad
    assert N.lib().gol_tile_window(262400, 2048, 0, 20, 472, None, None, None, None) == E
