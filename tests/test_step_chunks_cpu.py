"""The chunk plan of gol_step's chunked pipeline (goleng::chunk_bounds / chunk_deps through
gol_step_chunk_plan; no device), checked by brute force over rows.

Launch n reads board A and writes board B; launch n + 1 reads B and writes A.  A chunk with
output rows [lo, hi) of a launch of K turns reads rows lo - K .. hi + K - 1 (modulo the buffer
rows) and writes rows lo .. hi - 1.  Chunk q of the next launch must follow chunk p of the
previous one when q reads a row p wrote, or writes a row p read.
"""
import ctypes

import pytest

from gol import _native as N


def _plan(rows, kp, thp, np_, kn, thn, nn):
    cap = max(np_, nn)
    counts = (ctypes.c_int32 * 2)()
    pb = (ctypes.c_int32 * (cap + 1))()
    nb = (ctypes.c_int32 * (cap + 1))()
    deps = (ctypes.c_uint8 * (cap * cap))()
    rc = N.lib().gol_step_chunk_plan(rows, kp, thp, np_, kn, thn, nn, counts, pb, nb, deps, cap)
    assert rc == N.GOL_OK
    a, b = counts[0], counts[1]
    return (list(pb[:a + 1]), list(nb[:b + 1]),
            [[p for p in range(a) if deps[q * cap + p]] for q in range(b)])


def _rows(lo, hi, rows):
    return {r % rows for r in range(lo, hi)}


def _check(rows, kp, thp, np_, kn, thn, nn):
    pb, nb, deps = _plan(rows, kp, thp, np_, kn, thn, nn)
    for bounds, th, want in ((pb, thp, np_), (nb, thn, nn)):
        n = len(bounds) - 1
        assert 1 <= n <= want
        assert bounds[0] == 0 and bounds[-1] == rows
        assert all(lo < hi for lo, hi in zip(bounds, bounds[1:]))
        assert all(b % th == 0 for b in bounds[:-1])
        if n > 1:
            assert all(hi - lo >= max(kp, kn) for lo, hi in zip(bounds, bounds[1:]))
            # the tile rows spread evenly: floor(tile rows / n) each, one more for the last
            # tile rows % n chunks
            base, extra = divmod(-(-rows // th), n)
            sizes = [base + (i >= n - extra) for i in range(n)]
            assert bounds[:-1] == [sum(sizes[:i]) * th for i in range(n)]
    wrote = [_rows(lo, hi, rows) for lo, hi in zip(pb, pb[1:])]
    read = [_rows(lo - kp, hi + kp, rows) for lo, hi in zip(pb, pb[1:])]
    for q, (lo, hi) in enumerate(zip(nb, nb[1:])):
        q_reads, q_writes = _rows(lo - kn, hi + kn, rows), _rows(lo, hi, rows)
        need = [p for p in range(len(wrote)) if wrote[p] & q_reads or read[p] & q_writes]
        assert deps[q] == need, (q, deps[q], need)
    return pb, nb, deps


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 8])
def test_equal_shapes(n):
    """16 tile rows of 40 at K = 6: n chunks as asked; with 2 or 3 chunks on the torus every
    chunk follows all of them, with more only its neighbours and itself."""
    pb, nb, deps = _check(640, 6, 40, n, 6, 40, n)
    assert len(pb) - 1 == len(nb) - 1 == n
    if n == 1:
        assert deps == [[0]]
    elif n <= 3:
        assert all(d == list(range(n)) for d in deps)
    else:
        assert all(sorted(d) == sorted({(q - 1) % n, q, (q + 1) % n}) for q, d in enumerate(deps))


@pytest.mark.parametrize("rows,th,n", [(203, 40, 5), (203, 40, 3), (270, 40, 6), (1000, 48, 7)])
def test_ragged_last_tile_row(rows, th, n):
    """The last tile row is short: it belongs to the last chunk."""
    pb, nb, _ = _check(rows, 6, th, n, 5, th, n)
    assert len(pb) - 1 == n and pb == nb
    assert rows % th and pb[-1] - pb[-2] > rows % th


@pytest.mark.parametrize("first", [(30, 452), (20, 472)])
@pytest.mark.parametrize("n", [2, 5, 10, 20])
def test_pinned_65536_pair(first, n):
    """The 65536-row board's two pinned shapes after each other, either way round, and each
    after itself: different depths and tile heights, so the bounds do not line up."""
    second = (20, 472) if first == (30, 452) else (30, 452)
    for nxt in (second, first):
        pb, nb, deps = _check(65536, first[0], first[1], n, nxt[0], nxt[1], n)
        assert len(pb) - 1 == len(nb) - 1 == n
        if n >= 5:
            assert all(1 <= len(d) < n for d in deps), deps    # neighbours, never all


def test_even_spread():
    """145 tile rows in 20 chunks: fifteen of 7 and five of 8, not nineteen of 7 and one of 12."""
    pb, _, _ = _check(65536, 30, 452, 20, 30, 452, 20)
    tile_rows = [-(-(hi - lo) // 452) for lo, hi in zip(pb, pb[1:])]
    assert tile_rows == [7] * 15 + [8] * 5


def test_more_chunks_than_fit():
    """Fewer chunks than asked when they would be shorter than the deeper launch's turns, or
    than one tile row; one chunk when two do not fit."""
    pb, nb, _ = _check(203, 6, 40, 64, 6, 40, 64)      # 6 tile rows, the last one 3 rows
    assert len(pb) - 1 == len(nb) - 1 == 5
    pb, nb, _ = _check(280, 6, 40, 64, 6, 40, 64)
    assert len(pb) - 1 == 7
    pb, nb, _ = _check(640, 30, 16, 40, 6, 40, 16)     # 16-row tiles: two tile rows per chunk
    assert len(pb) - 1 == 20 and len(nb) - 1 == 16
    pb, nb, deps = _check(50, 30, 16, 4, 30, 16, 4)
    assert pb == nb == [0, 50] and deps == [[0]]


def test_bad_arguments():
    L = N.lib()
    c = (ctypes.c_int32 * 2)()
    b = (ctypes.c_int32 * 5)()
    d = (ctypes.c_uint8 * 16)()
    assert L.gol_step_chunk_plan(640, 6, 40, 4, 6, 40, 4, c, b, b, d, 4) == N.GOL_OK
    assert L.gol_step_chunk_plan(640, 6, 40, 5, 6, 40, 4, c, b, b, d, 4) == N.GOL_EINVAL
    assert L.gol_step_chunk_plan(0, 6, 40, 4, 6, 40, 4, c, b, b, d, 4) == N.GOL_EINVAL
    assert L.gol_step_chunk_plan(640, 0, 40, 4, 6, 40, 4, c, b, b, d, 4) == N.GOL_EINVAL
    assert L.gol_step_chunk_plan(640, 6, 40, 4, 6, 40, 4, None, b, b, d, 4) == N.GOL_EINVAL
