"""Structured boards and read-out checks shared by tests/test_gpu_io.py (in its own process and
in the child processes it starts on the small-staging library) and the CPU cross-check in
tests/test_oracle.py.

The boards are the edge contents of the load / read-out / count kernels (k_pack, k_unpack,
k_popcount, k_row_popcount, k_alive_scatter): nothing alive, everything alive, one cell in a
corner, only the last valid bit of every row's last word, the columns around a word boundary,
rows with equal alive-list offsets, a sparse and a dense random board.
"""
import numpy as np


def _empty(w, h):
    return np.zeros((h, w), dtype=np.uint8)


def _full(w, h):
    return np.full((h, w), 255, dtype=np.uint8)


def _first_cell(w, h):
    b = _empty(w, h)
    b[0, 0] = 255
    return b


def _last_cell(w, h):
    b = _empty(w, h)
    b[h - 1, w - 1] = 255
    return b


def _last_bit(w, h):
    """Only cell w-1 of every row: the last valid bit of the row's last word."""
    b = _empty(w, h)
    b[:, w - 1] = 255
    return b


def _word_edges(w, h):
    """Columns 63 / 64 / 65 (where the board has them) and w-1."""
    b = _empty(w, h)
    for x in (63, 64, 65, w - 1):
        if x < w:
            b[:, x] = 255
    return b


def _alt_rows(w, h):
    """Rows 0, 2, 4, ... full and the others empty: the alive list's row offsets repeat."""
    b = _empty(w, h)
    b[0::2] = 255
    return b


def _random(density):
    def make(w, h):
        rng = np.random.default_rng(1000003 * w + 101 * h + int(density * 64))
        return np.where(rng.random((h, w)) < density, 255, 0).astype(np.uint8)
    return make


MAKERS = {
    "empty": _empty,
    "full": _full,
    "first_cell": _first_cell,
    "last_cell": _last_cell,
    "last_bit": _last_bit,
    "word_edges": _word_edges,
    "alt_rows": _alt_rows,
    "random16": _random(1.0 / 16),
    "random50": _random(0.5),
}

NONBINARY_BYTES = np.array([0, 255, 1, 7, 128, 254], dtype=np.uint8)
NONBINARY_P = [0.45, 0.35, 0.05, 0.05, 0.05, 0.05]


def nonbinary_board(w, h):
    """The byte mix of test_gpu_engine.py::test_nonbinary_cells."""
    rng = np.random.default_rng(w + h)
    return rng.choice(NONBINARY_BYTES, size=(h, w), p=NONBINARY_P)


def np_alive_cells(board, row_offset=0):
    """Plain numpy restatement of the alive list: row-major (n, 2) int64 {x, y}."""
    yx = np.argwhere(np.asarray(board) == 255)
    out = yx[:, ::-1].astype(np.int64)
    out[:, 1] += row_offset
    return np.ascontiguousarray(out)


def check_readouts(O, e, want, turn, row_offset=0, tag=""):
    """The four read-outs of engine `e` against the byte board `want` (its owned rows; 0 / 255
    only) at `turn`: packed words (oracle.pack `O.pack`), bytes, (turn, alive) and the alive
    list (np_alive_cells, cross-checked against the oracle in tests/test_oracle.py)."""
    want = np.ascontiguousarray(want, dtype=np.uint8)
    packed = e.read_packed()
    assert packed.shape == (want.shape[0], (want.shape[1] + 63) // 64), (tag, packed.shape)
    assert np.array_equal(packed, O.pack(want)[0]), (tag, "read_packed")
    assert np.array_equal(e.read_board(), want), (tag, "read_board")
    assert e.snapshot() == (turn, int((want == 255).sum())), (tag, "snapshot", e.snapshot())
    cells = e.alive_cells()
    exp = np_alive_cells(want, row_offset)
    assert cells.shape == exp.shape, (tag, "alive_cells", cells.shape, exp.shape)
    assert np.array_equal(cells, exp), (tag, "alive_cells")


def alive_cells_capped(e, cap, canary=-7777, slack=8):
    """gol_alive_cells through the raw ABI with room for `cap` pairs in a canary-filled array
    `slack` pairs longer.  Returns (total, the whole array as (cap + slack, 2))."""
    import ctypes
    from gol import _native as N
    buf = np.full((cap + slack, 2), canary, dtype=np.int64)
    n = ctypes.c_int64(-1)
    rc = N.lib().gol_alive_cells(e.handle, buf.ctypes.data_as(N._i64p), int(cap), ctypes.byref(n))
    N.check(rc, e.handle)
    return int(n.value), buf


def check_capped(e, want, cap, row_offset=0, tag=""):
    """`*n` is the total, the first min(n, cap) pairs are the list's head, and nothing is
    written past them."""
    exp = np_alive_cells(want, row_offset)
    total, buf = alive_cells_capped(e, cap)
    assert total == len(exp), (tag, cap, total, len(exp))
    k = min(total, cap)
    assert np.array_equal(buf[:k], exp[:k]), (tag, cap, "head")
    assert (buf[k:] == -7777).all(), (tag, cap, "wrote past min(n, cap) pairs")
