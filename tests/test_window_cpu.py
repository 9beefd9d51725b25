"""The window calls on the CPU: the six functions are exported, and gol_window_word -- the host
build of the function the window kernels fetch their cells with (golk::window_word) -- agrees
with a bit model at every seam position.

The model is numpy: the row's cells as a 0 / 1 vector, np.roll'ed so that column `col` comes
first, the first 64 taken (a row narrower than 64 cells repeats: np.resize).  The interleaved
input is built in numpy too (even cells in a word's low dword, odd cells in the high one), so no
expected value comes from the library.
"""
import ctypes

import numpy as np
import pytest

from gol import _native as N

NAMES = ("gol_read_window", "gol_window_density", "gol_write_window", "gol_clear",
         "gol_board_layout", "gol_window_word")
# every r = width % 64 on rows of 5 words (4 whole words when r = 0), and the narrow rows: one
# that wraps 32 times, 63 / 64 / 65 round one word, 130 = two words and 2 cells
WIDTHS = tuple(range(256, 320)) + (2, 63, 64, 65, 130)


def test_window_functions_exported():
    L = N.lib()
    for name in NAMES:
        assert name in N.header_functions()
        assert name in N.SIGNATURES
        assert hasattr(L, name)


def _pack_std(bits):
    """cells (0 / 1) -> words of the standard layout (cell x = bit x % 64 of word x / 64)."""
    nw = (len(bits) + 63) // 64
    padded = np.zeros(nw * 64, np.uint8)
    padded[:len(bits)] = bits
    return np.packbits(padded.reshape(nw, 64), axis=1, bitorder="little").view(np.uint64).ravel()


def _pack_il(bits):
    """cells -> words of the interleaved layout: cell 2 i of a word -> bit i, cell 2 i + 1 ->
    bit 32 + i."""
    nw = (len(bits) + 63) // 64
    padded = np.zeros(nw * 64, np.uint8)
    padded[:len(bits)] = bits
    cells = padded.reshape(nw, 32, 2)
    il = np.concatenate([cells[:, :, 0], cells[:, :, 1]], axis=1)
    return np.packbits(il, axis=1, bitorder="little").view(np.uint64).ravel()


def test_interleaved_builder_is_the_documented_layout():
    """(the test's own builder) one cell set -> the documented bit."""
    for cell, bit in ((0, 0), (1, 32), (2, 1), (63, 63), (62, 31), (64 + 5, 64 + 32 + 2)):
        bits = np.zeros(128, np.uint8)
        bits[cell] = 1
        words = _pack_il(bits)
        assert int(words[bit // 64]) == 1 << (bit % 64), (cell, bit)
        assert int(_pack_std(bits)[cell // 64]) == 1 << (cell % 64)


@pytest.mark.parametrize("layout", [0, 1], ids=["standard", "interleaved"])
def test_window_word_against_bit_model(layout):
    L = N.lib()
    rng = np.random.default_rng(2024 + layout)
    out = ctypes.c_uint64()
    weights = np.uint64(1) << np.arange(64, dtype=np.uint64)
    for width in WIDTHS:
        bits = rng.integers(0, 2, width).astype(np.uint8)
        if width >= 64:
            assert 0 < int(bits.sum()) < width               # (alive and dead cells both)
        else:
            bits[0], bits[-1] = 1, 0
        words = np.ascontiguousarray(_pack_il(bits) if layout else _pack_std(bits))
        ptr = words.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
        for col in range(width):
            want_bits = np.resize(np.roll(bits, -col), 64)
            want = int((want_bits.astype(np.uint64) * weights).sum())
            assert L.gol_window_word(ptr, width, col, layout, ctypes.byref(out)) == N.GOL_OK
            assert out.value == want, (width, col, layout, hex(out.value), hex(want))


def test_window_word_ignores_padding_bits():
    """Set padding bits in the input (the board never has them) do not reach the answer."""
    L = N.lib()
    width = 100
    bits = np.zeros(width, np.uint8)
    bits[[0, 99]] = 1
    words = _pack_std(bits).copy()
    words[1] |= np.uint64(0xFFFFFFF000000000)               # bits 36 .. 63: past cell 99
    out = ctypes.c_uint64()
    ptr = words.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    assert L.gol_window_word(ptr, width, 64, 0, ctypes.byref(out)) == N.GOL_OK
    # cells 64 .. 99 (36 cells, cell 99 alive), then cells 0 .. 27 (cell 0 alive)
    assert out.value == (1 << 35) | (1 << 36)


def test_window_word_refusals():
    L = N.lib()
    words = (ctypes.c_uint64 * 5)()
    out = ctypes.c_uint64()
    ok = (words, 300, 0, 0, ctypes.byref(out))
    assert L.gol_window_word(*ok) == N.GOL_OK
    bad = [(None, 300, 0, 0, ctypes.byref(out)),            # null row
           (words, 300, 0, 0, None),                        # null out
           (words, 1, 0, 0, ctypes.byref(out)),             # width < 2
           (words, 0, 0, 0, ctypes.byref(out)),
           (words, 300, -1, 0, ctypes.byref(out)),          # col outside [0, width)
           (words, 300, 300, 0, ctypes.byref(out)),
           (words, 300, 0, 2, ctypes.byref(out)),           # unknown layout
           (words, 300, 0, -1, ctypes.byref(out))]
    for args in bad:
        assert L.gol_window_word(*args) == N.GOL_EINVAL, args[1:4]


def test_window_calls_refuse_null_engine():
    """Argument checks that need no device."""
    L = N.lib()
    buf = (ctypes.c_uint8 * 16)()
    cnt = (ctypes.c_uint32 * 16)()
    assert L.gol_read_window(None, 0, 0, 1, 1, buf, None) == N.GOL_EINVAL
    assert L.gol_window_density(None, 0, 0, 1, 1, 1, cnt, None) == N.GOL_EINVAL
    assert L.gol_write_window(None, 0, 0, 1, 1, buf) == N.GOL_EINVAL
    assert L.gol_clear(None) == N.GOL_EINVAL
    assert L.gol_board_layout(None) == N.GOL_EINVAL
