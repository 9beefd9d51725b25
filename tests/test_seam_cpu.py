"""K1t across the row seam, the parts that need no device: gol_tile_seam_codes (the k_step_tile
codes with a form for widths that are no multiple of 64, golk::kTileSeamCodes) and gol_seam_word
(the host build of the kernel's stitch: the word a lane holds at a virtual lane column of a row
whose last word is partial) against a numpy bit model, cell[(64 v + b) % width]."""
import ctypes as C

import numpy as np
import pytest

from conftest import TILE_CODES


def _lib():
    from gol import _native as N
    return N.lib()


def _codes(fn):
    n = fn(None, 0)
    buf = (C.c_int32 * n)()
    assert fn(buf, n) == n
    return tuple(buf)


# ------------------------------------------------------------------ gol_tile_seam_codes
def test_seam_codes_exported_without_a_device():
    from gol import _native as N
    L = _lib()
    for name in ("gol_tile_seam_codes", "gol_seam_word"):
        assert name in N.header_functions()
        assert name in N.SIGNATURES
    codes = _codes(L.gol_tile_seam_codes)
    assert len(codes) > 0 and len(set(codes)) == len(codes)


def test_seam_codes_are_shipped_tile_codes():
    L = _lib()
    codes = _codes(L.gol_tile_seam_codes)
    assert set(codes) <= set(_codes(L.gol_tile_codes)) == set(TILE_CODES)
    assert all(c < 1000 for c in codes)                  # one word per lane


def test_seam_codes_cover_the_families():
    """A short segment, turn order 1, both loop forms (turn pairs up to SEG 12, one body above)
    and 516, the large boards' kernel."""
    codes = set(_codes(_lib().gol_tile_seam_codes))
    assert 516 in codes
    assert any(c % 100 <= 6 for c in codes)
    assert any(c // 100 == 1 for c in codes)
    assert any(c % 100 <= 12 for c in codes) and any(c % 100 > 12 for c in codes)


def test_seam_codes_cap_convention():
    """cap = 0 returns n and writes nothing; a short buffer gets the first cap codes; a negative
    cap or a null buffer with cap > 0 is GOL_EINVAL (gol_tile_codes' convention)."""
    from gol import _native as N
    L = _lib()
    n = L.gol_tile_seam_codes(None, 0)
    assert n == len(_codes(L.gol_tile_seam_codes)) and n >= 3
    buf = (C.c_int32 * (n + 2))(*([-7] * (n + 2)))
    assert L.gol_tile_seam_codes(buf, 0) == n
    assert list(buf) == [-7] * (n + 2)
    assert L.gol_tile_seam_codes(buf, 3) == n
    assert tuple(buf[:3]) == _codes(L.gol_tile_seam_codes)[:3] and list(buf[3:]) == [-7] * (n - 1)
    assert L.gol_tile_seam_codes(buf, n + 2) == n and buf[n] == -7
    assert L.gol_tile_seam_codes(None, 4) == N.GOL_EINVAL
    assert L.gol_tile_seam_codes(buf, -1) == N.GOL_EINVAL


# ------------------------------------------------------------------ gol_seam_word
def _pack(cells):
    """Row of 0/1 cells -> standard words (cell c = bit c % 64 of word c // 64, zero padding)."""
    nw = (len(cells) + 63) // 64
    bits = np.zeros(nw * 64, dtype=np.uint8)
    bits[:len(cells)] = cells
    return np.packbits(bits.reshape(nw, 64), axis=1, bitorder="little").view("<u8").ravel().copy()


def _interleave(words):
    """Standard -> interleaved words: cell 2 i -> bit i, cell 2 i + 1 -> bit 32 + i."""
    bits = np.unpackbits(words.view(np.uint8).reshape(-1, 8), axis=1, bitorder="little")
    il = np.concatenate([bits[:, 0::2], bits[:, 1::2]], axis=1)
    return np.packbits(il, axis=1, bitorder="little").view("<u8").ravel().copy()


def _model_word(cells, v):
    """Virtual lane column v: bit b = cell (64 v + b) mod width, as a standard word."""
    idx = (64 * v + np.arange(64)) % len(cells)
    return _pack(cells[idx])[0]


def _seam_word(L, words, width, v, layout):
    out = C.c_uint64(0xDEADBEEF)
    row = words.ctypes.data_as(C.POINTER(C.c_uint64))
    rc = L.gol_seam_word(row, width, v, layout, C.byref(out))
    return rc, out.value


def _rows(width, rng):
    yield np.ones(width, dtype=np.uint8)                 # a lost or doubled seam bit shows here
    for _ in range(3):
        yield rng.integers(0, 2, width, dtype=np.uint8)


@pytest.mark.parametrize("nw", [5, 6])
def test_seam_word_matches_the_bit_model(nw):
    """Every r = width % 64 in 1 .. 63 at 5 and 6 words per row, every column in [-1, nw], both
    layouts, random rows and the row of all ones."""
    L = _lib()
    rng = np.random.default_rng(nw)
    for r in range(1, 64):
        width = 64 * (nw - 1) + r
        for cells in _rows(width, rng):
            std = _pack(cells)
            il = _interleave(std)
            for v in range(-1, nw + 1):
                want = _model_word(cells, v)
                rc, got = _seam_word(L, std, width, v, 0)
                assert rc == 0 and got == int(want), (width, v, "standard")
                rc, got = _seam_word(L, il, width, v, 1)
                assert rc == 0 and got == int(_interleave(np.array([want], dtype="<u8"))[0]), \
                    (width, v, "interleaved")


@pytest.mark.parametrize("width", [320, 384])
def test_seam_word_whole_words(width):
    """r = 0: the plain wrapped word, in either layout."""
    L = _lib()
    nw = width // 64
    cells = np.random.default_rng(width).integers(0, 2, width, dtype=np.uint8)
    std = _pack(cells)
    il = _interleave(std)
    for v in range(-1, nw + 1):
        assert _seam_word(L, std, width, v, 0) == (0, int(std[v % nw]))
        assert _seam_word(L, il, width, v, 1) == (0, int(il[v % nw]))


def test_seam_word_einval():
    from gol import _native as N
    L = _lib()
    width, nw = 300, 5
    std = _pack(np.ones(width, dtype=np.uint8))
    row = std.ctypes.data_as(C.POINTER(C.c_uint64))
    out = C.c_uint64(0)
    assert _seam_word(L, std, width, -2, 0)[0] == N.GOL_EINVAL
    assert _seam_word(L, std, width, nw + 1, 0)[0] == N.GOL_EINVAL
    assert _seam_word(L, std, width, -1, 0)[0] == 0 and _seam_word(L, std, width, nw, 1)[0] == 0
    assert _seam_word(L, _pack(np.ones(255, dtype=np.uint8)), 255, 0, 0)[0] == N.GOL_EINVAL
    assert _seam_word(L, std, width, 0, 2)[0] == N.GOL_EINVAL
    assert L.gol_seam_word(None, width, 0, 0, C.byref(out)) == N.GOL_EINVAL
    assert L.gol_seam_word(row, width, 0, 0, None) == N.GOL_EINVAL
