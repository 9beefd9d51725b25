"""gol_tile_count_codes: the k_step_tile codes with a counted form (golk::kTileCountCodes), the
ones a count_every_turn engine runs multi-turn launches on.  No device needed."""
import ctypes as C

from conftest import TILE_CODES


def _lib():
    from gol import _native as N
    return N.lib()


def _codes(fn):
    n = fn(None, 0)
    buf = (C.c_int32 * n)()
    assert fn(buf, n) == n
    return tuple(buf)


def test_count_codes_exported_without_a_device():
    from gol import _native as N
    L = _lib()
    assert "gol_tile_count_codes" in N.header_functions()
    assert "gol_tile_count_codes" in N.SIGNATURES
    codes = _codes(L.gol_tile_count_codes)
    assert len(codes) > 0 and len(set(codes)) == len(codes)


def test_count_codes_are_shipped_tile_codes():
    L = _lib()
    codes = _codes(L.gol_tile_count_codes)
    assert set(codes) <= set(_codes(L.gol_tile_codes)) == set(TILE_CODES)
    assert all(c < 1000 for c in codes)                  # one word per lane


def test_count_codes_cover_the_pinned_shapes_and_loop_forms():
    codes = set(_codes(_lib().gol_tile_count_codes))
    assert {516, 203, 112} <= codes                      # kKnownShapes' codes
    assert {512, 506, 503, 103, 106, 206} <= codes       # both loop forms, the pins' turn orders


def test_count_codes_cap_convention():
    """cap = 0 returns n and writes nothing; a short buffer gets the first cap codes; a negative
    cap or a null buffer with cap > 0 is GOL_EINVAL (gol_tile_codes' convention)."""
    from gol import _native as N
    L = _lib()
    n = L.gol_tile_count_codes(None, 0)
    assert n == len(_codes(L.gol_tile_count_codes))
    buf = (C.c_int32 * (n + 2))(*([-7] * (n + 2)))
    assert L.gol_tile_count_codes(buf, 0) == n
    assert list(buf) == [-7] * (n + 2)
    assert L.gol_tile_count_codes(buf, 3) == n
    assert tuple(buf[:3]) == _codes(L.gol_tile_count_codes)[:3] and list(buf[3:]) == [-7] * (n - 1)
    assert L.gol_tile_count_codes(buf, n + 2) == n and buf[n] == -7
    assert L.gol_tile_count_codes(None, 4) == N.GOL_EINVAL
    assert L.gol_tile_count_codes(buf, -1) == N.GOL_EINVAL
