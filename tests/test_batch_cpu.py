"""The batch section of the C ABI (gol_batch_*, include/gol_amd.h) where it needs no device:
argument checks come before device discovery, every call refuses a NULL handle, and a box without
a GPU answers a valid create with GOL_ENODEV."""
import ctypes as C

import pytest

import resident_cases as RC

INT32_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def lib():
    from gol import _native as N
    return N.lib(), N


def _create(L, width, height, boards, flags=0, device=-1):
    h = C.c_void_p()
    rc = L.gol_batch_create(width, height, boards, device, flags, C.byref(h))
    if rc == 0:                                  # (a GPU box: nothing may leak from a CPU test)
        L.gol_batch_destroy(h)
    else:
        assert not h.value
    return rc


@pytest.mark.parametrize("width,height,boards,flags", (
    (1, 16, 4, 0), (256, 16, 4, 0), (0, 16, 4, 0), (-5, 16, 4, 0),
    (64, 0, 4, 0), (64, -1, 4, 0),
    (64, 16, 0, 0), (64, 16, -3, 0),
    (64, 4096, INT32_MAX // 4096 + 1, 0),        # boards x height = 2^31
    (200, 77, INT32_MAX // 77 + 1, 0),
    (64, 16, 4, 0x2), (64, 16, 4, 0x8), (64, 16, 4, 0x1 | 0x10), (64, 16, 4, 0x80000000),
), ids=str)
def test_create_refuses_before_the_device(lib, width, height, boards, flags):
    L, N = lib
    assert _create(L, width, height, boards, flags) == N.GOL_EINVAL


@pytest.mark.parametrize("width", (64, 128, 191, 255, 2, 65))
def test_create_refuses_a_board_above_the_limit(lib, width):
    L, N = lib
    limit = RC.limit(width)
    assert limit == {1: 4096, 2: 2048, 3: 1280, 4: 1024}[RC.nwords(width)]
    assert RC.plan(width, limit) is not None and RC.plan(width, limit + 1) is None
    assert _create(L, width, limit + 1, 1) == N.GOL_EINVAL


def test_create_refuses_a_null_out(lib):
    L, N = lib
    assert L.gol_batch_create(64, 64, 4, -1, 0, None) == N.GOL_EINVAL


def test_null_handles(lib):
    L, N = lib
    i32 = [C.c_int32() for _ in range(7)]
    t = C.c_int64()
    words = (C.c_uint64 * 4)()
    cells = (C.c_uint8 * 4)()
    out = (C.c_int64 * 4)()
    a, b = C.c_int32(), C.c_int32()
    calls = {
        "gol_batch_get_info": lambda: L.gol_batch_get_info(None, *(C.byref(x) for x in i32),
                                                           C.byref(t)),
        "gol_batch_occupancy": lambda: L.gol_batch_occupancy(None, C.byref(a), C.byref(b)),
        "gol_batch_sync": lambda: L.gol_batch_sync(None),
        "gol_batch_load_packed": lambda: L.gol_batch_load_packed(None, 0, 1, words),
        "gol_batch_load": lambda: L.gol_batch_load(None, 0, 1, cells),
        "gol_batch_fill_random": lambda: L.gol_batch_fill_random(None, 1),
        "gol_batch_step": lambda: L.gol_batch_step(None, 1),
        "gol_batch_read_packed": lambda: L.gol_batch_read_packed(None, 0, 1, words),
        "gol_batch_read": lambda: L.gol_batch_read(None, 0, 1, cells),
        "gol_batch_alive": lambda: L.gol_batch_alive(None, 0, 1, out),
        "gol_batch_turn_counts": lambda: L.gol_batch_turn_counts(None, 1, 1, out),
    }
    # every gol_batch_* call of the header that takes a handle and returns a code is here
    takes_handle = {n for n in N.header_functions() if n.startswith("gol_batch_")}
    assert takes_handle - {"gol_batch_create", "gol_batch_destroy", "gol_batch_last_error",
                           "gol_batch_get_stream"} == set(calls)
    for name, call in calls.items():
        assert call() == N.GOL_EINVAL, name
    assert L.gol_batch_last_error(None) == b""
    assert L.gol_batch_get_stream(None) is None  # (a pointer, not a code)
    L.gol_batch_destroy(None)                    # (a no-op)


def test_valid_create_without_a_device(lib):
    L, N = lib
    import torch
    if not torch.cuda.is_available():
        assert _create(L, 64, 64, 4) == N.GOL_ENODEV
        assert _create(L, 255, 1024, 2, N.GOL_FLAG_COUNT_EVERY_TURN) == N.GOL_ENODEV
        assert _create(L, 64, 4096, INT32_MAX // 4096) == N.GOL_ENODEV


def test_python_class_is_exported():
    import gol
    assert gol.BatchEngine.__name__ == "BatchEngine"
    for name in ("load_packed", "load", "fill_random", "step", "read_packed", "read", "alive",
                 "turn_counts", "sync", "close", "turn", "info"):
        assert hasattr(gol.BatchEngine, name), name
