"""gol_flipped_cells (the per-turn CellFlipped list, K5) as far as it goes without a device: the
symbol is declared, exported and bound, the Python handle has the method, and the argument
checks come before any device work.  The lists themselves: tests/test_gpu_flips.py."""
import ctypes
import subprocess


def test_symbol_declared_exported_and_bound():
    from gol import _native as N
    assert "gol_flipped_cells" in N.header_functions()
    assert "gol_flipped_cells" in N.SIGNATURES
    assert N.SIGNATURES["gol_flipped_cells"] == N.SIGNATURES["gol_alive_cells"]
    nm = subprocess.run(["nm", "-D", "--defined-only", N.LIB_PATH], capture_output=True,
                        text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if " T " in line}
    assert "gol_flipped_cells" in exported
    assert hasattr(N.lib(), "gol_flipped_cells")


def test_engine_has_flipped_cells():
    import gol
    assert callable(getattr(gol.Engine, "flipped_cells", None))


def test_header_names_the_call_among_the_read_only_ones():
    """The threading paragraph lists it with the other calls that go through the reader path."""
    from gol import _native as N
    text = open(N.HEADER_PATH).read()
    para = text[text.index("Threading:"):text.index("Return codes:")]
    assert "gol_flipped_cells" in para


def test_argument_errors_need_no_device():
    """As tests/test_abi.py::test_strerror_and_no_device_paths: NULL engine, NULL count, a
    negative cap and a positive cap without a buffer are GOL_EINVAL before anything else."""
    from gol import _native as N
    L = N.lib()
    n = ctypes.c_int64(-5)
    xy = (ctypes.c_int64 * 4)(7, 7, 7, 7)
    assert L.gol_flipped_cells(None, xy, 2, ctypes.byref(n)) == N.GOL_EINVAL
    assert L.gol_flipped_cells(None, None, 0, ctypes.byref(n)) == N.GOL_EINVAL
    assert L.gol_flipped_cells(None, None, 0, None) == N.GOL_EINVAL
    # (a non-NULL handle is never dereferenced when the count pointer is missing)
    mem = ctypes.create_string_buffer(8)
    fake = ctypes.c_void_p(ctypes.addressof(mem))
    assert L.gol_flipped_cells(fake, xy, 2, None) == N.GOL_EINVAL
    assert L.gol_flipped_cells(fake, xy, -1, ctypes.byref(n)) == N.GOL_EINVAL
    assert L.gol_flipped_cells(fake, None, 2, ctypes.byref(n)) == N.GOL_EINVAL
    assert n.value == -5 and list(xy) == [7, 7, 7, 7]
