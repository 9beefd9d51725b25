"""The turn loop of k_step_tile_duo<16,5,1> (csrc/gol_tile.h, tile_pass DUO: the interior rows of
a segment ruled in pairs on shared row-pair sums), checked on the compiler's assembly as
test_tile_parity_cpu.py checks the plain kernel's: at most 328 VALU per turn with at most 232
v_bitop3 (the plain kernel: 356 with 288), no register copies, no scratch, at most 64 VGPRs and
8 waves per SIMD ("Shared row-pair sums").  No register plan ships for this kernel, so
the same-parity count is printed, not asserted.  No GPU: the unit is compiled to assembly with the
Makefile's flags and read by tools/vgpr_parity.py.  Skipped where there is no hipcc.
"""
import importlib.util
import os
import re
import shutil
import subprocess

import pytest

from conftest import PKG, ROOT

CSRC = os.path.join(PKG, "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
if not os.path.exists(HIPCC):
    HIPCC = shutil.which("hipcc")
NAME = "k_step_tile_duo<16,5,1>"


def _tool():
    spec = importlib.util.spec_from_file_location(
        "vgpr_parity", os.path.join(ROOT, "tools", "vgpr_parity.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _flags():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    cxx = re.search(r"^CXXFLAGS := (.*)$", mk, re.M).group(1)
    arch = re.search(r"^ARCH \?= (\S+)$", mk, re.M).group(1)
    cxx = cxx.replace("$(INC)", "-I" + os.path.join(ROOT, "include"))
    return [f"--offload-arch={arch}"] + cxx.split()


def _compile(out, extra=()):
    subprocess.run([HIPCC, *_flags(), *extra, "--cuda-device-only", "-S",
                    os.path.join(CSRC, "gol_tile_duo.hip"), "-o", out],
                   check=True, cwd=CSRC, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    return out


@pytest.fixture(scope="module")
def stats(tmp_path_factory):
    if not HIPCC:
        pytest.skip("no hipcc")
    path = _compile(str(tmp_path_factory.mktemp("duo") / "duo.s"))
    res = _tool().stats(path, re.escape(NAME) + "$")
    assert list(res) == [NAME], list(res)
    return res[NAME]


def test_duo_turn_loop(stats):
    """Per dword 32 row-sum operations, 7 pairs x 12 and two edge rows x 7: 232 v_bitop3 and 28
    VOP2 per wave and turn, 328 VALU with the lane shifts."""
    s = stats
    print(NAME, s)
    assert s["valu"] <= 328
    assert s["bitop3"] <= 232
    assert s["mov"] == 0
    assert s["scratch"] == 0
    assert s["vgprs"] <= 64 and s["occupancy"] == 8
