"""VGPR parity of the K1t turn loop (csrc/gol_tile.h, tile_parity_pins), checked on the compiler's
assembly: a v_bitop3_b32 whose three source VGPRs share one register-number parity issues at
half rate on gfx950, so the pinned instantiations must have none, at the parent's instruction
count, register copies, scratch and waves per SIMD; with -DGOL_TILE_PARITY_PINS=0 the compiler's
own numbering is back.  No GPU: the two tile units are compiled to assembly with the Makefile's
flags (about 20 s, the three compiles at once) and read by tools/vgpr_parity.py.  Skipped where
there is no hipcc.

PARENT holds the loop statistics of the commit before the pins, from the same tool.
"""
import importlib.util
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from conftest import PKG, ROOT

CSRC = os.path.join(PKG, "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
if not os.path.exists(HIPCC):
    HIPCC = shutil.which("hipcc")

# kernel: (VALU in the loop, v_mov_b32 in the loop, waves per SIMD, same-parity v_bitop3)
PARENT = {
    "k_step_tile<16,5,1>": (356, 0, 8, 43),
    "k_step_tile_cnt<16,5,1>": (482, 3, 8, 117),
    "k_step_tile_big<16,5>": (356, 0, 8, 25),
}
# (the big form stays on the compiler's numbers: pinned it measured slower)
PINNED = {"gol_tile": ["k_step_tile<16,5,1>", "k_step_tile_cnt<16,5,1>"]}


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


def _compile(unit, out, extra=()):
    subprocess.run([HIPCC, *_flags(), *extra, "--cuda-device-only", "-S",
                    os.path.join(CSRC, unit + ".hip"), "-o", out],
                   check=True, cwd=CSRC, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    return out


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not HIPCC:
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("parity")
    jobs = {"gol_tile": ("gol_tile", ()), "gol_tile_big": ("gol_tile_big", ()),
            "gol_tile_pins0": ("gol_tile", ("-DGOL_TILE_PARITY_PINS=0",))}
    with ThreadPoolExecutor(3) as ex:
        futs = {k: ex.submit(_compile, u, str(d / (k + ".s")), x) for k, (u, x) in jobs.items()}
        return {k: f.result() for k, f in futs.items()}


def _stats(path, name):
    res = _tool().stats(path, re.escape(name) + "$")
    assert list(res) == [name], (name, list(res))
    return res[name]


@pytest.mark.parametrize("unit,name", [(u, n) for u, ns in PINNED.items() for n in ns])
def test_pinned_turn_loop(asm, unit, name):
    """Every v_bitop3 of the loop reads both parities, at no cost in instructions, copies,
    scratch or waves per SIMD."""
    s = _stats(asm[unit], name)
    valu, mov, occ, _ = PARENT[name]
    print(name, s)
    assert s["bitop3"] == 288                            # 16 rows x (4 + 14)
    assert s["same"] == 0
    assert s["valu"] <= valu
    assert s["mov"] <= mov
    assert s["scratch"] == 0
    assert s["vgprs"] <= 64 and s["occupancy"] == occ


def test_big_form_is_the_parents(asm):
    s = _stats(asm["gol_tile_big"], "k_step_tile_big<16,5>")
    assert (s["valu"], s["mov"], s["occupancy"], s["same"]) == PARENT["k_step_tile_big<16,5>"]


def test_switch_restores_parent(asm):
    """-DGOL_TILE_PARITY_PINS=0: the compiler's own register numbers, as in the parent."""
    s = _stats(asm["gol_tile_pins0"], "k_step_tile<16,5,1>")
    assert (s["valu"], s["mov"], s["occupancy"], s["same"]) == PARENT["k_step_tile<16,5,1>"]
    s = _stats(asm["gol_tile_pins0"], "k_step_tile_cnt<16,5,1>")
    assert (s["valu"], s["mov"], s["occupancy"], s["same"]) == PARENT["k_step_tile_cnt<16,5,1>"]


def test_unpinned_kernels_unchanged(asm):
    """The instantiations outside the plan compile the same with the switch on and off."""
    tool = _tool()
    on, off = tool.stats(asm["gol_tile"], "k_step_tile"), tool.stats(asm["gol_tile_pins0"], "k_step_tile")
    assert set(on) == set(off) and len(on) > len(PINNED["gol_tile"])
    for name in on:
        if name not in PINNED["gol_tile"]:
            assert on[name] == off[name], name


# ---------------------------------------------------------------- the plan itself (no compiler)
def _cell(i, d):
    return 2 * i + d


def _sum(seg, j, k):
    base = 2 * seg + (16 if j == 1 else (j & 1) * 8 + ((j >> 1) & 1) * 4)
    return base + (k ^ 1 if j & 1 else k)


def _tmp(seg, d, t):
    return 2 * seg + 20 + 2 * t + (d ^ 1)


def _rule_regs(seg, i, d):
    """(lx, hm, hx) of row i's rule for dword d, and the sums they overwrite in place."""
    if i == 2:                                           # no donor: row 1's sums stay live
        return _tmp(seg, d, 0), _tmp(seg, d, 1), _cell(i, d)
    jd = 1 if i == 0 else i - 1
    r0, r1 = _sum(seg, jd, 2 * d), _sum(seg, jd, 2 * d + 1)
    if r1 & 1 == d:
        return r0, _tmp(seg, d, 0), r1
    return _tmp(seg, d, 0), r1, r0


def _mixed(*regs):
    return len({r & 1 for r in regs}) == 2


@pytest.mark.parametrize("seg", [4, 12, 16, 24])
def test_plan_mixes_every_triple(seg):
    """The plan of gol_tile.h (tile_pin_cell / tile_pin_sum / tile_pin_tmp, mirrored above): every
    triple of a turn is mixed whatever registers the unpinned values get, the sets of a window's
    three rows are disjoint, and the put tuples are even-aligned and in order."""
    # LDS tuples: position q has parity q; the bottom-edge array holds the sums as 1, 0, 3, 2
    top = [k for k in range(4)]                          # parity of sum k as read from the top array
    bot = [k ^ 1 for k in range(4)]
    assert [_sum(seg, 0, k) for k in range(4)] == list(range(2 * seg, 2 * seg + 4))
    last = [_sum(seg, seg - 1, k ^ 1) for k in range(4)]    # the order put stores them in
    assert last == list(range(last[0], last[0] + 4)) and last[0] % 2 == 0

    def sums(j):
        if j == -1:
            return bot                                   # U: the bottom edge of the segment above
        if j == seg:
            return top                                   # D: the top edge of the one below
        return [_sum(seg, j, k) for k in range(4)]

    for i in range(seg):
        a, b, c = sums(i - 1), sums(i), sums(i + 1)
        if i in (0, seg - 1):                            # (read back from LDS for the edge rules)
            b = top if i == 0 else bot
        for k in range(4):
            assert _mixed(a[k], b[k], c[k]), (i, k)
        if 1 <= i <= seg - 2 and i + 1 <= seg - 2:
            regs = [set(sums(j)) for j in (i - 1, i, i + 1)]
            assert not (regs[0] & regs[1] or regs[1] & regs[2] or regs[0] & regs[2]), i
            assert not any(set(sums(1)) & r for j, r in zip((i - 1, i, i + 1), regs) if j != 1), i
        for d in range(2):
            C = _cell(i, d)
            lx, hm, hx = _rule_regs(seg, i, d)
            assert len({lx, hm, hx}) == 3
            # (wl, e, o), (e, o, er): the row's two dwords
            assert _mixed(_cell(i, 0), _cell(i, 1))
            # (lm, lx, C), (hm, C, g1), (lx, hx, g2) with lm, g1, g2 anywhere
            assert _mixed(lx, C) and _mixed(hm, C) and _mixed(lx, hx)
    pinned = ({_cell(i, d) for i in range(seg) for d in range(2)}
              | {_sum(seg, j, k) for j in range(seg) for k in range(4)}
              | {_tmp(seg, d, t) for d in range(2) for t in range(2)})
    # (the plan's registers are v0 .. v(2 SEG + 23): a short segment leaves some sets unused)
    assert pinned <= set(range(2 * seg + 24)) and max(pinned) == 2 * seg + 23
    assert seg < 8 or pinned == set(range(2 * seg + 24))
