#!/usr/bin/env python3
"""VGPR parity of the v_bitop3_b32 in a kernel's turn loop, from a hipcc -S file.

usage: vgpr_parity.py file.s [kernel-name regex] [--json]

A v_bitop3_b32 whose three source VGPRs share one register-number parity issues at half
rate on gfx950 ("VGPR parity and a hand-assigned turn").  Per kernel whose
mangled or readable name (k_step_tile<16,5,1>) matches the pattern this prints, for the turn
loop -- the innermost loop holding the most v_bitop3_b32 --

  valu      VALU instructions in the loop (every v_* mnemonic)
  bitop3    v_bitop3_b32 among them
  same      v_bitop3_b32 with three VGPR sources of one parity
  mov       v_mov_b32 in the loop (register copies; DPP moves are counted apart as dpp)
  vgprs, scratch, occupancy   from the compiler's per-kernel comments

This generalises asm_loop_stats.py (one kernel's instruction mix); import stats() to use it
from a test.
"""
import json
import re
import sys

_FUNC = re.compile(r"^(_Z\w+):")
_LABEL = re.compile(r"^(\.LBB\w+):")
_BRANCH = re.compile(r"\bs_c?branch\w*\s+(\.LBB\w+)")
_BITOP = re.compile(r"^v_bitop3_b32\s+v\d+,\s*([^,]+),\s*([^,]+),\s*(\S+)")
_INT_ARGS = re.compile(r"(?:Li(\d+)E|Lb([01])E)")


def readable(mangled):
    """_ZN4golk11k_step_tileILi16ELi5ELi1EEEv... -> k_step_tile<16,5,1>"""
    m = re.match(r"_ZN4golk(\d+)", mangled)
    if not m:
        return mangled
    n = int(m.group(1))
    rest = mangled[m.end():]
    name, rest = rest[:n], rest[n:]
    if not rest.startswith("I"):
        return name
    args = []
    pos = 1
    while True:
        a = _INT_ARGS.match(rest, pos)
        if not a:
            break
        args.append(a.group(1) or a.group(2))
        pos = a.end()
    return f"{name}<{','.join(args)}>"


def _insn(line):
    t = line.strip()
    if not t or t[0] in ";." or t.endswith(":"):
        return None
    return t


def _loop_stats(body):
    labels = {}
    for i, l in enumerate(body):
        m = _LABEL.match(l)
        if m:
            labels[m.group(1)] = i
    loops = []
    for i, l in enumerate(body):
        m = _BRANCH.search(l)
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            loops.append((labels[m.group(1)], i))
    best = None
    for s, e in loops:
        st = {"valu": 0, "bitop3": 0, "same": 0, "mov": 0, "dpp": 0, "lines": [s, e]}
        for l in body[s:e + 1]:
            t = _insn(l)
            if not t or not t.startswith("v_"):
                continue
            st["valu"] += 1
            op = t.split()[0]
            if op == "v_mov_b32_dpp" or " row_" in t or " quad_perm" in t or " wave_" in t:
                st["dpp"] += 1
            elif op in ("v_mov_b32_e32", "v_mov_b32_e64", "v_mov_b32"):
                st["mov"] += 1
            b = _BITOP.match(t)
            if b:
                st["bitop3"] += 1
                regs = [re.fullmatch(r"v(\d+)", x.strip()) for x in b.groups()]
                if all(regs) and len({int(r.group(1)) & 1 for r in regs}) == 1:
                    st["same"] += 1
        # the turn loop: most v_bitop3; among equals the innermost (shortest)
        key = (st["bitop3"], -(e - s))
        if st["bitop3"] and (best is None or key > best[0]):
            best = (key, st)
    return best[1] if best else None


def stats(path, pattern=""):
    """{readable name: {...}} for every kernel of the file whose name matches `pattern`."""
    lines = open(path).read().splitlines()
    rx = re.compile(pattern)
    out = {}
    i = 0
    while i < len(lines):
        m = _FUNC.match(lines[i])
        if not m:
            i += 1
            continue
        name = m.group(1)
        end = next((j for j in range(i, len(lines)) if lines[j].startswith(".Lfunc_end")), len(lines))
        nice = readable(name)
        if rx.search(name) or rx.search(nice):
            st = _loop_stats(lines[i:end]) or {"valu": 0, "bitop3": 0, "same": 0, "mov": 0, "dpp": 0}
            # (the compiler's summary comments follow the function's end)
            for l in lines[end:end + 80]:
                for key, tag in (("vgprs", "NumVgprs"), ("scratch", "ScratchSize"),
                                 ("occupancy", "Occupancy")):
                    mm = re.match(rf"^;\s*{tag}:\s*(\d+)", l)
                    if mm and key not in st:
                        st[key] = int(mm.group(1))
            out[nice] = st
        i = end + 1
    return out


def main(argv):
    args = [a for a in argv[1:] if not a.startswith("--")]
    if not args:
        sys.exit(__doc__)
    res = stats(args[0], args[1] if len(args) > 1 else "")
    if "--json" in argv:
        print(json.dumps(res, indent=1))
        return
    print(f"{'kernel':36s} {'valu':>5s} {'bitop3':>6s} {'same':>5s} {'mov':>4s} {'vgprs':>5s} "
          f"{'scratch':>7s} {'occ':>3s}")
    for k, s in res.items():
        print(f"{k:36s} {s['valu']:5d} {s['bitop3']:6d} {s['same']:5d} {s['mov']:4d} "
              f"{s.get('vgprs', -1):5d} {s.get('scratch', -1):7d} {s.get('occupancy', -1):3d}")


if __name__ == "__main__":
    main(sys.argv)
