"""The shared row-pair rule of csrc/gol_device.h (life_pair_sum + life_rule_pair) against the plain
B3/S23 count, on all 4096 windows of 4 rows x 3 cells and both outputs of the pair.  The two
functions are read from the source (v_bitop3 immediates, index (src0 << 2) | (src1 << 1) | src2;
`&` and `^` for the two VOP2 operations), as tests/test_host_cpu.py reads life_rule7.  No GPU.
"""
import os
import re

import pytest

SRC = os.path.join(os.path.dirname(__file__), "..", "conway-s-gol-distributed_amd", "csrc",
                   "gol_device.h")
_LUT = {"xor3": 0x96, "maj": 0xE8}
_OP = re.compile(r"(?:const uint32_t )?(\w+|return)(?: =)? "
                 r"(?:(xor3|maj|bitop3<(0x[0-9a-f]+)>)\((\w+), (\w+), (\w+)\)|(\w+) ([&^]) (\w+));")


def _body(src, name):
    body = src[src.index(f" {name}("):]
    return body[body.index("{") + 1:body.index("\n}")]


def _ops(src, name):
    """The body of a device function as (dst, immediate or '&' / '^', sources)."""
    ops = []
    for line in _body(src, name).splitlines():
        m = _OP.search(line.strip())
        if not m:
            continue
        if m.group(2):
            imm = _LUT.get(m.group(2)) or int(m.group(3), 16)
            ops.append((m.group(1), imm, m.group(4, 5, 6)))
        else:
            ops.append((m.group(1), m.group(8), m.group(7, 9)))
    return ops


def _run(ops, env):
    for dst, op, args in ops:
        if op == "&":
            env[dst] = env[args[0]] & env[args[1]]
        elif op == "^":
            env[dst] = env[args[0]] ^ env[args[1]]
        else:
            x, y, z = (env[a] for a in args)
            env[dst] = (op >> ((x << 2) | (y << 1) | z)) & 1
    return env


def _failures(src):
    """Windows (m, output) on which the source's pair rule differs from the count."""
    pair, rule = _ops(src, "life_pair_sum"), _ops(src, "life_rule_pair")
    assert [o[0] for o in pair] == ["k", "p0", "p1", "p2"]
    assert [o[0] for o in rule] == ["u", "w", "z", "return"]
    bad = []
    for m in range(4096):
        cell = [(m >> i) & 1 for i in range(12)]
        rs = [sum(cell[3 * r:3 * r + 3]) for r in range(4)]
        p = _run(pair, {"b0": rs[1] & 1, "b1": rs[1] >> 1, "c0": rs[2] & 1, "c1": rs[2] >> 1})
        assert p["p0"] + 2 * p["p1"] + 4 * p["p2"] == rs[1] + rs[2]
        # output row 1: third row 0, centre cell 4; output row 2: third row 3, centre cell 7
        for out, (third, centre) in enumerate(((0, 4), (3, 7))):
            n = rs[1] + rs[2] + rs[third] - cell[centre]
            want = int(n == 3 or (cell[centre] == 1 and n == 2))
            env = _run(rule, {"a0": rs[third] & 1, "a1": rs[third] >> 1, "p0": p["p0"],
                              "p1": p["p1"], "p2": p["p2"], "x": cell[centre]})
            if env["return"] != want:
                bad.append((m, out))
    return bad


def test_pair_rule_truth_tables():
    assert _failures(open(SRC).read()) == []


@pytest.mark.parametrize("imm,wrong", [("0xbc", "0xb4"), ("0x94", "0x84"), ("0x82", "0x80"),
                                       ("0x42", "0x46")])
def test_wrong_immediate_fails(imm, wrong):
    """The check has teeth: one flipped table entry in a copy of the source is caught."""
    src = open(SRC).read()
    body = _body(src, "life_rule_pair")
    assert body.count(f"bitop3<{imm}>") == 1
    mutated = src.replace(body, body.replace(f"bitop3<{imm}>", f"bitop3<{wrong}>"))
    assert mutated != src
    assert _failures(mutated)


def test_wrong_pair_sum_fails():
    src = open(SRC).read()
    body = _body(src, "life_pair_sum")
    mutated = src.replace(body, body.replace("p1 = xor3(b1, c1, k)", "p1 = maj(b1, c1, k)"))
    assert mutated != src
    with pytest.raises(AssertionError):
        _failures(mutated)
