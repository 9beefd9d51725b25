"""k_step_tile on row strips, and the split launch of gol_step_overlap, at small shapes.

Every segment code the library runs is pinned on ragged strip engines (row_lo > 0, no row
wrap, a computed range that shrinks by k rows per launch, launches that start s0 > 0 turns into
a halo window), and the split first launch of an overlapped window runs in process with its
halo receives held back behind a delay, so that a boundary launch that did not wait for them,
or a next launch that did not wait for the boundary launches, computes a wrong board.

The reference everywhere is oracle.bit_run on the whole torus from oracle.gen_random, compared
bit for bit with the strips' owned rows (read_packed), concatenated.  The shapes come from
strip_tiles.py, whose tables test_strip_tiles_cpu.py checks without a GPU.
"""
import numpy as np
import pytest

import strip_tiles as S
from conftest import TILE_CODES, tools_only

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gol():
    import gol as g
    return g


def _pin_tile(monkeypatch, tw, code):
    monkeypatch.setenv("GOL_MULTI_VARIANT", "15")
    monkeypatch.setenv("GOL_TILE", f"{tw},{code}")


def _haloed(start, o, r, halo):
    """Packed global rows o - halo .. o + r + halo - 1 (mod H)."""
    H = start.shape[0]
    return np.ascontiguousarray(start[np.arange(o - halo, o + r + halo) % H])


class _Strips:
    """n strip engines of one board on device 0, exchanging by peer copies."""

    def __init__(self, gol, start, w, n, halo, **kw):
        self.start, self.w, self.n, self.halo = start, w, n, halo
        h = start.shape[0]
        self.parts = gol.strip_split(h, n)
        self.engs = []
        try:
            for o, r in self.parts:
                self.engs.append(gol.Engine(w, h, device=0, row_offset=o, rows=r, halo=halo, **kw))
            for e, (o, r) in zip(self.engs, self.parts):
                e.load_packed(_haloed(start, o, r, halo))
        except Exception:
            self.close()
            raise

    def close(self):
        for e in self.engs:
            e.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def exchange(self):
        n = self.n
        for i, e in enumerate(self.engs):
            e.copy_halo_from_upper(self.engs[(i - 1) % n])
            e.copy_halo_from_lower(self.engs[(i + 1) % n])
        for e in self.engs:
            e.halo_done()

    def step(self, turns, check=None):
        """One gol_step call's worth of turns: exchanges where the halos run out; check(engine,
        turns of this stretch) after every engine's step."""
        left = turns
        while left:
            if self.engs[0].halo_valid == 0:
                self.exchange()
            m = min(left, self.engs[0].halo_valid)
            for e in self.engs:
                e.step(m)
                if check:
                    check(e, m)
            left -= m

    def read(self):
        return np.concatenate([e.read_packed() for e in self.engs])


def _tile_launch_check(tw, code, tpl):
    """Every launch of the last step ran k_step_tile on exactly this shape: a silent fall-back
    to one-turn launches or to another kernel or code fails here."""
    def check(e, m):
        plan = e.last_launches()
        assert plan and [v for _, v, _ in plan] == [15] * len(plan), plan
        assert [k for k, _, _ in plan] == S.even_split(m, tpl), (m, plan)
        tiles = e.last_launch_tiles()
        assert [(a, b) for a, b, _ in tiles] == [(tw, code)] * len(plan), tiles
        assert all(1 <= v <= S.MAX_WAVES for _, _, v in tiles), tiles
        assert e.info().turns_per_launch == tpl
    return check


# --------------------------------------------------------- 1. every code, ragged strips
def _code_params():
    out = []
    for code in list(TILE_CODES) + [pytest.param(c, marks=tools_only) for c in S.TOOLS_CODES]:
        c = code.values[0] if hasattr(code, "values") else code
        tw, th = S.code_tile_w(c), S.code_tile_h(c)        # raises where no height exists
        assert S.tile_shape_ok(S.CODE_W // 64, S.CODE_TPL, th, tw, c)
        assert 1 <= S.tile_waves(S.CODE_TPL, th, tw, c) <= S.MAX_WAVES
        out.append(code)
    return out


@pytest.mark.parametrize("code", _code_params())
def test_tile_code_strips(gol, oracle, monkeypatch, code):
    """Every k_step_tile instantiation on three ragged strips of a 4224 x 157 board (53 / 52 /
    52 rows, 11-row halos): a window runs as a 6-turn launch and a 5-turn launch that starts 6
    turns in; 29 turns = two windows and a 7-turn one.  Partial last tile column, a short last
    tile row at every launch, several waves per workgroup.  The board is compared after the
    first window and at the end."""
    tw, th = S.code_tile_w(code), S.code_tile_h(code)
    w, h, n, halo, tpl = S.CODE_W, S.CODE_H, S.CODE_N, S.CODE_HALO, S.CODE_TPL
    _pin_tile(monkeypatch, tw, code)
    start = oracle.gen_random(code + 11, w, h)
    check = _tile_launch_check(tw, code, tpl)

    def check_waves(e, m):
        check(e, m)
        assert all(v > 1 for _, _, v in e.last_launch_tiles())

    with _Strips(gol, start, w, n, halo, band_rows=th, turns_per_launch=tpl) as s:
        assert [e.info().band_rows for e in s.engs] == [th] * n
        s.step(S.CODE_WINDOWS[0], check_waves)
        assert [k for k, _, _ in s.engs[0].last_launches()] == [6, 5]
        mid = s.read()
        s.step(sum(S.CODE_WINDOWS[1:]), check_waves)
        assert [k for k, _, _ in s.engs[0].last_launches()] == [7]
        got = s.read()
    want_mid = oracle.bit_run(start, w, S.CODE_WINDOWS[0])
    assert np.array_equal(mid, want_mid)
    assert np.array_equal(got, oracle.bit_run(want_mid, w, sum(S.CODE_WINDOWS[1:])))


# --------------------------------------------------------- 2. strip edge shapes
@pytest.mark.parametrize("name,code", S.edge_cases())
def test_tile_strip_edges(gol, oracle, monkeypatch, name, code):
    """One code per family (turn orders 0, 1, 2, 4, 5, 6 at one word per lane; 0, 1, 2 at two)
    on the strip shapes of strip_tiles.EDGE_SHAPES: strips that are all halo, a strip that is
    its own neighbour, ragged splits, halos deeper than the tile, 40- and 64-turn windows, a
    one-tile-column board, one lane group per wave, and a call that ends mid-window."""
    shape = S.EDGE_SHAPES[name]
    w, h, n, halo, tpl, th = (shape[k] for k in ("w", "h", "n", "halo", "tpl", "th"))
    tw = S.edge_tile_w(shape, code)
    _pin_tile(monkeypatch, tw, code)
    start = oracle.gen_random(code * 3 + h, w, h)
    check = _tile_launch_check(tw, code, tpl)
    want = start
    with _Strips(gol, start, w, n, halo, band_rows=th, turns_per_launch=tpl) as s:
        for turns in shape["steps"]:
            s.step(turns, check)
            want = oracle.bit_run(want, w, turns)
            assert np.array_equal(s.read(), want), turns


# --------------------------------------------------------- 3. the split launch
# The receives of a window are held back on the transport stream behind a chain of large
# device-to-device copies.  Measured on an MI355X with torch events: the undelayed first launch
# of the largest case here (4224 wide, 150-row strips, 128-row halos, code 516: one 32-turn
# launch as interior + two boundary launches and the join) takes 136-152 us on the engine's
# stream over ten runs (FIRST_LAUNCH_US); a chain of 24 copies of 256 MiB takes 2340-2353 us
# (DELAY_US: 15 times the slowest launch; 8 copies 780-890 us, 16 copies 1565-1700 us).  So the
# interior launch has long finished, and a boundary launch that did not wait for the receives
# would have run on the poison, when the rows land.  With step_overlap replaced by halo_done +
# step (no ordering after the transport stream) the comparison failed in 73 of the 74 cases
# below, k_step_tile and one-turn launches alike; the one that passed was the first of the
# process (streams that share a hardware queue run in submission order, which hides a missing
# wait, so a single case proves less than the table does).  No timing is asserted.
FIRST_LAUNCH_US = 152
DELAY_US = 2340
DELAY_COPIES = 24
DELAY_BYTES = 256 << 20
POISON = 0x5A5A5A5A5A5A5A5A
assert DELAY_US >= 10 * FIRST_LAUNCH_US


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def delay_buffers(torch):
    a = torch.zeros(DELAY_BYTES // 8, dtype=torch.int64, device="cuda:0")
    b = torch.zeros_like(a)
    yield a, b


def _run_split(gol, oracle, torch, monkeypatch, case, delay_buffers, step=None):
    """Run a split-launch case; returns (strips' boards, the torus start, per-strip engines'
    turn counts or None).  step(engine, m, xs): the overlapped step (default step_overlap)."""
    from gol.distributed import _DeviceRows
    mv, code, w, n, halo, tpl = (case[k] for k in ("mv", "code", "w", "n", "halo", "tpl"))
    h = case["h"][n]
    counts = bool(case.get("counts"))
    kw = dict(band_rows=case["band"], turns_per_launch=tpl, count_every_turn=counts)
    if mv:
        monkeypatch.setenv("GOL_MULTI_VARIANT", str(mv))
    if mv == 15:
        monkeypatch.setenv("GOL_TILE", f"{S.split_tile_w(code)},{code}")
        kw["band_rows"] = S.SPLIT_TILE_H
    if step is None:
        step = lambda e, m, xs: e.step_overlap(m, xs.cuda_stream)      # noqa: E731
    dev = torch.device("cuda", 0)
    start = oracle.gen_random(mv * 100 + code + w + n, w, h)
    a, b = delay_buffers
    with _Strips(gol, start, w, n, halo, **kw) as s:
        streams = [torch.cuda.Stream(dev) for _ in s.engs]
        xs = torch.cuda.Stream(dev)
        for e, st in zip(s.engs, streams):
            e.set_stream(st.cuda_stream)
        nw = s.engs[0].words_per_row
        for m in case["windows"]:
            views, layouts = [], []
            for e in s.engs:
                ptrs, lay = e.halo_buffers()
                views.append([torch.as_tensor(_DeviceRows(p, (halo, nw)), device=dev)
                              for p in ptrs])
                layouts.append(lay)
            assert len(set(layouts)) == 1, layouts
            for e in s.engs:
                e.stream_wait(xs.cuda_stream)
            with torch.cuda.stream(xs):
                for _, _, rt, rb in views:
                    rt.fill_(POISON)
                    rb.fill_(POISON)
                for _ in range(DELAY_COPIES // 2):
                    b.copy_(a, non_blocking=True)
                    a.copy_(b, non_blocking=True)
                for i, (_, _, rt, rb) in enumerate(views):
                    rt.copy_(views[(i - 1) % n][1], non_blocking=True)   # upper's send_bottom
                    rb.copy_(views[(i + 1) % n][0], non_blocking=True)   # lower's send_top
            for e in s.engs:
                step(e, m, xs)
            if mv == 15 and tpl > 1 and not counts and all(k >= 2 for k in S.even_split(m, tpl)):
                for e in s.engs:
                    _tile_launch_check(S.split_tile_w(code), code, tpl)(e, m)
        got = s.read()
        total = sum(case["windows"])
        tc = sum(e.turn_counts(1, total) for e in s.engs) if counts else None
        xs.synchronize()
    return got, start, tc


_SPLIT = S.split_cases()
assert all(S.split_ok(c) for _, c in _SPLIT)


@pytest.mark.parametrize("case", [c for _, c in _SPLIT], ids=[i for i, _ in _SPLIT])
def test_split_launch_parity(gol, oracle, torch, monkeypatch, delay_buffers, case):
    """gol_step_overlap with the halo rows poisoned and their receives delayed on the transport
    stream: n strips on their own streams, every kernel (mv 7, 8, 9, 13; 12 and 14, whose split
    launch runs as helix; k_step_tile codes, whose boundary launches run on 16-row tiles), the
    one-turn split, windows whose first launch has no interior rows, partial windows followed
    by further ones, and engines with per-turn counts (no split: the launch waits whole)."""
    got, start, tc = _run_split(gol, oracle, torch, monkeypatch, case, delay_buffers)
    total = sum(case["windows"])
    if tc is None:
        want = oracle.bit_run(start, case["w"], total)
    else:
        want, wc = oracle.bit_run(start, case["w"], total, counts=True)
        assert tc.tolist() == wc.astype(np.int64).tolist()
    assert np.array_equal(got, want)
