"""The K1t kernels whose turn runs under the VGPR parity plan (csrc/gol_tile.h, tile_parity_pins)
at their own pinned launch shape: code 516 at K = 30 on 30 x 452 tiles (kKnownShapes, the 65536^2
entry), on the smallest board that has two full tile columns, a repacked narrow column and a
short last tile row: 4096 x 941 (64 words: 30 + 30 + 4; 941 = 452 + 452 + 37 rows).  The other
suites run this code at other depths and tile heights.

The bottom-edge LDS array of a pinned turn holds its sums in another order than the top-edge one,
and every row's rule writes registers named by the plan over sums that die in it; a slip in
either shows in every segment of every tile.  Each case is pinned as test_gpu_tile_sweep.py pins
it, asserts its launches, and compares bit for bit with oracle.bit_run, computed once for all
cases.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 4096, 941
K, TH, TW, CODE, WAVES = 30, 452, 30, 516, 16
SEED = 516


@pytest.fixture(scope="module")
def gol():
    import gol as g
    return g


@pytest.fixture(scope="module")
def ref(oracle):
    """start, the board after K turns, the board after 3 K - 1, and the per-turn counts."""
    start = oracle.gen_random(SEED, W, H)
    mid, c0 = oracle.bit_run(start, W, K, counts=True)
    end, c1 = oracle.bit_run(mid, W, 2 * K - 1, counts=True)
    for a in (start, mid, end):
        a.setflags(write=False)
    return start, mid, end, np.concatenate([c0, c1]).astype(np.int64).tolist()


def _pin(monkeypatch):
    monkeypatch.setenv("GOL_MULTI_VARIANT", "15")
    monkeypatch.setenv("GOL_TILE", f"{TW},{CODE}")


def _two_steps(gol, ref, **kw):
    """step(K), then step(2 K - 1) as launches of K and K - 1; every launch is the tile kernel at
    code 516 in 16-wave workgroups."""
    start, want_mid, want, _ = ref
    with gol.Engine(W, H, device=0, band_rows=TH, turns_per_launch=K, **kw) as e:
        info = e.info()
        assert info.turns_per_launch == K and info.band_rows == TH
        e.load_packed(start)
        e.step(K)
        assert e.last_launches() == [(K, 15, TH)]
        tiles = e.last_launch_tiles(blocks=True)
        assert tiles and all(t == (TW, CODE, WAVES, K) for t in tiles), tiles
        mid = e.read_packed()
        e.step(2 * K - 1)
        assert sorted(e.last_launches()) == [(K - 1, 15, TH), (K, 15, TH)]
        tiles = e.last_launch_tiles(blocks=True)
        assert {t[:3] for t in tiles} == {(TW, CODE, WAVES)}, tiles
        assert sorted(t[3] for t in tiles) == [K - 1, K], tiles
        got = e.read_packed()
        counts = e.turn_counts(1, 3 * K - 1) if kw.get("count_every_turn") else None
    assert np.array_equal(mid, want_mid)
    assert np.array_equal(got, want)
    return counts


def test_plain(gol, ref, monkeypatch):
    """k_step_tile<16,5,1>."""
    _pin(monkeypatch)
    _two_steps(gol, ref)


def test_counted(gol, ref, monkeypatch):
    """k_step_tile_cnt<16,5,1>: the boards and all 3 K - 1 per-turn counts."""
    _pin(monkeypatch)
    counts = _two_steps(gol, ref, count_every_turn=True)
    assert counts.tolist() == ref[3]


def test_big(gol, ref, monkeypatch):
    """k_step_tile_big<16,5>: the windowed form forced on the same board (not pinned: it shares
    the shape and the engine's big-board path with the pinned kernels)."""
    _pin(monkeypatch)
    monkeypatch.setenv("GOL_TILE_BIG", "1")
    _two_steps(gol, ref)


def test_chunked_long_step(gol, ref, monkeypatch):
    """One step of 3 K - 1 turns with GOL_STEP_CHUNKS=4: three launches, each cut into the row
    chunks the planner fits, consecutive launches overlapping."""
    from gol import _native as N
    _pin(monkeypatch)
    monkeypatch.setenv("GOL_STEP_CHUNKS", "4")
    cap = 64
    n2 = (ctypes.c_int32 * 2)()
    b0, b1 = (ctypes.c_int32 * (cap + 1))(), (ctypes.c_int32 * (cap + 1))()
    deps = (ctypes.c_uint8 * (cap * cap))()
    assert N.lib().gol_step_chunk_plan(H, K, TH, 4, K, TH, 4, n2, b0, b1, deps, cap) == 0
    nchunks = n2[0]
    assert nchunks >= 2
    start, _, want, _ = ref
    with gol.Engine(W, H, device=0, band_rows=TH, turns_per_launch=K) as e:
        e.load_packed(start)
        e.step(3 * K - 1)
        plan = e.last_launches()
        assert sorted(k for k, _, _ in plan) == [K - 1, K, K], plan
        assert all(v == 15 and b == TH for _, v, b in plan), plan
        assert {t[:3] for t in e.last_launch_tiles(blocks=True)} == {(TW, CODE, WAVES)}
        assert e.last_step_chunks() == 3 * nchunks
        got = e.read_packed()
    assert np.array_equal(got, want)
