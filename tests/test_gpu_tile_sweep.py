"""k_step_tile, k_step_tile_cnt and k_step_tile_seam at every shape class the create-time tile
search can pick (tile_sweep.py): every code of the library's lists on exactly full tiles --
th = wv G SEG - 2 K, no spare segment, the last segment's last row a needed halo row -- at every
lane grouping (G = 21 .. 1, with and without idle lanes), at the search's floor (K = 8 in its
smallest workgroup) and at 16 waves under its deepest K (waves that leave the trapezoid early),
and one code per family at every tile width.

The reference everywhere is oracle.bit_run from oracle.gen_random, compared bit for bit.  Every
case asserts its launches (kernel, depth, tile height, tile width, code and waves per workgroup),
so none passes on another shape or on one turn per launch.  test_tile_sweep_cpu.py checks the
table against the library without a GPU; no case here skips.
"""
import numpy as np
import pytest

import tile_sweep as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gol():
    import gol as g
    return g


def _params(kind):
    cases = T.cases_of(kind)
    return pytest.mark.parametrize("c", cases, ids=[T.case_id(c) for c in cases])


def _pin(monkeypatch, c):
    monkeypatch.setenv("GOL_MULTI_VARIANT", "15")
    monkeypatch.setenv("GOL_TILE", f"{c.tw},{c.code}")


def _run(gol, oracle, c, seam=False):
    """step(K), then step(2 K - 1) as launches of K and K - 1 (the odd depth ends a paired turn
    loop on a single turn); both boards against the oracle's."""
    K = c.K
    start = oracle.gen_random(c.seed, c.w, c.h)
    with gol.Engine(c.w, c.h, device=0, band_rows=c.th, turns_per_launch=K) as e:
        info = e.info()
        assert info.turns_per_launch == K and info.band_rows == c.th
        assert not seam or info.fast_path == 0
        e.load_packed(start)
        e.step(K)
        assert e.last_launches() == [(K, 15, c.th)]
        tiles = e.last_launch_tiles(blocks=True)
        assert tiles and all(t == (c.tw, c.code, c.wv, K) for t in tiles), tiles
        mid = e.read_packed()
        e.step(2 * K - 1)
        plan = e.last_launches()
        assert sorted(plan) == [(K - 1, 15, c.th), (K, 15, c.th)], plan
        tiles = e.last_launch_tiles(blocks=True)
        assert {t[:2] for t in tiles} == {(c.tw, c.code)}, tiles
        assert {t[3] for t in tiles} == {K, K - 1}, tiles
        got = e.read_packed()
        alive = e.snapshot() if seam else None
    want_mid = oracle.bit_run(start, c.w, K)
    want = oracle.bit_run(want_mid, c.w, 2 * K - 1)
    assert np.array_equal(mid, want_mid)
    assert np.array_equal(got, want)
    if seam:
        # (the popcount reads every bit of the last word: its padding stayed zero)
        assert alive == (3 * K - 1, oracle.popcount(want, c.w))


@_params("plain")
def test_sweep_plain(gol, oracle, monkeypatch, c):
    """k_step_tile: every gol_tile_codes code at the sweep widths in cases A and B, and the edge
    codes at every tile width in case A."""
    _pin(monkeypatch, c)
    _run(gol, oracle, c)


@_params("seam")
def test_sweep_seam(gol, oracle, monkeypatch, c):
    """k_step_tile_seam: every gol_tile_seam_codes code on boards whose last word holds 1 or 40
    cells; the board, and the alive count after the last step."""
    _pin(monkeypatch, c)
    _run(gol, oracle, c, seam=True)


@_params("count")
def test_sweep_count(gol, oracle, monkeypatch, c):
    """k_step_tile_cnt: every gol_tile_count_codes code on a count engine -- the boards and all
    3 K - 1 per-turn counts (which waves count, and which only partly, follows from G)."""
    _pin(monkeypatch, c)
    K = c.K
    turns = 3 * K - 1
    start = oracle.gen_random(c.seed, c.w, c.h)
    with gol.Engine(c.w, c.h, device=0, band_rows=c.th, turns_per_launch=K,
                    count_every_turn=True) as e:
        e.load_packed(start)
        done = 0
        boards = []
        for n in (K, 2 * K - 1):
            e.step(n)
            plan = e.last_launches()
            assert plan and all(v == 15 and b == c.th for _, v, b in plan), plan
            assert max(k for k, _, _ in plan) == K and sum(k for k, _, _ in plan) == n, plan
            tiles = e.last_launch_tiles(blocks=True)
            assert {t[:2] for t in tiles} == {(c.tw, c.code)}, tiles
            assert all(t[2] == c.wv for t in tiles if t[3] == K), tiles
            assert sorted(t[3] for t in tiles) == sorted(k for k, _, _ in plan), tiles
            boards.append(e.read_packed())
            done += n
        counts = e.turn_counts(1, turns)
    want_mid, wc_mid = oracle.bit_run(start, c.w, K, counts=True)
    want, wc = oracle.bit_run(want_mid, c.w, 2 * K - 1, counts=True)
    assert done == turns
    assert counts.tolist() == np.concatenate([wc_mid, wc]).astype(np.int64).tolist()
    assert np.array_equal(boards[0], want_mid)
    assert np.array_equal(boards[1], want)
