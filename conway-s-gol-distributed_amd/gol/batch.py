"""BatchEngine: a Python handle on one gol_batch (include/gol_amd.h, "Batch").

Many torus boards of one shape narrower than 256 cells in one device buffer, every step one
k_step_resident_batch launch per 256 turns with one workgroup per board -- what a soup search, a
rule statistic or a sweep over seeds runs thousands of.  step_settle() is the same step with a
watch on every board (k_settle_resident_batch): settled() gives each board's period and the turn
it was found at, and a board known to repeat skips its settled turns.  No reference counterpart:
its Server runs one board.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple

import numpy as np

from . import _native as N


class BatchInfo(NamedTuple):
    width: int
    height: int
    boards: int
    words_per_row: int
    lanes: int
    rows_per_lane: int
    waves: int
    turn: int


class BatchEngine:
    def __init__(self, width: int, height: int, boards: int, *, device: int = -1,
                 count_every_turn: bool = False):
        L = N.lib()
        h = ctypes.c_void_p()
        flags = N.GOL_FLAG_COUNT_EVERY_TURN if count_every_turn else 0
        N.check(L.gol_batch_create(int(width), int(height), int(boards), int(device), flags,
                                   ctypes.byref(h)))
        self._h = h
        self._L = L
        i = self.info
        self.width, self.height, self.boards = i.width, i.height, i.boards
        self.words_per_row = i.words_per_row

    # -- lifetime
    def close(self):
        if getattr(self, "_h", None):
            self._L.gol_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def handle(self):
        return self._h

    def _c(self, rc):
        if rc < 0:
            msg = self._L.gol_strerror(rc).decode()
            detail = self._L.gol_batch_last_error(self._h)
            if detail:
                msg += ": " + detail.decode()
            raise N.GolError(rc, msg)
        return rc

    # -- info
    @property
    def info(self) -> BatchInfo:
        v = [ctypes.c_int32() for _ in range(7)]
        t = ctypes.c_int64()
        self._c(self._L.gol_batch_get_info(self._h, *(ctypes.byref(x) for x in v),
                                           ctypes.byref(t)))
        return BatchInfo(*(int(x.value) for x in v), int(t.value))

    @property
    def turn(self) -> int:
        return self.info.turn

    def occupancy(self):
        """(workgroups per CU, CUs): boards x what one launch keeps resident at once."""
        a, b = ctypes.c_int32(), ctypes.c_int32()
        self._c(self._L.gol_batch_occupancy(self._h, ctypes.byref(a), ctypes.byref(b)))
        return int(a.value), int(b.value)

    def stream(self) -> int:
        return int(self._L.gol_batch_get_stream(self._h) or 0)

    def sync(self):
        self._c(self._L.gol_batch_sync(self._h))

    def _range(self, first, n):
        first = int(first)
        return first, int(self.boards - first if n is None else n)

    # -- boards
    def load_packed(self, words: np.ndarray, first: int = 0):
        """uint64 (n, height, words_per_row): boards first .. first + n - 1."""
        w = np.ascontiguousarray(words, dtype=np.uint64)
        if w.ndim != 3 or w.shape[1:] != (self.height, self.words_per_row):
            raise ValueError(f"expected (n, {self.height}, {self.words_per_row}), got {w.shape}")
        self._c(self._L.gol_batch_load_packed(self._h, int(first), w.shape[0],
                                              w.ctypes.data_as(N._u64p)))

    def load(self, cells: np.ndarray, first: int = 0):
        """uint8 (n, height, width), 255 = alive, anything else dead."""
        b = np.ascontiguousarray(cells, dtype=np.uint8)
        if b.ndim != 3 or b.shape[1:] != (self.height, self.width):
            raise ValueError(f"expected (n, {self.height}, {self.width}), got {b.shape}")
        self._c(self._L.gol_batch_load(self._h, int(first), b.shape[0], b.ctypes.data_as(N._u8p)))

    def fill_random(self, seed: int):
        """Board i, row y = row i * height + y of Engine(width, boards * height).fill_random."""
        self._c(self._L.gol_batch_fill_random(self._h, ctypes.c_uint64(int(seed))))

    def step(self, turns: int = 1):
        self._c(self._L.gol_batch_step(self._h, int(turns)))

    def step_settle(self, turns: int = 1):
        """step(), watching every board for its period and skipping the turns of a board known
        to repeat (include/gol_amd.h, "Settle"); the boards end where step() puts them."""
        self._c(self._L.gol_settle_step(self._h, int(turns)))

    def settled(self, first: int = 0, n: int | None = None):
        """(settled_turn, period) of boards first .. first + n - 1 as int64 arrays: -1 and 0
        while a board's period is unknown."""
        first, n = self._range(first, n)
        turn = np.zeros(max(n, 1), dtype=np.int64)
        period = np.zeros(max(n, 1), dtype=np.int64)
        self._c(self._L.gol_settle_read(self._h, first, n, turn.ctypes.data_as(N._i64p),
                                        period.ctypes.data_as(N._i64p)))
        return turn[:n], period[:n]

    def read_packed(self, first: int = 0, n: int | None = None) -> np.ndarray:
        first, n = self._range(first, n)
        out = np.zeros((max(n, 1), self.height, self.words_per_row), dtype=np.uint64)
        self._c(self._L.gol_batch_read_packed(self._h, first, n, out.ctypes.data_as(N._u64p)))
        return out[:n]

    def read(self, first: int = 0, n: int | None = None) -> np.ndarray:
        first, n = self._range(first, n)
        out = np.zeros((max(n, 1), self.height, self.width), dtype=np.uint8)
        self._c(self._L.gol_batch_read(self._h, first, n, out.ctypes.data_as(N._u8p)))
        return out[:n]

    def alive(self, first: int = 0, n: int | None = None) -> np.ndarray:
        first, n = self._range(first, n)
        out = np.zeros(max(n, 1), dtype=np.int64)
        self._c(self._L.gol_batch_alive(self._h, first, n, out.ctypes.data_as(N._i64p)))
        return out[:n]

    def turn_counts(self, first_turn: int, n: int) -> np.ndarray:
        """int64 (n, boards): the alive cells of every board after turns first_turn ..."""
        n = int(n)
        out = np.zeros((max(n, 1), self.boards), dtype=np.int64)
        self._c(self._L.gol_batch_turn_counts(self._h, int(first_turn), n,
                                              out.ctypes.data_as(N._i64p)))
        return out[:n]
