// gol_window.h — rectangular windows of the board (gol_window.hip, the window calls of
// gol_io.cpp): the word fetch the window kernels and its host build gol_window_word share, and
// the kernels' launch interface.  Internal: not part of the C ABI.
//
// A window is w x h cells whose top-left cell is (x, y); column x + i means (x + i) mod width,
// row y + j means (y + j) mod height.  The kernels work on the board in whichever layout it is
// in (standard, or interleaved: even cells in a word's low dword, odd cells in the high one) and
// convert single words in registers, so a window call costs what the window covers and never a
// pass over the buffer.  Every element offset is size_t row x pitch: a buffer may be 2 GiB or
// more and the window may lie past byte 2^32 of it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace golk {

// one word between the layouts: the perfect shuffle and its inverse, five delta swaps each
// (Hacker's Delight 7-2; k_il_convert's pair, here for the host as well)
__host__ __device__ inline uint64_t win_dswap(uint64_t v, int s, uint64_t m)
{
    const uint64_t t = (v ^ (v >> s)) & m;
    return v ^ t ^ (t << s);
}
__host__ __device__ inline uint64_t win_to_il(uint64_t v)
{
    v = win_dswap(v, 1, 0x2222222222222222ull);
    v = win_dswap(v, 2, 0x0C0C0C0C0C0C0C0Cull);
    v = win_dswap(v, 4, 0x00F000F000F000F0ull);
    v = win_dswap(v, 8, 0x0000FF000000FF00ull);
    return win_dswap(v, 16, 0x00000000FFFF0000ull);
}
__host__ __device__ inline uint64_t win_to_std(uint64_t v)
{
    v = win_dswap(v, 16, 0x00000000FFFF0000ull);
    v = win_dswap(v, 8, 0x0000FF000000FF00ull);
    v = win_dswap(v, 4, 0x00F000F000F000F0ull);
    v = win_dswap(v, 2, 0x0C0C0C0C0C0C0C0Cull);
    return win_dswap(v, 1, 0x2222222222222222ull);
}

// The 64 cells at columns col .. col + 63 (mod width) of one row, in standard order: bit b =
// cell (col + b) mod width.  row: the row's ceil(width / 64) words in the standard layout or
// (il) the interleaved one; 0 <= col < width, width >= 2.
// The trap: with r = width % 64 != 0 the 64 cells can span THREE words -- the tail of word
// L - 1, the r cells of the last word L, then word 0 -- so "this word and the next" is not
// enough; and a row narrower than 64 cells wraps more than once (its cells repeat in the
// answer).  Hence the loop: each pass takes what is left of the word under the cursor, up to the
// row's end, and the cursor wraps to column 0.  Padding bits are masked out, not trusted.
__host__ __device__ inline uint64_t window_word(const uint64_t *row, int width, int col, bool il)
{
    uint64_t out = 0;
    int got = 0, c = col;
    while (got < 64) {
        const int j = c >> 6, b = c & 63;
        const int in_word = width - 64 * j < 64 ? width - 64 * j : 64;   // cells word j holds
        int take = in_word - b;
        if (take > 64 - got) take = 64 - got;
        uint64_t v = row[j];
        if (il) v = win_to_std(v);
        v >>= b;
        if (take < 64) v &= (1ull << take) - 1;
        out |= v << got;
        got += take;
        c += take;
        if (c >= width) c = 0;
    }
    return out;
}

// ---- launches (gol_window.hip).  Window geometry common to the three:
//   words / width / nw / pitch / il   board[cur] and its layout
//   modrows, brow0                    window row j is buffer row (brow0 + j) mod modrows
//   x, w                              the window's first column and width
// k_window_unpack: window rows [row0, row0 + nrows) -> bytes (nrows x w, 0 / 255, row stride w)
hipError_t launch_window_unpack(const uint64_t *words, int width, int pitch, bool il, int modrows,
                                int brow0, int x, int w, int row0, int nrows, uint8_t *bytes,
                                hipStream_t s);
// k_window_density: window rows [row0, row0 + nrows) (row0 a multiple of block) added into
// counts[(j - row0) / block][i / block], ceil(w / block) per row (caller zeroes)
hipError_t launch_window_density(const uint64_t *words, int width, int pitch, bool il, int modrows,
                                 int brow0, int x, int w, int row0, int nrows, int block,
                                 uint32_t *counts, hipStream_t s);
// k_window_pack: buffer rows [b0, b0 + nrows) take the byte rows bytes[r .. r + nrows) (row
// stride w; 255 = alive) at columns x .. x + w - 1 (mod width); cells outside stay, the bits
// past `width` in the last word are stored as 0
hipError_t launch_window_pack(uint64_t *words, int width, int nw, int pitch, bool il, int b0,
                              int nrows, int x, int w, const uint8_t *bytes, hipStream_t s);

}  // namespace golk
