// gol_window.hip — K6: rectangular windows of the board (gol_read_window, gol_window_density,
// gol_write_window).  The reference shows a board one pixel per cell (Local/sdl) and moves it
// whole ([][]uint8 over RPC); at 65536^2 and beyond a caller inspects, seeds and patches parts.
//
//   k_window_unpack   window -> staging bytes (0 / 255)
//   k_window_density  window -> alive counts per block x block cells
//   k_window_pack     staging bytes -> board words
//
// All three run on board[cur] as it is: a word of the interleaved layout is converted in
// registers (window_word, win_to_il), so no call converts the buffer or touches a row outside the
// window.  Row offsets are size_t row x pitch (buffers of 2 GiB and more).  The read kernels are
// organised by window word -- one thread per 64 window cells, fetched by window_word across the
// row's seam and wrap; the pack kernel by destination word -- one thread owns one (buffer row,
// word) and does one read-modify-write of it, so no two threads write a word.
// The byte side moves 16 bytes per access when a row of the window is a whole number of 16-byte
// units (k_pack / k_unpack's rule), else single bytes.
#include "gol_device.h"
#include "gol_window.h"

namespace golk {

namespace {

__device__ __forceinline__ uint64_t low_mask(int n) { return n >= 64 ? ~0ull : (1ull << n) - 1; }

inline int window_grid(long long total)
{
    long long g = (total + 255) / 256;
    if (g < 1) g = 1;
    return (int)(g > 4096 ? 4096 : g);
}

}  // namespace

// One thread per (window row, 64-column group of the window).
__global__ __launch_bounds__(256) void k_window_unpack(const uint64_t *__restrict__ words, int width,
                                                       int pitch, int il, int modrows, int brow0,
                                                       int x, int w, int row0, int nrows,
                                                       uint8_t *__restrict__ bytes)
{
    const int G = (w + 63) >> 6;
    const long long total = (long long)nrows * G;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const int r = (int)(i / G), g = (int)(i % G);
        const long long b = ((long long)brow0 + row0 + r) % modrows;
        const int col = (int)(((long long)x + 64ll * g) % width);
        const uint64_t v = window_word(words + (size_t)b * pitch, width, col, il != 0);
        uint8_t *dst = bytes + (size_t)r * w + (size_t)64 * g;
        const int n = min(64, w - 64 * g);
        if (n == 64 && (w & 15) == 0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                uint32_t d[4];
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const uint32_t bits = (uint32_t)(v >> (16 * q + 4 * m)) & 0xfu;
                    d[m] = ((bits & 1u) ? 0xffu : 0u) | ((bits & 2u) ? 0xff00u : 0u) |
                           ((bits & 4u) ? 0xff0000u : 0u) | ((bits & 8u) ? 0xff000000u : 0u);
                }
                reinterpret_cast<uint4 *>(dst)[q] = make_uint4(d[0], d[1], d[2], d[3]);
            }
        } else {
            for (int k = 0; k < n; ++k) dst[k] = ((v >> k) & 1ull) ? 255 : 0;
        }
    }
}

// One thread per (window row, 64-column group); its cells fall into one block column or more.
// The first piece goes through a wave sum when the whole wavefront adds to one entry (blocks of
// 4096 cells over a wide window: one atomic per wavefront instead of 64), the rest by atomics of
// their own.  The loop is wave-uniform: i0 is the wavefront's first item.
__global__ __launch_bounds__(256) void k_window_density(const uint64_t *__restrict__ words,
                                                        int width, int pitch, int il, int modrows,
                                                        int brow0, int x, int w, int row0,
                                                        int nrows, int block,
                                                        uint32_t *__restrict__ counts)
{
    const int G = (w + 63) >> 6;
    const int nbx = (w + block - 1) / block;
    const long long total = (long long)nrows * G;
    const int lane = threadIdx.x & 63;
    for (long long i0 = (long long)blockIdx.x * blockDim.x + (threadIdx.x & ~63); i0 < total;
         i0 += (long long)gridDim.x * blockDim.x) {
        const long long i = i0 + lane;
        const bool valid = i < total;
        long long idx = -1;
        unsigned cnt = 0;
        uint64_t rest = 0;
        int p = 0, pend = 0;
        size_t rowbase = 0;
        if (valid) {
            const int r = (int)(i / G), g = (int)(i % G);
            const long long b = ((long long)brow0 + row0 + r) % modrows;
            const int col = (int)(((long long)x + 64ll * g) % width);
            const int n = min(64, w - 64 * g);
            const uint64_t v = window_word(words + (size_t)b * pitch, width, col, il != 0) & low_mask(n);
            p = 64 * g;
            pend = p + n;
            rowbase = (size_t)(r / block) * nbx;
            const int I = p / block;
            const int len = (int)min((long long)pend, ((long long)I + 1) * block) - p;
            idx = (long long)(rowbase + I);
            cnt = (unsigned)__builtin_popcountll(v & low_mask(len));
            rest = len >= 64 ? 0ull : v >> len;
            p += len;
        }
        const long long ref = __shfl(idx, 0, 64);          // (lane 0 is valid: i0 < total)
        if (__all(!valid || (idx == ref && p >= pend))) {
            const unsigned long long s = wave_sum((unsigned long long)cnt);
            if (lane == 0 && s) atomicAdd(counts + ref, (uint32_t)s);
        } else if (valid) {
            if (cnt) atomicAdd(counts + idx, cnt);
            while (p < pend) {                             // (the first piece was shorter than 64)
                const int I = p / block;
                const int len = (int)min((long long)pend, ((long long)I + 1) * block) - p;
                const unsigned c = (unsigned)__builtin_popcountll(rest & low_mask(len));
                if (c) atomicAdd(counts + rowbase + I, c);
                rest >>= len;
                p += len;
            }
        }
    }
}

// `len` (1 .. 64) cells from bytes: bit k = (src[k] == 255)
__device__ __forceinline__ uint64_t window_gather(const uint8_t *__restrict__ src, int len)
{
    uint64_t bits = 0;
    if (len == 64 && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint4 v = reinterpret_cast<const uint4 *>(src)[q];
            const uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 16; ++k)
                bits |= (uint64_t)(((d[k >> 2] >> (8 * (k & 3))) & 0xffu) == 255u) << (16 * q + k);
        }
    } else {
        for (int k = 0; k < len; ++k) bits |= (uint64_t)(src[k] == 255u) << k;
    }
    return bits;
}

// One thread per (buffer row of the run, word the window touches): words jstart, jstart + 1, ...
// (mod nw), ntouch of them, each once.  The window's columns are the cyclic interval [x, x + w):
// the part up to the row's end and, when it wraps, the part from column 0 on; a word meets each
// in at most one run of bits.  A word the window covers whole is stored without the read; the
// bits past `width` in the last word are stored as 0.
__global__ __launch_bounds__(256) void k_window_pack(uint64_t *__restrict__ words, int width, int nw,
                                                     int pitch, int il, int b0, int nrows, int x,
                                                     int w, int jstart, int ntouch,
                                                     const uint8_t *__restrict__ bytes)
{
    const long long total = (long long)nrows * ntouch;
    const long long xe = (long long)x + w;                 // one past the window's last column
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const int r = (int)(i / ntouch), j = (int)((jstart + i % ntouch) % nw);
        const uint8_t *src = bytes + (size_t)r * w;
        const int c0 = 64 * j, n = min(64, width - c0);
        uint64_t mask = 0, val = 0;
        {
            const int lo = max(c0, x), hi = (int)min((long long)(c0 + n), min(xe, (long long)width));
            if (lo < hi) {
                mask |= low_mask(hi - lo) << (lo - c0);
                val |= window_gather(src + (lo - x), hi - lo) << (lo - c0);
            }
        }
        if (xe > width) {
            const int hi = (int)min((long long)(c0 + n), xe - width);
            if (c0 < hi) {
                mask |= low_mask(hi - c0);
                val |= window_gather(src + (size_t)(c0 + width - x), hi - c0);
            }
        }
        if (!mask) continue;
        const uint64_t keep = low_mask(n);
        uint64_t *dst = words + (size_t)(b0 + r) * pitch + j;
        uint64_t v = val;
        if (mask != keep) {
            uint64_t old = *dst;
            if (il) old = win_to_std(old);
            v = ((old & ~mask) | val) & keep;
        }
        *dst = il ? win_to_il(v) : v;
    }
}

// ------------------------------------------------------------------ launches
hipError_t launch_window_unpack(const uint64_t *words, int width, int pitch, bool il, int modrows,
                                int brow0, int x, int w, int row0, int nrows, uint8_t *bytes,
                                hipStream_t s)
{
    if (nrows <= 0) return hipSuccess;
    const int g = window_grid((long long)nrows * ((w + 63) / 64));
    hipLaunchKernelGGL(k_window_unpack, dim3(g), dim3(256), 0, s, words, width, pitch, (int)il,
                       modrows, brow0, x, w, row0, nrows, bytes);
    return hipGetLastError();
}

hipError_t launch_window_density(const uint64_t *words, int width, int pitch, bool il, int modrows,
                                 int brow0, int x, int w, int row0, int nrows, int block,
                                 uint32_t *counts, hipStream_t s)
{
    if (nrows <= 0) return hipSuccess;
    const int g = window_grid((long long)nrows * ((w + 63) / 64));
    hipLaunchKernelGGL(k_window_density, dim3(g), dim3(256), 0, s, words, width, pitch, (int)il,
                       modrows, brow0, x, w, row0, nrows, block, counts);
    return hipGetLastError();
}

hipError_t launch_window_pack(uint64_t *words, int width, int nw, int pitch, bool il, int b0,
                              int nrows, int x, int w, const uint8_t *bytes, hipStream_t s)
{
    if (nrows <= 0) return hipSuccess;
    // the words the window's columns touch, from word x / 64 on: up to the row's end and, past
    // the wrap, from word 0 on -- all nw when the two parts meet in one word
    const long long xe = (long long)x + w;
    long long ntouch;
    if (xe <= width)
        ntouch = (xe - 1) / 64 - x / 64 + 1;
    else
        ntouch = (nw - x / 64) + ((xe - width - 1) / 64 + 1);
    if (ntouch > nw) ntouch = nw;
    const int g = window_grid((long long)nrows * ntouch);
    hipLaunchKernelGGL(k_window_pack, dim3(g), dim3(256), 0, s, words, width, nw, pitch, (int)il, b0,
                       nrows, x, w, x / 64, (int)ntouch, bytes);
    return hipGetLastError();
}

}  // namespace golk
