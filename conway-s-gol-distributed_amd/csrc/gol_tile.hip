// gol_tile.hip -- the k_step_tile instantiation table (K1t, gol_tile.h) and its launcher.
// The tools build and two A/B builds (make variant VDEFS=-DGOL_TILE_PAIR=1, -DGOL_TILE_RAW=n) also
// compile gol_tile_lab.h, the experiments' kernels and hooks, which documents those macros.
// Their launchers are the tools region at the end of this file; their tables (persist_fn,
// ring_fn, stream_fn) stand where they always stood, between the product tables, because the
// order of the tables is the order of the kernels in the unit's code object, which the profiles
// and the assembly comparison of DESIGN.md rely on.
#if GOL_TOOLS || GOL_TILE_PAIR || GOL_TILE_RAW
#define GOL_TILE_LAB 1
#endif
#include "gol_tile.h"
#ifndef GOL_TILE_PAIR   // (no lab header in this build: the launcher below still asks)
#define GOL_TILE_PAIR 0
#endif

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <iterator>
#include <map>
#include <mutex>
#include <tuple>

namespace golk {

// tile_seg = SEG + 100 * ORD + 1000 * (W - 1) (gol_tile.h): ORD 1 = the turn's interior rows
// before the edge rows, W = words per lane
template <int ORD, int W>
static void *tile_fn(int seg)
{
    switch (seg) {
    case 2: return reinterpret_cast<void *>(&k_step_tile<2, ORD, W>);
    case 3: return reinterpret_cast<void *>(&k_step_tile<3, ORD, W>);
    case 4: return reinterpret_cast<void *>(&k_step_tile<4, ORD, W>);
    case 6: return reinterpret_cast<void *>(&k_step_tile<6, ORD, W>);
    case 8: return reinterpret_cast<void *>(&k_step_tile<8, ORD, W>);
    // (two words per lane stop at SEG 8: deeper segments spill at the 128-VGPR cap)
    case 12: return W == 1 ? reinterpret_cast<void *>(&k_step_tile<12, ORD, 1>) : nullptr;
    case 16: return W == 1 ? reinterpret_cast<void *>(&k_step_tile<16, ORD, 1>) : nullptr;
    case 24: return W == 1 ? reinterpret_cast<void *>(&k_step_tile<24, ORD, 1>) : nullptr;
    case 32: return W == 1 ? reinterpret_cast<void *>(&k_step_tile<32, ORD, 1>) : nullptr;
    case 40: return W == 1 ? reinterpret_cast<void *>(&k_step_tile<40, ORD, 1>) : nullptr;
    case 48: return W == 1 && ORD == 0 ? reinterpret_cast<void *>(&k_step_tile<48, 0, 1>) : nullptr;
    // (ORD 2 at SEG < 3 is ORD 1: no interior row; ORD 4: SEG 3..40, one word per lane)
    default: return nullptr;
    }
}

// k_tile_persist instantiations (K1p, small boards): one word per lane; in order (ORD 0),
// interior rows first with the workgroup barrier (ORD 1, 5) or with neighbour flags (ORD 4).
// Tools build only (round 5): K1p never won its own autotune (5120^2: 0.588 against 0.563 us
// per turn for plain launches, profiles/r04_c2_autotune_persist.log), and its uncached
// block hand-off is the scheme under which K1q computed wrong boards with the cause unknown.
static void *persist_fn(int code)
{
    static_assert(std::size(kTilePersistCodes) == 22, "persist_fn covers kTilePersistCodes");
#if !GOL_TOOLS
    (void)code;
    return nullptr;
#else
    switch (code) {
    case 102: return reinterpret_cast<void *>(&k_tile_persist<2, 1, 1>);
    case 103: return reinterpret_cast<void *>(&k_tile_persist<3, 1, 1>);
    case 104: return reinterpret_cast<void *>(&k_tile_persist<4, 1, 1>);
    case 106: return reinterpret_cast<void *>(&k_tile_persist<6, 1, 1>);
    case 108: return reinterpret_cast<void *>(&k_tile_persist<8, 1, 1>);
    case 112: return reinterpret_cast<void *>(&k_tile_persist<12, 1, 1>);
    case 116: return reinterpret_cast<void *>(&k_tile_persist<16, 1, 1>);
    case 403: return reinterpret_cast<void *>(&k_tile_persist<3, 4, 1>);
    case 404: return reinterpret_cast<void *>(&k_tile_persist<4, 4, 1>);
    case 406: return reinterpret_cast<void *>(&k_tile_persist<6, 4, 1>);
    case 408: return reinterpret_cast<void *>(&k_tile_persist<8, 4, 1>);
    case 412: return reinterpret_cast<void *>(&k_tile_persist<12, 4, 1>);
    case 416: return reinterpret_cast<void *>(&k_tile_persist<16, 4, 1>);
    case 2: return reinterpret_cast<void *>(&k_tile_persist<2, 0, 1>);
    case 3: return reinterpret_cast<void *>(&k_tile_persist<3, 0, 1>);
    case 4: return reinterpret_cast<void *>(&k_tile_persist<4, 0, 1>);
    case 6: return reinterpret_cast<void *>(&k_tile_persist<6, 0, 1>);
    case 8: return reinterpret_cast<void *>(&k_tile_persist<8, 0, 1>);
    case 503: return reinterpret_cast<void *>(&k_tile_persist<3, 5, 1>);
    case 504: return reinterpret_cast<void *>(&k_tile_persist<4, 5, 1>);
    case 506: return reinterpret_cast<void *>(&k_tile_persist<6, 5, 1>);
    case 508: return reinterpret_cast<void *>(&k_tile_persist<8, 5, 1>);
    default: return nullptr;
    }
#endif
}

// k_tile_ring instantiations (K1r, small torus boards): the C2 / C3 shape families
static void *ring_fn(int code)
{
    static_assert(std::size(kTileRingCodes) == 10, "ring_fn covers kTileRingCodes");
#if GOL_TOOLS
    switch (code) {
    case 103: return reinterpret_cast<void *>(&k_tile_ring<3, 1>);
    case 203: return reinterpret_cast<void *>(&k_tile_ring<3, 2>);
    case 503: return reinterpret_cast<void *>(&k_tile_ring<3, 5>);
    case 504: return reinterpret_cast<void *>(&k_tile_ring<4, 5>);
    case 506: return reinterpret_cast<void *>(&k_tile_ring<6, 5>);
    case 508: return reinterpret_cast<void *>(&k_tile_ring<8, 5>);
    case 512: return reinterpret_cast<void *>(&k_tile_ring<12, 5>);
    case 516: return reinterpret_cast<void *>(&k_tile_ring<16, 5>);
    case 112: return reinterpret_cast<void *>(&k_tile_ring<12, 1>);
    case 116: return reinterpret_cast<void *>(&k_tile_ring<16, 1>);
    default: return nullptr;
    }
#else
    (void)code;
    return nullptr;
#endif
}

// ORD 6 (the barrier after the interior rows, edge sums read back): the 6-8 waves per SIMD
// segments only
static void *tile_fn6(int seg)
{
    switch (seg) {
    case 12: return reinterpret_cast<void *>(&k_step_tile<12, 6, 1>);
    case 16: return reinterpret_cast<void *>(&k_step_tile<16, 6, 1>);
    case 24: return reinterpret_cast<void *>(&k_step_tile<24, 6, 1>);
    default: return nullptr;
    }
}

// k_tile_stream instantiations (K1q, large boards): the 65536^2 and 16384^2 shape families.
// Tools build only: K1q measured 28-42 % slower than plain launches, and a board with more
// workgroups than items per block still computed a wrong board now and then
static void *stream_fn(int code)
{
    static_assert(std::size(kTileStreamCodes) == 4, "stream_fn covers kTileStreamCodes");
#if GOL_TOOLS
    switch (code) {
    case 106: return reinterpret_cast<void *>(&k_tile_stream<6, 1, 1>);
    case 506: return reinterpret_cast<void *>(&k_tile_stream<6, 5, 1>);
    case 512: return reinterpret_cast<void *>(&k_tile_stream<12, 5, 1>);
    case 524: return reinterpret_cast<void *>(&k_tile_stream<24, 5, 1>);
    default: return nullptr;
    }
#else
    (void)code;
    return nullptr;
#endif
}

// (A/B builds: make variant VDEFS=-DGOL_TILE_W2_SEG12=1 adds two words per lane at SEG 12,
// ORD 1 and 5 -- codes 1112 and 1512 -- the round-5 verdict's candidate for fewer lane
// shifts per word at the VGPRs of SEG 24 with one word)
#ifndef GOL_TILE_W2_SEG12
#define GOL_TILE_W2_SEG12 0
#endif

void *tile_kernel(int code)
{
    const int seg = code % 100, ord = (code / 100) % 10, w = tile_seg_words(code);
#if GOL_TILE_W2_SEG12
    if (code == 1112) return reinterpret_cast<void *>(&k_step_tile<12, 1, 2>);
    if (code == 1512) return reinterpret_cast<void *>(&k_step_tile<12, 5, 2>);
#endif
#if GOL_TILE_PAIR   // ORD 3: two tiles per workgroup, software-pipelined (tile_pass_pair)
    if (ord == 3 && w == 1) {
        switch (seg) {
        case 2: return reinterpret_cast<void *>(&k_step_tile_pair<2>);
        case 3: return reinterpret_cast<void *>(&k_step_tile_pair<3>);
        case 4: return reinterpret_cast<void *>(&k_step_tile_pair<4>);
        case 6: return reinterpret_cast<void *>(&k_step_tile_pair<6>);
        case 8: return reinterpret_cast<void *>(&k_step_tile_pair<8>);
        default: return nullptr;
        }
    }
#elif GOL_TOOLS   // ORD 3: no barrier between turns (wrong boards): what the turn's sync costs
    if (ord == 3 && w == 1) return tile_fn<3, 1>(seg);
#endif
    if (code < 0 || w > 2) return nullptr;
    if (ord == 4) return w == 1 && seg >= 3 && seg <= 40 ? tile_fn<4, 1>(seg) : nullptr;
    if (ord == 5) return w == 1 && seg >= 3 && seg <= 40 ? tile_fn<5, 1>(seg) : nullptr;
    if (ord == 6) return w == 1 ? tile_fn6(seg) : nullptr;
    // ORD 7 (wave 0 holds the halo segments and skips the rows the trapezoid has left): the
    // 65536^2 segment only; tools build (it measured 0.5 % slower than ORD 5)
#if GOL_TOOLS
    // ORD 8 (ORD 5's turn in inline asm with a hand-made VGPR assignment): SEG 6, 12, 24
    if (ord == 8 && w == 1) {
        if (seg == 24) return reinterpret_cast<void *>(&k_step_tile<24, 8, 1>);
        if (seg == 12) return reinterpret_cast<void *>(&k_step_tile<12, 8, 1>);
        if (seg == 6) return reinterpret_cast<void *>(&k_step_tile<6, 8, 1>);
        return nullptr;
    }
    // ORD 9 (ORD 8 with the lane shifts' neighbour words by ds_bpermute instead of DPP)
    if (ord == 9 && w == 1) {
        if (seg == 24) return reinterpret_cast<void *>(&k_step_tile<24, 9, 1>);
        if (seg == 12) return reinterpret_cast<void *>(&k_step_tile<12, 9, 1>);
        if (seg == 6) return reinterpret_cast<void *>(&k_step_tile<6, 9, 1>);
        return nullptr;
    }
    if (ord == 7) return w == 1 && seg == 24 ? reinterpret_cast<void *>(&k_step_tile<24, 7, 1>) : nullptr;
#endif
    if (ord > 2) return nullptr;
    if (w == 2) return ord == 2 ? tile_fn<2, 2>(seg) : ord ? tile_fn<1, 2>(seg) : tile_fn<0, 2>(seg);
    return ord == 2 ? tile_fn<2, 1>(seg) : ord ? tile_fn<1, 1>(seg) : tile_fn<0, 1>(seg);
}

// k_step_tile_cnt instantiations (the per-turn alive counts fused): kTileCountCodes
void *tile_cnt_kernel(int code)
{
    static_assert(std::size(kTileCountCodes) == 24, "tile_cnt_kernel covers kTileCountCodes");
    switch (code) {
    case 4: return reinterpret_cast<void *>(&k_step_tile_cnt<4, 0, 1>);
    case 8: return reinterpret_cast<void *>(&k_step_tile_cnt<8, 0, 1>);
    case 16: return reinterpret_cast<void *>(&k_step_tile_cnt<16, 0, 1>);
    case 103: return reinterpret_cast<void *>(&k_step_tile_cnt<3, 1, 1>);
    case 104: return reinterpret_cast<void *>(&k_step_tile_cnt<4, 1, 1>);
    case 106: return reinterpret_cast<void *>(&k_step_tile_cnt<6, 1, 1>);
    case 108: return reinterpret_cast<void *>(&k_step_tile_cnt<8, 1, 1>);
    case 112: return reinterpret_cast<void *>(&k_step_tile_cnt<12, 1, 1>);
    case 116: return reinterpret_cast<void *>(&k_step_tile_cnt<16, 1, 1>);
    case 124: return reinterpret_cast<void *>(&k_step_tile_cnt<24, 1, 1>);
    case 203: return reinterpret_cast<void *>(&k_step_tile_cnt<3, 2, 1>);
    case 204: return reinterpret_cast<void *>(&k_step_tile_cnt<4, 2, 1>);
    case 206: return reinterpret_cast<void *>(&k_step_tile_cnt<6, 2, 1>);
    case 208: return reinterpret_cast<void *>(&k_step_tile_cnt<8, 2, 1>);
    case 406: return reinterpret_cast<void *>(&k_step_tile_cnt<6, 4, 1>);
    case 416: return reinterpret_cast<void *>(&k_step_tile_cnt<16, 4, 1>);
    case 503: return reinterpret_cast<void *>(&k_step_tile_cnt<3, 5, 1>);
    case 504: return reinterpret_cast<void *>(&k_step_tile_cnt<4, 5, 1>);
    case 506: return reinterpret_cast<void *>(&k_step_tile_cnt<6, 5, 1>);
    case 508: return reinterpret_cast<void *>(&k_step_tile_cnt<8, 5, 1>);
    case 512: return reinterpret_cast<void *>(&k_step_tile_cnt<12, 5, 1>);
    case 516: return reinterpret_cast<void *>(&k_step_tile_cnt<16, 5, 1>);
    case 524: return reinterpret_cast<void *>(&k_step_tile_cnt<24, 5, 1>);
    case 616: return reinterpret_cast<void *>(&k_step_tile_cnt<16, 6, 1>);
    default: return nullptr;
    }
}

bool tile_shape_ok(int nw, int turns, int tile_h, int tile_w, int seg, int width)
{
    if (turns < 2 || turns > 64 || tile_h < 1 || tile_w < 1 || tile_w + 2 > 64 || !tile_kernel(seg))
        return false;
    // across the row seam: a code with a seam instantiation, and a tile no wider than the row
    // (its lane columns then stay within [-1, nw]: two real words per stitched column)
    if (width > 0 && width % 64 != 0 &&
        (!tile_code_seam(seg) || !tile_seam_kernel(seg) || tile_w > nw || width < 256))
        return false;
    if (!GOL_TOOLS && !tile_code_shipped(seg) && !(GOL_TILE_W2_SEG12 && seg % 1000 == 112) &&
        !(GOL_TILE_W2_SEG12 && seg % 1000 == 512) && !(GOL_TILE_PAIR && seg / 100 == 3))
        return false;   // (untested instantiations)
    if (nw % tile_seg_words(seg)) return false;          // (whole word pairs per lane)
    const int C = tile_w + 2, G = 64 / C;
    const int ord = seg / 100 % 10;
    seg %= 100;
    const int nseg = (tile_h + 2 * turns + seg - 1) / seg;
    // ORD 7: two lane groups per wave (wave 0 = the top and the bottom segment), >= 3 segments
    if (ord == 7 && (G != 2 || nseg < 3)) return false;
    const int waves = (nseg + G - 1) / G;
    return waves <= kTileMaxWaves;
}

int tile_waves(int turns, int tile_h, int tile_w, int seg)
{
    const int C = tile_w + 2, G = 64 / C;
    seg %= 100;
    const int nseg = (tile_h + 2 * turns + seg - 1) / seg;
    return (nseg + G - 1) / G;
}

bool tile_duo_env()
{
    const char *e = getenv("GOL_TILE_DUO");
    return !e || atoi(e) != 0;
}

int tile_blocks_per_cu(int turns, int tile_h, int tile_w, int seg, int width)
{
    const bool seam = width > 0 && width % 64 != 0;      // (the seam kernel's own registers)
    // (the pair form's, where it launches)
    const bool duo = !seam && tile_duo_kernel(seg) && tile_duo_env();
    void *fn = seam ? tile_seam_kernel(seg) : duo ? tile_duo_kernel(seg) : tile_kernel(seg);
    if (!fn) return 0;
    const int waves = tile_waves(turns, tile_h, tile_w, seg);
    if (waves < 1 || waves > kTileMaxWaves) return 0;
    // (the planner asks for thousands of shapes: cache per (kernel, waves))
    static std::mutex mu;
    static std::map<std::tuple<int, int, int>, int> cache;
    std::lock_guard<std::mutex> lk(mu);
    const int form = seam ? 1 : duo ? 2 : 0;
    auto it = cache.find({seg, waves, form});
    if (it != cache.end()) return it->second;
    int blocks = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(
            &blocks, fn, 64 * waves, tile_lds_bytes_code(64 * waves, seg)) != hipSuccess)
        blocks = 0;
    cache[{seg, waves, form}] = blocks;
    return blocks;
}

TileGrid tile_grid(int nw, int rows, int turns, int tile_h, int tile_w, int seg)
{
    TileGrid g{0, 0, 0, 0, 0};
    if (nw < 1 || rows < 1 || tile_h < 1 || tile_w < 1 || tile_w + 2 > 64) return g;
    const int nl = nw / tile_seg_words(seg);
    const int ntx = (nl + tile_w - 1) / tile_w;
    g.ntx_main = ntx;
    g.nty_main = (rows + tile_h - 1) / tile_h;
    const int ord = seg / 100 % 10, segrows = seg % 100;
    // (ORD 7's wave 0 holds two lane groups by construction, ORD 8 / 9 and the ORD 3 forms
    // are tools-build experiments: they keep the rectangular grid)
    if (turns < 1 || segrows < 1 || ord == 3 || ord >= 7) return g;
    const char *env = getenv("GOL_TILE_REPACK");
    if (env && atoi(env) == 0) return g;
    const int r = nl - (ntx - 1) * tile_w;               // lanes of the last tile column
    if (r <= 0 || r >= tile_w) return g;
    const int G = 64 / (tile_w + 2), Gn = 64 / (r + 2);
    if (Gn <= G) return g;
    // blockDim is launch-uniform: the narrow tiles have the main tiles' waves
    const int waves = tile_waves(turns, tile_h, tile_w, seg);
    if (waves < 1 || waves > kTileMaxWaves) return g;
    const long long hmax = (long long)waves * Gn * segrows - 2 * turns;
    if (hmax < 1) return g;
    const long long n = (rows + hmax - 1) / hmax;
    if (n >= g.nty_main) return g;
    g.ntx_main = ntx - 1;
    g.n_narrow = (int)n;
    g.narrow_w = r;
    // evened out over the n tiles: the last one is no sliver
    g.narrow_h = (int)std::min<long long>((rows + n - 1) / n, rows);
    return g;
}

long long tile_count(int nw, int rows, int tile_h, int tile_w, int seg, int turns)
{
    if (turns > 0) return tile_grid(nw, rows, turns, tile_h, tile_w, seg).tiles();
    const long long nl = nw / tile_seg_words(seg);
    const long long ntx = (nl + tile_w - 1) / tile_w;
    return ntx * ((rows + tile_h - 1) / tile_h);
}

hipError_t launch_tile(const StepArgs &a, int turns, hipStream_t s)
{
    const int rows = a.row_hi - a.row_lo;
    if (!tile_shape_ok(a.nw, turns, a.band, a.tile_w, a.tile_seg, a.width)) return hipErrorInvalidValue;
    // a buffer of 2 GiB or more (or GOL_TILE_BIG=1: StepArgs::tile_big): the big form, on the
    // shapes it runs -- never the plain kernel, whose 32-bit offsets do not reach such a buffer's
    // rows.  Every tile's window wraps at most once and stays below 2 GiB: the launch's tile
    // height by tile_big_ok, the repacked narrow column's by tile_grid_big.
    const bool big = tile_buffer_big(a.modrows, a.pitch, a.tile_big != 0);
    if (big && (a.counts || !tile_big_kernel(a.tile_seg) ||
                !tile_big_ok(a.width, a.modrows, a.pitch, turns, a.band, a.tile_seg)))
        return hipErrorInvalidValue;
    // (ORD 3 with GOL_TILE_PAIR pairs tiles by index: tile_grid leaves its grid rectangular)
    const TileGrid g = big ? tile_grid_big(a.nw, rows, turns, a.band, a.tile_w, a.tile_seg,
                                           tile_big_max_h(a.modrows, a.pitch, turns))
                           : tile_grid(a.nw, rows, turns, a.band, a.tile_w, a.tile_seg);
    const int ntx = g.ntx_main;
    const long long ntiles = g.tiles();
    if (ntiles <= 0 || ntiles > (1 << 24)) return hipErrorInvalidValue;
    TileLaunch L{};
    L.ntiles = (int)ntiles;
    L.n_main = g.ntx_main * g.nty_main;
    L.ntx_main = g.ntx_main;
    L.inv_ntx = g.ntx_main > 1 ? (uint32_t)((1ull << 32) / (unsigned)g.ntx_main) + 1u : 0u;
    L.narrow_w = g.narrow_w;
    L.narrow_h = g.narrow_h;
    L.g[0] = 64 / (a.tile_w + 2);
    L.rcp[0] = tile_rcp16(a.tile_w + 2);
    L.g[1] = g.n_narrow ? 64 / (g.narrow_w + 2) : L.g[0];
    L.rcp[1] = g.n_narrow ? tile_rcp16(g.narrow_w + 2) : L.rcp[0];
    // (ORD 3 with GOL_TILE_PAIR: one workgroup per pair of tiles)
    const long long units = GOL_TILE_PAIR && a.tile_seg / 100 == 3 ? (ntiles + 1) / 2 : ntiles;
    const unsigned blocks = (unsigned)((units + 7) / 8 * 8);
    const int threads = 64 * tile_waves(turns, a.band, a.tile_w, a.tile_seg);
    // a.counts: `turns` consecutive zeroed slots of kShards accumulators, one per turn of the
    // launch -- the counted kernel, and an error for a code without one (never the uncounted
    // kernel with the counts dropped)
    // a width that is no multiple of 64: the seam kernel (which has no counted form)
    const bool seam = a.width % 64 != 0;
    // a plain launch (not big, seam or counted) of a code with a pair form, unless switched off:
    // k_step_tile_duo, on the plain kernel's grid, LDS bytes and arguments
    void *const duo = a.tile_duo ? tile_duo_kernel(a.tile_seg) : nullptr;
    void *fn = big    ? tile_big_kernel(a.tile_seg)
               : seam ? (a.counts ? nullptr : tile_seam_kernel(a.tile_seg))
               : a.counts ? tile_cnt_kernel(a.tile_seg)
               : duo      ? duo
                          : tile_kernel(a.tile_seg);
    if (!fn || (a.counts && !tile_code_counted(a.tile_seg))) return hipErrorInvalidValue;
    StepArgs args = a;
    const uint64_t *in = a.in;
    uint64_t *out = a.out;
    int k = turns, ntx_arg = ntx, nt = (int)ntiles;
    // (k_step_tile_pair keeps the rectangular grid's arguments)
    void *params_pair[] = {&in, &out, &args, &k, &ntx_arg, &nt};
    void *params[] = {&in, &out, &args, &k, &L};
    return hipLaunchKernel(fn, dim3(blocks), dim3(threads),
                           GOL_TILE_PAIR && a.tile_seg / 100 == 3 ? params_pair : params,
                           tile_lds_bytes_code(threads, a.tile_seg) + (a.counts ? tile_count_lds_bytes(threads) : 0),
                           s);
}

}  // namespace golk

// ---- Tools region: the launchers of the kernels of gol_tile_lab.h (K1p k_tile_persist, K1r
// k_tile_ring, K1q k_tile_stream).  A product build keeps these functions, which other units link
// against; its tables above are empty, so every *_ok is false and every launch an error.
namespace golk {

bool tile_persist_ok(int nw, int rows, int turns, int K, int tile_h, int tile_w, int seg, int ncu)
{
    if (!persist_fn(seg) || !tile_shape_ok(nw, K, tile_h, tile_w, seg) || turns < 1 || ncu < 1)
        return false;
    const int nty = (rows + tile_h - 1) / tile_h;
    const int last_h = rows - (nty - 1) * tile_h;
    // a tile's K halo rows come from the adjacent tile rows only
    if (K > tile_h || K > last_h) return false;
    const long long ntiles = tile_count(nw, rows, tile_h, tile_w, seg);
    const long long blocks = (ntiles + 7) / 8 * 8;
    const int waves = tile_waves(K, tile_h, tile_w, seg);
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(
            &per_cu, persist_fn(seg), 64 * waves, tile_lds_bytes(64 * waves, 1)) != hipSuccess)
        return false;
    // every tile resident at once: a tile waits for its neighbours
    return per_cu > 0 && blocks <= (long long)ncu * per_cu;
}

hipError_t launch_tile_persist(const StepArgs &a, int turns, int K, uint64_t *u0, uint64_t *u1,
                               unsigned *flags, unsigned epoch, hipStream_t s)
{
    const int rows = a.row_hi - a.row_lo;
    void *fn = persist_fn(a.tile_seg);
    if (!fn || !tile_shape_ok(a.nw, K, a.band, a.tile_w, a.tile_seg) || K > rows) return hipErrorInvalidValue;
    const int ntx = (a.nw + a.tile_w - 1) / a.tile_w;
    const long long ntiles = (long long)ntx * ((rows + a.band - 1) / a.band);
    if (ntiles <= 0 || ntiles > (1 << 20)) return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((ntiles + 7) / 8 * 8);
    const int threads = 64 * tile_waves(K, a.band, a.tile_w, a.tile_seg);
    StepArgs args = a;
    const uint64_t *in = a.in;
    uint64_t *out = a.out;
    int t = turns, k = K, ntx_arg = ntx, nt = (int)ntiles;
    void *params[] = {&in, &out, &u0, &u1, &args, &t, &k, &ntx_arg, &nt, &flags, &epoch};
    return hipLaunchKernel(fn, dim3(blocks), dim3(threads), params, tile_lds_bytes(threads, 1), s);
}

bool tile_ring_ok(int nw, int rows, int K, int tile_h, int tile_w, int seg, int ncu)
{
    void *fn = ring_fn(seg);
    if (!fn || !tile_shape_ok(nw, K, tile_h, tile_w, seg) || ncu < 1) return false;
    const int nty = (rows + tile_h - 1) / tile_h;
    const int last_h = rows - (nty - 1) * tile_h;
    // a tile's ring comes from its 8 neighbours only: K rows within every tile's interior
    if (K > tile_h || K > last_h) return false;
    const long long ntiles = tile_count(nw, rows, tile_h, tile_w, seg);
    const long long blocks = (ntiles + 7) / 8 * 8;
    const int threads = 64 * tile_waves(K, tile_h, tile_w, seg);
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, threads,
                                                     tile_lds_bytes_code(threads, seg)) != hipSuccess)
        return false;
    return per_cu > 0 && blocks <= (long long)ncu * per_cu;   // every tile resident at once
}

hipError_t launch_tile_ring(const StepArgs &a, int turns, int K, uint64_t *u0, uint64_t *u1,
                            unsigned *flags, unsigned epoch, unsigned *gcount, unsigned gbase,
                            hipStream_t s)
{
    const int rows = a.row_hi - a.row_lo;
    void *fn = ring_fn(a.tile_seg);
    if (!fn || !tile_shape_ok(a.nw, K, a.band, a.tile_w, a.tile_seg) || K > rows || turns < 1)
        return hipErrorInvalidValue;
    const int ntx = (a.nw + a.tile_w - 1) / a.tile_w;
    const long long ntiles = (long long)ntx * ((rows + a.band - 1) / a.band);
    if (ntiles <= 0 || ntiles > (1 << 20)) return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((ntiles + 7) / 8 * 8);
    const int threads = 64 * tile_waves(K, a.band, a.tile_w, a.tile_seg);
    StepArgs args = a;
    const uint64_t *in = a.in;
    uint64_t *out = a.out;
    int t = turns, k = K, ntx_arg = ntx, nt = (int)ntiles;
    int ablate = getenv("GOL_RING_ABLATE") ? atoi(getenv("GOL_RING_ABLATE")) : 0;   // (tools timing)
    void *params[] = {&in, &out, &u0, &u1, &args, &t, &k, &ntx_arg, &nt, &flags, &epoch,
                      &gcount, &gbase, &ablate};
    return hipLaunchKernel(fn, dim3(blocks), dim3(threads), params,
                           tile_lds_bytes_code(threads, a.tile_seg), s);
}

bool tile_stream_ok(int nw, int rows, int K, int tile_h, int tile_w, int seg)
{
    if (!stream_fn(seg) || !tile_shape_ok(nw, K, tile_h, tile_w, seg)) return false;
    const int nty = (rows + tile_h - 1) / tile_h;
    const int last_h = rows - (nty - 1) * tile_h;
    return K <= tile_h && K <= last_h;   // a tile's K halo rows come from adjacent tile rows only
}

hipError_t launch_tile_stream(const StepArgs &a, int turns, int K, uint64_t *u0, uint64_t *u1,
                              unsigned *flags, unsigned epoch, unsigned *counter, unsigned base,
                              int ncu, int max_grid, unsigned *grid_out, hipStream_t s)
{
    const int rows = a.row_hi - a.row_lo;
    void *fn = stream_fn(a.tile_seg);
    if (!fn || !tile_stream_ok(a.nw, rows, K, a.band, a.tile_w, a.tile_seg) || turns < 1 || ncu < 1)
        return hipErrorInvalidValue;
    const int ntx = (a.nw + a.tile_w - 1) / a.tile_w;
    const long long ntiles = (long long)ntx * ((rows + a.band - 1) / a.band);
    const long long nitems = ntiles * ((turns + K - 1) / K);
    if (ntiles <= 0 || nitems > (1ll << 30)) return hipErrorInvalidValue;
    const int threads = 64 * tile_waves(K, a.band, a.tile_w, a.tile_seg);
    const size_t lds = tile_lds_bytes(threads, 1);
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, threads, lds) != hipSuccess)
        per_cu = 0;
    // (at least what k_step_tile gets with the same registers and LDS: a workgroup that does
    // not fit yet just starts later and takes the items left then)
    per_cu = std::max(per_cu, tile_blocks_per_cu(K, a.band, a.tile_w, a.tile_seg));
    if (per_cu < 1) return hipErrorInvalidValue;
    if (getenv("GOL_STREAM_LOG"))
        fprintf(stderr, "k_tile_stream grid: %d CUs x %d workgroups of %d threads (occupancy API %d)\n",
                ncu, per_cu, threads, [&] { int q = 0; (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&q, fn, threads, lds); return q; }());
    long long g = std::min<long long>(nitems, (long long)ncu * per_cu);
    if (max_grid > 0) g = std::min<long long>(g, max_grid);   // (tests: few workgroups)
    const unsigned grid = (unsigned)g;
    StepArgs args = a;
    const uint64_t *in = a.in;
    uint64_t *out = a.out;
    int t = turns, k = K, ntx_arg = ntx, nt = (int)ntiles;
    void *params[] = {&in, &out, &u0, &u1, &args, &t, &k, &ntx_arg, &nt, &flags, &epoch, &counter,
                      &base};
    const hipError_t e = hipLaunchKernel(fn, dim3(grid), dim3(threads), params, lds, s);
    if (e == hipSuccess && grid_out) *grid_out = grid;
    return e;
}

}  // namespace golk
