// Internal launch interface of the gfx950 kernels (gol_kernels.hip).
// Not part of the C ABI; the engine's units (gol_ctx.h lists them) are the only callers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace golk {

constexpr int kShards = 64;            // popcount accumulator shards (one 512-B line)
constexpr int kTileWords = 128;        // fast stencil: words per wavefront tile (64 lanes x 2)

// One turn over rows [row_lo, row_hi) of a buffer of `modrows` rows (row index
// wraps mod modrows: torus engines; strip engines never reach the wrap).
struct StepArgs {
    const uint64_t *in;
    uint64_t *out;
    const uint64_t *blocked;           // non-binary mask (turn 1 only) or nullptr
    unsigned long long *counts;        // kShards accumulators or nullptr
    int width;                         // cells per row
    int nw;                            // words per row
    int pitch;                         // row stride in words
    int modrows;
    int row_lo, row_hi;
    int cnt_lo, cnt_hi;                // rows whose outputs are counted
    int band;                          // rows per wavefront (fast) / per thread (generic)
    int variant;                       // fast-path kernel variant (kVariant*)
    int multi_words;                   // k_step_multi words per lane (1 or 2)
    int multi_variant;                 // temporal-blocking kernel (kMulti*)
    // kMultiWgPg: boundary rows published between neighbouring bands (engine-owned, uncached)
    uint64_t *xrows;                   // 2 rows per stage, kPgStages stages, xlanes words each
    unsigned *xflags;                  // per (tile, stage): epoch of its last publication
    unsigned xlanes;                   // virtual lanes per published row
    unsigned epoch;                    // this launch's epoch (above every earlier launch's)
    // k_step_wg wave priorities (4-wave workgroups): wave w runs at s_setprio
    // (wg_prio >> 2w) & 3; 0 = the built-in grading
    unsigned wg_prio;
    // k_step_tile: 1 = the big form (k_step_tile_big: the buffer resources rebased per tile)
    // whatever the buffer's size -- GOL_TILE_BIG=1; a buffer of 2 GiB or more runs it anyway.
    // (it sits in what was padding before the pointer below: no other member moves)
    int tile_big;
    // engine-owned error word (host-mapped pinned memory, or nullptr): a k_step_wg wait that
    // gives up stores a kDevErr* code here, and the engine reports it as GOL_EHIP at its next
    // synchronising call instead of returning a corrupt board with GOL_OK
    unsigned *err;
    // k_step_tile (kMultiTile): tile width in words (the tile height is `band`) and rows per
    // lane segment
    int tile_w;
    int tile_seg;
    // k_step_tile: 1 = plain launches of a code with a pair form run it (k_step_tile_duo: the
    // interior rows ruled in pairs on shared row-pair sums).  The engine sets it at create unless
    // GOL_TILE_DUO=0; 0 (a StepArgs built elsewhere): the plain kernel.
    int tile_duo;
};

// device error codes (StepArgs::err)
constexpr unsigned kDevErrHandoff = 1u;    // k_step_wg: LDS hand-off wait timed out
constexpr unsigned kDevErrPgFlag = 2u;     // k_step_wg parallelogram: flag wait timed out
constexpr unsigned kDevErrTileFlag = 3u;   // k_tile_persist: a neighbour tile's flag wait timed out

// temporal-blocking kernels (A/B-able via GOL_MULTI_VARIANT; kMultiSkewILW16 is shipped)
enum : int {
    kMultiSerial = 0,       // k_step_multi: stages chained within a step
    kMultiSkew = 1,         // k_step_skew: stages one step apart, LDS-DMA prefetch of 8 rows,
                            //   4 waves/SIMD (V = 1, K < 8; 3 at K = 8), 7-op rule
    kMultiSkewPD5 = 2,      // k_step_skew, 5 rows in flight, no wave floor (V = 1, K = 6/8 only)
    kMultiSkewW1 = 3,       // k_step_skew, no wave floor                   (V = 1, K = 6/8 only)
    kMultiSkewRule8 = 4,    // k_step_skew with the 8-op rule               (V = 1, K = 6/8 only)
    kMultiSkewD1 = 5,       // k_step_skew, 1 dword (32 cells) per lane     (V = 1, K = 4/6/8 only)
    kMultiSkewIL = 6,       // k_step_skew on the interleaved board layout (V = 1)
    kMultiSkewILW16 = 7,    // kMultiSkewIL, one 16-B row DMA from half the lanes (V = 1; default)
    kMultiWg = 8,           // k_step_wg: one band's stages split over the 4 waves of a workgroup
                            //   (interleaved layout, V = 1, K = 4..16; K = 2, 3: kMultiSkewILW16)
    kMultiWgHx = 9,         // k_step_wg on helix tiles: the row bands end to end, cut every 62
                            //   lanes (no per-row remainder tile; needs nw even)
    kMultiWgNoBar = 10,     // k_step_wg without hand-off sync: timing ablation (wrong results)
    kMultiWgDiag = 11,      // k_step_wg with per-wave wait timing (tools/wg_diag.py)
    kMultiWgPg = 12,        // kMultiWgHx with parallelogram bands: a band's stages take their
                            //   last 2 input rows from the band below (published through
                            //   memory) instead of recomputing a 2K-row halo (band >= kPgMinBand)
    kMultiWgHxS = 13,       // kMultiWgHx with each wave's stages in order within a step (fill
                            //   and drain of 2 instead of 3 steps per stage)
    kMultiWgPgS = 14,       // kMultiWgPg, stages in order (band rule: golk::pg_ok(.., true))
    kMultiTile = 15,        // k_step_tile: a 2-D tile per workgroup, resident in registers for
                            //   all K turns (small boards: gol_tile.h)
    kMultiUserEnd = 16,     // variants 0 .. kMultiUserEnd - 1 may be requested (GOL_MULTI_VARIANT);
                            //   the ids from here on are engine-internal launch kinds
    kMultiTilePersist = 16, // K1p k_tile_persist: k_step_tile's tiles resident across blocks of
                            //   K turns (engine-internal; tools build only)
    kMultiTileStream = 17,  // K1q k_tile_stream: blocks of K turns over (block, tile) items taken
                            //   in order by resident workgroups (engine-internal; tools build only)
    kMultiResident = 18,    // K1r2 k_step_resident: a torus board narrower than 256 cells held
                            //   whole in the registers of one workgroup for the launch's turns
                            //   (engine-internal: GOL_FLAG_RESIDENT asks for it; gol_resident.h)
    kMultiInternalEnd = 19, // one past the engine-internal launch kinds (size of any table by kind)
    kMultiAblate = 100,     // 100 + ABL mask: k_step_skew<8> timing ablations (K = 8 only)
};
// k_step_resident's depth: 2 .. kResidentMaxTurns turns per launch (the count ring's kRingAhead:
// the slots of one counted launch are what one zeroing batch clears)
constexpr int kResidentMaxTurns = 256;
constexpr bool is_resident_variant(int v) { return v == kMultiResident; }
constexpr bool resident_turns_ok(int turns) { return turns >= 2 && turns <= kResidentMaxTurns; }

static_assert(kMultiTile < kMultiUserEnd && kMultiWgPgS < kMultiUserEnd,
              "every requestable variant lies below the engine-internal launch kinds");
static_assert(kMultiTilePersist >= kMultiUserEnd && kMultiTileStream < kMultiInternalEnd &&
              kMultiResident >= kMultiUserEnd && kMultiResident < kMultiInternalEnd &&
              kMultiInternalEnd < kMultiAblate, "engine-internal kinds between the two ranges");

#ifndef GOL_TOOLS
#define GOL_TOOLS 0   // 1: the tools build (libgolamd_tools.so, see the Makefile)
#endif

// the kernels the product library ships (gol_create_ex rejects the others unless GOL_TOOLS):
// k_step_skew on the interleaved layout with 16-B row DMA, the k_step_wg families and the
// LDS tile kernel.  The superseded skew variants (kMultiSerial .. kMultiSkewIL), the timing
// ablations and the wait diagnostics exist in the tools build only.
constexpr bool multi_variant_shipped(int v)
{
    return v == kMultiSkewILW16 || v == kMultiWg || v == kMultiWgHx || v == kMultiWgPg ||
           v == kMultiWgHxS || v == kMultiWgPgS || v == kMultiTile;
}

// the k_step_wg variants (one band pipeline per workgroup)
constexpr bool is_wg_variant(int v)
{
    return v == kMultiWg || v == kMultiWgHx || v == kMultiWgPg || v == kMultiWgNoBar ||
           v == kMultiWgDiag || v == kMultiWgHxS || v == kMultiWgPgS;
}

// fast-path stencil variants (A/B-able in one process; kVariantDefault is shipped)
enum : int {
    kVariantWindow = 0,     // k_step_fast: 3-row window, 1 row in flight
    kVariantRing2 = 1,      // k_step_ring<D=2>
    kVariantRing3 = 2,      // k_step_ring<D=3>
    kVariantRing3NT = 3,    // k_step_ring<D=3>, non-temporal stores
    kVariantRing5 = 4,      // k_step_ring<D=5>
    kVariantRing7 = 5,      // k_step_ring<D=7>
    kVariantRing5NT = 6,    // k_step_ring<D=5>, non-temporal stores
    kVariantCount = 7,
};
extern const int kVariantDefault;

bool fast_path_ok(int width);

// K turns per launch (temporal blocking): outputs rows [row_lo, row_hi) after `turns`
// turns, reading rows [row_lo - turns, row_hi + turns) (mod modrows).  No blocked mask,
// no counts.  turns in 2 .. multi_max_turns(variant).
constexpr int kMaxTurnsPerLaunch = 32;
// k_step_tile alone goes deeper: its halo word (64 cells) and K halo rows stay exact up to 64
// turns (the planner's per-depth tables stop at kMaxTurnsPerLaunch; deeper K1t launches are
// pinned or requested, never searched)
constexpr int kMaxTileTurns = 64;
// 32 for the helix k_step_wg variants, 16 for band-tiled k_step_wg, 8..12 for k_step_skew
int multi_max_turns(int variant);
// k_step_wg on helix tiles: wavefronts per workgroup at depth `turns` -- 4 up to K = 16, then
// one more per 4 stages (K = 17..32: 5..8 waves of at most 4 stages, <= 72 VGPRs each)
constexpr int wg_waves(int turns) { return turns <= 16 ? 4 : (turns + 3) / 4; }
constexpr int kWgDeepMax = 32;
// band height of the boundary launches of an overlapped step (rows next to the halos)
constexpr int kOverlapBand = 16;
// kMultiWgPg: stages per tile in the flag array, smallest band; it runs at depths K = 4, 8,
// 12, 16 (every wave the same stage count) with band = 3K/4 - 5 (mod kWgU) (its steady loop
// then ends on a whole unrolled iteration); other launches run as kMultiWgHx
constexpr int kPgStages = 16;
constexpr int kPgMinBand = 32;
// k_step_wg's steady-loop unroll (its LDS ring slots are immediates) and wave 0's input rows
// in flight (LDS-DMA ring of kWgDmaRows + 1 slots; kWgU a multiple of 3, of that and of 6).
// 11 rows in flight (unroll 12) measured no faster than 5 at 65536^2, K = 4..16 (the launch
// is not bound by the head's DMA latency) and cost PG 8-11 VGPRs: 5 / 6 stay.
constexpr int kWgDmaRows = 5;
constexpr int kWgU = 6;
// (ser: kMultiWgPgS, prologue 2G - 2 steps instead of 3G - 3, G = turns / 4)
constexpr bool pg_ok(int turns, int band, bool ser = false)
{
    return turns % 4 == 0 && turns <= kPgStages && band >= kPgMinBand &&
           (band + 2 - (ser ? 2 : 3) * (turns / 4 - 1)) % kWgU == 0;
}
// the nearest band >= `band` kMultiWgPg / kMultiWgPgS runs at depth `turns` (0: none)
constexpr int pg_band(int turns, int band, bool ser = false)
{
    for (int b = band < kPgMinBand ? kPgMinBand : band; b < band + kWgU + kPgMinBand; ++b)
        if (pg_ok(turns, b, ser)) return b;
    return 0;
}
constexpr bool is_pg_variant(int v) { return v == kMultiWgPg || v == kMultiWgPgS; }
constexpr bool is_helix_variant(int v)
{
    return v == kMultiWgHx || v == kMultiWgPg || v == kMultiWgHxS || v == kMultiWgPgS;
}
// (k_step_skew / k_step_wg: fast-path widths; kMultiTile: any width >= 256, and with a tile
// code given, one that runs at that width)
bool multi_ok(int width, int turns, int variant, int tile_code = 0);
// waves sharing one band pipeline at depth `turns` (k_step_wg: wg_waves, else 1)
int multi_waves_per_band(int variant, int turns);
// band pipelines per thread block (k_step_skew: 4 single-wave pipelines; k_step_wg: 1)
int multi_pipes_per_block(int variant);
bool multi_fits(int nw, int pitch, int rows);   // buffer < 2 GiB (k_step_skew buffer ranges)
// the temporal-blocking kernel for (words per lane, variant) runs on the interleaved layout
bool multi_is_il(int words_per_lane, int variant);
// standard <-> interleaved rows (row pitches in words; in and out may not alias)
hipError_t launch_il_convert(const uint64_t *in, int in_pitch, uint64_t *out, int out_pitch,
                             int nrows, int nw, bool to_il, hipStream_t s);
// dwords per lane of the temporal-blocking kernel (tiles advance by 62 x that many dwords)
int multi_lane_dwords(int words_per_lane, int variant);
// wavefront tiles per row band of the temporal-blocking kernel
long long multi_tiles(int width, int lane_dwords);
// band pipelines of one launch over `rows` rows in bands of `band` (workgroups for the
// k_step_wg variants, wavefronts for k_step_skew): tiles x bands, or the helix tile count
long long multi_pipes(int width, int rows, int band, int lane_dwords, int variant);
int auto_band_multi(int width, int rows, int lane_dwords);
// resident 256-thread blocks per CU of the temporal-blocking kernel (0 on error)
int multi_blocks_per_cu(int turns, int words_per_lane, int variant);
// band height minimising (residency rounds x per-wavefront work) for the multi kernel
int pick_band_multi(int width, int rows, int lane_dwords, int turns, int capacity_waves,
                    int variant);
hipError_t launch_step_multi(const StepArgs &a, int turns, hipStream_t s);
// k_step_resident (gol_resident.hip): `turns` turns of the whole torus board a.in -> a.out in one
// workgroup (a.counts: the counted form); hipErrorInvalidValue for a board, row range or depth
// it does not run (gol_resident.h, resident_plan)
hipError_t launch_resident(const StepArgs &a, int turns, hipStream_t s);
// k_step_resident_batch (gol_resident.hip): `turns` turns (1 .. kResidentMaxTurns: one turn is
// allowed here, the 2 of resident_turns_ok is the engine planner's rule) of `boards` torus boards
// of width x height cells, board b at words + b x height x nw, one workgroup each, IN PLACE.
// counts (nullable: the counted form): a ring of kResidentMaxTurns x boards uint32, the count
// after turn t of board b at [(t % kResidentMaxTurns) x boards + b]; turn0 = the batch's turn
// before the launch.  hipErrorInvalidValue for a shape resident_plan refuses, turns outside
// 1 .. kResidentMaxTurns, boards < 1 and boards x height > INT32_MAX.
hipError_t launch_resident_batch(uint64_t *words, uint32_t *counts, int width, int height,
                                 int boards, long long turn0, int turns, hipStream_t s);
// k_batch_alive: the alive cells of `boards` consecutive boards of board_words words each, one
// wavefront per board, one uint32 per board
hipError_t launch_batch_alive(const uint64_t *words, int board_words, int boards, uint32_t *out,
                              hipStream_t s);
// resident workgroups per CU of that shape's k_step_resident_batch (occupancy API: VGPRs, LDS;
// 0 on error)
int resident_batch_blocks_per_cu(int width, int height, bool cnt);
// k_settle_resident_batch (gol_settle.hip, gol_settle.h): launch_resident_batch's boards and
// checks (no counted form), `turns` 1 .. kSettleMaxDepth, with every board under the watch
// states[b] and its snapshot at snaps + b x height x nw; turn0 = the batch's turn before the
// launch, not reduced.
struct SettleState;
hipError_t launch_settle_batch(uint64_t *words, uint64_t *snaps, SettleState *states, int width,
                               int height, int boards, long long turn0, int turns, hipStream_t s);
// k_settle_init: the watch of boards first .. first + n - 1 begins at `turn` (unknown period,
// snapshot 0 held: the caller copies the boards' words to their snapshots)
hipError_t launch_settle_init(SettleState *states, int first, int n, long long turn, hipStream_t s);
// k_step_tile (gol_tile.hip): a launch of `turns` turns on tiles of band x tile_w words with
// tile_seg rows per lane; shape check, workgroup waves, tile count
constexpr int kTileMaxWavesHost = 16;  // k_step_tile: waves per workgroup (gol_tile.h)
// The k_step_tile segment codes (SEG + 100 * ORD + 1000 * (W - 1), gol_tile.h) the product
// library runs: every code the engine's shape searches can pick (tile_candidates, tile_search)
// and nothing else.  Each one is pinned by its own oracle parity test
// (tests/test_gpu_engine.py::test_tile_code_pinned, read through gol_tile_codes), and
// tile_shape_ok rejects the others outside the tools build.
constexpr int kTileCodes[] = {
    2,    3,    4,    6,    8,    12,   16,   24,   32,   40,   48,             // ORD 0, W 1
    102,  103,  104,  106,  108,  112,  116,  124,  132,  140,                  // ORD 1
    203,  204,  206,  208,  212,  216,  224,  232,  240,                        // ORD 2
    403,  404,  406,  408,  412,  416,  424,  432,  440,                        // ORD 4
    503,  504,  506,  508,  512,  516,  524,  532,  540,                        // ORD 5
    612,  616,  624,                                                            // ORD 6
    1002, 1003, 1004, 1006, 1008,                                               // W 2
    1102, 1103, 1104, 1106, 1108,
    1204, 1206, 1208,
};
// the codes k_tile_persist (K1p) is instantiated for in the tools build (gol_tile.hip
// persist_fn; each pinned by tests/test_gpu_engine.py::test_tile_persist_pinned through
// gol_tile_persist_codes, which reports none in the product library: K1p never won its
// autotune and its uncached hand-off shares K1q's unexplained wrong-board runs)
constexpr int kTilePersistCodes[] = {102, 103, 104, 106, 108, 112, 116,
                                     403, 404, 406, 408, 412, 416,
                                     2, 3, 4, 6, 8,
                                     503, 504, 506, 508};
// the codes k_tile_stream (K1q) is instantiated for (gol_tile.hip stream_fn; each pinned by
// tests/test_gpu_engine.py::test_tile_stream_pinned through gol_tile_stream_codes)
constexpr int kTileStreamCodes[] = {106, 506, 512, 524};
// the codes k_tile_ring (K1r) is instantiated for in the tools build (gol_tile.hip ring_fn)
constexpr int kTileRingCodes[] = {103, 203, 503, 504, 506, 508, 512, 516, 112, 116};
// (membership in one of the code sets here, and: every code of a set ships, one word per lane)
template <int N>
constexpr bool tile_code_in(const int (&set)[N], int code)
{
    for (int c : set)
        if (c == code) return true;
    return false;
}
constexpr bool tile_code_shipped(int code) { return tile_code_in(kTileCodes, code); }
template <int N>
constexpr bool tile_codes_shipped_w1(const int (&set)[N])
{
    for (int c : set)
        if (!tile_code_shipped(c) || c >= 1000) return false;
    return true;
}
// the codes k_step_tile_cnt is instantiated for (gol_tile.hip tile_cnt_kernel): K1t with the
// per-turn alive counts fused, what a GOL_FLAG_COUNT_EVERY_TURN engine's multi-turn launches
// run.  One word per lane; the pinned shapes' codes, both loop forms (turn pairs up to SEG 12,
// one body above) and every turn order the searches pick, at the segments they pick most.  Each
// one is pinned by tests/test_gpu_tile_counts.py through gol_tile_count_codes.
constexpr int kTileCountCodes[] = {
    4,   8,   16,                                                                // ORD 0
    103, 104, 106, 108, 112, 116, 124,                                           // ORD 1
    203, 204, 206, 208,                                                          // ORD 2
    406, 416,                                                                    // ORD 4
    503, 504, 506, 508, 512, 516, 524,                                           // ORD 5
    616,                                                                         // ORD 6
};
constexpr bool tile_code_counted(int code) { return tile_code_in(kTileCountCodes, code); }
static_assert(tile_codes_shipped_w1(kTileCountCodes), "kTileCountCodes: a subset of kTileCodes, W = 1");
// the codes k_step_tile_seam is instantiated for (gol_tile_seam.hip tile_seam_kernel): K1t on a
// board whose width is no multiple of 64, where the torus seam in x falls inside the row's last
// word (tile_pass SEAM, seam_stitch below).  One word per lane, plain launches, no counted form.
// Every code the shape search picks on such a board (gol_tune.cpp) is one of these: the short
// segments of the small boards (SEG 2 in both turn orders: what boards of a few thousand words
// run fastest on), both loop forms (turn pairs up to SEG 12, one body above) and the 80-VGPR
// ORD 5 family of the large ones.  Each one is pinned by
// tests/test_gpu_seam.py through gol_tile_seam_codes.
constexpr int kTileSeamCodes[] = {
    2,   16,                                                                     // ORD 0
    102, 104, 106, 108, 112, 116,                                                // ORD 1
    516, 524,                                                                    // ORD 5
};
constexpr bool tile_code_seam(int code) { return tile_code_in(kTileSeamCodes, code); }
static_assert(tile_codes_shipped_w1(kTileSeamCodes), "kTileSeamCodes: a subset of kTileCodes, W = 1");
// the codes k_step_tile_big is instantiated for (gol_tile_big.hip tile_big_kernel): K1t on a
// buffer of 2 GiB or more, whose rows a 32-bit byte offset from the buffer's start no longer
// reaches (tile_pass BIG, tile_window below).  One word per lane, plain launches, whole-word
// rows, no counted form.  The 65536^2 and 16384^2 pins (516, 112), the 6-waves-per-SIMD
// variant (524), and what the big-board search (gol_tune.cpp) draws from: one in-order code,
// both loop forms of ORD 1 and ORD 5, one ORD 6.  Each one is pinned by tests/test_gpu_big.py
// through gol_tile_big_codes.
constexpr int kTileBigCodes[] = {
    16,                                                                          // ORD 0
    108, 112, 116,                                                               // ORD 1
    512, 516, 524,                                                               // ORD 5
    616,                                                                         // ORD 6
};
constexpr bool tile_code_big(int code) { return tile_code_in(kTileBigCodes, code); }
static_assert(tile_codes_shipped_w1(kTileBigCodes), "kTileBigCodes: a subset of kTileCodes, W = 1");

// ---- the big form's window.  A tile at buffer row y0, tile_h rows high, run `turns` turns deep
// touches only buffer rows (y0 - turns + j) mod modrows, j = 0 .. tile_h + 2 turns - 1.  With
// modrows >= tile_h + 2 turns that window wraps past the buffer's last row at most once: rows_a
// rows from row0 on, then rows_b rows from row 0 on (none unless it wraps).  The kernel bases
// one buffer resource at each part (base_a_bytes past the buffer's start; the second part's is
// the buffer's start) and keeps 32-bit offsets within the part; every byte quantity here is
// 64-bit.  false (and empty parts): y0 outside [0, modrows), modrows < tile_h + 2 turns, or a
// window of 2 GiB or more.
constexpr int64_t kTileWindowMaxBytes = (int64_t)1 << 31;
__host__ __device__ inline bool tile_window(int64_t modrows, int64_t pitch_words, int64_t y0, int turns,
                                            int tile_h, int64_t *row0, int64_t *rows_a,
                                            int64_t *rows_b, uint64_t *base_a_bytes)
{
    *row0 = *rows_a = *rows_b = 0;
    *base_a_bytes = 0;
    const int64_t rows = (int64_t)tile_h + 2 * (int64_t)turns;
    if (turns < 1 || tile_h < 1 || pitch_words < 1 || y0 < 0 || y0 >= modrows || modrows < rows)
        return false;
    // (rows first: pitch_words * 8 * rows stays far below 2^63 once rows < 2^31 / 8)
    if (pitch_words >= kTileWindowMaxBytes / 8 || rows * (pitch_words * 8) >= kTileWindowMaxBytes)
        return false;
    const int64_t r0 = y0 - turns < 0 ? y0 - turns + modrows : y0 - turns;
    const int64_t ra = rows < modrows - r0 ? rows : modrows - r0;
    *row0 = r0;
    *rows_a = ra;
    *rows_b = rows - ra;
    *base_a_bytes = (uint64_t)r0 * (uint64_t)pitch_words * 8u;
    return true;
}
// the buffer a k_step_tile launch addresses runs the big form: forced, or 2 GiB and more
inline bool tile_buffer_big(long long modrows, long long pitch_words, bool forced)
{
    return forced || modrows * pitch_words * 8 >= (1ll << 31);
}
// a shape the big form runs on that buffer: a code of the set (one word per lane), whole-word
// rows of at least 256 cells, and a window that wraps at most once and stays below 2 GiB
inline bool tile_big_ok(int width, long long modrows, long long pitch_words, int turns, int tile_h,
                        int code)
{
    int64_t r0, ra, rb;
    uint64_t ba;
    return width >= 256 && width % 64 == 0 && tile_code_big(code) &&
           tile_window(modrows, pitch_words, 0, turns, tile_h, &r0, &ra, &rb, &ba);
}
// the tallest tile such a buffer takes at that depth (the repacked narrow column's tiles are
// taller than the launch's tile height: tile_grid_big below)
inline int tile_big_max_h(long long modrows, long long pitch_words, int turns)
{
    const long long by_bytes = ((1ll << 31) - 1) / (pitch_words * 8) - 2 * turns;
    const long long by_rows = modrows - 2 * turns;
    const long long h = by_rows < by_bytes ? by_rows : by_bytes;
    return h < 0 ? 0 : h > (1 << 30) ? 1 << 30 : (int)h;
}

// ---- the row seam.  A row of `width` cells, width % 64 = r in 1 .. 63, has nw = L + 1 words;
// its last word w[L] holds r cells and zero padding (the board invariant).  K1t's lanes hold
// virtual lane columns: column v = cells 64 v .. 64 v + 63 (mod width), so the columns -1 and
// >= L are no real word but the stitch of two:
//     v = -1          (w[L-1] >> r) | (w[L] << (64 - r))
//     v = L           w[L] | (w[0] << r)
//     v = L + 1 + j   (w[j] >> (64 - r)) | (w[j+1] << r)
// and 0 .. L - 1 are the words themselves.  A lane's primary word is the one at its column
// wrapped by whole words (v < 0: L; v >= nw: v - nw), the second word sits at seam_second_col.
__host__ __device__ inline int seam_primary_col(int v, int L) { return v < 0 ? L : v > L ? v - L - 1 : v; }
__host__ __device__ inline int seam_second_col(int v, int L) { return v < 0 ? L - 1 : v == L ? 0 : v - L; }
// (lo >> s) | (hi << (32 - s)), s in 0 .. 32
__host__ __device__ inline uint32_t seam_funnel32(uint32_t lo, uint32_t hi, int s)
{
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> s);
}
// (lo >> a) | (hi << (64 - a)), a in 1 .. 63, of two words in the standard layout or (il) in the
// interleaved one (even cells in the low dword, odd cells in the high one): there an even
// a = 2 q funnels both dword pairs by q, and an odd a = 2 q + 1 swaps their roles -- the new
// even dword is the odd dwords funnelled by q, the new odd dword the even ones by q + 1.
// (odd = a & 1, passed apart: the kernel's lanes funnel by r or by 64 - r, amounts that differ
// from lane to lane but have one parity, and that keeps this branch on the scalar unit)
__host__ __device__ inline uint64_t seam_funnel(uint64_t lo, uint64_t hi, int a, bool odd, bool il)
{
    if (!il) return (lo >> a) | (hi << (64 - a));
    const uint32_t le = (uint32_t)lo, lod = (uint32_t)(lo >> 32);
    const uint32_t he = (uint32_t)hi, hod = (uint32_t)(hi >> 32);
    const int q = a >> 1;
    uint32_t e, o;
    if (odd) {
        e = seam_funnel32(lod, hod, q);
        o = seam_funnel32(le, he, q + 1);
    } else {
        e = seam_funnel32(le, he, q);
        o = seam_funnel32(lod, hod, q);
    }
    return ((uint64_t)o << 32) | e;
}
// virtual column v (-1 or >= L) from its primary word p and its second word s.  odd = r & 1:
// r and 64 - r have one parity, so the interleaved funnel's form is the same for every lane
// (the kernel passes it as a constant of its load stage's two forms).
__host__ __device__ inline uint64_t seam_stitch(uint64_t p, uint64_t s, int v, int L, int r, bool odd,
                                                bool il)
{
    const bool west = v < 0, last = v == L;
    const uint64_t lo = west ? s : last ? 0ull : p, hi = west ? p : s;
    return (last ? p : 0ull) | seam_funnel(lo, hi, west ? r : 64 - r, odd, il);
}

// width: the board's, for a launch across the row seam (width % 64 != 0: a seam code, tiles no
// wider than the row); 0: a board of whole words
bool tile_shape_ok(int nw, int turns, int tile_h, int tile_w, int seg, int width = 0);
int tile_waves(int turns, int tile_h, int tile_w, int seg);
// resident workgroups per CU of that launch (occupancy API: VGPRs, LDS; 0 on error)
// (of the form launch_tile picks for a plain launch: the seam kernel by the width, the pair form
// by tile_duo_env, below)
int tile_blocks_per_cu(int turns, int tile_h, int tile_w, int seg, int width = 0);
// (gol_tile_seam.hip) the k_step_tile_seam instantiation of a code, or nullptr
void *tile_seam_kernel(int code);
// The tiles of one k_step_tile launch over `rows` rows of nw words.  A row's lane columns
// make ntx = ceil(nl / tile_w) tile columns; when the last one is ragged (r < tile_w lanes)
// and packs more row segments into a wave at its own width (G' = 64 / (r + 2) > G), it is cut
// into n_narrow tiles of narrow_w = r lanes x narrow_h rows of its own -- the workgroup size
// is the launch's, so such a tile holds waves x G' x SEG - 2 turns rows -- instead of nty_main
// full-price tiles: tiles [0, ntx_main x nty_main) are the full-width ones (ntx_main = ntx - 1
// columns), the rest the narrow column's, top to bottom.  No repack (n_narrow = 0, ntx_main =
// ntx): r = tile_w, G' = G, no fewer workgroups, ORD 3 / 7 / 8 / 9, or GOL_TILE_REPACK=0 in
// the environment (A/B runs; read at every call).
struct TileGrid {
    int ntx_main, nty_main;
    int n_narrow, narrow_w, narrow_h;
    long long tiles() const { return (long long)ntx_main * nty_main + n_narrow; }
};
TileGrid tile_grid(int nw, int rows, int turns, int tile_h, int tile_w, int seg);
// (gol_tile_big.hip) the k_step_tile_big instantiation of a code, or nullptr
void *tile_big_kernel(int code);
// (gol_tile_duo.hip) the k_step_tile_duo instantiation of a code, or nullptr
void *tile_duo_kernel(int code);
// GOL_TILE_DUO in the environment: unset or non-zero = the pair form where a code has one, 0 =
// the plain kernel everywhere (A/B runs).  Read at create (Ctx::tile_duo) and by
// tile_blocks_per_cu, which the planner and the tile search ask at create too.
bool tile_duo_env();
// tile_grid for a launch of the big form: the narrow column's tiles no taller than max_h
// (tile_big_max_h: their window, too, wraps at most once and stays below 2 GiB) -- more of
// them, or no repack when that saves no workgroup.  A real board of 2 GiB or more has far more
// rows than any tile; the cap binds on the small buffers the form is forced on.
inline TileGrid tile_grid_big(int nw, int rows, int turns, int tile_h, int tile_w, int seg, int max_h)
{
    TileGrid g = tile_grid(nw, rows, turns, tile_h, tile_w, seg);
    if (g.n_narrow > 0 && g.narrow_h > max_h) {
        const long long n = max_h > 0 ? ((long long)rows + max_h - 1) / max_h : g.nty_main;
        if (n >= g.nty_main) {
            g.ntx_main += 1;
            g.n_narrow = g.narrow_w = g.narrow_h = 0;
        } else {
            g.n_narrow = (int)n;
            g.narrow_h = (int)((rows + n - 1) / n);
        }
    }
    return g;
}
// workgroups of a plain launch of `turns` turns (tile_grid); turns = 0: the rectangular grid
// ntx x nty of the resident kernels (K1p / K1q / K1r find their neighbours by tile index)
long long tile_count(int nw, int rows, int tile_h, int tile_w, int seg, int turns = 0);
hipError_t launch_tile(const StepArgs &a, int turns, hipStream_t s);
// K1p k_tile_persist (gol_tile_lab.h): `turns` turns in blocks of K on tiles resident for the whole
// launch, exchanging borders between blocks through u0 / u1 (uncached, board-sized) and
// per-tile flags (uncached, one per tile; epoch above every earlier launch's flags).
// tile_persist_ok: an instantiated code, K within the tile rows, every tile resident at once.
bool tile_persist_ok(int nw, int rows, int turns, int K, int tile_h, int tile_w, int seg, int ncu);
hipError_t launch_tile_persist(const StepArgs &a, int turns, int K, uint64_t *u0, uint64_t *u1,
                               unsigned *flags, unsigned epoch, hipStream_t s);
// K1q k_tile_stream (gol_tile_lab.h): `turns` turns in blocks of K over (block, tile) items taken
// from *counter (value `base` at the launch) by min(items, CUs x occupancy, max_grid if > 0)
// workgroups, whose count goes to *grid (the counter advances by items + grid).  Same u0 / u1 / flags contract
// as K1p; tile_stream_ok: an instantiated code and K within the tile rows (no residency need).
bool tile_stream_ok(int nw, int rows, int K, int tile_h, int tile_w, int seg);
hipError_t launch_tile_stream(const StepArgs &a, int turns, int K, uint64_t *u0, uint64_t *u1,
                              unsigned *flags, unsigned epoch, unsigned *counter, unsigned base,
                              int ncu, int max_grid, unsigned *grid, hipStream_t s);
// K1r k_tile_ring (gol_tile_lab.h): K1p's contract (flags, epoch) with the tiles kept in registers
// across blocks; only their rings pass through u0 / u1 (uncached, board-sized).
bool tile_ring_ok(int nw, int rows, int K, int tile_h, int tile_w, int seg, int ncu);
// gcount (tools experiments, else nullptr): a grid-wide barrier per block on that counter,
// whose value at the launch is gbase (it advances by tiles x (blocks - 1))
hipError_t launch_tile_ring(const StepArgs &a, int turns, int K, uint64_t *u0, uint64_t *u1,
                            unsigned *flags, unsigned epoch, unsigned *gcount, unsigned gbase,
                            hipStream_t s);
int auto_band(int width, int rows);
hipError_t launch_step(const StepArgs &a, bool fast, hipStream_t s);

// Popcount of rows [row_lo, row_hi) into kShards accumulators (caller zeroes).
hipError_t launch_popcount(const uint64_t *w, int nw, int pitch, int row_lo, int row_hi,
                           unsigned long long *counts, hipStream_t s);

// bytes (nrows x width, row-major, device) -> words rows [row0, row0+nrows).
// blocked (nullable) gets the non-binary mask; nonbin accumulates its popcount.
hipError_t launch_pack(const uint8_t *bytes, int width, int nrows, uint64_t *words,
                       uint64_t *blocked, int nw, int pitch, int row0,
                       unsigned long long *nonbin, hipStream_t s);
// words rows [row0, row0+nrows) -> bytes (nrows x width, 0/255)
hipError_t launch_unpack(const uint64_t *words, int width, int nw, int pitch, int row0,
                         int nrows, uint8_t *bytes, hipStream_t s);

// Random board: buffer row b is global row (grow0 + b) mod gheight.
hipError_t launch_fill_random(uint64_t *words, int width, int nw, int pitch, int nrows,
                              long long grow0, int gheight, uint64_t seed, hipStream_t s);

// Alive list: per-row popcounts, then a row-major scatter of {x, y} int64 pairs.
hipError_t launch_row_popcount(const uint64_t *w, int nw, int pitch, int row0, int nrows,
                               long long *row_counts, hipStream_t s);
hipError_t launch_alive_scatter(const uint64_t *w, int nw, int pitch, int row0, int nrows,
                                long long grow0, const long long *row_offsets,
                                long long *xy, hipStream_t s);

// Flip list (cells that differ between two boards of one pitch, rows [row0, row0 + nrows)):
// per-row popcounts of cur ^ prev into row_counts[nrows], their exclusive scan into
// row_offsets[nrows + 1] (the last entry is the total) -- all on the device -- then a
// row-major scatter of {x, y} int64 pairs to xy[row_offsets[r] - rebase ...].
hipError_t launch_flip_offsets(const uint64_t *cur, const uint64_t *prev, int nw, int pitch,
                               int row0, int nrows, long long *row_counts,
                               long long *row_offsets, hipStream_t s);
hipError_t launch_flip_scatter(const uint64_t *cur, const uint64_t *prev, int nw, int pitch,
                               int row0, int nrows, long long grow0,
                               const long long *row_offsets, long long rebase, long long *xy,
                               hipStream_t s);

}  // namespace golk
