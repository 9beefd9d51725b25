// gol_tile.h -- K1t k_step_tile: K turns per launch on a 2-D tile held in registers, for
// boards too small to fill the GPU with K1s / K1w band pipelines (BASELINE configs[1],
// 5120^2: 80 words per row, 409 600 words in all -- a K1w band pipeline per workgroup leaves
// most CUs idle or runs 16-row bands that are mostly pipeline fill: 1.6 us per turn at best,
// tools/sweep.py).
//
// One workgroup per tile of TH rows x TW words (the reference's calculateNextState over a
// sub-rectangle, SubServer/distributor.go:119-208, advanced K turns at once):
//   * Tile + halo.  The workgroup loads rows [y0 - K, y0 + TH + K) of words
//     [x0 - 1, x0 + TW + 1) (torus wrap), C = TW + 2 words per row: K halo rows above and
//     below, one halo word (64 cells) left and right.  Cells next to the loaded region are
//     unknown; the error they cause moves one cell (row) per turn, so after K <= 64 turns it
//     is still inside the halos and the TH x TW interior is exact.
//   * Lanes.  A wave holds G = 64 / C row segments side by side: lane = group * C + column.
//     Each lane keeps SEG consecutive rows of its word column in registers (2 dwords per
//     row, interleaved layout) for all K turns: the tile never round-trips through memory
//     between turns.  Horizontal neighbours come from the adjacent lanes by DPP (the lanes
//     at a group edge read another group's word: only the halo columns see that); the
//     1-bit funnel shifts and the 7-op rule are K1s's (gol_device.h, life_rule7).
//   * Vertical neighbours.  Per turn each lane sums its segment's first and last row (the
//     3-cell horizontal sums every rule needs) and publishes the two sums in LDS
//     (double-buffered by turn parity: one barrier per turn), then reads the sums of the row
//     above its segment (the previous segment's last) and of the row below (the next one's
//     first), and sweeps its segment top to bottom with a 3-row window of row sums,
//     overwriting each row in place once its sums are taken.  Every row is summed once per
//     turn (exchanging raw rows cost each lane 2 extra row sums a turn: +33 % at SEG = 4).
//   * After K turns the lanes holding interior rows and columns store them.
// Work per turn and lane: SEG row sums (2 DPP, 2 v_alignbit, 4 v_bitop3) + SEG rules
// (14 v_bitop3) + 4 16-B LDS accesses; waste = the (TH + 2K) / TH halo rows, C / TW halo
// columns and the 64 - G C idle lanes.  The engine (tile_candidates + autotune) picks TW, TH,
// SEG and K.
#pragma once
#include "gol_device.h"

#include <type_traits>

#ifndef GOL_TILE_TURN_PAIRS_MAX   // (experiments: the longest segment that runs turns in pairs)
#define GOL_TILE_TURN_PAIRS_MAX 12
#endif
// West funnel shift by lane-mask carry (one word per lane): wl = (o << 1) | (west lane's o >>
// 31) as o + o + carry, the carry-in being the odd dwords' sign bits as a lane mask (one VOPC
// compare) shifted up one lane on the scalar unit, instead of a DPP move and a v_alignbit.
// It issues no faster (the isolated stream: 69.4-73.5 SIMD cycles per 4096 cell-updates
// against 67.8-70.8 for DPP + v_alignbit, tools/calib/stencil_issue.hip) but it drops the
// DPP's data hazard (s_nop) from each row's dependency chain, which pays where the turn is
// latency-bound: SEG 6 at 16384^2 3.02 against 3.22 us per turn, SEG 12 on the 8448-row
// strip 5.63 against 6.06, 33024-row strip 19.2 against 21.0; SEG 24 (issue-bound, 6 waves per
// SIMD) loses 1-3 %, SEG 3 about 1 % (profiles/r05_west_carry_ab.log).  So segments of 4..16
// rows take it.  GOL_TILE_WEST_CARRY=0: never (A/B builds).
#ifndef GOL_TILE_WEST_CARRY
#define GOL_TILE_WEST_CARRY 1
#endif
template <int SEG, int W>
constexpr bool tile_west_carry() { return GOL_TILE_WEST_CARRY && W == 1 && SEG >= 4 && SEG <= 16; }
// VGPR parity pins (tile_parity_pins below; 0: the compiler's own register numbers, A/B builds:
// make variant VDEFS=-DGOL_TILE_PARITY_PINS=0)
#ifndef GOL_TILE_PARITY_PINS
#define GOL_TILE_PARITY_PINS 1
#endif

namespace golk {

// vpin<N>(x): from here on x lives in VGPR N.  An empty asm statement whose operand is tied to
// the physical register: it emits nothing, the compiler writes x's definition straight into vN
// and goes on scheduling the instructions around it.  (Register names are string literals:
// hence a table, indexed at compile time from the pinned turn's unrolled rows.)
template <int N>
__device__ __forceinline__ void vpin(uint32_t &x);
#define GOL_VPIN(N)                                                                               \
    template <>                                                                                   \
    __device__ __forceinline__ void vpin<N>(uint32_t &x) { asm("" : "+{v" #N "}"(x)); }
#define GOL_VPIN8(A, B, C, D, E, F, G, H)                                                         \
    GOL_VPIN(A) GOL_VPIN(B) GOL_VPIN(C) GOL_VPIN(D) GOL_VPIN(E) GOL_VPIN(F) GOL_VPIN(G) GOL_VPIN(H)
GOL_VPIN8(0, 1, 2, 3, 4, 5, 6, 7)
GOL_VPIN8(8, 9, 10, 11, 12, 13, 14, 15)
GOL_VPIN8(16, 17, 18, 19, 20, 21, 22, 23)
GOL_VPIN8(24, 25, 26, 27, 28, 29, 30, 31)
GOL_VPIN8(32, 33, 34, 35, 36, 37, 38, 39)
GOL_VPIN8(40, 41, 42, 43, 44, 45, 46, 47)
GOL_VPIN8(48, 49, 50, 51, 52, 53, 54, 55)
GOL_VPIN8(56, 57, 58, 59, 60, 61, 62, 63)
GOL_VPIN8(64, 65, 66, 67, 68, 69, 70, 71)
GOL_VPIN8(72, 73, 74, 75, 76, 77, 78, 79)
#undef GOL_VPIN8
#undef GOL_VPIN

// The register plan of a pinned turn (ORD 5's turn4, one word per lane, SEG even).  A
// v_bitop3_b32 whose three source VGPRs share one register-number parity issues at half rate
// ("VGPR parity pins"), and the compiler does not number registers by parity.  The
// plan names a register for every value whose parity decides a triple; everything else --
// wl, er, lm, g1, g2, the LDS addresses, what ds_read returns -- stays the compiler's.
//   cells   row i: even dword v(2i), odd dword v(2i+1).  (wl, e, o) and (e, o, er) are mixed
//           whatever wl and er get.
//   sums    row j's sum k has parity (j + k) & 1: the rule's (a, b, c) triples read rows
//           j-1, j, j+1, so two of one parity and one of the other.  Five 4-register sets
//           from v(2 SEG) on: A0, A1 (even rows, sum k in base + k), B0, B1 (odd rows from 3
//           on, sum k in base + (k ^ 1)), S (row 1, as B: its sums stay live to the end of the
//           turn for row 0's rule).  Row j takes set (j >> 1) & 1 of its class, so the three
//           rows of a window never share a set.
//   LDS     put stores one even-aligned 4-register tuple and get returns one, so position q of
//           a slot has parity q & 1.  Row 0 (class A) is stored in order.  Row SEG - 1 is odd:
//           the bottom-edge array holds its sums in the order 1, 0, 3, 2, which is how set B
//           holds them -- no copy before the put, and what get returns from that array (the
//           row above the segment, the segment's own last row) has class B's parities.  Then
//           row 0's rule reads (U: B, F: A, S1: B) and row SEG - 1's (row SEG - 2: A, Lr: B,
//           D: A): the chain closes at both ends.
//   rule    per dword d (centre C = the cell, parity d): lx and hm opposite to C, hx opposite
//           to lx; then (lm, lx, C), (hm, C, g1) and (lx, hx, g2) are mixed whatever lm, g1,
//           g2 get.  Two of the three take the registers of the donor, the row whose sums die
//           in this rule (row i - 1; for row 0 the kept sums of row 1): its sums 2d and 2d + 1
//           sit in an even / odd pair.  The one with C's parity takes hx.  If that is sum
//           2d + 1's, lx overwrites sum 2d in place (after lm) and hx sum 2d + 1 (after hm);
//           else hx overwrites sum 2d (after lm and lx) and hm sum 2d + 1 (after hx).  The
//           third value (hm, resp. lx) takes one register per dword after the sums.  Row 2 has
//           no donor (row 1's sums stay live for row 0's rule): lx and hm take that register
//           and a second one, hx the cell's own register once g2 has read the centre.
//           Naming the donor's registers rather than a fixed set for all rows keeps the
//           rules of consecutive rows independent: with four fixed registers and hx always in
//           the cell the loop was as clean and no faster than the compiler's.
// tools/vgpr_parity.py counts the triples in the compiled loop; tests/test_tile_parity_cpu.py
// asserts the count is zero.
constexpr int tile_pin_cell(int i, int d) { return 2 * i + d; }
constexpr int tile_pin_sum(int seg, int j, int k)
{
    const int base = 2 * seg + (j == 1 ? 16 : (j & 1) * 8 + ((j >> 1) & 1) * 4);
    return base + ((j & 1) ? k ^ 1 : k);
}
// (t: 0 the third value of a rule, 1 row 2's second one)
constexpr int tile_pin_tmp(int seg, int d, int t) { return 2 * seg + 20 + 2 * t + (d ^ 1); }
// Which instantiations run the plan: the 65536^2-class segment in its plain and counted forms
// (tools/vgpr_parity.py: 43 and 117 same-parity v_bitop3 of 288 without it; +3 % on the bench,
// -10 % per turn on a count engine).  Not the big form: its loop is as clean under the plan
// (25 -> 0) and ran 11 % slower at 65536^2, 122.9-123.1k against 138.5-139.2k GCUPS under
// GOL_TILE_BIG=1 ("VGPR parity pins").
template <int SEG, int ORD, int W, bool PERSIST, bool CNT, bool SEAM, bool BIG>
constexpr bool tile_parity_pins()
{
    return GOL_TILE_PARITY_PINS && ORD == 5 && W == 1 && !PERSIST && !SEAM && !BIG &&
           SEG == 16;
}

constexpr int kTileMaxWaves = 16;                       // 1024 threads per workgroup
// dynamic LDS of a workgroup of `threads` threads: row sums of the segments' edge rows (16 B
// per word of the lane), first and last row, two turn parities; then one progress flag per
// wave (ORD 4), 64 B
constexpr size_t tile_lds_bytes(int threads, int words)
{
    return (size_t)threads * 4 * 16 * words + 4 * kTileMaxWaves;
}
// tile_seg = SEG + 100 * ORD + 1000 * (W - 1): rows per lane segment, turn order (0: in order;
// 1: interior rows, then the edge rows; 2: the same with the barrier after the interior rows;
// 4: ORD 1 with no workgroup barrier -- each wave waits only for its two neighbour waves'
// published edge sums, through per-wave progress flags in LDS; 5: ORD 1 with the edge sums
// read back from LDS instead of kept in registers; 6: ORD 5 with the barrier after the
// interior rows; 7: ORD 5 with the tile's two halo segments in wave 0, which skips the rows
// the shrinking trapezoid no longer needs -- see tile_pass; 8: ORD 5's turn as generated
// inline asm with a hand-made, parity-aware VGPR assignment; 9: ORD 8 with ds_bpermute lane
// shifts -- 7, 8 and 9 in the tools build only), words per lane
constexpr int tile_seg_rows(int code) { return code % 100; }
constexpr int tile_seg_words(int code) { return code / 1000 + 1; }
// counted launches (k_step_tile_cnt), after the flags: one sum per (turn, wave), then one word
// of row bits per thread
constexpr size_t tile_count_lds_bytes(int threads)
{
    return 4 * (size_t)kMaxTileTurns * kTileMaxWaves + 4 * (size_t)threads;
}
#if !GOL_TILE_LAB   // (a lab build: gol_tile_lab.h's, whose experiments lay their slots out otherwise)
constexpr size_t tile_lds_bytes_code(int threads, int code)
{
    return tile_lds_bytes(threads, tile_seg_words(code));
}
#endif

// lane / C for lane < 64 as a multiply and a shift: rcp = ceil(65536 / C), exact for every
// C = 3 .. 64 (checked below), so no kernel divides by a tile's width
constexpr uint32_t tile_rcp16(int c) { return (65536u + (uint32_t)c - 1u) / (uint32_t)c; }
constexpr bool tile_rcp16_exact()
{
    for (int c = 3; c <= 64; ++c)
        for (uint32_t l = 0; l < 64; ++l)
            if (((l * tile_rcp16(c)) >> 16) != l / (uint32_t)c) return false;
    return true;
}
static_assert(tile_rcp16_exact(), "lane * ceil(65536 / C) >> 16 == lane / C below 64");

// One tile of a launch, wave-uniform: its width in lanes and height in rows, its first lane
// column and buffer row, the row segments a wave holds side by side (64 / (tw + 2)) and
// tile_rcp16(tw + 2).  The tiles of one launch need not be alike (golk::tile_grid: the narrow
// last column); everything tile_pass does is expressed in these values.
struct TilePos {
    int tw, th, x0, y0, g;
    uint32_t rcp;
};
// One launch's tiles as k_step_tile / k_step_tile_cnt take them (launch_tile fills this from
// golk::tile_grid): tiles [0, n_main) are tile_w x band, ntx_main to a tile row; tiles
// [n_main, ntiles) are the narrow column's, narrow_w x narrow_h, at lane column ntx_main x
// tile_w.  Index 0 of g / rcp: the main tiles, 1: the narrow ones.
struct TileLaunch {
    int ntiles, n_main, ntx_main;
    uint32_t inv_ntx;           // floor(2^32 / ntx_main) + 1 (ntx_main >= 2; else unused)
    int narrow_w, narrow_h;
    int g[2];
    uint32_t rcp[2];
};
// (blockIdx-derived: the split stays on the scalar unit)
__device__ __forceinline__ TilePos tile_pos(const StepArgs &a, const TileLaunch &L, int tile)
{
    if (tile >= L.n_main)
        return TilePos{L.narrow_w, L.narrow_h, L.ntx_main * a.tile_w,
                       a.row_lo + (tile - L.n_main) * L.narrow_h, L.g[1], L.rcp[1]};
    // tile / ntx_main by the host's reciprocal: the estimate is the quotient or one more
    int ty = tile;
    if (L.ntx_main > 1) {
        ty = (int)__umulhi((uint32_t)tile, L.inv_ntx);
        ty -= ty * L.ntx_main > tile ? 1 : 0;
    }
    const int tx = tile - ty * L.ntx_main;
    return TilePos{a.tile_w, a.band, tx * a.tile_w, a.row_lo + ty * a.band, L.g[0], L.rcp[0]};
}

// 3-cell row sums of one row: per word w (even dword e, odd dword o) the sums of the even
// cells (s[4w], s[4w+1]) and of the odd cells (s[4w+2], s[4w+3]); K1s's stage, with the
// neighbour words inside the lane taken as they are
template <int SEG, int W>
__device__ __forceinline__ void tile_rsum(const uint32_t (&x)[2 * W], uint32_t (&s)[4 * W])
{
    constexpr int ND = 2 * W;
    const uint32_t Rt = dpp_from_upper_z(x[0]);      // east lane's first even cells
#pragma unroll
    for (int w = 0; w < W; ++w) {
        const uint32_t e = x[2 * w], o = x[2 * w + 1];
        uint32_t wl;
        if constexpr (tile_west_carry<SEG, W>()) {
            // every lane is active here (the idle lanes run the turn too), so the mask
            // holds every lane's sign bit; lane 0 gets carry 0, as the DPP's bound_ctrl
            const uint64_t m = __builtin_amdgcn_ballot_w64((int)o < 0) << 1;
            uint64_t co;
            asm("v_addc_co_u32_e64 %0, %1, %2, %2, %3" : "=v"(wl), "=&s"(co) : "v"(o), "s"(m));
        } else {
            const uint32_t L = dpp_from_lower_z(x[ND - 1]);   // west lane's last odd cells
            wl = __builtin_amdgcn_alignbit(o, w == 0 ? L : x[2 * w - 1], 31);
        }
        const uint32_t er = __builtin_amdgcn_alignbit(w == W - 1 ? Rt : x[2 * w + 2], e, 1);
        s[4 * w + 0] = xor3(wl, e, o);
        s[4 * w + 1] = maj(wl, e, o);
        s[4 * w + 2] = xor3(e, o, er);
        s[4 * w + 3] = maj(e, o, er);
    }
}
// next state of the lane's row from the sums of the rows above (A), at (B) and below (Cs)
template <int W>
__device__ __forceinline__ void tile_rule(const uint32_t (&A)[4 * W], const uint32_t (&B)[4 * W],
                                          const uint32_t (&Cs)[4 * W], uint32_t (&x)[2 * W])
{
    constexpr int ND = 2 * W;
    uint32_t n[ND];
#pragma unroll
    for (int d = 0; d < ND; ++d)
        n[d] = life_rule7(A[2 * d], B[2 * d], Cs[2 * d], A[2 * d + 1], B[2 * d + 1],
                          Cs[2 * d + 1], x[d]);
#pragma unroll
    for (int d = 0; d < ND; ++d) x[d] = n[d];
}
// What a lab hook sees of a pass: its rows, and copies of its geometry
template <int SEG, int ND>
struct TileView {
    uint32_t (&v)[SEG][ND];
    const StepArgs &a;
    const TilePos &pos;
    uint4 *xsh;
    __amdgpu_buffer_rsrc_t rout;
    int TW, C, G, K, TH, nl, y0, x0, lane, wave, nslot, myslot, s_up, s_dn;
    int wrow0, wrow1, lastrow;
    uint32_t pitch_b, span, off_first;
};
struct TileNoLab {
    static constexpr bool kBlocks = false;
};
// (defined in gol_tile_lab.h)
template <int SEG, int ORD, int W>
constexpr bool tile_lab_edge_rows();
template <int SEG>
__device__ __forceinline__ void tile_lab_put_rows(uint4 *slot, const uint32_t (&v)[SEG][2]);
template <int SEG, int W>
__device__ __forceinline__ void tile_lab_get_rows(const uint4 *base, int s_up, int s_dn,
                                                  uint32_t (&Us)[4 * W], uint32_t (&Ds)[4 * W]);
template <int SEG, int ORD, class View>
__device__ __forceinline__ void tile_lab_asm_loop(const View s);
#if !GOL_TILE_LAB
template <int SEG, int ORD, int W>
constexpr bool tile_lab_edge_rows() { return false; }
#endif
// W words per lane (2W dwords, interleaved layout word by word).  With W = 2 the lane's two
// words are neighbours, so only the outer edges need a lane shift: per row 2 DPP + 2W funnel
// shifts + 4W v_bitop3 instead of W x (2 + 2 + 4) -- 48 instead of 52 SIMD cycles per 4096
// cell-updates with the rule.
// One pass of K turns over one tile (the body of k_step_tile, and of each block of
// K1p / item of K1q, gol_tile_lab.h).  PERSIST: the workgroup stays for
// further passes, so no wave leaves the trapezoid early -- every wave runs every turn (a wave
// past the trapezoid computes halo rows nobody reads) and the pass returns on every path.  (A
// leaving wave would have to meet the barriers of its remaining turns, and that exit path alone
// took the SEG 24 pass from 80 to 126 VGPRs.)
// CNT (k_step_tile_cnt: GOL_FLAG_COUNT_EVERY_TURN on a K1t engine): after every turn t = 1 .. K
// the alive cells of the tile's counted region go to a.counts[(t - 1) * kShards + shard], the
// slot of turn turn0 + t (the engine passes K consecutive, zeroed slots).  The region is fixed
// for the launch and is exactly what the final store writes, cut to rows [cnt_lo, cnt_hi):
// tile rows [K, K + TH) below row_hi, interior lane columns inside the row -- every board word
// belongs to one tile's region.  Per turn a counting wave popcounts its counted rows
// (v_bcnt_u32_b32 accumulates: 2 VALU per row), reduces over its lanes by DPP and leaves the sum
// in its own LDS word [t][wave]; nothing else is synchronised per turn (also under ORD 4's
// flags).  Only the waves holding a row of [K, K + TH) count: they never leave the trapezoid,
// and one of them adds the waves' sums up after one barrier at the end of the launch -- one
// global atomic per (workgroup, turn) with a non-zero count.
// SEAM (k_step_tile_seam: a board whose width is no multiple of 64, r = width % 64 cells in the
// row's last word L = nw - 1): the torus seam in x falls inside a word, so the lanes whose
// virtual column is -1 or >= L (gol_kernels.h, seam_stitch) hold words stitched from two real
// ones -- the wrapped cells sit where the padding bits were, and they are halo like any other.
// Only the load stage (a second word per row for those lanes, in the tiles that touch the seam:
// the first tile column and the ones that reach column L) and the store stage (the lane of
// column L clears its bits r .. 63: the padding of both boards stays zero) differ; the turns
// and the LDS exchange are the plain kernel's.  One word per lane, plain launches, no counts.
// BIG (k_step_tile_big: a buffer of 2 GiB or more, whose rows a 32-bit byte offset from its start
// does not reach): the buffer resources are rebased per workgroup onto the rows the tile touches
// (gol_kernels.h, tile_window) -- a 64-bit base formed on the scalar unit, 32-bit offsets within
// the window, num_records the window's bytes.  Again only the load and the store stage differ
// (below); one word per lane, plain launches, whole-word rows, no counts.
// DUO (k_step_tile_duo: ORD 5's turn with the interior rows ruled in pairs): rows i and i + 1 of
// the pairs (1, 2), (3, 4), .., (SEG - 3, SEG - 2) share the binary sum of their two rows' sums
// (gol_device.h, life_pair_sum / life_rule_pair): 12 operations per pair and dword instead of
// 2 x life_rule7's 7.  Rows 0 and SEG - 1 keep life_rule7 on the sums turn4 has live at the end
// of the turn.  Only the turn differs (turn4d below): the loads, the LDS exchange, the barrier
// and the stores are the plain kernel's.  One word per lane, plain launches, whole-word rows.
// The registers are the compiler's: 47 of the loop's 232 v_bitop3 read three VGPRs of one
// parity.  A plan in the manner of tile_parity_pins brought that to 0 at the same 328 VALU and
// 64 VGPRs and measured no faster ("Shared row-pair sums"), so none is kept.
// Lab (gol_tile_lab.h): the experiments of the tools build enter the pass at named spots -- a
// block loop in place of the turn loop (Lab::kBlocks), the ORD 8 / 9 loop, and edge rows
// exchanged raw (kEdgeRows) -- each a function of that header over a TileView of the pass's
// locals.  A product build has none: the predicate is false and no hook is instantiated.
template <int SEG, int ORD, int W, bool PERSIST, bool CNT = false, bool SEAM = false,
          bool BIG = false, bool DUO = false, class Lab = TileNoLab>
__device__ __forceinline__ void tile_pass(const uint64_t *__restrict__ in,
                                          uint64_t *__restrict__ out, const StepArgs &a,
                                          int turns, const TilePos &pos, Lab lab = Lab{})
{
    constexpr int ND = 2 * W;                            // dwords per lane and row
    constexpr int NS = 2 * ND;                           // row-sum dwords (2 bits per dword)
    static_assert(SEG >= 2, "two edge rows per segment");
    constexpr bool kPins = !DUO && tile_parity_pins<SEG, ORD, W, PERSIST, CNT, SEAM, BIG>();
    static_assert(!DUO || (ORD == 5 && W == 1 && SEG % 2 == 0 && SEG >= 4 && !PERSIST &&
                           !CNT && !SEAM && !BIG),
                  "pair turns: ORD 5, an even segment (whole pairs between the two edge rows)");
    static_assert(!kPins || (SEG % 2 == 0 && SEG >= 4 && 2 * SEG + 24 <= 80),
                  "pinned turns: an even segment (the plan's last row is odd), registers below v80");
    // per turn parity: the 3-cell row sums of the first / last row of every segment,
    // segment-major, C slots per segment (dynamic LDS, W uint4 per slot)
    extern __shared__ uint4 xsh[];
    const int nslot = (int)(blockDim.x);                 // waves x 64 >= segments x C
    const int TW = pos.tw, C = TW + 2, G = pos.g;        // (in lanes of W words)
    const int K = turns, TH = pos.th;
    const int nl = a.nw / W;                             // lane columns per row
    const int y0 = pos.y0;
    const int x0 = pos.x0;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int group = (int)(((uint32_t)lane * pos.rcp) >> 16), col = lane - group * C;
    const bool live = group < G;                         // lanes past G groups: idle
    const int nseg = (TH + 2 * K + SEG - 1) / SEG;       // segments the tile needs
    // ORD 7 (G == 2, nseg >= 3; host-checked): wave 0 holds the top segment (group 0) and the
    // bottom one (group 1, its rows in reverse order), the other waves the segments between,
    // in order.  Both of wave 0's segments then leave the trapezoid from their local row 0
    // on: turn t changes tile rows [t + 1, 2K + TH - 1 - t), so local rows 0 .. t of either
    // segment are outside it, and wave 0 can skip them for both groups at once (turn4 below).
    // The rule is symmetric in up and down, so a reversed segment runs the same body; only
    // its loads, stores and LDS edge slots are mirrored.
    constexpr bool kHalo = ORD == 7;
    static_assert(!kHalo || W == 1, "ORD 7: one word per lane");
    const int seg = !kHalo ? wave * G + group
                           : wave == 0 ? (group == 0 ? 0 : nseg - 1) : (wave - 1) * G + group + 1;
    const bool rev = kHalo && wave == 0 && group == 1;   // (a lane-varying flag: group 1 only)
    const int slot = seg * C + col;

    // lane column (torus wrap) and the lane's rows: tile row t = seg * SEG + i is buffer row
    // y0 - K + t (mod modrows; rows past the tile are read, never stored)
    // (gx lies in [-1, nl + C - 2): one wrap either way unless the row is narrower than the
    // tile -- a wave-uniform case)
    int gx = x0 - 1 + (live ? col : 0);
    if (nl < C) {
        while (gx < 0) gx += nl;
        while (gx >= nl) gx -= nl;
    } else {
        gx += gx < 0 ? nl : 0;
        gx -= gx >= nl ? nl : 0;
    }
    static_assert(!SEAM || (W == 1 && !PERSIST && !CNT && ORD != 3 && ORD < 7),
                  "seam launches: plain k_step_tile, one word per lane, no counts");
    // SEAM: the lane's virtual column, and the byte distance from its primary word (column gx,
    // wrapped by whole words) to its second one; seam_tile is wave-uniform
    [[maybe_unused]] bool seam_tile = false, seam_lane = false;
    [[maybe_unused]] int seam_v = 0;
    [[maybe_unused]] uint32_t seam_d = 0;
    if constexpr (SEAM) {
        const int L = nl - 1;
        seam_tile = x0 == 0 || x0 + TW >= L;
        seam_v = x0 - 1 + (live ? col : 0);
        seam_lane = seam_tile && live && (seam_v < 0 || seam_v >= L);
        // (a column past nw is junk no stored cell's cone reaches: any word inside the row)
        const int g2 = seam_lane ? min(seam_second_col(seam_v, L), L) : gx;
        seam_d = (uint32_t)(g2 - gx) * 8u;
    }
    const int M = a.modrows;
    const uint32_t pitch_b = (uint32_t)a.pitch * 8u;
    const uint32_t span = (uint32_t)M * pitch_b;
    // the tile's first row wraps on the scalar unit; the lane's segment then starts less than
    // 2 M rows down unless the buffer is shorter than the workgroup's rows (one ballot)
    int rbase = y0 - K;                                  // (>= -K, < M)
    if (rbase < 0) {
        rbase += M;
        while (rbase < 0) rbase += M;                    // (a buffer of fewer than K rows)
    }
    int r = rbase + (live ? seg : 0) * SEG + (rev ? SEG - 1 : 0);
    if (__builtin_amdgcn_ballot_w64(r >= 2 * M) != 0) {
        while (r >= M) r -= M;
    } else {
        r -= r >= M ? M : 0;
    }
    uint32_t off = (uint32_t)r * pitch_b + (uint32_t)gx * (8u * W);
    [[maybe_unused]] const uint32_t off_first = off;     // (the segment's first row)
    const uint32_t lstep = rev ? span - pitch_b : pitch_b;   // (a reversed segment loads upwards)
    const __amdgpu_buffer_rsrc_t rin =
        __builtin_amdgcn_make_buffer_rsrc((void *)in, (short)0, (int)span, kBufFlags);
    static_assert(!BIG || (W == 1 && !PERSIST && !CNT && !SEAM && ORD != 3 && ORD < 7),
                  "big launches: plain k_step_tile, one word per lane, no seam, no counts");
    // BIG: the window's two parts (rows [0, big_ra) of the tile from buffer row row0 on, rows
    // [big_ra, big_ra + big_rb) from buffer row 0 on: none unless the tile wraps the torus) and
    // the stored rows [y0, y0 + big_rs), each behind a resource of its own whose range is that
    // part alone -- an offset outside it is dropped by the range check, whatever lies there.
    // All of it wave-uniform (the tile's position and the launch's arguments).
    [[maybe_unused]] int big_ra = 0, big_rb = 0, big_rs = 0;
    [[maybe_unused]] __amdgpu_buffer_rsrc_t rin_a = rin, rin_b = rin;
    [[maybe_unused]] auto big_rsrc = [](const void *p, uint64_t byte, int rows, uint32_t row_b) {
        const uint64_t ad = (uint64_t)(uintptr_t)p + byte;
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)ad);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(ad >> 32));
        const int bytes = __builtin_amdgcn_readfirstlane((int)((uint32_t)rows * row_b));
        return __builtin_amdgcn_make_buffer_rsrc((void *)(uintptr_t)(((uint64_t)hi << 32) | lo),
                                                 (short)0, bytes, kBufFlags);
    };
    if constexpr (BIG) {
        int64_t w0, wa, wb;
        uint64_t ba;
        // (host-checked, launch_tile: the window wraps at most once and is below 2 GiB; a tile
        // for which that fails gets empty parts -- it loads zeros and stores nothing)
        (void)tile_window(M, a.pitch, y0, K, TH, &w0, &wa, &wb, &ba);
        big_ra = __builtin_amdgcn_readfirstlane((int)wa);
        big_rb = __builtin_amdgcn_readfirstlane((int)wb);
        big_rs = big_ra > 0 ? max(0, min(TH, a.row_hi - y0)) : 0;
        rin_a = big_rsrc(in, ba, big_ra, pitch_b);
        rin_b = big_rsrc(in, 0, big_rb, pitch_b);
    }
    // (BIG: rows [y0, y0 + TH) below row_hi never wrap; the store offsets count from row y0)
    const __amdgpu_buffer_rsrc_t rout =
        BIG ? big_rsrc(out, (uint64_t)(uint32_t)y0 * pitch_b, big_rs, pitch_b)
            : __builtin_amdgcn_make_buffer_rsrc((void *)out, (short)0, (int)span, kBufFlags);

    // PERSIST: loads bypass this CU's vector L1 (sc1): block b reads rows other CUs wrote
    // since block b - 2 left lines of the same buffer in it, and the L1 is never refreshed
    // by another CU's stores
    constexpr int kLoadAux = PERSIST ? 16 : GOL_TILE_LOAD_AUX;
    uint32_t v[SEG][ND];
    auto load_row = [&](int i, uint32_t voff, uint32_t soff) {
        if constexpr (W == 1) {
            const u32x2 w = __builtin_amdgcn_raw_buffer_load_b64(rin, voff, soff, kLoadAux);
            v[i][0] = w.x;
            v[i][1] = w.y;
        } else {
            const u32x4 w = __builtin_amdgcn_raw_buffer_load_b128(rin, voff, soff, kLoadAux);
            v[i][0] = w.x;
            v[i][1] = w.y;
            v[i][2] = w.z;
            v[i][3] = w.w;
        }
    };
    // No segment of the wave wraps past the buffer's last row inside its SEG rows (one ballot;
    // nearly every wave): one lane offset, the rows stepped by the scalar offset of the buffer
    // instruction -- no VALU per row.  Otherwise the offset wraps row by row.
    // (SEAM: the seam tiles load in their own way, below)
    // BIG: three forms, picked on the scalar unit.  Every row of the wave in the window's first
    // part (nearly every wave): one lane offset from the part's base, the rows stepped by the
    // instruction's scalar offset -- all of it inside the part by the ballot, so nothing relies
    // on the range check, which sees the lane offset without the scalar part.  Otherwise the
    // offset is formed per row in the lane's register, where the range check does see it, with
    // the scalar offset 0: a tile that does not wrap loads through the one resource (its rows
    // past the window -- the last segments' surplus -- are clamped to the window's end, out of
    // range: zeros, which no stored cell's cone reaches); a tile that wraps (the first and
    // last tile rows of a torus) loads every row through both resources and selects per lane
    // -- a row's offset is in range in exactly one part: below the first part's end in the
    // one, negative (above 2^31 as unsigned) or past the end in the other.  kBigChunk rows at a
    // time, as the seam stage: no more than that many row pairs are held beside the segment.
    if constexpr (BIG) {
        const int tr0 = (live ? seg : 0) * SEG;          // the lane's first tile row
        const uint32_t cb = (uint32_t)gx * 8u;
        const int wlim = big_ra + big_rb;
        if (__builtin_amdgcn_ballot_w64(tr0 + SEG > big_ra) == 0) {
            const uint32_t o = (uint32_t)tr0 * pitch_b + cb;
#pragma unroll
            for (int i = 0; i < SEG; ++i) {
                const u32x2 w = __builtin_amdgcn_raw_buffer_load_b64(rin_a, o, (uint32_t)i * pitch_b, kLoadAux);
                v[i][0] = w.x;
                v[i][1] = w.y;
            }
        } else if (big_rb == 0) {
#pragma unroll
            for (int i = 0; i < SEG; ++i) {
                const uint32_t o = (uint32_t)min(tr0 + i, wlim) * pitch_b + cb;
                const u32x2 w = __builtin_amdgcn_raw_buffer_load_b64(rin_a, o, 0, kLoadAux);
                v[i][0] = w.x;
                v[i][1] = w.y;
            }
        } else {
            constexpr int kBigChunk = 4;
            int tb = tr0;
#pragma unroll
            for (int c0 = 0; c0 < SEG; c0 += kBigChunk) {
                u32x2 pa[kBigChunk], pb[kBigChunk];
#pragma unroll
                for (int j = 0; j < kBigChunk; ++j) {
                    if (c0 + j < SEG) {
                        const int t = min(tb + c0 + j, wlim);
                        const uint32_t oa = (uint32_t)t * pitch_b + cb;
                        const uint32_t ob = (uint32_t)(t - big_ra) * pitch_b + cb;
                        pa[j] = __builtin_amdgcn_raw_buffer_load_b64(rin_a, oa, 0, kLoadAux);
                        pb[j] = __builtin_amdgcn_raw_buffer_load_b64(rin_b, ob, 0, kLoadAux);
                    }
                }
#pragma unroll
                for (int j = 0; j < kBigChunk; ++j) {
                    if (c0 + j < SEG) {
                        const bool second = tb + c0 + j >= big_ra;
                        v[c0 + j][0] = second ? pb[j].x : pa[j].x;
                        v[c0 + j][1] = second ? pb[j].y : pa[j].y;
                    }
                }
                // (the next chunk's loads wait for this chunk's words, as in the seam stage)
                if (c0 + kBigChunk < SEG)
                    asm volatile("" : "+v"(tb) : "v"(v[c0 + kBigChunk - 1][0]),
                                 "v"(v[c0 + kBigChunk - 1][1]));
            }
        }
    } else if (SEAM && seam_tile) {
    } else if (!kHalo && __builtin_amdgcn_ballot_w64(r + SEG > M) == 0) {
#pragma unroll
        for (int i = 0; i < SEG; ++i) load_row(i, off, (uint32_t)i * pitch_b);
    } else {
#pragma unroll
        for (int i = 0; i < SEG; ++i) {
            load_row(i, off, 0);
            off += lstep;
            off = off >= span ? off - span : off;        // (the column stays < pitch_b)
        }
    }
    // SEAM: a seam tile loads two words per row -- the primary word and, for the seam lanes,
    // the second one (the other lanes read their primary word twice) -- and stitches, kSeamChunk
    // rows at a time: the loads of a chunk are in flight together, and no more than that many
    // word pairs are held beside the segment (all SEG at once would be 2 SEG more registers).
    // No lane branches: the lanes that are no seam lanes select their primary word.  Four forms
    // of the stage, picked on the scalar unit: the parity of r (seam_funnel's two forms, each
    // straight-line code) x the rows stepped by the instruction's scalar offset (no segment of
    // the wave wraps past the buffer's last row) or by offsets that wrap row by row.
    if constexpr (SEAM) {
        if (seam_tile) {
            const int L = nl - 1, rb = a.width & 63;
            auto seam_load = [&](auto ODD, auto STEP) {
                constexpr bool odd = decltype(ODD)::value, step = decltype(STEP)::value;
                constexpr int kSeamChunk = 4;
                uint32_t o1 = off_first, o2 = off_first + seam_d;
#pragma unroll
                for (int c0 = 0; c0 < SEG; c0 += kSeamChunk) {
                    u32x2 p[kSeamChunk], t[kSeamChunk];
#pragma unroll
                    for (int j = 0; j < kSeamChunk; ++j) {
                        if (c0 + j < SEG) {
                            const uint32_t so = step ? (uint32_t)(c0 + j) * pitch_b : 0u;
                            p[j] = __builtin_amdgcn_raw_buffer_load_b64(rin, o1, so, kLoadAux);
                            t[j] = __builtin_amdgcn_raw_buffer_load_b64(rin, o2, so, kLoadAux);
                            if constexpr (!step) {
                                o1 += lstep;
                                o1 = o1 >= span ? o1 - span : o1;
                                o2 += lstep;             // (its column stays < pitch_b too)
                                o2 = o2 >= span ? o2 - span : o2;
                            }
                        }
                    }
#pragma unroll
                    for (int j = 0; j < kSeamChunk; ++j) {
                        if (c0 + j < SEG) {
                            const uint64_t pw = ((uint64_t)p[j].y << 32) | p[j].x;
                            const uint64_t sw = ((uint64_t)t[j].y << 32) | t[j].x;
                            const uint64_t w = seam_stitch(pw, sw, seam_v, L, rb, odd, true);
                            v[c0 + j][0] = seam_lane ? (uint32_t)w : p[j].x;
                            v[c0 + j][1] = seam_lane ? (uint32_t)(w >> 32) : p[j].y;
                        }
                    }
                    // (the next chunk's loads wait for this chunk's words: their address passes
                    // through an empty asm that reads the chunk's last stitched row)
                    if (c0 + kSeamChunk < SEG)
                        asm volatile("" : "+v"(o1), "+v"(o2) : "v"(v[c0 + kSeamChunk - 1][0]),
                                     "v"(v[c0 + kSeamChunk - 1][1]));
                }
            };
            using std::false_type;
            using std::true_type;
            const bool nowrap = __builtin_amdgcn_ballot_w64(r + SEG > M) == 0;
            if (rb & 1) {
                if (nowrap) seam_load(true_type{}, true_type{});
                else seam_load(true_type{}, false_type{});
            } else {
                if (nowrap) seam_load(false_type{}, true_type{});
                else seam_load(false_type{}, false_type{});
            }
        }
    }

    // (the row sums and the rule: tile_rsum, tile_rule above)
    auto put = [&](uint4 *base, const uint32_t (&S)[NS]) {
#pragma unroll
        for (int q = 0; q < W; ++q)
            base[(size_t)q * nslot * 4] =
                make_uint4(S[4 * q], S[4 * q + 1], S[4 * q + 2], S[4 * q + 3]);
    };
    auto get = [&](const uint4 *base, uint32_t (&S)[NS]) {
#pragma unroll
        for (int q = 0; q < W; ++q) {
            const uint4 u = base[(size_t)q * nslot * 4];
            S[4 * q] = u.x;
            S[4 * q + 1] = u.y;
            S[4 * q + 2] = u.z;
            S[4 * q + 3] = u.w;
        }
    };
    // Slot arrays: [q][parity][top / bottom][slot], q = the word of the lane.  Every lane
    // writes and reads every turn, with no mask: the idle lanes (group >= G) own the slots
    // past the tile's (waves x G x C .. waves x 64), and a segment with no neighbour above
    // (below) reads its own slot.  What it reads there is junk, but it only reaches the tile's
    // outermost row, whose error moves inward one row per turn like that of any halo row.
    const int nlive = (int)(blockDim.x >> 6) * G * C;
    const int myslot = live ? slot : nlive + wave * (64 - G * C) + (lane - G * C);
    const int s_up = live && seg > 0 ? slot - C : myslot;
    const int s_dn = live && seg + 1 < nseg ? slot + C : myslot;
    // a lane's own edge slots and its neighbours', by the lane's local row order: its first
    // row's sums go to the top-edge array and its last row's to the bottom-edge array, and it
    // reads the bottom edge of the segment above and the top edge of the one below -- all
    // mirrored for a reversed segment (ORD 7), whose first row is physically its bottom one
    const int o_wt = (rev ? (int)nslot : 0) + myslot, o_wb = (rev ? 0 : (int)nslot) + myslot;
    const int o_up = rev ? s_dn : (int)nslot + s_up, o_dn = rev ? (int)nslot + s_up : s_dn;
    // Turn parity p uses the slots 2 p nslot further on.  Short segments run two turns per
    // loop iteration with p a compile-time constant (the parity's addresses hoisted out of the
    // loop: 11 % faster turns at SEG 3-4); long ones one turn body with the offset added per
    // turn -- the doubled body of a long segment ran 10-14 % slower (instruction fetch,
    // profiles/r03_tile_unroll_ab.log).  The threshold 12: pairs at SEG 8 are 2-3 % faster
    // than one body, at SEG 16 11-28 % slower (profiles/r03b_tile_pairs_threshold.log).
    constexpr bool kPairs = SEG * W <= GOL_TILE_TURN_PAIRS_MAX;
    constexpr bool kEdgeRows = tile_lab_edge_rows<SEG, ORD, W>();   // (gol_tile_lab.h; else false)
    // (with pairs the lane's four LDS addresses of each parity are loop-invariant registers;
    // one body forms them per turn -- precomputed there, the long bodies ran 4-8 % slower)
    uint4 *const wtop2[2] = {xsh + o_wt, xsh + 2 * nslot + o_wt};
    uint4 *const wbot2[2] = {xsh + o_wb, xsh + 2 * nslot + o_wb};
    const uint4 *const rup2[2] = {xsh + o_up, xsh + 2 * nslot + o_up};
    const uint4 *const rdn2[2] = {xsh + o_dn, xsh + 2 * nslot + o_dn};
    auto wtop = [&](int p, int off) { return kPairs ? wtop2[p] : xsh + off + o_wt; };
    auto wbot = [&](int p, int off) { return kPairs ? wbot2[p] : xsh + off + o_wb; };
    auto rup = [&](int p, int off) { return kPairs ? rup2[p] : (const uint4 *)(xsh + off + o_up); };
    auto rdn = [&](int p, int off) { return kPairs ? rdn2[p] : (const uint4 *)(xsh + off + o_dn); };
    // A wave whose rows are all outside the turn's trapezoid leaves: the tile's rows
    // [t + 1, 2K + TH - 1 - t) change at turn t (t = 0 .. K-1) and need the sums of the rows
    // one further out; a wave above row t (below row 2K + TH - 1 - t) holds no row that any
    // later turn or the final store needs (its rows are < K, resp. >= K + TH), and the
    // workgroup barrier no longer counts it once it has ended.
    // the wave's tile rows (ORD 7: wave 0 spans the whole tile -- it never leaves; wave w > 0
    // holds segments (w - 1) G + 1 ..)
    // (both through readfirstlane: the leave test of the turn loop stays on the scalar unit)
    const int wrow0 = __builtin_amdgcn_readfirstlane(
        !kHalo ? wave * G * SEG : wave == 0 ? 0 : ((wave - 1) * G + 1) * SEG);
    const int wrow1 = __builtin_amdgcn_readfirstlane(
        !kHalo ? wrow0 + G * SEG : wave == 0 ? 1 << 30 : wrow0 + G * SEG);
    // ORD 4: per-wave progress flags after the slot arrays.  flag[w] = the last turn whose
    // edge sums wave w has published (-1 before the first; INT_MAX once it has left), written
    // by lane 0 after its sums: the LDS serves one wave's requests in issue order, so a wave
    // that reads flag[w] >= t reads w's turn-t sums (the K1w hand-off assumption).
    // The sums are double-buffered by turn parity: a wave overwrites its turn-(t-2) slots only
    // after both neighbours published turn t-1, i.e. after they finished reading turn t-2.
    const int nwaves = (int)(blockDim.x >> 6);
    volatile int *const flag = (volatile int *)(xsh + 4 * (size_t)nslot * W);
    if constexpr (ORD == 4) {
        if (lane == 0) flag[wave] = -1;
        __syncthreads();                                  // (once per launch)
    }
    // CNT: the lane's counted rows are local rows [ci_lo, ci_hi) (none on a halo column, an
    // idle lane or a column past the row's end); the waves w_lo .. w_hi hold the tile rows
    // [K, K + TH), and their per-turn sums live after the flags: [turn][wave], 4 B each
    static_assert(!CNT || (W == 1 && !PERSIST && ORD != 3 && ORD < 7),
                  "counted launches: plain k_step_tile, one word per lane");
    [[maybe_unused]] uint32_t *const csum = (uint32_t *)(xsh + 4 * (size_t)nslot * W) + kTileMaxWaves;
    [[maybe_unused]] int cw_lo = 0, cw_hi = -1;
    static_assert(!CNT || SEG <= 32, "counted launches: one word of row bits per lane");
    [[maybe_unused]] bool cwave = false, cuni = false, cany = false;
    // (the lane's row bits wait in LDS, after the sums: only a partly counted wave reads them)
    [[maybe_unused]] uint32_t *const crow = csum + kMaxTileTurns * kTileMaxWaves;
    if constexpr (CNT) {
        cw_lo = K / (G * SEG);
        cw_hi = min(nwaves - 1, (K + TH - 1) / (G * SEG));
        cwave = wave >= cw_lo && wave <= cw_hi;          // (wave-uniform)
        const int ybase = y0 - K + seg * SEG;            // buffer row of the lane's local row 0
        const int ylo = max(y0, a.cnt_lo), yhi = min(min(y0 + TH, a.row_hi), a.cnt_hi);
        const bool ccol = live && col >= 1 && col <= TW && x0 + col - 1 < nl;
        const int ci_lo = min(max(ylo - ybase, 0), SEG), ci_hi = min(max(yhi - ybase, 0), SEG);
        const int cn = ccol && cwave ? max(ci_hi - ci_lo, 0) : 0;
        // bit i: the lane counts its local row i
        crow[threadIdx.x] = cn > 0 ? (~0u >> (32 - cn)) << ci_lo : 0u;
        cany = cn > 0;
        // most waves hold only lanes that count every row or none: 2 VALU per row and one
        // select; a wave with a partly counted segment masks row by row
        cuni = __builtin_amdgcn_ballot_w64(cn != 0 && cn != SEG) == 0;
    }
    // (v_bcnt_u32_b32 adds to its second operand: one chain of 2 SEG instructions.  Written as
    // popcount + sum the compiler counts every dword apart and adds the counts up as a tree, in
    // 2 SEG more instructions and ~25 more registers)
    auto bcnt = [](uint32_t x, uint32_t acc) {
        uint32_t r;
        asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(acc));
        return r;
    };
    auto bcnt0 = [](uint32_t x) {                        // (no register held for the zero)
        uint32_t r;
        asm("v_bcnt_u32_b32 %0, %1, 0" : "=v"(r) : "v"(x));
        return r;
    };
    auto count_turn = [&](int t) {
        if constexpr (CNT) {
            if (!cwave) return;
            uint32_t acc;
            if (cuni) {
                acc = bcnt(v[0][1], bcnt0(v[0][0]));
#pragma unroll
                for (int i = 1; i < SEG; ++i) acc = bcnt(v[i][1], bcnt(v[i][0], acc));
                acc = cany ? acc : 0u;                  // (all of the lane's rows or none)
            } else {
                // (the lane index and the row bits are formed every turn behind an opaque
                // mask: neither they nor the SEG row masks stay in registers across the turns)
                uint32_t all = ~0u;
                asm volatile("" : "+v"(all));
                const uint32_t ln = __builtin_amdgcn_mbcnt_hi(all, __builtin_amdgcn_mbcnt_lo(all, 0u));
                const uint32_t rlo = crow[wave * 64 + (int)ln];
                acc = 0;
#pragma unroll
                for (int i = 0; i < SEG; ++i) {
                    const uint32_t m = 0u - ((rlo >> i) & 1u);
                    acc = bcnt(v[i][1] & m, bcnt(v[i][0] & m, acc));
                }
                // (a DPP read needs 2 wait states after the VALU write of its source, and the
                // compiler does not count an inline-asm instruction as that write)
                asm("s_nop 1" : "+v"(acc));
            }
            // wave sum by DPP: inclusive scan within each row of 16 lanes (row_shr 1, 2, 4, 8),
            // then row 15 of rows 0 / 2 into rows 1 / 3 and lane 31 into rows 2 / 3: lane 63 holds
            // the total (at most 64 x SEG x 64 cells)
            acc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)acc, 0x111, 0xf, 0xf, true);
            acc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)acc, 0x112, 0xf, 0xf, true);
            acc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)acc, 0x114, 0xf, 0xf, true);
            acc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)acc, 0x118, 0xf, 0xf, true);
            acc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)acc, 0x142, 0xa, 0xf, false);
            acc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)acc, 0x143, 0xc, 0xf, false);
            if (lane == 63) csum[t * kTileMaxWaves + wave] = acc;
        }
    };
    auto publish = [&](int t) {
        if constexpr (ORD == 4) {
            asm volatile("" ::: "memory");
            if (lane == 0) flag[wave] = t;
        }
    };
    auto await_neighbours = [&](int t) {
        if constexpr (ORD == 4) {
            const int up = wave > 0 ? wave - 1 : wave, dn = wave + 1 < nwaves ? wave + 1 : wave;
            for (;;) {
                const int a = __builtin_amdgcn_readfirstlane(flag[up]);
                const int b = __builtin_amdgcn_readfirstlane(flag[dn]);
                if (a >= t && b >= t) break;
                __builtin_amdgcn_s_sleep(1);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        }
    };
    // ORD 4's turn: the edge sums F (row 0) and Lr (row SEG-1) go to LDS and are read back
    // from the wave's own slots when needed, instead of staying live across the interior rows
    // and the wait (64 VGPRs at SEG 16: 8 waves per SIMD).  ORD 5: the same turn with ORD 1's
    // workgroup barrier after the puts instead of the flags (80 VGPRs at SEG 24: 6 waves per
    // SIMD, where the stencil's instruction mix issues fastest -- tools/calib/valu_issue.hip
    // occupancy sweep).  ORD 6: the barrier where ORD 4 waits, after the interior rows (ORD
    // 2's placement: a wave that arrives early has done all the work that needs no neighbour;
    // the turn-parity double buffer still needs only the one barrier per turn)
    // ORD 7's wave 0 updates, at turn t, only its rows lo = t + 1 (at most SEG - 2) and above:
    // local rows 0 .. t of both its segments are outside the trapezoid.  The rules of the rows
    // below lo (14 of a row's 22 VALU) and row 0's neighbour read are skipped by wave-uniform
    // scalar branches (the other waves pass lo = 0 and never take one); the row sums stay
    // unconditional -- skipping them too made the sliding window's values conditional, and
    // the compiler paid 4 v_mov per row on every wave's path to merge them.  A skipped row goes
    // stale exactly when the trapezoid makes it junk, and row lo reads only rows lo - 1 ..,
    // which were updated at turn t - 1 (their lo was t).  For every other turn order lo is the
    // constant 0.
    auto turn4 = [&](auto P, int poff, int t, int lo_rt) {
        constexpr int p = decltype(P)::value;
        const int lo = ORD == 7 ? lo_rt : 0;
        const int off = poff;
        uint32_t Pw[NS], Q[NS], S1[NS];
        {
            uint32_t F[NS], Lr[NS];
            tile_rsum<SEG, W>(v[0], F);
            tile_rsum<SEG, W>(v[SEG - 1], Lr);
            put(wtop(p, off), F);
            put(wbot(p, off), Lr);
            if constexpr (ORD == 5 || ORD == 7) __syncthreads();
            else if constexpr (ORD == 4) publish(t);
#pragma unroll
            for (int k = 0; k < NS; ++k) Pw[k] = F[k];
        }
        tile_rsum<SEG, W>(v[1], Q);
#pragma unroll
        for (int k = 0; k < NS; ++k) S1[k] = Q[k];
#pragma unroll
        for (int i = 1; i + 1 < SEG; ++i) {
            uint32_t R[NS];
            if (i + 2 == SEG) get(wbot(p, off), R);   // (own bottom slot: Lr)
            else tile_rsum<SEG, W>(v[i + 1], R);
            if (i >= lo) tile_rule<W>(Pw, Q, R, v[i]);
#pragma unroll
            for (int k = 0; k < NS; ++k) {
                Pw[k] = Q[k];
                Q[k] = R[k];
            }
        }
        // (keep the wait after the interior rows: the compiler would otherwise sink them
        // below the poll loop)
#pragma unroll
        for (int i = 1; i + 1 < SEG; ++i)
#pragma unroll
            for (int d = 0; d < ND; ++d) asm volatile("" : "+v"(v[i][d]));
        if constexpr (ORD == 6) __syncthreads();
        else await_neighbours(t);
        uint32_t U[NS], D[NS], F[NS];
        if (lo == 0) {
            get(rup(p, off), U);
            get(wtop(p, off), F);
            tile_rule<W>(U, F, S1, v[0]);
        }
        get(rdn(p, off), D);
        get(wbot(p, off), F);                                 // (Lr)
        tile_rule<W>(Pw, F, D, v[SEG - 1]);
    };
    // ORD 5's turn under the register plan (tile_parity_pins, above): the same instructions in
    // the same order as turn4, the rows indexed at compile time so that each value can name
    // its register.  The bottom-edge array holds its sums in the order 1, 0, 3, 2 (swz).
    [[maybe_unused]] auto turn4p = [&](auto P, int poff) {
        if constexpr (kPins) {
            constexpr int p = decltype(P)::value;
            const int off = poff;
            auto swz = [](uint32_t (&S)[NS]) {
                const uint32_t s0 = S[0], s2 = S[2];
                S[0] = S[1];
                S[1] = s0;
                S[2] = S[3];
                S[3] = s2;
            };
            auto rsum_p = [&](auto J, uint32_t (&S)[NS]) {
                constexpr int j = decltype(J)::value;
                tile_rsum<SEG, W>(v[j], S);
                vpin<tile_pin_sum(SEG, j, 0)>(S[0]);
                vpin<tile_pin_sum(SEG, j, 1)>(S[1]);
                vpin<tile_pin_sum(SEG, j, 2)>(S[2]);
                vpin<tile_pin_sum(SEG, j, 3)>(S[3]);
            };
            auto rule_d = [&](auto I, auto Dw, const uint32_t (&A)[NS], const uint32_t (&B)[NS],
                              const uint32_t (&Cs)[NS]) {
                constexpr int i = decltype(I)::value, d = decltype(Dw)::value;
                // the donor: the row whose sums die in this rule (the plan's comment, above)
                constexpr int jd = i == 0 ? 1 : i - 1;
                constexpr int r0 = tile_pin_sum(SEG, jd, 2 * d), r1 = tile_pin_sum(SEG, jd, 2 * d + 1);
                constexpr int rt = tile_pin_tmp(SEG, d, 0);
                const uint32_t Cc = v[i][d];
                const uint32_t lm = maj(A[2 * d], B[2 * d], Cs[2 * d]);
                uint32_t lx = bitop3<0x7e>(A[2 * d], B[2 * d], Cs[2 * d]);
                uint32_t hm, hx;
                if constexpr (i == 2) {
                    // (row 1's sums stay live for row 0's rule: no donor; hx takes the cell's own
                    // register, free once g2 has read the centre)
                    vpin<rt>(lx);
                    hm = maj(A[2 * d + 1], B[2 * d + 1], Cs[2 * d + 1]);
                    vpin<tile_pin_tmp(SEG, d, 1)>(hm);
                    const uint32_t g1 = bitop3<0x16>(lm, lx, Cc);
                    const uint32_t g2 = bitop3<0x86>(hm, Cc, g1);
                    hx = xor3(A[2 * d + 1], B[2 * d + 1], Cs[2 * d + 1]);
                    vpin<tile_pin_cell(i, d)>(hx);
                    uint32_t n = bitop3<0x82>(lx, hx, g2);
                    vpin<tile_pin_cell(i, d)>(n);
                    return n;
                } else if constexpr ((r1 & 1) == d) {
                    vpin<r0>(lx);
                    hm = maj(A[2 * d + 1], B[2 * d + 1], Cs[2 * d + 1]);
                    vpin<rt>(hm);
                    hx = xor3(A[2 * d + 1], B[2 * d + 1], Cs[2 * d + 1]);
                    vpin<r1>(hx);
                } else {
                    vpin<rt>(lx);
                    hx = xor3(A[2 * d + 1], B[2 * d + 1], Cs[2 * d + 1]);
                    vpin<r0>(hx);
                    hm = maj(A[2 * d + 1], B[2 * d + 1], Cs[2 * d + 1]);
                    vpin<r1>(hm);
                }
                const uint32_t g1 = bitop3<0x16>(lm, lx, Cc);
                const uint32_t g2 = bitop3<0x86>(hm, Cc, g1);
                uint32_t n = bitop3<0x82>(lx, hx, g2);       // (life_rule7)
                vpin<tile_pin_cell(i, d)>(n);
                return n;
            };
            auto rule_p = [&](auto I, const uint32_t (&A)[NS], const uint32_t (&B)[NS],
                              const uint32_t (&Cs)[NS]) {
                constexpr int i = decltype(I)::value;
                const uint32_t n0 = rule_d(I, std::integral_constant<int, 0>{}, A, B, Cs);
                const uint32_t n1 = rule_d(I, std::integral_constant<int, 1>{}, A, B, Cs);
                v[i][0] = n0;
                v[i][1] = n1;
            };
            uint32_t Pw[NS], Q[NS], S1[NS];
            {
                uint32_t F[NS], Lr[NS];
                rsum_p(std::integral_constant<int, 0>{}, F);
                rsum_p(std::integral_constant<int, SEG - 1>{}, Lr);
                put(wtop(p, off), F);
                swz(Lr);
                put(wbot(p, off), Lr);
                __syncthreads();
#pragma unroll
                for (int k = 0; k < NS; ++k) Pw[k] = F[k];
            }
            rsum_p(std::integral_constant<int, 1>{}, Q);
#pragma unroll
            for (int k = 0; k < NS; ++k) S1[k] = Q[k];
            unroll_seq(std::make_integer_sequence<int, SEG - 2>{}, [&](auto I0) {
                constexpr int i = decltype(I0)::value + 1;
                uint32_t R[NS];
                if constexpr (i + 2 == SEG) {
                    get(wbot(p, off), R);                    // (own bottom slot: Lr)
                    swz(R);
                } else {
                    rsum_p(std::integral_constant<int, i + 1>{}, R);
                }
                rule_p(std::integral_constant<int, i>{}, Pw, Q, R);
#pragma unroll
                for (int k = 0; k < NS; ++k) {
                    Pw[k] = Q[k];
                    Q[k] = R[k];
                }
            });
#pragma unroll
            for (int i = 1; i + 1 < SEG; ++i)
#pragma unroll
                for (int d = 0; d < ND; ++d) asm volatile("" : "+v"(v[i][d]));
            uint32_t U[NS], D[NS], F[NS];
            get(rup(p, off), U);
            swz(U);
            get(wtop(p, off), F);
            rule_p(std::integral_constant<int, 0>{}, U, F, S1);
            get(rdn(p, off), D);
            get(wbot(p, off), F);                            // (Lr)
            swz(F);
            rule_p(std::integral_constant<int, SEG - 1>{}, Pw, F, D);
        }
    };
    // DUO: turn4 with the interior rows in pairs.  A, B: the sums of the row above the pair and
    // of its first row; per pair the sums of its second row and of the row below it are formed
    // (the last pair's: read back from the own bottom slot), then the pair goes dword by dword --
    // dword d needs only the sums 2d and 2d + 1, so one dword's P and temporaries are live at a
    // time.
    [[maybe_unused]] auto turn4d = [&](auto P, int poff) {
        if constexpr (DUO) {
            constexpr int p = decltype(P)::value;
            const int off = poff;
            uint32_t A[NS], B[NS], S1[NS];
            {
                uint32_t F[NS], Lr[NS];
                tile_rsum<SEG, W>(v[0], F);
                tile_rsum<SEG, W>(v[SEG - 1], Lr);
                put(wtop(p, off), F);
                put(wbot(p, off), Lr);
                __syncthreads();
#pragma unroll
                for (int k = 0; k < NS; ++k) A[k] = F[k];
            }
            tile_rsum<SEG, W>(v[1], B);
#pragma unroll
            for (int k = 0; k < NS; ++k) S1[k] = B[k];
#pragma unroll
            for (int i = 1; i + 1 < SEG; i += 2) {
                uint32_t Cs[NS], Dn[NS];
                tile_rsum<SEG, W>(v[i + 1], Cs);
                if (i + 3 == SEG) get(wbot(p, off), Dn);   // (own bottom slot: Lr)
                else tile_rsum<SEG, W>(v[i + 2], Dn);
#pragma unroll
                for (int d = 0; d < ND; ++d) {
                    uint32_t p0, p1, p2;
                    life_pair_sum(B[2 * d], Cs[2 * d], B[2 * d + 1], Cs[2 * d + 1], p0, p1, p2);
                    const uint32_t n0 = life_rule_pair(A[2 * d], A[2 * d + 1], p0, p1, p2, v[i][d]);
                    const uint32_t n1 =
                        life_rule_pair(Dn[2 * d], Dn[2 * d + 1], p0, p1, p2, v[i + 1][d]);
                    v[i][d] = n0;
                    v[i + 1][d] = n1;
                }
#pragma unroll
                for (int k = 0; k < NS; ++k) {
                    A[k] = Cs[k];
                    B[k] = Dn[k];
                }
            }
            // (A: the sums of row SEG - 2)
#pragma unroll
            for (int i = 1; i + 1 < SEG; ++i)
#pragma unroll
                for (int d = 0; d < ND; ++d) asm volatile("" : "+v"(v[i][d]));
            uint32_t U[NS], D[NS], F[NS];
            get(rup(p, off), U);
            get(wtop(p, off), F);
            tile_rule<W>(U, F, S1, v[0]);
            get(rdn(p, off), D);
            get(wbot(p, off), F);                            // (Lr)
            tile_rule<W>(A, F, D, v[SEG - 1]);
        }
    };
    auto turn = [&](auto P, int poff, int t) {
        if constexpr (DUO) {
            turn4d(P, poff);
            return;
        }
        if constexpr (kPins) {
            turn4p(P, poff);
            return;
        }
        if constexpr (ORD >= 4) {
            turn4(P, poff, t, kHalo && wave == 0 ? min(t + 1, SEG - 2) : 0);
            return;
        }
        constexpr int p = decltype(P)::value;
        const int off = poff;
        // the segment's first and last row sums go to the neighbours (row sums, not rows: no
        // lane sums a row twice -- SEG row sums and SEG rules per turn); kEdgeRows: the rows
        uint32_t F[NS], Lr[NS];
        tile_rsum<SEG, W>(v[0], F);
        tile_rsum<SEG, W>(v[SEG - 1], Lr);
        if constexpr (kEdgeRows) {
            tile_lab_put_rows<SEG>(wtop(p, off), v);
        } else {
            put(wtop(p, off), F);
            put(wbot(p, off), Lr);
        }
        uint32_t U[NS], D[NS];
        // (kEdgeRows: the neighbours' rows come back and are summed here)
        auto get_rows = [&](uint32_t (&Us)[NS], uint32_t (&Ds)[NS]) {
            tile_lab_get_rows<SEG, W>(kPairs ? xsh + 2 * nslot * p : xsh + off, s_up, s_dn, Us, Ds);
        };
        if constexpr (ORD < 2 || ORD == 3) {
            if constexpr (ORD != 3) __syncthreads();   // ORD 3: timing ablation (tools build)
            if constexpr (kEdgeRows) {
                get_rows(U, D);
            } else {
                get(rup(p, off), U);
                get(rdn(p, off), D);
            }
        }
        if constexpr (ORD == 0 || ORD == 3) {
            // in order: A, B, Cs = sums of rows i-1, i, i+1
            uint32_t A[NS], B[NS];
#pragma unroll
            for (int k = 0; k < NS; ++k) {
                A[k] = U[k];
                B[k] = F[k];
            }
#pragma unroll
            for (int i = 0; i < SEG; ++i) {
                uint32_t Cs[NS];
                if (i + 1 == SEG) {
#pragma unroll
                    for (int k = 0; k < NS; ++k) Cs[k] = D[k];
                } else if (i + 2 == SEG) {
#pragma unroll
                    for (int k = 0; k < NS; ++k) Cs[k] = Lr[k];
                } else {
                    tile_rsum<SEG, W>(v[i + 1], Cs);
                }
                tile_rule<W>(A, B, Cs, v[i]);
#pragma unroll
                for (int k = 0; k < NS; ++k) {
                    A[k] = B[k];
                    B[k] = Cs[k];
                }
            }
        } else {
            // ORD 1: interior rows 1 .. SEG-2 first (their sums are all local), so the LDS
            // reads land while they compute; window P, Q, R = sums of rows i-1, i, i+1
            uint32_t Pw[NS], Q[NS], S1[NS];
#pragma unroll
            for (int k = 0; k < NS; ++k) Pw[k] = F[k];
            if constexpr (SEG >= 3) {
                tile_rsum<SEG, W>(v[1], Q);
#pragma unroll
                for (int k = 0; k < NS; ++k) S1[k] = Q[k];
            } else {
#pragma unroll
                for (int k = 0; k < NS; ++k) S1[k] = Q[k] = Lr[k];
            }
#pragma unroll
            for (int i = 1; i + 1 < SEG; ++i) {
                uint32_t R[NS];
                if (i + 2 == SEG) {
#pragma unroll
                    for (int k = 0; k < NS; ++k) R[k] = Lr[k];
                } else {
                    tile_rsum<SEG, W>(v[i + 1], R);
                }
                tile_rule<W>(Pw, Q, R, v[i]);
#pragma unroll
                for (int k = 0; k < NS; ++k) {
                    Pw[k] = Q[k];
                    Q[k] = R[k];
                }
            }
            // (Pw = the sums of row SEG-2, or of row 0 when SEG == 2)
            if constexpr (ORD == 2) {
                // ORD 2: the barrier after the interior rows -- a wave that arrives early has
                // already done all the work that needs no neighbour
                __syncthreads();
                if constexpr (kEdgeRows) {
                    get_rows(U, D);
                } else {
                    get(rup(p, off), U);
                    get(rdn(p, off), D);
                }
            }
            tile_rule<W>(U, F, S1, v[0]);
            tile_rule<W>(Pw, Lr, D, v[SEG - 1]);
        }
    };
    // (the plan's cell registers from the first turn on: loop-carried values tied to one
    // register at the loop's head and at their redefinition need no copy)
    if constexpr (kPins) {
        unroll_seq(std::make_integer_sequence<int, SEG>{}, [&](auto I) {
            constexpr int i = decltype(I)::value;
            vpin<tile_pin_cell(i, 0)>(v[i][0]);
            vpin<tile_pin_cell(i, 1)>(v[i][1]);
        });
    }
    const int lastrow = 2 * K + TH - 1;
    // a wave leaving the trapezoid at turn t: its rows are all < K or >= K + TH, so it has
    // nothing to store.  It ends (the barrier stops counting it; ORD 4: its flag says it has
    // gone).  Persistent passes keep every wave to the end of the pass.
    auto leave = [&](int t) {
        if constexpr (ORD == 4) {
            if (lane == 0) flag[wave] = 0x7fffffff;
        }
    };
    bool gone = false;
    if constexpr (Lab::kBlocks) {
        // (gol_tile_lab.h: K1r -- the tile stays in registers over blocks of turns)
        static_assert(PERSIST && W == 1, "a block loop: a persistent pass, one word per lane");
        lab.template blocks<SEG, ORD, kPairs, kLoadAux>(
            TileView<SEG, ND>{v, a, pos, xsh, rout, TW, C, G, K, TH, nl, y0, x0, lane, wave, nslot, myslot,
                              s_up, s_dn, wrow0, wrow1, lastrow, pitch_b, span, off_first},
            turn);
    } else if constexpr (ORD == 8 || ORD == 9) {
        // (gol_tile_lab.h: the turn in inline asm, with a loop and a store of its own)
        tile_lab_asm_loop<SEG, ORD>(TileView<SEG, ND>{v, a, pos, xsh, rout, TW, C, G, K, TH, nl, y0, x0,
                                                      lane, wave, nslot, myslot, s_up, s_dn, wrow0,
                                                      wrow1, lastrow, pitch_b, span, off_first});
        return;
    } else if constexpr (kHalo) {
        static_assert(!kPairs, "ORD 7: long segments");
        for (int t = 0; t < K; ++t) {
            // (wave 0 spans the whole tile and never leaves: wrow1 is out of reach)
            if (!PERSIST && (wrow1 <= t || wrow0 > lastrow - t)) {   // (wave-uniform)
                leave(t);
                gone = true;
                break;
            }
            turn(std::integral_constant<int, 0>{}, (t & 1) * 2 * nslot, t);
        }
    } else if constexpr (!kPairs) {
        // (the second leave test as one scalar, formed once: t > lastrow - wrow0)
        const int tlast = __builtin_amdgcn_readfirstlane(lastrow - wrow0);
        for (int t = 0; t < K; ++t) {
            if (!PERSIST && (wrow1 <= t || t > tlast)) {         // (wave-uniform)
                leave(t);
                gone = true;
                break;
            }
            turn(std::integral_constant<int, 0>{}, (t & 1) * 2 * nslot, t);
            count_turn(t);
        }
    } else {
        for (int t = 0; t < K; t += 2) {
            if (!PERSIST && (wrow1 <= t || wrow0 > lastrow - t)) {
                leave(t);
                gone = true;
                break;
            }
            turn(std::integral_constant<int, 0>{}, 0, t);
            count_turn(t);
            if (t + 1 == K) break;
            if (!PERSIST && (wrow1 <= t + 1 || wrow0 > lastrow - t - 1)) {
                leave(t + 1);
                gone = true;
                break;
            }
            turn(std::integral_constant<int, 1>{}, 0, t + 1);
            count_turn(t + 1);
        }
    }
    if (!PERSIST && gone) return;
    if constexpr (CNT) {
        // the waves still here (a wave that left has ended: the barrier does not count it);
        // wave cw_lo never leaves.  Its lane t adds turn t + 1's sums of the counting waves
        __syncthreads();
        uint32_t all = ~0u;
        asm volatile("" : "+v"(all));
        const int ln = (int)__builtin_amdgcn_mbcnt_hi(all, __builtin_amdgcn_mbcnt_lo(all, 0u));
        if (wave == cw_lo && ln < K) {
            uint32_t s = 0;
            for (int w = cw_lo; w <= cw_hi; ++w) s += csum[ln * kTileMaxWaves + w];
            if (s)
                atomicAdd(a.counts + (size_t)ln * kShards + (blockIdx.x & (kShards - 1)),
                          (unsigned long long)s);
        }
    }
    // interior rows [K, K + TH) of the tile, below row_hi; interior columns inside the row
    if (gone) return;
    auto store_row = [&](int i, uint32_t voff, uint32_t soff) {
        if constexpr (W == 1 && GOL_TILE_STORE_AUX != 0) {
            const u32x2 d = {v[i][0], v[i][1]};
            __builtin_amdgcn_raw_buffer_store_b64(d, rout, voff, soff, GOL_TILE_STORE_AUX);
        } else {
            buf_store(v[i], rout, voff, soff);
        }
    };
    if constexpr (!kHalo) {
        // the lane's stored local rows [lo, hi): tile rows [K, K + TH) below row_hi
        // (the lane's column and segment formed again here, from the lane count of an opaque
        // mask: nothing of the store stage stays live across the turns -- 2 VGPRs less)
        uint32_t all = ~0u;
        asm volatile("" : "+v"(all));
        const int sl = (int)__builtin_amdgcn_mbcnt_hi(all, __builtin_amdgcn_mbcnt_lo(all, 0u));
        const int sg = (int)(((uint32_t)sl * pos.rcp) >> 16), sc = sl - sg * C;
        const bool scol = sg < G && sc >= 1 && sc <= TW && x0 + sc - 1 < nl;
        const int t0 = (wave * G + sg) * SEG;
        const int top = min(K + TH, a.row_hi - (y0 - K));    // (wave-uniform)
        const int lo = min(max(K - t0, 0), SEG), hi = min(max(top - t0, 0), SEG);
        // BIG: rout starts at row y0, so the lane's first row is t0 - K rows from it.  A lane
        // whose segment starts above the stored rows (t0 < K, also where y0 - K < 0) holds that
        // negative count times the pitch modulo 2^32; it steps by one pitch per row in the
        // lane's register and is exact from the first stored row on: (t0 + i - K) pitch + the
        // column, below the stored rows' bytes and so below 2^31.  A lane that stores its whole
        // segment under the scalar step has t0 >= K: its offset is a stored row's, in range.
        uint32_t so = (uint32_t)(BIG ? t0 - K : y0 - K + t0) * pitch_b + (uint32_t)(x0 + sc - 1) * (8u * W);
        // SEAM: the tile that holds column L (wave-uniform) clears that lane's bits r .. 63 --
        // the wrapped cells it carried through the turns -- so the padding stays zero
        if constexpr (SEAM) {
            const int L = nl - 1;
            if (x0 <= L && x0 + TW > L) {
                const int rb = a.width & 63;                 // (1 .. 63: a seam launch)
                const bool lastc = x0 + sc - 1 == L;
                const uint32_t me = lastc ? ~0u >> (32 - ((rb + 1) >> 1)) : ~0u;
                const uint32_t mo = lastc ? (1u << (rb >> 1)) - 1u : ~0u;
#pragma unroll
                for (int i = 0; i < SEG; ++i) {
                    v[i][0] &= me;
                    v[i][1] &= mo;
                }
            }
        }
        // Every storing lane of the wave stores its whole segment (one ballot; every wave but
        // the tile's first and last, and the board's last tile row): all SEG rows under one
        // exec mask, stepped by the instruction's scalar offset.  The lane's offset is that of
        // a stored row, inside the buffer (the range check sees it without the scalar part).
        if (__builtin_amdgcn_ballot_w64(scol && (lo > 0 || hi < SEG)) == 0) {
            if (scol) {
#pragma unroll
                for (int i = 0; i < SEG; ++i) store_row(i, so, (uint32_t)i * pitch_b);
            }
            return;
        }
        // a wave at the tile's edge: a row range per lane (the offset may start above row 0
        // and is exact once inside the stored rows, so it steps in the lane's register)
        if (!scol || hi <= lo) return;
#pragma unroll
        for (int i = 0; i < SEG; ++i) {
            if (i >= lo && i < hi) store_row(i, so, 0);
            so += pitch_b;
        }
        return;
    }
    if (!live || col < 1 || col > TW || x0 + col - 1 >= nl) return;
    const int t0 = seg * SEG + (rev ? SEG - 1 : 0);
    const int dr = rev ? -1 : 1;
    const uint32_t sstep = rev ? 0u - pitch_b : pitch_b;
    // per-lane byte offset (the segment differs between the lane groups of a wave); rows
    // y0 - K + t0 + i are stored only once inside [row_lo, row_hi): no wrap, and the
    // unsigned sum is exact there even if the first row of the segment lies above row 0
    uint32_t so = (uint32_t)(y0 - K + t0) * pitch_b + (uint32_t)(x0 + col - 1) * (8u * W);
#pragma unroll
    for (int i = 0; i < SEG; ++i) {
        const int tr = t0 + dr * i;
        if (tr >= K && tr < K + TH && y0 - K + tr < a.row_hi) {
            if constexpr (W == 1 && GOL_TILE_STORE_AUX != 0)
                buf_store_aux<GOL_TILE_STORE_AUX>(v[i], rout, so);
            else
                buf_store(v[i], rout, so, 0);
        }
        so += sstep;
    }
}

// XCD-aware tile order: blockIdx b runs on XCD b % 8, which gets a contiguous run of tiles
// (whole tile rows, so most halo rows were written by the same XCD's L2)
__device__ __forceinline__ int tile_of_block(int ntiles)
{
    const int per = (ntiles + 7) / 8;
    return (int)(blockIdx.x % 8) * per + (int)(blockIdx.x / 8);
}

// (ORD 4 up to SEG 16: 64 VGPRs, 8 waves per SIMD -- two 16-wave workgroups per CU)
template <int SEG, int ORD, int W>
__global__ __launch_bounds__(1024, (ORD == 7 ? 6 : 1)) void k_step_tile(const uint64_t *__restrict__ in,
                                                     uint64_t *__restrict__ out, StepArgs a,
                                                     int turns, TileLaunch L)
{
    const int tile = tile_of_block(L.ntiles);
    if (tile >= L.ntiles) return;                        // the whole workgroup
    tile_pass<SEG, ORD, W, false>(in, out, a, turns, tile_pos(a, L, tile));
}

// k_step_tile across the row seam (tile_pass SEAM; the instantiations: golk::kTileSeamCodes,
// gol_tile_seam.hip).  Its own entry point: the kernels of whole-word boards stay as they are.
// (the waves per SIMD of the plain kernel of the same code are asked for: left to itself the
// compiler takes 65 VGPRs at SEG 16 and 81 at SEG 24 for the load stage's sake, one register
// past 8 and 6 waves; held to the bound it spills one 64-bit value once, before the first turn)
template <int SEG, int ORD>
__global__ __launch_bounds__(1024, (SEG <= 16 ? 8 : 6)) void k_step_tile_seam(const uint64_t *__restrict__ in,
                                                            uint64_t *__restrict__ out, StepArgs a,
                                                            int turns, TileLaunch L)
{
    const int tile = tile_of_block(L.ntiles);
    if (tile >= L.ntiles) return;                        // the whole workgroup
    tile_pass<SEG, ORD, 1, false, false, true>(in, out, a, turns, tile_pos(a, L, tile));
}

// k_step_tile on a buffer of 2 GiB or more (tile_pass BIG; the instantiations:
// golk::kTileBigCodes, gol_tile_big.hip).  Its own entry point: the other kernels stay as they
// are.  The waves per SIMD of the plain kernel of the same code are asked for, as for the seam
// form (8 up to SEG 16, 6 at SEG 24: DESIGN.md "K1t on boards of 2 GiB and more" has both tables;
// no big kernel spills).
template <int SEG, int ORD>
__global__ __launch_bounds__(1024, (SEG <= 16 ? 8 : 6)) void k_step_tile_big(
    const uint64_t *__restrict__ in, uint64_t *__restrict__ out, StepArgs a, int turns, TileLaunch L)
{
    const int tile = tile_of_block(L.ntiles);
    if (tile >= L.ntiles) return;                        // the whole workgroup
    tile_pass<SEG, ORD, 1, false, false, false, true>(in, out, a, turns, tile_pos(a, L, tile));
}

// k_step_tile with the interior rows ruled in pairs (tile_pass DUO; the instantiations:
// gol_tile_duo.hip).  Its own entry point: the other kernels stay as they are.  The plain
// kernel's grid, LDS bytes, TileLaunch and launch bounds.
template <int SEG, int ORD, int W>
__global__ __launch_bounds__(1024, 1) void k_step_tile_duo(const uint64_t *__restrict__ in,
                                                           uint64_t *__restrict__ out, StepArgs a,
                                                           int turns, TileLaunch L)
{
    const int tile = tile_of_block(L.ntiles);
    if (tile >= L.ntiles) return;                        // the whole workgroup
    tile_pass<SEG, ORD, W, false, false, false, false, true>(in, out, a, turns,
                                                                    tile_pos(a, L, tile));
}

// k_step_tile with the per-turn alive counts fused (tile_pass CNT; the instantiations:
// golk::kTileCountCodes).  Its own entry point: the uncounted kernels stay as they are.
template <int SEG, int ORD, int W>
__global__ __launch_bounds__(1024, 1) void k_step_tile_cnt(const uint64_t *__restrict__ in,
                                                           uint64_t *__restrict__ out, StepArgs a,
                                                           int turns, TileLaunch L)
{
    const int tile = tile_of_block(L.ntiles);
    if (tile >= L.ntiles) return;                        // the whole workgroup
    tile_pass<SEG, ORD, W, false, true>(in, out, a, turns, tile_pos(a, L, tile));
}
}  // namespace golk

// (the tools build and the A/B builds of the tile unit: the experiments' kernels)
#if GOL_TILE_LAB
#include "gol_tile_lab.h"
#endif
