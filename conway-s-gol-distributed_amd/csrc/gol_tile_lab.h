// gol_tile_lab.h -- K1t experiments that lost: kernels that exist only in the tools build
// (GOL_TOOLS) and in the tile unit's A/B builds make variant VDEFS=-DGOL_TILE_PAIR=1 and
// -DGOL_TILE_RAW=n.  No product library holds any of them.  Included by gol_tile.h, at its end, in
// a unit that defines GOL_TILE_LAB before it (gol_tile.hip does, in those builds):
//   * ORD 3 under GOL_TILE_PAIR: two tiles per workgroup -- tile_pass_pair, k_step_tile_pair;
//   * K1p / K1q: resident and streamed blocks of tile_pass -- k_tile_persist, k_tile_stream;
//   * K1r: the tile stays in registers across blocks of turns -- TileRingLab, k_tile_ring;
//   * ORD 8 / 9: the turn in inline asm (gol_tile_turn.h), with its own loop and store --
//     tile_lab_asm_loop;
//   * raw edge rows (GOL_TILE_RAW) -- tile_lab_put_rows / tile_lab_get_rows.
// The last three run inside tile_pass, which calls them at its lab spots with a TileView of its
// locals.  (ORD 3's no-barrier form and ORD 7 are if-constexpr spots of gol_tile.h itself.)
#pragma once
#if GOL_TOOLS
#include "gol_tile_turn.h"   // (ORD 8 / 9's generated inline-asm turns: tools build only)
#else
namespace golk {
// (declared only: ORD 8 / 9 are instantiated in the tools build alone)
template <int SEG, int V>
__device__ __forceinline__ void tile_turn_asm(uint32_t (&v)[SEG][2], uint32_t (&ad)[4], uint32_t ps,
                                              uint32_t ba);
}  // namespace golk
#endif

// K1t ORD 8 / 9 (the turn in inline asm, gol_tile_turn.h): bit 1 = the workgroup barrier after
// rows 1 and 2 instead of right after the edge sums' stores, bit 2 = LDS slots 16 B apart
// instead of 64 (A/B builds: make variant VDEFS=-DGOL_TURN_VAR=n)
#ifndef GOL_TURN_VAR
#define GOL_TURN_VAR 4
#endif
// Raw edge rows (ORD 0-2, one word per lane, segments of up to GOL_TILE_RAW rows; 0 = never):
// each lane publishes its first and last row as they are -- one 16-B LDS slot, one
// ds_write_b128 -- instead of their two 3-cell row sums (two slots, two ds_write_b128), and
// sums the rows it reads from the segments above and below itself (two more row sums a turn).
// Half the LDS bytes per turn for 8 more VALU per neighbour row: the trade pays where a turn's
// LDS stores, not its VALU, are the critical path -- short segments on small boards.
#ifndef GOL_TILE_RAW
#define GOL_TILE_RAW 0
#endif
// ORD 3 = two tiles per workgroup, software-pipelined (tile_pass_pair below; A/B builds:
// make variant VDEFS=-DGOL_TILE_PAIR=1).  Without it ORD 3 is the tools build's no-barrier timing
// ablation.
#ifndef GOL_TILE_PAIR
#define GOL_TILE_PAIR 0
#endif
// (K1p / K1q / K1r, tools build: polls of a neighbour tile's flag before a wait gives up)
#ifndef GOL_TILE_SPIN_LIMIT
#define GOL_TILE_SPIN_LIMIT (1 << 22)
#endif

namespace golk {

// ORD 8 / 9 with the 16-B slot layout: the slot count rounded up to a power of two (the turn
// parity is an XOR of the addresses)
constexpr int tile_slots_pow2(int threads)
{
    int n = 64;
    while (n < threads) n *= 2;
    return n;
}
constexpr size_t tile_lds_bytes_code(int threads, int code)
{
    const int ord = code / 100 % 10;
    return (ord == 8 || ord == 9) && (GOL_TURN_VAR & 4)
               ? tile_lds_bytes(tile_slots_pow2(threads), 1)
           : ord == 3 && GOL_TILE_PAIR ? 2 * tile_lds_bytes(threads, 1)   // (two tiles' slots)
                                       : tile_lds_bytes(threads, tile_seg_words(code));
}

// tile `tile` of the rectangular grid of ntx columns (the resident kernels)
__device__ __forceinline__ TilePos tile_pos_rect(const StepArgs &a, int tile, int ntx)
{
    const int ty = tile / ntx, tx = tile - ty * ntx;
    const int c = a.tile_w + 2;
    return TilePos{a.tile_w, a.band, tx * a.tile_w, a.row_lo + ty * a.band, 64 / c, tile_rcp16(c)};
}

// ORD 3 (round 6): two tiles per workgroup, software-pipelined (the round-5 verdict's ask for
// small boards, whose turn is a serial chain: one barrier, the LDS round trip of the edge sums,
// the edge rules, the next turn's row sums and stores, then the barrier again -- the waves of a
// workgroup all reach each phase together, so the VALU idles while the LDS works and back).
// Every lane holds one SEG-row segment of tile A and one of tile B (the same local rows of two
// tiles), and each turn is split in two halves:
//   H1(X) -- the row sums of the segment's first and last rows, their stores to LDS, and the
//            interior rows (everything that needs no neighbour);
//   H2(X) -- the neighbours' edge sums read back and the first and last rows' rules.
// Between two workgroup barriers a lane runs H2 of one tile beside H1 of the other, so one
// tile's LDS reads are in flight while the other tile's VALU work issues:
//   H1(A, 0) | H2(A, t), H1(B, t) | H2(B, t), H1(A, t + 1) | ...
// Two barriers per turn for two tiles: one per tile-turn, as for one tile.  The edge sums stay
// double-buffered by turn parity per tile ([tile][parity][top, bottom][slot]).  One word per
// lane; segments of 2..8 rows.
template <int SEG>
__device__ __forceinline__ void tile_pass_pair(const uint64_t *__restrict__ in,
                                               uint64_t *__restrict__ out, const StepArgs &a,
                                               int turns, int tileA, int tileB, bool storeB,
                                               int ntx)
{
    constexpr int ND = 2, NS = 4;
    static_assert(SEG >= 2 && SEG <= 8, "ORD 3: short segments");
    extern __shared__ uint4 xsh[];
    const int nslot = (int)blockDim.x;
    const int TW = a.tile_w, C = TW + 2, G = 64 / C;
    const int K = turns, TH = a.band;
    const int nl = a.nw;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int group = lane / C, col = lane - group * C;
    const bool live = group < G;
    const int nseg = (TH + 2 * K + SEG - 1) / SEG;
    const int seg = wave * G + group;
    const int slot = seg * C + col;
    const int M = a.modrows;
    const uint32_t pitch_b = (uint32_t)a.pitch * 8u;
    const uint32_t span = (uint32_t)M * pitch_b;
    const __amdgpu_buffer_rsrc_t rin =
        __builtin_amdgcn_make_buffer_rsrc((void *)in, (short)0, (int)span, kBufFlags);
    const __amdgpu_buffer_rsrc_t rout =
        __builtin_amdgcn_make_buffer_rsrc((void *)out, (short)0, (int)span, kBufFlags);
    const int tiles[2] = {tileA, tileB};
    uint32_t v[2][SEG][ND];
    int y0s[2], x0s[2];
#pragma unroll
    for (int X = 0; X < 2; ++X) {
        const int ty = tiles[X] / ntx, tx = tiles[X] - ty * ntx;
        y0s[X] = a.row_lo + ty * TH;
        x0s[X] = tx * TW;
        int gx = x0s[X] - 1 + (live ? col : 0);
        while (gx < 0) gx += nl;
        while (gx >= nl) gx -= nl;
        int r = y0s[X] - K + (live ? seg : 0) * SEG;
        while (r < 0) r += M;
        while (r >= M) r -= M;
        uint32_t off = (uint32_t)r * pitch_b + (uint32_t)gx * 8u;
#pragma unroll
        for (int i = 0; i < SEG; ++i) {
            const u32x2 w = __builtin_amdgcn_raw_buffer_load_b64(rin, off, 0, 0);
            v[X][i][0] = w.x;
            v[X][i][1] = w.y;
            off += pitch_b;
            off = off >= span ? off - span : off;
        }
    }
    auto put = [&](uint4 *p, const uint32_t (&S)[NS]) { *p = make_uint4(S[0], S[1], S[2], S[3]); };
    auto get = [&](const uint4 *p, uint32_t (&S)[NS]) {
        const uint4 u = *p;
        S[0] = u.x;
        S[1] = u.y;
        S[2] = u.z;
        S[3] = u.w;
    };
    // slots as in tile_pass: idle lanes own the slots past the tile's, a segment with no
    // neighbour reads its own (junk that reaches only the tile's outermost row)
    const int nlive = (int)(blockDim.x >> 6) * G * C;
    const int myslot = live ? slot : nlive + wave * (64 - G * C) + (lane - G * C);
    const int s_up = live && seg > 0 ? slot - C : myslot;
    const int s_dn = live && seg + 1 < nseg ? slot + C : myslot;
    // [tile X][parity p][top 0 / bottom 1][slot]
    auto at = [&](int X, int p, int bt, int sl) { return xsh + ((X * 2 + p) * 2 + bt) * nslot + sl; };
    uint32_t F[2][NS], Lr[2][NS], S1[2][NS], Pl[2][NS];
    auto h1 = [&](auto XX, auto PP) {
        constexpr int X = decltype(XX)::value, p = decltype(PP)::value;
        tile_rsum<SEG, 1>(v[X][0], F[X]);
        tile_rsum<SEG, 1>(v[X][SEG - 1], Lr[X]);
        put(at(X, p, 0, myslot), F[X]);
        put(at(X, p, 1, myslot), Lr[X]);
        uint32_t Pw[NS], Q[NS];
#pragma unroll
        for (int k = 0; k < NS; ++k) Pw[k] = F[X][k];
        if constexpr (SEG >= 3) {
            tile_rsum<SEG, 1>(v[X][1], Q);
        } else {
#pragma unroll
            for (int k = 0; k < NS; ++k) Q[k] = Lr[X][k];
        }
#pragma unroll
        for (int k = 0; k < NS; ++k) S1[X][k] = Q[k];
#pragma unroll
        for (int i = 1; i + 1 < SEG; ++i) {
            uint32_t R[NS];
            if (i + 2 == SEG) {
#pragma unroll
                for (int k = 0; k < NS; ++k) R[k] = Lr[X][k];
            } else {
                tile_rsum<SEG, 1>(v[X][i + 1], R);
            }
            tile_rule<1>(Pw, Q, R, v[X][i]);
#pragma unroll
            for (int k = 0; k < NS; ++k) {
                Pw[k] = Q[k];
                Q[k] = R[k];
            }
        }
#pragma unroll
        for (int k = 0; k < NS; ++k) Pl[X][k] = Pw[k];   // sums of row SEG-2 (row 0 at SEG 2)
    };
    auto h2 = [&](auto XX, auto PP) {
        constexpr int X = decltype(XX)::value, p = decltype(PP)::value;
        uint32_t U[NS], D[NS];
        get(at(X, p, 1, s_up), U);
        get(at(X, p, 0, s_dn), D);
        tile_rule<1>(U, F[X], S1[X], v[X][0]);
        tile_rule<1>(Pl[X], Lr[X], D, v[X][SEG - 1]);
    };
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    const int lastrow = 2 * K + TH - 1;
    const int wrow0 = wave * G * SEG, wrow1 = wrow0 + G * SEG;
    auto leaves = [&](int t) { return wrow1 <= t || wrow0 > lastrow - t; };   // (wave-uniform)
    h1(I0{}, I0{});
    __syncthreads();
    bool gone = false;
    for (int t = 0; t < K; t += 2) {
        if (leaves(t)) {
            gone = true;
            break;
        }
        h2(I0{}, I0{});
        h1(I1{}, I0{});
        __syncthreads();
        h2(I1{}, I0{});
        if (t + 1 == K) break;
        h1(I0{}, I1{});
        __syncthreads();
        if (leaves(t + 1)) {
            gone = true;
            break;
        }
        h2(I0{}, I1{});
        h1(I1{}, I1{});
        __syncthreads();
        h2(I1{}, I1{});
        if (t + 2 == K) break;
        h1(I0{}, I0{});
        __syncthreads();
    }
    if (gone || !live || col < 1 || col > TW) return;
    // interior rows [K, K + TH) of each tile below row_hi, interior columns inside the row
    const int t0 = seg * SEG;
#pragma unroll
    for (int X = 0; X < 2; ++X) {
        if (X == 1 && !storeB) break;
        if (x0s[X] + col - 1 >= nl) continue;
        uint32_t so = (uint32_t)(y0s[X] - K + t0) * pitch_b + (uint32_t)(x0s[X] + col - 1) * 8u;
#pragma unroll
        for (int i = 0; i < SEG; ++i) {
            const int tr = t0 + i;
            if (tr >= K && tr < K + TH && y0s[X] - K + tr < a.row_hi) buf_store(v[X][i], rout, so, 0);
            so += pitch_b;
        }
    }
}

// ORD 3: tile pairs (tile_pass_pair).  Pair j runs tiles 2j and 2j + 1; with an odd count the
// last pair repeats its first tile and stores it once.
template <int SEG>
__global__ __launch_bounds__(1024, 1) void k_step_tile_pair(const uint64_t *__restrict__ in,
                                                            uint64_t *__restrict__ out, StepArgs a,
                                                            int turns, int ntx, int ntiles)
{
    const int npairs = (ntiles + 1) / 2;
    const int pair = tile_of_block(npairs);
    if (pair >= npairs) return;                          // the whole workgroup
    const int tA = 2 * pair, tB = 2 * pair + 1 < ntiles ? 2 * pair + 1 : 2 * pair;
    tile_pass_pair<SEG>(in, out, a, turns, tA, tB, 2 * pair + 1 < ntiles, ntx);
}

// K1p k_tile_persist: `turns` turns in blocks of K on tiles that stay resident for the whole
// launch (small boards: every tile is one resident workgroup, checked by the host).  A block
// is one tile_pass; between blocks a tile exchanges its borders with its 8 neighbours through
// memory instead of ending the launch: block b reads buffer u[(b-1) % 2] (block 0: `in`) and
// writes u[b % 2] (the last block: `out`); u0 / u1 are uncached (visible across the XCDs' L2s
// without cache maintenance, like the k_step_wg parallelogram rows) and read with sc1 loads
// that bypass the CU's vector L1.  flags[tile] = epoch + b
// + 1 once the tile's block-b stores completed; a tile starts block b when its 8 neighbours
// are there -- which also means they finished reading the buffer it is about to overwrite.
// A wait that gives up after GOL_TILE_SPIN_LIMIT polls marks the error word (GOL_EHIP at the next
// synchronising call) and goes on with a wrong board rather than hang.
template <int SEG, int ORD, int W>
__global__ __launch_bounds__(1024, 1) void k_tile_persist(
    const uint64_t *__restrict__ in, uint64_t *__restrict__ out, uint64_t *u0, uint64_t *u1,
    StepArgs a, int turns, int K, int ntx, int ntiles, unsigned *flags, unsigned epoch)
{
    const int tile = tile_of_block(ntiles);
    if (tile >= ntiles) return;                          // (never waited for)
    const int nty = ntiles / ntx, ty = tile / ntx, tx = tile - ty * ntx;
    // ceil(turns / K) blocks of near-equal depth (<= K): 1000 turns at K = 32 run as
    // 8 x 32 + 24 x 31, not 31 x 32 + 8
    const int nblocks = (turns + K - 1) / K, base = turns / nblocks, extra = turns % nblocks;
    bool gave_up = false;
    for (int b = 0; b < nblocks; ++b) {
        const int k = base + (b < extra ? 1 : 0);
        if (b > 0) {
            if (threadIdx.x < 8) {                        // one neighbour per lane 0..7
                const int j = (int)threadIdx.x + (threadIdx.x >= 4 ? 1 : 0);   // skip (0, 0)
                const int dy = j / 3 - 1, dx = j % 3 - 1;
                const int ny = (ty + dy + nty) % nty, nx = (tx + dx + ntx) % ntx;
                const unsigned want = epoch + (unsigned)b;
                unsigned *f = flags + ny * ntx + nx;
                bool seen = false;
                for (int spin = 0; !seen && spin < GOL_TILE_SPIN_LIMIT; ++spin) {
                    const unsigned v =
                        __hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    seen = (int)(v - want) >= 0;
                    if (!seen) __builtin_amdgcn_s_sleep(2);
                }
                gave_up |= !seen;
            }
            // (the loads of the block stay below the waits: the barrier and the fence)
            __atomic_signal_fence(__ATOMIC_SEQ_CST);
            __syncthreads();
        }
        const uint64_t *src = b == 0 ? in : ((b & 1) ? u0 : u1);
        uint64_t *dst = b + 1 == nblocks ? out : ((b & 1) ? u1 : u0);
        tile_pass<SEG, ORD, W, true>(src, dst, a, k, tile_pos_rect(a, tile, ntx));
        if (b + 1 == nblocks) break;
        __builtin_amdgcn_s_waitcnt((7 << 4) | (15 << 8));   // this wave's stores are done
        __syncthreads();                                     // ... and every wave's
        // (u0 / u1 are uncached: completed stores are in memory; the flag is an agent-scope
        // store, a workgroup-scope release would order nothing across CUs)
        if (threadIdx.x == 0)
            __hip_atomic_store(flags + tile, epoch + (unsigned)b + 1u, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
    }
    if (gave_up && a.err)
        __hip_atomic_store(a.err, kDevErrTileFlag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}


// ---- K1r: the block loop -------------------------------------------------------------------------
// K1r (RING): the tile stays in registers across blocks; between blocks only its ring is
// exchanged (k_tile_ring below)
struct RingArgs {
    int tile, ntx;              // the tile's index in the rectangular grid of ntx columns
    uint64_t *u0, *u1;          // board-layout edge buffers, block b writes u[b % 2]
    unsigned *flags;            // per tile: epoch + b + 1 once its block-b edges are stored
    unsigned epoch;
    int turns;                  // turns of the launch, in blocks of <= K
    unsigned *gcount;           // (tools, GOL_RING=2) non-null: a grid-wide barrier per block
    unsigned gbase;             // instead of the 8 neighbours: *gcount at the launch's start
    int ablate;                 // (tools timing ablations, wrong boards: 1 no edge stores, 2 no
                                // flag wait, 4 no ring loads)
};
// tile_pass's Lab of k_tile_ring: blocks() runs in place of the pass's turn loop
struct TileRingLab {
    static constexpr bool kBlocks = true;
    RingArgs ra;
    template <int SEG, int ORD, bool kPairs, int kLoadAux, class View, class Turn>
    __device__ __forceinline__ void blocks(const View s, Turn &&turn) const
    {
        auto &v = s.v;
        const StepArgs &a = s.a;
        const TilePos &pos = s.pos;
        const int TW = s.TW, C = s.C, G = s.G, K = s.K, TH = s.TH, nl = s.nl, y0 = s.y0, x0 = s.x0;
        const int lane = s.lane, wave = s.wave, nslot = (int)blockDim.x;
        const uint32_t pitch_b = s.pitch_b, span = s.span, off_first = s.off_first;
        // K1r: ceil(turns / K) blocks of near-equal depth <= K on the tile held in v.  After
        // block b the TH x TW interior is exact and everything else is stale; the tile stores
        // its ring's sources -- interior rows within K of its top or bottom edge and its first
        // and last interior columns -- into u[b % 2] at their board positions, flags them, waits
        // for its 8 neighbours' flags, and reloads from u[b % 2] what its neighbours stored: the
        // K rows above and below its interior (halo lanes included) and the two halo lanes.
        // Lanes and rows further out (a ragged tile's columns past the east halo lane, rows past
        // the bottom halo) stay stale: their error moves one cell per turn and the refreshed
        // halo word / K halo rows are as deep as a plain launch's.  Every tile's interior spans
        // >= K rows (host-checked), so each ring cell comes from one of the 8 neighbours.
        // Memory: K1p's uncached buffers (no cache maintenance; loads bypass the vector L1).
        static_assert(ORD != 4 && ORD != 7 && ORD < 8, "K1r: one word per lane");
        const int THv = min(TH, a.row_hi - y0), TWv = min(TW, nl - x0);
        const int nty = (a.row_hi - a.row_lo + TH - 1) / TH;
        const int tile = ra.tile, ntx = ra.ntx, ty = tile / ntx, tx = tile - ty * ntx;
        const int nblocks = (ra.turns + K - 1) / K, kbase = ra.turns / nblocks,
                  kextra = ra.turns % nblocks;
        bool gave_up = false;
        for (int b = 0; b < nblocks; ++b) {
            const int kb = kbase + (b < kextra ? 1 : 0);
            if constexpr (!kPairs) {
                for (int t = 0; t < kb; ++t) turn(std::integral_constant<int, 0>{}, (t & 1) * 2 * nslot, t);
            } else {
                for (int t = 0; t < kb; t += 2) {
                    turn(std::integral_constant<int, 0>{}, 0, t);
                    if (t + 1 == kb) break;
                    turn(std::integral_constant<int, 1>{}, 0, t + 1);
                }
            }
            if (b + 1 == nblocks) break;
            uint64_t *const X = (b & 1) ? ra.u1 : ra.u0;
            const __amdgpu_buffer_rsrc_t rx =
                __builtin_amdgcn_make_buffer_rsrc((void *)X, (short)0, (int)span, kBufFlags);
            // (the lane's values pass through an empty asm here, so that what the exchange
            // derives from them -- two predicates per row -- is formed per exchange instead of
            // hoisted out of the block loop and held in registers across the turns)
            int ln = lane, thv = THv, twv = TWv, kk = K;
            uint32_t off0 = off_first;
            asm volatile("" : "+v"(ln), "+v"(off0), "+s"(thv), "+s"(twv), "+s"(kk));
            const int gr = (int)(((uint32_t)ln * pos.rcp) >> 16), cl = ln - gr * C;
            const bool lv = gr < G;
            const int tr0 = (wave * G + gr) * SEG;       // the lane's first tile row
            if (lv && cl >= 1 && cl <= twv && !(ra.ablate & 1)) {
                const bool side = cl == 1 || cl == twv;
                uint32_t so = off0;
#pragma unroll
                for (int i = 0; i < SEG; ++i) {
                    const int j = tr0 + i - kk;           // interior row of the tile
                    if (j >= 0 && j < thv && (side || j < kk || j >= thv - kk))
                        buf_store(v[i], rx, so, 0);
                    so += pitch_b;
                    so = so >= span ? so - span : so;
                }
            }
            __builtin_amdgcn_s_waitcnt((7 << 4) | (15 << 8));   // this wave's stores are done
            __syncthreads();                                     // ... and every wave's
            // (u0 / u1 are uncached: completed stores are in memory, visible to every XCD)
            if (threadIdx.x == 0) {
                __hip_atomic_store(ra.flags + tile, ra.epoch + (unsigned)b + 1u, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
            }
            if (ra.gcount && threadIdx.x == 0) {        // (every tile: a grid-wide barrier)
                __hip_atomic_fetch_add(ra.gcount, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const unsigned want = ra.gbase + (unsigned)(b + 1) * (unsigned)(nty * ntx);
                bool seen = false;
                for (int spin = 0; !seen && spin < GOL_TILE_SPIN_LIMIT; ++spin) {
                    const unsigned fv = __hip_atomic_load(ra.gcount, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    seen = (int)(fv - want) >= 0;
                    if (!seen) __builtin_amdgcn_s_sleep(1);
                }
                gave_up |= !seen;
            }
            if (!ra.gcount && threadIdx.x < 8 && !(ra.ablate & 2)) {   // one neighbour per lane 0..7
                const int jn = (int)threadIdx.x + (threadIdx.x >= 4 ? 1 : 0);   // skip (0, 0)
                const int ny = (ty + jn / 3 - 1 + nty) % nty, nx = (tx + jn % 3 - 1 + ntx) % ntx;
                const unsigned want = ra.epoch + (unsigned)b + 1u;
                const unsigned *f = ra.flags + ny * ntx + nx;
                bool seen = false;
                for (int spin = 0; !seen && spin < GOL_TILE_SPIN_LIMIT; ++spin) {
                    const unsigned fv = __hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    seen = (int)(fv - want) >= 0;
                    if (!seen) __builtin_amdgcn_s_sleep(1);
                }
                gave_up |= !seen;
            }
            __atomic_signal_fence(__ATOMIC_SEQ_CST);
            __syncthreads();
            if (lv && !(ra.ablate & 4)) {
                const bool hl = cl == 0 || cl == twv + 1;
                uint32_t lo = off0;
#pragma unroll
                for (int i = 0; i < SEG; ++i) {
                    const int tr = tr0 + i;
                    if (tr < 2 * kk + thv && (hl || tr < kk || tr >= kk + thv)) {
                        const u32x2 w = __builtin_amdgcn_raw_buffer_load_b64(rx, lo, 0, kLoadAux);
                        v[i][0] = w.x;
                        v[i][1] = w.y;
                    }
                    lo += pitch_b;
                    lo = lo >= span ? lo - span : lo;
                }
            }
        }
        if (gave_up && a.err)
            __hip_atomic_store(a.err, kDevErrTileFlag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
};

// ---- ORD 8 / 9: the turn in inline asm -----------------------------------------------------------
template <int SEG, int ORD, class View>
__device__ __forceinline__ void tile_lab_asm_loop(const View s)
{
    auto &v = s.v;
    const StepArgs &a = s.a;
    const TilePos &pos = s.pos;
    uint4 *const xsh = s.xsh;
    const __amdgpu_buffer_rsrc_t rout = s.rout;
    const int TW = s.TW, C = s.C, G = s.G, K = s.K, TH = s.TH, nl = s.nl, y0 = s.y0, x0 = s.x0;
    const int lane = s.lane, wave = s.wave, nslot = (int)blockDim.x, myslot = s.myslot, s_up = s.s_up;
    const int s_dn = s.s_dn, wrow0 = s.wrow0, wrow1 = s.wrow1, lastrow = s.lastrow;
    const uint32_t pitch_b = s.pitch_b;
    // ORD 8: ORD 5's turn as one inline-asm block with a hand-made VGPR assignment
    // (gol_tile_turn.h, generated by gen_tile_turn.py: every v_bitop3 reads registers of
    // both parities, which the compiler's allocation does not ensure -- a v_bitop3 whose
    // sources all have one parity issues at half rate).  LDS: 64 B per slot, [slot][top,
    // bottom][turn parity]; the asm toggles the parity (bit 4) of the three addresses.
    // ORD 9: the same with the lane shifts' neighbour words fetched by ds_bpermute_b32 (the
    // LDS pipe) one row ahead instead of DPP moves (half-rate VALU instructions); lane l
    // reads lane l - 1 at address ba and lane l + 1 at ba + 8 (the wrap reaches only halo
    // and idle lanes, whose cells are junk anyway)
    static_assert(SEG % 3 == 0, "ORD 8/9: one word per lane, plain launches");
    // Registers: the asm holds v0 .. v(2 SEG + 25); everything else live across the turn
    // loop must fit the rest of the 80-VGPR budget (6 waves per SIMD): the three addresses,
    // a scalar turn count (the turn the wave leaves the trapezoid at, computed once), and
    // the store stage's lane values recomputed after the loop rather than kept.
    // (k_step_tile has no static LDS: the dynamic slots start at LDS address 0, so the
    // parity toggle is an XOR of each address with ps)
    constexpr int TV = (GOL_TURN_VAR & 6) | (ORD == 9 ? 1 : 0);
    const uint32_t base = (uint32_t)(uintptr_t)(lds_void *)xsh;
    uint32_t ad[4];
    uint32_t ps;
    if constexpr ((TV & 4) != 0) {
        // [parity][top, bottom][slot], 16 B per slot, the slot count a power of two
        // (tile_lds_bytes_code)
        const uint32_t ns = (uint32_t)tile_slots_pow2(nslot);
        ad[0] = base + 16u * (uint32_t)myslot;
        ad[1] = base + 16u * (ns + (uint32_t)myslot);
        ad[2] = base + 16u * (ns + (uint32_t)s_up);     // the segment above's last-row sums
        ad[3] = base + 16u * (uint32_t)s_dn;            // the segment below's first-row sums
        ps = 32u * ns;
    } else {
        // [slot][top, bottom][parity], 64 B per slot
        ad[0] = base + 64u * (uint32_t)myslot;
        ad[1] = 0u;
        ad[2] = base + 64u * (uint32_t)s_up + 32u;
        ad[3] = base + 64u * (uint32_t)s_dn;
        ps = 16u;
    }
    // the wave leaves at the first turn t with wrow1 <= t or wrow0 > lastrow - t
    const int tend = __builtin_amdgcn_readfirstlane(
        max(0, min(K, min(wrow1, lastrow - wrow0 + 1))));
    const uint32_t ba = ORD == 9 ? (uint32_t)((lane + 63) & 63) * 4u : 0u;
    ps = __builtin_amdgcn_readfirstlane(ps);
    for (int t = 0; t < tend; ++t) tile_turn_asm<SEG, TV>(v, ad, ps, ba);
    if (tend < K) return;
    // interior rows [K, K + TH) of the tile, below row_hi; interior columns inside the row
    // (the lane's values from the lane count of an opaque all-ones mask, formed after the
    // loop: neither the thread index nor anything derived from it stays live across it)
    uint32_t all = ~0u;
    asm volatile("" : "+v"(all));
    const int ln = (int)__builtin_amdgcn_mbcnt_hi(all, __builtin_amdgcn_mbcnt_lo(all, 0u));
    const int gr = (int)(((uint32_t)ln * pos.rcp) >> 16), cl = ln - gr * C;
    if (gr >= G || cl < 1 || cl > TW || x0 + cl - 1 >= nl) return;
    const int t0 = (wave * G + gr) * SEG;
    uint32_t so = (uint32_t)(y0 - K + t0) * pitch_b + (uint32_t)(x0 + cl - 1) * 8u;
#pragma unroll
    for (int i = 0; i < SEG; ++i) {
        const int tr = t0 + i;
        if (tr >= K && tr < K + TH && y0 - K + tr < a.row_hi) buf_store(v[i], rout, so, 0);
        so += pitch_b;
    }
    return;
}

// ---- Raw edge rows ---------------------------------------------------------------------------------
template <int SEG, int ORD, int W>
constexpr bool tile_lab_edge_rows() { return ORD < 4 && W == 1 && SEG <= GOL_TILE_RAW; }
// one slot holds both rows: the first in x, y, the last in z, w
template <int SEG>
__device__ __forceinline__ void tile_lab_put_rows(uint4 *slot, const uint32_t (&v)[SEG][2])
{
    *slot = make_uint4(v[0][0], v[0][1], v[SEG - 1][0], v[SEG - 1][1]);
}
// the last row of the segment above (the z, w half of its slot) and the first row of the one
// below (x, y), summed here
template <int SEG, int W>
__device__ __forceinline__ void tile_lab_get_rows(const uint4 *base, int s_up, int s_dn,
                                                  uint32_t (&Us)[4 * W], uint32_t (&Ds)[4 * W])
{
    constexpr int ND = 2 * W;
    const uint2 a = *(reinterpret_cast<const uint2 *>(base + s_up) + 1);
    const uint2 b = *reinterpret_cast<const uint2 *>(base + s_dn);
    const uint32_t ra[ND] = {a.x, a.y}, rb[ND] = {b.x, b.y};
    tile_rsum<SEG, W>(ra, Us);
    tile_rsum<SEG, W>(rb, Ds);
}

// K1r k_tile_ring: K1p's resident tiles without the round trip of the whole tile -- between
// blocks a tile stores and reloads only its ring (TileRingLab).  Small torus boards: every
// tile one resident workgroup (host-checked: a wait for a tile that never runs gives up after
// GOL_TILE_SPIN_LIMIT polls and marks the error word).  u0 / u1: uncached board-layout buffers.
template <int SEG, int ORD>
__global__ __launch_bounds__(1024, 1) void k_tile_ring(
    const uint64_t *__restrict__ in, uint64_t *__restrict__ out, uint64_t *u0, uint64_t *u1,
    StepArgs a, int turns, int K, int ntx, int ntiles, unsigned *flags, unsigned epoch,
    unsigned *gcount, unsigned gbase, int ablate)
{
    const int tile = tile_of_block(ntiles);
    if (tile >= ntiles) return;                          // (never waited for)
    tile_pass<SEG, ORD, 1, true, false, false, false, false, TileRingLab>(
        in, out, a, K, tile_pos_rect(a, tile, ntx),
        TileRingLab{RingArgs{tile, ntx, u0, u1, flags, epoch, turns, gcount, gbase, ablate}});
}

// K1q k_tile_stream: K1p's blocks for boards whose tiles do not all fit at once.  One launch
// runs `turns` turns as blocks of <= K turns; the (block, tile) items are taken in order from
// a device counter by a grid of resident workgroups, so one launch has one start and one tail
// instead of one per K turns (a K1t launch costs ~55 us besides its turns at 65536^2).  Item
// i = b * ntiles + j is tile row (j / ntx + 2 b) mod nty, column j % ntx of block b: every
// item of block b is taken before any of block b + 1, and an item waits only for its 8
// neighbours' block b - 1 (flags as K1p: epoch + b once a tile's block-b stores completed),
// and on its own block b - 1 (it ran on another workgroup), all taken earlier and so running
// or done -- no deadlock whatever the residency.
// Rotating the tile rows by 2 per block puts the first items of a block on rows whose
// neighbours were among the first of the block before (the torus wrap would otherwise make
// the first row wait for the previous block's last).  Block b reads u[(b-1) % 2] (block 0:
// `in`) and writes u[b % 2] (the last block: `out`), as K1p.  counter counts across
// launches: each workgroup takes one item past the end before it leaves, so a launch
// advances it by items + grid; `base` is its value at the launch (unsigned wrap).
// (the item loop holds registers across items: bound them to k_step_tile's budget -- 80
// VGPRs at SEG 24, 6 waves per SIMD; 64 below, 8)
template <int SEG, int ORD, int W>
__global__ __launch_bounds__(1024, (SEG >= 20 ? 6 : 8)) void k_tile_stream(
    const uint64_t *__restrict__ in, uint64_t *__restrict__ out, uint64_t *u0, uint64_t *u1,
    StepArgs a, int turns, int K, int ntx, int ntiles, unsigned *flags, unsigned epoch,
    unsigned *counter, unsigned base)
{
    __shared__ unsigned next_item;
    const int nty = ntiles / ntx;
    const int nblocks = (turns + K - 1) / K, kbase = turns / nblocks, extra = turns % nblocks;
    const unsigned nitems = (unsigned)nblocks * (unsigned)ntiles;
    bool gave_up = false;
    if (threadIdx.x == 0)
        next_item = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - base;
    __syncthreads();
    for (;;) {
        const unsigned item = next_item;
        __syncthreads();                                  // (everyone has read next_item)
        if (item >= nitems) break;                        // (workgroup-uniform)
        // the next item's fetch overlaps this one (its latency is a memory round trip, in
        // flight with the tile loads); thread 0 hands it over at the end of the item
        unsigned nxt = 0;
        if (threadIdx.x == 0)
            nxt = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - base;
        const int b = (int)(item / (unsigned)ntiles), j = (int)(item % (unsigned)ntiles);
        const int ty = (j / ntx + 2 * b) % nty, tx = j % ntx;
        const int tile = ty * ntx + tx;
        const int k = kbase + (b < extra ? 1 : 0);
        if (b > 0) {
            // the 8 neighbours AND the tile itself: unlike K1p, the tile's own block b - 1 ran
            // on some other workgroup, which may still be reading the buffer this item is about
            // to overwrite, and wrote the interior this item reads
            if (threadIdx.x < 9) {                        // one tile per lane 0..8
                const int jj = (int)threadIdx.x;
                const int dy = jj / 3 - 1, dx = jj % 3 - 1;
                const int ny = (ty + dy + nty) % nty, nx = (tx + dx + ntx) % ntx;
                const unsigned want = epoch + (unsigned)b;
                unsigned *f = flags + ny * ntx + nx;
                bool seen = false;
                for (int spin = 0; !seen && spin < GOL_TILE_SPIN_LIMIT; ++spin) {
                    const unsigned v =
                        __hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    seen = (int)(v - want) >= 0;
                    if (!seen) __builtin_amdgcn_s_sleep(2);
                }
                gave_up |= !seen;
            }
            __atomic_signal_fence(__ATOMIC_SEQ_CST);
            // cached block buffers (MI355X_MICROARCH, inter-workgroup visibility, consumer
            // form): one agent acquire in the polling wave, its wait, then the barrier
            if (threadIdx.x < 64) {
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            __syncthreads();
        }
        const uint64_t *src = b == 0 ? in : ((b & 1) ? u0 : u1);
        uint64_t *dst = b + 1 == nblocks ? out : ((b & 1) ? u1 : u0);
        // (the shape's scalars pass through an empty asm every item, so the lane constants
        // tile_pass derives from them are recomputed per item rather than hoisted out of the
        // loop and held in VGPRs across it: that spilled at SEG 24)
        StepArgs aa = a;
        asm volatile("" : "+s"(aa.tile_w), "+s"(aa.band), "+s"(aa.nw), "+s"(aa.pitch),
                     "+s"(aa.modrows));
        tile_pass<SEG, ORD, W, true>(src, dst, aa, k, tile_pos_rect(aa, tile, ntx));
        if (b + 1 < nblocks) {
            __builtin_amdgcn_s_waitcnt((7 << 4) | (15 << 8));   // this wave's stores are done
            __syncthreads();                                     // ... and every wave's
            // (producer form: lane 0 writes the XCD L2's dirty lines back, waits, then flags)
            if (threadIdx.x == 0) {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __hip_atomic_store(flags + tile, epoch + (unsigned)b + 1u, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        if (threadIdx.x == 0) next_item = nxt;
        __syncthreads();                                  // (and the LDS slots are free again)
    }
    if (gave_up && a.err)
        __hip_atomic_store(a.err, kDevErrTileFlag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

}  // namespace golk
