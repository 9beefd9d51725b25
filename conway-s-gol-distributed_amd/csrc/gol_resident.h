// gol_resident.h -- K1r2 k_step_resident: a torus board narrower than 256 cells, resident in the
// registers of one workgroup for all the turns of a launch (gol_resident.hip holds the kernel,
// its launch and the library's device-free model of it).
//
// A lane owns R consecutive rows and holds all nw = ceil(width / 64) words of each: at most
// kResidentMaxWords words per lane, at most kResidentMaxLanes lanes (4 wavefronts, one per SIMD).
// The x direction never leaves the lane (west_word / east_word on the lane's own words); in the
// y direction a lane's own rows neighbour each other in registers, and once per turn every lane
// publishes its first and its last row to LDS and reads lane - 1's last and lane + 1's first
// row, lane indices modulo the active lanes (a lane may be its own neighbour: a board of at most
// R rows).  The LDS area is double-buffered by turn parity, so the one workgroup barrier of a
// turn -- between the publication and the reads -- is enough: a lane that publishes turn t + 2
// has passed barrier t + 1, which every lane reaches after its reads of turn t.
//
// Everything a turn computes is written here once, __host__ __device__: the kernel runs it on
// its registers and LDS, gol_resident_host_run lane by lane on arrays indexed the same way.
#pragma once
#include "gol_device.h"

namespace golk {

constexpr int kResidentMaxWidth = 255;     // wider boards have k_step_tile
constexpr int kResidentMaxWords = 16;      // board words a lane holds
constexpr int kResidentMaxLanes = 256;
constexpr int kResidentMaxRowWords = 4;    // nw of the widest board

struct ResidentPlan {
    int lanes = 0;                         // active lanes: ceil(height / rows)
    int rows = 0;                          // R: rows per lane (the last active lane: the rest)
    int waves = 0;                         // wavefronts launched: ceil(lanes / 64)
};

// rows per lane the kernel is built for at nw words per row: the powers of two up to
// kResidentMaxWords / nw, and that bound itself (nw = 3: 5 rows)
constexpr bool resident_rows_built(int nw, int R)
{
    return nw >= 1 && nw <= kResidentMaxRowWords && R >= 1 && R * nw <= kResidentMaxWords &&
           ((R & (R - 1)) == 0 || R == kResidentMaxWords / nw);
}
// the tallest board of that width
constexpr int resident_max_height(int nw) { return kResidentMaxLanes * (kResidentMaxWords / nw); }
// eligible by shape
constexpr bool resident_shape_ok(int width, int height)
{
    return width >= 2 && width <= kResidentMaxWidth && height >= 1 &&
           height <= resident_max_height((width + 63) / 64);
}
// The partition.  The rule for R, the one place it is written: the fewest rows per lane the
// kernel is built for that fit the board into kResidentMaxLanes lanes -- the most lanes, so the
// least VALU work per wavefront.  A turn's time grows with the words a lane holds (a wavefront
// alone on its SIMD issues one VALU instruction per 4 cycles) and hardly with the wavefront
// count: twice the rows per lane measured 1.27-1.45x slower on 16^2, 64^2, 128^2 and 200 x 77,
// also where it saves the cross-wave barrier (128^2: 2 wavefronts of 2 words at 0.414 us per
// turn, 1 wavefront of 4 words at 0.526; DESIGN.md "K1r2: resident boards").
// rows_req > 0 (A/B runs): that R instead, where it is built and fits.
__host__ __device__ constexpr bool resident_plan(int width, int height, ResidentPlan *p, int rows_req = 0)
{
    if (!resident_shape_ok(width, height)) return false;
    const int nw = (width + 63) / 64;
    int R = 0;
    for (int r = 1; r * nw <= kResidentMaxWords && !R; ++r)
        if (resident_rows_built(nw, r) && (height + r - 1) / r <= kResidentMaxLanes) R = r;
    if (rows_req > 0 && resident_rows_built(nw, rows_req) &&
        (height + rows_req - 1) / rows_req <= kResidentMaxLanes)
        R = rows_req;
    if (!R) return false;
    p->rows = R;
    p->lanes = (height + R - 1) / R;
    p->waves = (p->lanes + 63) / 64;
    return true;
}

// rows lane `lane` owns (0: a lane past the board)
__host__ __device__ inline int resident_rows_of(int lane, int R, int height)
{
    const int left = height - lane * R;
    return left <= 0 ? 0 : left < R ? left : R;
}
// the lanes whose last / first row a lane reads: modulo the active lanes
__host__ __device__ inline int resident_north_lane(int lane, int lanes) { return lane == 0 ? lanes - 1 : lane - 1; }
__host__ __device__ inline int resident_south_lane(int lane, int lanes) { return lane == lanes - 1 ? 0 : lane + 1; }
// the exchange area: [turn parity][0 first row, 1 last row][word of the row][lane], in words
__host__ __device__ constexpr int resident_xch_words(int nw) { return 2 * 2 * nw * kResidentMaxLanes; }
__host__ __device__ inline int resident_xch_index(int nw, int parity, int which, int j, int lane)
{
    return ((parity * 2 + which) * nw + j) * kResidentMaxLanes + lane;
}
// cells in a row's last word, and the mask that keeps its padding bits zero
__host__ __device__ inline int resident_tail_bits(int width, int nw) { return width - 64 * (nw - 1); }
__host__ __device__ inline uint64_t resident_tail_mask(int nb) { return nb == 64 ? ~0ull : ((1ull << nb) - 1); }

// the 3-cell sums of a torus row (low bit s0, high bit s1 per cell), centre included
template <int NW>
__host__ __device__ __forceinline__ void resident_row_sums(const uint64_t (&row)[NW], int nb,
                                                           uint64_t (&s0)[NW], uint64_t (&s1)[NW])
{
#pragma unroll
    for (int j = 0; j < NW; ++j) {
        const uint64_t w = west_word(row, j, NW, nb), e = east_word(row, j, NW, nb);
        s0[j] = w ^ row[j] ^ e;
        s1[j] = maj3(w, row[j], e);
    }
}

// a lane's last own row (RAG: `mine` < R is possible -- the board's last lane; else row R - 1)
template <int NW, int R, bool RAG>
__host__ __device__ __forceinline__ void resident_last_row(const uint64_t (&v)[R][NW], int mine,
                                                           uint64_t (&last)[NW])
{
#pragma unroll
    for (int j = 0; j < NW; ++j) last[j] = v[RAG ? 0 : R - 1][j];
    if constexpr (RAG) {
#pragma unroll
        for (int i = 1; i < R; ++i)
#pragma unroll
            for (int j = 0; j < NW; ++j)
                if (i < mine) last[j] = v[i][j];
    }
}

// One turn of a lane's rows in place: v = its R rows (`mine` of them real), north = the row
// above its first, south = the row below its last real one.  Rows past `mine` come out as
// garbage that nothing reads.
template <int NW, int R, bool RAG>
__host__ __device__ __forceinline__ void resident_turn(uint64_t (&v)[R][NW], const uint64_t (&north)[NW],
                                                       const uint64_t (&south)[NW], int mine, int nb,
                                                       uint64_t tail)
{
    uint64_t a0[NW], a1[NW], b0[NW], b1[NW], c0[NW], c1[NW];
    resident_row_sums<NW>(north, nb, a0, a1);
    resident_row_sums<NW>(v[0], nb, b0, b1);
#pragma unroll
    for (int i = 0; i < R; ++i) {
        uint64_t below[NW];
#pragma unroll
        for (int j = 0; j < NW; ++j) {
            if (i + 1 == R) below[j] = south[j];
            else below[j] = RAG && i + 1 == mine ? south[j] : v[i + 1 < R ? i + 1 : i][j];
        }
        resident_row_sums<NW>(below, nb, c0, c1);
#pragma unroll
        for (int j = 0; j < NW; ++j) {
            uint64_t o = life_rule(a0[j], a1[j], b0[j], b1[j], c0[j], c1[j], v[i][j]);
            if (j == NW - 1) o &= tail;
            v[i][j] = o;
            a0[j] = b0[j];
            a1[j] = b1[j];
            b0[j] = c0[j];
            b1[j] = c1[j];
        }
    }
}

// alive cells of a lane's real rows
template <int NW, int R, bool RAG>
__host__ __device__ __forceinline__ uint32_t resident_alive(const uint64_t (&v)[R][NW], int mine)
{
    uint32_t n = 0;
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
        for (int j = 0; j < NW; ++j) {
            const uint32_t c = (uint32_t)__builtin_popcountll(v[i][j]);
            n += (RAG ? i < mine : mine > 0) ? c : 0u;
        }
    return n;
}

}  // namespace golk
