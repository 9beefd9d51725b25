// gol_plan.cpp — the launch planner: what gol_step runs next (kernel, depth, band, tile shape),
// whether a launch is cut into row chunks and where, and the calls that report plans and
// tables.  Nothing here touches a stream or an event; gol_step.cpp enqueues and orders.
#include <algorithm>
#include <cstdlib>
#include <iterator>

#include "gol_ctx.h"

using namespace goleng;

namespace goleng {

void set_shape(gol_ctx *c, LaunchShape s)
{
    c->shape = std::move(s);
    for (int &b : c->band_at) b = 0;
}

golk::StepArgs whole_buffer_args(const gol_ctx *c)
{
    golk::StepArgs a{};
    a.width = c->cfg.width;
    a.nw = c->nw;
    a.pitch = c->pitch;
    a.modrows = c->buf_rows;
    a.row_lo = 0;
    a.row_hi = c->buf_rows;
    a.cnt_lo = own_lo(c);
    a.cnt_hi = own_hi(c);
    a.variant = c->variant;
    a.multi_words = c->multi_words;
    a.wg_prio = c->wg_prio;
    a.tile_big = c->tile_big_forced ? 1 : 0;
    a.tile_duo = c->tile_duo ? 1 : 0;
    a.err = c->d_err;
    return a;
}

// The band a kernel tuned at (K0, band0) runs at depth k.  A launch of another depth -- the
// even split's shallower launches, a short gol_step, the last block before a halo exchange,
// a planned launch -- runs a kernel with another residency (k_step_wg: 4..8 waves per
// workgroup at 7 or 8 waves per SIMD; k_step_skew: 2..4 waves per SIMD), where band0 would
// leave resident slots idle or spill a few pipelines into one more round (65536^2: K = 16's
// band 607 fills 1791 of 1792 slots; a K = 20 launch has 1280).  Keep the tuned number of
// rounds instead: the smallest band whose grid fits them at depth k (kMultiWgPg: the next
// band it runs at).
int band_same_rounds(const gol_ctx *c, int var, int K0, int band0, int k)
{
    if (k == K0 || k < 2 || k > golk::kMaxTurnsPerLaunch || var == golk::kMultiTile)
        return band0;                        // (k_step_tile: the tile height stays)
    const int lane_dw = golk::multi_lane_dwords(c->multi_words, var);
    const int per = golk::multi_pipes_per_block(var);
    const long long cap_t = (long long)c->ncu * golk::multi_blocks_per_cu(K0, c->multi_words, var) * per;
    const long long cap_k = (long long)c->ncu * golk::multi_blocks_per_cu(k, c->multi_words, var) * per;
    if (cap_t <= 0 || cap_k <= 0) return band0;
    const int W = c->cfg.width, rows = c->buf_rows;
    const long long pipes = golk::multi_pipes(W, rows, band0, lane_dw, var);
    const long long rounds = std::max(1ll, (pipes + cap_t - 1) / cap_t);
    int b = band0;
    for (int band = 16; band <= std::max(rows, 16); ++band)
        if (golk::multi_pipes(W, rows, band, lane_dw, var) <= rounds * cap_k) {
            b = band;
            break;
        }
    const bool ser = var == golk::kMultiWgPgS;
    if (golk::is_pg_variant(var) && golk::pg_ok(k, golk::pg_band(k, b, ser), ser))
        b = golk::pg_band(k, b, ser);
    return b;
}

// the word layout a launch of depth k runs on
bool stepping_il(const gol_ctx *c, int k)
{
    return k > 1 && golk::multi_is_il(c->multi_words, c->shape.multi_variant);
}

}  // namespace goleng

namespace {

// band_same_rounds for the engine's kernel and depth (cached per shape: set_shape resets the
// cache, this fills it); a band the caller fixed (gol_config.band_rows) is kept
int band_for_depth(gol_ctx *c, int k)
{
    const LaunchShape &s = c->shape;
    if (s.short_k > 0 && s.multi_variant == golk::kMultiTile && c->cfg.band_rows <= 0 &&
        k >= 2 && k <= s.short_k)
        return s.short_band;
    if (k == s.tpl || c->cfg.band_rows > 0 || k < 2 || k > golk::kMaxTurnsPerLaunch)
        return s.band_multi;
    int &b = c->band_at[k];
    if (b <= 0) b = band_same_rounds(c, s.multi_variant, s.tpl, s.band_multi, k);
    return b;
}

// A count engine (GOL_FLAG_COUNT_EVERY_TURN) runs multi-turn launches only on k_step_tile at
// a code with a counted instantiation (golk::kTileCountCodes) and on k_step_resident (every
// instantiation has its counted form); every other count engine -- K1s
// / K1w kernels, a GOL_TILE code without one, generic widths, blocking_limited,
// GOL_COUNT_BLOCKING=0 -- runs one-turn launches with the count fused into the stencil.
bool count_fused(const gol_ctx *c)
{
    return (c->cfg.flags & GOL_FLAG_COUNT_EVERY_TURN) && c->count_blocking && c->shape.tpl > 1 &&
           (golk::is_resident_variant(c->shape.multi_variant) ||
            (c->shape.multi_variant == golk::kMultiTile &&
             golk::tile_code_counted(c->shape.tile_seg)));
}

// a k_step_resident launch of k turns (its one shape: the band is the create-time rows per lane,
// whatever the depth); a depth it does not run: one turn
Launch resident_launch(const gol_ctx *c, int k)
{
    if (!golk::resident_turns_ok(k)) return Launch{1, c->shape.multi_variant, c->band, 0, 0};
    return Launch{k, golk::kMultiResident, c->shape.band_multi, 0, 0};
}

}  // namespace

namespace goleng {

// The next launch when `room` turns remain before the next sync point (end of the gol_step
// call, or the next halo exchange of a strip engine).  k = 1: the one-turn kernel.
//  * Autotuned engines follow the launch plan for room <= kPlanMax: the sequence of launches
//    (depth and kernel) the create-time timing table says is fastest.  A short launch costs
//    nearly as much as a full one and the kernels differ in that fixed cost (65536^2,
//    profiles/r02_launch_table_65536.log: k_step_skew 260 us at K = 6 and 384 at K = 10;
//    k_step_wg 413 us at K = 4, 459 at 12, 595 at 16), so 20 turns run best as 10 + 10 on
//    k_step_skew although k_step_wg at K = 16 is the fastest per turn.  Longer stretches run
//    full launches of the tuned kernel and depth first.
//  * Otherwise the turns are spread over ceil(room / tpl) launches of near-equal depth: 128
//    turns at tpl 6 run as 18 x 6 + 4 x 5, not 21 x 6 + 2.
// gol_step and gol_halo_buffers both use this rule (the zero-copy halo layout must be the
// layout the first launch after an exchange runs on; every planned kernel runs on the
// interleaved layout).
Launch plan_launch(gol_ctx *c, int64_t room)
{
    const LaunchShape &s = c->shape;
    Launch L{1, s.multi_variant, c->band, 0, 0};
    if (s.tpl <= 1 || room < 2 || c->blocked_pending) return L;
    if (c->cfg.flags & GOL_FLAG_COUNT_EVERY_TURN) {
        if (!count_fused(c)) return L;
        // a counted launch adds into K consecutive slots of the count ring: it ends at the
        // ring's last slot at the latest (once per kRingSlots turns).  No K1p / K1q, no timed
        // plans (they mix kernels without a counted form): the even split at the tuned depth.
        room = std::min<int64_t>(room, kRingSlots - (c->turn + 1) % kRingSlots);
        if (room < 2) return L;
        const int64_t nl = (room + s.tpl - 1) / s.tpl;
        const int k = (int)((room + nl - 1) / nl);
        if (golk::is_resident_variant(s.multi_variant)) return resident_launch(c, k);
        const int band = band_for_depth(c, k);
        if (!golk::multi_ok(c->cfg.width, k, s.multi_variant, s.tile_seg) ||
            !golk::tile_shape_ok(c->nw, k, band, s.tile_w, s.tile_seg, c->cfg.width))
            return L;
        return Launch{k, s.multi_variant, band, s.tile_w, s.tile_seg};
    }
    if (blocks_plan(c, room, &L)) return L;  // K1p / K1q (tools build)
    if (!s.plan.empty()) {
        if (room > kPlanMax)
            return Launch{s.tpl, s.multi_variant, s.band_multi, s.tile_w, s.tile_seg};
        if (s.plan[room].k >= 2) return s.plan[room];
    }
    const int64_t nl = (room + s.tpl - 1) / s.tpl;
    const int k = (int)((room + nl - 1) / nl);
    if (golk::is_resident_variant(s.multi_variant)) return resident_launch(c, k);
    if (!golk::multi_ok(c->cfg.width, k, s.multi_variant, s.tile_seg)) return L;
    const int band = band_for_depth(c, k);
    // (a big engine: no depth at which the tile's window would not fit -- one turn instead)
    if (c->tile_big && !golk::tile_big_ok(c->cfg.width, c->buf_rows, c->pitch, k, band, s.tile_seg))
        return L;
    return Launch{k, s.multi_variant, band, s.tile_w, s.tile_seg};
}

const std::vector<Launch> *timed_sequence(const gol_ctx *c, int64_t turns)
{
    const auto &seq = c->shape.seq;
    const bool cnt = (c->cfg.flags & GOL_FLAG_COUNT_EVERY_TURN) != 0;
    // (a resident engine has no timed sequence: nothing was timed for it)
    return !is_strip(c) && !cnt && !c->blocked_pending && turns >= 2 && turns <= kSeqMax &&
                   turns < (int64_t)seq.size() && !seq[turns].empty()
               ? &seq[turns]
               : nullptr;
}

std::vector<int> chunk_bounds(int rows, int tile_h, int want, int min_rows)
{
    if (rows < 1 || tile_h < 1) return {0, std::max(rows, 0)};
    const int nty = (rows + tile_h - 1) / tile_h;
    for (int n = std::min({want, nty, kMaxStepChunks}); n >= 2; --n) {
        // floor(nty / n) tile rows each, one more for the last nty % n chunks; the last chunk
        // holds the ragged tile row
        const int base = nty / n, extra = nty % n;
        std::vector<int> b(n + 1);
        b[0] = 0;
        for (int i = 0; i < n; ++i)
            b[i + 1] = b[i] + (base + (i >= n - extra ? 1 : 0)) * tile_h;
        b[n] = rows;
        bool ok = true;
        for (int i = 0; i < n; ++i) ok = ok && b[i + 1] - b[i] >= min_rows;
        if (ok) return b;
    }
    return {0, rows};
}

namespace {
// rows [a0, a1) of the torus (0 <= a0 < a1 <= rows) meet rows [b0, b1) taken modulo `rows`
// (b0 may be negative and b1 past the end: a range widened by a launch's depth)
bool rows_meet(int rows, int a0, int a1, long long b0, long long b1)
{
    if (b1 - b0 >= rows) return true;
    for (long long s = -rows; s <= rows; s += rows)
        if (a0 < b1 + s && b0 + s < a1) return true;
    return false;
}
}  // namespace

// Launch n reads board A and writes board B, launch n + 1 reads B and writes A.  Chunk q of
// launch n + 1 computes its output rows from those rows of B widened by kn on both sides, and
// chunk p of launch n computed its own from A widened by kp.  So q follows p when
//   * p's output rows meet q's output rows widened by kn (q reads what p wrote), or
//   * p's output rows widened by kp meet q's output rows (q overwrites what p read).
// Nothing else needs an edge.  Two launches apart, chunk r of launch n + 2 overwrites rows of B
// that chunks p of launch n wrote: take a row x of both.  The chunk q of launch n + 1 that
// holds x among its output rows follows p by the first rule (x is in q's widened rows and in
// p's output) and r follows q by the second (x is in q's widened rows and in r's output), so
// the write-after-write order follows from the two edges.  Launch n + 2 reads A, which launch
// n only read.
std::vector<std::vector<int>> chunk_deps(int rows, const std::vector<int> &pb, int kp,
                                         const std::vector<int> &nb, int kn)
{
    const int np = (int)pb.size() - 1, nn = (int)nb.size() - 1;
    std::vector<std::vector<int>> deps(std::max(nn, 0));
    for (int q = 0; q < nn; ++q)
        for (int p = 0; p < np; ++p)
            if (rows_meet(rows, pb[p], pb[p + 1], (long long)nb[q] - kn, (long long)nb[q + 1] + kn) ||
                rows_meet(rows, nb[q], nb[q + 1], (long long)pb[p] - kp, (long long)pb[p + 1] + kp))
                deps[q].push_back(p);
    return deps;
}

// Chunks per launch in automatic mode: launches of at least kChunkMinRounds rounds of the
// resident workgroups (CUs x tile_blocks_per_cu) get chunks of about kChunkRounds rounds.
// 65536^2 (9.7 rounds per K = 30 launch), 960 turns, median of 3 alternating passes on one
// box, k GCUPS by chunks per launch: 1: 131.8, 3: 125.9 (every chunk follows every chunk),
// 4: 138.7, 5: 139.5, 6: 137.9, 7: 137.4, 8: 136.5, 10: 136.8, 20: 125.7
// (profiles/chunk_overlap_ab.log) -- 5 chunks of 1.9 rounds.  A third stream was level at
// best (5: 138.7, 8: 137.9, 10: 137.8) and is not built.
constexpr int kChunkMinRounds = 4;
constexpr double kChunkRounds = 2.0;

int chunk_request(const gol_ctx *c, bool ctl, bool overlapped)
{
    const char *env = getenv("GOL_STEP_CHUNKS");
    const int n = env ? atoi(env) : 0;
    const bool cnt = (c->cfg.flags & GOL_FLAG_COUNT_EVERY_TURN) != 0;
    if (is_strip(c) || cnt || ctl || overlapped || !c->side) return 1;
    return n <= 0 ? -1 : std::min(n, kMaxStepChunks);
}

namespace {

// a launch the pipeline may cut, in a step that may chunk at all (request != 1)
bool chunk_eligible(const gol_ctx *c, const Launch &L, int request)
{
    return request != 1 && L.k > 1 && L.var == golk::kMultiTile && !c->blocked_pending &&
           !c->readers.load(std::memory_order_relaxed);
}

int chunks_wanted(const gol_ctx *c, const Launch &L, int request)
{
    if (request > 0) return request;
    const long long wg = golk::tile_grid(c->nw, c->buf_rows, L.k, L.band, L.tw, L.seg).tiles();
    const long long slots =
        (long long)c->ncu * golk::tile_blocks_per_cu(L.k, L.band, L.tw, L.seg, c->cfg.width);
    if (slots <= 0 || wg < kChunkMinRounds * slots) return 1;
    return (int)std::min<long long>(kMaxStepChunks,
                                    std::max(2ll, (long long)((double)wg / (kChunkRounds * (double)slots) + 0.5)));
}

}  // namespace

std::vector<int> plan_chunks(gol_ctx *c, const Launch &L, int request, int64_t left,
                             const Launch *timed_next, int k_live)
{
    const int want = chunk_eligible(c, L, request) ? chunks_wanted(c, L, request) : 1;
    if (want <= 1) return {};                // (a board too small for chunks plans nothing more)
    // (the next launch as planned from here, before this one has advanced the engine: a
    // prediction that only decides whether to start a pipeline and how tall the chunks are --
    // chunk_deps is right for any bounds, so a wrong guess costs overlap alone)
    int k_next = 0;
    if (left >= 2) {
        const Launch nx = timed_next ? *timed_next : plan_launch(c, left);
        if (chunk_eligible(c, nx, request) && chunks_wanted(c, nx, request) > 1) k_next = nx.k;
    }
    if (!k_live && !k_next) return {};
    return chunk_bounds(c->buf_rows, L.band, want, std::max({L.k, k_next, k_live}));
}

}  // namespace goleng

// ================================================================ C ABI: plans and tables
namespace {

template <size_t N>
int code_list(const int (&table)[N], int n, int32_t *codes, int32_t cap)
{
    if (cap < 0 || (cap > 0 && !codes)) return GOL_EINVAL;
    for (int i = 0; i < std::min(n, (int)cap); ++i) codes[i] = table[i];
    return n;
}

}  // namespace

extern "C" {

int gol_last_launches(gol_ctx *c, int32_t *turns, int32_t *kernel, int32_t *band, int32_t cap)
{
    if (!c || cap < 0 || (cap > 0 && (!turns || !kernel || !band))) return GOL_EINVAL;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    const int n = (int)std::min<size_t>((size_t)cap, c->last.size());
    for (int i = 0; i < n; ++i) {
        turns[i] = c->last[i].k;
        kernel[i] = c->last[i].var;
        band[i] = c->last[i].band;
    }
    return (int)std::min<long long>(c->last_n, 0x7fffffff);
}

int gol_last_launch_tiles(gol_ctx *c, int32_t *tile_w, int32_t *tile_seg, int32_t *waves,
                          int32_t *block_turns, int32_t cap)
{
    if (!c || cap < 0 || (cap > 0 && (!tile_w || !tile_seg || !waves || !block_turns)))
        return GOL_EINVAL;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    const int n = (int)std::min<size_t>((size_t)cap, c->last.size());
    for (int i = 0; i < n; ++i) {
        const Launch &L = c->last[i];
        const bool p = L.var == golk::kMultiTilePersist || L.var == golk::kMultiTileStream;
        const bool t = L.k > 1 && (L.var == golk::kMultiTile || p);
        const int depth = p ? L.blk : L.k;               // (K1p / K1q: the waves fit one block)
        tile_w[i] = t ? L.tw : 0;
        tile_seg[i] = t ? L.seg : 0;
        waves[i] = t ? golk::tile_waves(depth, L.band, L.tw, L.seg) : 0;
        block_turns[i] = t ? depth : 0;
    }
    return (int)std::min<long long>(c->last_n, 0x7fffffff);
}

int gol_last_step_chunks(gol_ctx *c)
{
    if (!c) return GOL_EINVAL;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    return (int)std::min<long long>(c->last_chunks, 0x7fffffff);
}

int gol_step_chunk_plan(int32_t rows, int32_t k_prev, int32_t tile_h_prev, int32_t chunks_prev,
                        int32_t k_next, int32_t tile_h_next, int32_t chunks_next, int32_t *counts,
                        int32_t *prev_bounds, int32_t *next_bounds, uint8_t *deps, int32_t cap)
{
    if (rows < 1 || k_prev < 1 || k_next < 1 || tile_h_prev < 1 || tile_h_next < 1 ||
        chunks_prev < 1 || chunks_next < 1 || cap < 1 || chunks_prev > cap || chunks_next > cap ||
        !counts || !prev_bounds || !next_bounds || !deps)
        return GOL_EINVAL;
    const int min_rows = std::max(k_prev, k_next);
    const std::vector<int> pb = chunk_bounds(rows, tile_h_prev, chunks_prev, min_rows);
    const std::vector<int> nb = chunk_bounds(rows, tile_h_next, chunks_next, min_rows);
    const auto d = chunk_deps(rows, pb, k_prev, nb, k_next);
    counts[0] = (int32_t)pb.size() - 1;
    counts[1] = (int32_t)nb.size() - 1;
    std::copy(pb.begin(), pb.end(), prev_bounds);
    std::copy(nb.begin(), nb.end(), next_bounds);
    std::fill(deps, deps + (size_t)cap * cap, (uint8_t)0);
    for (size_t q = 0; q < d.size(); ++q)
        for (int p : d[q]) deps[q * cap + p] = 1;
    return GOL_OK;
}

int gol_tile_grid(int32_t nw, int32_t rows, int32_t turns, int32_t tile_h, int32_t tile_w,
                  int32_t seg, int32_t *grid)
{
    if (!grid || nw < 1 || rows < 1 || !golk::tile_shape_ok(nw, turns, tile_h, tile_w, seg))
        return GOL_EINVAL;
    const golk::TileGrid g = golk::tile_grid(nw, rows, turns, tile_h, tile_w, seg);
    grid[0] = g.ntx_main;
    grid[1] = g.nty_main;
    grid[2] = g.n_narrow;
    grid[3] = g.narrow_w;
    grid[4] = g.narrow_h;
    return GOL_OK;
}

int gol_seam_word(const uint64_t *row, int32_t width, int32_t v, int32_t layout, uint64_t *out)
{
    if (!row || !out || width < 256 || (layout != 0 && layout != 1)) return GOL_EINVAL;
    const int nw = (width + 63) / 64, L = nw - 1, r = width % 64;
    if (v < -1 || v > nw) return GOL_EINVAL;
    const uint64_t p = row[golk::seam_primary_col(v, L)];
    // whole words, or a column that is a real word: no stitch
    *out = r == 0 || (v >= 0 && v < L)
               ? p
               : golk::seam_stitch(p, row[golk::seam_second_col(v, L)], v, L, r, (r & 1) != 0,
                                 layout == 1);
    return GOL_OK;
}

// the code lists: the table's length, and its first min(length, cap) codes
int gol_tile_codes(int32_t *codes, int32_t cap)
{
    return code_list(golk::kTileCodes, (int)std::size(golk::kTileCodes), codes, cap);
}

int gol_tile_count_codes(int32_t *codes, int32_t cap)
{
    return code_list(golk::kTileCountCodes, (int)std::size(golk::kTileCountCodes), codes, cap);
}

int gol_tile_seam_codes(int32_t *codes, int32_t cap)
{
    return code_list(golk::kTileSeamCodes, (int)std::size(golk::kTileSeamCodes), codes, cap);
}

int gol_tile_big_codes(int32_t *codes, int32_t cap)
{
    return code_list(golk::kTileBigCodes, (int)std::size(golk::kTileBigCodes), codes, cap);
}

int gol_tile_window(int64_t modrows, int64_t pitch_words, int64_t y0, int32_t turns, int32_t tile_h,
                    int64_t *row0, int64_t *rows_a, int64_t *rows_b, uint64_t *base_a_bytes)
{
    if (!row0 || !rows_a || !rows_b || !base_a_bytes) return GOL_EINVAL;
    return golk::tile_window(modrows, pitch_words, y0, turns, tile_h, row0, rows_a, rows_b,
                             base_a_bytes)
               ? GOL_OK
               : GOL_EINVAL;
}

// (the product library has no K1p / K1q kernels: empty lists)
int gol_tile_persist_codes(int32_t *codes, int32_t cap)
{
    const int n = GOL_TOOLS ? (int)std::size(golk::kTilePersistCodes) : 0;
    return code_list(golk::kTilePersistCodes, n, codes, cap);
}

int gol_tile_stream_codes(int32_t *codes, int32_t cap)
{
    const int n = GOL_TOOLS ? (int)std::size(golk::kTileStreamCodes) : 0;
    return code_list(golk::kTileStreamCodes, n, codes, cap);
}

}  // extern "C"
