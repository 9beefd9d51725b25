// gol_step.cpp — the launch planner, gol_step / gol_step_overlap and the read-job queue.
#include <algorithm>
#include <cstdio>
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
    a.err = c->d_err;
    return a;
}

// The temporal-blocking kernel runs on the interleaved word layout (gol_kernels.h,
// multi_is_il); everything else -- the k = 1 stencils, PGM pack/unpack, the alive list,
// reads, loads, halo rows crossing the API -- sees the standard layout.  The engine
// converts lazily, whole buffer, when the next consumer needs the other layout (one read
// and one write of the board: at most twice per gol_step, never inside a run of
// multi-turn launches).  Popcounts do not depend on the layout.
int ensure_layout(gol_ctx *c, bool il)
{
    if (c->il == il) return GOL_OK;
    HIP_OR_FAIL(c, golk::launch_il_convert(c->board[c->cur], c->pitch, c->board[c->cur ^ 1],
                                           c->pitch, c->buf_rows, c->nw, il, c->stream));
    c->cur ^= 1;
    c->il = il;
    c->prev_valid = false;                   // the conversion overwrote the previous board
    return GOL_OK;
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
// a code with a counted instantiation (golk::kTileCountCodes); every other count engine -- K1s
// / K1w kernels, a GOL_TILE code without one, generic widths, blocking_limited,
// GOL_COUNT_BLOCKING=0 -- runs one-turn launches with the count fused into the stencil.
bool count_fused(const gol_ctx *c)
{
    return (c->cfg.flags & GOL_FLAG_COUNT_EVERY_TURN) && c->count_blocking && c->shape.tpl > 1 &&
           c->shape.multi_variant == golk::kMultiTile && golk::tile_code_counted(c->shape.tile_seg);
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
    if (!golk::multi_ok(c->cfg.width, k, s.multi_variant, s.tile_seg)) return L;
    return Launch{k, s.multi_variant, band_for_depth(c, k), s.tile_w, s.tile_seg};
}

// kMultiWgPg: the published-row scratch and flags for a launch of `a`, grown on demand (the
// engine's streams are drained first: a running launch may still use the old buffers), and
// a fresh epoch.  Other variants, and bands the kernel runs as kMultiWgHx, need nothing.
hipError_t pg_prepare(gol_ctx *c, golk::StepArgs &a, int k)
{
    a.xrows = nullptr;
    a.xflags = nullptr;
    if (!golk::is_pg_variant(a.multi_variant) ||
        !golk::pg_ok(k, a.band, a.multi_variant == golk::kMultiWgPgS))
        return hipSuccess;
    if (!device_exclusive(c->device)) {      // (launch_wg runs it as plain helix bands)
        a.multi_variant = a.multi_variant == golk::kMultiWgPgS ? golk::kMultiWgHxS
                                                               : golk::kMultiWgHx;
        return hipSuccess;
    }
    const long long T =
        golk::multi_pipes(a.width, a.row_hi - a.row_lo, a.band, 2, a.multi_variant);
    const size_t lanes = (size_t)T * 62 + 64;
    if (lanes > c->pg_lanes || (size_t)T > c->pg_tiles) {
        if (2ull * golk::kPgStages * lanes * 8 >= (1ull << 31)) return hipSuccess;   // helix
        hipError_t e = hipStreamSynchronize(c->stream);
        if (e == hipSuccess && c->side) e = hipStreamSynchronize(c->side);
        if (e != hipSuccess) return e;
        if (c->pg_rows) (void)hipFree(c->pg_rows);
        if (c->pg_flags) (void)hipFree(c->pg_flags);
        c->pg_rows = nullptr;
        c->pg_flags = nullptr;
        c->pg_lanes = c->pg_tiles = 0;
        e = hipExtMallocWithFlags((void **)&c->pg_rows, 2ull * golk::kPgStages * lanes * 8,
                                  hipDeviceMallocUncached);
        if (e == hipSuccess)
            e = hipExtMallocWithFlags((void **)&c->pg_flags,
                                      (size_t)T * golk::kPgStages * sizeof(unsigned),
                                      hipDeviceMallocUncached);
        if (e == hipSuccess)
            e = hipMemset(c->pg_flags, 0, (size_t)T * golk::kPgStages * sizeof(unsigned));
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) return e;
        c->pg_lanes = lanes;
        c->pg_tiles = (size_t)T;
    }
    a.xrows = c->pg_rows;
    a.xflags = c->pg_flags;
    a.xlanes = (unsigned)c->pg_lanes;
    a.epoch = ++c->pg_epoch;
    return hipSuccess;
}

}  // namespace goleng

namespace {

// Serve the read-only calls posted by run_read (the stepping thread, holding `mu`).
void serve_jobs(gol_ctx *c)
{
    std::vector<Job *> js;
    {
        std::lock_guard<std::mutex> jl(c->jm);
        js.swap(c->jobs);
        c->jobs_pending.store(false);
    }
    for (Job *j : js) {
        const int rc = j->fn();
        std::lock_guard<std::mutex> jl(c->jm);
        j->rc = rc;
        j->done = true;                      // (j lives on the waiter's stack: not touched again)
    }
    if (!js.empty()) c->jcv.notify_all();
}

void set_stepping(gol_ctx *c, bool on)
{
    std::lock_guard<std::mutex> jl(c->jm);
    c->stepping = on;
}

#if GOL_TOOLS
// Tools build only (GOL_MULTI_VARIANT=kMultiWgDiag): one k_step_wg launch with per-wave wait
// timing, summarised by wave role on stderr.  (C linkage: the library exports this name.)
extern "C" int wg_diag_launch(gol_ctx *c, golk::StepArgs a, int k)
{
    const long long ntx = golk::multi_tiles(c->cfg.width, 2);
    const long long pipes = ntx * ((a.row_hi - a.row_lo + a.band - 1) / a.band);
    const size_t n = (size_t)pipes * 4 * 10;
    unsigned long long *d = nullptr;
    HIP_OR_FAIL(c, hipMalloc(&d, n * 8));
    HIP_OR_FAIL(c, hipMemsetAsync(d, 0, n * 8, c->stream));
    a.counts = d;
    HIP_OR_FAIL(c, golk::launch_step_multi(a, k, c->stream));
    std::vector<unsigned long long> h(n);
    HIP_OR_FAIL(c, hipMemcpyAsync(h.data(), d, n * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_OR_FAIL(c, hipStreamSynchronize(c->stream));
    (void)hipFree(d);
    unsigned long long t0min = ~0ull, t1max = 0;
    std::vector<unsigned long long> starts, ends;        // wave 0's start / wave 3's end
    for (long long p = 0; p < pipes; ++p)
        for (int w = 0; w < 4; ++w) {
            const unsigned long long *e = &h[((size_t)p * 4 + w) * 10];
            if (e[8] == 0) continue;                     // a workgroup past the last band
            t0min = std::min(t0min, e[8]);
            t1max = std::max(t1max, e[9]);
            if (w == 0) starts.push_back(e[8]);
            if (w == 3) ends.push_back(e[9]);
        }
    auto pct = [](std::vector<unsigned long long> v, unsigned long long base, double q) {
        if (v.empty()) return 0.0;
        std::sort(v.begin(), v.end());
        return (double)(v[(size_t)(q * (double)(v.size() - 1))] - base);
    };
    fprintf(stderr,
            "wg_diag starts (100 MHz ticks after the first) p10 %.0f p50 %.0f p90 %.0f max %.0f; "
            "ends p10 %.0f p50 %.0f p90 %.0f max %.0f\n",
            pct(starts, t0min, 0.1), pct(starts, t0min, 0.5), pct(starts, t0min, 0.9),
            pct(starts, t0min, 1.0), pct(ends, t0min, 0.1), pct(ends, t0min, 0.5),
            pct(ends, t0min, 0.9), pct(ends, t0min, 1.0));
    for (int w = 0; w < 4; ++w) {
        double life = 0, first = 0, fw = 0, nf = 0, ew = 0, ne = 0, nl = 0;
        for (long long p = 0; p < pipes; ++p) {
            const unsigned long long *e = &h[((size_t)p * 4 + w) * 10];
            life += (double)e[0]; first += (double)e[1]; fw += (double)e[2];
            nf += (double)e[3]; ew += (double)e[4]; ne += (double)e[5]; nl += (double)e[6];
        }
        fprintf(stderr,
                "wg_diag K=%d band=%d pipes=%lld wave %d: life %.0f ticks, first-row wait %.1f%%, "
                "fetch waits %.1f%% (%.2f per row), emit waits %.1f%% (%.2f per row)\n",
                k, a.band, pipes, w, life / pipes, 100 * first / life, 100 * fw / life, nf / nl,
                100 * ew / life, ne / nl);
    }
    fprintf(stderr, "wg_diag launch span %llu ticks of 100 MHz\n", t1max - t0min);
    return GOL_OK;
}
#endif  // GOL_TOOLS

constexpr int kCtlDepth = 2;   // launches queued ahead while a control word is in use

// read-only calls from other threads are served at launch boundaries while one of these lives
struct Stepping {
    gol_ctx *c;
    explicit Stepping(gol_ctx *c_) : c(c_) { set_stepping(c, true); }
    ~Stepping()
    {
        set_stepping(c, false);              // later readers take the lock themselves
        serve_jobs(c);
    }
};

// control word: with a controlling thread present, keep at most kCtlDepth launches
// queued so a pause / stop takes effect within that many launches (and so does a reader:
// once one has been served during a step, steps keep the queue this short)
struct EventRing {
    hipEvent_t ev[kCtlDepth] = {};
    int n = 0;
    ~EventRing()
    {
        for (int i = 0; i < std::min(n, kCtlDepth); ++i) (void)hipEventDestroy(ev[i]);
    }
};

// bound the queue: wait for the launch kCtlDepth back, then mark this one
int bound_queue(gol_ctx *c, EventRing &ring)
{
    hipEvent_t &e = ring.ev[ring.n % kCtlDepth];
    if (ring.n >= kCtlDepth) {
        HIP_OR_FAIL(c, hipEventSynchronize(e));
        if (int rc = check_dev_err(c)) return rc;
    } else {
        HIP_OR_FAIL(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    HIP_OR_FAIL(c, hipEventRecord(e, c->stream));
    ++ring.n;
    return GOL_OK;
}

// The control word at a launch boundary: GOL_OK to go on, GOL_STOPPED, or an error.
int obey_control(gol_ctx *c, std::unique_lock<std::recursive_mutex> &lk, long long *zero_hi)
{
    int w = c->control.load();
    if (w == GOL_CONTROL_PAUSE) {
        // park at this launch boundary with the board complete (Server/gol/
        // distributor.go:147-156: the turn loop blocks until the second 'p'); the
        // engine is released while parked, so AliveCellsCount / GetWorld calls from
        // other threads run at once (the reference's ticker keeps firing while paused,
        // Local/gol/distributor.go:117-130,154-167)
        if (int rc = sync_checked(c)) return rc;
        set_stepping(c, false);
        serve_jobs(c);
        c->parked.store(true);
        lk.unlock();
        while ((w = c->control.load()) == GOL_CONTROL_PAUSE)
            std::this_thread::sleep_for(std::chrono::microseconds(200));
        lk.lock();
        *zero_hi = c->turn;                  // (the engine was released: zero again from here)
        set_stepping(c, true);
        c->parked.store(false);
    }
    // quit / kill (distributor.go:143-146,157-164)
    return w == GOL_CONTROL_STOP ? GOL_STOPPED : GOL_OK;
}

// Count engines: zero the count slots of a launch's turns c->turn + 1 .. c->turn + k (zero_hi:
// the last turn whose slot this step has zeroed; `left`: the turns the step still has to run).
// One memset clears from the first slot not yet zeroed to the end of its batch of kRingAhead
// slots (a batch never wraps the ring), but no further than the step's last turn and never
// past turn c->turn + kRingAhead: the slots up to there hold turns <= c->turn - kRing, which
// gol_turn_counts no longer accepts, now or at any later launch boundary.  A launch that
// straddles a batch boundary takes a second memset (k <= kRingAhead).
int zero_count_slots(gol_ctx *c, int k, int64_t left, long long *zero_hi)
{
    *zero_hi = std::max(*zero_hi, c->turn);
    while (*zero_hi < c->turn + k) {
        const long long z = *zero_hi + 1;
        const size_t slot = (size_t)(z % kRingSlots);
        const long long e = std::min({z + (long long)(kRingAhead - slot % kRingAhead) - 1,
                                      c->turn + (long long)kRingAhead,
                                      c->turn + (long long)left});
        HIP_OR_FAIL(c, hipMemsetAsync(c->counts + slot * kShards, 0,
                                      (size_t)(e - z + 1) * kShards * 8, c->stream));
        *zero_hi = e;
    }
    return GOL_OK;
}

// the count slot of the engine's next turn
unsigned long long *next_count_slot(gol_ctx *c)
{
    return c->counts + (size_t)((c->turn + 1) % kRingSlots) * kShards;
}

// One launch of k > 1 turns as planned.  split: the interior output rows [in_lo, in_hi) on the
// engine stream at once, the rows next to the halos on the side stream.
int launch_multi(gol_ctx *c, golk::StepArgs a, const Launch &plan, bool cnt, bool split,
                 int in_lo, int in_hi)
{
    const int k = plan.k;
    a.blocked = nullptr;
    // (a count engine's multi-turn launch: k_step_tile_cnt, k consecutive slots --
    // plan_launch stops at the ring's end)
    a.counts = cnt ? next_count_slot(c) : nullptr;
    a.band = plan.band;
    a.multi_variant = plan.var;
    const bool blocks = plan.var == golk::kMultiTilePersist || plan.var == golk::kMultiTileStream;
    if (plan.var == golk::kMultiTile || blocks) {
        a.tile_w = plan.tw;
        a.tile_seg = plan.seg;
    }
#if GOL_TOOLS
    if (c->shape.multi_variant == golk::kMultiWgDiag && !split) return wg_diag_launch(c, a, k);
#endif
    if (blocks) {
        HIP_OR_FAIL(c, blocks_launch(c, a, plan));
    } else if (split && in_lo < in_hi) {
        golk::StepArgs b = a;
        // concurrent launches cannot share the published-row scratch
        if (b.multi_variant == golk::kMultiWgPg) b.multi_variant = golk::kMultiWgHx;
        if (b.multi_variant == golk::kMultiWgPgS) b.multi_variant = golk::kMultiWgHxS;
        b.row_lo = in_lo;
        b.row_hi = in_hi;
        HIP_OR_FAIL(c, golk::launch_step_multi(b, k, c->stream));
        // boundary rows: short bands so the few rows still spread over many waves
        b.band = std::min(c->shape.band_multi, golk::kOverlapBand);
        b.row_lo = a.row_lo;
        b.row_hi = in_lo;
        HIP_OR_FAIL(c, golk::launch_step_multi(b, k, c->side));
        b.row_lo = in_hi;
        b.row_hi = a.row_hi;
        HIP_OR_FAIL(c, golk::launch_step_multi(b, k, c->side));
    } else {
        HIP_OR_FAIL(c, pg_prepare(c, a, k));
        HIP_OR_FAIL(c, golk::launch_step_multi(a, k, split ? c->side : c->stream));
    }
    return GOL_OK;
}

// One one-turn launch.  split: interior now, the 2 x (halo) boundary rows after the receives.
int launch_one(gol_ctx *c, golk::StepArgs a, bool cnt, bool split, int in_lo, int in_hi)
{
    a.blocked = c->blocked_pending ? c->blocked : nullptr;
    if (!split) {
        a.counts = cnt ? next_count_slot(c) : nullptr;
        HIP_OR_FAIL(c, golk::launch_step(a, c->fast, c->stream));
        return GOL_OK;
    }
    a.counts = nullptr;
    golk::StepArgs b = a;
    if (in_lo < in_hi) {
        b.row_lo = in_lo;
        b.row_hi = in_hi;
        HIP_OR_FAIL(c, golk::launch_step(b, c->fast, c->stream));
        b.row_lo = a.row_lo;
        b.row_hi = in_lo;
        HIP_OR_FAIL(c, golk::launch_step(b, c->fast, c->side));
        b.row_lo = in_hi;
        b.row_hi = a.row_hi;
        HIP_OR_FAIL(c, golk::launch_step(b, c->fast, c->side));
    } else {
        HIP_OR_FAIL(c, golk::launch_step(a, c->fast, c->side));
    }
    return GOL_OK;
}

// ---------------------------------------------------------------- the chunked pipeline
// Consecutive k_step_tile launches of a long torus step, each cut into row chunks on tile-row
// boundaries (chunk_bounds) that alternate between the engine stream and c->side.  A chunk
// follows only the chunks of the launch before that chunk_deps names -- stream order where they
// ran on its own stream, else the latest of them on the other stream through its event -- so
// the tail, the store burst and the load burst of one chunk run under another chunk's turns
// (DESIGN.md "Launches overlapped in row chunks").  Events are waited on only after they were
// recorded, the device waits on nothing else, and the kernels are the plain launch's.
//
// Chunks per launch in automatic mode: launches of at least kChunkMinRounds rounds of the
// resident workgroups (CUs x tile_blocks_per_cu) get chunks of about kChunkRounds rounds.
// 65536^2 (9.7 rounds per K = 30 launch), 960 turns, median of 3 alternating passes on one
// box, k GCUPS by chunks per launch: 1: 131.8, 3: 125.9 (every chunk follows every chunk),
// 4: 138.7, 5: 139.5, 6: 137.9, 7: 137.4, 8: 136.5, 10: 136.8, 20: 125.7
// (profiles/chunk_overlap_ab.log) -- 5 chunks of 1.9 rounds.  A third stream was level at
// best (5: 138.7, 8: 137.9, 10: 137.8) and is not built.
constexpr int kChunkMinRounds = 4;
constexpr double kChunkRounds = 2.0;

struct ChunkPipe {
    bool live = false;           // c->side holds chunks the engine stream has not joined
    int parity = 0;              // the event set of the last chunked launch
    int k = 0;                   // its depth
    std::vector<int> bounds;     // its chunks' rows
    std::vector<int> pos;        // chunk -> place in the issue order
    std::vector<int> on_side;    // chunk -> ran on c->side
    long long issued = 0;        // chunks issued since the pipe went live (stream alternation)
};

// GOL_STEP_CHUNKS, read per gol_step: 1 = off, n >= 2 = n chunks, unset / 0 = automatic (-1)
int chunk_request()
{
    const char *env = getenv("GOL_STEP_CHUNKS");
    const int n = env ? atoi(env) : 0;
    return n <= 0 ? -1 : std::min(n, kMaxStepChunks);
}

// a launch the pipeline may cut (request: chunk_request's, once per step)
bool chunk_eligible(const gol_ctx *c, const Launch &L, int request, bool cnt, bool ctl,
                    hipStream_t xstream)
{
    return request != 1 && L.k > 1 && L.var == golk::kMultiTile && !is_strip(c) && !cnt &&
           !c->blocked_pending && !xstream && !ctl && c->side &&
           !c->readers.load(std::memory_order_relaxed);
}

int chunks_wanted(const gol_ctx *c, const Launch &L, int request)
{
    if (request > 0) return request;
    const long long wg =
        golk::tile_grid(c->nw, c->buf_rows, L.k, L.band, L.tw, L.seg).tiles();
    const long long slots =
        (long long)c->ncu * golk::tile_blocks_per_cu(L.k, L.band, L.tw, L.seg, c->cfg.width);
    if (slots <= 0 || wg < kChunkMinRounds * slots) return 1;
    return (int)std::min<long long>(kMaxStepChunks,
                                    std::max(2ll, (long long)((double)wg / (kChunkRounds * (double)slots) + 0.5)));
}

hipEvent_t chunk_event(gol_ctx *c, int parity, int i)
{
    hipEvent_t &e = c->chunk_ev[parity][i];
    if (!e && hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) e = nullptr;
    return e;
}

// the engine stream joins the side stream: it waits for the side chunks of the last launch
// (stream order covers every earlier one)
int pipe_join(gol_ctx *c, ChunkPipe &p)
{
    if (!p.live) return GOL_OK;
    for (size_t q = 0; q < p.on_side.size(); ++q)
        if (p.on_side[q])
            HIP_OR_FAIL(c, hipStreamWaitEvent(c->stream, c->chunk_ev[p.parity][q], 0));
    p.live = false;
    return GOL_OK;
}

// One launch of plan.k turns as the chunks `bounds` (>= 2).  a: the whole-buffer arguments with
// the boards set.
int launch_chunked(gol_ctx *c, ChunkPipe &p, golk::StepArgs a, const Launch &plan,
                   const std::vector<int> &bounds)
{
    const int n = (int)bounds.size() - 1;
    a.blocked = nullptr;
    a.counts = nullptr;
    a.band = plan.band;
    a.multi_variant = plan.var;
    a.tile_w = plan.tw;
    a.tile_seg = plan.seg;
    std::vector<std::vector<int>> deps(n);
    std::vector<int> order(n), ready(n, -1);
    for (int q = 0; q < n; ++q) order[q] = q;
    if (p.live) {
        deps = chunk_deps(c->buf_rows, p.bounds, p.k, bounds, plan.k);
        // first the chunks whose last dependency was issued first
        for (int q = 0; q < n; ++q)
            for (int d : deps[q]) ready[q] = std::max(ready[q], p.pos[d]);
        std::stable_sort(order.begin(), order.end(),
                         [&](int x, int y) { return ready[x] < ready[y]; });
    } else {
        // the side stream starts behind everything queued on the engine stream
        HIP_OR_FAIL(c, hipEventRecord(c->ev_main, c->stream));
        HIP_OR_FAIL(c, hipStreamWaitEvent(c->side, c->ev_main, 0));
        p.issued = 0;
    }
    const int par = p.live ? p.parity ^ 1 : 0;
    std::vector<int> pos(n), on_side(n);
    for (int i = 0; i < n; ++i) {
        const int q = order[i];
        const int side = (int)(p.issued++ & 1);
        hipStream_t s = side ? c->side : c->stream;
        // the latest dependency on the other stream (same stream: stream order)
        int far = -1;
        for (int d : deps[q])
            if (p.on_side[d] != side && (far < 0 || p.pos[d] > p.pos[far])) far = d;
        if (far >= 0) HIP_OR_FAIL(c, hipStreamWaitEvent(s, c->chunk_ev[p.parity][far], 0));
        golk::StepArgs b = a;
        b.row_lo = bounds[q];
        b.row_hi = bounds[q + 1];
        HIP_OR_FAIL(c, golk::launch_step_multi(b, plan.k, s));
        hipEvent_t e = chunk_event(c, par, q);
        if (!e) return fail(c, GOL_EHIP, "hipEventCreate failed for a chunk event");
        HIP_OR_FAIL(c, hipEventRecord(e, s));
        pos[q] = i;
        on_side[q] = side;
    }
    p.live = true;
    p.parity = par;
    p.k = plan.k;
    p.bounds = bounds;
    p.pos = std::move(pos);
    p.on_side = std::move(on_side);
    c->last_chunks += n;
    return GOL_OK;
}

// gol_step / gol_step_overlap.  xstream != null: the first launch is split -- the rows
// whose k-turn dependency cone stays inside the owned rows run on the engine stream at
// once, the rows next to the halos run on the side stream after everything queued on
// xstream (the caller's halo receives) -- and the engine stream joins the side stream
// before the next launch.  `pipe`: the chunked pipeline's state; the caller joins it.
int step_loop(gol_ctx *c, int64_t turns, hipStream_t xstream,
              std::unique_lock<std::recursive_mutex> &lk, ChunkPipe &pipe)
{
    const bool cnt = (c->cfg.flags & GOL_FLAG_COUNT_EVERY_TURN) != 0;
    golk::StepArgs a = whole_buffer_args(c);
    a.band = c->band;
    a.multi_variant = c->shape.multi_variant;
    a.tile_w = c->shape.tile_w;
    a.tile_seg = c->shape.tile_seg;
    EventRing ring;
    const int chunk_req = chunk_request();
    const bool ctl = c->control_used.load();
    // a reader served during an earlier step does not shorten this one's queue: the bound
    // comes back when a reader is served during this step (a ticker's snapshot)
    c->readers.store(false);
    // a short torus step runs the sequence the autotune timed for exactly this many turns
    const auto &seq = c->shape.seq;
    const std::vector<Launch> *fixed =
        !is_strip(c) && !cnt && !c->blocked_pending && turns >= 2 && turns <= kSeqMax &&
                turns < (int64_t)seq.size() && !seq[turns].empty()
            ? &seq[turns]
            : nullptr;
    size_t fi = 0;
    long long zero_hi = c->turn;             // count engines: see zero_count_slots
    c->last.clear();
    c->last_n = 0;
    c->last_chunks = 0;
    for (int64_t t = 0; t < turns;) {
        if (c->jobs_pending.load(std::memory_order_relaxed)) {
            if (int rc = pipe_join(c, pipe)) return rc;      // readers use the engine stream
            serve_jobs(c);
        }
        if (ctl)                                 // (a controlled engine never chunks)
            if (int rc = obey_control(c, lk, &zero_hi)) return rc;
        int64_t room = turns - t;
        if (is_strip(c)) room = std::min<int64_t>(room, c->halo_valid);
        const Launch plan = fixed && fi < fixed->size() ? (*fixed)[fi++] : plan_launch(c, room);
        const int k = plan.k;
        // The chunked pipeline: a launch is cut when the one before it was, or when the next
        // one can be (a lone launch stays one kernel).  Its chunks are fixed here, at least as
        // tall as its own and both neighbours' depths.
        std::vector<int> chunks;
        const int want = chunk_eligible(c, plan, chunk_req, cnt, ctl, xstream)
                             ? chunks_wanted(c, plan, chunk_req)
                             : 1;
        if (want > 1) {                          // (a board too small for chunks plans nothing more)
            // (the next launch as planned from here, before this one has advanced the engine: a
            // prediction that only decides whether to start a pipeline and how tall the chunks
            // are -- chunk_deps is right for any bounds, so a wrong guess costs overlap alone)
            int k_next = 0;
            if (turns - t - k >= 2) {
                const Launch nx = fixed && fi < fixed->size() ? (*fixed)[fi]
                                                              : plan_launch(c, turns - t - k);
                if (chunk_eligible(c, nx, chunk_req, cnt, ctl, xstream) &&
                    chunks_wanted(c, nx, chunk_req) > 1)
                    k_next = nx.k;
            }
            if (pipe.live || k_next)
                chunks = chunk_bounds(c->buf_rows, plan.band, want,
                                      std::max({k, k_next, pipe.live ? pipe.k : 0}));
        }
        const bool chunked = chunks.size() > 2;
        if (!chunked)                            // a whole launch, a conversion: join first
            if (int rc = pipe_join(c, pipe)) return rc;
        // rows computed: torus -> all; strip -> [s, buf_rows - s) after turn s since exchange
        const int s0 = is_strip(c) ? c->cfg.halo - c->halo_valid : 0;
        if (is_strip(c)) {
            a.row_lo = s0 + k;
            a.row_hi = c->buf_rows - s0 - k;
        } else {
            a.row_lo = 0;
            a.row_hi = c->buf_rows;
        }
        // an overlapped window whose first launch runs on the other word layout (a one-turn
        // window on an engine of multi-turn launches): the conversion reads the halo rows, so
        // it follows the caller's receives -- gol_halo_buffers handed out rows of this board
        if (xstream && t == 0 && c->il != stepping_il(c, k)) {
            HIP_OR_FAIL(c, hipEventRecord(c->ev_side, xstream));
            HIP_OR_FAIL(c, hipStreamWaitEvent(c->stream, c->ev_side, 0));
        }
        if (int rc = ensure_layout(c, stepping_il(c, k))) return rc;
        a.in = c->board[c->cur];
        a.out = c->board[c->cur ^ 1];
        // split this launch around the incoming halos (first launch of an overlapped step;
        // with per-turn counts the launch waits for the receives whole instead)
        const bool split = xstream && t == 0 && is_strip(c) && !cnt;
        if (xstream && t == 0 && !split) {
            HIP_OR_FAIL(c, hipEventRecord(c->ev_side, xstream));
            HIP_OR_FAIL(c, hipStreamWaitEvent(c->stream, c->ev_side, 0));
        }
        const int H = c->cfg.halo;
        const int in_lo = H + k, in_hi = H + c->cfg.rows - k;   // interior output rows
        if (split) {
            // side stream: after the caller's receives (and the engine's queued work)
            HIP_OR_FAIL(c, hipEventRecord(c->ev_main, c->stream));
            HIP_OR_FAIL(c, hipStreamWaitEvent(c->side, c->ev_main, 0));
            HIP_OR_FAIL(c, hipEventRecord(c->ev_side, xstream));
            HIP_OR_FAIL(c, hipStreamWaitEvent(c->side, c->ev_side, 0));
        }
        if (cnt)
            if (int rc = zero_count_slots(c, k, turns - t, &zero_hi)) return rc;
        if (int rc = chunked ? launch_chunked(c, pipe, a, plan, chunks)
                     : k > 1 ? launch_multi(c, a, plan, cnt, split, in_lo, in_hi)
                             : launch_one(c, a, cnt, split, in_lo, in_hi))
            return rc;
        if (split) {   // join: the next launch overwrites rows the side launches read
            HIP_OR_FAIL(c, hipEventRecord(c->ev_side, c->side));
            HIP_OR_FAIL(c, hipStreamWaitEvent(c->stream, c->ev_side, 0));
        }
        c->cur ^= 1;
        // a step of exactly one turn leaves the board one turn back in the other half, both in
        // the standard layout; a longer step never does for its caller, however it was cut
        // into launches (a board without multi-turn kernels runs it as one-turn launches)
        c->prev_valid = k == 1 && turns == 1;
        c->turn += k;
        c->progress.store(c->turn);
        c->launches += 1;
        if (c->last.size() < kLastCap)
            c->last.push_back(k > 1 ? plan : Launch{1, 0, c->band, 0, 0});
        ++c->last_n;
        t += k;
        if (is_strip(c)) c->halo_valid -= k;
        if (c->blocked_pending) {
            // every cell is 0/255 after the first turn; the mask is dead from here on
            c->blocked_pending = false;
            c->raw_turn0.clear();
        }
        if (ctl || c->readers.load(std::memory_order_relaxed)) {
            if (int rc = pipe_join(c, pipe)) return rc;      // (the ring marks the engine stream)
            if (int rc = bound_queue(c, ring)) return rc;
        }
    }
    if (int rc = pipe_join(c, pipe)) return rc;
    if (c->blocked && !c->blocked_pending) {
        HIP_OR_FAIL(c, hipStreamSynchronize(c->stream));
        release_blocked(c);
    }
    return GOL_OK;
}

// (C linkage: the library exports this name.)
extern "C" int step_impl(gol_ctx *c, int64_t turns, hipStream_t xstream,
              std::unique_lock<std::recursive_mutex> &lk)
{
    if (is_strip(c) && turns > c->halo_valid)
        return fail(c, GOL_ESTATE, "strip engine: %lld turns requested, halos valid for %d",
                    (long long)turns, c->halo_valid);
    DeviceGuard g(c->device);
    Stepping stepping(c);                        // (its destructor serves readers: after the join)
    ChunkPipe pipe;
    const int rc = step_loop(c, turns, xstream, lk, pipe);
    if (rc < 0 && pipe.issued > 0) {
        // an error after chunks went out on both streams: drain them before the caller sees it
        (void)hipStreamSynchronize(c->side);
        (void)hipStreamSynchronize(c->stream);
    }
    return rc;
}

}  // namespace

// ================================================================ C ABI
extern "C" {

int gol_step(gol_ctx *c, int64_t turns)
{
    if (!c || turns < 0) return GOL_EINVAL;
    std::unique_lock<std::recursive_mutex> lk(c->mu);
    return step_impl(c, turns, nullptr, lk);
}

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

int gol_tile_codes(int32_t *codes, int32_t cap)
{
    const int n = (int)std::size(golk::kTileCodes);
    if (cap < 0 || (cap > 0 && !codes)) return GOL_EINVAL;
    for (int i = 0; i < std::min(n, (int)cap); ++i) codes[i] = golk::kTileCodes[i];
    return n;
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

int gol_tile_count_codes(int32_t *codes, int32_t cap)
{
    const int n = (int)std::size(golk::kTileCountCodes);
    if (cap < 0 || (cap > 0 && !codes)) return GOL_EINVAL;
    for (int i = 0; i < std::min(n, (int)cap); ++i) codes[i] = golk::kTileCountCodes[i];
    return n;
}

int gol_tile_seam_codes(int32_t *codes, int32_t cap)
{
    const int n = (int)std::size(golk::kTileSeamCodes);
    if (cap < 0 || (cap > 0 && !codes)) return GOL_EINVAL;
    for (int i = 0; i < std::min(n, (int)cap); ++i) codes[i] = golk::kTileSeamCodes[i];
    return n;
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

int gol_tile_persist_codes(int32_t *codes, int32_t cap)
{
    const int n = GOL_TOOLS ? (int)std::size(golk::kTilePersistCodes) : 0;   // (tools build)
    if (cap < 0 || (cap > 0 && !codes)) return GOL_EINVAL;
    for (int i = 0; i < std::min(n, (int)cap); ++i) codes[i] = golk::kTilePersistCodes[i];
    return n;
}

int gol_tile_stream_codes(int32_t *codes, int32_t cap)
{
    const int n = GOL_TOOLS ? (int)std::size(golk::kTileStreamCodes) : 0;   // (tools build)
    if (cap < 0 || (cap > 0 && !codes)) return GOL_EINVAL;
    for (int i = 0; i < std::min(n, (int)cap); ++i) codes[i] = golk::kTileStreamCodes[i];
    return n;
}

int gol_step_overlap(gol_ctx *c, int64_t turns, void *recv_stream)
{
    if (!c || turns < 0 || !recv_stream) return GOL_EINVAL;
    std::unique_lock<std::recursive_mutex> lk(c->mu);
    if (!is_strip(c)) return fail(c, GOL_ESTATE, "not a strip engine");
    c->halo_valid = c->cfg.halo;   // the receives queued on recv_stream refresh the halos
    return step_impl(c, turns, (hipStream_t)recv_stream, lk);
}

int gol_stream_wait(gol_ctx *c, void *stream)
{
    if (!c || !stream) return GOL_EINVAL;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    DeviceGuard g(c->device);
    HIP_OR_FAIL(c, hipEventRecord(c->ev_main, c->stream));
    HIP_OR_FAIL(c, hipStreamWaitEvent((hipStream_t)stream, c->ev_main, 0));
    return GOL_OK;
}

int gol_set_control(gol_ctx *c, int32_t word)
{
    if (!c || word < GOL_CONTROL_RUN || word > GOL_CONTROL_STOP) return GOL_EINVAL;
    c->control_used.store(true);
    c->control.store(word);
    return GOL_OK;
}

int gol_get_progress(gol_ctx *c, int64_t *turn, int32_t *parked)
{
    if (!c) return GOL_EINVAL;
    if (turn) *turn = c->progress.load();
    if (parked) *parked = c->parked.load() ? 1 : 0;
    return GOL_OK;
}

}  // extern "C"
