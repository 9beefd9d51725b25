// gol_step.cpp — gol_step / gol_step_overlap: what enqueues work and orders it.  The launches
// of a step, the streams they run on and the edges between them, the chunk pipeline, the
// read-job queue and the control word.  What runs is gol_plan.cpp's decision.
#include <algorithm>

#include "gol_ctx.h"

using namespace goleng;

namespace goleng {

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

// A cross-stream edge: what `waiter` is given from here on runs after everything queued on
// `signaller` so far.
int follow(gol_ctx *c, hipStream_t waiter, hipEvent_t ev, hipStream_t signaller)
{
    HIP_OR_FAIL(c, hipEventRecord(ev, signaller));
    HIP_OR_FAIL(c, hipStreamWaitEvent(waiter, ev, 0));
    return GOL_OK;
}

// A strip's interior output rows of a k-turn launch: their dependency cone stays inside the owned
// rows.  A launch split around the incoming halos runs them on the engine stream at once and the
// rows next to the halos on the side stream, at band edge_band.
bool has_interior(const gol_ctx *c, int k) { return 2 * k < c->cfg.rows; }
template <class F>
int launch_split(gol_ctx *c, golk::StepArgs a, int k, int edge_band, F &&launch)
{
    const int lo = a.row_lo, hi = a.row_hi;
    const int in_lo = c->cfg.halo + k, in_hi = c->cfg.halo + c->cfg.rows - k;
    a.row_lo = in_lo;
    a.row_hi = in_hi;
    HIP_OR_FAIL(c, launch(a, c->stream));
    a.band = edge_band;
    a.row_lo = lo;
    a.row_hi = in_lo;
    HIP_OR_FAIL(c, launch(a, c->side));
    a.row_lo = in_hi;
    a.row_hi = hi;
    HIP_OR_FAIL(c, launch(a, c->side));
    return GOL_OK;
}

// One launch of k > 1 turns as planned.  split: see launch_split; a launch without interior
// rows runs whole on the side stream.
int launch_multi(gol_ctx *c, golk::StepArgs a, const Launch &plan, bool cnt, bool split)
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
    auto launch = [k](const golk::StepArgs &b, hipStream_t s) {
        return golk::launch_step_multi(b, k, s);
    };
    if (blocks) {
        HIP_OR_FAIL(c, blocks_launch(c, a, plan));
    } else if (split && has_interior(c, k)) {
        // concurrent launches cannot share the published-row scratch
        if (a.multi_variant == golk::kMultiWgPg) a.multi_variant = golk::kMultiWgHx;
        if (a.multi_variant == golk::kMultiWgPgS) a.multi_variant = golk::kMultiWgHxS;
        // boundary rows: short bands so the few rows still spread over many waves
        return launch_split(c, a, k, std::min(c->shape.band_multi, golk::kOverlapBand), launch);
    } else {
        HIP_OR_FAIL(c, pg_prepare(c, a, k));
        HIP_OR_FAIL(c, launch(a, split ? c->side : c->stream));
    }
    return GOL_OK;
}

// One one-turn launch.  split: interior now, the 2 x (halo) boundary rows after the receives.
int launch_one(gol_ctx *c, golk::StepArgs a, bool cnt, bool split)
{
    a.blocked = c->blocked_pending ? c->blocked : nullptr;
    a.counts = cnt ? next_count_slot(c) : nullptr;           // (a split launch is never counted)
    auto launch = [c](const golk::StepArgs &b, hipStream_t s) {
        return golk::launch_step(b, c->fast, s);
    };
    if (split && has_interior(c, 1)) return launch_split(c, a, 1, a.band, launch);
    HIP_OR_FAIL(c, launch(a, split ? c->side : c->stream));
    return GOL_OK;
}

// ---------------------------------------------------------------- the chunked pipeline
// Consecutive k_step_tile launches of a long torus step, each cut into row chunks on tile-row
// boundaries (chunk_bounds) that alternate between the engine stream and c->side.  A chunk
// follows only the chunks of the launch before that chunk_deps names -- stream order where they
// ran on its own stream, else the latest of them on the other stream through its event -- so
// the tail, the store burst and the load burst of one chunk run under another chunk's turns
// (DESIGN.md "Launches overlapped in row chunks").  Events are waited on only after they were
// recorded, the device waits on nothing else, and the kernels are the plain launch's.  Which
// launches are cut, and where, is plan_chunks' decision (gol_plan.cpp).
struct ChunkPipe {
    bool live = false;           // c->side holds chunks the engine stream has not joined
    int parity = 0;              // the event set of the last chunked launch
    int k = 0;                   // its depth
    std::vector<int> bounds;     // its chunks' rows
    std::vector<int> pos;        // chunk -> place in the issue order
    std::vector<int> on_side;    // chunk -> ran on c->side
    long long issued = 0;        // chunks issued since the pipe went live (stream alternation)
};

hipEvent_t chunk_event(gol_ctx *c, int parity, int i)
{
    hipEvent_t &e = c->chunk_ev[parity][i];
    if (!e && hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) e = nullptr;
    return e;
}

// the engine stream joins the side stream: it waits for the side chunks of the last launch
// (stream order covers every earlier one; each chunk's event was recorded when it was issued)
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
        if (int rc = follow(c, c->side, c->ev_main, c->stream)) return rc;
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

// ---------------------------------------------------------------- one gol_step call
// What a gol_step / gol_step_overlap call fixes for all its launches, and its state between them.
struct StepCall {
    const int64_t turns;
    // gol_step_overlap: the stream of the caller's halo receives (gol_step: null).  The first
    // launch follows them (order_launch), split around the halos where it can be.
    const hipStream_t xstream;
    std::unique_lock<std::recursive_mutex> &lk;      // the engine lock (obey_control parks without it)
    ChunkPipe &pipe;                         // (step_impl's: it drains the streams after an error)
    const bool cnt;                          // per-turn counts
    const bool ctl;                          // a control word is in use: short queue, no chunks
    const int chunk_req;                     // chunk_request's answer for this call
    // a short torus step runs the sequence the autotune timed for exactly this many turns
    const std::vector<Launch> *const timed;
    size_t ti = 0;                           // the next launch of `timed`
    long long zero_hi;                       // count engines: see zero_count_slots
    EventRing ring;

    StepCall(gol_ctx *c, int64_t turns_, hipStream_t xstream_,
             std::unique_lock<std::recursive_mutex> &lk_, ChunkPipe &pipe_)
        : turns(turns_), xstream(xstream_), lk(lk_), pipe(pipe_),
          cnt((c->cfg.flags & GOL_FLAG_COUNT_EVERY_TURN) != 0), ctl(c->control_used.load()),
          chunk_req(chunk_request(c, ctl, xstream_ != nullptr)), timed(timed_sequence(c, turns_)),
          zero_hi(c->turn) {}
    const Launch *timed_next() const { return timed && ti < timed->size() ? &(*timed)[ti] : nullptr; }
    // the next launch: the timed sequence's while it lasts, else the planner's for `room` turns
    Launch take(gol_ctx *c, int64_t room)
    {
        return timed_next() ? (*timed)[ti++] : plan_launch(c, room);
    }
};

// The board in the layout a launch of depth k runs on and, for the first launch of an
// overlapped window (recv: the caller's receive stream, else null), the launch behind the
// receives.  The conversion reads the halo rows (a one-turn window on an engine of multi-turn
// launches: gol_halo_buffers handed out rows of this board), so it follows the receives too.
// A whole launch waits for them on the engine stream (with per-turn counts, or on a torus);
// a split launch's side stream follows the engine's queued work and the receives.
int order_launch(gol_ctx *c, hipStream_t recv, int k, bool split)
{
    const bool il = stepping_il(c, k);
    if (recv && c->il != il)
        if (int rc = follow(c, c->stream, c->ev_side, recv)) return rc;
    if (int rc = ensure_layout(c, il)) return rc;
    if (!recv) return GOL_OK;
    if (!split) return follow(c, c->stream, c->ev_side, recv);
    if (int rc = follow(c, c->side, c->ev_main, c->stream)) return rc;
    return follow(c, c->side, c->ev_side, recv);
}

// rows a launch of k turns computes: torus -> all; strip -> [s, buf_rows - s) when it ends at
// turn s since the exchange
void set_launch_rows(const gol_ctx *c, int k, golk::StepArgs &a)
{
    const int s = is_strip(c) ? c->cfg.halo - c->halo_valid + k : 0;
    a.row_lo = s;
    a.row_hi = c->buf_rows - s;
}

// the engine's books after a launch of plan.k turns went out
void commit_launch(gol_ctx *c, const Launch &plan, int64_t turns)
{
    const int k = plan.k;
    c->cur ^= 1;
    // a step of exactly one turn leaves the board one turn back in the other half, both in
    // the standard layout; a longer step never does for its caller, however it was cut
    // into launches (a board without multi-turn kernels runs it as one-turn launches)
    c->prev_valid = k == 1 && turns == 1;
    c->turn += k;
    c->progress.store(c->turn);
    c->launches += 1;
    if (c->last.size() < kLastCap) c->last.push_back(k > 1 ? plan : Launch{1, 0, c->band, 0, 0});
    ++c->last_n;
    if (is_strip(c)) c->halo_valid -= k;
    if (c->blocked_pending) {
        // every cell is 0/255 after the first turn; the mask is dead from here on
        c->blocked_pending = false;
        c->raw_turn0.clear();
    }
}

// Launch by launch: serve readers, obey control, plan, decide chunks, order, launch, commit,
// bound the queue.
int step_loop(gol_ctx *c, StepCall &&s)
{
    golk::StepArgs a = whole_buffer_args(c);
    a.band = c->band;
    a.multi_variant = c->shape.multi_variant;
    a.tile_w = c->shape.tile_w;
    a.tile_seg = c->shape.tile_seg;
    // a reader served during an earlier step does not shorten this one's queue: the bound
    // comes back when a reader is served during this step (a ticker's snapshot)
    c->readers.store(false);
    c->last.clear();
    c->last_n = 0;
    c->last_chunks = 0;
    for (int64_t t = 0; t < s.turns;) {
        if (c->jobs_pending.load(std::memory_order_relaxed)) {
            if (int rc = pipe_join(c, s.pipe)) return rc;    // readers use the engine stream
            serve_jobs(c);
        }
        if (s.ctl)                               // (a controlled engine never chunks)
            if (int rc = obey_control(c, s.lk, &s.zero_hi)) return rc;
        int64_t room = s.turns - t;
        if (is_strip(c)) room = std::min<int64_t>(room, c->halo_valid);
        const Launch plan = s.take(c, room);
        const int k = plan.k;
        // a launch is cut when the one before it was, or when the next one can be
        const std::vector<int> chunks = plan_chunks(c, plan, s.chunk_req, s.turns - t - k,
                                                    s.timed_next(), s.pipe.live ? s.pipe.k : 0);
        const bool chunked = chunks.size() > 2;
        if (!chunked)                            // a whole launch, a conversion: join first
            if (int rc = pipe_join(c, s.pipe)) return rc;
        // split this launch around the incoming halos (first launch of an overlapped step;
        // with per-turn counts the launch waits for the receives whole instead)
        const bool first = s.xstream && t == 0;
        const bool split = first && is_strip(c) && !s.cnt;
        if (int rc = order_launch(c, first ? s.xstream : nullptr, k, split)) return rc;
        set_launch_rows(c, k, a);
        a.in = c->board[c->cur];
        a.out = c->board[c->cur ^ 1];
        if (s.cnt)
            if (int rc = zero_count_slots(c, k, s.turns - t, &s.zero_hi)) return rc;
        if (int rc = chunked ? launch_chunked(c, s.pipe, a, plan, chunks)
                     : k > 1 ? launch_multi(c, a, plan, s.cnt, split)
                             : launch_one(c, a, s.cnt, split))
            return rc;
        if (split)     // join: the next launch overwrites rows the side launches read
            if (int rc = follow(c, c->stream, c->ev_side, c->side)) return rc;
        commit_launch(c, plan, s.turns);
        t += k;
        if (s.ctl || c->readers.load(std::memory_order_relaxed)) {
            if (int rc = pipe_join(c, s.pipe)) return rc;    // (the ring marks the engine stream)
            if (int rc = bound_queue(c, s.ring)) return rc;
        }
    }
    if (int rc = pipe_join(c, s.pipe)) return rc;
    if (c->blocked && !c->blocked_pending) {
        HIP_OR_FAIL(c, hipStreamSynchronize(c->stream));
        release_blocked(c);
    }
    return GOL_OK;
}

// gol_step / gol_step_overlap (xstream != null: see StepCall)
int step_impl(gol_ctx *c, int64_t turns, hipStream_t xstream,
              std::unique_lock<std::recursive_mutex> &lk)
{
    if (is_strip(c) && turns > c->halo_valid)
        return fail(c, GOL_ESTATE, "strip engine: %lld turns requested, halos valid for %d",
                    (long long)turns, c->halo_valid);
    DeviceGuard g(c->device);
    Stepping stepping(c);                        // (its destructor serves readers: after the join)
    ChunkPipe pipe;
    const int rc = step_loop(c, StepCall(c, turns, xstream, lk, pipe));
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
    return follow(c, (hipStream_t)stream, c->ev_main, c->stream);
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
