// gol_ctx.h — the engine's state and what its translation units call across files (internal:
// not part of the C ABI in include/gol_amd.h).
//
//   gol_engine.cpp   create / destroy, info, the pinned-shape table and its check, the
//                    per-device engine registry, errors
//   gol_tune.cpp     the k_step_tile model and search, the create-time autotune, the tune cache
//   gol_plan.cpp     the launch planner (kernel, depth, band, row chunks) and the calls that
//                    report plans and tables; no stream or event call
//   gol_step.cpp     gol_step / gol_step_overlap: launches, stream and event ordering, the chunk
//                    pipeline, the read-job queue, the control word
//   gol_io.cpp       load, read-out, counts, alive and flip lists, windows (gol_window.h)
//   gol_halo.cpp     halo exchange
//   gol_blocks.cpp   K1p / K1q / K1r host side and the k_step_wg wait diagnostic (tools build;
//                    stubs in the product)
//
// One gol_ctx = one MI355X holding either the whole torus board or one row
// strip of it (the reference's SubServer strip, Server/gol/distributor.go:
// 106-116 split; here the strip lives on the GPU for the whole run and only
// `halo` boundary rows move between strips every `halo` turns).
//
// Device memory per engine (owned here, freed in gol_destroy):
//   board[2]   double-buffered packed board, buffer_rows x pitch uint64
//   blocked    packed mask of the cells that were neither 0 nor 255 at load
//              (only while turn 1 is pending; reference quirk,
//              SubServer/distributor.go:178-200 + :122-125)
//   counts     popcount shards (kShards u64) x kRingSlots slots for the per-turn
//              series (GOL_FLAG_COUNT_EVERY_TURN) and one slot for snapshots
//   staging    byte / alive-list staging, allocated on demand
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <tuple>
#include <vector>

#include "gol_amd.h"
#include "gol_kernels.h"
#include "gol_internal.h"

using golk::kShards;

constexpr int kRing = 4096;                 // per-turn counts kept: gol_turn_counts' window
// The ring has kRingAhead more slots than the window (turn t -> slot t % kRingSlots): a step
// zeroes the slots of up to kRingAhead coming turns in one memset, and those slots hold turns
// <= turn + kRingAhead - kRingSlots = turn - kRing, already outside the window.  So a reader
// served in the middle of a step, or after a step that GOL_CONTROL_STOP cut short, never sees
// a zeroed slot for a turn the window accepts.
constexpr int kRingAhead = 256;
constexpr int kRingSlots = kRing + kRingAhead;
static_assert(kRingSlots % kRingAhead == 0, "a batch of zeroed slots never wraps the ring");

// one temporal-blocking launch: depth, kernel (golk::kMulti*), band, and for k_step_tile the
// tile width and segment code it was timed at (a plan may hold a tile family other than the
// engine's own pick: each launch carries its shape)
struct Launch {
    int k = 0, var = 0, band = 0;
    int tw = 0, seg = 0;
    int blk = 0;                             // kMultiTilePersist: turns per block
};
constexpr int kPlanMax = 128;               // launch plans cover gol_step / halo windows up to this
constexpr int kSeqMax = 32;                 // gol_step calls this short run a timed sequence
constexpr size_t kLastCap = 4096;           // gol_last_launches records at most this many
constexpr int kMaxStepChunks = 64;          // row chunks of one launch at the most (GOL_STEP_CHUNKS)

// a read-only call (gol_snapshot, gol_read_*, ...) run by a stepping thread at a launch boundary
struct Job {
    std::function<int()> fn;
    int rc = 0;
    bool done = false;
};

namespace goleng __attribute__((visibility("hidden"))) {

// Everything the create-time choice produces: defaults and experiment pins, the model's pick,
// the pinned table, the autotune or the tune cache.  An engine takes one through set_shape.
struct LaunchShape {
    int multi_variant = golk::kMultiSkewILW16;  // temporal-blocking kernel (kMulti*)
    int tpl = 1;                             // turns per stencil launch (temporal blocking)
    int band_multi = 64;                     // band height of the multi-turn kernel (depth tpl)
    // k_step_tile shape (kMultiTile): tile width in words, rows per lane segment (the tile
    // height is the launch's band)
    int tile_w = 0, tile_seg = 0;
    // a pinned k_step_tile shape's tile height for launches of depth <= short_k (0: none): a
    // short step's one shallow launch takes the taller tile its depth allows
    int short_k = 0, short_band = 0;
    // launch planner (autotuned engines): plan[t] = the first launch of the fastest measured
    // sequence of launches for t turns (t <= kPlanMax; k = 0: no plan, use the even split)
    std::vector<Launch> plan;
    // seq[r] (r <= kSeqMax, torus engines): the launch sequence of a gol_step of exactly r
    // turns, chosen by timing whole candidate sequences the way gol_step runs them (empty:
    // follow `plan`)
    std::vector<std::vector<Launch>> seq;
    // K1p (k_tile_persist, small torus boards): turns per block (0 = off) and its segment code
    // (plain launches keep tile_seg)
    int persist_k = 0, persist_seg = 0;
    // K1q (k_tile_stream, large torus boards): turns per block (0 = off) and its tile shape
    int stream_k = 0;
    int stream_tw = 0, stream_th = 0, stream_seg = 0;
    float tuned_us_per_turn = 0.f;           // autotune's best measurement (0 = not tuned)
};

// K1p / K1q / K1r (gol_blocks.cpp; tools build only): what the experiments asked for at create,
// the uncached block buffers and per-tile flags, the flags' epoch (grows by blocks + 1 per
// launch), K1q's item counter (uncached) and its host mirror (the value the next launch starts
// from)
struct BlockState {
    bool persist_forced = false;             // GOL_PERSIST (tests): also on a shared device
    bool persist_ring = false;               // GOL_RING: K1r instead of K1p
    bool stream_forced = false;              // GOL_STREAM (tests): also on a shared device
    uint64_t *pu[2] = {nullptr, nullptr};
    unsigned *pflags = nullptr;
    size_t pflags_n = 0;
    unsigned pepoch = 0;
    unsigned *pcounter = nullptr;
    unsigned pcount = 0;
    uint64_t *su[2] = {nullptr, nullptr};    // K1q block buffers (cached: hipMalloc)
};

}  // namespace goleng

struct gol_ctx {
    gol_config cfg{};
    int device = 0;
    int nw = 0, pitch = 0, buf_rows = 0;
    bool fast = false;
    // a width of >= 256 cells that is no multiple of 128 (a partial last word, or an odd word
    // count): multi-turn launches on k_step_tile alone, one word per lane -- across the row seam
    // at a golk::kTileSeamCodes code when width % 64 != 0.  (Off for forced-generic and count
    // engines, and under a GOL_MULTI_VARIANT other than k_step_tile: one turn per launch.)
    bool tile_only = false;
    // the engine's k_step_tile launches run the big form (k_step_tile_big): a buffer of 2 GiB or
    // more on whole-word rows of >= 256 cells (then also tile_only: no other kernel blocks such
    // a buffer), or GOL_TILE_BIG=1 at create on a buffer of any size.  tile_big_forced: the
    // latter, which also goes to the launches (StepArgs::tile_big)
    bool tile_big = false, tile_big_forced = false;
    // plain k_step_tile launches of a code with a pair form run it (k_step_tile_duo,
    // StepArgs::tile_duo): set at create unless GOL_TILE_DUO=0
    bool tile_duo = false;
    int band = 8;
    int variant = golk::kVariantDefault;
    int multi_words = 2;                     // k_step_multi words per lane
    unsigned wg_prio = 0;                    // k_step_wg priority override (GOL_WG_PRIO, tools)
    // the launch shape and band_for_depth's cache of its bands at other depths (0 = not yet):
    // assigned and reset together, by set_shape
    goleng::LaunchShape shape;
    int band_at[golk::kMaxTurnsPerLaunch + 1] = {};
    std::vector<Launch> last;                // launches of the last gol_step (gol_last_launches)
    long long last_n = 0;
    int ncu = 0;                             // compute units of the device
    int shape_source = 0;                    // gol_info.shape_source: 1 = searched, 2 = kKnownShapes
    uint64_t *board[2] = {nullptr, nullptr};
    int cur = 0;
    bool il = false;                         // board[cur] is in the interleaved layout
    uint64_t *blocked = nullptr;
    bool blocked_pending = false;
    long long nonbinary = 0;
    std::vector<uint8_t> raw_turn0;          // loaded bytes, kept only while non-binary & turn == 0
    unsigned long long *counts = nullptr;    // (kRingSlots + 1) * kShards
    unsigned long long *h_counts = nullptr;  // pinned mirror of one slot
    uint8_t *staging = nullptr;
    size_t staging_size = 0;
    // gol_flipped_cells: board[cur ^ 1] holds the board exactly one turn back, both halves in
    // the standard layout (the last step ran one turn and nothing has written the other half
    // or flipped `cur` since)
    bool prev_valid = false;
    long long *flip_rows = nullptr;          // rows counts + (rows + 1) offsets (first call on)
    long long *h_flip_total = nullptr;       // pinned: the list length
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    hipStream_t side = nullptr;              // boundary-band launches of gol_step_overlap
    hipEvent_t ev_side = nullptr, ev_main = nullptr;
    // the chunked pipeline of gol_step (gol_step.cpp, launch_chunked): one event per chunk and
    // launch parity, created at first use; the chunk kernels of the last gol_step
    hipEvent_t chunk_ev[2][kMaxStepChunks] = {};
    long long last_chunks = 0;
    long long turn = 0;
    long long launches = 0;
    int halo_valid = 0;
    // temporal blocking off: a buffer of 2 GiB or more that the big form does not run (a count
    // engine, width % 64 != 0, width < 256, forced-generic, another GOL_MULTI_VARIANT)
    bool blocking_limited = false;
    // GOL_FLAG_COUNT_EVERY_TURN engines: multi-turn launches with the counts fused into
    // k_step_tile are allowed (GOL_COUNT_BLOCKING=0 at create: one-turn launches, for A/B)
    bool count_blocking = false;
    // kMultiWgPg: published boundary rows and per-(tile, stage) flags (uncached, grow-only)
    uint64_t *pg_rows = nullptr;
    unsigned *pg_flags = nullptr;
    size_t pg_lanes = 0, pg_tiles = 0;
    unsigned pg_epoch = 0;
    // control word (gol_set_control): read by gol_step between launches, written by any
    // thread without the engine lock (the reference's CFput flag channel)
    std::atomic<int> control{GOL_CONTROL_RUN};
    std::atomic<bool> control_used{false};
    std::atomic<long long> progress{0};      // lock-free mirror of `turn` (gol_get_progress)
    std::atomic<bool> parked{false};         // gol_step is parked on GOL_CONTROL_PAUSE
    goleng::BlockState blocks;               // K1p / K1q / K1r (tools build)
    // device error word (host-mapped pinned memory; golk::kDevErr*): a k_step_wg wait that gave
    // up writes it, every synchronising call checks it
    unsigned *h_err = nullptr, *d_err = nullptr;
    bool registered = false;                 // counted in the per-device engine registry
    hipEvent_t ev_copy = nullptr;            // gol_copy_halo_from_*: ordering between engines
    std::string err;
    std::recursive_mutex mu;                 // engine state; held by gol_step except while parked
    // read-only calls from other threads while gol_step runs (run_read): served by the stepping
    // thread at its next launch boundary
    std::mutex jm;
    std::condition_variable jcv;
    std::vector<Job *> jobs;
    bool stepping = false;                   // (under jm) a gol_step holds `mu`
    std::atomic<bool> jobs_pending{false};
    std::atomic<bool> readers{false};        // a reader was served during a step: keep the queue short
};

namespace goleng __attribute__((visibility("hidden"))) {

// ---------------------------------------------------------------- gol_engine.cpp
int fail(gol_ctx *c, int code, const char *fmt, ...);
// kMultiWgPg and K1p run only on a device this process's one engine has to itself
bool device_exclusive(int dev);
// the device error word after a synchronisation (GOL_EHIP when a kernel's wait gave up)
int check_dev_err(gol_ctx *c);
int sync_checked(gol_ctx *c);
void clear_dev_err(gol_ctx *c);

#define HIP_OR_FAIL(c, expr)                                                                   \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail((c), e_ == hipErrorOutOfMemory ? GOL_ENOMEM : GOL_EHIP, "%s: %s (%s:%d)", \
                        #expr, hipGetErrorString(e_), __FILE__, __LINE__);                     \
    } while (0)

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev)
    {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard()
    {
        int now = -1;
        if (prev >= 0 && hipGetDevice(&now) == hipSuccess && now != prev) (void)hipSetDevice(prev);
    }
};

inline bool is_strip(const gol_ctx *c) { return c->cfg.halo > 0; }
// rows of the owned region inside the buffer
inline int own_lo(const gol_ctx *c) { return c->cfg.halo; }
inline int own_hi(const gol_ctx *c) { return c->cfg.halo + c->cfg.rows; }

// Run a read-only engine call.  No gol_step in progress: now, under the engine lock.  While
// another thread's gol_step runs: by that thread at its next launch boundary, on the board the
// step has enqueued so far (turn-consistent), so AliveCellsCount / GetWorld never wait for
// the whole step -- the reference's Alivecount and GetWorld take the Server mutex only around
// the per-turn commit (Server/gol/distributor.go:62-75,131-134).  While the step is parked on
// PAUSE it has released the engine, and the call runs now.
template <class F>
int run_read(gol_ctx *c, F &&fn)
{
    for (;;) {
        std::unique_lock<std::mutex> jl(c->jm);
        if (c->stepping) {
            Job j;
            j.fn = std::function<int()>(fn);
            c->jobs.push_back(&j);
            c->jobs_pending.store(true);
            c->readers.store(true);
            c->jcv.wait(jl, [&] { return j.done; });
            return j.rc;
        }
        if (c->mu.try_lock()) {              // (the owner of a recursive lock gets it too)
            jl.unlock();
            std::lock_guard<std::recursive_mutex> lk(c->mu, std::adopt_lock);
            return fn();
        }
        jl.unlock();                         // a short call holds the engine, or a step is
        std::this_thread::sleep_for(std::chrono::microseconds(50));   // about to flag itself
    }
}

// One event pair on a stream, for the create-time timings.  ms(enqueue): the time between the
// pair around whatever `enqueue` queues on the stream (it returns false on a failed launch),
// after waiting for it; 0 on any error.  Best-of-n is the caller's loop.
struct LaunchTimer {
    hipStream_t stream;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    explicit LaunchTimer(hipStream_t s) : stream(s)
    {
        if (hipEventCreate(&e0) != hipSuccess) e0 = nullptr;
        if (e0 && hipEventCreate(&e1) != hipSuccess) e1 = nullptr;
    }
    LaunchTimer(const LaunchTimer &) = delete;
    LaunchTimer &operator=(const LaunchTimer &) = delete;
    ~LaunchTimer()
    {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        (void)hipGetLastError();
    }
    bool ok() const { return e0 && e1; }
    template <class F>
    float ms(F &&enqueue)
    {
        float t = 0.f;
        const bool done = ok() && hipEventRecord(e0, stream) == hipSuccess && enqueue() &&
                          hipEventRecord(e1, stream) == hipSuccess &&
                          hipEventSynchronize(e1) == hipSuccess &&
                          hipEventElapsedTime(&t, e0, e1) == hipSuccess;
        return done ? t : 0.f;
    }
};

// ---------------------------------------------------------------- gol_plan.cpp
// The only place an engine's launch shape is assigned (it resets the per-depth band cache).
void set_shape(gol_ctx *c, LaunchShape s);
// StepArgs for the whole buffer on the engine's stream: everything but the kernel choice
// (multi_variant, band, tile shape), the boards and the count / mask pointers
golk::StepArgs whole_buffer_args(const gol_ctx *c);
int band_same_rounds(const gol_ctx *c, int var, int K0, int band0, int k);
Launch plan_launch(gol_ctx *c, int64_t room);
bool stepping_il(const gol_ctx *c, int k);
// the launch sequence the autotune timed for a torus gol_step of exactly `turns` turns
// (shape.seq), or null: follow plan_launch
const std::vector<Launch> *timed_sequence(const gol_ctx *c, int64_t turns);
// Row chunks of one k_step_tile launch over `rows` buffer rows on tiles of tile_h rows: the
// n + 1 bounds of n <= want chunks, cut on multiples of tile_h (the tile rows spread evenly:
// floor(tile rows / n) each, one more for the last tile rows % n chunks; the ragged tile row
// stays in the last chunk), every chunk at least min_rows tall -- fewer chunks when
// `want` cannot have that; one chunk = {0, rows}.
std::vector<int> chunk_bounds(int rows, int tile_h, int want, int min_rows);
// deps[q]: the chunks of the previous launch (bounds pb, depth kp) that chunk q of the next
// one (bounds nb, depth kn) must follow on the torus of `rows` buffer rows
std::vector<std::vector<int>> chunk_deps(int rows, const std::vector<int> &pb, int kp,
                                         const std::vector<int> &nb, int kn);
// Chunks per launch of one gol_step call, read once per call: 1 = never (GOL_STEP_CHUNKS=1, and
// every call that cannot chunk: strip and count engines, a control word in use, an overlapped
// window, no side stream), n >= 2 = n chunks (GOL_STEP_CHUNKS=n), -1 = automatic (unset / 0)
int chunk_request(const gol_ctx *c, bool ctl, bool overlapped);
// The chunk bounds of launch L under `request` (empty: one whole kernel).  A launch is cut when
// the one before it was (k_live: the depth of the live pipeline's last launch, else 0) or when
// the next one can be -- timed_next, or else plan_launch's for the `left` turns after L; a lone
// launch stays whole.  Every chunk is at least as tall as L's and both neighbours' depths.
std::vector<int> plan_chunks(gol_ctx *c, const Launch &L, int request, int64_t left,
                             const Launch *timed_next, int k_live);

// ---------------------------------------------------------------- gol_step.cpp
int ensure_layout(gol_ctx *c, bool il);
hipError_t pg_prepare(gol_ctx *c, golk::StepArgs &a, int k);

// ---------------------------------------------------------------- gol_io.cpp
void release_blocked(gol_ctx *c);

// ---------------------------------------------------------------- gol_tune.cpp
struct TileShape {
    int K = 0, th = 0, tw = 0, seg = 0;
    double model_us = 0;                     // modelled time per turn
};
// (width: the board's when its width is no multiple of 64 -- golk::tile_shape_ok; else 0)
double tile_model_us(int ncu, int nw, int rows, int K, int th, int tw, int seg, int width = 0);
// (big: for an engine that runs the big form on a buffer of `rows` rows of nw words -- codes of
// golk::kTileBigCodes and tile heights whose window it takes)
std::vector<TileShape> tile_candidates(int ncu, int nw, int rows, int keep, bool cnt = false,
                                       int width = 0, bool big = false);
// the engine runs k_step_tile at this shape (no plan, no K1p; K1q's shape and the measured time
// stay)
void apply_tile(gol_ctx *c, const TileShape &t);
void autotune_small(gol_ctx *c);
void autotune_multi(gol_ctx *c, bool tune_k, bool tune_variant);

// Create-time autotune results, per (device, width, buffer rows, requested depth, what was
// tuned): engines of one shape in one process -- the strips of a run, the engines a test suite
// or a sweep creates -- time their candidates once (GOL_AUTOTUNE_CACHE=0: always re-time).
struct TuneKey {
    int dev, width, rows, tpl_req, mode;
    bool operator<(const TuneKey &o) const
    {
        return std::tie(dev, width, rows, tpl_req, mode) <
               std::tie(o.dev, o.width, o.rows, o.tpl_req, o.mode);
    }
};
bool tune_cache_lookup(const TuneKey &key, LaunchShape *out);
void tune_cache_store(const TuneKey &key, const LaunchShape &s);

// one kernel's fastest (K, band) and its measured launch times at every depth (autotune_multi's
// launch planner): T[k] ms per launch of depth k at band band_k[k] (0: not run)
struct LaunchFamily {
    int var, K, band, tw, seg;
    float T[golk::kMaxTurnsPerLaunch + 1];
    int band_k[golk::kMaxTurnsPerLaunch + 1];
};

// ---------------------------------------------------------------- gol_blocks.cpp
// K1p / K1q / K1r.  The product library has none of these kernels: there the requests are
// refused, the tuners return at once and no launch of kind kMultiTilePersist / kMultiTileStream
// is ever planned.
// GOL_PERSIST / GOL_RING / GOL_STREAM at create (tests, experiments): GOL_OK or GOL_EINVAL
int blocks_parse_env(gol_ctx *c);
// K1p against plain launches at the tuned tile shape (small torus boards)
void blocks_tune_persist(gol_ctx *c);
// K1q against the tuned steady rate `best_ms` (ms per turn) at the tile family's shape; returns
// its ms per turn when it is kept (shape.stream_* set), else 0
float blocks_tune_stream(gol_ctx *c, golk::StepArgs a, const LaunchFamily *tile, float best_ms);
// the next launch as K1p / K1q blocks when the engine runs them and `room` turns allow
bool blocks_plan(gol_ctx *c, int64_t room, Launch *out);
// one launch of kind kMultiTilePersist / kMultiTileStream
hipError_t blocks_launch(gol_ctx *c, const golk::StepArgs &a, const Launch &L);
void blocks_free(gol_ctx *c);
#if GOL_TOOLS
// GOL_MULTI_VARIANT=kMultiWgDiag: one k_step_wg launch of `a` with per-wave wait timing
int wg_diag_launch(gol_ctx *c, golk::StepArgs a, int k);
#endif

}  // namespace goleng
