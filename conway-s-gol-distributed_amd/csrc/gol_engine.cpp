// gol_engine.cpp — the per-GPU engine behind include/gol_amd.h: create / destroy, the pinned
// launch shapes and their create-time check, the per-device engine registry and the error
// helpers.  The engine's state and the other units are listed in gol_ctx.h.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <new>
#include <set>

#include "gol_ctx.h"
#include "gol_resident.h"

namespace goleng {

namespace {

// engines alive per device in this process: kMultiWgPg runs only on a device with one engine
// (two concurrent parallelogram grids can each fill an XCD with tiles waiting for tiles of
// their own launch that sit undispatched behind the other grid's: the waits would time out),
// and not at all when GOL_SHARED_DEVICE is set (other processes share the GPU: torchrun ranks
// on one device).  The rows it would have published are recomputed as plain helix bands.
std::mutex g_dev_mu;
std::map<int, int> g_dev_engines;

// Pinned shapes whose create-time check (check_pinned) has run in this process, per (device,
// width, buffer rows): later engines of the same shape -- the strips of a run, a bench's second
// measurement, a gol.Run after an Engine -- skip it (its ~60 ms of launches are a cost of the
// first engine only).
std::mutex g_pin_mu;
std::set<std::tuple<int, int, int>> g_pin_checked;

}  // namespace

int fail(gol_ctx *c, int code, const char *fmt, ...)
{
    if (c) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        c->err = buf;
    }
    return code;
}

bool device_exclusive(int dev)
{
    static const bool shared = getenv("GOL_SHARED_DEVICE") && atoi(getenv("GOL_SHARED_DEVICE"));
    if (shared) return false;
    std::lock_guard<std::mutex> lk(g_dev_mu);
    auto it = g_dev_engines.find(dev);
    return it == g_dev_engines.end() || it->second <= 1;
}

// The device error word after a synchronisation: a k_step_wg hand-off or parallelogram flag
// wait gave up (a preempted or starved workgroup), so the board of that launch is wrong.  The
// word stays set until the board is replaced (gol_load*, gol_fill_random): every synchronising
// call reports it (the reference ignored its RPC errors, Server/gol/distributor.go:219).
int check_dev_err(gol_ctx *c)
{
    const unsigned e = c->h_err ? *(volatile unsigned *)c->h_err : 0u;
    if (!e) return GOL_OK;
    return fail(c, GOL_EHIP,
                "a %s wait timed out (device error word %u): the board is corrupt; reload it",
                e == golk::kDevErrPgFlag     ? "k_step_wg parallelogram flag"
                : e == golk::kDevErrTileFlag ? "k_tile_persist neighbour-tile flag"
                                             : "k_step_wg hand-off",
                e);
}

int sync_checked(gol_ctx *c)
{
    HIP_OR_FAIL(c, hipStreamSynchronize(c->stream));
    return check_dev_err(c);
}

void clear_dev_err(gol_ctx *c)
{
    if (c->h_err) *(volatile unsigned *)c->h_err = 0u;
}

}  // namespace goleng

using namespace goleng;

namespace {

// Pinned launch shapes for the BASELINE board sizes on an MI355X (gfx950, 256 CUs): an engine
// of one of these widths and buffer heights (a torus, or a row strip with its halos) with
// nothing pinned by the caller runs this k_step_tile shape and skips the create-time search.  The search's 0.5 ms timings put a dozen shapes within
// ~1.5 % of each other and picked different ones from box to box (round 4: 65536^2 K = 20 on
// 336-row tiles on one box, K = 32 on 512-row tiles or k_step_skew K = 8 on others; 16384^2
// bands 316 / 320), so the kernel a bench line timed was not reliably the one profiles/
// measured.  These are the search winners of the round-4 sweeps, each pinned by a full-size
// oracle digest (tests/test_gpu_engine.py::test_pinned_shape_digest) and profiled as is
// (profiles/r05_*_summary.json).  GOL_AUTOTUNE=2 measures instead.
struct KnownShape {
    int width, rows;
    TileShape t;                             // K, tile height, tile width (lanes), segment code
    float us_per_turn;                       // measured steady state (round-4 sweeps)
    int short_K = 0, short_th = 0;           // launches of depth <= short_K: tiles short_th tall
};
constexpr KnownShape kKnownShapes[] = {
#ifdef GOL_PIN_OVERRIDE   // (A/B builds: an entry ahead of the table, e.g. 65536,65536,{20,472,30,516,0},34.f)
    {GOL_PIN_OVERRIDE},
#endif
    // configs[3..4]: 30-lane tiles of ORD 5 SEG 16 in 16-wave workgroups (2 per CU, 8 waves
    // per SIMD).  Long steps: K = 30 on 30 x 452 tiles, 33.09-33.12 us per turn against
    // 33.72-33.75 for K = 20 (profiles/r06_c3_deep_k.log, 65536 sweep).  Launches of <= 20
    // turns -- the driver's 20-turn call is one launch of exactly 20 -- keep 30 x 472 tiles:
    // the fastest of 30 K = 20 shapes (33.6 us per turn; profiles/r06_headline_pin_ab.log) and,
    // in the bench, 118.3-121.0k against 117.7-119.4k for 30 x 536 SEG 24 12-wave tiles and
    // 115.9-118.4k for round 5's K = 24 on 30 x 336 8-wave tiles (alternating on one box)
    {65536, 65536, {30, 452, 30, 516, 0}, 33.1f, 20, 472},
    // configs[2]: ORD 5, SEG 16, 8-wave workgroups, 14 x 410 tiles, K = 51 (deeper than the
    // planner's tables: k_step_tile runs up to 64 turns): 760 tiles, at most 3 per CU, 2.726-2.730
    // us per turn against 2.742 for K = 48 on 14 x 416 and 2.83-2.84 for round 6's first pin,
    // 14 x 448 at K = 32 (703 tiles), which was the fastest of 36 K = 32 shapes
    // (profiles/r06_c3_deep_k.log; before it round 5's 14 x 320 ORD 1 SEG 12,
    // profiles/r06_headline_pin_ab.log)
    {16384, 16384, {51, 410, 14, 516, 0}, 2.73f},
    // configs[1]: ORD 2, SEG 3, 16-wave workgroups of 10-lane tiles (5 groups per wave), 10 x
    // 160 at K = 40: 8 x 32 = 256 tiles, one per CU with none idle (80 words = 8 x 10 exactly),
    // 0.524-0.530 us per turn against 0.550-0.553 for the earlier 14 x 128 at K = 32 (240
    // tiles; profiles/r06_c3_deep_k.log, C2 section)
    {5120, 5120, {40, 160, 10, 203, 0}, 0.53f},
    // configs[3..4] as row strips with 128-row halos (buffer = H / N + 256 rows):
    // N = 8 ORD 1 SEG 12 (west carry) on 14 x 352 tiles, 8 launches of 16 turns per window
    // (5.44-5.46 us per turn against 5.69-5.70 for ORD 5 SEG 12 on the same tiles,
    // profiles/r05_strip_seg12_ab.log; 5.61-5.71 for round 4's searched picks); N = 4 and 2
    // ORD 5 SEG 16 since round 6: 14 x 448 tiles K = 32 (9.14 against 9.21 us per turn for
    // round 5's 14 x 704 SEG 24) and 14 x 480 tiles K = 16 (16.97 against 17.91)
    // (profiles/r06_strip_sweep.log)
    {65536, 8448, {16, 352, 14, 112, 0}, 5.3f},
    {65536, 16640, {32, 448, 14, 516, 0}, 9.14f},
    {65536, 33024, {16, 480, 14, 516, 0}, 16.97f},
    // configs[3..4] as row strips with the bench's default halo for its 20-turn command
    // (min(128, turns): 20 rows, one exchange and one 20-turn launch per window; buffer = H / N
    // + 40 rows), K = 20, the fastest of 40-50 shapes swept per buffer
    // (profiles/r06_strip_sweep.log): N = 8 ORD 1 SEG 12 (west carry) on 14 x 344 tiles, 4.95
    // us per turn; N = 4 and 2 the headline's ORD 5 SEG 16 on 30 x 472 tiles in 16-wave
    // workgroups, 9.04 / 17.56 against 9.28-9.36 / 18.16 for 14 x 344 ORD 1 SEG 12
    {65536, 8232, {20, 344, 14, 112, 0}, 4.95f},
    {65536, 16424, {20, 472, 30, 516, 0}, 9.04f},
    {65536, 32808, {20, 472, 30, 516, 0}, 17.56f},
    // configs[2] on 2 GPUs: 16384^2 as 2 strips with 128-row halos (16384 x 8448): ORD 5 SEG 12
    // on 30 x 320 tiles, K = 32, 16-wave workgroups: 1.72 us per turn (30 x 320 ORD 1 SEG 12
    // 1.73, 14 x 704 ORD 5 SEG 12 1.74, the 14 x 320 ORD 1 torus pin slower;
    // profiles/r06_strip_sweep.log)
    {16384, 8448, {32, 320, 30, 512, 0}, 1.72f},
};

// (a count engine of a pinned size keeps the pinned shape: its launches run the counted form)
constexpr bool known_shapes_counted()
{
    for (const KnownShape &k : kKnownShapes)
        if (!golk::tile_code_counted(k.t.seg)) return false;
    return true;
}
static_assert(known_shapes_counted(), "every kKnownShapes code is in golk::kTileCountCodes");

bool known_shape(const gol_ctx *c, KnownShape *out)
{
    if (c->ncu != 256) return false;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, c->device) != hipSuccess ||
        std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return false;
    for (const KnownShape &k : kKnownShapes)
        if (k.width == c->cfg.width && k.rows == c->buf_rows &&
            golk::tile_shape_ok(c->nw, k.t.K, k.t.th, k.t.tw, k.t.seg) &&
            (!c->tile_big || golk::tile_big_ok(k.width, c->buf_rows, c->pitch, k.t.K, k.t.th, k.t.seg))) {
            *out = k;
            return true;
        }
    return false;
}

// timing events, destroyed with the list
struct EventList {
    std::vector<hipEvent_t> ev;
    bool ok = true;                          // every event was created
    explicit EventList(size_t n) : ev(n)
    {
        for (auto &e : ev)
            if (ok && hipEventCreate(&e) != hipSuccess) {
                e = nullptr;
                ok = false;
            }
    }
    ~EventList()
    {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

// A pinned shape is applied whenever the device, width and buffer rows match: the shape never
// depends on timing or load (round-5 advice: a slow or shared box must not change the kernel
// the tests and profiles pin).  The first engine of a pinned shape in a process then runs
// ~GOL_PIN_VERIFY_MS (default 60; 0 = off) ms of its launches on its own buffers and compares
// the median time per turn with the table's figure; more than 1.35x is only reported (stderr),
// a device unlike the one the table was measured on.  The check also keeps the GPU busy right
// before the caller's first steps: an MI355X that idled drops its clock, and a 20-turn 65536^2
// call then takes 810-850 us instead of 700 (profiles/r04_clock_ramp_20turn.log,
// profiles/r05_prewarm_probe.log).  Later engines of the same (device, width, buffer rows) skip
// it (g_pin_checked).  Returns the median us per turn (0 when it did not run).
float check_pinned(gol_ctx *c, const KnownShape &ks)
{
    const char *v = getenv("GOL_PIN_VERIFY_MS");
    const double budget_ms = v ? atof(v) : 60.0;
    if (budget_ms <= 0) return 0.f;
    const auto key = std::make_tuple(c->device, c->cfg.width, c->buf_rows);
    {
        std::lock_guard<std::mutex> lk(g_pin_mu);
        if (g_pin_checked.count(key)) return 0.f;
    }
    golk::StepArgs a = whole_buffer_args(c);
    a.multi_variant = golk::kMultiTile;
    a.band = ks.t.th;
    a.tile_w = ks.t.tw;
    a.tile_seg = ks.t.seg;
    if (golk::launch_fill_random(c->board[0], c->cfg.width, c->nw, c->pitch, c->buf_rows, 0,
                                 c->buf_rows, 12345, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess)
        return 0.f;
    // groups of ~1 ms of launches
    const int n = std::max(1, (int)std::ceil(1000.0 / (ks.t.K * ks.us_per_turn)));
    std::vector<float> us;
    // (default) one queue of back-to-back launches, an event pair per group, one sync at the
    // end: the GPU stays busy for the whole check (bench20 116.5-118.0k against 116.1-117.2k
    // with a sync after every burst, profiles/r05_verify_mode_ab.log); GOL_PIN_VERIFY_MODE=0:
    // bursts of ~1 ms, each ended by a sync
    const char *vm = getenv("GOL_PIN_VERIFY_MODE");
    const bool queued = !(vm && atoi(vm) == 0);
    if (queued) {
        const int groups = std::max(8, (int)std::ceil(budget_ms * 1000.0 / (n * ks.t.K * ks.us_per_turn)));
        const EventList events((size_t)groups + 1);
        if (!events.ok) return 0.f;
        const std::vector<hipEvent_t> &ev = events.ev;
        bool ok = hipEventRecord(ev[0], c->stream) == hipSuccess;
        for (int i = 0; ok && i < groups; ++i) {
            for (int j = 0; ok && j < n; ++j) {
                a.in = c->board[j & 1];
                a.out = c->board[(j + 1) & 1];
                ok = golk::launch_step_multi(a, ks.t.K, c->stream) == hipSuccess;
            }
            ok = ok && hipEventRecord(ev[i + 1], c->stream) == hipSuccess;
        }
        ok = ok && hipStreamSynchronize(c->stream) == hipSuccess;
        for (int i = 0; ok && i < groups; ++i) {
            float ms = 0.f;
            ok = hipEventElapsedTime(&ms, ev[i], ev[i + 1]) == hipSuccess;
            us.push_back(ms * 1e3f / (n * ks.t.K));
        }
        if (!ok) return 0.f;
    }
    // GOL_PIN_VERIFY_MODE=0: bursts of ~1 ms of launches, each ended by a sync (host wall time,
    // as gol_step runs)
    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; !queued && i < 2000; ++i) {
        const auto s0 = std::chrono::steady_clock::now();
        for (int j = 0; j < n; ++j) {
            a.in = c->board[j & 1];
            a.out = c->board[(j + 1) & 1];
            if (golk::launch_step_multi(a, ks.t.K, c->stream) != hipSuccess) return 0.f;
        }
        if (hipStreamSynchronize(c->stream) != hipSuccess) return 0.f;
        const auto s1 = std::chrono::steady_clock::now();
        us.push_back(std::chrono::duration<float, std::micro>(s1 - s0).count() / (n * ks.t.K));
        if (std::chrono::duration<double, std::milli>(s1 - t0).count() >= budget_ms && i >= 8) break;
    }
    (void)hipGetLastError();
    {
        std::lock_guard<std::mutex> lk(g_pin_mu);
        g_pin_checked.insert(key);
    }
    if (check_dev_err(c) != GOL_OK || us.empty()) return 0.f;
    std::vector<float> tail(us.begin() + us.size() / 2, us.end());
    std::sort(tail.begin(), tail.end());
    const float med = tail[tail.size() / 2];
    const bool slow = med > 1.35f * ks.us_per_turn;
    if (slow || getenv("GOL_AUTOTUNE_LOG"))
        fprintf(stderr, "%spinned shape %dx%d K=%d tile=%dx%d code=%d: %zu launches, median %.3f us per "
                "turn (table %.3f)%s\n", slow ? "gol: warning: " : "", c->cfg.width, c->buf_rows,
                ks.t.K, ks.t.tw, ks.t.th, ks.t.seg, us.size(), med, ks.us_per_turn,
                slow ? " -- more than 1.35x the table: not the device the table was measured on, "
                       "or a shared / throttled one (the pinned shape is kept)" : "");
    return med;
}

// The tile shape an engine starts from before anything is measured: small boards (and
// k_step_tile pinned by GOL_MULTI_VARIANT) take the model's best shape for the requested or
// default depth, then the experiments' overrides (GOL_TILE, a caller's band_rows, K1p / K1q).
// GOL_OK, or GOL_EINVAL for a shape that cannot run.  (Create time: no launch has been planned
// yet, so the overrides edit the shape in place.)
int initial_tile_shape(gol_ctx *c, bool cntb)
{
    const gol_config *cfg = &c->cfg;
    LaunchShape &s = c->shape;
    int K = cfg->turns_per_launch > 0 ? std::min(cfg->turns_per_launch, golk::kMaxTileTurns) : 0;
    if (const char *v = getenv("GOL_TURNS_PER_LAUNCH"))
        K = std::max(2, std::min(atoi(v), golk::kMaxTileTurns));
    std::vector<TileShape> cand =
        tile_candidates(c->ncu, c->nw, c->buf_rows, 1 << 20, cntb, c->cfg.width, c->tile_big);
    // a big engine starts from the 65536^2 pins (kKnownShapes: 30 lanes x 452 rows at K = 30,
    // 30 x 472 at K = 20, ORD 5 SEG 16 in 16-wave workgroups) where they run: rows as long and
    // a buffer as tall as that board's or more
    if (c->tile_big)
        for (const TileShape &t : {TileShape{20, 472, 30, 516, 0}, TileShape{30, 452, 30, 516, 0}})
            if (golk::tile_shape_ok(c->nw, t.K, t.th, t.tw, t.seg, c->cfg.width) &&
                golk::tile_big_ok(c->cfg.width, c->buf_rows, c->pitch, t.K, t.th, t.seg))
                cand.insert(cand.begin(), t);
    for (const TileShape &t : cand)
        if (K == 0 || t.K == K) {
            apply_tile(c, t);
            break;
        }
    if (K > 0 && s.multi_variant == golk::kMultiTile && s.tpl != K) {
        // no ranked shape at this depth (K not in the candidate list): best TW / TH at K
        TileShape best;
        for (const TileShape &t : cand) {
            const double m =
                tile_model_us(c->ncu, c->nw, c->buf_rows, K, t.th, t.tw, t.seg, c->cfg.width);
            if (m > 0 && (best.K == 0 || m < best.model_us)) best = {K, t.th, t.tw, t.seg, m};
        }
        if (best.K) apply_tile(c, best);
    }
    if (s.multi_variant == golk::kMultiTile && cfg->band_rows > 0)
        s.band_multi = cfg->band_rows;       // tile height pinned by the caller
    if (const char *v = getenv("GOL_TILE")) {           // experiments: "TW,SEG"
        int tw = 0, seg = 0;
        if (sscanf(v, "%d,%d", &tw, &seg) == 2 && tw > 0 && seg > 0) {
            s.multi_variant = golk::kMultiTile;
            s.tile_w = tw;
            s.tile_seg = seg;
        }
    }
    if (s.multi_variant == golk::kMultiTile &&
        !golk::tile_shape_ok(c->nw, s.tpl, s.band_multi, s.tile_w, s.tile_seg, c->cfg.width))
        return GOL_EINVAL;
    // the big form: a code of its set, a window that wraps at most once and stays below 2 GiB
    if (c->tile_big && (s.multi_variant != golk::kMultiTile ||
                        !golk::tile_big_ok(c->cfg.width, c->buf_rows, c->pitch, s.tpl, s.band_multi,
                                           s.tile_seg)))
        return GOL_EINVAL;
    if (int rc = blocks_parse_env(c)) return rc;   // GOL_PERSIST / GOL_RING / GOL_STREAM
    // (K1p / K1q / K1r know nothing of the row seam or of odd word counts)
    return c->tile_only && (s.persist_k > 0 || s.stream_k > 0) ? GOL_EINVAL : GOL_OK;
}

}  // namespace

// ================================================================ C ABI
extern "C" {

const char *gol_strerror(int code)
{
    switch (code) {
    case GOL_OK: return "ok";
    case GOL_EINVAL: return "invalid argument";
    case GOL_EHIP: return "HIP runtime error";
    case GOL_ENOMEM: return "out of memory";
    case GOL_ESTATE: return "invalid state";
    case GOL_ENODEV: return "no HIP device";
    case GOL_EIO: return "I/O error";
    case GOL_ECLOSED: return "channel closed";
    case GOL_ETIMEDOUT: return "timed out";
    default: return "unknown error";
    }
}

const char *gol_last_error(const gol_ctx *ctx) { return ctx ? ctx->err.c_str() : ""; }

int gol_create(int32_t width, int32_t height, uint32_t flags, gol_ctx **out)
{
    gol_config cfg{};
    cfg.width = width;
    cfg.height = height;
    cfg.device = -1;
    cfg.row_offset = 0;
    cfg.rows = height;
    cfg.halo = 0;
    cfg.flags = flags;
    cfg.band_rows = 0;
    return gol_create_ex(&cfg, out);
}

int gol_create_ex(const gol_config *cfg, gol_ctx **out)
{
    if (!cfg || !out) return GOL_EINVAL;
    *out = nullptr;
    if (cfg->width < 2 || cfg->height < 1 || cfg->rows < 1 || cfg->halo < 0) return GOL_EINVAL;
    if (cfg->halo == 0 && (cfg->rows != cfg->height || cfg->row_offset != 0)) return GOL_EINVAL;
    if (cfg->halo > 0 && (cfg->halo > cfg->rows || cfg->row_offset < 0 ||
                          cfg->row_offset + cfg->rows > cfg->height))
        return GOL_EINVAL;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return GOL_ENODEV;
    int dev = cfg->device;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) return GOL_ENODEV;
    if (dev >= ndev) return GOL_ENODEV;

    gol_ctx *c = new (std::nothrow) gol_ctx();
    if (!c) return GOL_ENOMEM;
    LaunchShape &s = c->shape;               // (create time: defaults and pins set in place)
    c->cfg = *cfg;
    c->cfg.device = dev;
    c->device = dev;
    c->nw = (cfg->width + 63) / 64;
    c->pitch = c->nw;
    c->buf_rows = cfg->rows + 2 * cfg->halo;
    c->fast = golk::fast_path_ok(cfg->width) && !(cfg->flags & GOL_FLAG_FORCE_GENERIC);
    c->band = cfg->band_rows > 0 ? cfg->band_rows : golk::auto_band(cfg->width, cfg->rows);
    if (const char *v = getenv("GOL_STENCIL_VARIANT")) {   // A/B experiments only
        const int k = atoi(v);
        if (k >= 0 && k < golk::kVariantCount) c->variant = k;
    }
    // temporal blocking defaults (tools/sweep.py on MI355X): 1 word per lane (more waves,
    // 87 VGPRs at K=4), K = 6 on large boards (64-row bands), K = 4 on smaller ones
    c->multi_words = 1;
    if (const char *v = getenv("GOL_MULTI_WORDS")) c->multi_words = atoi(v) == 1 ? 1 : 2;
    if (!GOL_TOOLS && c->multi_words != 1) {  // 2 words per lane: a superseded build
        delete c;
        return GOL_EINVAL;
    }
    if (const char *v = getenv("GOL_WG_PRIO")) {          // A/B experiments only: "3210" =
        for (int w = 0; w < 4 && v[w] >= '0' && v[w] <= '3'; ++w)   // wave 0..3's priority
            c->wg_prio |= (unsigned)(v[w] - '0') << (2 * w);
        if (!c->wg_prio) c->wg_prio = 0x100;              // all zero: still an override
    }
    // widths of >= 256 cells that are no multiple of 128: K1t alone blocks them (count engines:
    // it has no counted form across the seam, and they keep one rule at all these widths)
    c->tile_only = !golk::fast_path_ok(cfg->width) && cfg->width >= 256 && c->multi_words == 1 &&
                   !(cfg->flags & (GOL_FLAG_FORCE_GENERIC | GOL_FLAG_COUNT_EVERY_TURN));
    // a buffer of 2 GiB or more: the big form of K1t alone blocks it, on whole-word rows of >= 256
    // cells and with no counts (it has neither a seam nor a counted form).  GOL_TILE_BIG=1 (tests,
    // A/B runs) forces the form on a buffer of any size, and fails the create where it cannot run.
    c->tile_duo = golk::tile_duo_env();
    const char *tb = getenv("GOL_TILE_BIG");
    c->tile_big_forced = tb && atoi(tb) != 0;
    const bool big_buf = !golk::multi_fits(c->nw, c->pitch, c->buf_rows);
    const bool big_can = cfg->width >= 256 && cfg->width % 64 == 0 && c->multi_words == 1 &&
                         !(cfg->flags & (GOL_FLAG_FORCE_GENERIC | GOL_FLAG_COUNT_EVERY_TURN));
    if (c->tile_big_forced && !big_can) {
        delete c;
        return GOL_EINVAL;
    }
    c->tile_big = (big_buf || c->tile_big_forced) && big_can;
    if (c->tile_big) c->tile_only = true;                 // (K1t alone, searched: K1s / K1w stay out)
    if (c->tile_only) s.multi_variant = golk::kMultiTile;
    if (const char *v = getenv("GOL_MULTI_VARIANT")) {    // A/B experiments only
        const int k = atoi(v);
        const bool known = (k >= 0 && k < golk::kMultiUserEnd) || k > golk::kMultiAblate;
        // the product library ships only the kernels that compute the right board
        // (multi_variant_shipped); ablations, diagnostics and superseded variants need the
        // tools build (libgolamd_tools.so via GOL_AMD_LIB)
        if (!known || (!GOL_TOOLS && !golk::multi_variant_shipped(k))) {
            delete c;
            return GOL_EINVAL;
        }
        s.multi_variant = k;
        if (k != golk::kMultiTile) c->tile_only = false;   // (no other kernel runs these widths)
        if (k != golk::kMultiTile && c->tile_big) {        // (... nor such a buffer)
            if (c->tile_big_forced) {
                delete c;
                return GOL_EINVAL;
            }
            c->tile_big = false;
        }
    }
    // GOL_FLAG_RESIDENT, a request: a torus board that k_step_resident holds (by its shape:
    // golk::resident_plan) runs up to kResidentMaxTurns turns per launch in one workgroup --
    // nothing is searched, timed or pinned for it.  A depth of 1 (the caller's, or
    // GOL_TURNS_PER_LAUNCH's) switches it off like any blocking; so do a strip, a forced-generic
    // engine and a board outside the limits, which all run as without the flag.
    golk::ResidentPlan rplan;
    int rtpl = cfg->turns_per_launch > 0 ? cfg->turns_per_launch : golk::kResidentMaxTurns;
    if (const char *v = getenv("GOL_TURNS_PER_LAUNCH")) rtpl = atoi(v);
    const bool resident = (cfg->flags & GOL_FLAG_RESIDENT) && cfg->halo == 0 &&
                          !(cfg->flags & GOL_FLAG_FORCE_GENERIC) && rtpl != 1 &&
                          golk::resident_plan(cfg->width, cfg->height, &rplan);
    if (resident) s.multi_variant = golk::kMultiResident;
    const bool blockable = c->fast || c->tile_only || resident;
    const int lane_dw = golk::multi_lane_dwords(c->multi_words, s.multi_variant);
    const int auto_bm = golk::auto_band_multi(cfg->width, cfg->rows, lane_dw);
    const bool wg = golk::is_wg_variant(s.multi_variant);
    s.tpl = cfg->turns_per_launch > 0 ? cfg->turns_per_launch
                                      : (wg ? 16 : (auto_bm >= 48 ? 8 : 6));
    if (const char *v = getenv("GOL_TURNS_PER_LAUNCH")) s.tpl = atoi(v);
    s.tpl = std::max(1, std::min(s.tpl, golk::multi_max_turns(s.multi_variant)));
    if (resident) s.tpl = std::max(2, std::min(rtpl, golk::kResidentMaxTurns));
    if (blockable && s.tpl > 1 && big_buf && !c->tile_big)
        c->blocking_limited = true;   // reported in gol_info.blocking_limited
    if (!blockable || c->blocking_limited) s.tpl = 1;
    c->halo_valid = cfg->halo;
    if (cfg->flags & GOL_FLAG_COUNT_EVERY_TURN) {
        const char *v = getenv("GOL_COUNT_BLOCKING");    // 0: one-turn launches (A/B, probes)
        c->count_blocking = !v || atoi(v) != 0;
    }
    const bool cntb = c->count_blocking;

    DeviceGuard g(dev);
    (void)hipDeviceGetAttribute(&c->ncu, hipDeviceAttributeMultiprocessorCount, dev);
    s.band_multi = resident ? rplan.rows : cfg->band_rows;   // (resident: the rows per lane)
    if (s.band_multi <= 0 && s.tpl > 1) {
        const int ncu = c->ncu;
        const int bpc = golk::multi_blocks_per_cu(s.tpl, c->multi_words, s.multi_variant);
        s.band_multi = golk::pick_band_multi(cfg->width, cfg->rows, lane_dw, s.tpl,
                                             ncu * bpc *
                                                 golk::multi_pipes_per_block(s.multi_variant),
                                             s.multi_variant);
    }
    if (s.band_multi <= 0) s.band_multi = golk::auto_band_multi(cfg->width, cfg->rows, lane_dw);
    const size_t words = (size_t)c->buf_rows * c->pitch;
    int rc = GOL_OK;
    auto bail = [&](int code) {
        gol_destroy(c);
        return code;
    };
    hipError_t e;
    if ((e = hipMalloc(&c->board[0], words * 8)) != hipSuccess ||
        (e = hipMalloc(&c->board[1], words * 8)) != hipSuccess ||
        (e = hipMalloc(&c->counts, (size_t)(kRingSlots + 1) * kShards * 8)) != hipSuccess ||
        (e = hipHostMalloc(&c->h_counts, kShards * 8, hipHostMallocDefault)) != hipSuccess ||
        (e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&c->ev_side, hipEventDisableTiming)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&c->ev_main, hipEventDisableTiming)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&c->ev_copy, hipEventDisableTiming)) != hipSuccess ||
        (e = hipHostMalloc((void **)&c->h_err, sizeof(unsigned),
                           hipHostMallocMapped | hipHostMallocCoherent)) != hipSuccess ||
        (e = hipHostGetDevicePointer((void **)&c->d_err, c->h_err, 0)) != hipSuccess) {
        rc = e == hipErrorOutOfMemory ? GOL_ENOMEM : GOL_EHIP;
        return bail(rc);
    }
    clear_dev_err(c);
    {
        std::lock_guard<std::mutex> lk(g_dev_mu);
        ++g_dev_engines[dev];
        c->registered = true;
    }
    c->stream = c->own_stream;
    // small boards (and k_step_tile pinned by GOL_MULTI_VARIANT): k_step_tile at the model's
    // best shape for the requested or default depth; the autotune below times the model's best
    // shapes
    // (a tile_only engine of any size plans like a small board: k_step_tile, searched)
    const bool small = blockable && s.tpl > 1 &&
                       (c->tile_only || (long long)c->buf_rows * c->pitch < (1ll << 20));
    const bool pinned = getenv("GOL_MULTI_VARIANT") != nullptr;
    if (blockable && s.tpl > 1 && !resident &&
        ((small && !pinned && cfg->band_rows <= 0) || s.multi_variant == golk::kMultiTile))
        if (int rc2 = initial_tile_shape(c, cntb)) {
            // a tile_only board no tile shape fits (a few rows) and nothing pinned: one turn per
            // launch, as before; every other failure is the caller's shape
            if (!c->tile_only || pinned || getenv("GOL_TILE") || cfg->band_rows > 0 ||
                c->tile_big_forced)
                return bail(rc2);
            if (c->tile_big) {                   // (2 GiB of a few rows: no window fits)
                c->tile_big = false;
                c->blocking_limited = big_buf;
            }
            LaunchShape one;
            one.multi_variant = golk::kMultiTile;
            set_shape(c, std::move(one));
        }
    const char *at = getenv("GOL_AUTOTUNE");
    bool tuning = !(cfg->flags & GOL_FLAG_NO_AUTOTUNE) && (!at || atoi(at) != 0) &&
                  cfg->band_rows <= 0 && s.tpl > 1 && !resident;
    // a BASELINE board size on an MI355X: the pinned shape, no search (GOL_AUTOTUNE=2: search);
    // the first engine of the shape in this process times it once (check_pinned: a warning
    // when slow, never a different shape)
    KnownShape ks{};
    if (tuning && !pinned && cfg->turns_per_launch <= 0 && !getenv("GOL_TILE") &&
        !(at && atoi(at) == 2) && known_shape(c, &ks)) {
        apply_tile(c, ks.t);
        if (ks.short_K >= 2 && ks.short_K < ks.t.K &&
            golk::tile_shape_ok(c->nw, ks.short_K, ks.short_th, ks.t.tw, ks.t.seg) &&
            (!c->tile_big || golk::tile_big_ok(cfg->width, c->buf_rows, c->pitch, ks.short_K,
                                               ks.short_th, ks.t.seg))) {
            s.short_k = ks.short_K;
            s.short_band = ks.short_th;
        }
        s.tuned_us_per_turn = ks.us_per_turn;
        c->shape_source = 2;
        tuning = false;
        (void)check_pinned(c, ks);
    }
    const bool tune_small = small && s.multi_variant == golk::kMultiTile && !pinned &&
                            cfg->turns_per_launch <= 0;
    // the kernel is tuned too unless an experiment pins it (GOL_MULTI_VARIANT) or the requested
    // depth only one of them runs
    const bool tune_var = !pinned && c->multi_words == 1 &&
                          (cfg->turns_per_launch <= 0 || cfg->turns_per_launch <= 8);
    const TuneKey key{dev, cfg->width, c->buf_rows, cfg->turns_per_launch,
                      (tune_small ? 4 : 0) | (tune_var ? 2 : 0) | (pinned ? 1 : 0) |
                          (s.multi_variant << 3) | (cntb ? 1 << 24 : 0) |
                          (c->tile_big ? 1 << 25 : 0)};
    const char *tc = getenv("GOL_AUTOTUNE_CACHE");
    const bool use_cache = !tc || atoi(tc) != 0;
    bool cached = false;
    LaunchShape hit;
    if (tuning && use_cache && tune_cache_lookup(key, &hit)) {
        set_shape(c, std::move(hit));
        c->shape_source = 1;
        cached = true;
    }
    if (tuning && !cached && (tune_small || !small)) {
        if (tune_small) autotune_small(c);
        else autotune_multi(c, cfg->turns_per_launch <= 0, tune_var);
        c->shape_source = 1;
        // a wait that gave up while timing the candidates: fail loudly at create
        (void)hipStreamSynchronize(c->stream);
        if (check_dev_err(c)) return bail(GOL_EHIP);
        if (use_cache) tune_cache_store(key, c->shape);
    }
    if ((e = hipMemsetAsync(c->board[0], 0, words * 8, c->stream)) != hipSuccess ||
        (e = hipMemsetAsync(c->board[1], 0, words * 8, c->stream)) != hipSuccess ||
        (e = hipMemsetAsync(c->counts, 0, (size_t)(kRingSlots + 1) * kShards * 8, c->stream)) !=
            hipSuccess ||
        (e = hipStreamSynchronize(c->stream)) != hipSuccess)
        return bail(GOL_EHIP);
    c->prev_valid = false;                   // (the timing launches above stepped the buffers)
    *out = c;
    return GOL_OK;
}

void gol_destroy(gol_ctx *c)
{
    if (!c) return;
    if (c->registered) {
        std::lock_guard<std::mutex> lk(g_dev_mu);
        if (--g_dev_engines[c->device] <= 0) g_dev_engines.erase(c->device);
    }
    {
        DeviceGuard g(c->device);
        if (c->own_stream) (void)hipStreamSynchronize(c->own_stream);
        if (c->stream && c->stream != c->own_stream) (void)hipStreamSynchronize(c->stream);
        if (c->side) (void)hipStreamSynchronize(c->side);
        if (c->board[0]) (void)hipFree(c->board[0]);
        if (c->board[1]) (void)hipFree(c->board[1]);
        if (c->pg_rows) (void)hipFree(c->pg_rows);
        if (c->pg_flags) (void)hipFree(c->pg_flags);
        blocks_free(c);
        if (c->blocked) (void)hipFree(c->blocked);
        if (c->counts) (void)hipFree(c->counts);
        if (c->staging) (void)hipFree(c->staging);
        if (c->flip_rows) (void)hipFree(c->flip_rows);
        if (c->h_flip_total) (void)hipHostFree(c->h_flip_total);
        if (c->h_counts) (void)hipHostFree(c->h_counts);
        if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
        if (c->side) (void)hipStreamDestroy(c->side);
        if (c->ev_side) (void)hipEventDestroy(c->ev_side);
        if (c->ev_main) (void)hipEventDestroy(c->ev_main);
        for (auto &set : c->chunk_ev)
            for (hipEvent_t e : set)
                if (e) (void)hipEventDestroy(e);
        if (c->ev_copy) (void)hipEventDestroy(c->ev_copy);
        if (c->h_err) (void)hipHostFree(c->h_err);
    }
    delete c;
}

int gol_get_info(gol_ctx *c, gol_info *info)
{
    if (!c || !info) return GOL_EINVAL;
    return run_read(c, [&]() -> int {
        info->width = c->cfg.width;
        info->height = c->cfg.height;
        info->row_offset = c->cfg.row_offset;
        info->rows = c->cfg.rows;
        info->halo = c->cfg.halo;
        info->words_per_row = c->nw;
        info->pitch_words = c->pitch;
        info->buffer_rows = c->buf_rows;
        info->fast_path = c->fast ? 1 : 0;
        // band of the kernel in use
        info->band_rows = c->shape.tpl > 1 ? c->shape.band_multi : c->band;
        info->halo_valid = c->halo_valid;
        info->turns_per_launch = c->shape.tpl;
        info->device = c->device;
        info->turn = c->turn;
        info->nonbinary_cells = c->nonbinary;
        info->launches = c->launches;
        info->blocking_limited = c->blocking_limited ? 1 : 0;
        info->shape_source = c->shape_source;
        return GOL_OK;
    });
}

int gol_set_stream(gol_ctx *c, void *s)
{
    if (!c) return GOL_EINVAL;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    DeviceGuard g(c->device);
    // order the switch: everything queued on the old stream completes first
    HIP_OR_FAIL(c, hipStreamSynchronize(c->stream));
    c->stream = s ? (hipStream_t)s : c->own_stream;
    return GOL_OK;
}

void *gol_get_stream(gol_ctx *c) { return c ? (void *)c->stream : nullptr; }

int gol_sync(gol_ctx *c)
{
    if (!c) return GOL_EINVAL;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    DeviceGuard g(c->device);
    return sync_checked(c);
}

}  // extern "C"

// ------------------------------------------------- internal (driver) access
namespace golint {
long long engine_turn(gol_ctx *c) { return c->turn; }
int engine_device(gol_ctx *c) { return c->device; }
}  // namespace golint
