// gol_blocks.cpp — the host side of K1p / K1q / K1r (k_tile_persist, k_tile_stream,
// k_tile_ring): many blocks of turns in one launch, tiles handing their edges over through
// uncached buffers.  The kernels exist in the tools build only (make tools, -DGOL_TOOLS=1); the
// product library gets the stubs at the end of this file.  Also tools-only: the k_step_wg wait
// diagnostic launch (wg_diag_launch).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <iterator>

#include "gol_ctx.h"

namespace goleng {

#if GOL_TOOLS

namespace {

// K1p / K1q: the uncached block buffers (board-sized), per-tile flags and the item counter,
// allocated on first use (the engine's streams drained first)
hipError_t persist_buffers(gol_ctx *c, long long ntiles)
{
    BlockState &b = c->blocks;
    const size_t words = (size_t)c->buf_rows * c->pitch;
    if (b.pu[0] && b.pu[1] && (size_t)ntiles <= b.pflags_n && b.pcounter) return hipSuccess;
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return e;
    for (auto *&u : b.pu)
        if (!u && (e = hipExtMallocWithFlags((void **)&u, words * 8, hipDeviceMallocUncached)) !=
                      hipSuccess)
            return e;
    if (!b.pcounter) {
        if ((e = hipExtMallocWithFlags((void **)&b.pcounter, 64, hipDeviceMallocUncached)) !=
                hipSuccess ||
            (e = hipMemset(b.pcounter, 0, 64)) != hipSuccess ||
            (e = hipDeviceSynchronize()) != hipSuccess)
            return e;
        b.pcount = 0;
    }
    if ((size_t)ntiles > b.pflags_n) {
        if (b.pflags) (void)hipFree(b.pflags);
        b.pflags = nullptr;
        b.pflags_n = 0;
        if ((e = hipExtMallocWithFlags((void **)&b.pflags, (size_t)ntiles * sizeof(unsigned),
                                       hipDeviceMallocUncached)) != hipSuccess ||
            (e = hipMemset(b.pflags, 0, (size_t)ntiles * sizeof(unsigned))) != hipSuccess ||
            (e = hipDeviceSynchronize()) != hipSuccess)
            return e;
        b.pflags_n = (size_t)ntiles;
        b.pepoch = 0;
    }
    return hipSuccess;
}

// K1p: one launch of `turns` turns in blocks of K on resident tiles
hipError_t persist_launch(gol_ctx *c, golk::StepArgs a, int turns, int K)
{
    BlockState &b = c->blocks;
    const long long ntiles = golk::tile_count(c->nw, a.row_hi - a.row_lo, a.band, a.tile_w,
                                              a.tile_seg);
    if (hipError_t e = persist_buffers(c, ntiles)) return e;
    // flags of earlier launches are at most their epoch + blocks - 1: start above them all
    const unsigned nblocks = (unsigned)((turns + K - 1) / K);
    const unsigned epoch = b.pepoch + 1;
    b.pepoch = epoch + nblocks;
    if (b.persist_ring) {                    // K1r: only the rings pass through u0 / u1
        // (GOL_RING=2, experiments: a grid-wide barrier per block on K1q's counter)
        const bool grid = getenv("GOL_RING") && atoi(getenv("GOL_RING")) == 2;
        const unsigned base = b.pcount;
        if (grid) b.pcount += (unsigned)ntiles * (nblocks - 1);
        return golk::launch_tile_ring(a, turns, K, b.pu[0], b.pu[1], b.pflags, epoch,
                                      grid ? b.pcounter : nullptr, base, c->stream);
    }
    return golk::launch_tile_persist(a, turns, K, b.pu[0], b.pu[1], b.pflags, epoch, c->stream);
}

// K1q: one launch of `turns` turns in blocks of K, (block, tile) items taken from the counter
hipError_t stream_launch(gol_ctx *c, golk::StepArgs a, int turns, int K)
{
    BlockState &b = c->blocks;
    const long long ntiles = golk::tile_count(c->nw, a.row_hi - a.row_lo, a.band, a.tile_w,
                                              a.tile_seg);
    if (hipError_t e = persist_buffers(c, ntiles)) return e;
    for (auto *&u : b.su)
        if (!u) {
            hipError_t e = hipStreamSynchronize(c->stream);
            if (e == hipSuccess) e = hipMalloc((void **)&u, (size_t)c->buf_rows * c->pitch * 8);
            if (e != hipSuccess) return e;
        }
    const unsigned nblocks = (unsigned)((turns + K - 1) / K);
    const unsigned epoch = b.pepoch + 1;
    unsigned grid = 0;
    // GOL_STREAM_GRID (tests): cap the workgroups, so that each takes many items
    const int max_grid = getenv("GOL_STREAM_GRID") ? atoi(getenv("GOL_STREAM_GRID")) : 0;
    const hipError_t e = golk::launch_tile_stream(a, turns, K, b.su[0], b.su[1], b.pflags,
                                                  epoch, b.pcounter, b.pcount, c->ncu, max_grid,
                                                  &grid, c->stream);
    if (e != hipSuccess) return e;
    b.pepoch = epoch + nblocks;
    b.pcount += (unsigned)(ntiles * nblocks) + grid;   // items + one overshoot per workgroup
    return hipSuccess;
}

}  // namespace

int blocks_parse_env(gol_ctx *c)
{
    LaunchShape &s = c->shape;
    if (const char *v = getenv("GOL_PERSIST")) {       // tests / experiments: K1p blocks
        const int pk = atoi(v);
        if (pk > 0) {
            const char *rv = getenv("GOL_RING");
            const bool ring = rv && atoi(rv) > 0;
            if (s.multi_variant != golk::kMultiTile || is_strip(c) ||
                !(ring ? golk::tile_ring_ok(c->nw, c->buf_rows, pk, s.band_multi, s.tile_w,
                                            s.tile_seg, c->ncu)
                       : golk::tile_persist_ok(c->nw, c->buf_rows, 2 * pk, pk, s.band_multi,
                                               s.tile_w, s.tile_seg, c->ncu)))
                return GOL_EINVAL;
            s.persist_k = pk;
            c->blocks.persist_forced = true;
            c->blocks.persist_ring = ring;
        }
    }
    if (const char *v = getenv("GOL_STREAM")) {        // tests / experiments: K1q blocks
        const int sk = atoi(v);
        if (sk > 0) {
            if (s.multi_variant != golk::kMultiTile || is_strip(c) ||
                !golk::tile_stream_ok(c->nw, c->buf_rows, sk, s.band_multi, s.tile_w, s.tile_seg))
                return GOL_EINVAL;
            s.stream_k = sk;
            c->blocks.stream_forced = true;
            s.stream_tw = s.tile_w;
            s.stream_th = s.band_multi;
            s.stream_seg = s.tile_seg;
        }
    }
    return GOL_OK;
}

// K1p for a small torus board at the tuned tile shape: 256 turns as one k_tile_persist launch
// (blocks of Kp turns, tiles resident between blocks) against the same turns as k_step_tile
// launches of the tuned depth, best of 3 each; the persistent mode is kept (at its fastest
// block depth) when it is >= 2 % faster.  Only on a device this engine has to itself: every
// tile must be resident at once.
void blocks_tune_persist(gol_ctx *c)
{
    LaunchShape &s = c->shape;
    s.persist_k = 0;
    s.persist_seg = 0;
    const bool log = getenv("GOL_AUTOTUNE_LOG") != nullptr;
    if (is_strip(c) || s.multi_variant != golk::kMultiTile || !device_exclusive(c->device) ||
        getenv("GOL_NO_PERSIST")) {
        if (log)
            fprintf(stderr, "autotune persist skipped (strip %d variant %d exclusive %d)\n",
                    (int)is_strip(c), s.multi_variant, (int)device_exclusive(c->device));
        return;
    }
    golk::StepArgs a = whole_buffer_args(c);
    a.multi_variant = golk::kMultiTile;
    a.band = s.band_multi;
    a.tile_w = s.tile_w;
    a.tile_seg = s.tile_seg;
    const int N = 256;
    LaunchTimer timer(c->stream);
    if (!timer.ok()) return;
    auto timed = [&](auto &&launches) -> float {       // us per turn, best of 3
        float best = 0.f;
        for (int pass = 0; pass < 3; ++pass) {
            const float ms = timer.ms(launches);
            if (ms <= 0.f) return 0.f;
            const float us = ms * 1000.f / N;
            if (best == 0.f || us < best) best = us;
        }
        return best;
    };
    const float plain = timed([&]() {
        const int n = (N + s.tpl - 1) / s.tpl;
        for (int i = 0; i < n; ++i) {
            a.in = c->board[i & 1];
            a.out = c->board[(i + 1) & 1];
            const int k = N / n + (i < N % n ? 1 : 0);
            if (golk::launch_step_multi(a, k, c->stream) != hipSuccess) return false;
        }
        return true;
    });
    // the tuned code and its siblings with the same rows per segment (K1p is instantiated for
    // ORD 0, 1, 4 and 5 only: an ORD 2 pick runs persistent as one of those)
    float best = 0.f;
    int best_k = 0, best_code = 0;
    const int sg = s.tile_seg % 100;
    const int codes[] = {s.tile_seg, 100 + sg, 500 + sg, 400 + sg, sg};
    for (int ci = 0; ci < (int)std::size(codes); ++ci) {
        const int code = codes[ci];
        if (s.tile_seg >= 1000 || (ci > 0 && code == s.tile_seg)) continue;   // (W = 1 only)
        a.tile_seg = code;
        for (int Kp : {s.tpl, 8, 12, 16, 20, 24, 32}) {
            if (Kp < 2 || !golk::tile_persist_ok(c->nw, c->buf_rows, N, Kp, s.band_multi,
                                                 s.tile_w, code, c->ncu)) {
                if (log)
                    fprintf(stderr, "autotune persist K=%d: shape %d:%d:%d not persistent-capable\n",
                            Kp, s.tile_w, s.band_multi, code);
                continue;
            }
            const float us = timed([&]() {
                a.in = c->board[0];
                a.out = c->board[1];
                return persist_launch(c, a, N, Kp) == hipSuccess;
            });
            if (log)
                fprintf(stderr, "autotune persist %dx%d code=%d K=%d us_per_turn=%.4f (plain K=%d %.4f)\n",
                        c->cfg.width, c->buf_rows, code, Kp, us, s.tpl, plain);
            if (us > 0.f && (best == 0.f || us < best)) {
                best = us;
                best_k = Kp;
                best_code = code;
            }
        }
    }
    // (a wait that gave up while timing: no persistent mode, and the junk board's error word
    // is cleared -- the board is refilled before use)
    const bool bad = check_dev_err(c) != GOL_OK;
    if (bad) clear_dev_err(c);
    if (best > 0.f && plain > 0.f && best < 0.98f * plain && !bad) {
        s.persist_k = best_k;
        s.persist_seg = best_code;           // (plain launches keep the code they were timed at)
        s.tuned_us_per_turn = best;
    }
}

// K1q for the tile family: 240 turns as one k_tile_stream launch in blocks of Kp
// turns (one start and one tail instead of one per launch), against the tuned
// steady rate; kept when >= 2 % faster.  Torus engines only (a strip's halo window
// shrinks its rows from launch to launch).
float blocks_tune_stream(gol_ctx *c, golk::StepArgs a, const LaunchFamily *tf, float best_ms)
{
    LaunchShape &s = c->shape;
    s.stream_k = 0;
    if (is_strip(c) || getenv("GOL_NO_STREAM")) return 0.f;
    LaunchTimer timer(c->stream);
    const int N = 240;
    float sbest = 0.f;
    int sk = 0, sband = 0;
    for (int Kp : {tf ? tf->K : 0, 24}) {
        if (!tf || Kp < 2 || Kp > golk::kMaxTurnsPerLaunch || tf->band_k[Kp] <= 0)
            continue;
        // equal tile rows (the same count): a last tile row shorter than K would take
        // its halo from two tile rows up
        const int nty = (c->buf_rows + tf->band_k[Kp] - 1) / tf->band_k[Kp];
        const int th = (c->buf_rows + nty - 1) / nty;
        if (!golk::tile_stream_ok(c->nw, c->buf_rows, Kp, th, tf->tw, tf->seg)) continue;
        a.band = th;
        a.multi_variant = golk::kMultiTile;
        a.tile_w = tf->tw;
        a.tile_seg = tf->seg;
        a.in = c->board[0];
        a.out = c->board[1];
        float v = 0.f;
        for (int pass = 0; pass < 3; ++pass) {
            const float ms = timer.ms([&] { return stream_launch(c, a, N, Kp) == hipSuccess; });
            if (ms > 0.f && (v == 0.f || ms / N < v)) v = ms / N;
        }
        if (getenv("GOL_AUTOTUNE_LOG"))
            fprintf(stderr, "autotune stream %dx%d K=%d band=%d tile=%d,%d us_per_turn=%.3f "
                    "(tuned %.3f)\n", c->cfg.width, c->buf_rows, Kp, a.band, tf->tw, tf->seg,
                    v * 1000.f, best_ms * 1000.f);
        if (v > 0.f && (sbest == 0.f || v < sbest)) {
            sbest = v;
            sk = Kp;
            sband = a.band;
        }
    }
    // (a wait that gave up while timing: no K1q, and the junk board's error word is
    // cleared -- the board is refilled before use)
    const bool bad = check_dev_err(c) != GOL_OK;
    if (bad) clear_dev_err(c);
    if (!sk || !(sbest < 0.98f * best_ms) || bad) return 0.f;
    s.stream_k = sk;
    s.stream_tw = tf->tw;
    s.stream_th = sband;
    s.stream_seg = tf->seg;
    return sbest;
}

bool blocks_plan(gol_ctx *c, int64_t room, Launch *out)
{
    const LaunchShape &s = c->shape;
    // (another engine on the device could hold CUs the resident tiles need: then plain
    // launches -- a starved wait would give up and report GOL_EHIP, but never hang)
    if (s.persist_k > 0 && !is_strip(c) && room >= 2 * s.persist_k &&
        (c->blocks.persist_forced || device_exclusive(c->device))) {
        // K1p: blocks of <= persist_k turns in one launch, up to ~1 ms of work per launch so
        // the control word and readers are still served every millisecond or so
        const double us = s.tuned_us_per_turn > 0.f ? s.tuned_us_per_turn : 1.0;
        const int64_t cap = std::max<int64_t>(2 * s.persist_k, (int64_t)(1000.0 / us));
        *out = Launch{(int)std::min<int64_t>(room, cap), golk::kMultiTilePersist, s.band_multi,
                      s.tile_w, s.persist_seg ? s.persist_seg : s.tile_seg, s.persist_k};
        return true;
    }
    if (s.stream_k > 0 && !is_strip(c) && room >= 2 * s.stream_k) {
        // K1q: blocks of <= stream_k turns in one launch, up to ~8 ms of work per launch (the
        // control word and readers are served between launches)
        const double us = s.tuned_us_per_turn > 0.f ? s.tuned_us_per_turn : 1.0;
        const int64_t cap = std::max<int64_t>(2 * s.stream_k, (int64_t)(8000.0 / us));
        *out = Launch{(int)std::min<int64_t>(room, cap), golk::kMultiTileStream, s.stream_th,
                      s.stream_tw, s.stream_seg, s.stream_k};
        return true;
    }
    return false;
}

hipError_t blocks_launch(gol_ctx *c, const golk::StepArgs &a, const Launch &L)
{
    return L.var == golk::kMultiTilePersist ? persist_launch(c, a, L.k, L.blk)
                                            : stream_launch(c, a, L.k, L.blk);
}

void blocks_free(gol_ctx *c)
{
    BlockState &b = c->blocks;
    for (auto *u : b.pu)
        if (u) (void)hipFree(u);
    for (auto *u : b.su)
        if (u) (void)hipFree(u);
    if (b.pcounter) (void)hipFree(b.pcounter);
    if (b.pflags) (void)hipFree(b.pflags);
}

// GOL_MULTI_VARIANT=kMultiWgDiag: one k_step_wg launch with per-wave wait timing, summarised by
// wave role on stderr (tools/wg_diag.py reads the lines).
int wg_diag_launch(gol_ctx *c, golk::StepArgs a, int k)
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

#else  // the product library: no K1p / K1q / K1r kernels

int blocks_parse_env(gol_ctx *)
{
    for (const char *name : {"GOL_PERSIST", "GOL_STREAM"})
        if (const char *v = getenv(name))
            if (atoi(v) > 0) return GOL_EINVAL;
    return GOL_OK;
}

void blocks_tune_persist(gol_ctx *) {}
float blocks_tune_stream(gol_ctx *, golk::StepArgs, const LaunchFamily *, float) { return 0.f; }
bool blocks_plan(gol_ctx *, int64_t, Launch *) { return false; }
hipError_t blocks_launch(gol_ctx *, const golk::StepArgs &, const Launch &)
{
    return hipErrorInvalidValue;
}
void blocks_free(gol_ctx *) {}

#endif  // GOL_TOOLS

}  // namespace goleng
