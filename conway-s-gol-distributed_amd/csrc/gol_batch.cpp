// gol_batch.cpp -- K1r2b, the batched resident engine behind the "Batch" section of
// include/gol_amd.h: B torus boards of one shape narrower than 256 cells in one allocation, every
// step one k_step_resident_batch launch per 256 turns with one workgroup per board
// (gol_resident.hip).  One thread drives a batch: no lock, no cross-thread services, no control
// word.  The boards are stepped in place (one buffer, no double buffer), so nothing here needs a
// "current half".
// K1r2s, the "Settle" section: gol_settle_step advances the same boards with
// k_settle_resident_batch (gol_settle.hip), which watches every board for its period; the watch's
// state (one SettleState and one snapshot per board) is allocated at the first gol_settle_step.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "gol_ctx.h"
#include "gol_resident.h"
#include "gol_settle.h"

using goleng::DeviceGuard;

struct gol_batch {
    int device = -1;
    int width = 0, height = 0, boards = 0, nw = 0;
    uint32_t flags = 0;
    golk::ResidentPlan plan;
    hipStream_t stream = nullptr;            // its own
    uint64_t *words = nullptr;               // boards x height x nw, board b at b x height x nw
    uint32_t *counts = nullptr;              // GOL_FLAG_COUNT_EVERY_TURN: [turn % 256][board]
    uint32_t *alive = nullptr;               // gol_batch_alive: one count per board (first call on)
    long long turn = 0;                      // completed turns since the last whole-batch load
    uint64_t *snaps = nullptr;               // gol_settle_step: a snapshot per board (first call on)
    golk::SettleState *states = nullptr;     //   and its watch
    bool watching = false;                   // a watch is on: since a gol_settle_step, until a reset
    std::string err;
    void *staging = nullptr;                 // page-locked host memory, grows on demand
    size_t staging_size = 0;
    size_t board_words() const { return (size_t)height * nw; }
};

namespace {

// words staged per chunk of a byte load or read-out (whole boards: a board is at most 32 KiB)
constexpr size_t kBatchStagingBytes = 64u << 20;

int bfail(gol_batch *b, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    b->err = buf;
    return code;
}

#define BATCH_HIP(b, expr)                                                                     \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return bfail((b), e_ == hipErrorOutOfMemory ? GOL_ENOMEM : GOL_EHIP, "%s: %s (%s:%d)", \
                         #expr, hipGetErrorString(e_), __FILE__, __LINE__);                    \
    } while (0)

int ensure_staging(gol_batch *b, size_t bytes)
{
    if (b->staging_size >= bytes) return GOL_OK;
    if (b->staging) (void)hipHostFree(b->staging);
    b->staging = nullptr;
    b->staging_size = 0;
    BATCH_HIP(b, hipHostMalloc(&b->staging, bytes, hipHostMallocDefault));
    b->staging_size = bytes;
    return GOL_OK;
}

// boards [first, first + n) lie in the batch (n >= 1)
bool range_ok(const gol_batch *b, int32_t first, int32_t n)
{
    return first >= 0 && n >= 1 && (long long)first + n <= b->boards;
}

// boards per staged chunk
int chunk_boards(const gol_batch *b, int32_t n)
{
    const size_t per = kBatchStagingBytes / (b->board_words() * 8);
    return (int)std::max<size_t>(1, std::min<size_t>(per, (size_t)n));
}

// the watch of boards first .. first + n - 1 begins at the batch's turn, with snapshot 0 = the
// boards as they are (queued on the batch's stream)
int watch_from_here(gol_batch *b, int32_t first, int32_t n)
{
    const size_t bw = b->board_words();
    BATCH_HIP(b, hipMemcpyAsync(b->snaps + (size_t)first * bw, b->words + (size_t)first * bw,
                                (size_t)n * bw * 8, hipMemcpyDeviceToDevice, b->stream));
    BATCH_HIP(b, golk::launch_settle_init(b->states, first, n, b->turn, b->stream));
    return GOL_OK;
}

// after a load of boards first .. first + n - 1: a whole-batch load sets the turn to 0 and ends
// the watch; a partial load under a watch restarts the watch of its boards
int loaded(gol_batch *b, int32_t first, int32_t n)
{
    if (first == 0 && n == b->boards) {
        b->turn = 0;
        b->watching = false;
        return GOL_OK;
    }
    if (!b->watching) return GOL_OK;
    if (int rc = watch_from_here(b, first, n)) return rc;
    BATCH_HIP(b, hipStreamSynchronize(b->stream));
    return GOL_OK;
}

// GOL_SETTLE_DEPTH=D in the environment (read at every gol_settle_step): launches of at most D
// turns, 1 .. kSettleMaxDepth; anything else: kSettleMaxDepth
int settle_depth()
{
    const char *v = getenv("GOL_SETTLE_DEPTH");
    const int d = v ? atoi(v) : 0;
    return d >= 1 && d <= golk::kSettleMaxDepth ? d : golk::kSettleMaxDepth;
}

}  // namespace

// ================================================================ C ABI
extern "C" {

int gol_batch_create(int32_t width, int32_t height, int32_t boards, int32_t device, uint32_t flags,
                     gol_batch **out)
{
    if (!out) return GOL_EINVAL;
    *out = nullptr;
    golk::ResidentPlan plan;
    if ((flags & ~GOL_FLAG_COUNT_EVERY_TURN) || boards < 1 || device < -1 ||
        !golk::resident_plan(width, height, &plan) || (long long)boards * height > INT32_MAX)
        return GOL_EINVAL;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return GOL_ENODEV;
    int dev = device;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) return GOL_ENODEV;
    if (dev >= ndev) return GOL_ENODEV;

    gol_batch *b = new (std::nothrow) gol_batch();
    if (!b) return GOL_ENOMEM;
    b->device = dev;
    b->width = width;
    b->height = height;
    b->boards = boards;
    b->nw = (width + 63) / 64;
    b->flags = flags;
    b->plan = plan;
    DeviceGuard g(dev);
    const size_t bytes = (size_t)boards * b->board_words() * 8;
    const size_t cbytes = (size_t)golk::kResidentMaxTurns * boards * sizeof(uint32_t);
    hipError_t e;
    if ((e = hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipMalloc((void **)&b->words, bytes)) != hipSuccess ||
        ((flags & GOL_FLAG_COUNT_EVERY_TURN) &&
         (e = hipMalloc((void **)&b->counts, cbytes)) != hipSuccess) ||
        (e = hipMemsetAsync(b->words, 0, bytes, b->stream)) != hipSuccess ||
        (b->counts && (e = hipMemsetAsync(b->counts, 0, cbytes, b->stream)) != hipSuccess) ||
        (e = hipStreamSynchronize(b->stream)) != hipSuccess) {
        (void)hipGetLastError();
        gol_batch_destroy(b);
        return e == hipErrorOutOfMemory ? GOL_ENOMEM : GOL_EHIP;
    }
    *out = b;
    return GOL_OK;
}

void gol_batch_destroy(gol_batch *b)
{
    if (!b) return;
    {
        DeviceGuard g(b->device);
        if (b->stream) (void)hipStreamSynchronize(b->stream);
        if (b->words) (void)hipFree(b->words);
        if (b->counts) (void)hipFree(b->counts);
        if (b->alive) (void)hipFree(b->alive);
        if (b->snaps) (void)hipFree(b->snaps);
        if (b->states) (void)hipFree(b->states);
        if (b->staging) (void)hipHostFree(b->staging);
        if (b->stream) (void)hipStreamDestroy(b->stream);
    }
    delete b;
}

const char *gol_batch_last_error(const gol_batch *b) { return b ? b->err.c_str() : ""; }

int gol_batch_get_info(gol_batch *b, int32_t *width, int32_t *height, int32_t *boards,
                       int32_t *words_per_row, int32_t *lanes, int32_t *rows_per_lane,
                       int32_t *waves, int64_t *turn)
{
    if (!b) return GOL_EINVAL;
    if (width) *width = b->width;
    if (height) *height = b->height;
    if (boards) *boards = b->boards;
    if (words_per_row) *words_per_row = b->nw;
    if (lanes) *lanes = b->plan.lanes;
    if (rows_per_lane) *rows_per_lane = b->plan.rows;
    if (waves) *waves = b->plan.waves;
    if (turn) *turn = b->turn;
    return GOL_OK;
}

int gol_batch_occupancy(gol_batch *b, int32_t *blocks_per_cu, int32_t *cus)
{
    if (!b || !blocks_per_cu || !cus) return GOL_EINVAL;
    DeviceGuard g(b->device);
    int ncu = 0;
    BATCH_HIP(b, hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, b->device));
    const int n = golk::resident_batch_blocks_per_cu(b->width, b->height, b->counts != nullptr);
    if (n <= 0) return bfail(b, GOL_EHIP, "gol_batch_occupancy: the occupancy query failed");
    *blocks_per_cu = n;
    *cus = ncu;
    return GOL_OK;
}

void *gol_batch_get_stream(gol_batch *b) { return b ? (void *)b->stream : nullptr; }

int gol_batch_sync(gol_batch *b)
{
    if (!b) return GOL_EINVAL;
    DeviceGuard g(b->device);
    BATCH_HIP(b, hipStreamSynchronize(b->stream));
    return GOL_OK;
}

int gol_batch_load_packed(gol_batch *b, int32_t first, int32_t n, const uint64_t *words)
{
    if (!b || !words) return GOL_EINVAL;
    if (!range_ok(b, first, n))
        return bfail(b, GOL_EINVAL, "gol_batch_load_packed: boards %d .. %lld are not in a batch of %d",
                     first, (long long)first + n - 1, b->boards);
    // gol_load_packed's padding rule, checked on the host before anything is copied
    if (const int nb = b->width & 63) {
        const uint64_t pad = ~0ull << nb;
        for (int32_t i = 0; i < n; ++i)
            for (int r = 0; r < b->height; ++r)
                if (words[((size_t)i * b->height + r) * b->nw + b->nw - 1] & pad)
                    return bfail(b, GOL_EINVAL,
                                 "gol_batch_load_packed: board %d, row %d has bits set past width %d "
                                 "in its last word (the batch is unchanged)", first + i, r, b->width);
    }
    DeviceGuard g(b->device);
    const size_t bw = b->board_words();
    BATCH_HIP(b, hipMemcpyAsync(b->words + (size_t)first * bw, words, (size_t)n * bw * 8,
                                hipMemcpyHostToDevice, b->stream));
    BATCH_HIP(b, hipStreamSynchronize(b->stream));
    return loaded(b, first, n);
}

int gol_batch_load(gol_batch *b, int32_t first, int32_t n, const uint8_t *bytes)
{
    if (!b || !bytes) return GOL_EINVAL;
    if (!range_ok(b, first, n))
        return bfail(b, GOL_EINVAL, "gol_batch_load: boards %d .. %lld are not in a batch of %d", first,
                     (long long)first + n - 1, b->boards);
    DeviceGuard g(b->device);
    const size_t bw = b->board_words();
    const int per = chunk_boards(b, n);
    if (int rc = ensure_staging(b, (size_t)per * bw * 8)) return rc;
    uint64_t *st = (uint64_t *)b->staging;
    for (int32_t i0 = 0; i0 < n; i0 += per) {
        const int m = std::min<int32_t>(per, n - i0);
        const size_t rows = (size_t)m * b->height;
        std::memset(st, 0, rows * b->nw * 8);
        const uint8_t *src = bytes + (size_t)i0 * b->height * b->width;
        for (size_t r = 0; r < rows; ++r, src += b->width) {
            uint64_t *row = st + r * b->nw;
            for (int x = 0; x < b->width; ++x)
                if (src[x] == 255) row[x >> 6] |= 1ull << (x & 63);
        }
        BATCH_HIP(b, hipMemcpyAsync(b->words + (size_t)(first + i0) * bw, st, rows * b->nw * 8,
                                    hipMemcpyHostToDevice, b->stream));
        BATCH_HIP(b, hipStreamSynchronize(b->stream));      // (the staging area is reused)
    }
    return loaded(b, first, n);
}

int gol_batch_fill_random(gol_batch *b, uint64_t seed)
{
    if (!b) return GOL_EINVAL;
    DeviceGuard g(b->device);
    // one board of width x (boards x height) cells: board i, row y is its row i x height + y
    const int rows = b->boards * b->height;
    BATCH_HIP(b, golk::launch_fill_random(b->words, b->width, b->nw, b->nw, rows, 0, rows, seed,
                                          b->stream));
    BATCH_HIP(b, hipStreamSynchronize(b->stream));
    b->turn = 0;
    b->watching = false;
    return GOL_OK;
}

int gol_batch_step(gol_batch *b, int64_t turns)
{
    if (!b || turns < 0) return GOL_EINVAL;
    b->watching = false;
    DeviceGuard g(b->device);
    // ceil(turns / 256) launches of near-equal depth (plan_launch's split)
    for (int64_t left = turns; left > 0;) {
        const int64_t nl = (left + golk::kResidentMaxTurns - 1) / golk::kResidentMaxTurns;
        const int k = (int)((left + nl - 1) / nl);
        BATCH_HIP(b, golk::launch_resident_batch(b->words, b->counts, b->width, b->height, b->boards,
                                                 b->turn, k, b->stream));
        b->turn += k;
        left -= k;
    }
    return GOL_OK;
}

int gol_batch_read_packed(gol_batch *b, int32_t first, int32_t n, uint64_t *out)
{
    if (!b || !out) return GOL_EINVAL;
    if (!range_ok(b, first, n))
        return bfail(b, GOL_EINVAL, "gol_batch_read_packed: boards %d .. %lld are not in a batch of %d",
                     first, (long long)first + n - 1, b->boards);
    DeviceGuard g(b->device);
    const size_t bw = b->board_words();
    BATCH_HIP(b, hipMemcpyAsync(out, b->words + (size_t)first * bw, (size_t)n * bw * 8,
                                hipMemcpyDeviceToHost, b->stream));
    BATCH_HIP(b, hipStreamSynchronize(b->stream));
    return GOL_OK;
}

int gol_batch_read(gol_batch *b, int32_t first, int32_t n, uint8_t *out)
{
    if (!b || !out) return GOL_EINVAL;
    if (!range_ok(b, first, n))
        return bfail(b, GOL_EINVAL, "gol_batch_read: boards %d .. %lld are not in a batch of %d", first,
                     (long long)first + n - 1, b->boards);
    DeviceGuard g(b->device);
    const size_t bw = b->board_words();
    const int per = chunk_boards(b, n);
    if (int rc = ensure_staging(b, (size_t)per * bw * 8)) return rc;
    const uint64_t *st = (const uint64_t *)b->staging;
    for (int32_t i0 = 0; i0 < n; i0 += per) {
        const int m = std::min<int32_t>(per, n - i0);
        const size_t rows = (size_t)m * b->height;
        BATCH_HIP(b, hipMemcpyAsync(b->staging, b->words + (size_t)(first + i0) * bw, rows * b->nw * 8,
                                    hipMemcpyDeviceToHost, b->stream));
        BATCH_HIP(b, hipStreamSynchronize(b->stream));
        uint8_t *dst = out + (size_t)i0 * b->height * b->width;
        for (size_t r = 0; r < rows; ++r, dst += b->width) {
            const uint64_t *row = st + r * b->nw;
            for (int x = 0; x < b->width; ++x) dst[x] = (row[x >> 6] >> (x & 63)) & 1 ? 255 : 0;
        }
    }
    return GOL_OK;
}

int gol_batch_alive(gol_batch *b, int32_t first, int32_t n, int64_t *out)
{
    if (!b || !out) return GOL_EINVAL;
    if (!range_ok(b, first, n))
        return bfail(b, GOL_EINVAL, "gol_batch_alive: boards %d .. %lld are not in a batch of %d", first,
                     (long long)first + n - 1, b->boards);
    DeviceGuard g(b->device);
    if (!b->alive) BATCH_HIP(b, hipMalloc((void **)&b->alive, (size_t)b->boards * sizeof(uint32_t)));
    if (int rc = ensure_staging(b, (size_t)n * sizeof(uint32_t))) return rc;
    const size_t bw = b->board_words();
    BATCH_HIP(b, golk::launch_batch_alive(b->words + (size_t)first * bw, (int)bw, n, b->alive, b->stream));
    BATCH_HIP(b, hipMemcpyAsync(b->staging, b->alive, (size_t)n * sizeof(uint32_t),
                                hipMemcpyDeviceToHost, b->stream));
    BATCH_HIP(b, hipStreamSynchronize(b->stream));
    const uint32_t *h = (const uint32_t *)b->staging;
    for (int32_t i = 0; i < n; ++i) out[i] = h[i];
    return GOL_OK;
}

int gol_batch_turn_counts(gol_batch *b, int64_t first_turn, int64_t n, int64_t *out)
{
    if (!b || !out || n < 0) return GOL_EINVAL;
    if (!b->counts) return bfail(b, GOL_ESTATE, "batch created without GOL_FLAG_COUNT_EVERY_TURN");
    if (n == 0) return GOL_OK;
    // the ring holds the last 256 stepped turns, and a whole-batch load set the turn to 0
    if (first_turn < 1 || n > golk::kResidentMaxTurns || first_turn + n - 1 > b->turn ||
        first_turn <= b->turn - golk::kResidentMaxTurns)
        return bfail(b, GOL_EINVAL, "turns %lld..%lld not in the recorded window",
                     (long long)first_turn, (long long)(first_turn + n - 1));
    DeviceGuard g(b->device);
    const size_t ring = (size_t)golk::kResidentMaxTurns * b->boards;
    if (int rc = ensure_staging(b, ring * sizeof(uint32_t))) return rc;
    BATCH_HIP(b, hipMemcpyAsync(b->staging, b->counts, ring * sizeof(uint32_t), hipMemcpyDeviceToHost,
                                b->stream));
    BATCH_HIP(b, hipStreamSynchronize(b->stream));
    const uint32_t *h = (const uint32_t *)b->staging;
    for (int64_t i = 0; i < n; ++i) {
        const size_t slot = (size_t)((first_turn + i) % golk::kResidentMaxTurns);
        for (int k = 0; k < b->boards; ++k) out[(size_t)i * b->boards + k] = h[slot * b->boards + k];
    }
    return GOL_OK;
}

// ---------------------------------------------------------------- Settle
int gol_settle_step(gol_batch *b, int64_t turns)
{
    if (!b || turns < 0) return GOL_EINVAL;
    if (b->counts)
        return bfail(b, GOL_ESTATE, "gol_settle_step: the batch records per-turn counts "
                                    "(GOL_FLAG_COUNT_EVERY_TURN); use gol_batch_step");
    DeviceGuard g(b->device);
    if (!b->snaps)
        BATCH_HIP(b, hipMalloc((void **)&b->snaps, (size_t)b->boards * b->board_words() * 8));
    if (!b->states)
        BATCH_HIP(b, hipMalloc((void **)&b->states, (size_t)b->boards * sizeof(golk::SettleState)));
    if (!b->watching) {
        if (int rc = watch_from_here(b, 0, b->boards)) return rc;
        b->watching = true;
    }
    const int depth = settle_depth();
    for (int64_t left = turns; left > 0;) {
        const int k = golk::settle_next_depth(left, depth);
        BATCH_HIP(b, golk::launch_settle_batch(b->words, b->snaps, b->states, b->width, b->height,
                                               b->boards, b->turn, k, b->stream));
        b->turn += k;
        left -= k;
    }
    return GOL_OK;
}

int gol_settle_read(gol_batch *b, int32_t first, int32_t n, int64_t *settled_turn, int64_t *period)
{
    if (!b) return GOL_EINVAL;
    if (!range_ok(b, first, n))
        return bfail(b, GOL_EINVAL, "gol_settle_read: boards %d .. %lld are not in a batch of %d", first,
                     (long long)first + n - 1, b->boards);
    if (!b->watching)
        return bfail(b, GOL_ESTATE, "gol_settle_read: no watch is on (gol_settle_step starts one)");
    DeviceGuard g(b->device);
    if (int rc = ensure_staging(b, (size_t)n * sizeof(golk::SettleState))) return rc;
    BATCH_HIP(b, hipMemcpyAsync(b->staging, b->states + first, (size_t)n * sizeof(golk::SettleState),
                                hipMemcpyDeviceToHost, b->stream));
    BATCH_HIP(b, hipStreamSynchronize(b->stream));
    const golk::SettleState *h = (const golk::SettleState *)b->staging;
    for (int32_t i = 0; i < n; ++i) {
        if (settled_turn) settled_turn[i] = h[i].settled_turn;
        if (period) period[i] = h[i].period;
    }
    return GOL_OK;
}

}  // extern "C"
