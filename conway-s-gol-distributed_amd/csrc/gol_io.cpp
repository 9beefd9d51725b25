// gol_io.cpp — load, read-out, counts, alive and flip lists, windows.
#include <algorithm>
#include <cstring>

#include "gol_ctx.h"
#include "gol_window.h"

using namespace goleng;

namespace {

// byte staging chunk for load / read and the alive list (a test build shrinks it so that small
// boards take several chunks: make smallstage)
#ifndef GOL_STAGING_BYTES
#define GOL_STAGING_BYTES (256u << 20)
#endif
constexpr size_t kStagingBytes = GOL_STAGING_BYTES;
static_assert(kStagingBytes % 16 == 0 && kStagingBytes >= 4096,
              "staging chunks keep k_pack's 16-byte loads aligned and hold a few rows");

int ensure_staging(gol_ctx *c, size_t bytes)
{
    if (c->staging_size >= bytes) return GOL_OK;
    if (c->staging) (void)hipFree(c->staging);
    c->staging = nullptr;
    c->staging_size = 0;
    HIP_OR_FAIL(c, hipMalloc(&c->staging, bytes));
    c->staging_size = bytes;
    return GOL_OK;
}

// popcount of owned rows of the current board -> *alive (synchronous)
int count_now(gol_ctx *c, long long *alive)
{
    unsigned long long *slot = c->counts + (size_t)kRingSlots * kShards;
    HIP_OR_FAIL(c, hipMemsetAsync(slot, 0, kShards * sizeof(unsigned long long), c->stream));
    HIP_OR_FAIL(c, golk::launch_popcount(c->board[c->cur], c->nw, c->pitch, own_lo(c), own_hi(c),
                                         slot, c->stream));
    HIP_OR_FAIL(c, hipMemcpyAsync(c->h_counts, slot, kShards * sizeof(unsigned long long),
                                  hipMemcpyDeviceToHost, c->stream));
    if (int rc = sync_checked(c)) return rc;
    unsigned long long s = 0;
    for (int i = 0; i < kShards; i++) s += c->h_counts[i];
    *alive = (long long)s;
    return GOL_OK;
}

// owned rows as 0/255 bytes (the caller holds the engine: run_read).  (C linkage: the library
// exports this name.)
extern "C" int read_board_bytes(gol_ctx *c, uint8_t *out)
{
    const size_t row_bytes = (size_t)c->cfg.width;
    if (!c->raw_turn0.empty()) {
        std::memcpy(out, c->raw_turn0.data(), c->raw_turn0.size());
        return GOL_OK;
    }
    DeviceGuard g(c->device);
    if (int rc_ = ensure_layout(c, false)) return rc_;
    const int chunk_rows = (int)std::max<size_t>(
        1, std::min<size_t>(kStagingBytes / row_bytes, (size_t)c->cfg.rows));
    int rc = ensure_staging(c, (size_t)chunk_rows * row_bytes);
    if (rc) return rc;
    for (int r0 = 0; r0 < c->cfg.rows; r0 += chunk_rows) {
        const int nr = std::min(chunk_rows, c->cfg.rows - r0);
        HIP_OR_FAIL(c, golk::launch_unpack(c->board[c->cur], c->cfg.width, c->nw, c->pitch,
                                           own_lo(c) + r0, nr, c->staging, c->stream));
        HIP_OR_FAIL(c, hipMemcpyAsync(out + (size_t)r0 * row_bytes, c->staging,
                                      (size_t)nr * row_bytes, hipMemcpyDeviceToHost, c->stream));
        if (int rc2 = sync_checked(c)) return rc2;
    }
    return GOL_OK;
}

// ---- windows (gol_window.h).  The arguments of a window call: in range, and on a strip engine
// (read calls: owned = true) every window row an owned row.
bool window_ok(const gol_ctx *c, int32_t x, int32_t y, int32_t w, int32_t h, bool owned)
{
    if (x < 0 || x >= c->cfg.width || y < 0 || y >= c->cfg.height || w < 1 || w > c->cfg.width ||
        h < 1 || h > c->cfg.height)
        return false;
    if (owned && is_strip(c) &&
        (y < c->cfg.row_offset || (long long)y + h > (long long)c->cfg.row_offset + c->cfg.rows))
        return false;
    return true;
}
// the buffer row of window row 0 of a read call, and the row count its rows wrap at (a torus
// engine's buffer is the board; a strip's window never reaches its buffer's end)
int window_brow0(const gol_ctx *c, int32_t y) { return y - c->cfg.row_offset + own_lo(c); }

}  // namespace

namespace goleng {

void release_blocked(gol_ctx *c)
{
    if (c->blocked) (void)hipFree(c->blocked);
    c->blocked = nullptr;
    c->blocked_pending = false;
}

}  // namespace goleng

// ================================================================ C ABI
extern "C" {

int gol_load(gol_ctx *c, const uint8_t *bytes)
{
    if (!c || !bytes) return GOL_EINVAL;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    DeviceGuard g(c->device);
    const int W = c->cfg.width;
    const size_t row_bytes = (size_t)W;
    int chunk_rows = (int)std::max<size_t>(1, std::min<size_t>(kStagingBytes / row_bytes,
                                                               (size_t)c->buf_rows));
    int rc = ensure_staging(c, (size_t)chunk_rows * row_bytes);
    if (rc) return rc;
    release_blocked(c);
    c->prev_valid = false;                   // (the first chunk may overwrite board[cur ^ 1])
    const size_t words = (size_t)c->buf_rows * c->pitch;
    HIP_OR_FAIL(c, hipMalloc(&c->blocked, words * 8));
    unsigned long long *nb = c->counts + (size_t)kRingSlots * kShards;
    HIP_OR_FAIL(c, hipMemsetAsync(nb, 0, kShards * 8, c->stream));
    uint64_t *dst = c->board[0];
    for (int r0 = 0; r0 < c->buf_rows; r0 += chunk_rows) {
        const int nr = std::min(chunk_rows, c->buf_rows - r0);
        HIP_OR_FAIL(c, hipMemcpyAsync(c->staging, bytes + (size_t)r0 * row_bytes,
                                      (size_t)nr * row_bytes, hipMemcpyHostToDevice, c->stream));
        HIP_OR_FAIL(c, golk::launch_pack(c->staging, W, nr, dst, c->blocked, c->nw, c->pitch, r0,
                                         nb, c->stream));
    }
    HIP_OR_FAIL(c, hipMemcpyAsync(c->h_counts, nb, kShards * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_OR_FAIL(c, hipStreamSynchronize(c->stream));
    unsigned long long s = 0;
    for (int i = 0; i < kShards; i++) s += c->h_counts[i];
    c->nonbinary = (long long)s;
    c->cur = 0;
    c->il = false;
    clear_dev_err(c);                        // a new board: earlier hand-off failures are moot
    c->turn = 0;
    c->progress.store(0);
    c->launches = 0;
    c->halo_valid = c->cfg.halo;
    c->raw_turn0.clear();
    if (s == 0) {
        release_blocked(c);
    } else {
        c->blocked_pending = true;
        // the reference returns the raw bytes unchanged at Turns = 0 (Server loop never runs)
        const size_t own_bytes = (size_t)c->cfg.rows * row_bytes;
        c->raw_turn0.assign(bytes + (size_t)own_lo(c) * row_bytes,
                            bytes + (size_t)own_lo(c) * row_bytes + own_bytes);
    }
    return GOL_OK;
}

int gol_load_packed(gol_ctx *c, const uint64_t *words)
{
    if (!c || !words) return GOL_EINVAL;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    DeviceGuard g(c->device);
    // the bits past `width` in a row's last word must be 0: the stencil shifts them in as the
    // east neighbour of cell width - 1, and the counts and the alive list would include them
    if (const int nb = c->cfg.width & 63) {
        const uint64_t pad = ~0ull << nb;
        for (int r = 0; r < c->buf_rows; ++r)
            if (words[(size_t)r * c->nw + c->nw - 1] & pad)
                return fail(c, GOL_EINVAL,
                            "gol_load_packed: buffer row %d has bits set past width %d in its "
                            "last word (the board is unchanged)", r, c->cfg.width);
    }
    release_blocked(c);
    c->prev_valid = false;
    HIP_OR_FAIL(c, hipMemcpy2DAsync(c->board[0], (size_t)c->pitch * 8, words, (size_t)c->nw * 8,
                                    (size_t)c->nw * 8, c->buf_rows, hipMemcpyHostToDevice,
                                    c->stream));
    HIP_OR_FAIL(c, hipStreamSynchronize(c->stream));
    c->cur = 0;
    c->il = false;
    clear_dev_err(c);                        // a new board: earlier hand-off failures are moot
    c->turn = 0;
    c->progress.store(0);
    c->launches = 0;
    c->nonbinary = 0;
    c->raw_turn0.clear();
    c->halo_valid = c->cfg.halo;
    return GOL_OK;
}

int gol_fill_random(gol_ctx *c, uint64_t seed)
{
    if (!c) return GOL_EINVAL;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    DeviceGuard g(c->device);
    release_blocked(c);
    c->prev_valid = false;
    const long long grow0 = (long long)c->cfg.row_offset - c->cfg.halo;
    HIP_OR_FAIL(c, golk::launch_fill_random(c->board[0], c->cfg.width, c->nw, c->pitch,
                                            c->buf_rows, grow0, c->cfg.height, seed, c->stream));
    HIP_OR_FAIL(c, hipStreamSynchronize(c->stream));
    c->cur = 0;
    c->il = false;
    clear_dev_err(c);                        // a new board: earlier hand-off failures are moot
    c->turn = 0;
    c->progress.store(0);
    c->launches = 0;
    c->nonbinary = 0;
    c->raw_turn0.clear();
    c->halo_valid = c->cfg.halo;
    return GOL_OK;
}

int gol_snapshot(gol_ctx *c, int64_t *turn, int64_t *alive)
{
    if (!c || !turn || !alive) return GOL_EINVAL;
    return run_read(c, [&]() -> int {
        DeviceGuard g(c->device);
        long long n = 0;
        int rc = count_now(c, &n);
        if (rc) return rc;
        *turn = c->turn;
        *alive = n;
        return GOL_OK;
    });
}

int gol_turn_counts(gol_ctx *c, int64_t first_turn, int64_t n, int64_t *out)
{
    if (!c || !out || n < 0) return GOL_EINVAL;
    return run_read(c, [&]() -> int {
        if (!(c->cfg.flags & GOL_FLAG_COUNT_EVERY_TURN))
            return fail(c, GOL_ESTATE, "engine created without GOL_FLAG_COUNT_EVERY_TURN");
        if (n == 0) return GOL_OK;
        if (first_turn < 1 || first_turn + n - 1 > c->turn || first_turn <= c->turn - kRing)
            return fail(c, GOL_EINVAL, "turns %lld..%lld not in the recorded window",
                        (long long)first_turn, (long long)(first_turn + n - 1));
        DeviceGuard g(c->device);
        std::vector<unsigned long long> h((size_t)kRingSlots * kShards);
        HIP_OR_FAIL(c, hipMemcpyAsync(h.data(), c->counts, h.size() * 8, hipMemcpyDeviceToHost,
                                      c->stream));
        if (int rc = sync_checked(c)) return rc;
        for (int64_t i = 0; i < n; ++i) {
            const size_t slot = (size_t)((first_turn + i) % kRingSlots);
            unsigned long long s = 0;
            for (int k = 0; k < kShards; k++) s += h[slot * kShards + k];
            out[i] = (int64_t)s;
        }
        return GOL_OK;
    });
}

int gol_read_board(gol_ctx *c, uint8_t *out)
{
    if (!c || !out) return GOL_EINVAL;
    return run_read(c, [&]() -> int { return read_board_bytes(c, out); });
}

int gol_get_world(gol_ctx *c, uint8_t *out, int64_t *turn)
{
    if (!c || !out || !turn) return GOL_EINVAL;
    return run_read(c, [&]() -> int {
        const int rc = read_board_bytes(c, out);
        if (rc == GOL_OK) *turn = c->turn;
        return rc;
    });
}

int gol_read_packed(gol_ctx *c, uint64_t *out)
{
    if (!c || !out) return GOL_EINVAL;
    return run_read(c, [&]() -> int {
        DeviceGuard g(c->device);
        if (int rc_ = ensure_layout(c, false)) return rc_;
        HIP_OR_FAIL(c, hipMemcpy2DAsync(out, (size_t)c->nw * 8,
                                        c->board[c->cur] + (size_t)own_lo(c) * c->pitch,
                                        (size_t)c->pitch * 8, (size_t)c->nw * 8, c->cfg.rows,
                                        hipMemcpyDeviceToHost, c->stream));
        return sync_checked(c);
    });
}

int gol_alive_cells(gol_ctx *c, int64_t *xy, int64_t cap, int64_t *n)
{
    if (!c || !n || cap < 0 || (cap > 0 && !xy)) return GOL_EINVAL;
    return run_read(c, [&]() -> int {
        DeviceGuard g(c->device);
        if (int rc_ = ensure_layout(c, false)) return rc_;
        const int rows = c->cfg.rows;
        std::vector<long long> rc((size_t)rows), off((size_t)rows);
        long long *d_rc = nullptr;
        HIP_OR_FAIL(c, hipMalloc((void **)&d_rc, (size_t)rows * 8 * 2));
        long long *d_off = d_rc + rows;
        int err = GOL_OK;
        auto done = [&](int code) {
            (void)hipStreamSynchronize(c->stream);
            (void)hipFree(d_rc);
            return code;
        };
        hipError_t e = golk::launch_row_popcount(c->board[c->cur], c->nw, c->pitch, own_lo(c), rows,
                                                 d_rc, c->stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(rc.data(), d_rc, (size_t)rows * 8, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) return done(fail(c, GOL_EHIP, "alive count: %s", hipGetErrorString(e)));
        if (int rc2 = check_dev_err(c)) return done(rc2);
        long long total = 0;
        for (int r = 0; r < rows; r++) {
            off[(size_t)r] = total;
            total += rc[(size_t)r];
        }
        *n = total;
        if (cap == 0 || total == 0) return done(GOL_OK);
        // scatter in row chunks so the device list stays within the staging budget
        const long long per_cell = 16;
        long long r0 = 0;
        while (r0 < rows && off[(size_t)r0] < cap) {
            // rows [r0, r1) whose cells fit in kStagingBytes
            long long r1 = r0;
            while (r1 < rows && (off[(size_t)r1] + rc[(size_t)r1] - off[(size_t)r0]) * per_cell <=
                                    (long long)kStagingBytes)
                ++r1;
            if (r1 == r0) r1 = r0 + 1;  // a single row larger than the budget
            const long long cells = off[(size_t)r1 - 1] + rc[(size_t)r1 - 1] - off[(size_t)r0];
            err = ensure_staging(c, (size_t)std::max<long long>(cells * per_cell, 16));
            if (err) return done(err);
            // offsets relative to this chunk: subtract off[r0] via a shifted copy
            std::vector<long long> rel((size_t)(r1 - r0));
            for (long long r = r0; r < r1; r++) rel[(size_t)(r - r0)] = off[(size_t)r] - off[(size_t)r0];
            e = hipMemcpyAsync(d_off + r0, rel.data(), rel.size() * 8, hipMemcpyHostToDevice,
                               c->stream);
            if (e == hipSuccess)
                e = golk::launch_alive_scatter(c->board[c->cur], c->nw, c->pitch,
                                               own_lo(c) + (int)r0, (int)(r1 - r0),
                                               (long long)c->cfg.row_offset + r0, d_off + r0,
                                               (long long *)c->staging, c->stream);
            const long long want = std::min<long long>(cells, cap - off[(size_t)r0]);
            if (e == hipSuccess)
                e = hipMemcpyAsync(xy + 2 * off[(size_t)r0], c->staging, (size_t)want * per_cell,
                                   hipMemcpyDeviceToHost, c->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
            if (e != hipSuccess)
                return done(fail(c, GOL_EHIP, "alive scatter: %s", hipGetErrorString(e)));
            r0 = r1;
        }
        return done(GOL_OK);
    });
}

int gol_flipped_cells(gol_ctx *c, int64_t *xy, int64_t cap, int64_t *n)
{
    if (!c || !n || cap < 0 || (cap > 0 && !xy)) return GOL_EINVAL;
    return run_read(c, [&]() -> int {
        if (!c->prev_valid || c->il)
            return fail(c, GOL_ESTATE,
                        "gol_flipped_cells: the previous board is not held (valid after a "
                        "one-turn gol_step, until the next load, longer step or layout change)");
        DeviceGuard g(c->device);
        const int rows = c->cfg.rows;
        if (!c->flip_rows) {                 // scratch for the engine's lifetime
            HIP_OR_FAIL(c, hipMalloc((void **)&c->flip_rows, ((size_t)rows * 2 + 1) * 8));
            HIP_OR_FAIL(c, hipHostMalloc((void **)&c->h_flip_total, 8, hipHostMallocDefault));
        }
        long long *d_rc = c->flip_rows, *d_off = c->flip_rows + rows;
        const uint64_t *cur = c->board[c->cur], *prev = c->board[c->cur ^ 1];
        const long long per_cell = 16;
        HIP_OR_FAIL(c, golk::launch_flip_offsets(cur, prev, c->nw, c->pitch, own_lo(c), rows, d_rc,
                                                 d_off, c->stream));
        HIP_OR_FAIL(c, hipMemcpyAsync(c->h_flip_total, d_off + rows, 8, hipMemcpyDeviceToHost,
                                      c->stream));
        if (int rc = sync_checked(c)) return rc;
        const long long total = *c->h_flip_total;
        *n = total;
        if (cap == 0 || total == 0) return GOL_OK;
        if (total * per_cell <= (long long)kStagingBytes) {
            // the common case: one scatter, and the host reads nothing but the list.  The
            // staging buffer grows by doubling, so a run's lists soon stop reallocating it.
            if (c->staging_size < (size_t)(total * per_cell))
                if (int rc = ensure_staging(c, std::min<size_t>(kStagingBytes,
                                                                (size_t)(total * per_cell) * 2)))
                    return rc;
            HIP_OR_FAIL(c, golk::launch_flip_scatter(cur, prev, c->nw, c->pitch, own_lo(c), rows,
                                                     (long long)c->cfg.row_offset, d_off, 0,
                                                     (long long *)c->staging, c->stream));
            HIP_OR_FAIL(c, hipMemcpyAsync(xy, c->staging,
                                          (size_t)std::min<long long>(total, cap) * per_cell,
                                          hipMemcpyDeviceToHost, c->stream));
            return sync_checked(c);
        }
        // a list larger than the staging budget: row chunks, as gol_alive_cells (the row counts
        // come to the host to cut the chunks; the device offsets are rebased per chunk)
        std::vector<long long> rc((size_t)rows), off((size_t)rows);
        HIP_OR_FAIL(c, hipMemcpyAsync(rc.data(), d_rc, (size_t)rows * 8, hipMemcpyDeviceToHost,
                                      c->stream));
        if (int rc2 = sync_checked(c)) return rc2;
        long long sum = 0;
        for (int r = 0; r < rows; r++) {
            off[(size_t)r] = sum;
            sum += rc[(size_t)r];
        }
        long long r0 = 0;
        while (r0 < rows && off[(size_t)r0] < cap) {
            long long r1 = r0;
            while (r1 < rows && (off[(size_t)r1] + rc[(size_t)r1] - off[(size_t)r0]) * per_cell <=
                                    (long long)kStagingBytes)
                ++r1;
            if (r1 == r0) r1 = r0 + 1;  // a single row larger than the budget
            const long long cells = off[(size_t)r1 - 1] + rc[(size_t)r1 - 1] - off[(size_t)r0];
            if (int rc2 = ensure_staging(c, (size_t)std::max<long long>(cells * per_cell, 16)))
                return rc2;
            HIP_OR_FAIL(c, golk::launch_flip_scatter(cur, prev, c->nw, c->pitch,
                                                     own_lo(c) + (int)r0, (int)(r1 - r0),
                                                     (long long)c->cfg.row_offset + r0, d_off + r0,
                                                     off[(size_t)r0], (long long *)c->staging,
                                                     c->stream));
            const long long want = std::min<long long>(cells, cap - off[(size_t)r0]);
            if (want > 0)
                HIP_OR_FAIL(c, hipMemcpyAsync(xy + 2 * off[(size_t)r0], c->staging,
                                              (size_t)want * per_cell, hipMemcpyDeviceToHost,
                                              c->stream));
            if (int rc2 = sync_checked(c)) return rc2;
            r0 = r1;
        }
        return GOL_OK;
    });
}

// ---------------------------------------------------------------- windows
int gol_read_window(gol_ctx *c, int32_t x, int32_t y, int32_t w, int32_t h, uint8_t *out,
                    int64_t *turn)
{
    if (!c || !out) return GOL_EINVAL;
    return run_read(c, [&]() -> int {
        if (!window_ok(c, x, y, w, h, true)) return GOL_EINVAL;
        if (turn) *turn = c->turn;
        if (!c->raw_turn0.empty()) {         // the loaded bytes as they are (gol_read_board)
            const int W = c->cfg.width, rows = c->cfg.rows;
            for (int j = 0; j < h; ++j) {
                const uint8_t *src =
                    c->raw_turn0.data() + (size_t)((y - c->cfg.row_offset + j) % rows) * W;
                uint8_t *dst = out + (size_t)j * w;
                const int n = std::min(w, W - x);
                std::memcpy(dst, src + x, (size_t)n);
                if (n < w) std::memcpy(dst + n, src, (size_t)(w - n));
            }
            return GOL_OK;
        }
        DeviceGuard g(c->device);
        const size_t row_bytes = (size_t)w;
        const int chunk_rows =
            (int)std::max<size_t>(1, std::min<size_t>(kStagingBytes / row_bytes, (size_t)h));
        if (int rc = ensure_staging(c, (size_t)chunk_rows * row_bytes)) return rc;
        for (int r0 = 0; r0 < h; r0 += chunk_rows) {
            const int nr = std::min(chunk_rows, h - r0);
            HIP_OR_FAIL(c, golk::launch_window_unpack(c->board[c->cur], c->cfg.width, c->pitch,
                                                      c->il, c->buf_rows, window_brow0(c, y), x, w,
                                                      r0, nr, c->staging, c->stream));
            HIP_OR_FAIL(c, hipMemcpyAsync(out + (size_t)r0 * row_bytes, c->staging,
                                          (size_t)nr * row_bytes, hipMemcpyDeviceToHost, c->stream));
            if (int rc = sync_checked(c)) return rc;
        }
        return GOL_OK;
    });
}

int gol_window_density(gol_ctx *c, int32_t x, int32_t y, int32_t w, int32_t h, int32_t block,
                       uint32_t *out, int64_t *turn)
{
    if (!c || !out || block < 1 || block > 4096) return GOL_EINVAL;
    return run_read(c, [&]() -> int {
        if (!window_ok(c, x, y, w, h, true)) return GOL_EINVAL;
        if (turn) *turn = c->turn;
        DeviceGuard g(c->device);
        // whole block rows per staging chunk (one, however long, when a single one exceeds it)
        const int nbx = (w + block - 1) / block, nby = (h + block - 1) / block;
        const size_t brow_bytes = (size_t)nbx * sizeof(uint32_t);
        const int chunk_brows =
            (int)std::max<size_t>(1, std::min<size_t>(kStagingBytes / brow_bytes, (size_t)nby));
        if (int rc = ensure_staging(c, std::max<size_t>((size_t)chunk_brows * brow_bytes, 16)))
            return rc;
        for (int J0 = 0; J0 < nby; J0 += chunk_brows) {
            const int nJ = std::min(chunk_brows, nby - J0);
            const int r0 = J0 * block;                   // (< h <= 2^31 - 1)
            const int nr = (int)std::min<long long>((long long)nJ * block, (long long)h - r0);
            HIP_OR_FAIL(c, hipMemsetAsync(c->staging, 0, (size_t)nJ * brow_bytes, c->stream));
            HIP_OR_FAIL(c, golk::launch_window_density(c->board[c->cur], c->cfg.width, c->pitch,
                                                       c->il, c->buf_rows, window_brow0(c, y), x, w,
                                                       r0, nr, block, (uint32_t *)c->staging,
                                                       c->stream));
            HIP_OR_FAIL(c, hipMemcpyAsync(out + (size_t)J0 * nbx, c->staging, (size_t)nJ * brow_bytes,
                                          hipMemcpyDeviceToHost, c->stream));
            if (int rc = sync_checked(c)) return rc;
        }
        return GOL_OK;
    });
}

int gol_write_window(gol_ctx *c, int32_t x, int32_t y, int32_t w, int32_t h, const uint8_t *bytes)
{
    if (!c || !bytes) return GOL_EINVAL;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    if (!window_ok(c, x, y, w, h, false)) return GOL_EINVAL;
    if (!c->raw_turn0.empty() || c->blocked_pending)
        return fail(c, GOL_ESTATE, "gol_write_window: the engine holds a non-binary turn-0 board "
                                   "(a window has no non-binary semantics)");
    DeviceGuard g(c->device);
    const size_t row_bytes = (size_t)w;
    const int chunk_rows =
        (int)std::max<size_t>(1, std::min<size_t>(kStagingBytes / row_bytes, (size_t)h));
    if (int rc = ensure_staging(c, (size_t)chunk_rows * row_bytes)) return rc;
    c->prev_valid = false;
    // Buffer row b holds global row (g0 + b) mod height; it lies in the window when
    // (g0 + b - y) mod height < h, i.e. b = s + t + m x height with s = (y - g0) mod height and t
    // the window row: one run of h buffer rows per m, cut to the buffer.  A torus engine's runs
    // are the window's rows up to the board's end (m = 0) and past the wrap (m = -1); a strip's
    // buffer may hold a global row twice (rows == height with halos), then both copies are
    // written; it may hold none of the window's, and nothing is.
    const long long H = c->cfg.height;
    const long long g0 = (long long)c->cfg.row_offset - c->cfg.halo;
    const long long s = (((long long)y - g0) % H + H) % H;
    for (int r0 = 0; r0 < h; r0 += chunk_rows) {
        const int nr = std::min(chunk_rows, h - r0);
        bool staged = false;
        for (long long first = s - H; first < c->buf_rows; first += H) {
            // window rows [r0, r0 + nr) of this run are buffer rows first + r0 ...
            const long long lo = std::max<long long>(0, first + r0);
            const long long hi = std::min<long long>(c->buf_rows, first + r0 + nr);
            if (lo >= hi) continue;
            if (!staged) {
                HIP_OR_FAIL(c, hipMemcpyAsync(c->staging, bytes + (size_t)r0 * row_bytes,
                                              (size_t)nr * row_bytes, hipMemcpyHostToDevice,
                                              c->stream));
                staged = true;
            }
            HIP_OR_FAIL(c, golk::launch_window_pack(
                               c->board[c->cur], c->cfg.width, c->nw, c->pitch, c->il, (int)lo,
                               (int)(hi - lo), x, w,
                               c->staging + (size_t)(lo - first - r0) * row_bytes, c->stream));
        }
    }
    return sync_checked(c);
}

int gol_clear(gol_ctx *c)
{
    if (!c) return GOL_EINVAL;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    DeviceGuard g(c->device);
    release_blocked(c);
    c->prev_valid = false;
    HIP_OR_FAIL(c, hipMemsetAsync(c->board[0], 0, (size_t)c->buf_rows * c->pitch * 8, c->stream));
    HIP_OR_FAIL(c, hipStreamSynchronize(c->stream));
    c->cur = 0;
    c->il = false;
    clear_dev_err(c);                        // a new board: earlier hand-off failures are moot
    c->turn = 0;
    c->progress.store(0);
    c->launches = 0;
    c->nonbinary = 0;
    c->raw_turn0.clear();
    c->halo_valid = c->cfg.halo;
    return GOL_OK;
}

int gol_board_layout(gol_ctx *c)
{
    if (!c) return GOL_EINVAL;
    return run_read(c, [&]() -> int { return c->il ? 1 : 0; });
}

int gol_window_word(const uint64_t *row, int32_t width, int32_t col, int32_t layout, uint64_t *out)
{
    if (!row || !out || width < 2 || col < 0 || col >= width || (layout != 0 && layout != 1))
        return GOL_EINVAL;
    *out = golk::window_word(row, width, col, layout == 1);
    return GOL_OK;
}

}  // extern "C"
