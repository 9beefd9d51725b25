// gol_model_engine.cpp -- a CPU model of the engine calls and the HIP runtime calls that
// csrc/gol_run.cpp leaves undefined, so the unmodified run driver links into a host-only
// program (tests/harness/gol_run_hostcheck.cpp) and runs under ThreadSanitizer,
// AddressSanitizer and UBSan without a GPU (csrc/Makefile `hostcheck`,
// tests/test_run_host_cpu.py).  Test infrastructure only: it stands for the CONTRACT of
// include/gol_amd.h at the driver's boundary, not for the engine (no kernels, no streams, no
// cross-thread read service; DESIGN.md "Host driver under sanitizers").
//
// Board model: one byte per cell, plain loops.  A torus engine holds height x width bytes; a
// strip engine holds (rows + 2 * halo) x width bytes = global rows row_offset - halo ..
// row_offset + rows + halo - 1 (mod height).  One turn follows the reference rule on bytes: a
// cell is alive iff its byte is 255; a 255 cell with 2 or 3 alive neighbours and a 0 cell with 3
// stay / become 255; every other cell -- a byte that is neither 0 nor 255 included -- becomes 0.
// So a non-binary cell has packed bit 0, is never alive after its first turn, and
// gol_read_board at turn 0 returns the bytes as they were loaded.  A strip steps all of its
// buffer rows with dead rows beyond the buffer, so the outermost valid halo row goes stale every
// turn: halo_valid starts at halo, drops by one per turn, gol_step beyond it is GOL_ESTATE, and
// gol_halo_done resets it after the halo copies.
//
// Control word: gol_step reads it before every turn (after the GOL_MODEL_TURN_US sleep, so a
// key pressed during the sleep stops the step before that turn): STOP returns GOL_STOPPED,
// PAUSE waits for the word to change.  It is the only engine state another thread may touch.
//
// HIP shim: everything is synchronous; an event is a heap object (a leaked or twice-destroyed
// event is an ASan / LSan report); hipHostMalloc is malloc.
//
// Environment:
//   GOL_MODEL_DEVICES=<n>      hipGetDeviceCount (default 2)
//   GOL_MODEL_TURN_US=<us>     sleep per turn, so keys and ticks land mid-run
//   GOL_MODEL_FAIL=<call>:<n>  the n-th call of that name fails with its natural error
//                              (<n>+ : the n-th and every later one).  Engine calls return
//                              GOL_EHIP and set gol_last_error ("model: injected failure of
//                              <call>"); gol_create_ex returns GOL_EHIP and no engine; shim calls
//                              return a HIP error.  Injectable calls:
//     gol_create_ex gol_load gol_load_packed gol_read_packed gol_read_board gol_step gol_sync
//     gol_snapshot gol_alive_cells gol_flipped_cells gol_copy_halo_from_upper
//     gol_copy_halo_from_lower
//     hipGetDeviceCount hipDeviceCanAccessPeer hipDeviceEnablePeerAccess hipHostMalloc
//     hipEventCreateWithFlags hipEventRecord hipEventSynchronize
#include <hip/hip_runtime_api.h>

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "gol_amd.h"
#include "gol_internal.h"

namespace {

// ------------------------------------------------------------- failure injection
struct Inject {
    std::mutex mu;
    bool parsed = false;
    std::string call;
    long nth = 0;
    bool onward = false;
    long seen = 0;
};

bool inject(const char *name)
{
    static Inject in;
    std::lock_guard<std::mutex> lk(in.mu);
    if (!in.parsed) {
        in.parsed = true;
        if (const char *e = getenv("GOL_MODEL_FAIL")) {
            const std::string s(e);
            const size_t colon = s.find(':');
            if (colon != std::string::npos) {
                in.call = s.substr(0, colon);
                in.nth = atol(s.c_str() + colon + 1);
                in.onward = !s.empty() && s.back() == '+';
            }
        }
    }
    if (in.call != name) return false;
    in.seen++;
    return in.onward ? in.seen >= in.nth : in.seen == in.nth;
}

int env_int(const char *name, int dflt)
{
    const char *e = getenv(name);
    return e && *e ? atoi(e) : dflt;
}

thread_local int t_device = 0;

}  // namespace

// ------------------------------------------------------------------- engine
struct gol_ctx {
    gol_config cfg{};
    int buf_rows = 0, nw = 0;
    bool torus = true;
    std::vector<uint8_t> cur, prev;       // buf_rows x width bytes
    bool prev_valid = false;
    long long turn = 0;
    long long nonbinary = 0;
    int halo_valid = 0;
    int turn_us = 0;
    std::atomic<int32_t> control{GOL_CONTROL_RUN};
    std::string err;

    int own_lo() const { return torus ? 0 : cfg.halo; }
    int fail(const char *call)
    {
        err = std::string("model: injected failure of ") + call;
        return GOL_EHIP;
    }
    bool alive(const std::vector<uint8_t> &b, int r, int x) const
    {
        const int W = cfg.width;
        x = (x + W) % W;
        if (torus) r = (r + buf_rows) % buf_rows;
        else if (r < 0 || r >= buf_rows) return false;
        return b[(size_t)r * W + x] == 255;
    }
    void one_turn()
    {
        const int W = cfg.width;
        prev.swap(cur);
        cur.assign(prev.size(), 0);
        for (int r = 0; r < buf_rows; r++)
            for (int x = 0; x < W; x++) {
                int n = 0;
                for (int dy = -1; dy <= 1; dy++)
                    for (int dx = -1; dx <= 1; dx++)
                        if ((dy || dx) && alive(prev, r + dy, x + dx)) n++;
                const uint8_t c = prev[(size_t)r * W + x];
                if ((c == 255 && (n == 2 || n == 3)) || (c == 0 && n == 3))
                    cur[(size_t)r * W + x] = 255;
            }
    }
};

#define INJECT_ENGINE(c, call) \
    do {                       \
        if (inject(call)) return (c)->fail(call); \
    } while (0)

namespace golint {
long long engine_turn(gol_ctx *c) { return c ? c->turn : 0; }
int engine_device(gol_ctx *c) { return c ? c->cfg.device : -1; }
}  // namespace golint

extern "C" {

const char *gol_strerror(int code)
{
    switch (code) {
    case GOL_OK: return "ok";
    case GOL_EINVAL: return "invalid argument";
    case GOL_EHIP: return "HIP runtime error";
    case GOL_ENOMEM: return "out of memory";
    case GOL_ESTATE: return "call not valid in this state";
    case GOL_ENODEV: return "no usable HIP device";
    case GOL_EIO: return "PGM file missing or malformed";
    case GOL_ECLOSED: return "event channel closed";
    case GOL_ETIMEDOUT: return "timed out";
    case GOL_STOPPED: return "stopped";
    }
    return "unknown error";
}

int gol_create_ex(const gol_config *cfg, gol_ctx **out)
{
    if (!cfg || !out) return GOL_EINVAL;
    *out = nullptr;
    if (cfg->width < 2 || cfg->height < 1 || cfg->rows < 1 || cfg->rows > cfg->height ||
        cfg->row_offset < 0 || cfg->row_offset + cfg->rows > cfg->height || cfg->halo < 0)
        return GOL_EINVAL;
    const bool torus = cfg->rows == cfg->height && cfg->halo == 0;
    if (!torus && (cfg->halo < 1 || cfg->halo > cfg->rows)) return GOL_EINVAL;
    int ndev = env_int("GOL_MODEL_DEVICES", 2);
    if (cfg->device >= ndev || cfg->device < -1) return GOL_ENODEV;
    if (inject("gol_create_ex")) return GOL_EHIP;
    gol_ctx *c = new gol_ctx();
    c->cfg = *cfg;
    if (c->cfg.device < 0) c->cfg.device = t_device;
    c->torus = torus;
    c->buf_rows = cfg->rows + 2 * cfg->halo;
    c->nw = (cfg->width + 63) / 64;
    c->cur.assign((size_t)c->buf_rows * cfg->width, 0);
    c->prev = c->cur;
    c->halo_valid = cfg->halo;
    c->turn_us = env_int("GOL_MODEL_TURN_US", 0);
    *out = c;
    return GOL_OK;
}

void gol_destroy(gol_ctx *c) { delete c; }

const char *gol_last_error(const gol_ctx *c) { return c ? c->err.c_str() : ""; }

int gol_get_info(gol_ctx *c, gol_info *info)
{
    if (!c || !info) return GOL_EINVAL;
    std::memset(info, 0, sizeof *info);
    info->width = c->cfg.width;
    info->height = c->cfg.height;
    info->row_offset = c->cfg.row_offset;
    info->rows = c->cfg.rows;
    info->halo = c->cfg.halo;
    info->words_per_row = c->nw;
    info->pitch_words = c->nw;
    info->buffer_rows = c->buf_rows;
    info->band_rows = 1;
    info->halo_valid = c->halo_valid;
    info->turns_per_launch = 1;
    info->device = c->cfg.device;
    info->turn = c->turn;
    info->nonbinary_cells = c->nonbinary;
    info->launches = c->turn;
    return GOL_OK;
}

int gol_load(gol_ctx *c, const uint8_t *bytes)
{
    if (!c || !bytes) return GOL_EINVAL;
    INJECT_ENGINE(c, "gol_load");
    std::memcpy(c->cur.data(), bytes, c->cur.size());
    c->nonbinary = 0;
    for (uint8_t b : c->cur) c->nonbinary += b != 0 && b != 255;
    c->prev_valid = false;
    c->turn = 0;
    c->halo_valid = c->cfg.halo;
    return GOL_OK;
}

int gol_load_packed(gol_ctx *c, const uint64_t *words)
{
    if (!c || !words) return GOL_EINVAL;
    INJECT_ENGINE(c, "gol_load_packed");
    const int W = c->cfg.width;
    if (const int nb = W & 63) {
        const uint64_t pad = ~0ull << nb;
        for (int r = 0; r < c->buf_rows; r++)
            if (words[(size_t)r * c->nw + c->nw - 1] & pad) {
                c->err = "gol_load_packed: bits set past the width";
                return GOL_EINVAL;
            }
    }
    for (int r = 0; r < c->buf_rows; r++)
        for (int x = 0; x < W; x++)
            c->cur[(size_t)r * W + x] =
                (words[(size_t)r * c->nw + x / 64] >> (x % 64)) & 1 ? 255 : 0;
    c->nonbinary = 0;
    c->prev_valid = false;
    c->turn = 0;
    c->halo_valid = c->cfg.halo;
    return GOL_OK;
}

int gol_read_packed(gol_ctx *c, uint64_t *out)
{
    if (!c || !out) return GOL_EINVAL;
    INJECT_ENGINE(c, "gol_read_packed");
    const int W = c->cfg.width;
    std::memset(out, 0, (size_t)c->cfg.rows * c->nw * 8);
    for (int r = 0; r < c->cfg.rows; r++)
        for (int x = 0; x < W; x++)
            if (c->cur[(size_t)(c->own_lo() + r) * W + x] == 255)
                out[(size_t)r * c->nw + x / 64] |= 1ull << (x % 64);
    return GOL_OK;
}

int gol_read_board(gol_ctx *c, uint8_t *out)
{
    if (!c || !out) return GOL_EINVAL;
    INJECT_ENGINE(c, "gol_read_board");
    const size_t W = (size_t)c->cfg.width;
    std::memcpy(out, c->cur.data() + (size_t)c->own_lo() * W, (size_t)c->cfg.rows * W);
    return GOL_OK;
}

int gol_set_control(gol_ctx *c, int32_t word)
{
    if (!c || word < GOL_CONTROL_RUN || word > GOL_CONTROL_STOP) return GOL_EINVAL;
    c->control.store(word);
    return GOL_OK;
}

int gol_step(gol_ctx *c, int64_t turns)
{
    if (!c || turns < 0) return GOL_EINVAL;
    INJECT_ENGINE(c, "gol_step");
    if (!c->torus && turns > c->halo_valid) {
        c->err = "gol_step: more turns than the halo allows";
        return GOL_ESTATE;
    }
    for (int64_t t = 0; t < turns; t++) {
        if (c->turn_us > 0) std::this_thread::sleep_for(std::chrono::microseconds(c->turn_us));
        int32_t w;
        while ((w = c->control.load()) == GOL_CONTROL_PAUSE)
            std::this_thread::sleep_for(std::chrono::microseconds(200));
        if (w == GOL_CONTROL_STOP) return GOL_STOPPED;
        c->one_turn();
        c->turn++;
        if (!c->torus) c->halo_valid--;
        c->prev_valid = turns == 1;
    }
    return GOL_OK;
}

int gol_sync(gol_ctx *c)
{
    if (!c) return GOL_EINVAL;
    INJECT_ENGINE(c, "gol_sync");
    return GOL_OK;
}

// a distinct non-null stream per engine, never dereferenced
void *gol_get_stream(gol_ctx *c) { return c; }

int gol_snapshot(gol_ctx *c, int64_t *turn, int64_t *alive)
{
    if (!c || !turn || !alive) return GOL_EINVAL;
    INJECT_ENGINE(c, "gol_snapshot");
    const size_t W = (size_t)c->cfg.width;
    int64_t n = 0;
    for (size_t i = (size_t)c->own_lo() * W; i < (size_t)(c->own_lo() + c->cfg.rows) * W; i++)
        n += c->cur[i] == 255;
    *turn = c->turn;
    *alive = n;
    return GOL_OK;
}

static int list_cells(gol_ctx *c, bool flips, int64_t *xy, int64_t cap, int64_t *n)
{
    const int W = c->cfg.width;
    int64_t k = 0;
    for (int r = 0; r < c->cfg.rows; r++)
        for (int x = 0; x < W; x++) {
            const size_t i = (size_t)(c->own_lo() + r) * W + x;
            const bool now = c->cur[i] == 255;
            if (flips ? now != (c->prev[i] == 255) : now) {
                if (xy && k < cap) {
                    xy[2 * k] = x;
                    xy[2 * k + 1] = c->cfg.row_offset + r;
                }
                k++;
            }
        }
    *n = k;
    return GOL_OK;
}

int gol_alive_cells(gol_ctx *c, int64_t *xy, int64_t cap, int64_t *n)
{
    if (!c || !n || cap < 0 || (cap > 0 && !xy)) return GOL_EINVAL;
    INJECT_ENGINE(c, "gol_alive_cells");
    return list_cells(c, false, xy, cap, n);
}

int gol_flipped_cells(gol_ctx *c, int64_t *xy, int64_t cap, int64_t *n)
{
    if (!c || !n || cap < 0 || (cap > 0 && !xy)) return GOL_EINVAL;
    INJECT_ENGINE(c, "gol_flipped_cells");
    if (!c->prev_valid) {
        c->err = "gol_flipped_cells: the last step was not one turn";
        return GOL_ESTATE;
    }
    return list_cells(c, true, xy, cap, n);
}

static int copy_halo(gol_ctx *dst, gol_ctx *src, bool upper)
{
    if (!dst || !src || dst->torus || src->torus || dst->cfg.width != src->cfg.width ||
        dst->cfg.halo != src->cfg.halo)
        return GOL_EINVAL;
    const size_t W = (size_t)dst->cfg.width, K = (size_t)dst->cfg.halo;
    // only halo rows of the current board change: the flip list (owned rows) stays valid
    const size_t from = upper ? (size_t)src->cfg.rows : K;     // src's last / first K owned rows
    const size_t to = upper ? 0 : K + (size_t)dst->cfg.rows;
    std::memcpy(dst->cur.data() + to * W, src->cur.data() + from * W, K * W);
    return GOL_OK;
}

int gol_copy_halo_from_upper(gol_ctx *dst, gol_ctx *src)
{
    if (dst) INJECT_ENGINE(dst, "gol_copy_halo_from_upper");
    return copy_halo(dst, src, true);
}

int gol_copy_halo_from_lower(gol_ctx *dst, gol_ctx *src)
{
    if (dst) INJECT_ENGINE(dst, "gol_copy_halo_from_lower");
    return copy_halo(dst, src, false);
}

int gol_halo_done(gol_ctx *c)
{
    if (!c || c->torus) return GOL_EINVAL;
    c->halo_valid = c->cfg.halo;
    return GOL_OK;
}

// ------------------------------------------------------------------ HIP shim
struct ihipEvent_t {
    uint32_t magic;
    bool recorded;
};
static const uint32_t kEventMagic = 0x45564e54u;

hipError_t hipGetDeviceCount(int *count)
{
    if (!count) return hipErrorInvalidValue;
    if (inject("hipGetDeviceCount")) return hipErrorNoDevice;
    *count = env_int("GOL_MODEL_DEVICES", 2);
    return hipSuccess;
}

hipError_t hipGetDevice(int *device)
{
    if (!device) return hipErrorInvalidValue;
    *device = t_device;
    return hipSuccess;
}

hipError_t hipSetDevice(int device)
{
    if (device < 0 || device >= env_int("GOL_MODEL_DEVICES", 2)) return hipErrorInvalidDevice;
    t_device = device;
    return hipSuccess;
}

hipError_t hipDeviceCanAccessPeer(int *can, int device, int peer)
{
    if (!can) return hipErrorInvalidValue;
    if (inject("hipDeviceCanAccessPeer")) return hipErrorInvalidDevice;
    *can = device != peer;
    return hipSuccess;
}

hipError_t hipDeviceEnablePeerAccess(int peer, unsigned int flags)
{
    if (inject("hipDeviceEnablePeerAccess")) return hipErrorInvalidDevice;
    return peer == t_device ? hipErrorInvalidDevice : hipSuccess;
}

hipError_t hipGetLastError(void) { return hipSuccess; }

const char *hipGetErrorName(hipError_t e)
{
    switch (e) {
    case hipSuccess: return "hipSuccess";
    case hipErrorInvalidValue: return "hipErrorInvalidValue";
    case hipErrorOutOfMemory: return "hipErrorOutOfMemory";
    case hipErrorInvalidDevice: return "hipErrorInvalidDevice";
    case hipErrorNoDevice: return "hipErrorNoDevice";
    case hipErrorInvalidHandle: return "hipErrorInvalidHandle";
    case hipErrorLaunchFailure: return "hipErrorLaunchFailure";
    default: return "hipErrorUnknown";
    }
}

const char *hipGetErrorString(hipError_t e) { return hipGetErrorName(e); }

hipError_t hipHostMalloc(void **ptr, size_t size, unsigned int flags)
{
    if (!ptr) return hipErrorInvalidValue;
    *ptr = nullptr;
    if (inject("hipHostMalloc")) return hipErrorOutOfMemory;
    *ptr = std::malloc(size);
    return *ptr ? hipSuccess : hipErrorOutOfMemory;
}

hipError_t hipHostFree(void *ptr)
{
    std::free(ptr);
    return hipSuccess;
}

hipError_t hipEventCreateWithFlags(hipEvent_t *event, unsigned flags)
{
    if (!event) return hipErrorInvalidValue;
    if (inject("hipEventCreateWithFlags")) return hipErrorOutOfMemory;
    *event = new ihipEvent_t{kEventMagic, false};
    return hipSuccess;
}

hipError_t hipEventRecord(hipEvent_t event, hipStream_t stream)
{
    if (!event || event->magic != kEventMagic) return hipErrorInvalidHandle;
    if (inject("hipEventRecord")) return hipErrorLaunchFailure;
    event->recorded = true;
    return hipSuccess;
}

hipError_t hipEventSynchronize(hipEvent_t event)
{
    if (!event || event->magic != kEventMagic) return hipErrorInvalidHandle;
    if (inject("hipEventSynchronize")) return hipErrorLaunchFailure;
    return hipSuccess;
}

hipError_t hipEventDestroy(hipEvent_t event)
{
    if (!event || event->magic != kEventMagic) return hipErrorInvalidHandle;
    event->magic = 0;
    delete event;
    return hipSuccess;
}

}  // extern "C"
