// gol_halo.cpp — halo exchange between strip engines.
#include "gol_ctx.h"

using namespace goleng;

namespace {

int copy_rows_between(gol_ctx *dst, int dst_row, gol_ctx *src, int src_row, int K)
{
    if (dst->nw != src->nw) return fail(dst, GOL_EINVAL, "width mismatch");
    if (src->il != dst->il) {   // raw row copies need one layout on both sides
        DeviceGuard gs(src->device);
        if (int rc = ensure_layout(src, dst->il)) return rc;
    }
    // dst stream waits for src's queued work (src's event, on src's device); copy on dst's
    // stream; then src's stream waits for the copy (dst's event)
    {
        DeviceGuard g(src->device);
        HIP_OR_FAIL(dst, hipEventRecord(src->ev_copy, src->stream));
    }
    DeviceGuard g(dst->device);
    HIP_OR_FAIL(dst, hipStreamWaitEvent(dst->stream, src->ev_copy, 0));
    const size_t rowb = (size_t)dst->nw * 8;
    uint64_t *d = dst->board[dst->cur] + (size_t)dst_row * dst->pitch;
    const uint64_t *s = src->board[src->cur] + (size_t)src_row * src->pitch;
    if (dst->device == src->device) {
        HIP_OR_FAIL(dst, hipMemcpy2DAsync(d, (size_t)dst->pitch * 8, s, (size_t)src->pitch * 8,
                                          rowb, K, hipMemcpyDeviceToDevice, dst->stream));
    } else {
        // rows are contiguous when pitch == nw (always true for engines created here)
        HIP_OR_FAIL(dst, hipMemcpyPeerAsync(d, dst->device, s, src->device, rowb * K,
                                            dst->stream));
    }
    // src must not overwrite these rows before the copy lands
    HIP_OR_FAIL(dst, hipEventRecord(dst->ev_copy, dst->stream));
    {
        DeviceGuard g2(src->device);
        HIP_OR_FAIL(dst, hipStreamWaitEvent(src->stream, dst->ev_copy, 0));
    }
    return GOL_OK;
}

}  // namespace

extern "C" {

int gol_export_halo(gol_ctx *c, void *top, void *bottom, void *s)
{
    if (!c || !top || !bottom) return GOL_EINVAL;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    if (!is_strip(c)) return fail(c, GOL_ESTATE, "not a strip engine");
    DeviceGuard g(c->device);
    hipStream_t st = s ? (hipStream_t)s : c->stream;
    if (st != c->stream) {
        // make the caller's stream wait for the engine's queued turns
        hipEvent_t ev;
        HIP_OR_FAIL(c, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        HIP_OR_FAIL(c, hipEventRecord(ev, c->stream));
        HIP_OR_FAIL(c, hipStreamWaitEvent(st, ev, 0));
        (void)hipEventDestroy(ev);
    }
    const int K = c->cfg.halo;
    const size_t rowb = (size_t)c->nw * 8;
    const uint64_t *b = c->board[c->cur];
    if (c->il) {   // halo rows cross the API in the standard layout
        HIP_OR_FAIL(c, golk::launch_il_convert(b + (size_t)own_lo(c) * c->pitch, c->pitch,
                                               (uint64_t *)top, c->nw, K, c->nw, false, st));
        HIP_OR_FAIL(c, golk::launch_il_convert(b + (size_t)(own_hi(c) - K) * c->pitch, c->pitch,
                                               (uint64_t *)bottom, c->nw, K, c->nw, false, st));
        return GOL_OK;
    }
    HIP_OR_FAIL(c, hipMemcpy2DAsync(top, rowb, b + (size_t)own_lo(c) * c->pitch,
                                    (size_t)c->pitch * 8, rowb, K, hipMemcpyDeviceToDevice, st));
    HIP_OR_FAIL(c, hipMemcpy2DAsync(bottom, rowb, b + (size_t)(own_hi(c) - K) * c->pitch,
                                    (size_t)c->pitch * 8, rowb, K, hipMemcpyDeviceToDevice, st));
    return GOL_OK;
}

int gol_import_halo(gol_ctx *c, const void *top, const void *bottom, void *s)
{
    if (!c || !top || !bottom) return GOL_EINVAL;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    if (!is_strip(c)) return fail(c, GOL_ESTATE, "not a strip engine");
    DeviceGuard g(c->device);
    hipStream_t st = s ? (hipStream_t)s : c->stream;
    const int K = c->cfg.halo;
    const size_t rowb = (size_t)c->nw * 8;
    uint64_t *b = c->board[c->cur];
    if (c->il) {
        HIP_OR_FAIL(c, golk::launch_il_convert((const uint64_t *)top, c->nw, b, c->pitch, K, c->nw,
                                               true, st));
        HIP_OR_FAIL(c, golk::launch_il_convert((const uint64_t *)bottom, c->nw,
                                               b + (size_t)own_hi(c) * c->pitch, c->pitch, K,
                                               c->nw, true, st));
    } else {
        HIP_OR_FAIL(c, hipMemcpy2DAsync(b, (size_t)c->pitch * 8, top, rowb, rowb, K,
                                        hipMemcpyDeviceToDevice, st));
        HIP_OR_FAIL(c, hipMemcpy2DAsync(b + (size_t)own_hi(c) * c->pitch, (size_t)c->pitch * 8,
                                        bottom, rowb, rowb, K, hipMemcpyDeviceToDevice, st));
    }
    if (st != c->stream) {
        hipEvent_t ev;
        HIP_OR_FAIL(c, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        HIP_OR_FAIL(c, hipEventRecord(ev, st));
        HIP_OR_FAIL(c, hipStreamWaitEvent(c->stream, ev, 0));
        (void)hipEventDestroy(ev);
    }
    c->halo_valid = K;
    return GOL_OK;
}

int gol_copy_halo_from_upper(gol_ctx *dst, gol_ctx *src)
{
    if (!dst || !src || !is_strip(dst) || !is_strip(src) || dst->cfg.halo != src->cfg.halo)
        return GOL_EINVAL;
    // both engines at once, deadlock-free in any order (a ring pair exchanging both ways from
    // two host threads); dst == src (one strip exchanging with itself) is one recursive lock
    std::scoped_lock lk(dst->mu, src->mu);
    const int K = dst->cfg.halo;
    return copy_rows_between(dst, 0, src, own_hi(src) - K, K);
}

int gol_copy_halo_from_lower(gol_ctx *dst, gol_ctx *src)
{
    if (!dst || !src || !is_strip(dst) || !is_strip(src) || dst->cfg.halo != src->cfg.halo)
        return GOL_EINVAL;
    std::scoped_lock lk(dst->mu, src->mu);
    const int K = dst->cfg.halo;
    return copy_rows_between(dst, own_hi(dst), src, own_lo(src), K);
}

int gol_halo_done(gol_ctx *c)
{
    if (!c || !is_strip(c)) return GOL_EINVAL;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    c->halo_valid = c->cfg.halo;
    return GOL_OK;
}

int gol_halo_buffers(gol_ctx *c, void **send_top, void **send_bottom, void **recv_top,
                     void **recv_bottom, int32_t *layout)
{
    if (!c || !send_top || !send_bottom || !recv_top || !recv_bottom || !layout)
        return GOL_EINVAL;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    if (!is_strip(c)) return fail(c, GOL_ESTATE, "not a strip engine");
    DeviceGuard g(c->device);
    // the layout the first launch after a full exchange runs on: gol_step's own rule
    // (plan_launch) with halo turns to go -- whatever the step after the exchange asks
    // for, its first launch has the depth plan_launch gives min(turns, halo); the layout is
    // the same for every depth >= 2, and a function of width, halo and flags only, so equal
    // on every rank
    const bool il = stepping_il(c, plan_launch(c, c->cfg.halo).k);
    if (int rc = ensure_layout(c, il)) return rc;
    uint64_t *b = c->board[c->cur];
    const int K = c->cfg.halo;
    *send_top = b + (size_t)own_lo(c) * c->pitch;
    *send_bottom = b + (size_t)(own_hi(c) - K) * c->pitch;
    *recv_top = b;
    *recv_bottom = b + (size_t)own_hi(c) * c->pitch;
    *layout = c->il ? 1 : 0;
    return GOL_OK;
}

}  // extern "C"
