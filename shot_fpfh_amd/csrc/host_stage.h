// host_stage.h -- what an entry point starts and ends with: the checks of a radius and of a list set against its cloud, the
// staging of host / device operands of any element type, and the closing wait (every .hip with an SF_IN_DEVICE / SF_OUT_DEVICE
// entry point uses it; DESIGN.md 3, "Host plumbing").
#pragma once
#include <cmath>

#include "common.h"

static inline int sf_check_radius(const char *who, const char *what, double r)
{
    if (r > 0.0 && std::isfinite(r)) return SF_OK;
    sf_set_error("%s: %s must be positive and finite (got %g)", who, what, r);
    return SF_ERR_ARG;
}

static inline int check_nbrs(sf_ctx *ctx, sf_cloud *c, sf_nbrs *nb, const char *who)
{
    if (!ctx || !c || !nb) { sf_set_error("%s: null argument", who); return SF_ERR_ARG; }
    if (!c->xs) { sf_set_error("%s: grid not built", who); return SF_ERR_STATE; }
    SF_CHECK(sf_nbrs_on_grid(nb, c, who));
    SF_HIP(hipSetDevice(ctx->device));
    return SF_OK;
}

// Host <-> device staging of one entry point.  Buffers come from the context pool through the caller's guard (released on
// every return path); copies are asynchronous on the context stream.  The call is closed by stage_sync() where it waits
// whenever any host buffer was involved, by stage_sync_out() where only an output that went to the host makes it wait.
template <typename T>
static inline int stage_in(sf_pool_guard &g, const T *src, size_t count, int flags, const T **dev)
{
    if (!src) { *dev = nullptr; return SF_OK; }
    if (flags & SF_IN_DEVICE) { *dev = src; return SF_OK; }
    T *owned = nullptr;
    SF_CHECK(g.alloc(&owned, count));
    if (count) SF_HIP(hipMemcpyAsync(owned, src, count * sizeof(T), hipMemcpyHostToDevice, g.ctx->stream));
    *dev = owned;
    return SF_OK;
}

template <typename T>
static inline int stage_out(sf_pool_guard &g, T *dst, size_t count, int flags, T **dev)
{
    if (flags & SF_OUT_DEVICE) { *dev = dst; return SF_OK; }
    return g.alloc(dev, count);
}

template <typename T>
static inline int finish_out(sf_ctx *ctx, T *dst, size_t count, int flags, const T *dev)
{
    if (!(flags & SF_OUT_DEVICE) && count)
        SF_HIP(hipMemcpyAsync(dst, dev, count * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
    return SF_OK;
}

static inline int stage_sync(sf_ctx *ctx, int flags)
{
    if ((flags & (SF_IN_DEVICE | SF_OUT_DEVICE)) != (SF_IN_DEVICE | SF_OUT_DEVICE)) SF_HIP(hipStreamSynchronize(ctx->stream));
    return SF_OK;
}

static inline int stage_sync_out(sf_ctx *ctx, int flags)
{
    if (!(flags & SF_OUT_DEVICE)) SF_HIP(hipStreamSynchronize(ctx->stream));
    return SF_OK;
}
