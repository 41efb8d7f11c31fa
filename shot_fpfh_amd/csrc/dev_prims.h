// dev_prims.h -- the rocPRIM device primitives as the host code calls them: the sort configuration, the two-phase call (size
// query, temporary from the pool, the call proper under its timer) and the selection of indices that four stages end with.
#pragma once
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include <optional>

#include "common.h"

// rocPRIM's radix sort falls back to a merge sort up to 2^20 items (a 1M-point cloud: block sort + 10 merge passes
// x 2 kernels = 21 launches, 0.16 ms); Onesweep above 64k items does the 16-17 cell-id bits in a few launches.
// ... and rocPRIM 4.2 carries no tuned Onesweep configuration for gfx950: the generic one sorts 4 bits per pass.  Ten bits per
// pass (1024-thread blocks, 6 items per thread, match ranking) sorts the 20-bit cell ids of a 1M-point cloud in two passes:
// 0.117 -> 0.068 ms (8 bits: 0.092-0.102, 11 bits: 0.090, 12 bits: does not fit LDS; tools/ab_k1.sh)
#ifndef SF_SORT_BITS
#define SF_SORT_BITS 10
#endif
#ifndef SF_SORT_BLOCK
#define SF_SORT_BLOCK 1024
#endif
#ifndef SF_SORT_ITEMS
#define SF_SORT_ITEMS 6
#endif
using sf_onesweep = rocprim::radix_sort_onesweep_config<rocprim::kernel_config<SF_SORT_BLOCK, SF_SORT_ITEMS>, rocprim::kernel_config<SF_SORT_BLOCK, SF_SORT_ITEMS>,
                                                        SF_SORT_BITS, rocprim::block_radix_rank_algorithm::match>;
using sf_sort_config = rocprim::radix_sort_config<rocprim::default_config, rocprim::default_config, sf_onesweep, 65536>;

// One rocPRIM device primitive: call(nullptr, bytes) asks for the size of the temporary, alloc(bytes, &tmp) provides it,
// call(tmp, bytes) runs -- under the launch timer `name` when `timed`; a caller that sits inside a block timer of its own
// passes false, `name` then only labels the error.  `call` is hipError_t(void *tmp, size_t &bytes): a lambda that names the
// primitive and its arguments once.  `alloc` is int(size_t bytes, void **tmp).
template <typename Alloc, typename Call>
static inline int sf_rocprim_in(sf_ctx *ctx, Alloc alloc, const char *name, bool timed, Call call)
{
    size_t bytes = 0;
    hipError_t e = call(nullptr, bytes);
    if (e == hipSuccess) {
        void *tmp = nullptr;
        SF_CHECK(alloc(bytes ? bytes : 8, &tmp));
        std::optional<sf_launch_timer> t_;
        if (timed) t_.emplace(ctx, name);
        e = call(tmp, bytes);
    }
    if (e == hipSuccess) return SF_OK;
    sf_set_error("%s: rocPRIM call failed: %s", name, hipGetErrorString(e));
    return SF_ERR_HIP;
}
// ... with the temporary lent by the guard from the pool (until the guard leaves scope): every site but voxel.hip's two, which
// keep the context scratch they had until the pool is measured there
template <typename Call>
static inline int sf_rocprim(sf_ctx *ctx, sf_pool_guard &g, const char *name, bool timed, Call call)
{
    return sf_rocprim_in(ctx, [&](size_t bytes, void **tmp) { return g.alloc((char **)tmp, bytes); }, name, timed, call);
}

// out[0 .. *dnum) = the i of 0 .. n - 1 with pred(i), ascending (device arrays; *dnum a device word), under the timer `name`
template <typename I, typename Pred>
static inline int sf_select_indices(sf_ctx *ctx, sf_pool_guard &g, const char *name, int64_t n, Pred pred, I *out, size_t *dnum)
{
    return sf_rocprim(ctx, g, name, true, [&](void *tmp, size_t &bytes) {
        return rocprim::select(tmp, bytes, rocprim::counting_iterator<I>(0), out, dnum, (size_t)n, pred, ctx->stream);
    });
}
