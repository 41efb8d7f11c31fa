// outliers.hip -- K20: outlier removal in front of the normals, the two filters PCL and Open3D put there.
//
//   statistical (k, std_ratio):   mean[i] = (sum of the distances from point i to its k + 1 nearest cloud points) / k -- the nearest
//                                 is i itself or an exact duplicate, distance 0, so this is the mean distance to the k nearest
//                                 OTHER points; mu = sum(mean) / n, sigma = sqrt(sum((mean - mu)^2) / (n - 1)),
//                                 threshold = mu + std_ratio sigma; point i is kept <=> mean[i] <= threshold (PCL's rule).
//   radius (radius, min_neighbors): count[i] = size of the ball of `radius` around point i, i included (the project's ball rule,
//                                 search.hip); point i is kept <=> count[i] - 1 >= min_neighbors.
//   Both return the kept indices, int64, ascending, in the caller's numbering (the convention of sf_iss_select).
//
// Mapping.  The statistical filter is a CONSUMER of the k-NN search: sf_knn_search answers the self query at k + 1 (k_knn4 /
// k_knn with their status and retry rounds, untouched), and k_knn_mean_distance walks the finished lists -- positions in the
// final grid, nearest first -- one 16-lane DPP row per query, four queries per wave as in the K2 family, lanes striding over the
// list, any length.  A lane gathers its neighbours' coordinates from the cell-sorted SoA (24 MB per 1M points: resident in the
// L2s), forms d2 by the ball rule's three operations, takes the correctly rounded square root and adds it to its own partial in
// list order; the sixteen partials are folded by the four DPP steps of sf_row16_sum.  One order of additions per list length: no
// atomics, a call repeats bit for bit.  Ties in d2 change which index a list names, never the distances, and equal distances
// are adjacent in the list, so the sequence of terms -- hence every bit of mean -- is a function of the cloud and k alone.
// mu and sigma are two passes over mean: block partials through sf_block_sum4_stage / sf_block_sum4_at on a grid fixed by n,
// then a one-block fold in a fixed order; the fold of the second pass forms the threshold, once, and the mask is taken against
// that stored value.  The radius filter is K2's count sweep (k_radius, MODE 0: search.hip::sf_k2_count_self) on the grid built for
// `radius`, a scatter to the caller's order, and the same select.  Compaction: rocprim's select over a counting iterator, as
// sf_iss_select uses it.
// What bounds it: the search in front (the mean pass reads 4 (k + 1) B of list and gathers 24 (k + 1) B from L2 per point, an
// order of magnitude below the search's candidate sweep); the radius filter is the count sweep.
#include <cmath>

#include "host_stage.h"
#include "search_util.h"

namespace {

#define SF_OUT_WPB 4 // waves per workgroup of the mean pass, four queries (16-lane rows) each: 256 threads, 16 queries

// mean[row of slot q] = (sum_t |p[idx[q L + t]] - query q|) / (L - 1) over the L = k + 1 entries of the list of processing slot q.
// qrow: slot -> query row (null: identity), zperm: query row (the cloud's internal order) -> the caller's index.
__global__ __launch_bounds__(64 * SF_OUT_WPB) void k_knn_mean_distance(const double *__restrict__ xs, const double *__restrict__ ys,
                                                                       const double *__restrict__ zs, const double *__restrict__ qx,
                                                                       const double *__restrict__ qy, const double *__restrict__ qz,
                                                                       const int32_t *__restrict__ idx, const int32_t *__restrict__ qrow,
                                                                       const int32_t *__restrict__ zperm, int64_t m, int len,
                                                                       double *__restrict__ mean)
{
    const int sl = threadIdx.x & 15;
    const int64_t q = (int64_t)blockIdx.x * (4 * SF_OUT_WPB) + (threadIdx.x >> 4);
    const bool live = q < m; // (no early return: the row reduction below is executed by whole waves)
    double acc = 0.0;
    if (live) {
        const double px = qx[q], py = qy[q], pz = qz[q];
        const int32_t *const list = idx + q * (int64_t)len;
        for (int t = sl; t < len; t += 16) {
            const int j = SF_LIST_LOAD(list + t);
            const double dx = xs[j] - px, dy = ys[j] - py, dz = zs[j] - pz;
            acc += sqrt((dx * dx + dy * dy) + dz * dz);
        }
    }
    const double sum = sf_row16_sum(acc);
    if (live && sl == 0) {
        const int32_t row = qrow ? qrow[q] : (int32_t)q;
        mean[zperm[row]] = sum / (double)(len - 1);
    }
}

// ---- mu, sigma, threshold: stats[0 .. 2] on the device ------------------------------------------------------------------
// PASS 0: partial[b] = this block's share of sum(x).  PASS 1: of sum((x - mu)^2), mu read from stats[0].  The grid is
// stats_blocks(n) blocks of 256 threads; thread t of block b adds elements (b + j B) 256 + t, j = 0, 1, .., in that order.
#define SF_OUT_FOLD 256
template <int PASS>
__global__ __launch_bounds__(256) void k_outlier_stats(const double *__restrict__ x, int64_t n, const double *__restrict__ stats,
                                                       double *__restrict__ partial)
{
    __shared__ double sh[4][1];
    const double mu = PASS == 1 ? stats[0] : 0.0;
    double acc[1] = {0.0};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double d = x[i] - mu;
        acc[0] += PASS == 1 ? d * d : d;
    }
    sf_block_sum4_stage(acc, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = sf_block_sum4_at(sh, 0);
}

// One block: thread t adds partial[t], partial[t + 256], .. in that order, then the block sum.  PASS 0: stats[0] = mu = S / n.
// PASS 1: stats[1] = sigma = sqrt(S / (n - 1)), stats[2] = threshold = mu + std_ratio sigma.
template <int PASS>
__global__ __launch_bounds__(SF_OUT_FOLD) void k_outlier_fold(const double *__restrict__ partial, int nb, int64_t n, double std_ratio,
                                                              double *__restrict__ stats)
{
    __shared__ double sh[4][1];
    double acc[1] = {0.0};
    for (int b = threadIdx.x; b < nb; b += SF_OUT_FOLD) acc[0] += partial[b];
    sf_block_sum4_stage(acc, sh);
    if (threadIdx.x == 0) {
        const double s = sf_block_sum4_at(sh, 0);
        if (PASS == 0) {
            stats[0] = s / (double)n;
        } else {
            const double sigma = sqrt(s / (double)(n - 1));
            stats[1] = sigma;
            stats[2] = stats[0] + std_ratio * sigma;
        }
    }
}

int stats_blocks(int64_t n) { return (int)std::min<int64_t>(std::max<int64_t>(sf_div_up(n, 1024), 1), 1024); } // (n alone)

struct keep_near { // mean[i] <= threshold, the stored one
    const double *mean, *stats;
    __host__ __device__ bool operator()(int64_t i) const { return mean[i] <= stats[2]; }
};
struct keep_dense { // count[i] - 1 >= min_neighbors
    const int32_t *count;
    int min_neighbors;
    __host__ __device__ bool operator()(int64_t i) const { return count[i] - 1 >= min_neighbors; }
};

// mean (device, n, caller order) of the self query at k + 1
int mean_dev(sf_ctx *ctx, sf_cloud *c, int k, double *mean)
{
    const int64_t n = c->n;
    sf_nbrs *nb = sf_knn_search(ctx, c, c->xyz_orig, n, k + 1, SF_IN_DEVICE); // (builds its own grid: no trace of earlier searches)
    if (!nb) return SF_ERR_HIP; // (the search has set the message)
    int rc = sf_nbrs_on_grid(nb, c, "sf_knn_mean_distance");
    if (rc == SF_OK) {
        sf_launch_timer t_(ctx, "k20_mean_distance");
        hipLaunchKernelGGL(k_knn_mean_distance, dim3((unsigned)sf_div_up(n, 4 * SF_OUT_WPB)), dim3(64 * SF_OUT_WPB), 0, ctx->stream,
                           (const double *)c->xs, (const double *)c->ys, (const double *)c->zs, (const double *)nb->qx,
                           (const double *)nb->qy, (const double *)nb->qz, (const int32_t *)nb->idx, (const int32_t *)nb->qrow,
                           (const int32_t *)c->zperm, n, k + 1, mean);
        if (hipGetLastError() != hipSuccess) { sf_set_error("sf_knn_mean_distance: launch failed"); rc = SF_ERR_HIP; }
    }
    sf_nbrs_free(ctx, nb); // (stream-ordered: the blocks go back to the pool behind the kernel)
    return rc;
}

// stats[0 .. 2] (device) of mean
int stats_dev(sf_ctx *ctx, const double *mean, int64_t n, double std_ratio, double *stats)
{
    sf_pool_guard tmp(ctx);
    const int nb = stats_blocks(n);
    double *partial = nullptr;
    SF_CHECK(tmp.alloc(&partial, (size_t)nb));
    SF_LAUNCH(ctx, "k20_stats", k_outlier_stats<0>, dim3(nb), dim3(256), mean, n, (const double *)stats, partial);
    SF_LAUNCH(ctx, "k20_stats", k_outlier_fold<0>, dim3(1), dim3(SF_OUT_FOLD), (const double *)partial, nb, n, std_ratio, stats);
    SF_LAUNCH(ctx, "k20_stats", k_outlier_stats<1>, dim3(nb), dim3(256), mean, n, (const double *)stats, partial);
    SF_LAUNCH(ctx, "k20_stats", k_outlier_fold<1>, dim3(1), dim3(SF_OUT_FOLD), (const double *)partial, nb, n, std_ratio, stats);
    return SF_OK;
}

// the indices i of 0 .. n - 1 with pred(i), ascending (device), and their number (device word *dnum)
template <typename Pred>
int select_dev(sf_ctx *ctx, int64_t n, Pred pred, int64_t *selected, size_t *dnum)
{
    sf_pool_guard tmp(ctx);
    return sf_select_indices(ctx, tmp, "k20_select", n, pred, selected, dnum);
}

// ball sizes (device, n, caller order) on the grid built for `radius`
int counts_dev(sf_ctx *ctx, sf_cloud *c, double radius, int32_t *count)
{
    sf_pool_guard tmp(ctx);
    int32_t *sorted = nullptr;
    SF_CHECK(sf_k2_ball_sizes(ctx, c, tmp, radius, "k20_ball_count", &sorted));
    return sf_perm_scatter(ctx, "k20_scatter", c, (const int32_t *)sorted, count);
}

// The tail of both filters: everything the host wants is queued behind the kernels -- the count and the three statistics into
// the context's pinned words, the per-point array and (n_selected being unknown until then) all n index slots to the caller --
// and the call waits ONCE.  With SF_OUT_DEVICE only the pinned words travel.
int finish(sf_ctx *ctx, int64_t n, const size_t *dnum, const double *dstats, double *stats, const int64_t *dsel, int64_t *selected,
           int64_t *n_selected, const void *dvals, void *vals, size_t val_bytes, int flags)
{
    void *pin = nullptr;
    SF_CHECK(sf_ctx_pinned(ctx, &pin));
    SF_HIP(hipMemcpyAsync(pin, dnum, sizeof(size_t), hipMemcpyDeviceToHost, ctx->stream));
    if (dstats) SF_HIP(hipMemcpyAsync((char *)pin + 8, dstats, 3 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (!(flags & SF_OUT_DEVICE)) {
        SF_HIP(hipMemcpyAsync(selected, dsel, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
        if (vals) SF_HIP(hipMemcpyAsync(vals, dvals, (size_t)n * val_bytes, hipMemcpyDeviceToHost, ctx->stream));
    }
    SF_HIP(hipStreamSynchronize(ctx->stream));
    *n_selected = (int64_t) * (const size_t *)pin;
    if (dstats && stats) memcpy(stats, (const char *)pin + 8, 3 * sizeof(double));
    return SF_OK;
}

int check_statistical(const char *who, const sf_cloud *c, int k, double std_ratio)
{
    if (c->n < 2) { sf_set_error("%s: the cloud needs at least two points (has %lld)", who, (long long)c->n); return SF_ERR_ARG; }
    if (k < 1 || (int64_t)k > c->n - 1) {
        sf_set_error("%s: k=%d must be in 1..%lld (the number of other cloud points)", who, k, (long long)(c->n - 1));
        return SF_ERR_ARG;
    }
    if (!std::isfinite(std_ratio)) { sf_set_error("%s: std_ratio must be finite (got %g)", who, std_ratio); return SF_ERR_ARG; }
    return SF_OK;
}

int check_radius_rule(const char *who, double radius, int min_neighbors)
{
    SF_CHECK(sf_check_radius(who, "radius", radius));
    if (min_neighbors < 0) { sf_set_error("%s: min_neighbors must not be negative (got %d)", who, min_neighbors); return SF_ERR_ARG; }
    return SF_OK;
}

} // namespace

extern "C" int sf_knn_mean_distance(sf_ctx *ctx, sf_cloud *c, int k, double *mean, int flags)
{
    if (!ctx || !c || !mean) { sf_set_error("sf_knn_mean_distance: null argument"); return SF_ERR_ARG; }
    SF_CHECK(check_statistical("sf_knn_mean_distance", c, k, 0.0));
    SF_HIP(hipSetDevice(ctx->device));
    const int64_t n = c->n;
    sf_pool_guard tmp(ctx);
    double *dmean = nullptr;
    SF_CHECK(stage_out(tmp, mean, (size_t)n, flags, &dmean));
    SF_CHECK(mean_dev(ctx, c, k, dmean));
    SF_CHECK(finish_out(ctx, mean, (size_t)n, flags, dmean));
    return stage_sync_out(ctx, flags);
}

extern "C" int sf_outliers_statistical(sf_ctx *ctx, sf_cloud *c, int k, double std_ratio, double *mean, double *stats, int64_t *selected,
                                       int64_t *n_selected, int flags)
{
    if (!ctx || !c || !selected || !n_selected) { sf_set_error("sf_outliers_statistical: null argument"); return SF_ERR_ARG; }
    SF_CHECK(check_statistical("sf_outliers_statistical", c, k, std_ratio));
    SF_HIP(hipSetDevice(ctx->device));
    const int64_t n = c->n;
    *n_selected = 0;
    sf_pool_guard tmp(ctx);
    const bool dev_out = (flags & SF_OUT_DEVICE) != 0;
    double *dmean = mean, *dstats = nullptr;
    int64_t *dsel = nullptr;
    size_t *dnum = nullptr;
    if (!dev_out || !mean) SF_CHECK(tmp.alloc(&dmean, (size_t)n)); // (wanted on the host, or not wanted at all)
    SF_CHECK(stage_out(tmp, selected, (size_t)n, flags, &dsel));
    SF_CHECK(tmp.alloc(&dstats, 3));
    SF_CHECK(tmp.alloc(&dnum, 1));
    SF_CHECK(mean_dev(ctx, c, k, dmean));
    SF_CHECK(stats_dev(ctx, dmean, n, std_ratio, dstats));
    SF_CHECK(select_dev(ctx, n, keep_near{dmean, dstats}, dsel, dnum));
    return finish(ctx, n, dnum, dstats, stats, dsel, selected, n_selected, dmean, mean, sizeof(double), flags);
}

extern "C" int sf_ball_counts(sf_ctx *ctx, sf_cloud *c, double radius, int32_t *count, int flags)
{
    if (!ctx || !c || !count) { sf_set_error("sf_ball_counts: null argument"); return SF_ERR_ARG; }
    SF_CHECK(check_radius_rule("sf_ball_counts", radius, 0));
    SF_HIP(hipSetDevice(ctx->device));
    const int64_t n = c->n;
    if (!n) return SF_OK;
    sf_pool_guard tmp(ctx);
    int32_t *dcount = nullptr;
    SF_CHECK(stage_out(tmp, count, (size_t)n, flags, &dcount));
    SF_CHECK(counts_dev(ctx, c, radius, dcount));
    SF_CHECK(finish_out(ctx, count, (size_t)n, flags, dcount));
    return stage_sync_out(ctx, flags);
}

extern "C" int sf_outliers_radius(sf_ctx *ctx, sf_cloud *c, double radius, int min_neighbors, int32_t *count, int64_t *selected,
                                  int64_t *n_selected, int flags)
{
    if (!ctx || !c || !selected || !n_selected) { sf_set_error("sf_outliers_radius: null argument"); return SF_ERR_ARG; }
    SF_CHECK(check_radius_rule("sf_outliers_radius", radius, min_neighbors));
    SF_HIP(hipSetDevice(ctx->device));
    const int64_t n = c->n;
    *n_selected = 0;
    if (!n) return SF_OK;
    sf_pool_guard tmp(ctx);
    const bool dev_out = (flags & SF_OUT_DEVICE) != 0;
    int32_t *dcount = count;
    int64_t *dsel = nullptr;
    size_t *dnum = nullptr;
    if (!dev_out || !count) SF_CHECK(tmp.alloc(&dcount, (size_t)n)); // (wanted on the host, or not wanted at all)
    SF_CHECK(stage_out(tmp, selected, (size_t)n, flags, &dsel));
    SF_CHECK(tmp.alloc(&dnum, 1));
    SF_CHECK(counts_dev(ctx, c, radius, dcount));
    SF_CHECK(select_dev(ctx, n, keep_dense{dcount, min_neighbors}, dsel, dnum));
    return finish(ctx, n, dnum, nullptr, nullptr, dsel, selected, n_selected, dcount, count, sizeof(int32_t), flags);
}
