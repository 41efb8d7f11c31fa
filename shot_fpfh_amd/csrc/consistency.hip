// consistency.hip -- K13: the geometric-consistency filter of a set of matches.
//
// No counterpart in the reference.  A rigid motion keeps lengths, so two matches i and j can both be true only if the scan side's
// |a_i - a_j| equals the reference side's |b_i - b_j| within the noise.  With, in unfused float64 and exactly this order,
//   dp(i,j) = sqrt(((ax_i - ax_j)^2 + (ay_i - ay_j)^2) + (az_i - az_j)^2),   dq(i,j) the same on b,
//   compat(i,j) = i != j  and  |dp - dq| <= distance_threshold  and  min(dp, dq) >= min_edge        (a NaN compares false),
//   degree[i] = #{ j : member[j] and compat(i,j) }                                                  (no mask: every column),
// the group is: deg over all columns; seed = the LOWEST index among the maxima of deg; member = compat(seed, .) with the seed
// itself; g = sum member; gdeg = degree over the member columns -- the definition of tests/consistency_numpy.py.  Every output is
// an integer decided in float64, so the device agrees with the statement exactly, whatever the order the pairs are visited in.
//
// k13_degree is the m^2 part: a thread owns a row (6 coordinates in registers), the columns go through LDS a tile at a time and
// every lane of a wave reads the SAME column (a broadcast read), so the inner loop is 16 float64 operations, two square roots and
// three compares per pair and nothing else.  The grid is 2-D, row blocks x column slices, so that a few thousand matches already
// fill the chip; a slice adds its count into the row's uint32 with one integer atomic, which is exact in any order.  A column
// outside the mask is staged as NaN: it is compatible with nothing, and the inner loop carries no mask test.
// The chain of sf_consistency_group (degree, arg-max, mark, count, masked degree) is queued on the stream; the host waits once.
#include "common.h"
#include "device_util.h"

namespace {

constexpr int K13_BLOCK = 256;          // rows of a block, one per thread
constexpr int K13_TILE = 128;           // columns staged through LDS at a time: 16 row blocks x 32 tiles at m = 4096, 2 blocks per CU
constexpr int K13_TARGET_BLOCKS = 4096; // column slices are cut until the grid has about this many blocks (16 per CU)
constexpr int K13_FOLD = 1024;          // threads of the single-block kernels
constexpr double K13_DBL_MAX = 1.7976931348623157e308;

// the device info block (int64)
enum { IN_SEED = 0, IN_SEED_DEGREE = 1, IN_GROUP = 2, IN_STATUS = 3, IN_SIZE = 4 };

// (min(dp, dq) >= min_edge as two compares: the same decision, and false for a NaN like every comparison of the definition)
__device__ __forceinline__ bool k13_compat(double ax, double ay, double az, double bx, double by, double bz, double cax, double cay,
                                           double caz, double cbx, double cby, double cbz, double thr, double min_edge)
{
    const double ux = ax - cax, uy = ay - cay, uz = az - caz;
    const double vx = bx - cbx, vy = by - cby, vz = bz - cbz;
    const double dp = sqrt((ux * ux + uy * uy) + uz * uz);
    const double dq = sqrt((vx * vx + vy * vy) + vz * vz);
    return fabs(dp - dq) <= thr && dp >= min_edge && dq >= min_edge;
}

// grid: (row blocks, column slices).  Slice y counts columns [y, y + 1) * tiles_per_slice * K13_TILE of the rows of block x.
__global__ __launch_bounds__(K13_BLOCK) void k13_degree(const double *__restrict__ a, const double *__restrict__ b, int64_t m,
                                                        const unsigned char *__restrict__ member, double thr, double min_edge,
                                                        int tiles_per_slice, unsigned *__restrict__ degree)
{
    __shared__ __attribute__((aligned(16))) double col[K13_TILE * 6]; // per column: ax ay az bx by bz
    const double nan = __builtin_nan("");
    const int64_t i = (int64_t)blockIdx.x * K13_BLOCK + threadIdx.x;
    double ax = nan, ay = nan, az = nan, bx = nan, by = nan, bz = nan; // (a thread past the last row counts nothing)
    if (i < m) {
        ax = a[3 * i]; ay = a[3 * i + 1]; az = a[3 * i + 2];
        bx = b[3 * i]; by = b[3 * i + 1]; bz = b[3 * i + 2];
    }
    const int64_t tile0 = (int64_t)blockIdx.y * tiles_per_slice;
    unsigned count = 0;
    for (int t = 0; t < tiles_per_slice; ++t) {
        const int64_t j0 = (tile0 + t) * K13_TILE;
        if (j0 >= m) break; // (the same for the whole block)
        __syncthreads();    // the previous tile has been read by every wave
        for (int e = threadIdx.x; e < 6 * K13_TILE; e += K13_BLOCK) { // 3 K13_TILE doubles of a, then of b: coalesced
            const int side = e >= 3 * K13_TILE ? 1 : 0;
            const int r = e - side * 3 * K13_TILE, c = r / 3;
            const int64_t j = j0 + c;
            double v = nan;
            if (j < m && (!member || member[j])) v = (side ? b : a)[3 * j0 + r];
            col[6 * c + 3 * side + (r - 3 * c)] = v;
        }
        __syncthreads();
        const int lim = (int)(m - j0 < K13_TILE ? m - j0 : K13_TILE);
#pragma unroll 4
        for (int c = 0; c < lim; ++c) {
            const double *q = col + 6 * c; // one address for the whole wave: a broadcast read
            const bool ok = k13_compat(ax, ay, az, bx, by, bz, q[0], q[1], q[2], q[3], q[4], q[5], thr, min_edge);
            count += (ok && j0 + c != i) ? 1u : 0u;
        }
    }
    if (i < m && count) atomicAdd(&degree[i], count);
}

// One block: the first maximum of degree[0 .. m), as the 64-bit maximum of degree << 32 | ~index.
__global__ __launch_bounds__(K13_FOLD) void k13_argmax(const unsigned *__restrict__ degree, int64_t m, int64_t *__restrict__ info)
{
    __shared__ unsigned long long sh[K13_FOLD / SF_WAVE];
    unsigned long long best = 0; // (degree 0 at index 2^32 - 1: below every real entry, m <= 2^31 - 1)
    for (int64_t j = threadIdx.x; j < m; j += K13_FOLD) {
        const unsigned long long key = ((unsigned long long)degree[j] << 32) | (unsigned)~(unsigned)j;
        best = key > best ? key : best;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long y = __shfl_xor(best, off);
        best = y > best ? y : best;
    }
    if ((threadIdx.x & (SF_WAVE - 1)) == 0) sh[threadIdx.x / SF_WAVE] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < K13_FOLD / SF_WAVE; ++w) best = sh[w] > best ? sh[w] : best;
        info[IN_SEED] = (int64_t)(unsigned)~(unsigned)(best & 0xffffffffull);
        info[IN_SEED_DEGREE] = (int64_t)(best >> 32);
    }
}

// member[j] = compat(seed, j), and the seed itself; all zeros when no pair is compatible.  The seed is read from device memory.
__global__ __launch_bounds__(K13_BLOCK) void k13_mark(const double *__restrict__ a, const double *__restrict__ b, int64_t m, double thr,
                                                      double min_edge, const int64_t *__restrict__ info,
                                                      unsigned char *__restrict__ member)
{
    const int64_t j = (int64_t)blockIdx.x * K13_BLOCK + threadIdx.x;
    if (j >= m) return;
    const int64_t seed = info[IN_SEED];
    if (info[IN_SEED_DEGREE] == 0) { member[j] = 0; return; }
    const bool ok = k13_compat(a[3 * seed], a[3 * seed + 1], a[3 * seed + 2], b[3 * seed], b[3 * seed + 1], b[3 * seed + 2], a[3 * j],
                               a[3 * j + 1], a[3 * j + 2], b[3 * j], b[3 * j + 1], b[3 * j + 2], thr, min_edge);
    member[j] = (ok || j == seed) ? 1 : 0;
}

// One block: g = the number of members; the status (1: no compatible pair).
__global__ __launch_bounds__(K13_FOLD) void k13_count(const unsigned char *__restrict__ member, int64_t m, int64_t *__restrict__ info)
{
    __shared__ unsigned long long sh[K13_FOLD / SF_WAVE];
    unsigned long long n = 0;
    for (int64_t j = threadIdx.x; j < m; j += K13_FOLD) n += member[j] ? 1 : 0;
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off);
    if ((threadIdx.x & (SF_WAVE - 1)) == 0) sh[threadIdx.x / SF_WAVE] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < K13_FOLD / SF_WAVE; ++w) n += sh[w];
        info[IN_GROUP] = (int64_t)n;
        info[IN_STATUS] = info[IN_SEED_DEGREE] == 0 ? 1 : 0;
    }
}

int k13_check(const char *who, bool pointers, int64_t m, double thr, double min_edge)
{
    if (!pointers || m < 0) { sf_set_error("%s: bad argument", who); return SF_ERR_ARG; }
    if (m > 0x7fffffffll) { sf_set_error("%s: %lld matches, at most 2^31 - 1", who, (long long)m); return SF_ERR_ARG; }
    if (!(thr >= 0.0 && thr <= K13_DBL_MAX) || !(min_edge >= 0.0 && min_edge <= K13_DBL_MAX)) {
        sf_set_error("%s: distance_threshold %g and min_edge %g must be finite and not negative", who, thr, min_edge);
        return SF_ERR_ARG;
    }
    return SF_OK;
}

// degree_dev <- 0, then one launch: the slices add into it.
int k13_launch_degree(sf_ctx *ctx, const double *a, const double *b, int64_t m, const unsigned char *member, double thr,
                      double min_edge, unsigned *degree_dev)
{
    const int64_t row_blocks = sf_div_up(m, K13_BLOCK), tiles = sf_div_up(m, K13_TILE);
    const int64_t want = std::min<int64_t>(tiles, std::max<int64_t>(1, sf_div_up(K13_TARGET_BLOCKS, row_blocks)));
    const int tiles_per_slice = (int)sf_div_up(tiles, want);
    const int64_t slices = sf_div_up(tiles, tiles_per_slice); // <= K13_TARGET_BLOCKS
    SF_HIP(hipMemsetAsync(degree_dev, 0, (size_t)m * sizeof(unsigned), ctx->stream));
    SF_LAUNCH(ctx, "k13_degree", k13_degree, dim3((unsigned)row_blocks, (unsigned)slices), dim3(K13_BLOCK), a, b, m, member, thr,
              min_edge, tiles_per_slice, degree_dev);
    return SF_OK;
}

} // namespace

extern "C" int sf_consistency_degree(sf_ctx *ctx, const double *a_dev, const double *b_dev, int64_t m,
                                     const unsigned char *member_dev, double distance_threshold, double min_edge,
                                     unsigned *degree_dev)
{
    SF_CHECK(k13_check("sf_consistency_degree", ctx && a_dev && b_dev && degree_dev, m, distance_threshold, min_edge));
    if (m == 0) return SF_OK;
    SF_HIP(hipSetDevice(ctx->device));
    return k13_launch_degree(ctx, a_dev, b_dev, m, member_dev, distance_threshold, min_edge, degree_dev);
}

extern "C" int sf_consistency_group(sf_ctx *ctx, const double *a_dev, const double *b_dev, int64_t m, double distance_threshold,
                                    double min_edge, unsigned *degree_dev, unsigned char *member_dev, unsigned *group_degree_dev,
                                    int64_t *info)
{
    SF_CHECK(k13_check("sf_consistency_group", ctx && a_dev && b_dev && degree_dev && member_dev && group_degree_dev && info, m,
                       distance_threshold, min_edge));
    if (m == 0) return SF_OK;
    SF_HIP(hipSetDevice(ctx->device));
    sf_pool_guard tmp(ctx);
    int64_t *dinfo = nullptr;
    SF_CHECK(tmp.alloc(&dinfo, IN_SIZE));
    const dim3 one(1), fold(K13_FOLD);
    // queued back to back: nothing below waits for the device
    SF_CHECK(k13_launch_degree(ctx, a_dev, b_dev, m, nullptr, distance_threshold, min_edge, degree_dev));
    SF_LAUNCH(ctx, "k13_argmax", k13_argmax, one, fold, (const unsigned *)degree_dev, m, dinfo);
    SF_LAUNCH(ctx, "k13_mark", k13_mark, dim3((unsigned)sf_div_up(m, K13_BLOCK)), dim3(K13_BLOCK), a_dev, b_dev, m, distance_threshold,
              min_edge, (const int64_t *)dinfo, member_dev);
    SF_LAUNCH(ctx, "k13_count", k13_count, one, fold, (const unsigned char *)member_dev, m, dinfo);
    SF_CHECK(k13_launch_degree(ctx, a_dev, b_dev, m, member_dev, distance_threshold, min_edge, group_degree_dev));
    void *pin = nullptr;
    SF_CHECK(sf_ctx_pinned(ctx, &pin));
    int64_t *hi = (int64_t *)pin;
    SF_HIP(hipMemcpyAsync(hi, dinfo, IN_SIZE * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    SF_HIP(hipStreamSynchronize(ctx->stream)); // the one wait of the call
    for (int v = 0; v < IN_SIZE; ++v) info[v] = hi[v];
    if (info[IN_STATUS] != 0) info[IN_SEED] = -1; // no compatible pair: no seed, no group
    return SF_OK;
}
