// ransac.hip -- K11: RANSAC with pre-rejection, the Kabsch fits on the device and the sums of a refit over the inliers.
//
// No counterpart in the reference, whose ransac_on_matches (ransac.py:17-82) scores every draw and keeps the first best minimal
// sample.  Here, per draw (k11_hypotheses, one thread each):
//   1. the edge-length test of Open3D's CorrespondenceCheckerBasedOnEdgeLength / PCL's SampleConsensusPrerejective: a rigid motion
//      keeps distances, so a sample whose scan-side and reference-side edges disagree (ea < sim eb or eb < sim ea for a pair) holds a
//      wrong match and is dropped before anybody scores it                                                     -> status 1
//   2. the Kabsch fit of the sample: centroids, centred cross-covariance H, R = argmax tr(R H) by Horn's quaternion form (horn4.h),
//      t = bbar - R abar.  gap = s2 + sign(det H) s3 <= 1e-6 s1 (H = 0, collinear samples, non-finite input) -> status 2
// The surviving transforms are compacted IN DRAW ORDER (count per block, scan of the block counts, scatter: no atomics decide a
// position), scored by K9 (sf_ransac_score, match.hip -- reused as it is) and reduced to the first maximum.
// k11_pair_sums are the two passes of a Kabsch fit over ALL inliers of one transform -- K9's inlier rule, centroids first, then the
// centred cross-covariance, block partials folded in a fixed order as icp.hip does for nearest-neighbour pairs -- whose 3x3 problem
// the caller solves on the host.
#include "common.h"
#include "device_util.h"
#include "horn4.h"
#include "match.h"
#include "ransac.h"

namespace {

constexpr int K11_MAX_DRAW = SF_RANSAC_MAX_DRAW_SIZE;
constexpr int K11_BLOCK = 256;       // draws per block of the compaction kernels
constexpr int K11_SUM_BLOCKS = 256;  // blocks of the pair sums (fixed: the fold order does not depend on m)
constexpr int K11_NV = 10;           // values per partial row (pass 0: 7, pass 1: 10)
constexpr int64_t K11_MAX_DRAWS = (int64_t)65535 * 8192; // K9's limit (match.hip)

__global__ __launch_bounds__(64) void k11_hypotheses(const double *__restrict__ a, const double *__restrict__ b, int64_t m,
                                                     const int64_t *__restrict__ draws, int64_t n_draws, int size, double sim,
                                                     unsigned char *__restrict__ status, double *__restrict__ Rt)
{
    const int64_t d = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (d >= n_draws) return;
    // the sample: arrays indexed by unrolled loop counters only (registers)
    double ax[K11_MAX_DRAW], ay[K11_MAX_DRAW], az[K11_MAX_DRAW], bx[K11_MAX_DRAW], by[K11_MAX_DRAW], bz[K11_MAX_DRAW];
    bool bad = false;
#pragma unroll
    for (int s = 0; s < K11_MAX_DRAW; ++s) {
        ax[s] = ay[s] = az[s] = bx[s] = by[s] = bz[s] = 0.0;
        if (s < size) {
            int64_t i = draws[d * size + s];
            if (i < 0 || i >= m) { bad = true; i = 0; } // never dereferenced out of range (m >= 1 here)
            ax[s] = a[3 * i]; ay[s] = a[3 * i + 1]; az[s] = a[3 * i + 2];
            bx[s] = b[3 * i]; by[s] = b[3 * i + 1]; bz[s] = b[3 * i + 2];
        }
    }
    bool pass = true;
#pragma unroll
    for (int i = 0; i < K11_MAX_DRAW; ++i)
#pragma unroll
        for (int j = i + 1; j < K11_MAX_DRAW; ++j)
            if (j < size) {
                const double ux = ax[i] - ax[j], uy = ay[i] - ay[j], uz = az[i] - az[j];
                const double vx = bx[i] - bx[j], vy = by[i] - by[j], vz = bz[i] - bz[j];
                const double ea = sqrt((ux * ux + uy * uy) + uz * uz), eb = sqrt((vx * vx + vy * vy) + vz * vz);
                pass &= (ea >= sim * eb) & (eb >= sim * ea);
            }
    unsigned char st = bad ? 3 : (pass ? 0 : 1);
    double o[12];
#pragma unroll
    for (int v = 0; v < 12; ++v) o[v] = 0.0;
    if (st == 0) {
        double ma0 = 0, ma1 = 0, ma2 = 0, mb0 = 0, mb1 = 0, mb2 = 0;
#pragma unroll
        for (int s = 0; s < K11_MAX_DRAW; ++s)
            if (s < size) { ma0 += ax[s]; ma1 += ay[s]; ma2 += az[s]; mb0 += bx[s]; mb1 += by[s]; mb2 += bz[s]; }
        const double n = (double)size;
        ma0 /= n; ma1 /= n; ma2 /= n; mb0 /= n; mb1 /= n; mb2 /= n;
        double h00 = 0, h01 = 0, h02 = 0, h10 = 0, h11 = 0, h12 = 0, h20 = 0, h21 = 0, h22 = 0;
#pragma unroll
        for (int s = 0; s < K11_MAX_DRAW; ++s)
            if (s < size) {
                const double px = ax[s] - ma0, py = ay[s] - ma1, pz = az[s] - ma2;
                const double qx = bx[s] - mb0, qy = by[s] - mb1, qz = bz[s] - mb2;
                h00 += px * qx; h01 += px * qy; h02 += px * qz;
                h10 += py * qx; h11 += py * qy; h12 += py * qz;
                h20 += pz * qx; h21 += pz * qy; h22 += pz * qz;
            }
        const double mean[6] = {ma0, ma1, ma2, mb0, mb1, mb2}, H[9] = {h00, h01, h02, h10, h11, h12, h20, h21, h22};
        if (!sf_horn::rigid_from_moments(mean, H, o)) st = 2;
    }
    status[d] = st;
#pragma unroll
    for (int v = 0; v < 12; ++v) Rt[12 * d + v] = o[v];
}

// survivors (status 0) per block of K11_BLOCK draws; tallies[1..3]: draws of status 1, 2, 3
__global__ __launch_bounds__(K11_BLOCK) void k11_count(const unsigned char *__restrict__ status, int64_t n_draws,
                                                       int *__restrict__ block_count, unsigned long long *__restrict__ tallies)
{
    __shared__ int c[4];
    if (threadIdx.x < 4) c[threadIdx.x] = 0;
    __syncthreads();
    const int64_t d = (int64_t)blockIdx.x * K11_BLOCK + threadIdx.x;
    const int st = d < n_draws ? (int)status[d] : -1;
    for (int v = 0; v < 4; ++v) {
        const int n = __popcll(__ballot(st == v));
        if ((threadIdx.x & 63) == 0 && n) atomicAdd(&c[v], n);
    }
    __syncthreads();
    if (threadIdx.x == 0) block_count[blockIdx.x] = c[0];
    if (threadIdx.x >= 1 && threadIdx.x < 4 && c[threadIdx.x]) atomicAdd(&tallies[threadIdx.x], (unsigned long long)c[threadIdx.x]);
}

// exclusive scan of the block counts by ONE block (a chunk of 256 per step, carried); tallies[0] = number of survivors
__global__ __launch_bounds__(256) void k11_scan(const int *__restrict__ block_count, int64_t nblocks, int64_t *__restrict__ block_off,
                                                unsigned long long *__restrict__ tallies)
{
    __shared__ int64_t sh[256];
    int64_t carry = 0;
    for (int64_t base = 0; base < nblocks; base += 256) {
        const int64_t i = base + threadIdx.x;
        const int64_t mine = i < nblocks ? block_count[i] : 0;
        sh[threadIdx.x] = mine;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {
            const int64_t add = threadIdx.x >= off ? sh[threadIdx.x - off] : 0;
            __syncthreads();
            sh[threadIdx.x] += add;
            __syncthreads();
        }
        if (i < nblocks) block_off[i] = carry + sh[threadIdx.x] - mine;
        carry += sh[255];
        __syncthreads();
    }
    if (threadIdx.x == 0) tallies[0] = (unsigned long long)carry;
}

// survivors to their slot, draw order kept: slot = block offset + survivors before this one in the block
__global__ __launch_bounds__(K11_BLOCK) void k11_scatter(const unsigned char *__restrict__ status, const double *__restrict__ Rt_all,
                                                         int64_t n_draws, const int64_t *__restrict__ block_off,
                                                         double *__restrict__ Rt_out, int64_t *__restrict__ map)
{
    __shared__ int wave_n[K11_BLOCK / 64];
    const int64_t d = (int64_t)blockIdx.x * K11_BLOCK + threadIdx.x;
    const bool keep = d < n_draws && status[d] == 0;
    const unsigned long long mask = __ballot(keep);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wave_n[wave] = __popcll(mask);
    __syncthreads();
    if (!keep) return;
    int before = __popcll(mask & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) before += wave_n[w];
    const int64_t slot = block_off[blockIdx.x] + before;
    map[slot] = d;
#pragma unroll
    for (int v = 0; v < 12; ++v) Rt_out[12 * slot + v] = Rt_all[12 * d + v];
}

// first maximum of counts[0..n): out = {slot, draw, count}, best_rt = that slot's transform.  One block.
__global__ __launch_bounds__(1024) void k11_argmax(const int64_t *__restrict__ counts, int64_t n, const int64_t *__restrict__ map,
                                                   const double *__restrict__ Rt, int64_t *__restrict__ out, double *__restrict__ best_rt)
{
    __shared__ int64_t sc[16], si[16];
    int64_t best = -1, bi = INT64_MAX;
    for (int64_t i = threadIdx.x; i < n; i += 1024) { // ascending per thread: strict > keeps its first maximum
        const int64_t c = counts[i];
        if (c > best) { best = c; bi = i; }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const int64_t c2 = __shfl_xor(best, off), i2 = __shfl_xor(bi, off);
        if (c2 > best || (c2 == best && i2 < bi)) { best = c2; bi = i2; }
    }
    if ((threadIdx.x & 63) == 0) { sc[threadIdx.x >> 6] = best; si[threadIdx.x >> 6] = bi; }
    __syncthreads();
    if (threadIdx.x < 64) {
        best = threadIdx.x < 16 ? sc[threadIdx.x] : -1;
        bi = threadIdx.x < 16 ? si[threadIdx.x] : INT64_MAX;
        for (int off = 8; off > 0; off >>= 1) {
            const int64_t c2 = __shfl_xor(best, off), i2 = __shfl_xor(bi, off);
            if (c2 > best || (c2 == best && i2 < bi)) { best = c2; bi = i2; }
        }
        best = __shfl(best, 0); bi = __shfl(bi, 0);
        const bool any = best >= 0;
        if (threadIdx.x == 0) { out[0] = any ? bi : -1; out[1] = any ? map[bi] : -1; out[2] = any ? best : 0; }
        if (threadIdx.x < 12) best_rt[threadIdx.x] = any ? Rt[12 * bi + threadIdx.x] : 0.0;
    }
}

// pass 0: inlier count, sum of inlier a, sum of inlier b.  pass 1: centred H = sum (a - abar)(b - bbar)^T (9), sum of squared residuals.
// The inliers are K9's: ((a R^T) + t) - b formed left to right, sqrt(s) <= thr decided through the band (sf_ransac_band).
template <int PASS>
__global__ __launch_bounds__(256) void k11_pair_sums(const double *__restrict__ a, const double *__restrict__ b, int64_t m,
                                                     const double *__restrict__ R, double thr, double lo, double hi,
                                                     const double *__restrict__ mean /* 6, pass 1 */, double *__restrict__ partial)
{
    constexpr int NV = PASS == 0 ? 7 : 10;
    __shared__ double sh[4][K11_NV];
    double acc[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[v] = 0.0;
    const double r0 = R[0], r1 = R[1], r2 = R[2], r3 = R[3], r4 = R[4], r5 = R[5], r6 = R[6], r7 = R[7], r8 = R[8];
    const double t0 = R[9], t1 = R[10], t2 = R[11];
    double mu[6] = {0, 0, 0, 0, 0, 0};
    if (PASS == 1) { mu[0] = mean[0]; mu[1] = mean[1]; mu[2] = mean[2]; mu[3] = mean[3]; mu[4] = mean[4]; mu[5] = mean[5]; }
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
        const double px = a[3 * i], py = a[3 * i + 1], pz = a[3 * i + 2];
        const double qx = b[3 * i], qy = b[3 * i + 1], qz = b[3 * i + 2];
        const double e0 = ((px * r0 + py * r1) + pz * r2) + t0 - qx;
        const double e1 = ((px * r3 + py * r4) + pz * r5) + t1 - qy;
        const double e2 = ((px * r6 + py * r7) + pz * r8) + t2 - qz;
        const double s = (e0 * e0 + e1 * e1) + e2 * e2;
        if (!(s <= lo || (s < hi && sqrt(s) <= thr))) continue;
        if (PASS == 0) {
            sf_refit_add_pair(acc, px, py, pz, qx, qy, qz);
        } else {
            sf_refit_add_centred(acc, mu, px, py, pz, qx, qy, qz);
            acc[NV - 1] += s;
        }
    }
    sf_block_sum4_stage(acc, sh);
    if (threadIdx.x < NV) partial[(size_t)blockIdx.x * K11_NV + threadIdx.x] = sf_block_sum4_at(sh, threadIdx.x);
}

// the block partials folded in block order into sums[24] (layout: sf_ransac_refit_sums); pass 0 also leaves the centroids
__global__ __launch_bounds__(64) void k11_sums_final(const double *__restrict__ partial, int nblocks, int pass, double *__restrict__ sums)
{
    const int v = threadIdx.x, nv = pass == 0 ? 7 : 10;
    double x = 0.0;
    if (v < nv)
        for (int blk = 0; blk < nblocks; ++blk) x += partial[(size_t)blk * K11_NV + v];
    const double cnt = __shfl(x, 0);
    if (pass == 0) {
        if (v == 0) { sums[RS_COUNT] = x; sums[RS_SPARE] = 0.0; }
        if (v >= 1 && v < 7) { sums[RS_SUM_A + v - 1] = x; sums[RS_ABAR + v - 1] = cnt > 0.0 ? x / cnt : 0.0; } // a, then b
    } else if (v < 10) {
        sums[RS_H + v] = x; // the nine of H, then RS_SSR
    }
}

int launch_hypotheses(sf_ctx *ctx, const char *who, const double *a, const double *b, int64_t m, const int64_t *draws,
                      int64_t n_draws, int draw_size, double sim, unsigned char *status, double *Rt)
{
    if (draw_size < SF_RANSAC_MIN_DRAW_SIZE || draw_size > SF_RANSAC_MAX_DRAW_SIZE) {
        sf_set_error("%s: draw_size %d outside %d .. %d", who, draw_size, SF_RANSAC_MIN_DRAW_SIZE, SF_RANSAC_MAX_DRAW_SIZE);
        return SF_ERR_UNSUPPORTED;
    }
    if (!(sim >= 0.0 && sim < 1.0)) { sf_set_error("%s: edge_similarity %g outside [0, 1)", who, sim); return SF_ERR_ARG; }
    if (n_draws > K11_MAX_DRAWS) { sf_set_error("%s: more than 65535 x 8192 draws", who); return SF_ERR_UNSUPPORTED; }
    if (n_draws && m < draw_size) { sf_set_error("%s: %lld matches, fewer than the draw size %d", who, (long long)m, draw_size); return SF_ERR_ARG; }
    if (!n_draws) return SF_OK;
    SF_LAUNCH(ctx, "k11_hypotheses", k11_hypotheses, dim3((unsigned)sf_div_up(n_draws, 64)), dim3(64), a, b, m, draws, n_draws,
              draw_size, sim, status, Rt);
    return SF_OK;
}

} // namespace

// ---- the back half of K11, for the other estimators that rank fitted transforms (K15, consistency.hip; ransac.h) -------------------
// The status-0 rows of Rt_all compacted in order into Rt_out, map[slot] = their position; tallies (4, zeroed here) <- the number of
// status 0 (after the scan), 1, 2, 3.  block_count / block_off: sf_k11_blocks(n) entries of scratch each.  Queued, no host wait.
int64_t sf_k11_blocks(int64_t n) { return std::max<int64_t>(sf_div_up(n, K11_BLOCK), 1); }

int sf_k11_compact(sf_ctx *ctx, const unsigned char *status, const double *Rt_all, int64_t n, double *Rt_out, int64_t *map,
                   int *block_count, int64_t *block_off, unsigned long long *tallies)
{
    const int64_t nblocks = sf_div_up(n, K11_BLOCK);
    SF_HIP(hipMemsetAsync(tallies, 0, 4 * sizeof(unsigned long long), ctx->stream));
    SF_LAUNCH(ctx, "k11_count", k11_count, dim3((unsigned)nblocks), dim3(K11_BLOCK), status, n, block_count, tallies);
    SF_LAUNCH(ctx, "k11_scan", k11_scan, dim3(1), dim3(256), (const int *)block_count, nblocks, block_off, tallies);
    SF_LAUNCH(ctx, "k11_scatter", k11_scatter, dim3((unsigned)nblocks), dim3(K11_BLOCK), status, Rt_all, n, (const int64_t *)block_off,
              Rt_out, map);
    return SF_OK;
}

// The first maximum of counts[0 .. n): win (3, device) <- {slot, map[slot], count} ({-1, -1, 0} when no count is >= 0), best_rt
// (12, device) <- that slot's row of Rt.  Queued, no host wait.
int sf_k11_first_max(sf_ctx *ctx, const int64_t *counts, int64_t n, const int64_t *map, const double *Rt, int64_t *win, double *best_rt)
{
    SF_LAUNCH(ctx, "k11_argmax", k11_argmax, dim3(1), dim3(1024), counts, n, map, Rt, win, best_rt);
    return SF_OK;
}

extern "C" int sf_ransac_hypotheses(sf_ctx *ctx, const double *a_dev, const double *b_dev, int64_t m, const int64_t *draws_dev,
                                    int64_t n_draws, int draw_size, double edge_similarity, unsigned char *status_dev,
                                    double *Rt_dev)
{
    if (!ctx || !a_dev || !b_dev || !draws_dev || !status_dev || !Rt_dev || m < 0 || n_draws < 0) {
        sf_set_error("sf_ransac_hypotheses: bad argument");
        return SF_ERR_ARG;
    }
    SF_HIP(hipSetDevice(ctx->device));
    return launch_hypotheses(ctx, "sf_ransac_hypotheses", a_dev, b_dev, m, draws_dev, n_draws, draw_size, edge_similarity,
                             status_dev, Rt_dev);
}

extern "C" int sf_ransac_refit_sums(sf_ctx *ctx, const double *a_dev, const double *b_dev, int64_t m, const double *Rt, double thr,
                                    double *sums)
{
    if (!ctx || !a_dev || !b_dev || !Rt || !sums || m < 0) { sf_set_error("sf_ransac_refit_sums: bad argument"); return SF_ERR_ARG; }
    SF_HIP(hipSetDevice(ctx->device));
    for (int i = 0; i < RS_SIZE; ++i) sums[i] = 0.0;
    if (!m) return SF_OK;
    sf_pool_guard tmp(ctx);
    double *dRt = nullptr, *partial = nullptr, *dsums = nullptr;
    SF_CHECK(tmp.alloc(&dRt, 12));
    SF_CHECK(tmp.alloc(&partial, (size_t)K11_SUM_BLOCKS * K11_NV));
    SF_CHECK(tmp.alloc(&dsums, RS_SIZE));
    SF_HIP(hipMemcpyAsync(dRt, Rt, 12 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    double lo, hi;
    sf_ransac_band(thr, &lo, &hi);
    const dim3 grid(K11_SUM_BLOCKS), block(256);
    SF_LAUNCH(ctx, "k11_pair_sums", k11_pair_sums<0>, grid, block, a_dev, b_dev, m, (const double *)dRt, thr, lo, hi,
              (const double *)nullptr, partial);
    SF_LAUNCH(ctx, "k11_sums_final", k11_sums_final, dim3(1), dim3(64), (const double *)partial, K11_SUM_BLOCKS, 0, dsums);
    SF_LAUNCH(ctx, "k11_pair_sums", k11_pair_sums<1>, grid, block, a_dev, b_dev, m, (const double *)dRt, thr, lo, hi,
              (const double *)(dsums + RS_ABAR), partial);
    SF_LAUNCH(ctx, "k11_sums_final", k11_sums_final, dim3(1), dim3(64), (const double *)partial, K11_SUM_BLOCKS, 1, dsums);
    SF_HIP(hipMemcpyAsync(sums, dsums, RS_SIZE * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    SF_HIP(hipStreamSynchronize(ctx->stream)); // Rt and sums are host buffers
    return SF_OK;
}

extern "C" int sf_ransac_prerejective(sf_ctx *ctx, const double *a_dev, const double *b_dev, int64_t m, const int64_t *draws_dev,
                                      int64_t n_draws, int draw_size, double edge_similarity, double thr,
                                      unsigned char *status_dev, double *Rt_dev, int64_t *map_dev, int64_t *counts_dev,
                                      int64_t *result, double *best_Rt)
{
    if (!ctx || !a_dev || !b_dev || !draws_dev || !result || !best_Rt || m < 0 || n_draws < 0) {
        sf_set_error("sf_ransac_prerejective: bad argument");
        return SF_ERR_ARG;
    }
    SF_HIP(hipSetDevice(ctx->device));
    for (int i = 0; i < 8; ++i) result[i] = 0;
    result[3] = result[5] = -1;
    for (int i = 0; i < 12; ++i) best_Rt[i] = 0.0;
    sf_pool_guard tmp(ctx);
    const size_t nd = (size_t)std::max<int64_t>(n_draws, 1);
    const int64_t nblocks = sf_div_up(n_draws, K11_BLOCK);
    double *Rt_all = nullptr, *dbest = nullptr;
    int *block_count = nullptr;
    int64_t *block_off = nullptr, *dwin = nullptr;
    unsigned long long *tallies = nullptr;
    if (!status_dev) SF_CHECK(tmp.alloc(&status_dev, nd));
    if (!Rt_dev) SF_CHECK(tmp.alloc(&Rt_dev, nd * 12));
    if (!map_dev) SF_CHECK(tmp.alloc(&map_dev, nd));
    if (!counts_dev) SF_CHECK(tmp.alloc(&counts_dev, nd));
    SF_CHECK(tmp.alloc(&Rt_all, nd * 12));
    SF_CHECK(tmp.alloc(&block_count, (size_t)std::max<int64_t>(nblocks, 1)));
    SF_CHECK(tmp.alloc(&block_off, (size_t)std::max<int64_t>(nblocks, 1)));
    SF_CHECK(tmp.alloc(&tallies, 4));
    SF_CHECK(tmp.alloc(&dwin, 4));
    SF_CHECK(tmp.alloc(&dbest, 12));
    SF_CHECK(launch_hypotheses(ctx, "sf_ransac_prerejective", a_dev, b_dev, m, draws_dev, n_draws, draw_size, edge_similarity,
                               status_dev, Rt_all));
    if (!n_draws) return SF_OK;
    SF_CHECK(sf_k11_compact(ctx, status_dev, Rt_all, n_draws, Rt_dev, map_dev, block_count, block_off, tallies));
    // the number of survivors sizes K9's launch: the one read-back between the two halves
    void *pin = nullptr;
    SF_CHECK(sf_ctx_pinned(ctx, &pin));
    unsigned long long *ht = (unsigned long long *)pin;
    SF_HIP(hipMemcpyAsync(ht, tallies, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    SF_HIP(hipStreamSynchronize(ctx->stream));
    const int64_t n_scored = (int64_t)ht[0], n_rej = (int64_t)ht[1], n_deg = (int64_t)ht[2], n_bad = (int64_t)ht[3];
    result[0] = n_rej; result[1] = n_deg; result[2] = n_scored; result[6] = n_bad;
    if (n_bad) {
        sf_set_error("sf_ransac_prerejective: %lld draws name a match outside [0, %lld)", (long long)n_bad, (long long)m);
        return SF_ERR_ARG;
    }
    if (!n_scored) return SF_OK;
    SF_CHECK(sf_ransac_score(ctx, a_dev, b_dev, m, Rt_dev, n_scored, thr, counts_dev, SF_IN_DEVICE | SF_OUT_DEVICE));
    SF_CHECK(sf_k11_first_max(ctx, counts_dev, n_scored, map_dev, Rt_dev, dwin, dbest));
    int64_t *hw = (int64_t *)pin;
    double *hb = (double *)((char *)pin + 64);
    SF_HIP(hipMemcpyAsync(hw, dwin, 3 * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    SF_HIP(hipMemcpyAsync(hb, dbest, 12 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    SF_HIP(hipStreamSynchronize(ctx->stream));
    result[5] = hw[0]; result[3] = hw[1]; result[4] = hw[2];
    memcpy(best_Rt, hb, 12 * sizeof(double));
    return SF_OK;
}
