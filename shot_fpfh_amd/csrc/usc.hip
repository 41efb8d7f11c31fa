// usc.hip -- K21: Unique Shape Context (Tombari, Salti, Di Stefano 2010; pcl::UniqueShapeContext), the 3-D shape context in
// SHOT's local reference frame: per keypoint a histogram over L azimuth x K elevation x J log-radial bins of its neighbours'
// offsets in the frame K4 computes, every neighbour weighted by 1 / (points within density_radius of it) and every bin by
// 1 / cbrt(its volume).  Rows of D = L K J <= SF_USC_MAX_BINS doubles, bin (l, k, j) at (l K + k) J + j.  No normals.
// The definition -- decided here, modelled on PCL -- is tests/usc_numpy.py: bins by comparisons against tables computed once on
// the host (sf_usc_tables), never by a transcendental function in the kernel; arithmetic unfused, in the statement's order.
//
// Mapping: the streaming shape of k_shot_bins.  One wave per keypoint, the list in steps of 128 (shot_list_entry /
// shot_gather_entry), any length.  A wave owns 16 B of LDS per bin: the two integer limbs of usc_acc.h, each receiving one
// 64-bit LDS integer atomic add per neighbour, so the sum of a bin is exact whatever the order of the adds, and the read-out
// rounds it once: row[b] = fsum(weights of the bin) vol[b], every bit a function of the cloud alone.  The wave's LDS phases are
// ordered by SF_SHOT_SYNC (no workgroup barrier: the waves of a workgroup are independent); the waves per workgroup follow from
// D (usc_waves).  The bin tables (J + 1 + L + K + 1 doubles) are read at wave-uniform addresses through the scalar cache: one
// load serves the 128 neighbours of a step, and a comparison takes the edge as its scalar operand -- a linear count is 2
// (radial), 3 (elevation) and 5 (azimuth) vector instructions per edge and neighbour.  vol is read per bin at the read-out.
// One sweep: the gate (neighbours at non-zero distance) is counted in the sweep that accumulates, a failed gate writes zeros.
// HBM roofline, algorithmic bytes per keypoint: the 8 D B row (15 680 B at the defaults: the floor), 24 B keypoint + 72 B
// frame, and per list entry 4 B index + 48 B record + 8 B weight (the records and weights of a resident cloud come from L2).
//
// The density weights are a pass of their own (sf_usc_weights): K2's count sweep on the grid built for density_radius
// (outliers.hip's route), then w = 1.0 / (double)count, one correctly rounded division, in the caller's order.  It REBUILDS the
// grid, so it runs before the search whose lists sf_usc is given; sf_usc brings the weights into the current grid's order.
#include "common.h"
#include "device_util.h"
#include "host_stage.h"
#include "search_util.h"
#include "shot_core.h"
#include "usc_acc.h"

#include <cmath>

namespace {

// where the tables start in the one array a launch is given: e2[J + 1] | ca[L / 2] | sa[L / 2] | q[K + 1] | vol[D]
struct usc_shape {
    int L2, K, J, D; // L2 = L / 2
    __host__ __device__ int at_ca() const { return J + 1; }
    __host__ __device__ int at_sa() const { return J + 1 + L2; }
    __host__ __device__ int at_q() const { return J + 1 + 2 * L2; }
    __host__ __device__ int at_vol() const { return J + 1 + 2 * L2 + K + 1; }
    __host__ __device__ int size() const { return at_vol() + D; }
};

// One wave per keypoint, blockDim.x / 64 waves per workgroup, each with its own 2 x D limbs of the dynamic LDS.
// lrf: finished frames (m x 9, by caller row); w: the density weights by cell-sorted position; err: set to 1 (a plain store)
// by a weight outside [2^-22, 1] or a list of 2^24 entries or more.
__global__ __launch_bounds__(256) void k_usc(const double *__restrict__ rec, const double *__restrict__ qx,
                                             const double *__restrict__ qy, const double *__restrict__ qz,
                                             const int64_t *__restrict__ offset, const int32_t *__restrict__ cnt,
                                             const int32_t *__restrict__ idx, const int32_t *__restrict__ qrow, int64_t m,
                                             const double *__restrict__ lrf, const double *__restrict__ w,
                                             const double *__restrict__ tab_, usc_shape S, int normalize, int min_nb,
                                             double *__restrict__ out, int *__restrict__ err)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long usc_lds[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nw = blockDim.x >> 6;
    const int D = S.D;
    unsigned long long *const acc_lo = usc_lds + (size_t)2 * D * wave;
    unsigned long long *const acc_hi = acc_lo + D;
    const int64_t q = sf_xcd_block() * nw + wave;
    if (q >= m) return;
    const int64_t s = offset[q];
    const int k = sf_uniform(cnt[q]);
    const int64_t row = qrow ? qrow[q] : q;
    double *o = out + (int64_t)D * row;
    const double px = qx[q], py = qy[q], pz = qz[q];
    for (int b = lane; b < 2 * D; b += 64) acc_lo[b] = 0ull;
    double E[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) E[i] = lrf[9 * row + i];
    const sf_const_doubles tab = (sf_const_doubles)tab_;
    SF_SHOT_SYNC(); // (the cleared limbs)

    int npos = 0;
    const int steps_end = k < USC_ACC_MAX_LIST ? k : 0; // (a list that could overflow a limb is not walked)
    bool bad = k >= USC_ACC_MAX_LIST;
    for (int t0 = 0; t0 < steps_end; t0 += 128) {
        double cx[2], cy[2], cz[2], nx, ny, nz, r2[2], lx[2], ly[2], lz[2], u_[2], v_[2], zz[2], wt[2];
        int jj[2], bj[2], bl[2], bk[2];
        bool at[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) jj[u] = shot_list_entry<true>(idx + s, t0 + 64 * u + lane, k); // (both indices before a record)
#pragma unroll
        for (int u = 0; u < 2; ++u) wt[u] = w[jj[u] < 0 ? 0 : jj[u]]; // (requested with the records, used after the bins)
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const bool on = shot_gather_entry(rec, jj[u], px, py, pz, cx[u], cy[u], cz[u], nx, ny, nz);
            r2[u] = (cx[u] * cx[u] + cy[u] * cy[u]) + cz[u] * cz[u];
            at[u] = on && r2[u] > 0.0; // (the keypoint itself and its exact duplicates take no part)
            lx[u] = (cx[u] * E[0] + cy[u] * E[3]) + cz[u] * E[6];
            ly[u] = (cx[u] * E[1] + cy[u] * E[4]) + cz[u] * E[7];
            lz[u] = (cx[u] * E[2] + cy[u] * E[5]) + cz[u] * E[8];
            // azimuth: the half turn the point lies in, then its offset (u, v) turned into the upper one
            const bool h = ly[u] < 0.0 || (ly[u] == 0.0 && lx[u] < 0.0);
            u_[u] = h ? -lx[u] : lx[u];
            v_[u] = h ? -ly[u] : ly[u];
            zz[u] = lz[u] * fabs(lz[u]);
            bj[u] = 0;
            bl[u] = h ? S.L2 : 0;
            bk[u] = 0;
        }
        // (unrolled by four: the four edges of a round arrive by one scalar load instead of four dependent ones)
#pragma unroll 4
        for (int i = 1; i < S.J; ++i) { // radial: j = #{1 <= i < J : r2 >= e2[i]}
            const double e2 = tab[i];
#pragma unroll
            for (int u = 0; u < 2; ++u) bj[u] += r2[u] >= e2 ? 1 : 0;
        }
#pragma unroll 4
        for (int i = 1; i < S.L2; ++i) { // azimuth: l = #{1 <= i < L / 2 : ca[i] v - sa[i] u >= 0} + h L / 2
            const double ca = tab[S.at_ca() + i], sa = tab[S.at_sa() + i];
#pragma unroll
            for (int u = 0; u < 2; ++u) bl[u] += ca * v_[u] - sa * u_[u] >= 0.0 ? 1 : 0;
        }
#pragma unroll 4
        for (int i = 1; i < S.K; ++i) { // elevation: k = #{1 <= i < K : lz |lz| <= q[i] r2}
            const double qi = tab[S.at_q() + i];
#pragma unroll
            for (int u = 0; u < 2; ++u) bk[u] += zz[u] <= qi * r2[u] ? 1 : 0;
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            npos += __popcll(__ballot(at[u]));
            if (at[u]) {
                unsigned long long lo, hi;
                if (usc_acc_split(wt[u], lo, hi)) {
                    const int b = (bl[u] * S.K + bk[u]) * S.J + bj[u]; // (every count stays below its bound: b < D)
                    atomicAdd(&acc_lo[b], lo);
                    atomicAdd(&acc_hi[b], hi);
                } else {
                    bad = true;
                }
            }
        }
    }
    if (__ballot(bad)) {
        if (bad) *err = 1;
        npos = -1; // (the call fails: the row is not used)
    }
    if (!(npos > min_nb)) { // (min_nb arrives clamped into [-1, 2^31 - 1])
        for (int b = lane; b < D; b += 64) sf_store_stream(o + b, 0.0);
        return;
    }
    SF_SHOT_SYNC();

    // ---- the row: the limbs of a bin rounded once, times vol[b]; stored at once, or (normalize) kept in the lo limbs the lane
    // has read until the norm is known ----
    // Eight bins per lane and round: their vol loads and limb reads are requested together, in straight-line code, before the
    // first rounding (which branches) -- 16 B of LDS per bin leave one wave per SIMD, which hides no latency by itself.
    double ss = 0.0;
    for (int b0 = lane; b0 < D; b0 += 64 * 8) {
        double vv[8];
        unsigned long long lo[8], hi[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int b = b0 + 64 * u < D ? b0 + 64 * u : lane; // (past the end: the lane's first bin, read and dropped)
            vv[u] = tab_[S.at_vol() + b];
            lo[u] = acc_lo[b];
            hi[u] = acc_hi[b];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int b = b0 + 64 * u;
            if (b < D) {
                const double v = usc_acc_round(lo[u], hi[u]) * vv[u];
                if (normalize) { // (wave-uniform) the value waits in the lo limb for the norm
                    acc_lo[b] = (unsigned long long)__double_as_longlong(v);
                    ss += v * v;
                } else {
                    sf_store_stream(o + b, v);
                }
            }
        }
    }
    if (!normalize) return;
    const double scale = shot_row_scale(ss, 1, false);
#pragma unroll 8
    for (int b = lane; b < D; b += 64) sf_store_stream(o + b, __longlong_as_double((long long)acc_lo[b]) * scale);
}

struct reciprocal { // a ball size -> its density weight
    __host__ __device__ double operator()(int32_t count) const { return 1.0 / (double)count; }
};

// Waves per workgroup for rows of D bins: as many as keep the workgroup's LDS within 64 KiB (4 up to 1024, 2 up to 2048, 1 above).
int usc_waves(int D) { return D <= 1024 ? 4 : (D <= 2048 ? 2 : 1); }

int usc_check_shape(const char *who, double radius, double min_radius, int64_t L, int64_t K, int64_t J)
{
    SF_CHECK(sf_check_radius(who, "radius", radius));
    if (!(min_radius > 0.0) || !(min_radius < radius)) {
        sf_set_error("%s: min_radius must lie strictly between 0 and the radius %g (got %g)", who, radius, min_radius);
        return SF_ERR_ARG;
    }
    if (L < 2 || (L & 1)) { sf_set_error("%s: azimuth_bins must be even and at least 2 (got %lld)", who, (long long)L); return SF_ERR_ARG; }
    if (K < 1) { sf_set_error("%s: elevation_bins must be at least 1 (got %lld)", who, (long long)K); return SF_ERR_ARG; }
    if (J < 1) { sf_set_error("%s: radius_bins must be at least 1 (got %lld)", who, (long long)J); return SF_ERR_ARG; }
    if (L > SF_USC_MAX_BINS || K > SF_USC_MAX_BINS || J > SF_USC_MAX_BINS || L * K * J > SF_USC_MAX_BINS) {
        sf_set_error("%s: %lld x %lld x %lld bins make rows longer than %d", who, (long long)L, (long long)K, (long long)J, SF_USC_MAX_BINS);
        return SF_ERR_ARG;
    }
    return SF_OK;
}

} // namespace

// The tables of a bin shape, on the host: e2[J + 1], ca[L / 2], sa[L / 2], q[K + 1], vol[L K J].
extern "C" int sf_usc_tables(double radius, double min_radius, int64_t L_, int64_t K_, int64_t J_, double *e2, double *ca, double *sa,
                             double *q, double *vol)
{
    SF_CHECK(usc_check_shape("sf_usc_tables", radius, min_radius, L_, K_, J_));
    if (!e2 || !ca || !sa || !q || !vol) { sf_set_error("sf_usc_tables: null output"); return SF_ERR_ARG; }
    const int L = (int)L_, K = (int)K_, J = (int)J_;
    const double pi = 3.141592653589793;
    std::vector<double> e((size_t)J + 1), ct((size_t)K + 1);
    // every function value through the extended-precision libm, rounded once: the double ones are up to a few ulp off, and
    // the shell volumes below amplify an ulp of e several times
    const double l0 = (double)logl(min_radius), lr = (double)logl(radius / min_radius);
    for (int j = 0; j <= J; ++j) e[j] = (double)expl(l0 + ((double)j / (double)J) * lr);
    e[0] = min_radius;
    e[J] = radius;
    for (int j = 0; j <= J; ++j) e2[j] = e[j] * e[j];
    for (int i = 0; i < L / 2; ++i) {
        const double a = 2.0 * pi * (double)i / (double)L;
        ca[i] = (double)cosl(a);
        sa[i] = (double)sinl(a);
    }
    for (int i = 0; i <= K; ++i) ct[i] = (double)cosl(pi * (double)i / (double)K);
    ct[0] = 1.0;
    ct[K] = -1.0;
    if (K % 2 == 0) ct[K / 2] = 0.0;
    for (int i = 0; i <= K; ++i) q[i] = ct[i] * fabs(ct[i]);
    for (int l = 0; l < L; ++l)
        for (int k = 0; k < K; ++k)
            for (int j = 0; j < J; ++j) {
                const double shell = e[j + 1] * e[j + 1] * e[j + 1] - e[j] * e[j] * e[j];
                const long double cell = (2.0 * pi / (double)L) * (ct[k] - ct[k + 1]) * shell / 3.0;
                vol[((size_t)l * K + k) * J + j] = (double)(1.0L / cbrtl(cell));
            }
    return SF_OK;
}

// w[i] = 1.0 / (number of cloud points within density_radius of point i, itself included), n doubles in the caller's order.
extern "C" int sf_usc_weights(sf_ctx *ctx, sf_cloud *c, double density_radius, double *weight, int flags)
{
    if (!ctx || !c || !weight) { sf_set_error("sf_usc_weights: null argument"); return SF_ERR_ARG; }
    SF_CHECK(sf_check_radius("sf_usc_weights", "density_radius", density_radius));
    SF_HIP(hipSetDevice(ctx->device));
    const int64_t n = c->n;
    if (!n) return SF_OK;
    sf_pool_guard tmp(ctx);
    int32_t *sorted = nullptr;
    double *dw;
    SF_CHECK(sf_k2_ball_sizes(ctx, c, tmp, density_radius, "k21_ball_count", &sorted));
    SF_CHECK(stage_out(tmp, weight, (size_t)n, flags, &dw));
    SF_CHECK(sf_perm_scatter(ctx, "k21_weights", c, (const int32_t *)sorted, dw, reciprocal())); // (cell-sorted counts -> w = 1 / count, caller order)
    SF_CHECK(finish_out(ctx, weight, (size_t)n, flags, dw));
    return stage_sync_out(ctx, flags);
}

extern "C" int sf_usc(sf_ctx *ctx, sf_cloud *c, sf_nbrs *nb, const double *lrf, const double *weight, double min_radius,
                      int64_t L, int64_t K, int64_t J, int normalize, int64_t min_nb, double *out, int flags)
{
    SF_CHECK(check_nbrs(ctx, c, nb, "sf_usc"));
    if (!weight || !out) { sf_set_error("sf_usc: null %s", weight ? "out" : "weight"); return SF_ERR_ARG; }
    SF_CHECK(usc_check_shape("sf_usc", nb->radius, min_radius, L, K, J));
    if (!(c->pop_begin == 0 && c->pop_end == c->n)) { sf_set_error("sf_usc: needs the whole cloud's grid, not a block of it"); return SF_ERR_UNSUPPORTED; }
    const usc_shape S{(int)L / 2, (int)K, (int)J, (int)(L * K * J)};
    const int64_t m = nb->m, n = c->n;
    std::vector<double> htab((size_t)S.size());
    SF_CHECK(sf_usc_tables(nb->radius, min_radius, L, K, J, &htab[0], &htab[S.at_ca()], &htab[S.at_sa()], &htab[S.at_q()], &htab[S.at_vol()]));
    sf_pool_guard guard(ctx);
    const double *dlrf_in, *dw_in;
    double *dlrf = nullptr, *dws = nullptr, *dtab = nullptr, *dout;
    int *derr = nullptr;
    SF_CHECK(stage_in(guard, lrf, (size_t)m * 9, flags, &dlrf_in));
    SF_CHECK(stage_in(guard, weight, (size_t)n, flags, &dw_in));
    SF_CHECK(guard.alloc(&dws, (size_t)n));
    SF_CHECK(guard.alloc(&dtab, htab.size()));
    SF_CHECK(guard.alloc(&derr, 1));
    SF_CHECK(stage_out(guard, out, (size_t)m * S.D, flags, &dout));
    SF_HIP(hipMemsetAsync(derr, 0, sizeof(int), ctx->stream));
    SF_HIP(hipMemcpyAsync(dtab, htab.data(), htab.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (!dlrf_in) { // K4 on these lists, as sf_shot_lrf runs it
        SF_CHECK(guard.alloc(&dlrf, (size_t)m * 9));
        SF_CHECK(sf_launch_shot_lrf(ctx, c, nb, 0, 0, dlrf));
        dlrf_in = dlrf;
    }
    if (n) SF_CHECK(sf_perm_gather(ctx, "k21_sort_weights", c, dw_in, 0, dws));
    int nmin = (int)std::min<int64_t>(std::max<int64_t>(min_nb, -1), 2147483647LL);
    if (m) {
        const int wv = usc_waves(S.D);
        const size_t lds = (size_t)wv * 2 * S.D * sizeof(unsigned long long);
        sf_launch_timer t_(ctx, "k21_usc");
        hipLaunchKernelGGL(k_usc, dim3(sf_xcd_grid(sf_div_up(m, wv))), dim3(64 * wv), lds, ctx->stream, (const double *)c->rec,
                           (const double *)nb->qx, (const double *)nb->qy, (const double *)nb->qz, (const int64_t *)nb->offset,
                           (const int32_t *)nb->count, (const int32_t *)nb->idx, (const int32_t *)nb->qrow, m, dlrf_in,
                           (const double *)dws, (const double *)dtab, S, normalize, nmin, dout, derr);
        SF_HIP(hipGetLastError());
    }
    SF_CHECK(finish_out(ctx, out, (size_t)m * S.D, flags, dout));
    void *pin = nullptr; // (the table upload reads htab until the stream has passed it: the call always waits)
    SF_CHECK(sf_ctx_pinned(ctx, &pin));
    SF_HIP(hipMemcpyAsync(pin, derr, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    SF_HIP(hipStreamSynchronize(ctx->stream));
    if (*(const int *)pin) {
        sf_set_error("sf_usc: a density weight outside [2^-22, 1] (not 1 / count of a ball of fewer than 2^22 points), or a list of "
                     "2^24 entries or more");
        return SF_ERR_ARG;
    }
    return SF_OK;
}
