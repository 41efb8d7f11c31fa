// iss.hip -- K10: ISS keypoints (Intrinsic Shape Signatures, Zhong 2009; the rule PCL's and Open3D's detectors are documented
// with), the one stage of the pipeline the reference has no counterpart of.
//
//   saliency[i] = e3 of the covariance of the ball B(i, r_s) (eigenvalues e1 >= e2 >= e3), or -1 when the ball has fewer than
//                 min_neighbors points, e2 / e1 >= gamma_21, e3 / e2 >= gamma_32, e1 <= 0, e2 <= 0 or e3 <= 1e-12 e1;
//   keypoint i  <=> saliency[i] > 0, |B(i, r_n)| >= min_neighbors, and no j in B(i, r_n) has saliency[j] > saliency[i].
//
// Mapping: the covariances are K2 + K3's fused sweep (search.hip::k_radius_cov, unchanged, with its count output switched on);
// k_iss_saliency is one eigen-solve per lane on top (eigh3.h; K4's note on one-thread solves applies, the stage is small);
// k_iss_nms is the K2 family's candidate sweep (search_util.h) -- four queries per wave, run tables per 16-lane row, candidate
// pairs, the conservative x window -- that reads the candidates' saliency next to their coordinates (a fourth coalesced
// 16-byte load: the array sits in the cell-sorted order of xs / ys / zs) and keeps two wave-wide facts per query, the hit count
// and "some hit is strictly larger".  No lists, no LDS ring: one int32 flag per point leaves the kernel.
// What bounds it: the saliency pass is k_radius_cov (issue-bound sweep) + 1M eigen-solves; the suppression is the sweep of
// K2's count pass with one more load per step and an early exit at the first larger hit.
//
// Orders.  Between the two passes the saliency lives in the CALLER's point order: a grid is kept or rebuilt per radius
// (cell in [r, 2 r]) and a rebuild changes the cell-sorted order, so each pass maps through the perm of the grid it runs on.
// The saliency pass always runs on the grid sf_cloud_build_grid makes for r_s itself -- the order of a covariance's sums
// follows the cell-sorted order, and points with equal neighbour sets differ by that rounding alone, so the keypoints of a
// cloud must not depend on which radius it happened to be searched with before.  The suppression compares stored values and
// tests exact ball membership: it gives the same flags on any valid grid and takes whichever is there.
#include <cmath>

#include "eigh3.h"
#include "host_stage.h"
#include "search_util.h"

namespace {

#define SF_ISS_FLOOR 1e-12 // e3 > SF_ISS_FLOOR * e1: a float64 covariance of k <= 1e4 points carries ~k 2^-53 e1 of rounding

// One lane per cell-sorted position: eigenvalues of the covariance k_radius_cov left (c11 c21 c31 c22 c32 c33), the rule
// above, the result scattered to the caller's numbering.
__global__ __launch_bounds__(64) void k_iss_saliency(const double *__restrict__ cov, const int32_t *__restrict__ cnt,
                                                     const int32_t *__restrict__ perm, int64_t n, double gamma_21, double gamma_32,
                                                     int min_neighbors, double *__restrict__ saliency, int32_t *__restrict__ count)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double *c = cov + 6 * i;
    const sf_eig::eig3 e = sf_eig::eigh3_lower(c[0], c[1], c[2], c[3], c[4], c[5]);
    const double e1 = e.w3, e2 = e.w2, e3 = e.w1;
    const int k = cnt[i];
    const bool salient = k >= min_neighbors && e1 > 0.0 && e2 > 0.0 && e2 / e1 < gamma_21 && e3 / e2 < gamma_32 && e3 > SF_ISS_FLOOR * e1;
    const int64_t o = perm[i];
    saliency[o] = salient ? e3 : -1.0;
    if (count) count[o] = k;
}

#ifndef SF_ISS_WPB
#define SF_ISS_WPB 8 // waves per workgroup, four queries each (K2's shape)
#endif

// Non-maximum suppression of `sal` (cell-sorted order) over the ball of squared radius r2 around every cloud point.
// flag[perm[q]] = 1 <=> sal[q] > 0, at least min_neighbors points in the ball (q included), none of them with a larger value.
__global__ __launch_bounds__(64 * SF_ISS_WPB) void k_iss_nms(sf_grid_desc g, const int32_t *__restrict__ cell_start,
                                                             const double *__restrict__ xs, const double *__restrict__ ys,
                                                             const double *__restrict__ zs, const double *__restrict__ sal,
                                                             const int32_t *__restrict__ perm, int64_t m, double r2,
                                                             int min_neighbors, int32_t *__restrict__ flag)
{
    const int lane = threadIdx.x & 63, sl = lane & 15, rw = lane >> 4;
    const int64_t q0 = sf_uniform64((sf_xcd_block() * SF_ISS_WPB + (threadIdx.x >> 6)) * 4);
    if (q0 >= m) return;
    const int nq = (int)(m - q0 < 4 ? m - q0 : 4);
    const int64_t qm = q0 + (rw < nq ? rw : 0);
    const double pxv = xs[qm], pyv = ys[qm], pzv = zs[qm], sv = sal[qm]; // this row's query
    int y0, y1, z0, z1;
    stencil_bounds(pyv, g.lo[1], g.inv_cell, g.dim[1], y0, y1);
    stencil_bounds(pzv, g.lo[2], g.inv_cell, g.dim[2], z0, z1);
    __shared__ int4 runs[SF_ISS_WPB][4][12];
    int4(*const tabs)[12] = runs[threadIdx.x >> 6];
    int s, e; // (the run tables of the four queries, all of them whatever their saliency)
    sf_k2_window(g, cell_start, pxv, pyv, pzv, r2, sl, rw < nq, y0, y1, z0, z1, s, e);
    const int first_slot = sf_k2_store_runs(s, e, sl, tabs[rw]);
    __builtin_amdgcn_wave_barrier(); // the tables are written and read by this wave only
    for (int qi = 0; qi < nq; ++qi) {
        const int64_t q = q0 + qi;
        // the query's own value as a scalar: a point that is not salient is no keypoint whatever surrounds it, and the whole
        // wave skips its sweep together (no lane reads a run table under a divergent mask)
        const double sq = sf_read_lane(sv, 16 * qi);
        int keep = 0;
        if (sq > 0.0) {
            const int4 *const tab = tabs[qi];
            const double px = sf_read_lane(pxv, 16 * qi), py = sf_read_lane(pyv, 16 * qi), pz = sf_read_lane(pzv, 16 * qi);
            const int b4 = __shfl(first_slot, 16 * qi + 4), b8 = __shfl(first_slot, 16 * qi + 8);
            const int nslots = sf_uniform(__shfl(first_slot, 16 * qi + 9));
            int total = 0;
            bool larger = false;
            for (int f0 = 0; f0 < nslots; f0 += 64) {
                const sf_k2_pair c = sf_k2_load_pair(tab, b4, b8, nslots, f0 + lane, xs, ys, zs);
                const double2 S = *reinterpret_cast<const double2 *>(sal + c.j);
                const double dxa = c.X.x - px, dya = c.Y.x - py, dza = c.Z.x - pz;
                const double dxb = c.X.y - px, dyb = c.Y.y - py, dzb = c.Z.y - pz;
                const double d2a = (dxa * dxa + dya * dya) + dza * dza, d2b = (dxb * dxb + dyb * dyb) + dzb * dzb;
                const bool hit0 = c.in0 & (d2a <= r2);
                const bool hit1 = c.in1 & (d2b <= r2);
                total += __popcll(__ballot(hit0)) + __popcll(__ballot(hit1));
                if (__ballot((hit0 & (S.x > sq)) | (hit1 & (S.y > sq)))) { larger = true; break; } // (wave-uniform)
            }
            keep = !larger && total >= min_neighbors;
        }
        if (lane == 0) flag[perm[q]] = keep;
    }
}

struct flag_set {
    const int32_t *flag;
    __host__ __device__ bool operator()(int64_t i) const { return flag[i] != 0; }
};

int check_rule(const char *who, double gamma_21, double gamma_32, int min_neighbors)
{
    if (!(gamma_21 > 0.0 && gamma_21 <= 1.0) || !(gamma_32 > 0.0 && gamma_32 <= 1.0)) {
        sf_set_error("%s: gamma_21 and gamma_32 must lie in (0, 1] (got %g, %g)", who, gamma_21, gamma_32);
        return SF_ERR_ARG;
    }
    if (min_neighbors < 1) { sf_set_error("%s: min_neighbors must be at least 1 (got %d)", who, min_neighbors); return SF_ERR_ARG; }
    return SF_OK;
}

// saliency (and counts, nullable) of every point in the caller's order, device pointers
int saliency_dev(sf_ctx *ctx, sf_cloud *c, double radius, double gamma_21, double gamma_32, int min_neighbors, double *saliency,
                 int32_t *count)
{
    const int64_t n = c->n;
    if (!n) return SF_OK;
    SF_CHECK(sf_k2_own_grid(ctx, c, radius)); // (see "Orders" above)
    sf_pool_guard tmp(ctx);
    double *cov = nullptr;
    int32_t *cnt = nullptr;
    SF_CHECK(tmp.alloc(&cov, (size_t)n * 6));
    SF_CHECK(tmp.alloc(&cnt, (size_t)n));
    SF_CHECK(sf_k2_radius_cov_self(ctx, c, radius, "k10_iss_cov", cov, cnt));
    SF_LAUNCH(ctx, "k10_iss_saliency", k_iss_saliency, dim3((unsigned)sf_div_up(n, 64)), dim3(64), (const double *)cov,
              (const int32_t *)cnt, (const int32_t *)c->perm, n, gamma_21, gamma_32, min_neighbors, saliency, count);
    return SF_OK;
}

} // namespace

// the selected points of a score in the caller's order (device), ascending, and their number (device word *dnum)
int sf_k10_select_dev(sf_ctx *ctx, sf_cloud *c, const double *score, double radius, int min_neighbors, int64_t *selected, size_t *dnum)
{
    const int64_t n = c->n;
    SF_CHECK(sf_k2_ensure_grid(ctx, c, radius));
    sf_pool_guard tmp(ctx);
    double *sorted = nullptr;
    int32_t *flag = nullptr;
    SF_CHECK(tmp.alloc(&sorted, (size_t)n + 2));
    SF_CHECK(tmp.alloc(&flag, (size_t)n));
    SF_CHECK(sf_perm_gather(ctx, "k10_iss_gather", c, score, 2, sorted)); // (+ the two elements the pair loads may touch past the end)
    const sf_grid_desc g = sf_make_grid_desc(c);
    SF_LAUNCH(ctx, "k10_iss_nms", k_iss_nms, dim3(sf_xcd_grid(sf_div_up(n, 4 * SF_ISS_WPB))), dim3(64 * SF_ISS_WPB), g,
              (const int32_t *)c->cell_start, (const double *)c->xs, (const double *)c->ys, (const double *)c->zs, (const double *)sorted,
              (const int32_t *)c->perm, n, radius * radius, min_neighbors, flag);
    return sf_select_indices(ctx, tmp, "k10_iss_compact", n, flag_set{flag}, selected, dnum);
}

// the tail of both selecting entry points: the count to the host (one read-back), then the indices if the host wants them
int sf_k10_finish_selection(sf_ctx *ctx, const size_t *dnum, const int64_t *dsel, int64_t *selected, int64_t *n_selected, int flags)
{
    void *pin = nullptr;
    SF_CHECK(sf_ctx_pinned(ctx, &pin));
    SF_HIP(hipMemcpyAsync(pin, dnum, sizeof(size_t), hipMemcpyDeviceToHost, ctx->stream));
    SF_HIP(hipStreamSynchronize(ctx->stream));
    const size_t k = *(const size_t *)pin;
    *n_selected = (int64_t)k;
    if (!(flags & SF_OUT_DEVICE) && k) {
        SF_HIP(hipMemcpyAsync(selected, dsel, k * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
        SF_HIP(hipStreamSynchronize(ctx->stream));
    }
    return SF_OK;
}

extern "C" int sf_iss_saliency(sf_ctx *ctx, sf_cloud *c, double salient_radius, double gamma_21, double gamma_32, int min_neighbors,
                               double *saliency, int32_t *count, int flags)
{
    if (!ctx || !c || !saliency) { sf_set_error("sf_iss_saliency: null argument"); return SF_ERR_ARG; }
    SF_CHECK(sf_check_radius("sf_iss_saliency", "salient_radius", salient_radius));
    SF_CHECK(check_rule("sf_iss_saliency", gamma_21, gamma_32, min_neighbors));
    SF_HIP(hipSetDevice(ctx->device));
    const int64_t n = c->n;
    if (!n) return SF_OK;
    sf_pool_guard tmp(ctx);
    double *dsal = nullptr;
    int32_t *dcnt = nullptr;
    SF_CHECK(stage_out(tmp, saliency, (size_t)n, flags, &dsal));
    if (count) SF_CHECK(stage_out(tmp, count, (size_t)n, flags, &dcnt));
    SF_CHECK(saliency_dev(ctx, c, salient_radius, gamma_21, gamma_32, min_neighbors, dsal, dcnt));
    SF_CHECK(finish_out(ctx, saliency, (size_t)n, flags, dsal));
    if (count) SF_CHECK(finish_out(ctx, count, (size_t)n, flags, dcnt));
    return stage_sync_out(ctx, flags);
}

extern "C" int sf_iss_select(sf_ctx *ctx, sf_cloud *c, const double *saliency, double non_max_radius, int min_neighbors,
                             int64_t *selected, int64_t *n_selected, int flags)
{
    if (!ctx || !c || !saliency || !selected || !n_selected) { sf_set_error("sf_iss_select: null argument"); return SF_ERR_ARG; }
    SF_CHECK(sf_check_radius("sf_iss_select", "non_max_radius", non_max_radius));
    SF_CHECK(check_rule("sf_iss_select", 1.0, 1.0, min_neighbors));
    SF_HIP(hipSetDevice(ctx->device));
    const int64_t n = c->n;
    *n_selected = 0;
    if (!n) return SF_OK;
    sf_pool_guard tmp(ctx);
    const double *dsal = nullptr;
    int64_t *dsel = nullptr;
    size_t *dnum = nullptr;
    SF_CHECK(stage_in(tmp, saliency, (size_t)n, flags, &dsal));
    SF_CHECK(stage_out(tmp, selected, (size_t)n, flags, &dsel));
    SF_CHECK(tmp.alloc(&dnum, 1));
    SF_CHECK(sf_k10_select_dev(ctx, c, dsal, non_max_radius, min_neighbors, dsel, dnum));
    return sf_k10_finish_selection(ctx, dnum, dsel, selected, n_selected, flags);
}

extern "C" int sf_iss_keypoints(sf_ctx *ctx, sf_cloud *c, double salient_radius, double non_max_radius, double gamma_21, double gamma_32,
                                int min_neighbors, double *saliency, int64_t *selected, int64_t *n_selected, int flags)
{
    if (!ctx || !c || !selected || !n_selected) { sf_set_error("sf_iss_keypoints: null argument"); return SF_ERR_ARG; }
    SF_CHECK(sf_check_radius("sf_iss_keypoints", "salient_radius", salient_radius));
    SF_CHECK(sf_check_radius("sf_iss_keypoints", "non_max_radius", non_max_radius));
    SF_CHECK(check_rule("sf_iss_keypoints", gamma_21, gamma_32, min_neighbors));
    SF_HIP(hipSetDevice(ctx->device));
    const int64_t n = c->n;
    *n_selected = 0;
    if (!n) return SF_OK;
    sf_pool_guard tmp(ctx);
    const bool dev_out = (flags & SF_OUT_DEVICE) != 0;
    double *dsal = saliency;
    int64_t *dsel = nullptr;
    size_t *dnum = nullptr;
    if (!dev_out || !saliency) SF_CHECK(tmp.alloc(&dsal, (size_t)n)); // (wanted on the host, or not wanted at all)
    SF_CHECK(stage_out(tmp, selected, (size_t)n, flags, &dsel));
    SF_CHECK(tmp.alloc(&dnum, 1));
    SF_CHECK(saliency_dev(ctx, c, salient_radius, gamma_21, gamma_32, min_neighbors, dsal, nullptr));
    SF_CHECK(sf_k10_select_dev(ctx, c, dsal, non_max_radius, min_neighbors, dsel, dnum));
    if (saliency) SF_CHECK(finish_out(ctx, saliency, (size_t)n, flags, dsal));
    return sf_k10_finish_selection(ctx, dnum, dsel, selected, n_selected, flags);
}
