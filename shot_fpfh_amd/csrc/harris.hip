// harris.hip -- K23: Harris 3D keypoints (the detector of pcl::HarrisKeypoint3D: Sipiran & Bustos 2011 on the normals), the
// second detector that looks at the geometry.  ISS (K10) scores the spread of the POSITIONS of a ball; Harris scores how the
// NORMALS of the ball turn -- corners and creases, not blobs.
//
//   C[i]        = (1 / k) sum over j in B(i, r) of n_j n_j^T, k = |B(i, r)| (i included); no centring, the normals as given;
//   response[i] = harris: 0.04 + det C - 0.04 tr^2   noble: det C / tr   lowe: det C / tr^2   tomasi: the smallest eigenvalue
//                 of C   curvature: e3 / (e1 + e2 + e3) of the mean-centred POSITION covariance of the same ball (no normals);
//                 -1 when k < min_neighbors, tr <= 0, the matrix is numerically rank-deficient (det <= 1e-12 tr^3, tomasi:
//                 lambda_min <= 1e-12 tr, curvature: e3 <= 1e-12 e1) or the value is not > threshold (a NaN is not);
//   keypoint i  <=> response[i] > 0, |B(i, r_n)| >= min_neighbors, and no j in B(i, r_n) has a larger response (K10's chain).
//
// Mapping.  k_harris_tensor is the K2 family's candidate sweep (search_util.h), set up exactly as k_iss_nms: four queries per
// wave, run tables per 16-lane row, candidate pairs, the conservative x window, the ball test d2 <= r2 in unfused float64.  A
// step of the sweep takes 128 candidates with SIX 16-byte loads per lane: the three coordinate pairs of sf_k2_load_pair and the
// three pairs of the candidates' normal components, from a cell-sorted SoA of the normals (nsx / nsy / nsz, padded by the two
// elements a pair load may touch past the end) that k_harris_normals_soa fills from the records beforehand.  Reading the
// normals out of the 48-byte records instead would cost FOUR loads per step for the normals alone (a candidate's normal is
// rec[6 j + 3 .. 6 j + 5], which straddles the aligned 16-byte pieces {z, nx} and {ny, nz}: two loads per candidate), and the
// vector-memory pipe is paid per wave instruction whatever its width: seven loads per step against six.  The SoA costs one
// pass of 48 n bytes read and 24 n written per call, a per cent of the sweep.
// A hit's normal enters six products; a miss's is replaced by zero BEFORE the products (three selects per candidate instead of
// six on the products, and a non-finite normal outside the ball never meets the sums).  Per step and lane: 18 float64
// instructions for the two ball tests, 24 for the twelve products and their additions.  The six per-lane sums are reduced across
// the wave in one fixed order (sf_wave_sum8, as k_radius_cov's moments) once per query, six lanes divide by k and store.
// No list, no ring, no second sweep: nothing is centred, so the one sweep serves a ball of any size.  The only LDS is the run
// tables (6 KB per workgroup).
// What bounds it: the vector-memory pipe's issue rate, like every sweep of the family -- six load instructions per step where
// the count sweep has three, and it takes about twice the count sweep's time (the figures: DESIGN 3, K23); the 42 float64
// instructions of a step fit under the loads.  It works per CANDIDATE (about three per ball member), where k_radius_cov pays
// its moments per MEMBER out of LDS: cheaper than that kernel on balls of hundreds of points (no second and third sweep),
// somewhat dearer at a hundred.
//
// Orders (iss.hip's note applies word for word): the tensor pass always runs on the grid sf_cloud_build_grid makes for r itself
// (sf_k2_own_grid) -- the order of the sums follows the cell-sorted order -- and the response goes to the CALLER's order
// through that grid's perm; the suppression takes whichever grid is there.  (-n)(-n)^T = n n^T to the bit: the sign PCA normals
// come with does not reach the tensor.
#include <cmath>

#include "eigh3.h"
#include "host_stage.h"
#include "search_util.h"

namespace {

#define SF_HARRIS_FLOOR 1e-12 // det > FLOOR tr^3, lambda_min > FLOOR tr, e3 > FLOOR e1: a float64 sum of k <= 1e4 terms carries ~k 2^-53 tr

#ifndef SF_HARRIS_WPB
#define SF_HARRIS_WPB 8 // waves per workgroup, four queries each (k_iss_nms's shape)
#endif

// rec {x, y, z, nx, ny, nz} by cell-sorted position -> the three normal components as arrays of n + 2 (the pad: zeros)
__global__ __launch_bounds__(256) void k_harris_normals_soa(const double *__restrict__ rec, int64_t n, double *__restrict__ nsx,
                                                            double *__restrict__ nsy, double *__restrict__ nsz)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n + 2) return;
    double a = 0.0, b = 0.0, c = 0.0;
    if (i < n) {
        const double2 *p = reinterpret_cast<const double2 *>(rec + 6 * i);
        const double2 u = p[1], v = p[2];
        a = u.y; b = v.x; c = v.y;
    }
    nsx[i] = a; nsy[i] = b; nsz[i] = c;
}

// tensor[6 q .. 6 q + 5] = (1 / k) sum of n n^T over the ball of squared radius r2 around position q (xx yx zx yy zy zz, the
// order of k_radius_cov's output), count[q] = k; q = cell-sorted position
__global__ __launch_bounds__(64 * SF_HARRIS_WPB) void k_harris_tensor(sf_grid_desc g, const int32_t *__restrict__ cell_start,
                                                                      const double *__restrict__ xs, const double *__restrict__ ys,
                                                                      const double *__restrict__ zs, const double *__restrict__ nsx,
                                                                      const double *__restrict__ nsy, const double *__restrict__ nsz,
                                                                      int64_t m, double r2, double *__restrict__ tensor,
                                                                      int32_t *__restrict__ count)
{
    const int lane = threadIdx.x & 63, sl = lane & 15, rw = lane >> 4;
    const int64_t q0 = sf_uniform64((sf_xcd_block() * SF_HARRIS_WPB + (threadIdx.x >> 6)) * 4);
    if (q0 >= m) return;
    const int nq = (int)(m - q0 < 4 ? m - q0 : 4);
    const int64_t qm = q0 + (rw < nq ? rw : 0);
    const double pxv = xs[qm], pyv = ys[qm], pzv = zs[qm]; // this row's query
    int y0, y1, z0, z1;
    stencil_bounds(pyv, g.lo[1], g.inv_cell, g.dim[1], y0, y1);
    stencil_bounds(pzv, g.lo[2], g.inv_cell, g.dim[2], z0, z1);
    __shared__ int4 runs[SF_HARRIS_WPB][4][12];
    int4(*const tabs)[12] = runs[threadIdx.x >> 6];
    int s, e;
    sf_k2_window(g, cell_start, pxv, pyv, pzv, r2, sl, rw < nq, y0, y1, z0, z1, s, e);
    const int first_slot = sf_k2_store_runs(s, e, sl, tabs[rw]);
    __builtin_amdgcn_wave_barrier(); // the tables are written and read by this wave only
    for (int qi = 0; qi < nq; ++qi) {
        const int64_t q = q0 + qi;
        const int4 *const tab = tabs[qi];
        const double px = sf_read_lane(pxv, 16 * qi), py = sf_read_lane(pyv, 16 * qi), pz = sf_read_lane(pzv, 16 * qi);
        const int b4 = __shfl(first_slot, 16 * qi + 4), b8 = __shfl(first_slot, 16 * qi + 8);
        const int nslots = sf_uniform(__shfl(first_slot, 16 * qi + 9));
        int total = 0;
        double part[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int f0 = 0; f0 < nslots; f0 += 64) {
            const sf_k2_pair c = sf_k2_load_pair(tab, b4, b8, nslots, f0 + lane, xs, ys, zs);
            const double2 NX = *reinterpret_cast<const double2 *>(nsx + c.j);
            const double2 NY = *reinterpret_cast<const double2 *>(nsy + c.j);
            const double2 NZ = *reinterpret_cast<const double2 *>(nsz + c.j);
            const double dxa = c.X.x - px, dya = c.Y.x - py, dza = c.Z.x - pz;
            const double dxb = c.X.y - px, dyb = c.Y.y - py, dzb = c.Z.y - pz;
            const double d2a = (dxa * dxa + dya * dya) + dza * dza, d2b = (dxb * dxb + dyb * dyb) + dzb * dzb;
            const bool hit0 = c.in0 & (d2a <= r2);
            const bool hit1 = c.in1 & (d2b <= r2);
            total += __popcll(__ballot(hit0)) + __popcll(__ballot(hit1));
            const double ax = hit0 ? NX.x : 0.0, ay = hit0 ? NY.x : 0.0, az = hit0 ? NZ.x : 0.0; // (a miss adds +0 six times)
            const double bx = hit1 ? NX.y : 0.0, by = hit1 ? NY.y : 0.0, bz = hit1 ? NZ.y : 0.0;
            part[0] += ax * ax; part[1] += ay * ax; part[2] += az * ax; part[3] += ay * ay; part[4] += az * ay; part[5] += az * az;
            part[0] += bx * bx; part[1] += by * bx; part[2] += bz * bx; part[3] += by * by; part[4] += bz * by; part[5] += bz * bz;
        }
        const double tot = sf_wave_sum8(part); // lanes 8 i .. 8 i + 7 hold the sum of part[i]
        const double kk = (double)(total > 0 ? total : 1);
        const int t = lane >> 3;
        if ((lane & 7) == 0 && t < 6) tensor[6 * q + t] = tot / kk; // one correctly rounded division per entry
        if (lane == 0) count[q] = total;
    }
}

// One lane per cell-sorted position: the response rule above on the 3 x 3 matrix `mat` left by k_harris_tensor (or, for
// curvature, by k_radius_cov), scattered to the caller's numbering with the ball size and the matrix if they are wanted.
__global__ __launch_bounds__(64) void k_harris_response(const double *__restrict__ mat, const int32_t *__restrict__ cnt,
                                                        const int32_t *__restrict__ perm, int64_t n, int method, double threshold,
                                                        int min_neighbors, double *__restrict__ response, int32_t *__restrict__ count,
                                                        double *__restrict__ mat_out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double *c = mat + 6 * i;
    const double c11 = c[0], c21 = c[1], c31 = c[2], c22 = c[3], c32 = c[4], c33 = c[5];
    const int k = cnt[i];
    double tr = (c11 + c22) + c33, value;
    bool full; // the matrix is above its rank floor
    if (method == SF_HARRIS_TOMASI || method == SF_HARRIS_CURVATURE) {
        const sf_eig::eig3 e = sf_eig::eigh3_lower(c11, c21, c31, c22, c32, c33);
        if (method == SF_HARRIS_TOMASI) {
            value = e.w1;
            full = e.w1 > SF_HARRIS_FLOOR * tr;
        } else {
            tr = (e.w3 + e.w2) + e.w1;
            value = e.w1 / tr;
            full = e.w1 > SF_HARRIS_FLOOR * e.w3;
        }
    } else {
        const double det = (c11 * (c22 * c33 - c32 * c32) - c21 * (c21 * c33 - c32 * c31)) + c31 * (c21 * c32 - c22 * c31);
        full = det > SF_HARRIS_FLOOR * ((tr * tr) * tr);
        value = method == SF_HARRIS_HARRIS ? (0.04 + det) - 0.04 * (tr * tr) : method == SF_HARRIS_NOBLE ? det / tr : det / (tr * tr);
    }
    const bool ok = k >= min_neighbors && tr > 0.0 && full && value > threshold;
    const int64_t o = perm[i];
    response[o] = ok ? value : -1.0;
    if (count) count[o] = k;
    if (mat_out) {
        double *d = mat_out + 6 * o;
        d[0] = c11; d[1] = c21; d[2] = c31; d[3] = c22; d[4] = c32; d[5] = c33;
    }
}

int check_rule(const char *who, int method, double threshold, int min_neighbors)
{
    if (method < SF_HARRIS_HARRIS || method > SF_HARRIS_CURVATURE) { sf_set_error("%s: unknown method %d", who, method); return SF_ERR_ARG; }
    if (!(threshold >= 0.0 && std::isfinite(threshold))) {
        sf_set_error("%s: threshold must be finite and not negative (got %g): the suppression only considers responses above 0", who, threshold);
        return SF_ERR_ARG;
    }
    if (min_neighbors < 1) { sf_set_error("%s: min_neighbors must be at least 1 (got %d)", who, min_neighbors); return SF_ERR_ARG; }
    return SF_OK;
}

int check_normals(const char *who, const sf_cloud *c, int method)
{
    if (method == SF_HARRIS_CURVATURE || c->nrm_orig) return SF_OK;
    sf_set_error("%s: every method but SF_HARRIS_CURVATURE needs normals, and the cloud has none", who);
    return SF_ERR_STATE;
}

// response (and counts and matrices, nullable) of every point in the caller's order, device pointers
int response_dev(sf_ctx *ctx, sf_cloud *c, double radius, int method, double threshold, int min_neighbors, double *response,
                 int32_t *count, double *mat_out)
{
    const int64_t n = c->n;
    if (!n) return SF_OK;
    SF_CHECK(sf_k2_own_grid(ctx, c, radius)); // (see "Orders" above)
    sf_pool_guard tmp(ctx);
    double *mat = nullptr;
    int32_t *cnt = nullptr;
    SF_CHECK(tmp.alloc(&mat, (size_t)n * 6));
    SF_CHECK(tmp.alloc(&cnt, (size_t)n));
    if (method == SF_HARRIS_CURVATURE) {
        SF_CHECK(sf_k2_radius_cov_self(ctx, c, radius, "k23h_position_cov", mat, cnt));
    } else {
        SF_CHECK(sf_cloud_ensure_sorted_normals(ctx, c));
        double *soa = nullptr;
        const size_t lde = ((size_t)n + 3) & ~(size_t)1; // n + 2 rounded up to even: every array starts 16-byte aligned, as its pairs do
        SF_CHECK(tmp.alloc(&soa, 3 * lde));
        SF_LAUNCH(ctx, "k23h_normals_soa", k_harris_normals_soa, dim3((unsigned)sf_div_up(n + 2, 256)), dim3(256), (const double *)c->rec, n,
                  soa, soa + lde, soa + 2 * lde);
        const sf_grid_desc g = sf_make_grid_desc(c);
        SF_LAUNCH(ctx, "k23h_harris_tensor", k_harris_tensor, dim3(sf_xcd_grid(sf_div_up(n, 4 * SF_HARRIS_WPB))), dim3(64 * SF_HARRIS_WPB), g,
                  (const int32_t *)c->cell_start, (const double *)c->xs, (const double *)c->ys, (const double *)c->zs, (const double *)soa,
                  (const double *)(soa + lde), (const double *)(soa + 2 * lde), n, radius * radius, mat, cnt);
    }
    SF_LAUNCH(ctx, "k23h_harris_response", k_harris_response, dim3((unsigned)sf_div_up(n, 64)), dim3(64), (const double *)mat,
              (const int32_t *)cnt, (const int32_t *)c->perm, n, method, threshold, min_neighbors, response, count, mat_out);
    return SF_OK;
}

} // namespace

extern "C" int sf_harris_response(sf_ctx *ctx, sf_cloud *c, double radius, int method, double threshold, int min_neighbors,
                                  double *response, int32_t *count, double *tensor, int flags)
{
    if (!ctx || !c || !response) { sf_set_error("sf_harris_response: null argument"); return SF_ERR_ARG; }
    SF_CHECK(sf_check_radius("sf_harris_response", "radius", radius));
    SF_CHECK(check_rule("sf_harris_response", method, threshold, min_neighbors));
    SF_CHECK(check_normals("sf_harris_response", c, method));
    SF_HIP(hipSetDevice(ctx->device));
    const int64_t n = c->n;
    if (!n) return SF_OK;
    sf_pool_guard tmp(ctx);
    double *dres = nullptr, *dten = nullptr;
    int32_t *dcnt = nullptr;
    SF_CHECK(stage_out(tmp, response, (size_t)n, flags, &dres));
    if (count) SF_CHECK(stage_out(tmp, count, (size_t)n, flags, &dcnt));
    if (tensor) SF_CHECK(stage_out(tmp, tensor, (size_t)n * 6, flags, &dten));
    SF_CHECK(response_dev(ctx, c, radius, method, threshold, min_neighbors, dres, dcnt, dten));
    SF_CHECK(finish_out(ctx, response, (size_t)n, flags, dres));
    if (count) SF_CHECK(finish_out(ctx, count, (size_t)n, flags, dcnt));
    if (tensor) SF_CHECK(finish_out(ctx, tensor, (size_t)n * 6, flags, dten));
    return stage_sync_out(ctx, flags);
}

extern "C" int sf_harris_keypoints(sf_ctx *ctx, sf_cloud *c, double radius, double non_max_radius, int method, double threshold,
                                   int min_neighbors, double *response, int64_t *selected, int64_t *n_selected, int flags)
{
    if (!ctx || !c || !selected || !n_selected) { sf_set_error("sf_harris_keypoints: null argument"); return SF_ERR_ARG; }
    SF_CHECK(sf_check_radius("sf_harris_keypoints", "radius", radius));
    SF_CHECK(sf_check_radius("sf_harris_keypoints", "non_max_radius", non_max_radius));
    SF_CHECK(check_rule("sf_harris_keypoints", method, threshold, min_neighbors));
    SF_CHECK(check_normals("sf_harris_keypoints", c, method));
    SF_HIP(hipSetDevice(ctx->device));
    const int64_t n = c->n;
    *n_selected = 0;
    if (!n) return SF_OK;
    sf_pool_guard tmp(ctx);
    const bool dev_out = (flags & SF_OUT_DEVICE) != 0;
    double *dres = response;
    int64_t *dsel = nullptr;
    size_t *dnum = nullptr;
    if (!dev_out || !response) SF_CHECK(tmp.alloc(&dres, (size_t)n)); // (wanted on the host, or not wanted at all)
    SF_CHECK(stage_out(tmp, selected, (size_t)n, flags, &dsel));
    SF_CHECK(tmp.alloc(&dnum, 1));
    SF_CHECK(response_dev(ctx, c, radius, method, threshold, min_neighbors, dres, nullptr, nullptr));
    SF_CHECK(sf_k10_select_dev(ctx, c, dres, non_max_radius, min_neighbors, dsel, dnum));
    if (response) SF_CHECK(finish_out(ctx, response, (size_t)n, flags, dres));
    return sf_k10_finish_selection(ctx, dnum, dsel, selected, n_selected, flags);
}
