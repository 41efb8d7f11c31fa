// search_util.h -- what the radius search (search.hip), the k-NN search (knn.hip), the ISS suppression (iss.hip), the Harris
// tensor sweep (harris.hip), the outlier filters (outliers.hip) and USC (usc.hip) share: the stencil bounds of a query, the run tables and the candidate step of the K2
// family's sweeps, the maps between the caller's point order and the cell-sorted one, and the prototypes of the sweeps that
// search.hip runs for the other files.  (The sort configuration and the rocPRIM call helper: dev_prims.h.)
#pragma once
#include "common.h"
#include "dev_prims.h"
#include "device_util.h"

namespace {


struct to_i64 {
    __host__ __device__ int64_t operator()(int32_t v) const { return (int64_t)v; }
};

__device__ inline void stencil_bounds(double v, double lo, double inv_cell, int dim, int &c0, int &c1)
{
    double t = floor((v - lo) * inv_cell);
    double top = (double)(dim - 1);
    double a = t - 1.0, b = t + 1.0;
    if (!(a >= 0.0)) a = 0.0;
    if (a > top) a = top;
    if (!(b >= 0.0)) b = 0.0;
    if (b > top) b = top;
    c0 = (int)a;
    c1 = (int)b;
}

// ---- the K2 family: k_radius, k_radius_cov (search.hip), k_knn4 (knn.hip), k_iss_nms (iss.hip) ------------------------------
// A wave serves FOUR consecutive queries, one per 16-lane DPP row.  The stencil of a query is up to 9 runs of consecutive
// positions, one per (cz, cy) row of cells; lanes 0..8 of the query's row describe them (sf_k2_window).  The runs are laid end
// to end in units of candidate PAIRS (a pair = one even-aligned 16-byte load: the vector-memory pipe of a CU accepts one wave
// instruction per 16 cycles whatever its width per lane, so two candidates per lane cost 3 loads per 128 candidates instead of
// 3 per 64) and every step of a sweep takes the next 64 pairs, whichever runs they fall in (sf_k2_load_pair).  Everything a
// lane needs to find its pair is vector work -- a DPP scan gives the runs' first pair slots, the table goes to LDS
// (sf_k2_store_runs) -- because the scalar unit is shared by the whole CU.

// MODE 0: count only.  MODE 1: fill at the exact CSR offsets of a previous count + scan.
// MODE 2: optimistic single pass -- query q owns the fixed slot [q*cap, (q+1)*cap) of idx; hits beyond cap
//         are counted but not stored, and the host falls back to the exact two-pass scheme if any list
//         overflowed (HBM is plentiful: slots cost cap*4 B per query).
#ifndef SF_K2_WPB
#define SF_K2_WPB 8 // waves per workgroup, four queries each (0.521 / 0.516 / 0.498 / 0.489 ms at C3 for 1 / 2 / 4 / 8)
#endif

// Positions [s, e) of run sl (lanes 0..8 of a row; the other lanes and the rows past the last query, !row_live, get an empty
// one) of the query (px, py, pz), whose stencil is the cell rows y0..y1 x z0..z1.
// The row (cy, cz) of cells is the band [lo + c edge, lo + (c + 1) edge) in y and in z.  A point of it within r
// of the query is at least (dy, dz) away in those two axes -- the gaps between the query and the bands -- so
// its x lies within w = sqrt(r^2 - dy^2 - dz^2) of the query's: only the FINE x cells (xsub per edge) that
// [px - w, px + w] touches are swept, 12-14 edge-lengths of cells per query instead of 27.  The cell of a
// coordinate is a monotone function of it, so every point with px - w <= x <= px + w lies in a cell between
// the cells of the two ends; the gaps shrink and w grows by a slack that is far above any rounding involved (next
// paragraph), so the sweep can only be wider than necessary, never narrower.
// All of it in GRID-RELATIVE coordinates (p - lo, what the cell assignment itself uses): the rounding of a relative
// coordinate, of a band edge c * cell and of fl(1 / cell) is a few ulps of the grid's EXTENT, whereas band edges
// and px +- w formed in absolute coordinates would round by ulps of |lo| and |p| -- for a cloud in UTM-like
// coordinates (1e6 .. 1e7 with a cell of 1e-2) far more than any fixed fraction of the cell.  `slack` covers both: 1e-9
// of the cell plus 1e-15 of the relative coordinates involved.
__device__ __forceinline__ void sf_k2_window(const sf_grid_desc &g, const int32_t *__restrict__ cell_start, double px, double py,
                                             double pz, double r2, int sl, bool row_live, int y0, int y1, int z0, int z1, int &s,
                                             int &e)
{
    const int r = sl < 9 ? sl : 8;
    const int cz = z0 + r / 3, cy = y0 + r % 3;
    bool ok = sl < 9 && row_live && cz <= z1 && cy <= y1;
    const int64_t row = ((int64_t)(ok ? cz : z0) * g.dim[1] + (ok ? cy : y0)) * g.dim[0];
    const double pxr = px - g.lo[0], pyr = py - g.lo[1], pzr = pz - g.lo[2];
    const double by0 = (double)cy * g.cell, bz0 = (double)cz * g.cell;
    const double slack_y = 1e-9 * g.cell + 1e-15 * (fabs(pyr) + by0 + g.cell);
    const double slack_z = 1e-9 * g.cell + 1e-15 * (fabs(pzr) + bz0 + g.cell);
    const double dy = fmax(fmax(by0 - pyr, pyr - (by0 + g.cell)) - slack_y, 0.0);
    const double dz = fmax(fmax(bz0 - pzr, pzr - (bz0 + g.cell)) - slack_z, 0.0);
    const double w2 = (r2 * (1.0 + 1e-9) - dy * dy) - dz * dz;
    ok = ok && w2 >= 0.0;
    const double w = sf_sqrt_fast(fmax(w2, 0.0)) * (1.0 + 1e-9) + 1e-9 * g.cell +
                     1e-15 * (fabs(pxr) + (double)g.dim[0] * (g.cell / (double)g.xsub));
    s = 0;
    e = 0;
    if (sl < 9) {
        s = cell_start[row + sf_cell_coord(pxr - w, 0.0, g.inv_cell_x, g.dim[0])];
        e = cell_start[row + sf_cell_coord(pxr + w, 0.0, g.inv_cell_x, g.dim[0]) + 1];
    }
    if (!ok) { s = 0; e = 0; }
}

// Lane sl of a row enters its run [s, e) into the row's table (12 entries, 9 runs) and returns the run's first pair slot:
// lane r < 9: of run r; lane 9 (npairs = 0): the total number of pair slots.
__device__ __forceinline__ int sf_k2_store_runs(int s, int e, int sl, int4 *tab_row)
{
    const int base = s & ~1; // pairs start at an EVEN position: every 16-byte load is naturally aligned
    const int npairs = (e - base + 1) >> 1;
    // inclusive scan of npairs inside the 16-lane row (row_shr DPP steps), then exclusive = inclusive - own
    int inc = npairs;
    inc += __builtin_amdgcn_update_dpp(0, inc, 0x111, 0xf, 0xf, false); // row_shr:1
    inc += __builtin_amdgcn_update_dpp(0, inc, 0x112, 0xf, 0xf, false); // row_shr:2
    inc += __builtin_amdgcn_update_dpp(0, inc, 0x114, 0xf, 0xf, false); // row_shr:4
    inc += __builtin_amdgcn_update_dpp(0, inc, 0x118, 0xf, 0xf, false); // row_shr:8
    const int first_slot = inc - npairs;
    if (sl < 12) tab_row[sl] = make_int4(base - 2 * first_slot, s, e, first_slot); // j = .x + 2 * slot; .w: first slot
    return first_slot;
}

// One lane's share of a sweep step: the candidate pair (j, j + 1) of slot f of the table `tab`, which of the two lie inside
// their run (in0, in1: the alignment padding of a run is a candidate of the neighbouring row, which that row's own run also
// brings), and their coordinates.  b4, b8: first slots of runs 4 and 8; nslots: the total (scalars, from sf_k2_store_runs).
struct sf_k2_pair {
    int j;
    bool in0, in1;
    double2 X, Y, Z;
};
__device__ __forceinline__ sf_k2_pair sf_k2_load_pair(const int4 *tab, int b4, int b8, int nslots, int f, const double *__restrict__ xs,
                                                      const double *__restrict__ ys, const double *__restrict__ zs)
{
    // run of slot f = last run whose first slot is <= f: a three-level binary search, the first level against a
    // scalar, the other two against the first-slot column of the table in LDS (an LDS read costs the vector
    // pipe one instruction; eight compare-and-add pairs cost it sixteen and more)
    int r = f >= b4 ? 4 : 0;
    r += f >= tab[r + 2].w ? 2 : 0;
    r += f >= tab[r + 1].w ? 1 : 0;
    r = f >= b8 ? 8 : r;
    const int4 t = tab[r];
    const bool live = f < nslots;
    sf_k2_pair p;
    p.j = live ? t.x + 2 * f : 0; // idle lanes of the last step load pair 0 (always there)
    p.in0 = live & (p.j >= t.y);
    p.in1 = live & (p.j + 1 < t.z);
    p.X = *reinterpret_cast<const double2 *>(xs + p.j);
    p.Y = *reinterpret_cast<const double2 *>(ys + p.j);
    p.Z = *reinterpret_cast<const double2 *>(zs + p.j);
    return p;
}

// List positions of a lane's two hits, lists being in scan order (slot by slot, the pair's first candidate first): .x of
// candidate j (if hit0), .y of candidate j + 1; m0, m1: the wave's hit masks of the two, total: hits of the steps before.
__device__ __forceinline__ int2 sf_k2_hit_pos(int total, unsigned long long m0, unsigned long long m1, bool hit0)
{
    const int pos = total + sf_prefix_count(m0) + sf_prefix_count(m1);
    return make_int2(pos, pos + (hit0 ? 1 : 0));
}

#define SF_K2_SAMPLE 2048 // queries whose lists are counted before a first search sizes its slots

// ---- the caller's point order <-> the cell-sorted order of the current grid (perm: cell-sorted position -> caller index) ------
struct sf_identity {
    template <typename T> __host__ __device__ T operator()(T v) const { return v; }
};
// out[perm[i]] = f(sorted[i]), i < n
template <typename S, typename T, typename F>
__global__ void k_perm_scatter(const S *__restrict__ sorted, const int32_t *__restrict__ perm, int64_t n, T *__restrict__ out, F f)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[perm[i]] = f(sorted[i]);
}
// sorted[i] = src[perm[i]], i < n; sorted[n .. n + pad) = 0 (what a sweep's pair loads may touch past the end)
template <typename T>
__global__ void k_perm_gather(const T *__restrict__ src, const int32_t *__restrict__ perm, int64_t n, int pad, T *__restrict__ sorted)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) sorted[i] = src[perm[i]];
    else if (i < n + pad) sorted[i] = T(0);
}
template <typename S, typename T, typename F = sf_identity>
int sf_perm_scatter(sf_ctx *ctx, const char *name, const sf_cloud *c, const S *sorted, T *out, F f = F())
{
    SF_LAUNCH(ctx, name, (k_perm_scatter<S, T, F>), dim3((unsigned)sf_div_up(c->n, 256)), dim3(256), sorted, (const int32_t *)c->perm, c->n, out, f);
    return SF_OK;
}
template <typename T>
int sf_perm_gather(sf_ctx *ctx, const char *name, const sf_cloud *c, const T *src, int pad, T *sorted)
{
    SF_LAUNCH(ctx, name, k_perm_gather<T>, dim3((unsigned)sf_div_up(c->n + pad, 256)), dim3(256), src, (const int32_t *)c->perm, c->n, pad, sorted);
    return SF_OK;
}

} // namespace

// search.hip, for knn.hip: queries into processing order, and the lists of a strided sample of them counted at a radius
int sf_k2_prepare_queries(sf_ctx *ctx, sf_cloud *c, sf_nbrs *nb, const double *queries, int flags);
int sf_k2_count_sample(sf_ctx *ctx, sf_cloud *c, sf_nbrs *nb, double r2, int32_t *sel_dev, int32_t *cnt_dev);
// search.hip, for iss.hip and outliers.hip: keep or rebuild the grid for a radius (sf_k2_own_grid: the grid sf_cloud_build_grid
// makes for this very radius, whatever valid grid the cloud carries), k_radius_cov over the whole cloud with its counts, and
// the count sweep (k_radius, MODE 0) over the whole cloud: count[n + 1] by cell-sorted position
int sf_k2_ensure_grid(sf_ctx *ctx, sf_cloud *c, double radius);
int sf_k2_own_grid(sf_ctx *ctx, sf_cloud *c, double radius);
int sf_k2_radius_cov_self(sf_ctx *ctx, sf_cloud *c, double radius, const char *prof, double *cov, int32_t *count);
int sf_k2_count_self(sf_ctx *ctx, sf_cloud *c, double radius, const char *prof, int32_t *count);
// ... and the prologue of every stage that weighs or filters by density: sf_k2_own_grid, then that sweep into n + 1 words of the guard
int sf_k2_ball_sizes(sf_ctx *ctx, sf_cloud *c, sf_pool_guard &g, double radius, const char *prof, int32_t **count);
// iss.hip, for harris.hip: K10's selection chain on any per-point score in the caller's order (device).  sf_k10_select_dev: the
// suppression over the balls of `radius` on whichever grid serves it, then the selected indices, ascending, and their number
// (device word *dnum); sf_k10_finish_selection: the count to the host (one read-back), then the indices if the host wants them
int sf_k10_select_dev(sf_ctx *ctx, sf_cloud *c, const double *score, double radius, int min_neighbors, int64_t *selected, size_t *dnum);
int sf_k10_finish_selection(sf_ctx *ctx, const size_t *dnum, const int64_t *dsel, int64_t *selected, int64_t *n_selected, int flags);

