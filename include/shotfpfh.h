/*
 * shotfpfh.h -- C ABI of libshotfpfh.so, the MI355X (gfx950) SHOT / FPFH descriptor engine.
 *
 * This is the drop-in boundary for the hot path of aubin-tchoi/shot-fpfh.  The reference is pure
 * Python with no FFI of its own; each entry point below replaces the NumPy / scikit-learn /
 * SciPy call named next to it (file:line into the reference checkout) and is what a ctypes stub
 * in the reference would bind.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes.  No torch / numpy types.
 *   - Every int-returning call returns SF_OK (0) or a negative SF_ERR_* code; the message is
 *     available from sf_last_error() (thread-local).  Handle-returning calls return NULL on error.
 *   - All floating-point data is float64, row-major.  Indices into the cloud are int32/int64 in
 *     the caller's ORIGINAL point numbering unless a parameter says otherwise.
 *   - `flags` tells where the data pointers of a call live:
 *       SF_HOST (0)      every data pointer is host memory (the library copies in/out)
 *       SF_OUT_DEVICE    output pointers are device memory of ctx's GPU (no D2H copy)
 *       SF_IN_DEVICE     input data pointers are device memory (no H2D copy)
 *     Handles (sf_cloud, sf_nbrs, sf_spfh) always live on the device.
 *   - The library never keeps a caller pointer after a call returns.
 *   - One sf_ctx per GPU and per host thread; calls on one ctx are stream-ordered on the ctx's
 *     own HIP stream (sf_stream).  Do not fork() after sf_create().
 *   - There is NO CPU fallback: without a GPU sf_create() fails.
 */
#ifndef SHOTFPFH_H
#define SHOTFPFH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SF_OK 0
#define SF_ERR_ARG (-1)
#define SF_ERR_HIP (-2)
#define SF_ERR_NOMEM (-3)
#define SF_ERR_COMM (-4)
#define SF_ERR_STATE (-5)
#define SF_ERR_UNSUPPORTED (-6)
#define SF_ERR_BIN_RANGE (-7) /* sf_shot_serial_bins: a neighbour in cosine bin n (the reference's IndexError) */

#define SF_HOST 0
#define SF_OUT_DEVICE 1
#define SF_IN_DEVICE 2

#define SF_SHOT_LEN 352 /* 11 cosine x 8 azimuth x 2 elevation x 2 radial bins (shot.py:195) */
#define SF_SHOT_MAX_COSINE_BINS 64 /* sf_shot_serial_bins: rows of up to 32 x 64 = 2048 bins */
#define SF_USC_MAX_BINS 4096 /* sf_usc: azimuth_bins x elevation_bins x radius_bins at most (16 B of LDS per bin and wave) */
#define SF_PFH_MAX_BINS 16 /* sf_pfh: bins per angle; rows of n_bins^3 <= 4096 doubles, the row cap of sf_usc */
#define SF_SPIN_MAX_WIDTH 44 /* sf_spin_images: image_width at most; rows of (W + 1)(2 W + 1) <= 4005 doubles, within the row cap of sf_usc */
#define SF_FAST_FPFH_BINS 8 /* n_bins up to here: LDS-histogram K6 and the matrix-core / streaming K7 */
#define SF_MAX_FPFH_BINS 1290 /* n_bins^3 must fit an int; the reference takes any n_bins (fpfh.py:16).  What bounds n_bins in
                                practice is the table of n x n_bins^3 32-bit counts in HBM (the reference holds twice that in host RAM) */

typedef struct sf_ctx sf_ctx;     /* one GPU: device id, stream, scratch, optional RCCL comm  */
typedef struct sf_cloud sf_cloud; /* resident point cloud + uniform grid (replaces KDTree(X))  */
typedef struct sf_nbrs sf_nbrs;   /* resident CSR radius-neighbour lists of a query set        */
typedef struct sf_spfh sf_spfh;   /* resident SPFH table (integer bin counts + list lengths)   */
typedef struct sf_voxels sf_voxels; /* voxel partition of a point set (grid_subsampling)       */

/* ---- library / context ---------------------------------------------------------------- */
const char *sf_last_error(void);
const char *sf_version(void);
int sf_device_count(void);
sf_ctx *sf_create(int device);
void sf_destroy(sf_ctx *ctx);
int sf_sync(sf_ctx *ctx);
void *sf_stream(sf_ctx *ctx); /* hipStream_t the kernels are launched on */
/* A context owns two HIP streams.  sf_fork: following calls go to the side stream, ordered after the work issued so
 * far; sf_switch(0|1) picks the stream of the following calls while forked; sf_join: back on the main stream, ordered
 * after the side stream.  While forked only calls that neither allocate nor free device memory may be issued
 * (resident K4-K7 calls).  Used to run the FPFH chain and the SHOT chain of one pass side by side. */
int sf_fork(sf_ctx *ctx);
int sf_switch(sf_ctx *ctx, int side);
int sf_join(sf_ctx *ctx);
/* sf_mark: remember the point reached on the current stream; sf_wait_mark: the current stream waits for that point -- and
 * only for it, not for work issued on the marked stream later (sf_join waits for everything). */
int sf_mark(sf_ctx *ctx);
int sf_wait_mark(sf_ctx *ctx);

/* ---- raw device memory (for callers that keep results resident) ------------------------- */
void *sf_dev_alloc(sf_ctx *ctx, size_t bytes);
int sf_dev_free(sf_ctx *ctx, void *dev_ptr);
/* Page-locked host memory: host output pointers of any call may point into it, and the device-to-host copy is then one
 * DMA at PCIe speed instead of a staged copy into pageable memory.  Pinning is slow: allocate once, reuse.
 * sf_host_free may be called after sf_destroy (ctx is ignored). */
void *sf_host_alloc(sf_ctx *ctx, size_t bytes);
int sf_host_free(sf_ctx *ctx, void *host_ptr);
int sf_h2d(sf_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);
int sf_d2h(sf_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);
int sf_d2d(sf_ctx *ctx, void *dst_dev, const void *src_dev, size_t bytes); /* stream-ordered, asynchronous */

/* ---- cloud + grid: replaces sklearn KDTree(X) -------------------------------------------
 * call sites: fpfh.py:26, shot_parallelization.py:167,220,229,283, pca_based_descriptors.py:45-49
 * sf_cloud_upload copies xyz (n x 3) and normals (n x 3, nullable) to the GPU.
 * sf_cloud_build_grid (kernel K1) bins the points into cells of edge >= `cell`, sorts them by cell
 * and keeps cell-sorted SoA copies of xyz / normals; it must be called with cell >= the largest
 * radius later searched (re-callable; a search with a larger radius -- or one below half the cell, for speed -- and every
 * k-NN search rebuild automatically).  Every build re-sorts into fresh arrays: list sets (sf_nbrs) made on an earlier build
 * are refused by their consumers with SF_ERR_STATE from then on -- use a search's lists before the next rebuild. */
sf_cloud *sf_cloud_upload(sf_ctx *ctx, const double *xyz, const double *normals, int64_t n, int flags);
int sf_cloud_set_normals(sf_ctx *ctx, sf_cloud *cloud, const double *normals, int flags);
int sf_cloud_build_grid(sf_ctx *ctx, sf_cloud *cloud, double cell);
/* Multi-GPU variant of K1: build only what the queries at cell-sorted positions [begin, end) -- a rank's block --
 * can reach within `reach` grid cells (1 for SHOT / normals / SPFH of the block, 2 when the SPFH rows of the
 * block's one-cell halo are recomputed locally for FPFH).  Whole z-layers of cells are kept; positions, perm and
 * the cell table keep their GLOBAL numbering, so block / halo ranges and every result are exactly those of a
 * whole-cloud build, but only ~1/N of the cloud is sorted and gathered.  [*pop_begin, *pop_end) (nullable) returns
 * the populated position range; self-searches must stay inside it (anything else rebuilds the whole grid). */
int sf_cloud_build_grid_block(sf_ctx *ctx, sf_cloud *cloud, double cell, int64_t begin, int64_t end, int reach,
                              int64_t *pop_begin, int64_t *pop_end);
int64_t sf_cloud_size(const sf_cloud *cloud);
void sf_cloud_free(sf_ctx *ctx, sf_cloud *cloud);
/* cell-sorted position -> original index (n entries, host) */
int sf_cloud_perm(sf_ctx *ctx, sf_cloud *cloud, int32_t *perm);
/* Multi-GPU sharding helper: the smallest range [halo_begin, halo_end) of cell-sorted positions that
 * contains every point within one grid cell (>= the search radius) of the block [begin, end).  The grid
 * orders cells z-slowest, so a block is a z-slab and its halo is one contiguous run on each side. */
int sf_cloud_halo_range(sf_ctx *ctx, sf_cloud *cloud, int64_t begin, int64_t end, int64_t *halo_begin,
                        int64_t *halo_end);
/* first[z] = first cell-sorted position of z-layer z of the grid's cells, z = 0 .. *n_layers (first[*n_layers] = n);
 * `first` (host, nullable) has room for `cap` entries.  A block build keeps the table for the WHOLE replicated cloud
 * (it comes out of its per-layer histogram), so every rank can work out every rank's block, halo and the rows two
 * ranks exchange (shot_fpfh_amd/sharding.py) without talking to anybody. */
int sf_cloud_layer_table(sf_ctx *ctx, sf_cloud *cloud, int64_t *first, int64_t cap, int64_t *n_layers);

/* ---- radius search: replaces KDTree.query_radius (kernels K2 count / fill) --------------
 * Inclusion rule of sklearn's euclidean KDTree: ((dx*dx + dy*dy) + dz*dz) <= r*r in float64,
 * evaluated without FMA, self-match included.
 * sf_radius_search:        m arbitrary query points (shot_parallelization.py:167-169,
 *                          pca_based_descriptors.py:48).
 * sf_radius_search_self:   the cloud's own points as queries (fpfh.py:28-30); [begin, end) is a
 *                          range of CELL-SORTED positions (0, n = everything), which is how a
 *                          multi-GPU shard selects its block of queries.
 * sf_nbrs_export returns the lists in the caller's numbering, ascending inside each list, with
 * distances sqrt(d2) when `dist` is non-NULL (KDTree return_distance=True). Host pointers only. */
sf_nbrs *sf_radius_search(sf_ctx *ctx, sf_cloud *cloud, const double *queries, int64_t m, double radius,
                          int flags);
sf_nbrs *sf_radius_search_self(sf_ctx *ctx, sf_cloud *cloud, double radius, int64_t begin, int64_t end);
/* k nearest neighbours: replaces KDTree.query(Q, k=k, return_distance=False) (pca_based_descriptors.py:46).
 * Every list has exactly k entries, nearest first (ties: lower cell-sorted position).  1 <= k <= n (k <= 1984: the k best
 * are kept in LDS during one sweep; beyond: count / fill / segmented sort through global memory). */
sf_nbrs *sf_knn_search(sf_ctx *ctx, sf_cloud *cloud, const double *queries, int64_t m, int k, int flags);
/* Caller-supplied neighbourhoods: ShotMultiprocessor.compute_local_rf / compute_descriptor work on the lists they are HANDED --
 * support[neighborhoods[i]], shot_parallelization.py:46-84, 86-133 -- whatever made them (KDTree.query_radius of another radius,
 * KDTree.query, a selection of the caller's).  sf_nbrs_import makes a list set of them that sf_shot_lrf / sf_shot / sf_normals /
 * sf_pca consume like a search result.  queries: m x 3 (row i = keypoint i); offsets: m + 1 ascending from 0; idx:
 * offsets[m] point indices in the numbering of sf_cloud_upload (each in 0 .. n-1, else SF_ERR_ARG through NULL + sf_last_error);
 * radius: the value get_local_rf / compute_single_shot_descriptor are called with (shot.py:16-48, 175-306) -- it enters their
 * formulas and filters nothing.  flags: SF_HOST, or SF_IN_DEVICE with all three arrays on the device.  Like every list set, the
 * result is bound to the cloud's current grid: use it before the next search with another radius (consumers return
 * SF_ERR_STATE otherwise). */
sf_nbrs *sf_nbrs_import(sf_ctx *ctx, sf_cloud *cloud, const double *queries, int64_t m, const int64_t *offsets,
                        const int64_t *idx, double radius, int flags);
/* non-owning view of queries [first, first+count) of `nbrs` (free it before the parent).  sf_nbrs_total of a view is -1;
 * sf_nbrs_export serves a view of a self search (a first call with idx == NULL returns the offsets: offsets[count] sizes idx
 * and dist), which is how a sample of a search too large for the host is read. */
sf_nbrs *sf_nbrs_slice(sf_ctx *ctx, sf_nbrs *nbrs, int64_t first, int64_t count);
int64_t sf_nbrs_num_queries(const sf_nbrs *nbrs);
int64_t sf_nbrs_total(const sf_nbrs *nbrs);
int64_t sf_nbrs_max_count(const sf_nbrs *nbrs);
/* the longest list over EVERY rank's searches when sf_comm_collective_stats is on (else = sf_nbrs_max_count) */
int64_t sf_nbrs_max_count_all(const sf_nbrs *nbrs);
int sf_nbrs_export(sf_ctx *ctx, sf_cloud *cloud, sf_nbrs *nbrs, int64_t *offsets /* m+1 */,
                   int32_t *idx /* total */, double *dist /* nullable, total */);
/* For tests and A/B runs.  sf_nbrs_export_raw: the list set as the search left it -- count and offset (m + 1 each) word for word,
 * and, with idx non-NULL, the lists packed end to end in their stored order (cell-sorted positions).  sf_k2_debug_paths: with
 * SF_K2_SHARED=2 in the environment the single sweep counts its waves by path; out[0] = waves that swept the union of their four
 * queries' windows once, out[1] = waves that swept query by query, since the previous call. */
int sf_nbrs_export_raw(sf_ctx *ctx, sf_cloud *cloud, sf_nbrs *nbrs, int32_t *count, int64_t *offset, int32_t *idx);
int sf_k2_debug_paths(sf_ctx *ctx, int64_t *out /* 2 */);
void sf_nbrs_free(sf_ctx *ctx, sf_nbrs *nbrs);

/* ---- PCA normals: compute_normals radius branch (pca_based_descriptors.py:15-59), K3 ----
 * `nbrs` = lists of the query points. pre (m x 3, nullable) = pre_computed_normals. Without it the
 * sign is the one LAPACK dsyevd returns for the lower-triangle covariance (emulated on device). */
/* compute_normals(query_points, cloud_points, radius=...) -- pca_based_descriptors.py:29-59, the radius branch (:48) -- in ONE
 * sweep: the neighbour lists are never materialised (the hits of the candidate sweep are reduced to the covariance in LDS).
 * queries == NULL: the cloud's own points at cell-sorted positions [begin, end) (row i of `out` = position begin + i; m is
 * ignored); else m coordinate queries, rows in the caller's order.  `pre` (nullable): pre_computed_normals, m x 3.
 * Bit-identical to sf_radius_search(_self) followed by sf_normals. */
int sf_normals_radius(sf_ctx *ctx, sf_cloud *cloud, const double *queries, int64_t m, int64_t begin, int64_t end, double radius,
                      const double *pre, double *out /* m x 3 */, int flags);
int sf_normals(sf_ctx *ctx, sf_cloud *cloud, sf_nbrs *nbrs, const double *pre, double *out /* m x 3 */,
               int flags);

/* ---- ISS keypoints (Intrinsic Shape Signatures, Zhong 2009), K10: a detector the reference does not have ----
 * saliency[i] = the smallest eigenvalue e3 of the covariance of the ball of salient_radius around point i (the very numbers
 * compute_normals(radius=) decomposes; eigenvalues e1 >= e2 >= e3), or -1.0 unless the ball holds at least min_neighbors points
 * (i included), e2 / e1 < gamma_21, e3 / e2 < gamma_32, e1 > 0, e2 > 0 and e3 > 1e-12 e1 (a fixed floor: an exactly flat ball
 * must not become salient through the rounding of a sum).  Rows in the CALLER's point order, n of them; count (nullable):
 * the ball sizes.  gammas in (0, 1], min_neighbors >= 1.  The pass runs on the grid sf_cloud_build_grid makes for
 * salient_radius (rebuilt if the cloud carries another one), so its bits do not depend on earlier searches.
 * flags: SF_OUT_DEVICE = saliency / count are device pointers. */
int sf_iss_saliency(sf_ctx *ctx, sf_cloud *cloud, double salient_radius, double gamma_21, double gamma_32, int min_neighbors,
                    double *saliency /* n */, int32_t *count /* nullable, n */, int flags);
/* Non-maximum suppression of ANY per-point score (caller order, n values) -- ISS saliencies and Harris responses (K23) alike:
 * point i is selected <=> score[i] > 0, the ball of non_max_radius around it holds at least min_neighbors points, and none of
 * them has a strictly larger score (exact float64 comparisons: points that tie are all kept).  selected (room for n): the
 * int64 indices in ascending caller order; *n_selected (host): how many.  flags: SF_IN_DEVICE = score is a device pointer,
 * SF_OUT_DEVICE = selected is one. */
int sf_iss_select(sf_ctx *ctx, sf_cloud *cloud, const double *saliency /* n */, double non_max_radius, int min_neighbors,
                  int64_t *selected /* n */, int64_t *n_selected, int flags);
/* sf_iss_saliency followed by sf_iss_select without the saliency leaving the device; bit-identical to the two calls.
 * saliency (nullable, n): receives the scores; flags: SF_OUT_DEVICE = saliency and selected are device pointers. */
int sf_iss_keypoints(sf_ctx *ctx, sf_cloud *cloud, double salient_radius, double non_max_radius, double gamma_21, double gamma_32,
                     int min_neighbors, double *saliency /* nullable, n */, int64_t *selected /* n */, int64_t *n_selected,
                     int flags);
/* ---- Harris 3D keypoints (K23): the detector of pcl::HarrisKeypoint3D on the normals; the reference has none ----
 * With B the ball of `radius` around point i (i included, |p_j - p_i|^2 <= radius^2), k = |B| and C = (1 / k) sum over B of
 * n_j n_j^T (the normals as uploaded: not normalised, not centred, their sign does not matter):
 *   SF_HARRIS_HARRIS     0.04 + det C - 0.04 trace(C)^2 (= det C for unit normals)
 *   SF_HARRIS_NOBLE      det C / trace C
 *   SF_HARRIS_LOWE       det C / trace(C)^2
 *   SF_HARRIS_TOMASI     the smallest eigenvalue of C
 *   SF_HARRIS_CURVATURE  e3 / (e1 + e2 + e3), e1 >= e2 >= e3 the eigenvalues of the mean-centred POSITION covariance of B (the
 *                        numbers sf_iss_saliency decomposes; needs no normals)
 * response[i] = that value, or -1.0 when k < min_neighbors, the trace is not above 0, the matrix is numerically rank-deficient
 * (det <= 1e-12 trace^3; tomasi: lambda_min <= 1e-12 trace; curvature: e3 <= 1e-12 e1) or the value is not > threshold (a NaN
 * is not).  threshold >= 0 and finite, min_neighbors >= 1, else SF_ERR_ARG; a method that needs normals on a cloud without them:
 * SF_ERR_STATE.  count (nullable): the ball sizes; tensor (nullable, n x 6): C as xx yx zx yy zy zz -- for SF_HARRIS_CURVATURE
 * the position covariance.  Everything in the caller's point order.  The pass runs on the grid sf_cloud_build_grid makes for
 * `radius` (rebuilt if the cloud carries another one), so its bits do not depend on earlier searches.
 * flags: SF_OUT_DEVICE = response / count / tensor are device pointers.
 * Non-maximum suppression of a response array is sf_iss_select: it serves both detectors. */
enum { SF_HARRIS_HARRIS = 0, SF_HARRIS_NOBLE = 1, SF_HARRIS_LOWE = 2, SF_HARRIS_TOMASI = 3, SF_HARRIS_CURVATURE = 4 };
int sf_harris_response(sf_ctx *ctx, sf_cloud *cloud, double radius, int method, double threshold, int min_neighbors,
                       double *response /* n */, int32_t *count /* nullable, n */, double *tensor /* nullable, n x 6 */, int flags);
/* sf_harris_response followed by sf_iss_select(non_max_radius) without the response leaving the device; bit-identical to the
 * two calls.  response (nullable, n): receives the scores; flags: SF_OUT_DEVICE = response and selected are device pointers. */
int sf_harris_keypoints(sf_ctx *ctx, sf_cloud *cloud, double radius, double non_max_radius, int method, double threshold,
                        int min_neighbors, double *response /* nullable, n */, int64_t *selected /* n */, int64_t *n_selected,
                        int flags);
/* ---- Outlier removal (K20): the filters PCL and Open3D run in front of the normals; the reference has neither ----
 * Statistical: mean[i] = (sum of the distances from point i to its k + 1 nearest cloud points) / k -- the nearest is the point
 * itself or an exact duplicate, distance 0 -- i.e. the mean distance to the k nearest OTHER points; mu = sum(mean) / n,
 * sigma = sqrt(sum((mean - mu)^2) / (n - 1)), threshold = mu + std_ratio sigma; point i is kept <=> mean[i] <= threshold.
 * n >= 2, 1 <= k <= n - 1, std_ratio finite.  sf_knn_mean_distance: mean in the CALLER's point order (the self query of
 * sf_knn_search at k + 1, which builds its own grid, and one pass over its lists: the bits depend on the cloud and k alone).
 * flags: SF_OUT_DEVICE = mean is a device pointer. */
int sf_knn_mean_distance(sf_ctx *ctx, sf_cloud *cloud, int k, double *mean /* n */, int flags);
/* sf_knn_mean_distance, the two statistics (fixed-order sums: a call repeats bit for bit) and the selection, nothing leaving
 * the device in between; bit-identical to the separate steps.  mean (nullable, n): receives the mean distances; stats (host,
 * nullable, 3): mu, sigma, threshold -- the very threshold the mask was taken against; selected (room for n): the kept int64
 * indices in ascending caller order; *n_selected (host): how many.  Behind the search the call waits for the device once, at
 * its end (a host `selected` receives all n slots then, the first *n_selected of them meaningful).
 * flags: SF_OUT_DEVICE = mean and selected are device pointers. */
int sf_outliers_statistical(sf_ctx *ctx, sf_cloud *cloud, int k, double std_ratio, double *mean /* nullable, n */,
                            double *stats /* host, 3: mu, sigma, threshold */, int64_t *selected /* n */, int64_t *n_selected,
                            int flags);
/* Radius: count[i] = the size of the ball of `radius` around point i, i included (the inclusion rule of sf_radius_search; K2's
 * count sweep, no lists), caller order; point i is kept <=> count[i] - 1 >= min_neighbors.  radius > 0 and finite,
 * min_neighbors >= 0.  The sweep runs on the grid sf_cloud_build_grid makes for `radius` (rebuilt if the cloud carries another).
 * flags: SF_OUT_DEVICE = count (sf_outliers_radius: nullable) and selected are device pointers. */
int sf_ball_counts(sf_ctx *ctx, sf_cloud *cloud, double radius, int32_t *count /* n */, int flags);
int sf_outliers_radius(sf_ctx *ctx, sf_cloud *cloud, double radius, int min_neighbors, int32_t *count /* nullable, n */,
                       int64_t *selected /* n */, int64_t *n_selected, int flags);
/* Local PCA of every query's neighbourhood, same kernel (K3) with the full decomposition as output: replaces
 * the per-point loops of compute_sphericity / compute_pca_based_basic_features (pca_based_descriptors.py:60-73,
 * 150-187, via pca() :15-26) and compute_local_pca_with_moments (:75-146).  eigenvalues: ascending, m x 3.
 * eigenvectors: m x 3 x 3 row-major exactly as numpy.linalg.eigh returns them (column k = eigenvector k, LAPACK
 * dsyevd signs).  moments (nullable, m x 8): |mean(c V^T)| (3), mean((c V^T)^2) (3), mean(c_z), mean(c_z^2) with c
 * the neighbours centred on their barycentre (:121-144).  The feature formulas on top stay on the host. */
int sf_pca(sf_ctx *ctx, sf_cloud *cloud, sf_nbrs *nbrs, double *eigenvalues /* m x 3 */,
           double *eigenvectors /* m x 9 */, double *moments /* nullable, m x 8 */, int flags);
/* numpy.linalg.eigh of m symmetric 3 x 3 matrices given by their lower triangles, elementwise: the device function K3, K4 and
 * the ISS saliency solve with (LAPACK dsyevd's values, eigenvector order AND signs for max|a| in [1.0010415475915505e-146,
 * 9.989595361011175e+145]; outside it LAPACK rescales the matrix first and this function does not).  w: ascending;
 * v[9 i + 3 r + k] = component r of eigenvector k of matrix i, as sf_pca stores them.  A test hook: one matrix per lane.
 * m == 0 returns at once.  flags: SF_IN_DEVICE = lower is a device pointer, SF_OUT_DEVICE = w and v are. */
int sf_eigh3(sf_ctx *ctx, const double *lower /* m x 6: a11 a21 a31 a22 a32 a33 */, int64_t m, double *w /* m x 3 */,
             double *v /* m x 9 */, int flags);

/* ---- SHOT --------------------------------------------------------------------------------
 * sf_shot_lrf (K4): get_local_rf (shot.py:16-48) for every query of `nbrs`; radius = the search
 *   radius of `nbrs`.  lrf is m x 9, row-major 3x3 with COLUMNS x, y, z (shot.py:48).
 * sf_shot (K5): compute_single_shot_descriptor (shot.py:175-306) incl. the last-writer-wins
 *   semantics of the ten fancy-index "+=" statements (shot.py:244-298).  out is m x 352.
 *   Neighbours at EQUAL distance (the reference leaves their order to np.argsort, shot.py:218): the ten statements see the
 *   neighbours in one order, ascending distance and among bit-equal distances ascending index in the caller's cloud array,
 *   so among equally far neighbours the one with the largest index writes last -- whatever kernel form serves the keypoint,
 *   for searched and imported lists, in every entry point that computes SHOT rows. */
int sf_shot_lrf(sf_ctx *ctx, sf_cloud *cloud, sf_nbrs *nbrs, double *lrf /* m x 9 */, int flags);
int sf_shot(sf_ctx *ctx, sf_cloud *cloud, sf_nbrs *nbrs, const double *lrf /* m x 9 */, int normalize,
            int64_t min_neighborhood_size, double *out /* m x 352 */, int flags);
/* compute_descriptor_single_scale in one call (shot_parallelization.py:135-183): frames and descriptors from the
 * same lists; the frame's sign votes are fused into K5.  lrf (m x 9, nullable) receives the frames. */
int sf_shot_single_scale(sf_ctx *ctx, sf_cloud *cloud, sf_nbrs *nbrs, int normalize, int64_t min_neighborhood_size,
                         double *lrf /* m x 9, nullable */, double *out /* m x 352 */, int flags);

/* get_azimuth_idx (shot.py:51-70), elementwise: octant 0..7 of (x, y), a boundary ray belonging to the LOWER octant
 * (+x -> 3, +y -> 5, -x -> 7, -y -> 1, diagonals 4 / 6 / 0 / 2, origin -> 0).  The device function K5 bins with. */
int sf_azimuth_idx(sf_ctx *ctx, const double *x, const double *y, int64_t n, int64_t *idx, int flags);
/* compute_shot_descriptor, the reference's serial variant (shot.py:310-499; "debug only", not in descriptors.__all__):
 * per keypoint the gate `#(rho > 0) > min_neighborhood_size` (:360), the frame from the neighbours at NON-ZERO distance
 * only (:361-363 -- the keypoint and its duplicates neither weigh in the covariance normaliser nor vote), the ten
 * statements of sf_shot -- with sf_shot's order among neighbours at equal distance (ascending index in the caller's cloud
 * array) -- and a row that is always L2-normalised (:496-497). */
int sf_shot_serial(sf_ctx *ctx, sf_cloud *cloud, sf_nbrs *nbrs, int64_t min_neighborhood_size, double *out /* m x 352 */,
                   int flags);
/* sf_shot_serial with n_cosine_bins = n, the one bin count the reference lets a caller change (shot.py:316, 328): rows of 32 n
 * bins, (cosine, azimuth, elevation, shell) in C order, the cosine bin rint((cosine + 1) n / 2 - 0.5) and its neighbour bin
 * wrapped modulo n (:386-401).  1 <= n <= SF_SHOT_MAX_COSINE_BINS, else SF_ERR_ARG; every n, 11 included, runs K4 with the
 * zero-distance neighbours left out and then a kernel of its own (shot_bins.hip), not K5.  Returns SF_ERR_BIN_RANGE when a
 * neighbour of a keypoint that passes the gate has a clipped cosine of exactly +1 with n even (rint(n - 0.5) = n: the reference
 * raises IndexError for the whole call); `out` is then undefined.  flags: SF_HOST, or SF_OUT_DEVICE with `out` on the device.
 * The call waits for its kernels (it reads the range flag back). */
int sf_shot_serial_bins(sf_ctx *ctx, sf_cloud *cloud, sf_nbrs *nbrs, int64_t n_cosine_bins, int64_t min_neighborhood_size,
                        double *out /* m x 32 n */, int flags);

/* ---- Unique Shape Context (K21; Tombari, Salti, Di Stefano 2010, pcl::UniqueShapeContext; the reference has none) ----------
 * Per keypoint a histogram of its neighbours' offsets in the frame of sf_shot_lrf over L azimuth x K elevation x J log-radial
 * bins, bin (l, k, j) at (l K + k) J + j of a row of D = L K J doubles: row[b] = (the exactly rounded sum of the density
 * weights of the neighbours in bin b) vol[b].  L even and >= 2, K >= 1, J >= 1, D <= SF_USC_MAX_BINS, 0 < min_radius < radius.
 * sf_usc_tables (host only, no context): what decides a bin, and the bin weights -- e2[J + 1], squared radial edges from
 *   min_radius^2 to radius^2 in equal steps of log r; ca, sa [L / 2] = cos, sin(2 pi i / L); q[K + 1] = ct |ct| of
 *   ct = cos(pi i / K); vol[D] = 1 / cbrt(bin volume).  A neighbour at offset d, r2 = |d|^2 > 0 (zero: skipped), (lx, ly, lz)
 *   in the frame: j = #{1 <= i < J: r2 >= e2[i]}; h = ly < 0 or (ly == 0 and lx < 0), (u, v) = h ? (-lx, -ly) : (lx, ly),
 *   l = #{1 <= i < L / 2: ca[i] v - sa[i] u >= 0} + h L / 2; k = #{1 <= i < K: lz |lz| <= q[i] r2}; unfused float64.
 * sf_usc_weights: weight[i] = 1.0 / (number of cloud points within density_radius of point i, itself included), n doubles in
 *   the caller's order.  It REBUILDS the grid for density_radius: call it before the search whose lists sf_usc is given (lists
 *   of an earlier grid are refused with SF_ERR_STATE).  flags: SF_OUT_DEVICE = weight is a device pointer.
 * sf_usc: the rows of the queries of `nbrs`, whose radius is R.  lrf (m x 9, nullable): the frames, as sf_shot_lrf lays them
 *   out; NULL: K4 on these very lists.  weight: n doubles in the caller's order, each 1 / c of an integer 1 <= c < 2^22 (any
 *   double in [2^-22, 1] is summed exactly).  normalize != 0: rows divided by their L2 norm.  A keypoint with at most
 *   min_neighborhood_size neighbours at non-zero distance gets a row of zeros.  Returns SF_ERR_ARG when a weight lies outside
 *   [2^-22, 1] or a list has 2^24 entries or more; `out` is then undefined.  flags: SF_IN_DEVICE = lrf and weight are device
 *   pointers, SF_OUT_DEVICE = out is.  The call waits for its kernel (it reads the error word back). */
int sf_usc_tables(double radius, double min_radius, int64_t azimuth_bins, int64_t elevation_bins, int64_t radius_bins,
                  double *e2 /* J + 1 */, double *ca /* L / 2 */, double *sa /* L / 2 */, double *q /* K + 1 */, double *vol /* L K J */);
int sf_usc_weights(sf_ctx *ctx, sf_cloud *cloud, double density_radius, double *weight /* n */, int flags);
int sf_usc(sf_ctx *ctx, sf_cloud *cloud, sf_nbrs *nbrs, const double *lrf /* m x 9, nullable: K4 on these lists */,
           const double *weight /* n */, double min_radius, int64_t azimuth_bins, int64_t elevation_bins, int64_t radius_bins,
           int normalize, int64_t min_neighborhood_size, double *out /* m x L K J */, int flags);

/* ---- Point Feature Histograms (K22; Rusu et al. 2008, pcl::PFHEstimation; the reference has only its fast form, FPFH) --------
 * Per keypoint a histogram over S x S x S bins (S = n_bins, 1 <= S <= SF_PFH_MAX_BINS) of the Darboux angles of EVERY unordered
 * pair of the k entries of its list: the pair with bins (b1, b2, b3) of (theta, alpha, phi) at b1 + S b2 + S^2 b3 of a row of
 * S^3 doubles, row[b] = (100.0 count[b]) / (k (k - 1) / 2); zeros for k < 2.  Bin contents are integers: a row is exact, a
 * function of the cloud alone (not of the order of a list or of the cloud), and a call repeats bit for bit.
 * sf_pfh_tables (host only, no context): what decides a bin, S + 1 entries each, the interior ones 1 .. S - 1 used --
 *   q = c |c| of c[i] = -1 + 2 i / S; ca, sa = cos, sin of e[i] = -pi + 2 pi i / S ((1, 0) exactly where e[i] = 0); g = the sign
 *   of e[i].  A pair {s, t}, unfused float64: d = p_t - p_s, d2 = |d|^2 (zero: skipped); a_s = n_s.d, a_t = -(n_t.d); the source
 *   is the one with the larger |a|, then the larger a, then the point first in (x, y, z) order; t the source: d := -d.  n1 the
 *   source's normal, n2 the other, num3 the source's a; v = d x n1, v2 = |v|^2 (zero: skipped); num2 = v.n2; w = n1 x v;
 *   a = w.n2; B = (n1.n2) sqrt(v2), B := 1 where a = B = 0.  b3 = #{i: num3 |num3| >= q[i] d2}, b2 = #{i: num2 |num2| >= q[i] v2},
 *   b1 = #{i: theta = atan2(a, B) >= e[i]} decided by X_i = (ca[i] a - sa[i] B >= 0) and up = (a >= 0): up or X_i where g[i] < 0,
 *   up and X_i where g[i] > 0, up where g[i] = 0.  The whole statement: tests/pfh_numpy.py.
 * sf_pfh: the rows of the queries of `nbrs` (a radius search, or sf_nbrs_import).  The cloud must have normals (sf_cloud_upload
 *   or sf_cloud_set_normals): SF_ERR_STATE otherwise.  Returns SF_ERR_ARG when a list has 65 536 entries or more (its pairs
 *   would not fit the 32-bit counters); `out` is then undefined.  flags: SF_OUT_DEVICE = out is a device pointer.  The call
 *   waits for its kernel (it reads the error word back).  Work is quadratic in the list length: k (k - 1) / 2 pairs of about a
 *   hundred float64 operations per keypoint. */
int sf_pfh_tables(int64_t n_bins, double *q /* S + 1 */, double *ca /* S + 1 */, double *sa /* S + 1 */, int32_t *g /* S + 1 */);
int sf_pfh(sf_ctx *ctx, sf_cloud *cloud, sf_nbrs *nbrs, int64_t n_bins, double *out /* m x S^3 */, int flags);

/* ---- Spin images (K24; Johnson, Hebert 1999, pcl::SpinImageEstimation; the reference has none) --------------------------------
 * Per keypoint p with axis n (its normal, used as given: neither normalised nor centred) a 2-D image over the cylindrical
 * coordinates of its neighbours about the line through p along n: alpha, the distance from the line, and beta, the signed height
 * along it.  W = image_width, 1 <= W <= SF_SPIN_MAX_WIDTH; the signed image has (W + 1) x (2 W + 1) nodes, the unsigned one
 * (|beta|) (W + 1) x (W + 1); node (iu, iv) at iu NV + iv of a row of D = (W + 1) NV doubles.  The image covers the cylinder of
 * radius and half-height R / sqrt 2, inscribed in the search ball of radius R.  No local reference frame.
 * sf_spin_scale (host only, no context): *inv_bin = (W sqrt(2.0)) / radius, bins per unit length (PCL's bin_size = R / W / sqrt 2).
 * A list entry at x with normal m, unfused float64: d = x - p, d2 = (dx dx + dy dy) + dz dz, beta = (nx dx + ny dy) + nz dz,
 *   a2 = d2 - beta beta (0 when negative), alpha = sqrt(a2) correctly rounded, u = alpha inv_bin, t = beta inv_bin (signed) or
 *   |beta| inv_bin.  It contributes iff d2 > 0, u <= W, |t| <= W and, with use_min_cos, c >= min_cos (signed) or |c| >= min_cos of
 *   c = (nx mx + ny my) + nz mz; a NaN contributes nothing.  v = t + W (signed) or t.  With iu = floor(u), qu = floor((u - iu) 65536)
 *   and the same for v, it adds the INTEGER weights (65536 - qu)(65536 - qv), qu (65536 - qv), (65536 - qu) qv, qu qv to nodes
 *   (iu, iv), (iu + 1, iv), (iu, iv + 1), (iu + 1, iv + 1) -- 2^32 in all, a zero weight not added.  Bin contents are integers: a
 *   row is exact, a function of the cloud alone (not of the order of a list or of the cloud), and a call repeats bit for bit.
 *   With c contributing entries: zeros when c <= min_neighborhood_size, else row[b] = (double)count[b] 2^-32, or with
 *   normalize != 0 (double)count[b] / ((double)c 2^32) (the row sums to 1).  The whole statement: tests/spin_numpy.py.
 * sf_spin_images: the rows of the queries of `nbrs` (a radius search, or sf_nbrs_import), whose radius is R.  axes: m x 3, by
 *   query row.  Positions alone suffice unless use_min_cos != 0, which needs the cloud's normals (SF_ERR_STATE without them).
 *   contrib (nullable): c per query.  Returns SF_ERR_ARG for image_width outside [1, SF_SPIN_MAX_WIDTH], a null pointer,
 *   non-finite host axes, min_cos outside [-1, 1], or a list of 2^24 entries or more (`out` is then undefined).
 *   flags: SF_IN_DEVICE = axes is a device pointer, SF_OUT_DEVICE = out and contrib are.  The call waits for its kernel (it reads
 *   the error word back).  Not built: PCL's angular and radial image domains, a rotation axis other than the one given per
 *   keypoint, sharded (block-grid) clouds, compressed (PCA) images. */
int sf_spin_scale(double radius, int64_t image_width, double *inv_bin);
int sf_spin_images(sf_ctx *ctx, sf_cloud *cloud, sf_nbrs *nbrs, const double *axes /* m x 3 */, int64_t image_width,
                   int signed_beta, int use_min_cos, double min_cos, int normalize, int64_t min_neighborhood_size,
                   double *out /* m x D */, int32_t *contrib /* m, nullable */, int flags);

/* ---- a repeated step as ONE launch (HIP graph) -------------------------------------------------------------------------
 * sf_graph_begin .. sf_graph_end capture every device operation the calls in between issue on the context's streams (nothing
 * runs yet) into an executable graph; sf_graph_launch replays it on the main stream.  What is captured must not synchronise with
 * the device: a REPEATED step of the path qualifies (same cloud, radius and buffers: every launch is planned from the previous
 * search's record), a first one does not -- run the step once eagerly and capture only if sf_sync_count() did not move (a
 * capture that hits a wait is invalidated by the runtime: sf_graph_end then returns NULL with its reason).  The arguments of the
 * captured calls (device buffers, sizes) are part of the graph: replay only while they are alive and unchanged.  Launch timers
 * (sf_profile) must be off.  Not part of the reference's API: a host-overhead lever for small, repeated steps (a rank's share
 * of a strong-scaled job). */
typedef struct sf_graph sf_graph;
unsigned long long sf_sync_count(void); /* host waits on a stream made by the library so far, in this process */
int sf_graph_begin(sf_ctx *ctx);
sf_graph *sf_graph_end(sf_ctx *ctx);
int sf_graph_launch(sf_ctx *ctx, sf_graph *graph);
void sf_graph_free(sf_ctx *ctx, sf_graph *graph);

/* ---- FPFH: compute_fpfh_descriptor (fpfh.py:16-117, decorrelated=False) -------------------
 * sf_spfh_create allocates the table for all n cloud points; sf_spfh_compute (K6) fills the rows of
 * the queries of `self_nbrs` (a sf_radius_search_self result); edges = 3 x (n_bins+1) histogram
 * edges exactly as np.histogramdd builds them (np.linspace; fpfh.py:82-87).
 * sf_fpfh (K7) reduces  spfh[kp] + sum_{j, d_j>0} spfh[j]/d_j / k  (fpfh.py:101-116) for keypoints
 * given either as original indices kp_idx (m; needs lists of the whole cloud) or, when kp_idx == NULL,
 * for every query of `self_nbrs` in cell-sorted order (m must equal its query count; with a
 * sf_nbrs_slice view this is how a shard reduces only its own block).
 * sf_spfh_export writes the float64 SPFH table (n x n_bins^3, original numbering).
 * max_count (the largest neighbourhood the table will see, sf_nbrs_max_count; over every rank of a sharded job:
 * sf_nbrs_max_count_all) picks the storage of the integer bin counts: bytes for n_bins <= 5 and lists of at most 65535
 * points -- with a second table for count >> 8 of the points that have more than 255 neighbours, allocated when max_count
 * exceeds 255 --, else 16 bits up to 65535, 32 bits beyond.  Every list-driven entry point dispatches per keypoint by list
 * length: a list of more than 255 points is served by a second launch, it never changes the kernels the others run.
 * On the byte table sf_spfh_compute also records which 16-bin blocks of the rows hold any count; sf_fpfh reads that
 * mask back (8 bytes, once per sf_spfh_compute: it waits for K6 on the context's stream) and, when at most two of the
 * eight blocks do, multiplies only those -- same results, bit for bit. */
sf_spfh *sf_spfh_create(sf_ctx *ctx, sf_cloud *cloud, int n_bins, int64_t max_count);
/* The table for a KNOWN search radius (the `radius` argument of compute_fpfh_descriptor, fpfh.py:19).  alpha = (c x u) . n_j
 * with v not normalised (fpfh.py:60) never exceeds radius * max|n|^2: when that stays inside the one or two central bins of
 * the alpha histogram (an even n_bins has an edge at 0), only those bins' n_bins^2 (2 n_bins^2) slots of a row can ever hold a
 * count.  For n_bins = 6, 7, 8, 9, 11 -- 72 of 216, 49 of 343, 128 of 512, 81 of 729, 121 of 1331 bins: every count whose
 * window fits the 128 columns of a byte row -- the table then keeps exactly that window of bins,
 * one byte each, and the whole byte-table path (packed rows, high bytes, K7 on the matrix cores, the wire image of the
 * exchange) serves these bin counts too; sf_fpfh writes zeros for the bins outside the window.  Without a usable window
 * (radius <= 0, no normals, a larger reach, other bin counts) this IS sf_spfh_create.  sf_spfh_compute fails with
 * SF_ERR_STATE when it is run with a radius that reaches beyond the table's window.  sf_spfh_elem_bytes: 1, 2 or 4. */
sf_spfh *sf_spfh_create_for_radius(sf_ctx *ctx, sf_cloud *cloud, int n_bins, int64_t max_count, double radius);
int sf_spfh_elem_bytes(const sf_spfh *spfh);
int sf_spfh_compute(sf_ctx *ctx, sf_cloud *cloud, sf_nbrs *self_nbrs, sf_spfh *spfh, const double *edges);
/* Extension for callers that want FPFH and SHOT from the SAME self-search lists (both descriptors of config 3 / 5):
 * sf_spfh_compute_moments is sf_spfh_compute that also leaves, per query of `self_nbrs`, the weighted covariance of
 * the SHOT local frame (get_local_rf, shot.py:27-35; 6 doubles c11 c21 c31 c22 c32 c33, device memory) -- the
 * neighbours are gathered once instead of twice.  sf_shot_from_moments is sf_shot_single_scale starting from those
 * moments (eigen-solves, then the fused K5); `nbrs` may be a sf_nbrs_slice view with cov advanced accordingly. */
int sf_spfh_compute_moments(sf_ctx *ctx, sf_cloud *cloud, sf_nbrs *self_nbrs, sf_spfh *spfh, const double *edges,
                            double *cov_dev /* m x 6 */);
int sf_shot_from_moments(sf_ctx *ctx, sf_cloud *cloud, sf_nbrs *nbrs, const double *cov_dev /* m x 6 */, int normalize,
                         int64_t min_neighborhood_size, double *lrf /* m x 9, nullable */, double *out /* m x 352 */,
                         int flags);
/* The two halves of sf_shot_from_moments (device pointers only): the eigen-solves, which leave the raw axes in
 * lrf_dev, and the fused K5, which completes the frames in place and writes the descriptors. */
int sf_lrf_raw_from_moments(sf_ctx *ctx, sf_cloud *cloud, sf_nbrs *nbrs, const double *cov_dev, double *lrf_dev);
int sf_shot_from_raw_lrf(sf_ctx *ctx, sf_cloud *cloud, sf_nbrs *nbrs, double *lrf_dev, int normalize,
                         int64_t min_neighborhood_size, double *out_dev);
int sf_spfh_allgather(sf_ctx *ctx, sf_spfh *spfh, int64_t rows_per_rank); /* RCCL, in place */
/* Neighbour-to-neighbour exchange of SPFH rows in one RCCL send/recv group: operation i sends this rank's rows
 * [send_begin[i], send_end[i]) to rank peer[i] and receives that rank's rows into [recv_begin[i], recv_end[i]) (cell-sorted
 * positions; the two sides of an operation must name equally many rows).  Per row only what K7 reads per neighbour
 * travels (64 B on the byte table with at most two live blocks).  See fpfh.hip. */
int sf_spfh_exchange_rows(sf_ctx *ctx, sf_spfh *spfh, int n_ops, const int *peer, const int64_t *send_begin,
                          const int64_t *send_end, const int64_t *recv_begin, const int64_t *recv_end);
/* The same wire image of rows [begin, end) through HOST memory, for transports other than RCCL: write_back = 0 copies it
 * out of the table into `host` (cap bytes of room), 1 copies it from `host` into the table's rows; *bytes (nullable)
 * receives the image size, and host == NULL only queries it. */
int sf_spfh_rows_image(sf_ctx *ctx, sf_spfh *spfh, int64_t begin, int64_t end, void *host, size_t cap, int write_back,
                       size_t *bytes);
int sf_spfh_export(sf_ctx *ctx, sf_cloud *cloud, sf_spfh *spfh, double *out /* n x nb^3 */, int flags);
void sf_spfh_free(sf_ctx *ctx, sf_spfh *spfh);
int sf_fpfh(sf_ctx *ctx, sf_cloud *cloud, sf_nbrs *self_nbrs, sf_spfh *spfh, const int64_t *kp_idx, int64_t m,
            double *out /* m x nb^3 */, int flags);
/* The frame moments of sf_spfh_compute_moments from K7's weight pass instead of K6's sweep (K6 has no issue slot nor
 * register to spare, K7 has both): sf_fpfh_moments is sf_fpfh over every query of `self_nbrs` (no kp_idx) that also leaves
 * the 6 doubles per query in cov_dev -- bit for bit what sf_spfh_compute_moments leaves there -- so that the table can be
 * computed by the plain sf_spfh_compute.  Only some forms of K7 carry the moments (the byte table with at most two live
 * 16-bin blocks, no list longer than 192 points): sf_fpfh_carries_moments says, from what the host knows and without a
 * launch, whether a call on these lists and this table would (1) or not (0); asked BEFORE sf_spfh_compute it still holds
 * after it unless the data of that pass widens the table's block mask.  sf_fpfh_moments returns SF_ERR_UNSUPPORTED, having
 * launched nothing, when the form does not carry them: the caller then runs sf_spfh_compute_moments and sf_fpfh. */
int sf_fpfh_carries_moments(sf_ctx *ctx, sf_nbrs *self_nbrs, sf_spfh *spfh);
int sf_fpfh_moments(sf_ctx *ctx, sf_cloud *cloud, sf_nbrs *self_nbrs, sf_spfh *spfh, int64_t m, double *out /* m x nb^3 */,
                    double *cov_dev /* m x 6 */, int flags);

/* ---- matching: cdist + argmin (matching.py:47-52, 63-65, 164-168), K8 ---------------------
 * a: m1 x d, b: m2 x d.  idx[i] = first j minimising sqrt(sum_t (a[i,t]-b[j,t])^2), summed left to
 * right in float64 without FMA (scipy's cdist loop); dist (nullable) = that distance; col_idx
 * (nullable, m2) = argmin over axis 0 (for the reciprocity test). */
int sf_match_argmin(sf_ctx *ctx, const double *a, int64_t m1, const double *b, int64_t m2, int64_t d,
                    int64_t *idx, double *dist, int64_t *col_idx, int flags);
/* Two nearest reference rows of every scan row: idx[2i], idx[2i+1] = j1, j2; dist (nullable) = d1, d2
 * (j2 = -1, d2 = +inf when m2 == 1).  n_exact (nullable, host) = rows decided by the exact kernel.
 * flags: SF_HOST, or SF_IN_DEVICE | SF_OUT_DEVICE with a, b, idx, dist on the device.
 * Rows rank by (distance, column), the distance as in sf_match_argmin: j1, d1 are its idx, dist.  A non-finite entry of a or
 * b is refused with SF_ERR_ARG, as is m2 == 0 with m1 > 0. */
int sf_match_top2(sf_ctx *ctx, const double *a, int64_t m1, const double *b, int64_t m2, int64_t d,
                  int64_t *idx, double *dist, int64_t *n_exact, int flags);

/* Multi-scale ("minimum over scales") form of match_descriptors (matching.py:77-136).  a: n_scales x m1 x d,
 * b: n_scales x m2 x d; a_ok / b_ok: n_scales x m bytes, 1 where the row has a non-zero entry at that scale.
 * dist(i,j) = min over scales of (a_ok && b_ok ? euclidean distance : max_val); idx = first arg-min over j. */
/* mask_dev[i] = 1 when row i of the device matrix rows_dev (m x d) has a non-zero entry (np.any(desc, axis=1)). */
int sf_rows_nonzero(sf_ctx *ctx, const double *rows_dev, int64_t m, int64_t d, unsigned char *mask_dev);
/* out_dev row i = row sel_dev[i] of rows_dev (n_rows x d; all device memory), or a zero row where sel_dev[i] < 0: selects a
 * keypoint subset of a resident descriptor matrix, padded to the equal per-rank block an all-gather needs (zero rows are
 * skipped by the matching, matching.py:162-163).  A selection >= n_rows is never dereferenced: its row comes out zero and
 * the next synchronising call on the context (sf_sync, sf_d2h) returns SF_ERR_ARG. */
int sf_rows_gather(sf_ctx *ctx, const double *rows_dev, int64_t n_rows, const int64_t *sel_dev, int64_t m, int64_t d,
                   double *out_dev);
/* flags: SF_HOST, or SF_IN_DEVICE | SF_OUT_DEVICE with every pointer (masks included) on the device -- the form
 * the sharded matching uses with n_scales = 1 and max_val = +inf to skip all-zero descriptors in place. */
int sf_match_argmin_multiscale(sf_ctx *ctx, const double *a, const double *b, int n_scales, int64_t m1, int64_t m2,
                               int64_t d, const unsigned char *a_ok, const unsigned char *b_ok, double max_val,
                               int64_t *idx, double *dist, int flags);

/* Reciprocity test of match_descriptors (matching.py:62-74) when the scan rows are sharded over ranks: with each rank's
 * column arg-min over its own scan block (sf_match_argmin_multiscale, operands swapped) and the all-reduced column minimum
 * (sf_comm_allreduce_min_u64 on the distances' bit patterns), cand[j] = row_offset + local_idx[j] where this rank attains
 * the global minimum of column j, ~0 elsewhere; a second all-reduce(min) of `cand` leaves distance_matrix.argmin(axis=0),
 * first minimum included.  All pointers device memory. */
int sf_match_col_candidates(sf_ctx *ctx, const double *local_dist_dev, const double *global_dist_dev,
                            const int64_t *local_idx_dev, int64_t row_offset, int64_t m, void *cand_dev);

/* K8 while the reference rows are still ARRIVING (a sharded matching: every scan row must see every reference row, and the rows
 * of the other ranks cross xGMI in chunks -- sf_comm_exchange on the context's side stream).  sf_match_stream_begin takes the
 * resident scan rows a (m1 x d, mask a_ok) and the buffer b (m2 x d, mask b_ok) the reference rows will land in, in their final
 * order; b_entry_max: the largest |entry| of ANY reference row (sf_rows_abs_max of the local block, max over the ranks -- any
 * positive value is valid, the quantisation error is measured, a poor one only costs speed); max_ranges: how many
 * sf_match_stream_feed calls will follow.  sf_match_stream_feed(begin, end): rows [begin, end) of b AND of b_ok are now in place
 * (begin a multiple of 64, end a multiple of 64 or m2; every row exactly once, any order): their int8 image is made and the
 * integer pass (match_i8.hip) takes its minima over them for every scan row, on the context's current stream, while the next
 * chunk travels.  sf_match_stream_end: the decision steps over all chunks' minima -- idx / dist as sf_match_argmin_multiscale
 * (n_scales = 1) leaves them, bit for bit; the handle is released.  When the integer pass does not suit the problem (d > 352,
 * most rows without a clear nearest descriptor, SF_MATCH_I8=0) the feeds cost nothing and _end runs the one-shot paths.
 * All pointers device memory. */
typedef struct sf_match_stream sf_match_stream;
sf_match_stream *sf_match_stream_begin(sf_ctx *ctx, const double *a_dev, const unsigned char *a_ok_dev, int64_t m1,
                                       const double *b_dev, const unsigned char *b_ok_dev, int64_t m2, int64_t d,
                                       double b_entry_max, int64_t max_ranges);
int sf_match_stream_feed(sf_ctx *ctx, sf_match_stream *stream, int64_t row_begin, int64_t row_end);
int sf_match_stream_end(sf_ctx *ctx, sf_match_stream *stream, int64_t *idx_dev, double *dist_dev /* nullable */);
void sf_match_stream_abort(sf_ctx *ctx, sf_match_stream *stream);
/* largest |entry| of m x d resident rows (+inf when an entry is not finite) -> *out_host */
int sf_rows_abs_max(sf_ctx *ctx, const double *rows_dev, int64_t m, int64_t d, double *out_host);

/* ---- RANSAC scoring: inlier count of ransac.py:60-67, K9 ----------------------------------
 * a, b: m x 3 matched points; Rt: n_draws x 12 (row-major R, then t); counts ||a R^T + t - b|| <= thr. */
int sf_ransac_score(sf_ctx *ctx, const double *a, const double *b, int64_t m, const double *Rt, int64_t n_draws,
                    double thr, int64_t *inliers, int flags);

/* ---- RANSAC with pre-rejection, device-side Kabsch and a refit over the inliers: K11 (no counterpart in the reference) ----
 * a_dev, b_dev: m x 3 matched points; draws_dev: n_draws x draw_size int64 indices into them (3 <= draw_size <= 8).  All data
 * pointers are DEVICE memory except where a parameter says "host".
 * sf_ransac_hypotheses: per draw one status byte and one row [R row-major (9), t (3)] (zeros unless the status is 0):
 *     0  a transform: R = argmax tr(R H) over SO(3) for the sample's centred cross-covariance H, t = bbar - R abar
 *     1  rejected: some pair i < j of the sample has edge lengths ea = |a_i - a_j|, eb = |b_i - b_j| with
 *        ea < edge_similarity * eb or eb < edge_similarity * ea            (edge_similarity in [0, 1); 0 passes everything)
 *     2  degenerate: s2 + sign(det H) s3 <= 1e-6 s1 for H's singular values s1 >= s2 >= s3 (H = 0 and non-finite input included)
 *     3  an index outside [0, m): never dereferenced, the draw is left out
 *   Asynchronous on the context's stream.
 * sf_ransac_refit_sums: the sums of one Kabsch fit over ALL inliers ||a R^T + t - b|| <= thr (K9's rule, bit for bit) of the
 *   transform Rt (12 host doubles), centroids first, then the centred cross-covariance; block partials are folded in a fixed
 *   order, so a call repeats bit for bit.  sums[24] (host): [0] inlier count, [1..3] abar, [4..6] bbar over the inliers,
 *   [7..15] sum (a - abar)(b - bbar)^T row-major, [16] sum of squared residuals, [17..19] sum a, [20..22] sum b, [23] 0.
 * sf_ransac_prerejective: sf_ransac_hypotheses, the status-0 rows compacted in draw order, sf_ransac_score over them and the
 *   FIRST maximum.  Optional device outputs (NULL: not wanted): status_dev (n_draws), Rt_dev (n_draws x 12: the first n_scored
 *   rows are the compacted transforms), map_dev (n_draws: slot -> draw number, strictly increasing), counts_dev (n_draws: K9's
 *   counts per slot).  result[8] (host): [0] rejected, [1] degenerate, [2] scored draws, [3] the winning draw (-1: nothing was
 *   scored), [4] its inlier count, [5] its slot, [6] draws of status 3 (then the call returns SF_ERR_ARG), [7] 0;
 *   best_Rt[12] (host): the winner's transform. */
#define SF_RANSAC_MIN_DRAW_SIZE 3
#define SF_RANSAC_MAX_DRAW_SIZE 8
int sf_ransac_hypotheses(sf_ctx *ctx, const double *a_dev, const double *b_dev, int64_t m, const int64_t *draws_dev,
                         int64_t n_draws, int draw_size, double edge_similarity, unsigned char *status_dev, double *Rt_dev);
int sf_ransac_refit_sums(sf_ctx *ctx, const double *a_dev, const double *b_dev, int64_t m, const double *Rt /* 12 */, double thr,
                         double *sums /* 24 */);
int sf_ransac_prerejective(sf_ctx *ctx, const double *a_dev, const double *b_dev, int64_t m, const int64_t *draws_dev,
                           int64_t n_draws, int draw_size, double edge_similarity, double thr, unsigned char *status_dev,
                           double *Rt_dev, int64_t *map_dev, int64_t *counts_dev, int64_t *result /* 8 */, double *best_Rt /* 12 */);

/* ---- fast global registration over given matches: K12 (no counterpart in the reference) --------------------------------------
 * Zhou, Park, Koltun (ECCV 2016): a scaled Geman-McClure cost over the matched pairs, minimised by graduated non-convexity -- a
 * fixed number of weighted Gauss-Newton steps on SE(3), no draws.  a_dev, b_dev: m x 3 matched points (DEVICE); sel_dev: NULL (the
 * rows are matches 0 .. k-1, k <= m) or k int64 match ids (DEVICE, duplicates allowed; an id outside [0, m) is never dereferenced
 * and makes the call return SF_ERR_ARG); k >= 3.  With ca, cb the means of the rows, s = max(max |a - ca|, max |b - cb|),
 * x = (a - ca) / s, y = (b - cb) / s and the state R = I, t = 0, mu = 1, `iterations` times:
 *     p = R x + t, r = p - y, l = mu / (mu + r.r), w = l^2, J = [-[p]x | I]:  A = sum w J^T J, g = sum w J^T r,
 *     E = sum (w r.r + mu (l - 1)^2), W = sum w;  A xi = -g by LDL^T;  R <- exp([xi_0..2]x) R, t <- exp([xi_0..2]x) t + xi_3..5;
 *     after every decrease_every-th iteration mu <- max(mu / division_factor, (distance_threshold / s)^2).
 *   The sums are block partials folded in a fixed order (no atomics): a call repeats bit for bit.  All launches are queued on the
 *   context's stream without a host wait in between; the call waits once, for the result.
 * sf_fgr_sums: ONE pass at the state given (host, 20: ca (3), cb (3), s, R row-major (9), t (3), mu).  sums[32] (host): [0..20] A's
 *   upper triangle row by row, [21..26] g, [27] E, [28] W, [29] the row count, [30], [31] 0.
 * sf_fgr: the whole optimisation.  Rt[12] (host): R row-major and the denormalised t = s t + cb - R ca.  info[8] (host):
 *   [0] status (0 done; 1 degenerate: a pivot d_j of A's LDL^T was not positive up to rounding, d_j <= 1e-12 A_jj -- the weighted
 *   points do not determine a motion: all on one line, or within about 1e-6 of their extent of one -- and the transform of the
 *   previous iteration is returned; 2 the rows have no extent or are not finite: no transform), [1] iterations
 *   run, [2] final mu, [3] s, [4] E and [5] W of the last pass, [6], [7] 0.  trace (host, nullable): iterations x 4 rows
 *   [mu, E, W, |xi|] of the iterations run, zeros after them.
 *   SF_ERR_ARG: k < 3, iterations < 1, decrease_every < 1, division_factor <= 1, a threshold that is not finite. */
int sf_fgr_sums(sf_ctx *ctx, const double *a_dev, const double *b_dev, int64_t m, const int64_t *sel_dev /* nullable */, int64_t k,
                const double *state /* 20 */, double *sums /* 32 */);
int sf_fgr(sf_ctx *ctx, const double *a_dev, const double *b_dev, int64_t m, const int64_t *sel_dev /* nullable */, int64_t k,
           double distance_threshold, int iterations, int decrease_every, double division_factor, double *Rt /* 12 */,
           double *info /* 8 */, double *trace /* nullable, iterations x 4 */);

/* ---- geometric-consistency filter of a set of matches: K13 (no counterpart in the reference) ----------------------------------
 * A rigid motion keeps lengths: matches i and j can both be true only if |a_i - a_j| and |b_i - b_j| agree within the noise.
 * a_dev, b_dev: m x 3 matched points (DEVICE), m <= 2^31 - 1.  In unfused float64, in this order:
 *     dp(i,j) = sqrt(((ax_i - ax_j)^2 + (ay_i - ay_j)^2) + (az_i - az_j)^2),  dq(i,j) the same on b;
 *     compat(i,j) = i != j and |dp - dq| <= distance_threshold and min(dp, dq) >= min_edge     (any comparison with a NaN is
 *     false: a row that is not finite is compatible with nothing);
 *     degree[i] = #{ j : member[j] and compat(i,j) }.
 *   Every result is an integer decided in float64 and summed with integer adds: exact, and the same on every call.
 * sf_consistency_degree: degree_out_dev (m uint32) over the columns j with member_dev[j] != 0 (m bytes; NULL: all columns).
 *   Asynchronous on the context's stream.
 * sf_consistency_group: degree_dev <- the degree over all columns; seed = the LOWEST index among its maxima; member_dev[j] <-
 *   compat(seed, j), member_dev[seed] <- 1; g = sum member; group_degree_dev <- the degree over the member columns.  Five
 *   launches queued without a host wait in between; the call waits once, for info (host, 4 int64): [0] seed, [1] its degree,
 *   [2] g, [3] status (0: a group; 1: no compatible pair -- then seed = -1, g = 0, member and group_degree are all zero).
 *   SF_ERR_ARG: a NULL pointer (but member_dev of sf_consistency_degree), m < 0, m > 2^31 - 1, a distance_threshold or min_edge that
 *   is negative or not finite.  m = 0: SF_OK, nothing is written. */
int sf_consistency_degree(sf_ctx *ctx, const double *a_dev, const double *b_dev, int64_t m,
                          const unsigned char *member_dev /* nullable */, double distance_threshold, double min_edge,
                          unsigned *degree_out_dev);
int sf_consistency_group(sf_ctx *ctx, const double *a_dev, const double *b_dev, int64_t m, double distance_threshold,
                         double min_edge, unsigned *degree_dev, unsigned char *member_dev, unsigned *group_degree_dev,
                         int64_t *info /* 4 */);

/* ---- second-order consistency of a set of matches (SC2; Chen, Sun, Yang, Tao, CVPR 2022): K14 ---------------------------------
 * With compat(i,j) exactly as above:  C[i][j] = 1 if compat(i,j) else 0 (symmetric, zero diagonal);
 *     s2[i] = sum_j C[i][j] sum_k C[i][k] C[j][k]       -- the pairs (j, k) compatible with i AND with each other, twice the
 *     triangles through i in the compatibility graph.  True matches form a clique, accidental ones do not.
 * The matrix is bytes, 16-byte aligned, m_pad x m_pad row-major with m_pad = SF_SC2_PAD(m) and every byte of the padding zero; m <=
 * SF_SC2_MAX_MATCHES (a 1 GiB matrix, s2 < 2^30).  The m^3 sum is an integer GEMM on the int8 matrix cores: exact.
 * sf_consistency_matrix: cmat_dev (m_pad x m_pad bytes, padding included) <- C.  Asynchronous.
 * sf_consistency_sc2: s2_dev (m uint32) <- s2 of ANY matrix of 0 / 1 bytes in that layout, symmetric or not, with the formula
 *   above (row i against row j, weighted by C[i][j]); other byte values, or a padding that is not zero, are unspecified.
 *   Asynchronous.
 * sf_consistency_sc2_group: the matrix (from the context's pool) and s2_dev; seed = the LOWEST index among the maxima of s2;
 *   member_dev[j] <- compat(seed, j), member_dev[seed] <- 1; g = sum member; group_degree_dev <- the degree over the member
 *   columns, as sf_consistency_group (for a member j other than the seed it is C[seed][j] N[seed][j] + 1).  Queued without a
 *   host wait in between; the call waits once, for info (host, 4 int64): [0] seed, [1] s2[seed], [2] g, [3] status (0: a group;
 *   1: no consistent triple -- then seed = -1, g = 0, member and group_degree are all zero).
 *   SF_ERR_ARG: a NULL pointer, m < 0, m > SF_SC2_MAX_MATCHES (refused before anything is allocated), a distance_threshold or
 *   min_edge that is negative or not finite.  m = 0: SF_OK, nothing is written. */
#define SF_SC2_MAX_MATCHES 32768
#define SF_SC2_TILE 256
#define SF_SC2_PAD(m) (((m) + SF_SC2_TILE - 1) / SF_SC2_TILE * SF_SC2_TILE)
int sf_consistency_matrix(sf_ctx *ctx, const double *a_dev, const double *b_dev, int64_t m, double distance_threshold,
                          double min_edge, unsigned char *cmat_dev);
int sf_consistency_sc2(sf_ctx *ctx, const unsigned char *cmat_dev, int64_t m, unsigned *s2_dev);
int sf_consistency_sc2_group(sf_ctx *ctx, const double *a_dev, const double *b_dev, int64_t m, double distance_threshold,
                             double min_edge, unsigned *s2_dev, unsigned char *member_dev, unsigned *group_degree_dev,
                             int64_t *info /* 4 */);

/* ---- SC2 registration: one fit per second-order seed, ranked by inliers over all matches: K15 (the other half of SC2-PCR) -----
 * With C, s2 and the matrix layout of K14 above; all data pointers are DEVICE memory except result and best_Rt.
 * sf_sc2_seeds: seeds_dev (n_seeds int32) <- the matches of the n_seeds largest s2, s2 descending and position ascending, those
 *   with s2 > 0 only; the slots after the last one hold -1.  Exact (a rank count).  Asynchronous.
 * sf_sc2_seed_rows: rows_dev (n_seeds x m_pad uint32, every entry written) <- row_s[j] = C[seed_s][j] sum_k C[seed_s][k] C[j][k]
 *   for ANY matrix of 0 / 1 bytes in K14's layout, symmetric or not -- an integer GEMM on the int8 matrix cores over tiles of
 *   SF_SC2_SEED_TILE seeds x SF_SC2_TILE columns.  Seeds may repeat and come in any order; a seed of -1, or outside [0, m),
 *   gives a zero row; the padding columns are zero.  sum_j row_s[j] = s2[seed_s].  Asynchronous.
 * sf_sc2_seed_fits: per seed, top = max_j row_s[j]; member j iff j = seed_s or (row_s[j] >= 1 and (double)row_s[j] >=
 *   group_share * (double)top) -- the rule of second_order_consistency_filter; size_dev (n_seeds int32) <- the member count;
 *   the Kabsch fit over the members (centroids first, then the centred cross-covariance; partial sums folded in a fixed order:
 *   a call repeats bit for bit) with the rules and constants of sf_ransac_hypotheses.  status_dev (n_seeds bytes): 0 a transform,
 *   1 fewer than three members, 2 degenerate (no unique rotation, or not finite), 3 no seed in the slot.  Rt_dev (n_seeds x 12:
 *   R row-major, t; zeros unless the status is 0).  Optional (NULL: not wanted): sums_dev (n_seeds x 24, the layout of
 *   sf_ransac_refit_sums over the members, [16] = 0), member_dev (n_seeds x m bytes).  Asynchronous.
 * sf_sc2_registration: sf_consistency_matrix, sf_consistency_sc2, the three calls above, the status-0 transforms compacted in
 *   seed order, sf_ransac_score over them at distance_threshold and the FIRST maximum, queued without a host wait in between; the
 *   call waits once, for the result.  The matrix and the rows (n_seeds x m_pad x 4 bytes) come from the context's pool.  Optional
 *   device outputs (NULL: not wanted): s2_dev (m uint32), seeds_dev, status_dev, size_dev (n_seeds each, as above), Rt_dev
 *   (n_seeds x 12: the first `scored` rows are the compacted transforms, the others zero), map_dev (n_seeds int64: slot -> position
 *   among the seeds, strictly increasing, then -1), counts_dev (n_seeds int64: the inlier count per slot, then -1).
 *   result[8] (host): [0] seeds found, [1] seeds with fewer than three members, [2] degenerate, [3] scored, [4] the winning
 *   seed's match (-1: nothing was scored), [5] its inlier count, [6] its position among the seeds (-1), [7] its consensus size;
 *   best_Rt[12] (host): its transform (zeros when nothing was scored).
 *   SF_ERR_ARG: a NULL pointer that is not optional, m < 0, m > SF_SC2_MAX_MATCHES, n_seeds outside 1 .. SF_SC2_MAX_SEEDS, a
 *   group_share outside (0, 1], a distance_threshold or min_edge that is negative or not finite -- all refused before anything is
 *   allocated.  m = 0: SF_OK, nothing is written. */
#define SF_SC2_MAX_SEEDS 1024
#define SF_SC2_SEED_TILE 64
int sf_sc2_seeds(sf_ctx *ctx, const unsigned *s2_dev, int64_t m, int64_t n_seeds, int *seeds_dev);
int sf_sc2_seed_rows(sf_ctx *ctx, const unsigned char *cmat_dev, int64_t m, const int *seeds_dev, int64_t n_seeds,
                     unsigned *rows_dev);
int sf_sc2_seed_fits(sf_ctx *ctx, const double *a_dev, const double *b_dev, int64_t m, const int *seeds_dev,
                     const unsigned *rows_dev, int64_t n_seeds, double group_share, unsigned char *status_dev, int *size_dev,
                     double *Rt_dev, double *sums_dev /* nullable */, unsigned char *member_dev /* nullable */);
int sf_sc2_registration(sf_ctx *ctx, const double *a_dev, const double *b_dev, int64_t m, double distance_threshold,
                        double min_edge, int64_t n_seeds, double group_share, unsigned *s2_dev, int *seeds_dev,
                        unsigned char *status_dev, int *size_dev, double *Rt_dev, int64_t *map_dev, int64_t *counts_dev,
                        int64_t *result /* 8 */, double *best_Rt /* 12 */);

/* ---- voxel subsampling: grid_subsampling (core/subsampling.py:5-39) and the voxel loop of
 * select_keypoints_with_density_threshold (keypoint_selection.py:80-101) ---------------------------------
 * sf_voxels_build: keys ((p - min p) // voxel).astype(int) with NumPy's floor_divide, voxels ranked in np.unique's
 *   lexicographic key order (stable device sort).  xyz: n x 3, host or (SF_IN_DEVICE) device memory that must stay valid.
 * sf_voxels_count: number of occupied voxels.
 * sf_voxels_inverse: np.unique's `inverse` (voxel rank of every point, n, host).
 * sf_voxels_select: per voxel the point closest to the voxel's barycentre (first minimum) and, optionally, the voxel
 *   populations (np.unique's counts).  `order` (nullable, n, host) is the visiting order of the points, grouped by voxel
 *   in voxel order -- the reference uses np.argsort(inverse), an UNSTABLE sort whose order decides exact distance ties
 *   (every two-point voxel is one); NULL = ascending point index inside a voxel. */
sf_voxels *sf_voxels_build(sf_ctx *ctx, const double *xyz, int64_t n, double voxel_size, int flags);
int64_t sf_voxels_count(const sf_voxels *vox);
int sf_voxels_inverse(sf_ctx *ctx, sf_voxels *vox, int64_t *inverse /* n */);
int sf_voxels_select(sf_ctx *ctx, sf_voxels *vox, const int64_t *order /* nullable, n */, int64_t *selected /* count */,
                     int64_t *counts /* nullable, count */);
void sf_voxels_free(sf_ctx *ctx, sf_voxels *vox);

/* ---- ICP: one iteration's device work (icp.py:64-72, 108-124, 160-183; core/solvers.py:17-18, 38-46) --------
 * sf_icp_accumulate: rows sel_dev[0..m) (or 0..m when NULL) of the resident points pts_dev are moved by Rt (12 host
 *   doubles: R row-major then t; NULL = identity), their nearest reference point found (KDTree.query, k = 1), pairs
 *   with distance <= d_max kept, and the sums of the iteration's solver returned in sums[40] (host):
 *     [0] inlier count, [1..3] sum of inlier points p, [4..6] sum of their neighbours q,
 *     mode 0 (point to point): [8..16] sum (p - pbar)(q - qbar)^T row-major, [17] sum |p - q|^2
 *     mode 1 (point to plane; the cloud needs normals): [8..28] upper triangle of G^T G row by row, [29..34] G^T h,
 *       [35] sum |h|, with g = [p x n, n], h = (q - p) . n;
 *     the rest is zero, and so is everything when no pair is kept.
 * sf_transform_points: p <- p R^T + t in place on resident points (RigidTransform.__getitem__). */
int sf_icp_accumulate(sf_ctx *ctx, sf_cloud *ref, const double *pts_dev, const int64_t *sel_dev, int64_t m, const double *Rt,
                      double d_max, int mode, double *sums /* 40 */);
int sf_transform_points(sf_ctx *ctx, double *pts_dev, int64_t n, const double *Rt /* 12 */);

/* ---- generalized (plane-to-plane) ICP, K16 (Segal, Haehnel, Thrun, RSS 2009; no counterpart in the reference) --------
 * One iteration's device work, the chain of the call above in a third mode.  Every point carries the covariance
 * C = I - (1 - epsilon) n n^T of its unit normal n (a zero normal: C = I; the sign of n does not matter).  The reference
 * cloud needs normals; nrm_dev holds the scan's, one row per row of pts_dev (n x 3 doubles on the device), and a row is
 * reached through sel_dev exactly as its point is (repeated ids allowed).  Rt as above; NULL leaves the normals alone too.
 * For a kept pair (distance <= d_max) with p the moved point, b its neighbour, nb b's normal and m = R n_scan:
 *   S = 2 I - (1 - epsilon) (nb nb^T + m m^T),  M = S^-1 (symmetric adjugate over the determinant),  r = b - p,
 *   J = [-[p]x, I] (3 x 6).
 * sums[40] (host):
 *   [0] pair count, [1..3] sum of p, [4..6] sum of b,
 *   [8..28] upper triangle of H = sum J^T M J, row by row, [29..34] g = sum J^T M r,
 *   [35] sum r^T M r, [36] sum |r|^2; the rest is zero.
 * The Gauss-Newton step is xi = H^-1 g, (rotation vector, translation), applied on the left.  0 < epsilon <= 1. */
int sf_icp_accumulate_gicp(sf_ctx *ctx, sf_cloud *ref, const double *pts_dev, const double *nrm_dev /* n x 3, scan normals */,
                           const int64_t *sel_dev, int64_t m, const double *Rt, double d_max, double epsilon, double *sums /* 40 */);

/* ---- robust losses for all three modes, K17 (no counterpart in the reference) --------
 * The chain of the two calls above -- transform, k = 1 search, the d_max gate, pass A, pass B, one copy back, one wait -- with a
 * weight w = psi(r) / r per kept pair (iteratively reweighted least squares).  mode 0 point to point, 1 point to plane (the
 * reference cloud needs normals), 2 generalized (nrm_dev and epsilon as above; both are ignored in modes 0 and 1, nrm_dev may
 * be NULL there).  The gate is applied first and is unchanged.  The pair's squared residual r2:
 *   mode 0: |q - p|^2     mode 1: h^2, h = (q - p) . n     mode 2: r^T M r, clamped at 0
 * and its weight from `loss` and `scale` = k (positive, finite; in the unit of sqrt(r2): a length in modes 0 and 1, a Mahalanobis
 * distance in mode 2, where a residual h across both surfaces counts as h / sqrt(2 epsilon)), with s = r2 / (k k):
 *   0 none           w = 1
 *   1 Huber          w = 1 for sqrt(r2) <= k, else k / sqrt(r2)
 *   2 Cauchy         w = 1 / (1 + s)
 *   3 Geman-McClure  w = 1 / (1 + s)^2
 *   4 Tukey          w = (1 - s)^2 for s <= 1, else 0
 * sums[48] (host):
 *   [0] pair count, [1..3] sum p, [4..6] sum q            unweighted, as above
 *   [7] sum w
 *   [8..36] the mode's layout above with every FIT term times w: mode 0 [8..16] sum w (p - pw)(q - qw)^T, centred with the
 *           WEIGHTED centroids pw = sum w p / sum w, qw = sum w q / sum w (zero when sum w is 0); mode 1 [8..28] G^T W G,
 *           [29..34] G^T W h; mode 2 [8..28] sum w J^T M J, [29..34] sum w J^T M r.  The residual sums stay unweighted:
 *           [17] sum |p - q|^2 (mode 0), [35] sum |h| (mode 1) or sum r^T M r (mode 2), [36] sum |r|^2 (mode 2)
 *   [40..42] sum w p, [43..45] sum w q, [46] sum w r2
 *   the rest, [47] included, is zero, and so is everything when no pair is kept.
 * sf_icp_accumulate and sf_icp_accumulate_gicp are this call with loss 0: they return its [0..39] with [7] cleared.  So with loss
 * 0, or Huber with k above every residual, [0..39] are their numbers bit for bit, [7] = [0] and [40..45] = [1..6].  SF_ERR_ARG names the offending argument in sf_last_error(). */
int sf_icp_accumulate_robust(sf_ctx *ctx, sf_cloud *ref, const double *pts_dev, const double *nrm_dev /* NULL unless mode 2 */,
                             const int64_t *sel_dev, int64_t m, const double *Rt, double d_max, int mode /* 0, 1, 2 */, double epsilon,
                             int loss /* 0 .. 4 */, double scale, double *sums /* 48 */);

/* ---- the exact k-th smallest of doubles on the device, K18 (no counterpart in the reference) --------
 * sf_select_kth: the rank-th smallest (1-based, 1 <= rank <= n) of keys_dev[0..n) (doubles on the device), by radix selection on
 * the bit patterns: six histogram passes over the keys, no host wait in between, integer atomics only -- a call repeats bit for bit.
 * The order is that of the patterns with the sign bit cleared, np.partition's on non-negative keys: -0.0 orders as zero, +inf
 * above every finite value, the NaNs last.  out[4] (host):
 *   [0] the value (a zero comes back as +0.0), [1] how many keys order below it, [2] how many order at or below it, [3] 0.
 * SF_ERR_ARG names the offending argument in sf_last_error(): n < 1, a rank outside 1 .. n, a null pointer. */
int sf_select_kth(sf_ctx *ctx, const double *keys_dev, int64_t n, int64_t rank, double *out /* 4 */);

/* ---- trimmed ICP for all three modes, K18 (Chetverikov, Stepanov, Krsek 2002/2005; no counterpart in the reference) --------
 * sf_icp_accumulate_robust's chain over the best-fitting share of the pairs only.  With n0 the pairs inside d_max (the gate is
 * applied first and is unchanged) and r2 the mode's squared residual as above (mode 2's clamped term may be -0.0: it orders as zero):
 *   rank = min(n0, max(1, (int64) ceil(trim * (double) n0))),   cut = the rank-th smallest r2 (sf_select_kth's order),
 * a pair is USED iff it is inside d_max and r2 <= cut -- every tie at the cut is used, so the used set does not depend on the
 * order of the pairs and may exceed the rank.  Both sums passes and both folds run over the used pairs; a robust weight is taken
 * over them from the same r2.  Between the search and pass A the chain gains a key pass and the selection; rank and cut are formed
 * and read on the device, and the call still has one host wait, at its end.  trim in (0, 1].
 * sums[48] (host): sf_icp_accumulate_robust's layout with [0] the USED pair count, and
 *   [37] n0, [38] the rank, [47] the cut.
 * With trim == 1.0 no selection is launched: [0..36] and [40..46] are sf_icp_accumulate_robust's bit for bit, [37] = [38] = [0]
 * and [47] = 0.  With no pair inside d_max everything is zero.  SF_ERR_ARG names the offending argument in sf_last_error(). */
int sf_icp_accumulate_trimmed(sf_ctx *ctx, sf_cloud *ref, const double *pts_dev, const double *nrm_dev /* NULL unless mode 2 */,
                              const int64_t *sel_dev, int64_t m, const double *Rt, double d_max, int mode /* 0, 1, 2 */, double epsilon,
                              int loss /* 0 .. 4 */, double scale, double trim /* in (0, 1] */, double *sums /* 48 */);

/* ---- symmetric point-to-plane ICP, K19 (Rusinkiewicz, "A Symmetric Objective Function for ICP", SIGGRAPH 2019; no counterpart in
 * the reference) --------
 * The chain of the calls above in a fourth mode, with sf_icp_accumulate_robust's weight and sf_icp_accumulate_trimmed's share.  The
 * reference cloud needs normals; nrm_dev holds the scan's (required), reached through sel_dev and turned by Rt as in
 * sf_icp_accumulate_gicp.  For a pair inside d_max (the gate is applied first and is unchanged) with p the moved point, b its
 * neighbour, nb b's normal and m = R n_scan:
 *   s = +1 if (m0 nb0 + m1 nb1) + m2 nb2 >= 0, else -1          the sign of either normal cancels
 *   n = 0.5 (nb + s m)                                          the mean normal; a zero row on one side leaves half the other
 *   h = (b - p) . n,  r2 = h h                                  a length: point-to-plane's h for parallel unit normals
 *   c = p + b,  g = [c x n, n]
 * The weight comes from r2, loss and scale as in sf_icp_accumulate_robust; rank, cut and the used pairs from r2 and trim as in
 * sf_icp_accumulate_trimmed.  sums[48] (host), that call's layout with mode 1's slots:
 *   [0] the USED pair count, [1..3] sum p, [4..6] sum b, [7] sum w,
 *   [8..28] upper triangle of sum w g g^T row by row, [29..34] sum w g h, [35] sum |h|, [36] sum |b - p|^2  (both unweighted),
 *   [37] n0, [38] the rank, [40..42] sum w p, [43..45] sum w b, [46] sum w r2, [47] the cut; the rest is zero.
 * The host step: x = solve(sum w g g^T, sum w g h), a = x[0..2], t = x[3..5], theta = atan |a|, R_h the rotation by theta about a;
 * e = a / |a|; the pair of clouds is aligned by p <- R_h (R_h p + cos(theta) t + (1 - cos(theta)) (e . t) e).
 * With trim == 1.0 no selection is launched: [37] = [38] = [0] and [47] = 0.  One host wait, at the end.  With no pair inside d_max
 * everything is zero.  SF_ERR_ARG names the offending argument in sf_last_error(). */
int sf_icp_accumulate_symmetric(sf_ctx *ctx, sf_cloud *ref, const double *pts_dev, const double *nrm_dev /* scan normals, required */,
                                const int64_t *sel_dev, int64_t m, const double *Rt, double d_max, int loss /* 0 .. 4 */, double scale,
                                double trim /* in (0, 1] */, double *sums /* 48 */);

/* ---- multi-GPU: RCCL over xGMI (no counterpart in the reference) --------------------------
 * One process per GPU.  Rank 0 calls sf_comm_unique_id, ships the 128 bytes to the other ranks by
 * any host channel, then every rank calls sf_comm_init.  sf_comm_allgather gathers
 * bytes_per_rank from each rank into recv (rank-major); send may alias recv + rank*bytes_per_rank. */
int sf_comm_unique_id(char id[128]);
int sf_comm_init(sf_ctx *ctx, const char id[128], int nranks, int rank);
int sf_comm_allgather(sf_ctx *ctx, const void *send_dev, void *recv_dev, size_t bytes_per_rank);
/* Grouped point-to-point exchange (ncclSend / ncclRecv in one group): operation i sends send_bytes[i] bytes to rank
 * peer[i] and receives recv_bytes[i] bytes from it; a rank may name itself. */
int sf_comm_exchange(sf_ctx *ctx, int n_ops, const int *peer, const void *const *send_dev, const size_t *send_bytes,
                     void *const *recv_dev, const size_t *recv_bytes);
/* element-wise minimum over the ranks of n unsigned 64-bit words (ncclAllReduce; in place allowed): the column arg-min of
 * a sharded matching travels as packed (distance bits, index) keys */
int sf_comm_allreduce_min_u64(sf_ctx *ctx, const void *send_dev, void *recv_dev, size_t n);
/* on: every radius search of the context also folds its longest-list statistic over all ranks (collective call) */
int sf_comm_collective_stats(sf_ctx *ctx, int on);
int sf_comm_destroy(sf_ctx *ctx);

/* ---- per-kernel timing with HIP events on the ctx stream -------------------------------- */
int sf_profile_enable(sf_ctx *ctx, int on);
int sf_profile_reset(sf_ctx *ctx);
/* time launches of this kernel name only (NULL or "" = all): two event records per launch cost a few microseconds, which a
 * caller timing whole passes may not want on every kernel */
int sf_profile_only(sf_ctx *ctx, const char *name);
/* writes "name launches total_ms\n" lines; returns bytes needed (call with buf == NULL to size) */
int64_t sf_profile_report(sf_ctx *ctx, char *buf, int64_t cap);

#ifdef __cplusplus
}
#endif
#endif /* SHOTFPFH_H */
