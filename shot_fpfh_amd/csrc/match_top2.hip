// match_top2.hip -- K8 top-2: the two nearest reference rows of every scan row with their exact float64 distances (the ratio
// test in front of RANSAC, matching/match.py: ratio_test_matching).
//
// dist(i, j) is the reference's distance (scipy's loop: the float64 sum of (a[i,t] - b[j,t])^2 left to right without FMA, then
// sqrt).  The reference rows of scan row i are ranked by the pair (dist(i, j), j); j1, j2 are the first two.  So j1 and d1 are
// what sf_match_argmin returns (first minimum), and duplicated reference rows give d1 == d2 with j1 < j2.  The order is total:
// every merge below (lanes, tiles, column splits) gives the same pairs in any order, and every path gives the same bits.
//
// Two paths behind the arg-min's size rule (match.hip: match_dispatch):
//  * k_top2_tile: the exact tile kernel of match.hip (64 x 64 tile per workgroup, the descriptor dimension streamed through LDS
//    in slices of 16), keeping (d1, j1, d2, j2) per row; k_top2_merge folds the column splits into the result.
//  * k_top2_gemm: the FP64 matrix-core GEMM of match_gemm.hip on the key s = ||b_j||^2 - 2 a_i . b_j, keeping the three
//    smallest keys and the columns of the first two.  k_top2_decide merges the splits.  When k3 - k2 > tol (the tol of
//    k_match_decide and its argument, match_gemm.hip), every other column's reference distance exceeds those of the columns of
//    k1 and k2 whatever the rounding, so those two are j1 and j2; their scipy-order distances put them in order (a gap between
//    k1 and k2 is not needed).  Other rows (ties among ranks 2 and 3, e.g. duplicated descriptors) are gathered, matched by
//    k_top2_tile and scattered back.
// Roofline: as the arg-min (FP64 matrix cores, 2 m1 m2 d flop); the epilogue only sees keys below the running third.
#include <cfloat>
#include <climits>
#include <cmath>

#include "device_util.h"
#include "match.h"
#include "match_mainloop.h"

namespace {

// ---- exact tile kernel ----------------------------------------------------------------------------------------------------------
constexpr int64_t NONE = INT64_MAX; // an empty slot: (+inf, NONE) ranks after every reference row
constexpr int NONE_L = INT_MAX;     // the same inside a tile (columns relative to the tile's first)

// (da, ja) before (db, jb) in the (dist, column) order
template <typename J>
__device__ __forceinline__ bool top2_lt(double da, J ja, double db, J jb)
{
    return da < db || (da == db && ja < jb);
}

// the first two of a set in the (dist, column) order
template <typename J>
struct top2d {
    double d1, d2;
    J j1, j2;
};
template <typename J>
__device__ __forceinline__ void top2d_insert(top2d<J> &p, double d, J j)
{
    if (top2_lt(d, j, p.d1, p.j1)) { p.d2 = p.d1; p.j2 = p.j1; p.d1 = d; p.j1 = j; }
    else if (top2_lt(d, j, p.d2, p.j2)) { p.d2 = d; p.j2 = j; }
}
// union with the first two (o1 before o2) of a disjoint set
template <typename J>
__device__ __forceinline__ void top2d_merge(top2d<J> &p, double od1, J oj1, double od2, J oj2)
{
    if (top2_lt(od1, oj1, p.d1, p.j1)) {
        if (top2_lt(od2, oj2, p.d1, p.j1)) { p.d2 = od2; p.j2 = oj2; }
        else { p.d2 = p.d1; p.j2 = p.j1; }
        p.d1 = od1; p.j1 = oj1;
    } else if (top2_lt(od1, oj1, p.d2, p.j2)) {
        p.d2 = od1; p.j2 = oj1;
    }
}

// One 64 x 64 tile of dist(i, j) per workgroup, 4 x 4 per thread, from the loop k_match_tile (match.hip) runs.  Partials of
// split s: pd[(2 s + q) m1 + i], pj[(2 s + q) m1 + i] for q = 0, 1 (the first and the second of the split's columns).
__global__ __launch_bounds__(256) void k_top2_tile(const double *__restrict__ a, int64_t m1, const double *__restrict__ b,
                                                   int64_t m2, int64_t d, int64_t tiles_per_split, double *__restrict__ pd,
                                                   int64_t *__restrict__ pj)
{
    __shared__ double As[TK][TM + 1];
    __shared__ double Bs[TK][TN + 1];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int64_t i0 = (int64_t)blockIdx.x * TM;
    const int split = blockIdx.y;
    int64_t jt0, jt1;
    sf_split_tiles(m2, TN, tiles_per_split, jt0, jt1);
    top2d<int64_t> best[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) best[u] = {INFINITY, INFINITY, NONE, NONE};

    for (int64_t jt = jt0; jt < jt1; ++jt) {
        const int64_t j0 = jt * TN;
        double acc[4][4];
        sf_tile_sqdist(As, Bs, a, m1, i0, b, m2, j0, d, acc);
        // per row: the first two of the thread's 4 columns, then of the 16 tx lanes of the row group, then of the running pair
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            top2d<int> t = {INFINITY, INFINITY, NONE_L, NONE_L};
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int jl = tx * 4 + v;
                if (j0 + jl < m2) top2d_insert(t, sqrt(acc[u][v]), jl);
            }
#pragma unroll
            for (int off = 1; off < 16; off <<= 1) {
                const double od1 = __shfl_xor(t.d1, off, 16), od2 = __shfl_xor(t.d2, off, 16);
                const int oj1 = __shfl_xor(t.j1, off, 16), oj2 = __shfl_xor(t.j2, off, 16);
                top2d_merge(t, od1, oj1, od2, oj2);
            }
            top2d_merge(best[u], t.d1, t.j1 == NONE_L ? NONE : j0 + t.j1, t.d2, t.j2 == NONE_L ? NONE : j0 + t.j2);
        }
    }
    if (tx == 0) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t i = i0 + ty * 4 + u;
            if (i < m1) {
                pd[(int64_t)(2 * split) * m1 + i] = best[u].d1;
                pd[(int64_t)(2 * split + 1) * m1 + i] = best[u].d2;
                pj[(int64_t)(2 * split) * m1 + i] = best[u].j1;
                pj[(int64_t)(2 * split + 1) * m1 + i] = best[u].j2;
            }
        }
    }
}

// the column splits of k_top2_tile -> idx[2 i], idx[2 i + 1] (-1 for an empty second slot, m2 == 1), dist (nullable) alike
__global__ void k_top2_merge(const double *__restrict__ pd, const int64_t *__restrict__ pj, int64_t m1, int nsplit,
                             int64_t *__restrict__ idx, double *__restrict__ dist)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m1) return;
    top2d<int64_t> p = {pd[i], pd[m1 + i], pj[i], pj[m1 + i]};
    for (int s = 1; s < nsplit; ++s)
        top2d_merge(p, pd[(int64_t)(2 * s) * m1 + i], pj[(int64_t)(2 * s) * m1 + i], pd[(int64_t)(2 * s + 1) * m1 + i],
                    pj[(int64_t)(2 * s + 1) * m1 + i]);
    idx[2 * i] = p.j1;
    idx[2 * i + 1] = p.j2 == NONE ? -1 : p.j2;
    if (dist) {
        dist[2 * i] = p.d1;
        dist[2 * i + 1] = p.d2;
    }
}

// ---- FP64 matrix-core path --------------------------------------------------------------------------------------------------------
// the three smallest keys of a set and the columns of the first two; ties between keys are broken by arrival, which only the
// columns of equal keys depend on -- a row whose k2 equals k3 is never decided, and the two columns of k1, k2 are re-ordered by
// their exact distances
template <typename J>
struct top3k {
    double k1, k2, k3;
    J j1, j2;
};
template <typename J>
__device__ __forceinline__ void top3k_insert(top3k<J> &t, double s, J j)
{
    if (s < t.k1) { t.k3 = t.k2; t.k2 = t.k1; t.j2 = t.j1; t.k1 = s; t.j1 = j; }
    else if (s < t.k2) { t.k3 = t.k2; t.k2 = s; t.j2 = j; }
    else if (s < t.k3) t.k3 = s;
}
// union with the triple (o1 <= o2 <= o3) of a disjoint set: once o1 and o2 are in, k2 <= o2 <= o3, so o3 can only be third
template <typename J>
__device__ __forceinline__ void top3k_merge(top3k<J> &t, double o1, J oj1, double o2, J oj2, double o3)
{
    top3k_insert(t, o1, oj1);
    top3k_insert(t, o2, oj2);
    t.k3 = fmin(t.k3, o3);
}

// sf_gemm_tile (match_mainloop.h), which is k_match_gemm's loop, with a top-3 epilogue.  Partials of split s: pk[(3 s + q) m1 + i] for
// the keys q = 0, 1, 2, pj[(2 s + q) m1 + i] for the columns of the first two.  The VEC form spills 16 bytes: one loop-invariant
// row address of the staging loads, reloaded once per column tile, and tid_end, reloaded behind the loop; nothing inside the k loop.
template <bool VEC>
__global__ __launch_bounds__(256, 2) void k_top2_gemm(const double *__restrict__ a, int64_t m1, const double *__restrict__ b,
                                                   int64_t m2, int64_t d, const double *__restrict__ nb,
                                                   int64_t tiles_per_split, double *__restrict__ pk, int64_t *__restrict__ pj)
{
    __shared__ __attribute__((aligned(16))) double As[2][GM][LDS_P];
    __shared__ __attribute__((aligned(16))) double Bs[2][GN][LDS_P];
    const int tid = threadIdx.x, lane = tid & 63, wc = (tid >> 6) & 1;
    const int64_t i0 = (int64_t)blockIdx.x * GM;
    const int split = blockIdx.y;
    int64_t jt0, jt1;
    sf_split_tiles(m2, GN, tiles_per_split, jt0, jt1);
    const int l15 = lane & 15;

    int tid_end = tid; // for the hand-over behind the loop: one register kept across it instead of the four pieces of `own`
    asm volatile("" : "+v"(tid_end));
    top3k<int64_t> run = {INFINITY, INFINITY, INFINITY, 0, 0}; // the row this lane owns in its DPP row (as k_match_gemm)

    for (int64_t jt = jt0; jt < jt1; ++jt) {
        const int64_t j0 = jt * GN;
        d4 acc[4][4];
        sf_gemm_tile<VEC>(As, Bs, a, m1, i0, b, m2, j0, d, acc);
        double nbv[4];
        int64_t jcol[4];
        sf_gemm_cols(j0, m2, nb, jcol, nbv);
        // Per row (TI, R): the lane's four keys against the row's running THIRD key (broadcast from its owner with
        // row_newbcast); only a key below it changes the triple, so the butterfly is skipped wave-uniformly for most tiles.
#define SF_TOP3_STEP(CTRL)                                                                                          \
    {                                                                                                               \
        const double o1 = sf_dpp<CTRL>(t.k1), o2 = sf_dpp<CTRL>(t.k2), o3 = sf_dpp<CTRL>(t.k3);                     \
        const int oj1 = sf_dpp<CTRL>(t.j1), oj2 = sf_dpp<CTRL>(t.j2);                                               \
        top3k_merge(t, o1, oj1, o2, oj2, o3);                                                                       \
    }
#define SF_EPI_ROW(TI, R)                                                                                           \
    {                                                                                                               \
        const double thr = sf_dpp<0x150 + 4 * (TI) + (R)>(run.k3);                                                  \
        double key[4];                                                                                              \
        bool below = false;                                                                                         \
        _Pragma("unroll") for (int tj = 0; tj < 4; ++tj) {                                                          \
            key[tj] = jcol[tj] < m2 ? nbv[tj] - 2.0 * acc[TI][tj][R] : INFINITY;                                    \
            below |= key[tj] < thr;                                                                                 \
        }                                                                                                           \
        if (__ballot(below)) {                                                                                      \
            top3k<int> t = {INFINITY, INFINITY, INFINITY, 0, 0}; /* columns inside the tile */                      \
            _Pragma("unroll") for (int tj = 0; tj < 4; ++tj) top3k_insert(t, key[tj], (int)(jcol[tj] - j0));        \
            SF_TOP3_STEP(0xB1)  /* quad_perm [1,0,3,2] */                                                           \
            SF_TOP3_STEP(0x4E)  /* quad_perm [2,3,0,1] */                                                           \
            SF_TOP3_STEP(0x141) /* row_half_mirror */                                                               \
            SF_TOP3_STEP(0x140) /* row_mirror */                                                                    \
            if (l15 == 4 * (TI) + (R)) top3k_merge(run, t.k1, j0 + t.j1, t.k2, j0 + t.j2, t.k3);                    \
        }                                                                                                           \
    }
#define SF_EPI_TI(TI) SF_EPI_ROW(TI, 0) SF_EPI_ROW(TI, 1) SF_EPI_ROW(TI, 2) SF_EPI_ROW(TI, 3)
        SF_EPI_TI(0) SF_EPI_TI(1) SF_EPI_TI(2) SF_EPI_TI(3)
#undef SF_EPI_TI
#undef SF_EPI_ROW
#undef SF_TOP3_STEP
    }
    // the two column halves (waves wc = 0, 1 of the same row half) through LDS
    __syncthreads();
    double *sk = &As[0][0][0];                                 // 3 x 128 keys
    int64_t *sj = reinterpret_cast<int64_t *>(&Bs[0][0][0]); // 2 x 128 columns
    const int own = sf_gemm_own_row(tid_end);
    if (wc == 1) {
        sk[own] = run.k1; sk[GM + own] = run.k2; sk[2 * GM + own] = run.k3;
        sj[own] = run.j1; sj[GM + own] = run.j2;
    }
    __syncthreads();
    if (wc == 0) {
        top3k_merge(run, sk[own], sj[own], sk[GM + own], sj[GM + own], sk[2 * GM + own]);
        const int64_t i = i0 + own;
        if (i < m1) {
            pk[(int64_t)(3 * split) * m1 + i] = run.k1;
            pk[(int64_t)(3 * split + 1) * m1 + i] = run.k2;
            pk[(int64_t)(3 * split + 2) * m1 + i] = run.k3;
            pj[(int64_t)(2 * split) * m1 + i] = run.j1;
            pj[(int64_t)(2 * split + 1) * m1 + i] = run.j2;
        }
    }
}

// Merge the splits, apply the gap test between ranks 2 and 3, and for decided rows order the two columns by their reference
// distances (one lane per row, scipy's loop).  Undecided rows are flagged for k_top2_tile.
__global__ void k_top2_decide(const double *__restrict__ a, int64_t m1, const double *__restrict__ b, int64_t d,
                              const double *__restrict__ pk, const int64_t *__restrict__ pj, int nsplit, double nb_max,
                              int64_t *__restrict__ idx, double *__restrict__ dist, int *__restrict__ flag,
                              int *__restrict__ n_flagged)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m1) return;
    top3k<int64_t> t = {pk[i], pk[m1 + i], pk[2 * m1 + i], pj[i], pj[m1 + i]};
    for (int s = 1; s < nsplit; ++s)
        top3k_merge(t, pk[(int64_t)(3 * s) * m1 + i], pj[(int64_t)(2 * s) * m1 + i], pk[(int64_t)(3 * s + 1) * m1 + i],
                    pj[(int64_t)(2 * s + 1) * m1 + i], pk[(int64_t)(3 * s + 2) * m1 + i]);
    double na = 0.0, acc1 = 0.0, acc2 = 0.0;
    const double *ai = a + i * d, *b1 = b + t.j1 * d, *b2 = b + t.j2 * d;
    for (int64_t u = 0; u < d; ++u) {
        const double av = ai[u], df1 = av - b1[u], df2 = av - b2[u];
        na += av * av;
        acc1 += df1 * df1; // left to right, no FMA: scipy's euclidean loop
        acc2 += df2 * df2;
    }
    const bool decided = (t.k3 - t.k2) > sf_match_tol(d, na, nb_max); // false for NaN as well
    flag[i] = decided ? 0 : 1;
    if (!decided) {
        atomicAdd(n_flagged, 1);
        return;
    }
    double d1 = sqrt(acc1), d2 = sqrt(acc2);
    int64_t j1 = t.j1, j2 = t.j2;
    if (top2_lt(d2, j2, d1, j1)) {
        const double dd = d1; d1 = d2; d2 = dd;
        const int64_t jj = j1; j1 = j2; j2 = jj;
    }
    idx[2 * i] = j1;
    idx[2 * i + 1] = j2;
    if (dist) {
        dist[2 * i] = d1;
        dist[2 * i + 1] = d2;
    }
}

} // namespace

// The exact path on device pointers.
static int top2_exact(sf_ctx *ctx, const double *da, int64_t m1, const double *db, int64_t m2, int64_t d, int64_t *didx,
                      double *ddist, const char *name)
{
    const int64_t row_tiles = sf_div_up(m1, TM), col_tiles = sf_div_up(m2, TN);
    int64_t tiles_per_split = 0;
    const int64_t nsplit = sf_match_col_splits(row_tiles, col_tiles, 2048, &tiles_per_split);
    sf_pool_guard tmp(ctx);
    double *pd = nullptr;
    int64_t *pj = nullptr;
    SF_CHECK(tmp.alloc(&pd, (size_t)(2 * nsplit * m1)));
    SF_CHECK(tmp.alloc(&pj, (size_t)(2 * nsplit * m1)));
    SF_LAUNCH(ctx, name, k_top2_tile, dim3((unsigned)row_tiles, (unsigned)nsplit), dim3(256), da, m1, db, m2, d, tiles_per_split,
              pd, pj);
    SF_LAUNCH(ctx, "k8_top2_merge", k_top2_merge, dim3((unsigned)sf_div_up(m1, 256)), dim3(256), (const double *)pd,
              (const int64_t *)pj, m1, (int)nsplit, didx, ddist);
    return SF_OK;
}

// The FP64 matrix-core path on device pointers; *n_exact = rows it handed to the exact kernel.
static int top2_gemm(sf_ctx *ctx, const double *da, int64_t m1, const double *db, int64_t m2, int64_t d, int64_t *didx,
                     double *ddist, int64_t *n_exact)
{
    sf_pool_guard tmp(ctx);
    double *nb = nullptr, *part = nullptr;
    SF_CHECK(tmp.alloc(&nb, (size_t)m2));
    SF_CHECK(tmp.alloc(&part, (size_t)256));
    SF_CHECK(sf_match_sqnorm(ctx, "k8_top2_sqnorm", db, m2, d, nullptr, nb));
    double nb_max = 0.0;
    SF_CHECK(sf_match_max(ctx, "k8_top2_max", nb, m2, part, &nb_max));
    const int64_t row_tiles = sf_div_up(m1, GM), col_tiles = sf_div_up(m2, GN);
    int64_t tiles_per_split = 0;
    const int64_t nsplit = sf_match_col_splits(row_tiles, col_tiles, 1024, &tiles_per_split);
    double *pk = nullptr;
    int64_t *pj = nullptr;
    int *flag = nullptr, *nflag = nullptr;
    SF_CHECK(tmp.alloc(&pk, (size_t)(3 * nsplit * m1)));
    SF_CHECK(tmp.alloc(&pj, (size_t)(2 * nsplit * m1)));
    SF_CHECK(tmp.alloc(&flag, (size_t)m1));
    SF_CHECK(tmp.alloc(&nflag, (size_t)1));
    SF_HIP(hipMemsetAsync(nflag, 0, sizeof(int), ctx->stream));
    const bool vec = (d % 2 == 0) && ((uintptr_t)da % 16 == 0) && ((uintptr_t)db % 16 == 0);
    if (vec) {
        SF_LAUNCH(ctx, "k8_top2_gemm", k_top2_gemm<true>, dim3((unsigned)row_tiles, (unsigned)nsplit), dim3(256), da, m1, db, m2,
                  d, (const double *)nb, tiles_per_split, pk, pj);
    } else {
        SF_LAUNCH(ctx, "k8_top2_gemm", k_top2_gemm<false>, dim3((unsigned)row_tiles, (unsigned)nsplit), dim3(256), da, m1, db, m2,
                  d, (const double *)nb, tiles_per_split, pk, pj);
    }
    SF_LAUNCH(ctx, "k8_top2_decide", k_top2_decide, dim3((unsigned)sf_div_up(m1, 256)), dim3(256), da, m1, db, d,
              (const double *)pk, (const int64_t *)pj, (int)nsplit, nb_max, didx, ddist, flag, nflag);
    int nf = 0;
    SF_HIP(hipMemcpyAsync(&nf, nflag, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    SF_HIP(hipStreamSynchronize(ctx->stream));
    // the undecided rows through the exact kernel, two results per row
    return sf_match_rescue(ctx, da, m1, d, flag, nf, [&](const double *sub, int64_t nr, int64_t *sidx, double *sdist) {
        return top2_exact(ctx, sub, nr, db, m2, d, sidx, sdist, "k8_top2_tile_slowpath");
    }, didx, ddist, n_exact, 2, "k8_top2_gather", "k8_top2_scatter");
}

// The arg-min's size rule (match.hip: match_dispatch) and SF_MATCH_EXACT.  Entries so large that a squared norm could overflow
// (the matrix-core key would be inf - inf) take the exact kernel, whose distances saturate at +inf and still rank by column.
static int top2_dispatch(sf_ctx *ctx, const double *da, int64_t m1, const double *db, int64_t m2, int64_t d, double entry_max,
                         int64_t *didx, double *ddist, int64_t *n_exact)
{
    static const bool force_exact = getenv("SF_MATCH_EXACT") && getenv("SF_MATCH_EXACT")[0] == '1';
    const bool huge = !(8.0 * (double)d * entry_max * entry_max < 1e300);
    if (force_exact || sf_match_small(m1, m2, d) || huge) {
        *n_exact = m1;
        return top2_exact(ctx, da, m1, db, m2, d, didx, ddist, "k8_top2_tile");
    }
    return top2_gemm(ctx, da, m1, db, m2, d, didx, ddist, n_exact);
}

extern "C" int sf_match_top2(sf_ctx *ctx, const double *a, int64_t m1, const double *b, int64_t m2, int64_t d, int64_t *idx,
                             double *dist, int64_t *n_exact, int flags)
{
    if (n_exact) *n_exact = 0;
    if (!ctx || !a || !b || !idx || m1 < 0 || m2 < 0 || d <= 0) { sf_set_error("sf_match_top2: bad argument"); return SF_ERR_ARG; }
    if (m2 == 0 && m1 > 0) { sf_set_error("sf_match_top2: empty reference set"); return SF_ERR_ARG; }
    if (flags != SF_HOST && flags != (SF_IN_DEVICE | SF_OUT_DEVICE)) {
        sf_set_error("sf_match_top2: flags must be SF_HOST or SF_IN_DEVICE|SF_OUT_DEVICE");
        return SF_ERR_UNSUPPORTED;
    }
    if (!m1) return SF_OK;
    SF_HIP(hipSetDevice(ctx->device));
    const bool dev = flags != SF_HOST;
    sf_pool_guard tmp(ctx);
    double *da = const_cast<double *>(a), *db = const_cast<double *>(b), *ddist = dist;
    int64_t *didx = idx;
    if (!dev) {
        SF_CHECK(tmp.alloc(&da, (size_t)(m1 * d)));
        SF_CHECK(tmp.alloc(&db, (size_t)(m2 * d)));
        SF_HIP(hipMemcpyAsync(da, a, (size_t)(m1 * d) * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        SF_HIP(hipMemcpyAsync(db, b, (size_t)(m2 * d) * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        SF_CHECK(tmp.alloc(&didx, (size_t)(2 * m1)));
        if (dist) SF_CHECK(tmp.alloc(&ddist, (size_t)(2 * m1)));
    }
    double amax = 0.0, bmax = 0.0;
    SF_CHECK(sf_rows_abs_max(ctx, da, m1, d, &amax));
    SF_CHECK(sf_rows_abs_max(ctx, db, m2, d, &bmax));
    if (!(amax <= DBL_MAX && bmax <= DBL_MAX)) { sf_set_error("sf_match_top2: a descriptor entry is not finite"); return SF_ERR_ARG; }
    int64_t ne = 0;
    SF_CHECK(top2_dispatch(ctx, da, m1, db, m2, d, std::max(amax, bmax), didx, ddist, &ne));
    if (!dev) {
        SF_HIP(hipMemcpyAsync(idx, didx, (size_t)(2 * m1) * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
        if (dist) SF_HIP(hipMemcpyAsync(dist, ddist, (size_t)(2 * m1) * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        SF_HIP(hipStreamSynchronize(ctx->stream)); // host buffers are the caller's again
    }
    if (n_exact) *n_exact = ne;
    return SF_OK;
}
