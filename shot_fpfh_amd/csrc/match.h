// match.h -- internal to K8 (match.hip, match_gemm.hip, match_half.hip, match_i8.hip, match_top2.hip): the entry points these
// files call across each other, the flagged-row rescue, the split and size rules they share, and their common device helpers.
// Not part of include/shotfpfh.h.  (The main loops of the float64 kernels: match_mainloop.h.)
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <functional>

#include "common.h"

// ---- entry points (device pointers) -------------------------------------------------------------------------------------------
// match.hip: the exact tile kernel; a scan row whose a_ok is 0 is at +inf from everything, a reference row whose b_ok is 0 too
int sf_match_exact(sf_ctx *ctx, const double *da, int64_t m1, const double *db, int64_t m2, int64_t d, int64_t *didx,
                   double *ddist, const char *name, const unsigned char *a_ok, const unsigned char *b_ok);
// match_gemm.hip: the matrix-core paths behind one size-based choice; *n_slow = rows that went to the next slower path
int sf_match_gemm(sf_ctx *ctx, const double *da, int64_t m1, const double *db, int64_t m2, int64_t d, int64_t *didx,
                  double *ddist, const char *name, int64_t *n_slow, const unsigned char *a_ok, const unsigned char *b_ok);
// out[i] = ||rows[i]||^2, or +inf where ok (nullable) is 0: such a row stays out of every arg-min without touching the GEMM
int sf_match_sqnorm(sf_ctx *ctx, const char *name, const double *rows, int64_t m, int64_t d, const unsigned char *ok, double *out);
int sf_match_gemm_f64(sf_ctx *ctx, const double *da, int64_t m1, const double *db, int64_t m2, int64_t d, int64_t *didx,
                      double *ddist, const char *name, int64_t *n_slow, const unsigned char *a_ok, const unsigned char *b_ok);
// match_half.hip, match_i8.hip: the pre-filters; *used = 0 (nothing the caller relies on written) when the input does not suit
// them.  The modes: -1 = by size, 0 = off, 1 = forced (SF_MATCH_HALF, SF_MATCH_I8).
int sf_match_half_mode();
int sf_match_half(sf_ctx *ctx, const double *da, int64_t m1, const double *db, int64_t m2, int64_t d, int64_t *didx,
                  double *ddist, const char *name, int64_t *n_slow, const unsigned char *a_ok, const unsigned char *b_ok,
                  int *used);
int sf_match_i8_mode();
int sf_match_i8(sf_ctx *ctx, const double *da, int64_t m1, const double *db, int64_t m2, int64_t d, int64_t *didx,
                double *ddist, const char *name, int64_t *n_slow, const unsigned char *a_ok, const unsigned char *b_ok,
                int *used);

// ---- host helpers (match.hip) ----------------------------------------------------------------------------------------------------
// The rows a path could not decide (flag[i] != 0, nf of them among the m1 rows of da) through the next slower path:
// next(sub, nr, sidx, sdist) matches the nr gathered rows `sub` and writes their results to sidx / sdist, which are then
// scattered back into didx / ddist.  *n_slow = nr.  per_row results per row (1: arg-min, 2: top-2) in all four arrays; the last
// two arguments are the names of the gather and the scatter in the engine's profile.
typedef std::function<int(const double *sub, int64_t nr, int64_t *sidx, double *sdist)> sf_match_next;
int sf_match_rescue(sf_ctx *ctx, const double *da, int64_t m1, int64_t d, const int *flag, int nf, const sf_match_next &next,
                    int64_t *didx, double *ddist, int64_t *n_slow, int per_row = 1, const char *gather_name = "k8_gather_rows",
                    const char *scatter_name = "k8_scatter_results");
// max over i < n of v[i] >= 0 (+inf when an entry is non-finite or negative, so that the caller can refuse it) -> *out (host);
// part: 256 doubles of device scratch
int sf_match_max(sf_ctx *ctx, const char *name, const double *v, int64_t n, double *part, double *out);

// The size rule of the float64 paths: below it the fixed costs of the matrix-core path dominate and the exact tile kernel runs
// K9's inlier rule sqrt(s) <= thr without the square root: certain for s <= lo = thr^2 rounded down, impossible for s >= hi =
// (next double)^2 rounded up (sqrt is monotone and correctly rounded); a negative or NaN threshold admits nothing.  Shared by
// K9 (match.hip) and the refit sums of K11 (ransac.hip), which must take the very same pairs.
static inline void sf_ransac_band(double thr, double *lo, double *hi)
{
    *lo = *hi = -1.0;
    if (thr >= 0.0) {
        const double up = std::nextafter(thr, INFINITY);
        *lo = std::nextafter(thr * thr, -INFINITY);
        *hi = std::isinf(up) ? INFINITY : std::nextafter(up * up, INFINITY);
        if (std::isinf(thr)) *lo = *hi = INFINITY; // everything finite is an inlier; s = inf: sqrt path
    }
}

static inline bool sf_match_small(int64_t m1, int64_t m2, int64_t d)
{
    return (double)m1 * (double)m2 * (double)d < 5e8 || m2 < 256;
}

// Column splits of a float64 kernel's grid (row_tiles x splits workgroups, the second grid dimension): with fewer than `target`
// row tiles the columns are split until about `target` workgroups exist.  Returns the count, every split non-empty.
static inline int64_t sf_match_col_splits(int64_t row_tiles, int64_t col_tiles, int64_t target, int64_t *tiles_per_split)
{
    int64_t nsplit = 1;
    if (row_tiles < target) nsplit = std::min<int64_t>(col_tiles, sf_div_up(target, row_tiles));
    if (nsplit > 65535) nsplit = 65535;
    *tiles_per_split = sf_div_up(col_tiles, nsplit);
    return sf_div_up(col_tiles, *tiles_per_split);
}

// Column splits of a pre-filter pass (tile_bytes: one 64-column tile of the reference image): (1) each split is short enough for
// an XCD's workgroups to share its tiles through their L2 (8 MB: hit rate 0.83 against 0.90 / 0.89 at 2 / 4 MB with fewer lists
// to walk, profiles/r03_match_summary.md) -- see the note above k_match_half; (2) with few row blocks, enough workgroups for two
// per CU's worth of the chip, each with at least 32 tiles to scan.  The variable `env` overrides the count.
static inline int64_t sf_match_splits(int64_t col_tiles, int64_t tile_bytes, int64_t row_blocks, const char *env)
{
    const int64_t chunk_kb = 8192;
    const int64_t tiles_in_l2 = std::max<int64_t>(8, chunk_kb * 1024 / tile_bytes);
    int64_t nsplit = sf_div_up(col_tiles, tiles_in_l2);
    if (row_blocks * nsplit < 512) nsplit = std::max<int64_t>(nsplit, std::min<int64_t>(sf_div_up(512, row_blocks), std::max<int64_t>(col_tiles / 32, 1)));
    if (const char *e = getenv(env)) nsplit = std::max<int64_t>(1, std::min<int64_t>(atoll(e), col_tiles));
    return nsplit;
}

// ---- device helpers ----------------------------------------------------------------------------------------------------------------
// v of the lane the DPP control CTRL names (bound_ctrl off, all rows and banks)
template <int CTRL>
__device__ __forceinline__ int sf_dpp(int v)
{
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, false);
}
template <int CTRL>
__device__ __forceinline__ float sf_dpp(float v)
{
    return __int_as_float(sf_dpp<CTRL>(__float_as_int(v)));
}
template <int CTRL>
__device__ __forceinline__ double sf_dpp(double v)
{
    return __hiloint2double(sf_dpp<CTRL>(__double2hiint(v)), sf_dpp<CTRL>(__double2loint(v)));
}

// The gap between a row's keys above which their order is the reference's whatever the rounding (match_gemm.hip, "Exactness"):
// 8 d eps (||a_i||^2 + max_j ||b_j||^2)
__device__ __forceinline__ double sf_match_tol(int64_t d, double na, double nb_max)
{
    return 8.0 * (double)d * 1.1102230246251565e-16 * (na + nb_max);
}

// The float64 re-check of a pre-filter's candidates (k_half_final, k_i8_final): a scan row's best column so far, its reference
// distance, and whether every candidate's pre-filter key agreed with the float64 one.
struct sf_recheck {
    double best = INFINITY;
    int64_t bj = -1;
    bool ok = true;
};

// Candidate column j of scan row ai (||ai||^2 = na), whose pre-filter key is `key` in units of 1 / unit: the reference's
// distance (scipy's loop order), the error model's check, and the reference's tie rule (smaller column).
__device__ __forceinline__ void sf_recheck_candidate(sf_recheck &r, const double *ai, const double *b, int64_t d, int64_t j,
                                                     double key, double na, double unit, double half_w)
{
    const double *bjp = b + j * d;
    double acc = 0.0;
    for (int64_t u = 0; u < d; ++u) {
        const double df = ai[u] - bjp[u];
        acc += df * df; // left to right, no FMA: scipy's euclidean loop
    }
    // safety net for the error model: the pre-filter's key of this pair must be within half the row's window of the float64
    // one, ||a - b||^2 - ||a||^2; a row where it is not is handed on
    r.ok &= fabs((acc - na) * unit - key) <= half_w;
    const double dj = sqrt(acc);
    if (dj < r.best || (dj == r.best && j < r.bj) || r.bj < 0) {
        if (!(dj == dj)) return; // NaN: leave the row to the float64 path
        r.best = dj;
        r.bj = j;
    }
}

// Fold of the LPR lanes that share a scan row (minimum with the smaller column on ties: the order of the fold does not matter)
template <int LPR>
__device__ __forceinline__ void sf_recheck_fold(sf_recheck &r)
{
#pragma unroll
    for (int off = LPR / 2; off > 0; off >>= 1) {
        const double ob = __shfl_xor(r.best, off);
        const int64_t oj = __shfl_xor(r.bj, off);
        const int om = __shfl_xor((int)r.ok, off);
        if (oj >= 0 && (r.bj < 0 || ob < r.best || (ob == r.best && oj < r.bj))) {
            r.best = ob;
            r.bj = oj;
        }
        r.ok = r.ok && om;
    }
}
