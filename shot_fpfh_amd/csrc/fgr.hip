// fgr.hip -- K12: fast global registration (Zhou, Park, Koltun, ECCV 2016) over given matches.
//
// No counterpart in the reference.  A scaled Geman-McClure cost over ALL matched pairs (or a selection of them), minimised by
// graduated non-convexity: a fixed number of weighted Gauss-Newton steps on SE(3), the definition of tests/fgr_numpy.py.  With the
// normalised rows x = (a - ca) / s, y = (b - cb) / s and the state (R, t, mu):
//   p = R x + t, r = p - y, l = mu / (mu + r.r), w = l^2, J = [-[p]x | I]
//   A = sum w J^T J = sum w [[(p.p) I - p p^T, [p]x], [-[p]x, I]],  g = sum w J^T r = sum w [p x r; r],
//   E = sum (w r.r + mu (l - 1)^2),  W = sum w;   A xi = -g,  R <- exp([xi_0..2]x) R,  t <- exp([xi_0..2]x) t + xi_3..5.
// The whole optimisation stays on the device: per iteration ONE pass over the rows (k12_fgr_sums: a row of partials per block,
// the grid sized to the chip, not to the rows) and ONE single-block kernel (k12_fgr_step: the partial rows folded in a fixed
// order across the lanes of its waves, the 6 x 6 LDL^T solve, Rodrigues, the state update and a trace row), queued back to back;
// the host waits once, at the end.  A kernel that finds the status no longer 0 returns at once.  No atomics on any sum: a call
// repeats bit for bit.
#include "common.h"
#include "device_util.h"

namespace {

constexpr int K12_BLOCK = 256;
constexpr int K12_MAX_BLOCKS = 1024;  // four blocks of 256 per CU: the partial rows of a pass are at most this many, whatever k
constexpr int K12_NV = 32;            // doubles per partial row: the 29 sums, the row count, two zeros
constexpr int K12_NACC = 18;          // distinct accumulators of a pass (A's translation blocks repeat +-sum w p and sum w)
constexpr int K12_FOLD = 1024;        // threads of the single-block kernels: 32 columns x 32 row groups
constexpr int K12_MAX_ITER = 1 << 20;
constexpr double K12_PIVOT_TOL = 1e-12; // an LDL^T pivot d_j <= tol A_jj is "not positive" (rounding leaves ~2^-52 A_jj for an exact 0)

// the device state block (doubles)
enum { ST_CA = 0, ST_CB = 3, ST_S = 6, ST_R = 7, ST_T = 16, ST_MU = 19, ST_FLOOR = 20, ST_STATUS = 21, ST_ITER = 22, ST_E = 23,
       ST_W = 24, ST_SIZE = 32 };

// partial-row column -> accumulator (-1: a structural zero of A), and the columns that hold the negated sum
__constant__ int k12_src[K12_NV] = {0, 1, 2, -1, 8, 7, 3, 4, 8, -1, 6, 5, 7, 6, -1, 9, -1, -1, 9, -1, 9,
                                    10, 11, 12, 13, 14, 15, 16, 9, 17, -1, -1};
__constant__ int k12_neg[K12_NV] = {0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

__device__ __forceinline__ bool k12_row(const int64_t *__restrict__ sel, int64_t i, int64_t m, int64_t &row)
{
    row = sel ? sel[i] : i;
    return row >= 0 && row < m; // a selected row outside [0, m) is never dereferenced: it is left out and the row count tells
}

// nb partial rows folded in a fixed order by a block of 32 G threads (G a power of two): group g adds rows g, g + G, ... in
// ascending order, the groups are then added as a tree.  The 32 results are in sh[0..32) after the call.
template <bool MAX>
__device__ __forceinline__ void k12_fold_rows(const double *__restrict__ partial, int nb, double *sh)
{
    const int v = threadIdx.x & 31, g = threadIdx.x >> 5, G = blockDim.x >> 5;
    double x = 0.0;
    for (int r = g; r < nb; r += G) {
        const double y = partial[(size_t)r * K12_NV + v];
        x = MAX ? fmax(x, y) : x + y;
    }
    sh[threadIdx.x] = x;
    __syncthreads();
    for (int off = G >> 1; off > 0; off >>= 1) {
        if (g < off) {
            const double y = sh[threadIdx.x + 32 * off];
            sh[threadIdx.x] = MAX ? fmax(sh[threadIdx.x], y) : sh[threadIdx.x] + y;
        }
        __syncthreads();
    }
}

// PASS 0: sum a (3), sum b (3), rows left out (1).  PASS 1: max |a - ca|^2, max |b - cb|^2 (ca, cb from the state).
template <int PASS>
__global__ __launch_bounds__(K12_BLOCK) void k12_fgr_moments(const double *__restrict__ a, const double *__restrict__ b, int64_t m,
                                                             const int64_t *__restrict__ sel, int64_t k,
                                                             const double *__restrict__ state, double *__restrict__ partial)
{
    constexpr int NV = PASS == 0 ? 7 : 2;
    __shared__ double sh[4][8];
    if (PASS == 1 && state[ST_STATUS] != 0.0) return;
    double acc[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[v] = 0.0;
    double c0 = 0, c1 = 0, c2 = 0, d0 = 0, d1 = 0, d2 = 0;
    if (PASS == 1) { c0 = state[ST_CA]; c1 = state[ST_CA + 1]; c2 = state[ST_CA + 2]; d0 = state[ST_CB]; d1 = state[ST_CB + 1]; d2 = state[ST_CB + 2]; }
    for (int64_t i = (int64_t)blockIdx.x * K12_BLOCK + threadIdx.x; i < k; i += (int64_t)gridDim.x * K12_BLOCK) {
        int64_t row;
        if (!k12_row(sel, i, m, row)) { if (PASS == 0) acc[NV - 1] += 1.0; continue; }
        const double ax = a[3 * row], ay = a[3 * row + 1], az = a[3 * row + 2];
        const double bx = b[3 * row], by = b[3 * row + 1], bz = b[3 * row + 2];
        if (PASS == 0) {
            acc[0] += ax; acc[1] += ay; acc[2] += az;
            acc[3] += bx; acc[4] += by; acc[5] += bz;
        } else {
            const double ux = ax - c0, uy = ay - c1, uz = az - c2, vx = bx - d0, vy = by - d1, vz = bz - d2;
            double na = (ux * ux + uy * uy) + uz * uz, nb = (vx * vx + vy * vy) + vz * vz;
            // (a NaN must not get lost in fmax: it becomes +inf, which the set-up kernel refuses)
            if (!(na == na)) na = INFINITY;
            if (!(nb == nb)) nb = INFINITY;
            acc[0] = fmax(acc[0], na);
            acc[1] = fmax(acc[1], nb);
        }
    }
    sf_block_sum4_stage<PASS == 1>(acc, sh);
    if (threadIdx.x < K12_NV) {
        double x = 0.0;
        if (threadIdx.x < NV) {
            const int v = threadIdx.x;
            x = PASS == 0 ? sf_block_sum4_at(sh, v) : fmax(fmax(sh[0][v], sh[1][v]), fmax(sh[2][v], sh[3][v]));
        }
        partial[(size_t)blockIdx.x * K12_NV + threadIdx.x] = x;
    }
}

// One block.  MODE 0: the sums of pass 0 -> centres (status 3 when a selected row lies outside [0, m)).  MODE 1: the maxima of
// pass 1 -> s; R = I, t = 0, mu = 1, mu_floor = (thr / s)^2 (status 2 when s is 0 or not finite).
template <int MODE>
__global__ __launch_bounds__(K12_FOLD) void k12_fgr_setup(const double *__restrict__ partial, int nb, int64_t k, double thr,
                                                          double *__restrict__ state)
{
    __shared__ double sh[K12_FOLD];
    if (MODE == 1 && state[ST_STATUS] != 0.0) return;
    k12_fold_rows<MODE == 1>(partial, nb, sh);
    if (MODE == 0) {
        if (threadIdx.x < 6) state[threadIdx.x] = sh[threadIdx.x] / (double)k;
        if (threadIdx.x >= 6 && threadIdx.x < ST_SIZE) state[threadIdx.x] = 0.0;
        if (threadIdx.x == ST_STATUS && sh[6] != 0.0) state[ST_STATUS] = 3.0;
    } else if (threadIdx.x == 0) {
        const double s = sqrt(fmax(sh[0], sh[1]));
        const bool ok = s > 0.0 && s <= SF_DBL_MAX;
        state[ST_S] = ok ? s : 0.0;
        state[ST_R] = state[ST_R + 4] = state[ST_R + 8] = 1.0;
        state[ST_MU] = 1.0;
        state[ST_FLOOR] = ok ? (thr / s) * (thr / s) : 0.0;
        if (!ok) state[ST_STATUS] = 2.0;
    }
}

// One pass over the rows: a row of K12_NV partials per block.
__global__ __launch_bounds__(K12_BLOCK) void k12_fgr_sums(const double *__restrict__ a, const double *__restrict__ b, int64_t m,
                                                          const int64_t *__restrict__ sel, int64_t k,
                                                          const double *__restrict__ state, double *__restrict__ partial)
{
    __shared__ double sh[4][K12_NACC];
    if (state[ST_STATUS] != 0.0) return;
    const double c0 = state[ST_CA], c1 = state[ST_CA + 1], c2 = state[ST_CA + 2];
    const double d0 = state[ST_CB], d1 = state[ST_CB + 1], d2 = state[ST_CB + 2], s = state[ST_S];
    const double r00 = state[ST_R], r01 = state[ST_R + 1], r02 = state[ST_R + 2], r10 = state[ST_R + 3], r11 = state[ST_R + 4],
                 r12 = state[ST_R + 5], r20 = state[ST_R + 6], r21 = state[ST_R + 7], r22 = state[ST_R + 8];
    const double t0 = state[ST_T], t1 = state[ST_T + 1], t2 = state[ST_T + 2], mu = state[ST_MU];
    double acc[K12_NACC];
#pragma unroll
    for (int v = 0; v < K12_NACC; ++v) acc[v] = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * K12_BLOCK + threadIdx.x; i < k; i += (int64_t)gridDim.x * K12_BLOCK) {
        int64_t row;
        if (!k12_row(sel, i, m, row)) continue;
        const double x0 = (a[3 * row] - c0) / s, x1 = (a[3 * row + 1] - c1) / s, x2 = (a[3 * row + 2] - c2) / s;
        const double y0 = (b[3 * row] - d0) / s, y1 = (b[3 * row + 1] - d1) / s, y2 = (b[3 * row + 2] - d2) / s;
        const double p0 = ((r00 * x0 + r01 * x1) + r02 * x2) + t0;
        const double p1 = ((r10 * x0 + r11 * x1) + r12 * x2) + t1;
        const double p2 = ((r20 * x0 + r21 * x1) + r22 * x2) + t2;
        const double e0 = p0 - y0, e1 = p1 - y1, e2 = p2 - y2;
        const double rr = (e0 * e0 + e1 * e1) + e2 * e2;
        const double l = mu / (mu + rr), w = l * l;
        const double wp0 = w * p0, wp1 = w * p1, wp2 = w * p2, wr0 = w * e0, wr1 = w * e1, wr2 = w * e2, lm = l - 1.0;
        acc[0] += w * (p1 * p1 + p2 * p2); acc[1] += -(wp0 * p1); acc[2] += -(wp0 * p2);
        acc[3] += w * (p0 * p0 + p2 * p2); acc[4] += -(wp1 * p2);
        acc[5] += w * (p0 * p0 + p1 * p1);
        acc[6] += wp0; acc[7] += wp1; acc[8] += wp2;
        acc[9] += w;
        acc[10] += p1 * wr2 - p2 * wr1; acc[11] += p2 * wr0 - p0 * wr2; acc[12] += p0 * wr1 - p1 * wr0;
        acc[13] += wr0; acc[14] += wr1; acc[15] += wr2;
        acc[16] += w * rr + mu * (lm * lm);
        acc[17] += 1.0;
    }
    sf_block_sum4_stage(acc, sh);
    if (threadIdx.x < K12_NV) {
        const int src = k12_src[threadIdx.x];
        double x = 0.0;
        if (src >= 0) {
            x = sf_block_sum4_at(sh, src);
            if (k12_neg[threadIdx.x]) x = -x;
        }
        partial[(size_t)blockIdx.x * K12_NV + threadIdx.x] = x;
    }
}

// One block: the partial rows of a pass folded into out[K12_NV] (sf_fgr_sums).
__global__ __launch_bounds__(K12_FOLD) void k12_fgr_fold(const double *__restrict__ partial, int nb, double *__restrict__ out)
{
    __shared__ double sh[K12_FOLD];
    k12_fold_rows<false>(partial, nb, sh);
    if (threadIdx.x < K12_NV) out[threadIdx.x] = sh[threadIdx.x];
}

// One block: fold, solve, update.
__global__ __launch_bounds__(K12_FOLD) void k12_fgr_step(const double *__restrict__ partial, int nb, int decrease_every,
                                                         double division_factor, double *__restrict__ state,
                                                         double *__restrict__ trace)
{
    __shared__ double sh[K12_FOLD];
    if (state[ST_STATUS] != 0.0) return;
    k12_fold_rows<false>(partial, nb, sh);
    if (threadIdx.x != 0) return;
    // (every index below is a constant after unrolling: the arrays live in registers)
    double A[6][6], L[6][6], d[6], z[6], xi[6];
    {
        int n = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = i; j < 6; ++j) { A[i][j] = A[j][i] = sh[n]; ++n; }
    }
    const double E = sh[27], W = sh[28];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double dj = A[j][j];
#pragma unroll
        for (int q = 0; q < j; ++q) dj = dj - (L[j][q] * L[j][q]) * d[q];
        ok = ok && dj > K12_PIVOT_TOL * A[j][j] && dj <= SF_DBL_MAX;
        d[j] = ok ? dj : 1.0; // (keeps the arithmetic below finite; the result is not used)
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double v = A[i][j];
#pragma unroll
            for (int q = 0; q < j; ++q) v = v - (L[i][q] * L[j][q]) * d[q];
            L[i][j] = v / d[j];
        }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double v = -sh[21 + i];
#pragma unroll
        for (int q = 0; q < i; ++q) v = v - L[i][q] * z[q];
        z[i] = v;
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double v = z[i] / d[i];
#pragma unroll
        for (int q = i + 1; q < 6; ++q) v = v - L[q][i] * xi[q];
        xi[i] = v;
    }
    const double mag = ((fabs(xi[0]) + fabs(xi[1])) + (fabs(xi[2]) + fabs(xi[3]))) + (fabs(xi[4]) + fabs(xi[5]));
    ok = ok && mag <= SF_DBL_MAX;
    state[ST_E] = E;
    state[ST_W] = W;
    if (!ok) { state[ST_STATUS] = 1.0; return; } // degenerate: the transform of the previous iteration stays
    // exp([om]x) = I + (sin th / th) K + 1/2 (sin(th/2) / (th/2))^2 K^2
    const double o0 = xi[0], o1 = xi[1], o2 = xi[2];
    const double th = sqrt((o0 * o0 + o1 * o1) + o2 * o2);
    double D[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (th > 0.0) {
        const double ca = sin(th) / th, h = sin(0.5 * th) / (0.5 * th), cb = 0.5 * (h * h);
        const double K[9] = {0.0, -o2, o1, o2, 0.0, -o0, -o1, o0, 0.0};
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const double kk = (K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j]) + K[3 * i + 2] * K[6 + j];
                D[3 * i + j] = (D[3 * i + j] + ca * K[3 * i + j]) + cb * kk;
            }
    }
    double Rn[9], tn[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j)
            Rn[3 * i + j] = (D[3 * i] * state[ST_R + j] + D[3 * i + 1] * state[ST_R + 3 + j]) + D[3 * i + 2] * state[ST_R + 6 + j];
        tn[i] = ((D[3 * i] * state[ST_T] + D[3 * i + 1] * state[ST_T + 1]) + D[3 * i + 2] * state[ST_T + 2]) + xi[3 + i];
    }
#pragma unroll
    for (int v = 0; v < 9; ++v) state[ST_R + v] = Rn[v];
#pragma unroll
    for (int v = 0; v < 3; ++v) state[ST_T + v] = tn[v];
    const int it = (int)state[ST_ITER];
    const double mu = state[ST_MU];
    trace[4 * it] = mu;
    trace[4 * it + 1] = E;
    trace[4 * it + 2] = W;
    trace[4 * it + 3] = sqrt((((xi[0] * xi[0] + xi[1] * xi[1]) + xi[2] * xi[2]) + (xi[3] * xi[3] + xi[4] * xi[4])) + xi[5] * xi[5]);
    state[ST_ITER] = (double)(it + 1);
    if ((it + 1) % decrease_every == 0) state[ST_MU] = fmax(mu / division_factor, state[ST_FLOOR]);
}

int k12_blocks(int64_t k) { return (int)std::min<int64_t>(K12_MAX_BLOCKS, std::max<int64_t>(1, sf_div_up(k, K12_BLOCK))); }

int k12_check_rows(const char *who, int64_t m, const int64_t *sel, int64_t k)
{
    if (k < 3) { sf_set_error("%s: %lld rows, at least 3 matched pairs are needed", who, (long long)k); return SF_ERR_ARG; }
    if (!sel && k > m) { sf_set_error("%s: %lld rows of %lld matches and no selection", who, (long long)k, (long long)m); return SF_ERR_ARG; }
    return SF_OK;
}

} // namespace

extern "C" int sf_fgr_sums(sf_ctx *ctx, const double *a_dev, const double *b_dev, int64_t m, const int64_t *sel_dev, int64_t k,
                           const double *state, double *sums)
{
    if (!ctx || !a_dev || !b_dev || !state || !sums || m < 0) { sf_set_error("sf_fgr_sums: bad argument"); return SF_ERR_ARG; }
    SF_CHECK(k12_check_rows("sf_fgr_sums", m, sel_dev, k));
    if (!(state[6] > 0.0) || !(state[19] > 0.0)) { sf_set_error("sf_fgr_sums: the scale s and mu must be positive"); return SF_ERR_ARG; }
    SF_HIP(hipSetDevice(ctx->device));
    for (int i = 0; i < 32; ++i) sums[i] = 0.0;
    sf_pool_guard tmp(ctx);
    const int nb = k12_blocks(k);
    double *dstate = nullptr, *partial = nullptr, *dsums = nullptr;
    SF_CHECK(tmp.alloc(&dstate, ST_SIZE));
    SF_CHECK(tmp.alloc(&partial, (size_t)nb * K12_NV));
    SF_CHECK(tmp.alloc(&dsums, K12_NV));
    void *pin = nullptr;
    SF_CHECK(sf_ctx_pinned(ctx, &pin));
    double *hs = (double *)pin, *ho = hs + ST_SIZE;
    for (int i = 0; i < ST_SIZE; ++i) hs[i] = i < 20 ? state[i] : 0.0; // (the 20 host values are the head of the device state)
    SF_HIP(hipMemcpyAsync(dstate, hs, ST_SIZE * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    SF_LAUNCH(ctx, "k12_fgr_sums", k12_fgr_sums, dim3(nb), dim3(K12_BLOCK), a_dev, b_dev, m, sel_dev, k, (const double *)dstate, partial);
    SF_LAUNCH(ctx, "k12_fgr_fold", k12_fgr_fold, dim3(1), dim3(K12_FOLD), (const double *)partial, nb, dsums);
    SF_HIP(hipMemcpyAsync(ho, dsums, K12_NV * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    SF_HIP(hipStreamSynchronize(ctx->stream));
    memcpy(sums, ho, K12_NV * sizeof(double));
    if (sums[29] != (double)k) {
        sf_set_error("sf_fgr_sums: %lld selected rows lie outside [0, %lld)", (long long)(k - (int64_t)sums[29]), (long long)m);
        return SF_ERR_ARG;
    }
    return SF_OK;
}

extern "C" int sf_fgr(sf_ctx *ctx, const double *a_dev, const double *b_dev, int64_t m, const int64_t *sel_dev, int64_t k,
                      double distance_threshold, int iterations, int decrease_every, double division_factor, double *Rt,
                      double *info, double *trace)
{
    if (!ctx || !a_dev || !b_dev || !Rt || !info || m < 0) { sf_set_error("sf_fgr: bad argument"); return SF_ERR_ARG; }
    SF_CHECK(k12_check_rows("sf_fgr", m, sel_dev, k));
    if (iterations < 1 || decrease_every < 1 || !(division_factor > 1.0) ||
        !(fabs(distance_threshold) <= SF_DBL_MAX)) {
        sf_set_error("sf_fgr: iterations %d >= 1, decrease_every %d >= 1, division_factor %g > 1 and a finite threshold are needed",
                     iterations, decrease_every, division_factor);
        return SF_ERR_ARG;
    }
    if (iterations > K12_MAX_ITER) { sf_set_error("sf_fgr: more than %d iterations", K12_MAX_ITER); return SF_ERR_UNSUPPORTED; }
    SF_HIP(hipSetDevice(ctx->device));
    for (int i = 0; i < 12; ++i) Rt[i] = 0.0;
    for (int i = 0; i < 8; ++i) info[i] = 0.0;
    sf_pool_guard tmp(ctx);
    const int nb = k12_blocks(k);
    double *dstate = nullptr, *partial = nullptr;
    SF_CHECK(tmp.alloc(&dstate, (size_t)ST_SIZE + 4 * (size_t)iterations)); // the state, then the trace
    SF_CHECK(tmp.alloc(&partial, (size_t)nb * K12_NV));
    double *dtrace = dstate + ST_SIZE;
    SF_HIP(hipMemsetAsync(dtrace, 0, 4 * (size_t)iterations * sizeof(double), ctx->stream));
    const dim3 grid(nb), block(K12_BLOCK), one(1), fold(K12_FOLD);
    SF_LAUNCH(ctx, "k12_fgr_moments", k12_fgr_moments<0>, grid, block, a_dev, b_dev, m, sel_dev, k, (const double *)dstate, partial);
    SF_LAUNCH(ctx, "k12_fgr_setup", k12_fgr_setup<0>, one, fold, (const double *)partial, nb, k, distance_threshold, dstate);
    SF_LAUNCH(ctx, "k12_fgr_moments", k12_fgr_moments<1>, grid, block, a_dev, b_dev, m, sel_dev, k, (const double *)dstate, partial);
    SF_LAUNCH(ctx, "k12_fgr_setup", k12_fgr_setup<1>, one, fold, (const double *)partial, nb, k, distance_threshold, dstate);
    for (int it = 0; it < iterations; ++it) { // queued back to back: nothing below waits for the device
        SF_LAUNCH(ctx, "k12_fgr_sums", k12_fgr_sums, grid, block, a_dev, b_dev, m, sel_dev, k, (const double *)dstate, partial);
        SF_LAUNCH(ctx, "k12_fgr_step", k12_fgr_step, one, fold, (const double *)partial, nb, decrease_every, division_factor, dstate,
                  dtrace);
    }
    void *pin = nullptr;
    SF_CHECK(sf_ctx_pinned(ctx, &pin));
    double *hs = (double *)pin;
    SF_HIP(hipMemcpyAsync(hs, dstate, ST_SIZE * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (trace) SF_HIP(hipMemcpyAsync(trace, dtrace, 4 * (size_t)iterations * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    SF_HIP(hipStreamSynchronize(ctx->stream)); // the one wait of the call
    const int status = (int)hs[ST_STATUS];
    info[0] = hs[ST_STATUS]; info[1] = hs[ST_ITER]; info[2] = hs[ST_MU]; info[3] = hs[ST_S]; info[4] = hs[ST_E]; info[5] = hs[ST_W];
    if (status == 3) { sf_set_error("sf_fgr: selected rows lie outside [0, %lld)", (long long)m); return SF_ERR_ARG; }
    if (status == 2) return SF_OK; // no extent: no transform (zeros)
    const double *R = hs + ST_R, *t = hs + ST_T, *ca = hs + ST_CA, *cb = hs + ST_CB, s = hs[ST_S];
    for (int v = 0; v < 9; ++v) Rt[v] = R[v];
    for (int i = 0; i < 3; ++i) // t_out = (s t + cb) - R ca
        Rt[9 + i] = (s * t[i] + cb[i]) - ((R[3 * i] * ca[0] + R[3 * i + 1] * ca[1]) + R[3 * i + 2] * ca[2]);
    return SF_OK;
}
