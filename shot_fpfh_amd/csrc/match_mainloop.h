// match_mainloop.h -- internal to K8's float64 kernels (match.hip, match_gemm.hip, match_top2.hip): the main loops that the
// arg-min and the top-2 kernels run in front of their own epilogues, their tile constants and the LDS swizzle.  The exact tile
// loop has this one copy; of the FP64 matrix-core loop k_match_gemm keeps its own (see there), k_top2_gemm calls this one.
#pragma once
#include <cmath>
#include <cstdint>

#include <hip/hip_runtime.h>

// [jt0, jt1): the column tiles (of `tile` columns) of column split blockIdx.y
__device__ __forceinline__ void sf_split_tiles(int64_t m2, int tile, int64_t tiles_per_split, int64_t &jt0, int64_t &jt1)
{
    const int64_t ntiles = (m2 + tile - 1) / tile;
    jt0 = (int64_t)blockIdx.y * tiles_per_split;
    jt1 = jt0 + tiles_per_split < ntiles ? jt0 + tiles_per_split : ntiles;
}

// ---- exact tile kernels: 64 x 64 tile per 256-thread workgroup, 4 x 4 per thread -------------------------------------------------
constexpr int TM = 64, TN = 64, TK = 16;

// acc[u][v] = sum over t < d of (a[i0 + 4 ty + u][t] - b[j0 + 4 tx + v][t])^2, left to right without FMA: the order is the
// contract (scipy's euclidean loop).  The descriptor dimension goes through LDS in slices of TK, rows past m1 / m2 as zeros.
__device__ __forceinline__ void sf_tile_sqdist(double (&As)[TK][TM + 1], double (&Bs)[TK][TN + 1], const double *__restrict__ a,
                                               int64_t m1, int64_t i0, const double *__restrict__ b, int64_t m2, int64_t j0,
                                               int64_t d, double (&acc)[4][4])
{
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[u][v] = 0.0;
    for (int64_t t0 = 0; t0 < d; t0 += TK) {
        // stage TM x TK of a and TN x TK of b (zero padded); 1024 elements each, 4 per thread
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int lin = tid + 256 * e; // 0..1023
            const int r = lin >> 4, cc = lin & 15;
            const int64_t t = t0 + cc;
            As[cc][r] = (i0 + r < m1 && t < d) ? a[(i0 + r) * d + t] : 0.0;
            Bs[cc][r] = (j0 + r < m2 && t < d) ? b[(j0 + r) * d + t] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < TK; ++t) {
            double av[4], bv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { av[u] = As[t][ty * 4 + u]; bv[u] = Bs[t][tx * 4 + u]; }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const double df = av[u] - bv[v];
                    acc[u][v] += df * df;
                }
        }
        __syncthreads();
    }
}

// ---- FP64 matrix-core kernels: 128 x 128 tile per 256-thread workgroup, 64 x 64 (16 accumulators) per wave --------------------
typedef double d4 __attribute__((ext_vector_type(4)));
constexpr int GM = 128, GN = 128, GK = 16;
// LDS tiles are row-major [row][k], 16 doubles per row, columns swizzled by sw() (see there).
constexpr int LDS_P = 16; // no padding: bank conflicts are avoided by the XOR swizzle sw() below

// LDS column swizzle: a tile row holds GK = 16 doubles = four 32-byte groups; row r stores group g at slot
// g ^ (r & 3).  An MFMA fragment read (16 consecutive rows x the 4 k of one group, 8 bytes per lane) then touches
// every bank exactly once per 16 lanes -- the minimum of four passes per wave read -- where the padded layout
// (pitch 18) had rows r and r + 8 and neighbouring k colliding; and without padding the tile pair is 64 KB, so
// two workgroups fit a CU's LDS.
__device__ __forceinline__ int sw(int row, int c) { return (((c >> 2) ^ (row & 3)) << 2) | (c & 3); }

// acc = a[i0 .. i0 + 128) . b[j0 .. j0 + 128)^T over all of d on v_mfma_f64_16x16x4_f64: wave (wr, wc) = (wave >> 1, wave & 1)
// holds rows 64 wr + 16 ti + l4 + 4 r, columns 64 wc + 16 tj + l15 in acc[ti][tj][r] (l15 = lane & 15, l4 = lane >> 4).  LDS
// double-buffered in slices of GK; ends behind a __syncthreads(), so the caller may reuse As / Bs.
// VEC: the descriptor length is even and both matrices are 16-byte aligned -> a stage is fetched with 16-byte
// loads, eight lanes per 128-byte row segment (8 cache lines per wave instruction instead of 64).
template <bool VEC>
__device__ __forceinline__ void sf_gemm_tile(double (&As)[2][GM][LDS_P], double (&Bs)[2][GN][LDS_P], const double *__restrict__ a,
                                             int64_t m1, int64_t i0, const double *__restrict__ b, int64_t m2, int64_t j0, int64_t d,
                                             d4 (&acc)[4][4])
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int srow = tid & 127, skh = tid >> 7; // staging: this thread's tile row and its half of the 16 k
    const int nk = (int)((d + GK - 1) / GK);
    const int l15 = lane & 15, l4 = lane >> 4;
#pragma unroll
    for (int ti = 0; ti < 4; ++ti)
#pragma unroll
        for (int tj = 0; tj < 4; ++tj) acc[ti][tj] = d4{0.0, 0.0, 0.0, 0.0};
    double ra[8], rb[8];
    auto fetch = [&](int kt) {
        if (VEC) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int p = tid + 256 * u, row = p >> 3, kp = p & 7;
                const int64_t k = (int64_t)kt * GK + 2 * kp, ar = i0 + row, br = j0 + row;
                double2 va = make_double2(0.0, 0.0), vb = make_double2(0.0, 0.0);
                if (ar < m1 && k < d) va = *reinterpret_cast<const double2 *>(a + ar * d + k);
                if (br < m2 && k < d) vb = *reinterpret_cast<const double2 *>(b + br * d + k);
                ra[2 * u] = va.x; ra[2 * u + 1] = va.y;
                rb[2 * u] = vb.x; rb[2 * u + 1] = vb.y;
            }
        } else {
            const int64_t kbase = (int64_t)kt * GK + skh * 8;
            const int64_t ar = i0 + srow, br = j0 + srow;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int64_t k = kbase + u;
                ra[u] = (ar < m1 && k < d) ? a[ar * d + k] : 0.0;
                rb[u] = (br < m2 && k < d) ? b[br * d + k] : 0.0;
            }
        }
    };
    auto stash = [&](int buf) {
        if (VEC) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int p = tid + 256 * u, row = p >> 3, kp = p & 7;
                *reinterpret_cast<double2 *>(&As[buf][row][sw(row, 2 * kp)]) = make_double2(ra[2 * u], ra[2 * u + 1]);
                *reinterpret_cast<double2 *>(&Bs[buf][row][sw(row, 2 * kp)]) = make_double2(rb[2 * u], rb[2 * u + 1]);
            }
        } else {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                As[buf][srow][sw(srow, skh * 8 + u)] = ra[u];
                Bs[buf][srow][sw(srow, skh * 8 + u)] = rb[u];
            }
        }
    };
    fetch(0);
    stash(0);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nk) fetch(kt + 1);
#pragma unroll
        for (int kk = 0; kk < GK / 4; ++kk) {
            double af[4], bf[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                af[t] = As[buf][64 * wr + 16 * t + l15][sw(l15, kk * 4 + l4)]; // (row & 3) == (l15 & 3)
                bf[t] = Bs[buf][64 * wc + 16 * t + l15][sw(l15, kk * 4 + l4)];
            }
#pragma unroll
            for (int ti = 0; ti < 4; ++ti)
#pragma unroll
                for (int tj = 0; tj < 4; ++tj)
                    acc[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[ti], bf[tj], acc[ti][tj], 0, 0, 0);
        }
        if (kt + 1 < nk) stash(buf ^ 1);
        __syncthreads();
    }
}

// the lane's four columns of the tile at j0 (acc[.][tj]) and their ||b_j||^2, +inf past the last column
__device__ __forceinline__ void sf_gemm_cols(int64_t j0, int64_t m2, const double *__restrict__ nb, int64_t (&jcol)[4],
                                             double (&nbv)[4])
{
    const int lane = threadIdx.x & 63, wc = (threadIdx.x >> 6) & 1;
#pragma unroll
    for (int tj = 0; tj < 4; ++tj) {
        jcol[tj] = j0 + 64 * wc + 16 * tj + (lane & 15);
        nbv[tj] = jcol[tj] < m2 ? nb[jcol[tj]] : INFINITY;
    }
}

// The tile row whose running result this lane OWNS within its 16-lane DPP row: row (ti, r) of the wave's block belongs to lane
// 4 ti + r of the DPP row, so ti = l15 >> 2, r = l15 & 3 -> 64 wr + 16 ti + l4 + 4 r
__device__ __forceinline__ int sf_gemm_own_row(int tid)
{
    const int lane = tid & 63, wr = tid >> 7, l15 = lane & 15, l4 = lane >> 4;
    return 64 * wr + 16 * (l15 >> 2) + l4 + 4 * (l15 & 3);
}
