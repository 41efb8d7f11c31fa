// icp.hip -- one ICP iteration on the device: transform, nearest neighbour, inlier filter and the normal-equation sums.
//
// Replaces, per iteration of shot_fpfh/icp.py (:64-72, :108-124, :160-183):
//   transformation[points]                          core/rigid_transform.py:81-88
//   kdtree.query(points_aligned)                    the grid k-NN kernel with k = 1 (search.hip)
//   the inlier filter  distances <= d_max
//   solver_point_to_point's centroids and 3x3 cross-covariance      core/solvers.py:17-18
//   solver_point_to_plane's G^T G (6x6) and G^T h (6)                core/solvers.py:38-46
//   the residuals the reference reports as "rms"                     icp.py:66-69, 176-182
// The reference forms these with NumPy over (n_inliers, 3) arrays on the host, after shipping distances and indices
// back from the tree.  Here the scan subset stays in HBM; per iteration ~30 doubles come back, and the host does what is
// left: a 3x3 SVD or a 6x6 solve, and the composition of the transform.
//
// Sums are accumulated per thread, folded per block (shuffles + LDS) and then over the block partials by ONE block in a
// fixed order, so a run is reproducible bit for bit.  Point-to-point is centred in a second pass (centroids first),
// which keeps the cross-covariance free of cancellation, like the reference's explicit centring.
//
// ONE kernel family, k_icp_sums<PASS, MODE>, and ONE host chain, icp_chain, serve every entry point:
//   MODE 0 point to point, MODE 1 point to plane (sf_icp_accumulate);
//   MODE 2 generalized (plane-to-plane) ICP, K16 (Segal, Haehnel, Thrun, RSS 2009; no counterpart in the reference): every pair is
//     weighted by M = (C_b + R C_a R^T)^-1, C = I - (1 - eps) n n^T from the unit normal of either point, and the 6x6 Gauss-Newton
//     system of sum r^T M r is left for the host (sf_icp_accumulate_gicp);
//   K17, robust losses for all three modes (no counterpart in the reference): every kept pair has a weight psi(r) / r of its
//     residual (Huber, Cauchy, Geman-McClure, Tukey), and the weighted sums are left for the host (sf_icp_accumulate_robust).
//   K18, trimmed ICP for all three modes (no counterpart in the reference): a key pass writes every pair's squared residual, the radix
//     selection of select.hip finds the order statistic that bounds the best-fitting share of them, and both sums passes leave out the
//     pairs beyond that cut (sf_icp_accumulate_trimmed).  The residual is formed by ONE function, icp_pair_residual, for all of them.
//   K19, MODE 3, the symmetric point-to-plane objective (Rusinkiewicz, SIGGRAPH 2019; no counterpart in the reference): the residual
//     of a pair is taken along the mean of its two normals and its lever arm is p + b; the 6x6 system is point-to-plane's, with a loss
//     and a trim like the others (sf_icp_accumulate_symmetric).
// The two plain entry points are the chain with loss none: every weight is 1.0, w * term is the term, and they return the first 40
// of its 48 numbers with [7] (sum w) cleared.
#include "common.h"
#include "device_util.h"
#include "select.h"

namespace {

constexpr int ICP_BLOCKS = 256;
constexpr int ICP_NV = 32; // values per partial row (largest mode: 21 + 6 + 2 = 29)

// p <- p R^T + t, rows (optionally selected by `sel`) written to out (may alias pts when sel == null)
__global__ void k_transform(const double *__restrict__ pts, const int64_t *__restrict__ sel, int64_t m,
                            const double *__restrict__ Rt, double *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const int64_t j = sel ? sel[i] : i;
    const double x = pts[3 * j], y = pts[3 * j + 1], z = pts[3 * j + 2];
    double ox = x, oy = y, oz = z;
    if (Rt) {
        ox = ((x * Rt[0] + y * Rt[1]) + z * Rt[2]) + Rt[9];
        oy = ((x * Rt[3] + y * Rt[4]) + z * Rt[5]) + Rt[10];
        oz = ((x * Rt[6] + y * Rt[7]) + z * Rt[8]) + Rt[11];
    }
    out[3 * i] = ox; out[3 * i + 1] = oy; out[3 * i + 2] = oz;
}

// fold the block partials in block order (PASS 1 of every mode; k_icp_means folds PASS 0)
__global__ __launch_bounds__(64) void k_icp_final(const double *__restrict__ partial, int nblocks, int nv, double *__restrict__ out)
{
    const int v = threadIdx.x;
    double a = 0.0;
    if (v < nv)
        for (int b = 0; b < nblocks; ++b) a += partial[(size_t)b * ICP_NV + v];
    if (v < nv) out[v] = a;
}

// ---- the weight of a kept pair (K17) ------------------------------------------------------------------------------------------
// The weight psi(r) / r of a kept pair from its squared residual r2 and the scale k (kk = k * k), one rounding per operation,
// which tests/icp_robust_numpy.py repeats operation by operation:
//   0 none            1
//   1 Huber           a = sqrt(r2);  a <= k ? 1 : k / a
//   2 Cauchy          s = r2 / kk;   1 / (1 + s)
//   3 Geman-McClure   c = 1 / (1 + s);  c c
//   4 Tukey           s <= 1 ? (1 - s)(1 - s) : 0
// `loss` is uniform over the launch: one kernel per (pass, mode), not one per loss.
__device__ inline double robust_weight(int loss, double r2, double k, double kk)
{
    if (loss == 0) return 1.0;
    if (loss == 1) {
        const double a = sqrt(r2);
        return a <= k ? 1.0 : k / a;
    }
    const double s = r2 / kk;
    if (loss == 4) {
        const double o = 1.0 - s;
        return s <= 1.0 ? o * o : 0.0;
    }
    const double c = 1.0 / (1.0 + s);
    return loss == 2 ? c : c * c;
}

// One pair of the chain: slot i's moved scan point p, its nearest reference point (x, y, z) with normal n, d = q - p, d2, and the
// mode's squared residual r2 with what PASS 1 needs beside it (h; the Mahalanobis term, M and u = M d).  Formed HERE and nowhere else:
// the key pass of the trimmed chain (K18) and both sums passes call this one function, so their r2 agree bit for bit.
struct icp_pair {
    double px, py, pz, x, y, z, nx, ny, nz, dx, dy, dz, d2, h, maha, r2, M[3][3], u[3];
};

// false: the pair is outside d_max (r2 and what follows d2 are then not formed)
template <int MODE>
__device__ inline bool icp_pair_residual(int64_t i, const double *__restrict__ qx, const double *__restrict__ qy,
                                         const double *__restrict__ qz, const int32_t *__restrict__ idx,
                                         const int32_t *__restrict__ qrow, const double *__restrict__ rec,
                                         const double *__restrict__ nrm, const int64_t *__restrict__ sel, bool turned,
                                         const double (&R)[9], double c, double d_max, icp_pair &P)
{
    const double px = qx[i], py = qy[i], pz = qz[i];
    double x, y, z, nx = 0, ny = 0, nz = 0;
    if (MODE == 0) sf_load_xyz(rec, idx[i], x, y, z);
    else sf_load_pn(rec, idx[i], x, y, z, nx, ny, nz);
    const double dx = x - px, dy = y - py, dz = z - pz;
    const double d2 = (dx * dx + dy * dy) + dz * dz;
    if (!(sqrt(d2) <= d_max)) return false; // KDTree.query returns sqrt(d2); `distances <= d_max` (icp.py:64, 112, 164)
    P.px = px; P.py = py; P.pz = pz; P.x = x; P.y = y; P.z = z; P.nx = nx; P.ny = ny; P.nz = nz;
    P.dx = dx; P.dy = dy; P.dz = dz; P.d2 = d2;
    P.r2 = d2; P.h = 0.0; P.maha = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        P.u[a] = 0.0;
#pragma unroll
        for (int b = 0; b < 3; ++b) P.M[a][b] = 0.0;
    }
    if (MODE == 1) {
        P.h = (dx * nx + dy * ny) + dz * nz;
        P.r2 = P.h * P.h;
    }
    if (MODE == 2) {
        const int64_t row = qrow ? (int64_t)qrow[i] : i;
        const int64_t j = sel ? sel[row] : row;
        const double ax = nrm[3 * j], ay = nrm[3 * j + 1], az = nrm[3 * j + 2];
        double m0 = ax, m1 = ay, m2 = az;
        if (turned) {
            m0 = (ax * R[0] + ay * R[1]) + az * R[2];
            m1 = (ax * R[3] + ay * R[4]) + az * R[5];
            m2 = (ax * R[6] + ay * R[7]) + az * R[8];
        }
        const double s00 = 2.0 - c * (nx * nx + m0 * m0), s11 = 2.0 - c * (ny * ny + m1 * m1), s22 = 2.0 - c * (nz * nz + m2 * m2);
        const double s01 = -(c * (nx * ny + m0 * m1)), s02 = -(c * (nx * nz + m0 * m2)), s12 = -(c * (ny * nz + m1 * m2));
        const double a00 = s11 * s22 - s12 * s12, a01 = s02 * s12 - s01 * s22, a02 = s01 * s12 - s02 * s11;
        const double a11 = s00 * s22 - s02 * s02, a12 = s01 * s02 - s00 * s12, a22 = s00 * s11 - s01 * s01;
        const double det = (s00 * a00 + s01 * a01) + s02 * a02;
        const double inv = 1.0 / det;
        P.M[0][0] = a00 * inv; P.M[0][1] = P.M[1][0] = a01 * inv; P.M[0][2] = P.M[2][0] = a02 * inv;
        P.M[1][1] = a11 * inv; P.M[1][2] = P.M[2][1] = a12 * inv; P.M[2][2] = a22 * inv;
#pragma unroll
        for (int b = 0; b < 3; ++b) P.u[b] = (P.M[b][0] * dx + P.M[b][1] * dy) + P.M[b][2] * dz;
        P.maha = (dx * P.u[0] + dy * P.u[1]) + dz * P.u[2];
        P.r2 = P.maha < 0.0 ? 0.0 : P.maha;
    }
    if (MODE == 3) { // K19: the residual along the mean of the two normals; P.nx .. P.nz become that mean
        const int64_t row = qrow ? (int64_t)qrow[i] : i;
        const int64_t j = sel ? sel[row] : row;
        const double ax = nrm[3 * j], ay = nrm[3 * j + 1], az = nrm[3 * j + 2];
        double m0 = ax, m1 = ay, m2 = az;
        if (turned) {
            m0 = (ax * R[0] + ay * R[1]) + az * R[2];
            m1 = (ax * R[3] + ay * R[4]) + az * R[5];
            m2 = (ax * R[6] + ay * R[7]) + az * R[8];
        }
        const double s = (m0 * nx + m1 * ny) + m2 * nz >= 0.0 ? 1.0 : -1.0; // the sign of either normal cancels
        P.nx = 0.5 * (nx + s * m0); P.ny = 0.5 * (ny + s * m1); P.nz = 0.5 * (nz + s * m2);
        P.h = (dx * P.nx + dy * P.ny) + dz * P.nz;
        P.r2 = P.h * P.h;
    }
    return true;
}

// The key pass of the trimmed chain (K18): one key per slot for the selection (select.hip), r2's bit pattern for a pair inside d_max
// and the all-ones pattern, which orders last, for a slot outside it.
template <int MODE>
__global__ __launch_bounds__(256) void k_icp_keys(const double *__restrict__ qx, const double *__restrict__ qy,
                                                  const double *__restrict__ qz, const int32_t *__restrict__ idx,
                                                  const int32_t *__restrict__ qrow, const double *__restrict__ rec,
                                                  const double *__restrict__ nrm, const int64_t *__restrict__ sel,
                                                  const double *__restrict__ Rt, int64_t m, double d_max, double epsilon,
                                                  uint64_t *__restrict__ keys)
{
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if ((MODE == 2 || MODE == 3) && Rt) {
#pragma unroll
        for (int v = 0; v < 9; ++v) R[v] = Rt[v];
    }
    const double c = 1.0 - epsilon;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
        icp_pair P;
        const bool kept = icp_pair_residual<MODE>(i, qx, qy, qz, idx, qrow, rec, nrm, sel, Rt != nullptr, R, c, d_max, P);
        keys[i] = kept ? (uint64_t)__double_as_longlong(P.r2) : ~0ull;
    }
}

// Both passes of the three modes, with a weight w per kept pair; every line one rounding per operation, left to right, which
// tests/icp_numpy.py, tests/gicp_numpy.py and tests/icp_robust_numpy.py repeat operation by operation.
//   PASS 0 (15): inlier count, sum of inlier points p, sum of their neighbours q (7), then w, w p (3), w q (3), w r2
//   PASS 1, MODE 0 (point to point): centred cross-covariance H = sum w (p - pbar)(q - qbar)^T (9) and sum |p - q|^2, centred with
//           `mean`, the WEIGHTED centroids k_icp_means leaves
//   PASS 1, MODE 1 (point to plane): upper triangle of G^T G (21), G^T h (6), sum |h| with g = [p x n, n], h = (q - p) . n
//   PASS 1, MODE 3 (symmetric, K19): MODE 1's sums with the lever arm c = p + b for p and the mean normal n = (nb + s m) / 2 for nb
//           (m as in MODE 2, s = +1 if (m0 nb0 + m1 nb1) + m2 nb2 >= 0 else -1), h = (b - p) . n, and sum |b - p|^2 behind sum |h| (29)
//   PASS 1, MODE 2 (generalized, K16): with p the moved scan point, b its nearest reference point, nb b's normal, na the scan point's
//           normal (row qrow[slot] of the scan, through sel) and c = 1 - eps:
//     m   = (na.x R0 + na.y R1) + na.z R2 per row of R (no t; m = na when Rt is null)
//     S   = 2 I - c (nb nb^T + m m^T):  S_ii = 2 - c (nb_i nb_i + m_i m_i),  S_ij = -(c (nb_i nb_j + m_i m_j))
//     adj = symmetric adjugate of S, each entry ONE difference of two products; det = (S00 adj00 + S01 adj01) + S02 adj02
//     M   = adj * (1 / det)                                                    (six entries)
//     r   = b - p,  u = M r with u_i = (M_i0 r0 + M_i1 r1) + M_i2 r2
//     Q   = [p]x M  (Q_0j = py M_2j - pz M_1j, ...),  T = Q [p]x^T  (T_i0 = py Q_i2 - pz Q_i1, ...)
//     H   = J^T M J = [[T, Q], [Q^T, M]] (upper triangle, 21),  g = J^T M r = [p x u; u] (6),  r.u,  |r|^2  with J = [-[p]x, I]
//           A zero normal makes its dyad vanish (C = I); the sign of a normal cancels in the dyad.
// The pair's squared residual r2 is d2 (MODE 0), h h (MODES 1 and 3) or the Mahalanobis term (r0 u0 + r1 u1) + r2 u2 clamped at 0 (MODE 2),
// formed by icp_pair_residual above, and both passes form w from it by the same operations, so they get the same bits.  PASS 1
// multiplies every fit term by w (one more rounding); the residual sums the host reports as rms stay unweighted: d2 (MODE 0: [9],
// MODE 2: [28]), |h| (MODE 1: [27]), the Mahalanobis term as formed (MODE 2: [27]).
// Given `cut` (K18, the trimmed chain) both passes leave out the pairs with r2 above cut[0], a number the selection left on the device.
// With w = 1 (loss none, or Huber with k above every residual) w * term is the term, bit for bit: the plain entry points.
template <int PASS, int MODE>
__global__ __launch_bounds__(256) void k_icp_sums(const double *__restrict__ qx, const double *__restrict__ qy,
                                                  const double *__restrict__ qz, const int32_t *__restrict__ idx,
                                                  const int32_t *__restrict__ qrow, const double *__restrict__ rec,
                                                  const double *__restrict__ nrm, const int64_t *__restrict__ sel,
                                                  const double *__restrict__ Rt, int64_t m, double d_max, double epsilon, int loss,
                                                  double k, const double *__restrict__ mean /* 6, PASS 1 MODE 0 */,
                                                  const double *__restrict__ cut /* null: no trimming */, double *__restrict__ partial)
{
    constexpr int NV = PASS == 0 ? 15 : (MODE == 0 ? 10 : (MODE == 1 ? 28 : 29));
    __shared__ double sh[4][ICP_NV];
    double acc[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[v] = 0.0;
    const double kk = k * k;
    double pm[3] = {0, 0, 0}, qm[3] = {0, 0, 0};
    if (PASS == 1 && MODE == 0) {
        pm[0] = mean[0]; pm[1] = mean[1]; pm[2] = mean[2];
        qm[0] = mean[3]; qm[1] = mean[4]; qm[2] = mean[5];
    }
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if ((MODE == 2 || MODE == 3) && Rt) {
#pragma unroll
        for (int v = 0; v < 9; ++v) R[v] = Rt[v];
    }
    const double c = 1.0 - epsilon;
    const bool trimmed = cut != nullptr;
    const double r2_max = trimmed ? cut[0] : 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
        icp_pair P;
        if (!icp_pair_residual<MODE>(i, qx, qy, qz, idx, qrow, rec, nrm, sel, Rt != nullptr, R, c, d_max, P)) continue;
        if (trimmed && !(P.r2 <= r2_max)) continue; // K18: the pairs beyond the cut are not used; ties at the cut are
        const double px = P.px, py = P.py, pz = P.pz, x = P.x, y = P.y, z = P.z, nx = P.nx, ny = P.ny, nz = P.nz;
        const double d2 = P.d2, h = P.h, maha = P.maha, r2 = P.r2;
        const double(&M)[3][3] = P.M;
        const double(&u)[3] = P.u;
        const double w = robust_weight(loss, r2, k, kk);
        if constexpr (PASS == 0) {
            acc[0] += 1.0;
            acc[1] += px; acc[2] += py; acc[3] += pz;
            acc[4] += x; acc[5] += y; acc[6] += z;
            acc[7] += w;
            acc[8] += w * px; acc[9] += w * py; acc[10] += w * pz;
            acc[11] += w * x; acc[12] += w * y; acc[13] += w * z;
            acc[14] += w * r2;
        } else if constexpr (MODE == 0) {
            const double ax = px - pm[0], ay = py - pm[1], az = pz - pm[2];
            const double bx = x - qm[0], by = y - qm[1], bz = z - qm[2];
            acc[0] += w * (ax * bx); acc[1] += w * (ax * by); acc[2] += w * (ax * bz);
            acc[3] += w * (ay * bx); acc[4] += w * (ay * by); acc[5] += w * (ay * bz);
            acc[6] += w * (az * bx); acc[7] += w * (az * by); acc[8] += w * (az * bz);
            acc[9] += d2;
        } else if constexpr (MODE == 1 || MODE == 3) {
            // the lever arm: p (MODE 1), c = p + b (MODE 3, where n is the mean normal icp_pair_residual left)
            const double lx = MODE == 3 ? px + x : px, ly = MODE == 3 ? py + y : py, lz = MODE == 3 ? pz + z : pz;
            const double g[6] = {ly * nz - lz * ny, lz * nx - lx * nz, lx * ny - ly * nx, nx, ny, nz}; // cross(lever, n), n
            int t = 0;
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
                for (int b = a; b < 6; ++b) acc[t++] += w * (g[a] * g[b]);
#pragma unroll
            for (int a = 0; a < 6; ++a) acc[21 + a] += w * (g[a] * h);
            acc[27] += fabs(h);
            if constexpr (MODE == 3) acc[28] += d2;
        } else {
            double Q[3][3];
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                Q[0][b] = py * M[2][b] - pz * M[1][b];
                Q[1][b] = pz * M[0][b] - px * M[2][b];
                Q[2][b] = px * M[1][b] - py * M[0][b];
            }
            acc[0] += w * (py * Q[0][2] - pz * Q[0][1]);  // H row 0: T00 T01 T02 Q00 Q01 Q02
            acc[1] += w * (pz * Q[0][0] - px * Q[0][2]);
            acc[2] += w * (px * Q[0][1] - py * Q[0][0]);
            acc[3] += w * Q[0][0]; acc[4] += w * Q[0][1]; acc[5] += w * Q[0][2];
            acc[6] += w * (pz * Q[1][0] - px * Q[1][2]);  // row 1: T11 T12 Q10 Q11 Q12
            acc[7] += w * (px * Q[1][1] - py * Q[1][0]);
            acc[8] += w * Q[1][0]; acc[9] += w * Q[1][1]; acc[10] += w * Q[1][2];
            acc[11] += w * (px * Q[2][1] - py * Q[2][0]); // row 2: T22 Q20 Q21 Q22
            acc[12] += w * Q[2][0]; acc[13] += w * Q[2][1]; acc[14] += w * Q[2][2];
            acc[15] += w * M[0][0]; acc[16] += w * M[0][1]; acc[17] += w * M[0][2]; // rows 3 .. 5: M
            acc[18] += w * M[1][1]; acc[19] += w * M[1][2];
            acc[20] += w * M[2][2];
            acc[21] += w * (py * u[2] - pz * u[1]);       // g = [p x u; u]
            acc[22] += w * (pz * u[0] - px * u[2]);
            acc[23] += w * (px * u[1] - py * u[0]);
            acc[24] += w * u[0]; acc[25] += w * u[1]; acc[26] += w * u[2];
            acc[27] += maha;
            acc[28] += d2;
        }
    }
    sf_block_sum4_stage(acc, sh);
    if (threadIdx.x < NV) partial[(size_t)blockIdx.x * ICP_NV + threadIdx.x] = sf_block_sum4_at(sh, threadIdx.x);
}

// fold PASS 0's block partials in block order into sums[48]: [0..7] as they are, w p, w q, w r2 to [40..46]; and leave the
// weighted centroids sum w p / sum w, sum w q / sum w (zero when sum w is not positive) for PASS 1 of MODE 0
__global__ __launch_bounds__(64) void k_icp_means(const double *__restrict__ partial, int nblocks, double *__restrict__ out,
                                                  double *__restrict__ mean)
{
    const int v = threadIdx.x;
    double a = 0.0;
    if (v < 15)
        for (int b = 0; b < nblocks; ++b) a += partial[(size_t)b * ICP_NV + v];
    if (v < 8) out[v] = a;
    else if (v < 15) out[32 + v] = a;
    const double sw = __shfl(a, 7);
    if (v >= 8 && v <= 13) mean[v - 8] = sw > 0.0 ? a / sw : 0.0;
}

} // namespace

extern "C" int sf_transform_points(sf_ctx *ctx, double *pts_dev, int64_t n, const double *Rt)
{
    if (!ctx || !pts_dev || !Rt || n < 0) { sf_set_error("sf_transform_points: bad argument"); return SF_ERR_ARG; }
    SF_HIP(hipSetDevice(ctx->device));
    if (!n) return SF_OK;
    sf_pool_guard tmp(ctx);
    double *dRt = nullptr;
    SF_CHECK(tmp.alloc(&dRt, 12));
    SF_HIP(hipMemcpyAsync(dRt, Rt, 12 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    SF_LAUNCH(ctx, "i0_transform", k_transform, dim3((unsigned)sf_div_up(n, 256)), dim3(256), (const double *)pts_dev,
              (const int64_t *)nullptr, n, (const double *)dRt, pts_dev);
    SF_HIP(hipStreamSynchronize(ctx->stream)); // Rt is a host buffer
    return SF_OK;
}

// The chain of the three entry points, which have checked their arguments, set the device and returned for m == 0: move the rows,
// find their nearest reference points, both sums passes with their folds, and the 48 numbers (layout in include/shotfpfh.h) back
// in `sums`.  `who` names the entry point in the empty-reference error.
// K18: with trim < 1 a key pass and the selection (select.hip) come between the search and pass A, queued like the rest; the cut stays
// on the device, where both sums passes read it, and n0, the rank and the cut come back behind the 48 numbers in the same copy.
static int icp_chain(const char *who, sf_ctx *ctx, sf_cloud *ref, const double *pts_dev, const double *nrm_dev, const int64_t *sel_dev,
                     int64_t m, const double *Rt, double d_max, int mode, double epsilon, int loss, double scale, double *sums,
                     double trim = 1.0)
{
    if (ref->n < 1) { sf_set_error("%s: empty reference cloud", who); return SF_ERR_ARG; }
    sf_pool_guard tmp(ctx);
    double *dRt = nullptr, *moved = nullptr, *partial = nullptr, *dout = nullptr, *dmean = nullptr;
    if (Rt) {
        SF_CHECK(tmp.alloc(&dRt, 12));
        SF_HIP(hipMemcpyAsync(dRt, Rt, 12 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    }
    SF_CHECK(tmp.alloc(&moved, (size_t)m * 3));
    SF_CHECK(tmp.alloc(&partial, (size_t)ICP_BLOCKS * ICP_NV));
    SF_CHECK(tmp.alloc(&dout, 80));
    SF_CHECK(tmp.alloc(&dmean, 8));
    SF_LAUNCH(ctx, "i0_transform", k_transform, dim3((unsigned)sf_div_up(m, 256)), dim3(256), pts_dev, sel_dev, m,
              (const double *)dRt, moved);
    sf_nbrs *nb = sf_knn_search(ctx, ref, moved, m, 1, SF_IN_DEVICE); // kdtree.query(points_aligned)
    if (!nb) return SF_ERR_HIP;
    struct nb_guard { sf_ctx *c; sf_nbrs *n; ~nb_guard() { sf_nbrs_free(c, n); } } nbg{ctx, nb};
    // both passes read the reference's normals: the weight comes from h or from M (fails when it was uploaded without normals)
    if (mode != 0) SF_CHECK(sf_cloud_ensure_sorted_normals(ctx, ref));
    SF_HIP(hipMemsetAsync(dout, 0, 48 * sizeof(double), ctx->stream)); // the slots of no pass, [47] among them
    // the k-NN lists are in PROCESSING order (queries sorted by cell): sums do not care, and qx / qy / qz follow it
    const dim3 grid(ICP_BLOCKS), block(256);
    const int32_t *qrow = (const int32_t *)nb->qrow;
    const double *no_mean = nullptr, *cut = nullptr;
    const bool trimmed = trim < 1.0;
    if (trimmed) {
        uint64_t *keys = nullptr;
        SF_CHECK(tmp.alloc(&keys, (size_t)m));
#define SF_ICP_KEYS(MODE)                                                                                                            \
    SF_LAUNCH(ctx, "i2_icp_keys", (k_icp_keys<MODE>), grid, block, nb->qx, nb->qy, nb->qz, nb->idx, qrow, ref->rec, nrm_dev, sel_dev, \
              (const double *)dRt, m, d_max, epsilon, keys)
        if (mode == 0) { SF_ICP_KEYS(0); }
        else if (mode == 1) { SF_ICP_KEYS(1); }
        else if (mode == 2) { SF_ICP_KEYS(2); }
        else { SF_ICP_KEYS(3); }
#undef SF_ICP_KEYS
        SF_CHECK(sf_select_launch(ctx, keys, m, 0, trim, dout + 48)); // [48] the cut, [52] n0, [53] the rank
        cut = dout + 48;
    }
#define SF_ICP_PASS(PASS, MODE, mean)                                                                                                \
    SF_LAUNCH(ctx, "i1_icp_sums", (k_icp_sums<PASS, MODE>), grid, block, nb->qx, nb->qy, nb->qz, nb->idx, qrow, ref->rec, nrm_dev,    \
              sel_dev, (const double *)dRt, m, d_max, epsilon, loss, scale, mean, cut, partial)
    if (mode == 0) { SF_ICP_PASS(0, 0, no_mean); }
    else if (mode == 1) { SF_ICP_PASS(0, 1, no_mean); }
    else if (mode == 2) { SF_ICP_PASS(0, 2, no_mean); }
    else { SF_ICP_PASS(0, 3, no_mean); }
    SF_LAUNCH(ctx, "i1_icp_means", k_icp_means, dim3(1), dim3(64), (const double *)partial, ICP_BLOCKS, dout, dmean);
    if (mode == 0) { SF_ICP_PASS(1, 0, (const double *)dmean); }
    else if (mode == 1) { SF_ICP_PASS(1, 1, no_mean); }
    else if (mode == 2) { SF_ICP_PASS(1, 2, no_mean); }
    else { SF_ICP_PASS(1, 3, no_mean); }
#undef SF_ICP_PASS
    SF_LAUNCH(ctx, "i1_icp_final", k_icp_final, dim3(1), dim3(64), (const double *)partial, ICP_BLOCKS, mode == 0 ? 10 : (mode == 1 ? 28 : 29),
              dout + 8);
    double all[56];
    SF_HIP(hipMemcpyAsync(all, dout, (trimmed ? 56 : 48) * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    SF_HIP(hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < 48; ++i) sums[i] = all[i];
    if (trimmed) { sums[37] = all[52]; sums[38] = all[53]; sums[47] = all[48]; }
    return SF_OK;
}

// the chain without a loss, into the caller's sums[40]: every weight is 1.0, and [7], the sum of the weights, belongs to no pass here
static int icp_chain_plain(const char *who, sf_ctx *ctx, sf_cloud *ref, const double *pts_dev, const double *nrm_dev,
                           const int64_t *sel_dev, int64_t m, const double *Rt, double d_max, int mode, double epsilon, double *sums)
{
    double all[48];
    SF_CHECK(icp_chain(who, ctx, ref, pts_dev, nrm_dev, sel_dev, m, Rt, d_max, mode, epsilon, 0, 1.0, all));
    for (int i = 0; i < 40; ++i) sums[i] = all[i];
    sums[7] = 0.0;
    return SF_OK;
}

extern "C" int sf_icp_accumulate(sf_ctx *ctx, sf_cloud *ref, const double *pts_dev, const int64_t *sel_dev, int64_t m,
                                 const double *Rt, double d_max, int mode, double *sums)
{
    if (!ctx || !ref || !pts_dev || !sums || m < 0 || (mode != 0 && mode != 1)) { sf_set_error("sf_icp_accumulate: bad argument"); return SF_ERR_ARG; }
    SF_HIP(hipSetDevice(ctx->device));
    for (int i = 0; i < 40; ++i) sums[i] = 0.0;
    if (!m) return SF_OK;
    return icp_chain_plain("sf_icp_accumulate", ctx, ref, pts_dev, nullptr, sel_dev, m, Rt, d_max, mode, 1.0, sums);
}

extern "C" int sf_icp_accumulate_gicp(sf_ctx *ctx, sf_cloud *ref, const double *pts_dev, const double *nrm_dev, const int64_t *sel_dev,
                                      int64_t m, const double *Rt, double d_max, double epsilon, double *sums)
{
    if (!ctx || !ref || !pts_dev || !nrm_dev || !sums || m < 0 || !(epsilon > 0.0 && epsilon <= 1.0)) {
        sf_set_error("sf_icp_accumulate_gicp: bad argument (epsilon must lie in (0, 1])");
        return SF_ERR_ARG;
    }
    SF_HIP(hipSetDevice(ctx->device));
    for (int i = 0; i < 40; ++i) sums[i] = 0.0;
    if (!m) return SF_OK;
    return icp_chain_plain("sf_icp_accumulate_gicp", ctx, ref, pts_dev, nrm_dev, sel_dev, m, Rt, d_max, 2, epsilon, sums);
}

// K17: a robust weight per kept pair (sums[48], layout in include/shotfpfh.h)
extern "C" int sf_icp_accumulate_robust(sf_ctx *ctx, sf_cloud *ref, const double *pts_dev, const double *nrm_dev, const int64_t *sel_dev,
                                        int64_t m, const double *Rt, double d_max, int mode, double epsilon, int loss, double scale,
                                        double *sums)
{
    const char *bad = nullptr;
    if (!ctx) bad = "ctx";
    else if (!ref) bad = "ref";
    else if (!pts_dev) bad = "pts_dev";
    else if (!sums) bad = "sums";
    else if (m < 0) bad = "m (negative)";
    else if (mode < 0 || mode > 2) bad = "mode (0 point to point, 1 point to plane, 2 generalized)";
    else if (mode == 2 && !nrm_dev) bad = "nrm_dev (mode 2 needs the scan's normals)";
    else if (mode == 2 && !(epsilon > 0.0 && epsilon <= 1.0)) bad = "epsilon (must lie in (0, 1])";
    else if (loss < 0 || loss > 4) bad = "loss (0 none, 1 Huber, 2 Cauchy, 3 Geman-McClure, 4 Tukey)";
    else if (!(scale > 0.0 && scale < INFINITY)) bad = "scale (must be positive and finite)";
    if (bad) { sf_set_error("sf_icp_accumulate_robust: bad argument %s", bad); return SF_ERR_ARG; }
    SF_HIP(hipSetDevice(ctx->device));
    for (int i = 0; i < 48; ++i) sums[i] = 0.0;
    if (!m) return SF_OK;
    return icp_chain("sf_icp_accumulate_robust", ctx, ref, pts_dev, nrm_dev, sel_dev, m, Rt, d_max, mode, epsilon, loss, scale, sums);
}

// K18: trimmed ICP, the chain over the best-fitting share of the pairs inside d_max (sums[48], layout in include/shotfpfh.h)
extern "C" int sf_icp_accumulate_trimmed(sf_ctx *ctx, sf_cloud *ref, const double *pts_dev, const double *nrm_dev, const int64_t *sel_dev,
                                         int64_t m, const double *Rt, double d_max, int mode, double epsilon, int loss, double scale,
                                         double trim, double *sums)
{
    const char *bad = nullptr;
    if (!ctx) bad = "ctx";
    else if (!ref) bad = "ref";
    else if (!pts_dev) bad = "pts_dev";
    else if (!sums) bad = "sums";
    else if (m < 0) bad = "m (negative)";
    else if (mode < 0 || mode > 2) bad = "mode (0 point to point, 1 point to plane, 2 generalized)";
    else if (mode == 2 && !nrm_dev) bad = "nrm_dev (mode 2 needs the scan's normals)";
    else if (mode == 2 && !(epsilon > 0.0 && epsilon <= 1.0)) bad = "epsilon (must lie in (0, 1])";
    else if (loss < 0 || loss > 4) bad = "loss (0 none, 1 Huber, 2 Cauchy, 3 Geman-McClure, 4 Tukey)";
    else if (!(scale > 0.0 && scale < INFINITY)) bad = "scale (must be positive and finite)";
    else if (!(trim > 0.0 && trim <= 1.0)) bad = "trim (must lie in (0, 1])";
    if (bad) { sf_set_error("sf_icp_accumulate_trimmed: bad argument %s", bad); return SF_ERR_ARG; }
    SF_HIP(hipSetDevice(ctx->device));
    for (int i = 0; i < 48; ++i) sums[i] = 0.0;
    if (!m) return SF_OK;
    SF_CHECK(icp_chain("sf_icp_accumulate_trimmed", ctx, ref, pts_dev, nrm_dev, sel_dev, m, Rt, d_max, mode, epsilon, loss, scale, sums, trim));
    if (trim == 1.0) sums[37] = sums[38] = sums[0]; // no selection: every pair inside d_max is used, and the cut stays 0
    return SF_OK;
}

// K19: the symmetric point-to-plane objective, the chain in its fourth mode with a loss and a trim (sums[48], layout in include/shotfpfh.h)
extern "C" int sf_icp_accumulate_symmetric(sf_ctx *ctx, sf_cloud *ref, const double *pts_dev, const double *nrm_dev, const int64_t *sel_dev,
                                           int64_t m, const double *Rt, double d_max, int loss, double scale, double trim, double *sums)
{
    const char *bad = nullptr;
    if (!ctx) bad = "ctx";
    else if (!ref) bad = "ref";
    else if (!pts_dev) bad = "pts_dev";
    else if (!nrm_dev) bad = "nrm_dev (the symmetric objective needs the scan's normals)";
    else if (!sums) bad = "sums";
    else if (m < 0) bad = "m (negative)";
    else if (loss < 0 || loss > 4) bad = "loss (0 none, 1 Huber, 2 Cauchy, 3 Geman-McClure, 4 Tukey)";
    else if (!(scale > 0.0 && scale < INFINITY)) bad = "scale (must be positive and finite)";
    else if (!(trim > 0.0 && trim <= 1.0)) bad = "trim (must lie in (0, 1])";
    if (bad) { sf_set_error("sf_icp_accumulate_symmetric: bad argument %s", bad); return SF_ERR_ARG; }
    SF_HIP(hipSetDevice(ctx->device));
    for (int i = 0; i < 48; ++i) sums[i] = 0.0;
    if (!m) return SF_OK;
    SF_CHECK(icp_chain("sf_icp_accumulate_symmetric", ctx, ref, pts_dev, nrm_dev, sel_dev, m, Rt, d_max, 3, 1.0, loss, scale, sums, trim));
    if (trim == 1.0) sums[37] = sums[38] = sums[0]; // no selection: every pair inside d_max is used, and the cut stays 0
    return SF_OK;
}
