// shot_bins.hip -- the reference's serial SHOT (compute_shot_descriptor, shot.py:310-499) with ANY number of cosine bins n,
// 1 <= n <= SF_SHOT_MAX_COSINE_BINS (rows of 32 n bins, (cos, azimuth, elevation, shell) in C order).
//
// K5's tuned forms (shot.hip) are built around 352-bin rows -- 9-bit bin fields, LDS tables of exactly 352 slots, a slot
// re-mapping, a literal 11 in the cosine bin -- and stay as they are; this is a kernel of its own, with the bin count a runtime
// argument.  Same arithmetic per neighbour (the helpers of shot_core.h), same last-writer-wins semantics of the ten statements.
// Mapping: one wave per keypoint, the list streamed 128 neighbours at a time, so a list of any length works.  LDS per wave:
// four tables of 32 n 8-byte slots -- the keys of the S2+S5+S8+S10 (A), S1 (B) and S9 (G) elections, later their tagged values,
// and vx, the S3/S4 + S6/S7 addends by destination bin -- 1 KiB x n, 64 KiB at n = 64; the waves per workgroup follow from n
// (shot_bins_waves).  Three sweeps over the list, each recomputing the geometry (no wave can keep a list of any length in
// registers): (1) the three elections (64-bit LDS atomic max on rho's bit pattern) and the gate count; (2) every winner of A
// claims its slot -- compare-and-swap of its key into the key with the sign bit set, which the other winners of the quad still
// read as that key -- and adds its S3/S4, S6/S7 values into vx, the winners of B and G replace their key by their tagged
// value; (3) the claimed A slots receive their tagged value.  The row is ((A + vx) + B) + G per bin in that fixed order: vx
// receives two addends at most (from the winners of bin ^ 1 and bin ^ 2), so every bit of the row is independent of the
// order of the atomics, and at n = 11 the sums equal the team form's (k_shot_team) bin for bin.
// HBM roofline, algorithmic bytes: the 256 n B row + 24 B keypoint + 72 B frame per keypoint, plus the list (4 B per entry)
// and the 48 B record of every neighbour, read three times.
#include "common.h"
#include "device_util.h"
#include "host_stage.h"
#include "shot_core.h"
#include <hip/amd_detail/amd_hip_unsafe_atomics.h>

int sf_launch_shot_lrf(sf_ctx *ctx, sf_cloud *c, sf_nbrs *nb, int raw, int skip_zero, double *dlrf); // normals_lrf.hip

namespace {

constexpr unsigned long long SHOT_BINS_SIGN = 0x8000000000000000ull;

// The geometry of one neighbour for n cosine bins: shot_geometry (shot.hip) with the bin count a runtime value.  Bins of up to
// 2 048-slot rows do not fit its 9-bit fields: bins0 = base | bcos << 16, bins1 = valid << 31 | bth << 2 | (base & 3) (bits 0-1,
// shell and half-space, as shot_weights reads them).  Returns false for a neighbour whose cosine bin is n (a clipped cosine of
// exactly +1 with n even: rint(n - 0.5) = n, the reference's IndexError), which then takes part in nothing.
__device__ inline bool shot_bins_geometry(double cx, double cy, double cz, double d2, double nx, double ny, double nz,
                                          const double *E, double half_r, int n, double nd, shot_kept &o)
{
    double rho, inv_rho;
    sf_sqrt_rsqrt(d2, rho, inv_rho);
    const double lx = sf_dot3(cx, cy, cz, E[0], E[3], E[6]);
    const double ly = sf_dot3(cx, cy, cz, E[1], E[4], E[7]);
    const double lz = sf_dot3(cx, cy, cz, E[2], E[5], E[8]);
    double cosine = sf_dot3(nx, ny, nz, E[2], E[5], E[8]);
    cosine = fmin(fmax(cosine, -1.0), 1.0);
    // bin_dist = (cosine + 1.0) * n / 2.0 - 0.5 in that order, unfused (shot.py:386); rint rounds half to even (:387)
    const double cpos = (cosine + 1.0) * nd / 2.0 - 0.5;
    const double cf = rint(cpos);
    const int ci = (int)cf; // 0 .. n (-0.5 rounds to -0)
    if (ci >= n) return false;
    const int ti = azimuth_octant_wave(lx, ly);
    const int pi_ = lz > 0.0 ? 1 : 0;
    const int ri = rho > half_r ? 1 : 0;
    const double dc = cpos - cf;
    const int sc = (dc > 0.0) - (dc < 0.0);
    int cin = ci + sc; // -1 .. n, wrapped as the reference's % n does (shot.py:401): n = 1 wraps onto itself
    cin = cin < 0 ? n - 1 : (cin >= n ? 0 : cin);
    // the azimuth neighbour: the side of the octant's centre ray (shot_geometry has the derivation)
    const double C8 = 0.9238795325112867, S8 = 0.3826834323650898; // cos, sin of pi/8
    const double am = fmax(fabs(lx), fabs(ly)), bm = fmin(fabs(lx), fabs(ly));
    const double crs = __builtin_fma(C8, bm, -(S8 * am));
    const double dot = __builtin_fma(C8, am, S8 * bm);
    const double cross = (ti & 1) ? -crs : crs;
    int sth;
    if (fabs(cross) > 1e-9 * (fabs(lx) + fabs(ly))) {
        sth = cross > 0.0 ? 1 : -1;
    } else { // on (or within rounding of) the centre ray, or lx = ly = 0: the reference's expression decides
        const double tsz = 2 * SHOT_PI / 8;
        double dth = (atan2(ly, lx) - (-SHOT_PI + ti * tsz)) / tsz - 0.5;
        dth = fmin(fmax(dth, -0.5), 0.5);
        sth = (dth > 0.0) - (dth < 0.0);
    }
    const int tin = (ti + sth) & 7;
    const unsigned base = (unsigned)(((ci * 8 + ti) * 2 + pi_) * 2 + ri);
    const unsigned bcos = (unsigned)(((cin * 8 + ti) * 2 + pi_) * 2 + ri);
    const unsigned bth = (unsigned)(((ci * 8 + tin) * 2 + pi_) * 2 + ri);
    // lz / rho with one residual correction (see shot_geometry: acos is steep at +-1)
    double lzr = lz * inv_rho;
    lzr = __builtin_fma(__builtin_fma(-lzr, rho, lz), inv_rho, lzr);
    o.rho = rho; o.dc = dc; o.tcross = cross; o.tdot = dot; o.lzr = lzr;
    o.bins0 = base | (bcos << 16);
    o.bins1 = 0x80000000u | (bth << 2) | (base & 3u);
    return true;
}

__device__ inline unsigned shot_bins_a(const shot_kept &g) { return g.bins0 & 0xffffu; }
__device__ inline unsigned shot_bins_b(const shot_kept &g) { return g.bins0 >> 16; }
__device__ inline unsigned shot_bins_g(const shot_kept &g) { return (g.bins1 >> 2) & 0xfffu; }

// One wave per keypoint, blockDim.x / 64 waves per workgroup, each with its own 4 x 32 n slots of the dynamic LDS.
// lrf: finished frames (K4 with skip_zero); err: set to 1 (a plain store) when a keypoint that passes the gate has a neighbour
// in cosine bin n.  Rows of keypoints that fail the gate are zero.
__global__ __launch_bounds__(256) void k_shot_bins(const double *__restrict__ rec, const double *__restrict__ qx,
                                                   const double *__restrict__ qy, const double *__restrict__ qz,
                                                   const int64_t *__restrict__ offset, const int32_t *__restrict__ cnt,
                                                   const int32_t *__restrict__ idx, const int32_t *__restrict__ qrow, int64_t m,
                                                   shot_consts K, const double *__restrict__ lrf, int n, int min_nb,
                                                   double *__restrict__ out, int *__restrict__ err)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long shot_bins_lds[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nw = blockDim.x >> 6;
    const int S = 32 * n; // bins per row = slots per table
    unsigned long long *const keyA = shot_bins_lds + (size_t)4 * S * wave;
    unsigned long long *const keyB = keyA + S;
    unsigned long long *const keyG = keyB + S;
    double *const vx = reinterpret_cast<double *>(keyG + S);
    const int64_t q = sf_xcd_block() * nw + wave;
    if (q >= m) return;
    const int64_t s = offset[q];
    const int k = sf_uniform(cnt[q]);
    const int64_t row = qrow ? qrow[q] : q;
    double *o = out + (int64_t)S * row;
    const double px = qx[q], py = qy[q], pz = qz[q];
    const double nd = (double)n;
    for (int b = lane; b < 4 * S; b += 64) keyA[b] = 0ull;
    double E[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) E[i] = lrf[9 * row + i];
    SF_SHOT_SYNC(); // (the cleared tables)

    // one step of a sweep: 128 neighbours gathered together, their geometry; bins1 bit 31 marks a neighbour at non-zero
    // distance whose bins are in range, `over` the ones at non-zero distance in cosine bin n
    auto geometry128 = [&](int t0, shot_kept (&g)[2], unsigned long long (&pos)[2], unsigned long long (&over)[2]) {
        int jj[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int t = t0 + 64 * u + lane;
            jj[u] = t < k ? SF_LIST_LOAD(idx + s + t) : -1;
        }
        double cx[2], cy[2], cz[2], nx[2], ny[2], nz[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            double x, y, z;
            sf_load_pn(rec, jj[u] < 0 ? 0 : jj[u], x, y, z, nx[u], ny[u], nz[u]);
            cx[u] = x - px; cy[u] = y - py; cz[u] = z - pz;
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            g[u].bins1 = 0u;
            const double d2 = (cx[u] * cx[u] + cy[u] * cy[u]) + cz[u] * cz[u];
            const bool on = jj[u] >= 0 && d2 > 0.0;
            bool bad = false;
            if (on) bad = !shot_bins_geometry(cx[u], cy[u], cz[u], d2, nx[u], ny[u], nz[u], E, K.half_r, n, nd, g[u]);
            pos[u] = __ballot(on);
            over[u] = __ballot(bad);
        }
    };

    // ---- sweep 1: the three elections, the gate count (shot.py:360) ----
    int npos = 0;
    bool any_over = false;
    for (int t0 = 0; t0 < k; t0 += 128) {
        shot_kept g[2];
        unsigned long long pos[2], over[2];
        geometry128(t0, g, pos, over);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            npos += __popcll(pos[u]);
            any_over |= over[u] != 0ull;
            if (g[u].bins1 >> 31) {
                const unsigned long long key = (unsigned long long)__double_as_longlong(g[u].rho);
                atomicMax(&keyA[shot_bins_a(g[u])], key);
                atomicMax(&keyB[shot_bins_b(g[u])], key);
                atomicMax(&keyG[shot_bins_g(g[u])], key);
            }
        }
    }
    if (!(npos > min_nb) || any_over) { // (min_nb arrives clamped into [-1, 2^31 - 1])
        if (npos > min_nb && lane == 0) *err = 1; // the reference raises IndexError for the whole call: the row is not used
        for (int b = lane; b < S; b += 64) o[b] = 0.0;
        return;
    }
    SF_SHOT_SYNC();

    // ---- sweep 2: A claimed (key -> key | sign), S3/S4 and S6/S7 added into vx; B and G resolved ----
    for (int t0 = 0; t0 < k; t0 += 128) {
        shot_kept g[2];
        unsigned long long pos[2], over[2];
        geometry128(t0, g, pos, over);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (g[u].bins1 >> 31) {
                const unsigned long long key = (unsigned long long)__double_as_longlong(g[u].rho);
                const unsigned iA = shot_bins_a(g[u]);
                const bool up = iA & 2u, odd = iA & 1u; // (bit 1: z > 0, bit 0: outer shell)
                const unsigned long long own = keyA[iA], other_shell = keyA[iA ^ 1u], other_half = keyA[iA ^ 2u] & ~SHOT_BINS_SIGN;
                double vA, v_cd, v_ef, adth;
                shot_weights(g[u], K, vA, v_cd, v_ef, adth);
                if (own == key && atomicCAS(&keyA[iA], key, key | SHOT_BINS_SIGN) == key) {
                    // S3/S4: the farthest neighbour of the cell over BOTH shells; S6/S7: the farther of the two half-spaces'
                    // winners (equal distances: z > 0, as in every K5 form)
                    if ((odd || other_shell == 0ull) && v_cd != 0.0) unsafeAtomicAdd(&vx[iA ^ 1u], v_cd);
                    if ((key > other_half || (key == other_half && up)) && v_ef != 0.0) unsafeAtomicAdd(&vx[iA ^ 2u], v_ef);
                }
                atomicCAS(&keyB[shot_bins_b(g[u])], key, tag_value(fabs(g[u].dc)));
                atomicCAS(&keyG[shot_bins_g(g[u])], key, tag_value(adth));
            }
        }
    }
    SF_SHOT_SYNC();

    // ---- sweep 3: the claimed A slots receive their value ----
    for (int t0 = 0; t0 < k; t0 += 128) {
        shot_kept g[2];
        unsigned long long pos[2], over[2];
        geometry128(t0, g, pos, over);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (g[u].bins1 >> 31) {
                const unsigned long long claimed = (unsigned long long)__double_as_longlong(g[u].rho) | SHOT_BINS_SIGN;
                const unsigned iA = shot_bins_a(g[u]);
                if (keyA[iA] == claimed) {
                    double vA, v_cd, v_ef, adth;
                    shot_weights(g[u], K, vA, v_cd, v_ef, adth);
                    atomicCAS(&keyA[iA], claimed, tag_value(vA));
                }
            }
        }
    }
    SF_SHOT_SYNC();

    // ---- the row: ((A + vx) + B) + G per bin, L2-normalised (shot.py:496-497) ----
    double ss = 0.0;
    for (int b = lane; b < S; b += 64) {
        const double v = ((shot_untag(keyA[b]) + vx[b]) + shot_untag(keyB[b])) + shot_untag(keyG[b]);
        ss += v * v;
    }
    double nrm, inv_nrm;
    sf_sqrt_rsqrt_uniform(sf_wave_sum(ss), nrm, inv_nrm);
    const double scale = nrm > 0.0 ? inv_nrm : 0.0;
    for (int b = lane; b < S; b += 64) {
        const double v = ((shot_untag(keyA[b]) + vx[b]) + shot_untag(keyB[b])) + shot_untag(keyG[b]);
        sf_store_stream(o + b, v * scale);
    }
}

} // namespace

// Waves per workgroup for n cosine bins: as many as keep the workgroup's LDS within 64 KiB (4 up to n = 16, 2 up to 32, 1 above).
static int shot_bins_waves(int n) { return n <= 16 ? 4 : (n <= 32 ? 2 : 1); }

// compute_shot_descriptor with n_cosine_bins = n (shot.py:310-499): K4 with skip_zero, then k_shot_bins.
extern "C" int sf_shot_serial_bins(sf_ctx *ctx, sf_cloud *c, sf_nbrs *nb, int64_t n_cosine_bins, int64_t min_nb, double *out,
                                   int flags)
{
    SF_CHECK(check_nbrs(ctx, c, nb, "sf_shot_serial_bins"));
    if (!out) { sf_set_error("sf_shot_serial_bins: null out"); return SF_ERR_ARG; }
    if (n_cosine_bins < 1 || n_cosine_bins > SF_SHOT_MAX_COSINE_BINS) {
        sf_set_error("sf_shot_serial_bins: n_cosine_bins = %lld outside [1, %d]", (long long)n_cosine_bins, SF_SHOT_MAX_COSINE_BINS);
        return SF_ERR_ARG;
    }
    SF_CHECK(sf_cloud_ensure_sorted_normals(ctx, c));
    const int n = (int)n_cosine_bins;
    const int64_t m = nb->m;
    const size_t row = (size_t)32 * n;
    sf_pool_guard guard(ctx);
    double *dlrf = nullptr, *dout = out;
    int *derr = nullptr;
    SF_CHECK(guard.alloc(&dlrf, (size_t)m * 9));
    SF_CHECK(guard.alloc(&derr, 1));
    if (!(flags & SF_OUT_DEVICE)) SF_CHECK(guard.alloc(&dout, (size_t)m * row));
    SF_HIP(hipMemsetAsync(derr, 0, sizeof(int), ctx->stream));
    SF_CHECK(sf_launch_shot_lrf(ctx, c, nb, 0, 1, dlrf));
    if (!ctx->shot_coef) { // (once per context; K5 shares it)
        SF_HIP(hipMalloc(&ctx->shot_coef, sizeof(SF_SHOT_COEF)));
        SF_HIP(hipMemcpy(ctx->shot_coef, SF_SHOT_COEF, sizeof(SF_SHOT_COEF), hipMemcpyHostToDevice));
    }
    if (m) {
        const double r_ = nb->radius;
        const shot_consts K{r_, r_ / 2, r_ / 4, r_ * 3 / 4, 1.0 / (r_ / 2), ctx->shot_coef}; // as launch_shot (shot.py:95-117, 235)
        const int nmin = (int)std::min<int64_t>(std::max<int64_t>(min_nb, -1), 2147483647LL);
        const int w = shot_bins_waves(n);
        const size_t lds = (size_t)w * 4 * row * sizeof(unsigned long long);
        sf_launch_timer t_(ctx, "k5_shot_bins");
        hipLaunchKernelGGL(k_shot_bins, dim3(sf_xcd_grid(sf_div_up(m, w))), dim3(64 * w), lds, ctx->stream, c->rec, nb->qx, nb->qy,
                           nb->qz, nb->offset, nb->count, nb->idx, nb->qrow, m, K, (const double *)dlrf, n, nmin, dout, derr);
        SF_HIP(hipGetLastError());
    }
    if (dout != out && m) SF_HIP(hipMemcpyAsync(out, dout, (size_t)m * row * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    int herr = 0;
    SF_HIP(hipMemcpyAsync(&herr, derr, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    SF_HIP(hipStreamSynchronize(ctx->stream));
    if (herr) {
        sf_set_error("sf_shot_serial_bins: a neighbour of a keypoint that passes the gate falls in cosine bin %d, past the last "
                     "(%d): a clipped cosine of +1 with an even bin count, where the reference raises IndexError", n, n - 1);
        return SF_ERR_BIN_RANGE;
    }
    return SF_OK;
}
