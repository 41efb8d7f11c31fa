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
// registers): (1) the three elections (64-bit LDS atomic max on rho's bit pattern) and the gate count; (2) every winner of A, B
// and G claims its slot -- compare-and-swap of its key into the key with the sign bit set, which the other winners of the quad
// still read as that key, and which tells a second holder of that key that it has met a tie (shot_core.h: the keypoint is
// reported and its row computed again by k_shot_tied) -- and the winner of A adds its S3/S4, S6/S7 values into vx; (3) the
// claimed slots receive their tagged value.  The row is ((A + vx) + B) + G per bin in that fixed order: vx
// receives two addends at most (from the winners of bin ^ 1 and bin ^ 2), so every bit of the row is independent of the
// order of the atomics, and at n = 11 the sums equal the team form's (k_shot_team) bin for bin.
// HBM roofline, algorithmic bytes: the 256 n B row + 24 B keypoint + 72 B frame per keypoint, plus the list (4 B per entry)
// and the 48 B record of every neighbour, read three times.
#include "common.h"
#include "device_util.h"
#include "host_stage.h"
#include "shot_core.h"
#include <hip/amd_detail/amd_hip_unsafe_atomics.h>

namespace {

constexpr unsigned long long SHOT_BINS_SIGN = 0x8000000000000000ull;

// One wave per keypoint, blockDim.x / 64 waves per workgroup, each with its own 4 x 32 n slots of the dynamic LDS.
// lrf: finished frames (K4 with skip_zero); err: set to 1 (a plain store) when a keypoint that passes the gate has a neighbour
// in cosine bin n.  Rows of keypoints that fail the gate are zero.
__global__ __launch_bounds__(256) void k_shot_bins(const double *__restrict__ rec, const double *__restrict__ qx,
                                                   const double *__restrict__ qy, const double *__restrict__ qz,
                                                   const int64_t *__restrict__ offset, const int32_t *__restrict__ cnt,
                                                   const int32_t *__restrict__ idx, const int32_t *__restrict__ qrow, int64_t m,
                                                   shot_consts K, const double *__restrict__ lrf, int n, int min_nb,
                                                   double *__restrict__ out, int *__restrict__ err, shot_ties ties)
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

    // one step of a sweep (shot_geometry128 with the bin count a run-time value)
    auto geometry128 = [&](int t0, shot_kept (&g)[2], unsigned long long (&pos)[2], unsigned long long (&over)[2]) {
        shot_geometry128<0, true>(rec, idx + s, t0, k, lane, px, py, pz, E, K.half_r, n, nd, g, pos, over);
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
                atomicMax(&keyA[shot_slot_a<0>(g[u])], shot_key(g[u]));
                atomicMax(&keyB[shot_slot_b<0>(g[u])], shot_key(g[u]));
                atomicMax(&keyG[shot_slot_g<0>(g[u])], shot_key(g[u]));
            }
        }
    }
    if (!(npos > min_nb) || any_over) { // (min_nb arrives clamped into [-1, 2^31 - 1])
        if (npos > min_nb && lane == 0) *err = 1; // the reference raises IndexError for the whole call: the row is not used
        for (int b = lane; b < S; b += 64) o[b] = 0.0;
        return;
    }
    SF_SHOT_SYNC();

    // ---- sweep 2: A, B and G claimed (key -> key | sign), S3/S4 and S6/S7 added into vx ----
    bool tie = false;
    for (int t0 = 0; t0 < k; t0 += 128) {
        shot_kept g[2];
        unsigned long long pos[2], over[2];
        geometry128(t0, g, pos, over);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (g[u].bins1 >> 31) {
                const unsigned long long key = shot_key(g[u]);
                const unsigned iA = shot_slot_a<0>(g[u]);
                // (bit 1 of a slot: z > 0, bit 0: outer shell; the other half-space's key may be claimed already: its sign bit off)
                const unsigned long long own = keyA[iA], other_shell = keyA[iA ^ 1u], other_half = keyA[iA ^ 2u] & ~SHOT_BINS_SIGN;
                double vA, v_cd, v_ef, adth;
                shot_weights(g[u], K, vA, v_cd, v_ef, adth);
                if ((own & ~SHOT_BINS_SIGN) == key) {
                    tie |= other_half == key;
                    if (atomicCAS(&keyA[iA], key, shot_claimed(key)) == key) {
                        if (shot_writes_cd(iA & 1u, other_shell) && v_cd != 0.0) unsafeAtomicAdd(&vx[iA ^ 1u], v_cd);
                        if (shot_writes_ef(key, other_half, iA & 2u) && v_ef != 0.0) unsafeAtomicAdd(&vx[iA ^ 2u], v_ef);
                    } else {
                        tie = true; // (another holder of this key was here first)
                    }
                }
                tie |= atomicCAS(&keyB[shot_slot_b<0>(g[u])], key, shot_claimed(key)) == shot_claimed(key);
                tie |= atomicCAS(&keyG[shot_slot_g<0>(g[u])], key, shot_claimed(key)) == shot_claimed(key);
            }
        }
    }
    SF_SHOT_SYNC();

    // ---- sweep 3: the claimed slots receive their value ----
    for (int t0 = 0; t0 < k; t0 += 128) {
        shot_kept g[2];
        unsigned long long pos[2], over[2];
        geometry128(t0, g, pos, over);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (g[u].bins1 >> 31) {
                const unsigned long long claimed = shot_key(g[u]) | SHOT_BINS_SIGN;
                const unsigned iA = shot_slot_a<0>(g[u]), iB = shot_slot_b<0>(g[u]), iG = shot_slot_g<0>(g[u]);
                const bool wA = keyA[iA] == claimed, wB = keyB[iB] == claimed, wG = keyG[iG] == claimed;
                if (wA || wB || wG) {
                    double vA, v_cd, v_ef, adth;
                    shot_weights(g[u], K, vA, v_cd, v_ef, adth);
                    if (wA) atomicCAS(&keyA[iA], claimed, tag_value(vA));
                    if (wB) atomicCAS(&keyB[iB], claimed, tag_value(fabs(g[u].dc)));
                    if (wG) atomicCAS(&keyG[iG], claimed, tag_value(adth));
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
    const double scale = shot_row_scale(ss, 1, false);
    for (int b = lane; b < S; b += 64) {
        const double v = ((shot_untag(keyA[b]) + vx[b]) + shot_untag(keyB[b])) + shot_untag(keyG[b]);
        sf_store_stream(o + b, v * scale);
    }
    if (__ballot(tie) && lane == 0) shot_report_tie(ties, q);
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
    double *dlrf = nullptr, *dout;
    int *derr = nullptr;
    SF_CHECK(guard.alloc(&dlrf, (size_t)m * 9));
    SF_CHECK(guard.alloc(&derr, 1));
    SF_CHECK(stage_out(guard, out, (size_t)m * row, flags, &dout));
    SF_HIP(hipMemsetAsync(derr, 0, sizeof(int), ctx->stream));
    SF_CHECK(sf_launch_shot_lrf(ctx, c, nb, 0, 1, dlrf));
    shot_consts K;
    int nmin;
    SF_CHECK(sf_shot_consts(ctx, nb->radius, min_nb, &K, &nmin)); // (the coefficients: once per context; K5 shares them)
    shot_ties ties;
    SF_CHECK(sf_shot_ties_begin(ctx, guard, m, &ties));
    if (m) {
        const int w = shot_bins_waves(n);
        const size_t lds = (size_t)w * 4 * row * sizeof(unsigned long long);
        sf_launch_timer t_(ctx, "k5_shot_bins");
        hipLaunchKernelGGL(k_shot_bins, dim3(sf_xcd_grid(sf_div_up(m, w))), dim3(64 * w), lds, ctx->stream, c->rec, nb->qx, nb->qy,
                           nb->qz, nb->offset, nb->count, nb->idx, nb->qrow, m, K, (const double *)dlrf, n, nmin, dout, derr, ties);
        SF_HIP(hipGetLastError());
    }
    if (m) SF_CHECK(sf_shot_ties_finish<0>(ctx, c, nb, K, dlrf, false, n, 1, dout, ties));
    SF_CHECK(finish_out(ctx, out, (size_t)m * row, flags, dout));
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
