// spin.hip -- K24: spin images (Johnson, Hebert 1999; pcl::SpinImageEstimation), the local descriptor that needs no reference
// frame: every neighbour of a keypoint p with axis n is reduced to two cylindrical coordinates about the line through p along n --
// alpha, its distance from the line, and beta, its signed height along it -- and spread bilinearly over a small 2-D image of
// (W + 1) x NV nodes, NV = 2 W + 1 (signed beta) or W + 1 (|beta|), node (iu, iv) at iu NV + iv of a row of D <= 4096 doubles.
// The image covers the cylinder of radius and half-height R / sqrt 2, inscribed in the search ball: the ball's lists suffice.
// The definition -- decided here, modelled on PCL -- is tests/spin_numpy.py: unfused float64 in the statement's order, one IEEE
// root, and the two bilinear fractions quantised to 2^-16 of a bin, so that the four weights of a neighbour are INTEGERS that sum
// to exactly 2^32.  Bin contents are integers: a row is exact whatever the order of the adds, of a list or of the cloud, a call
// repeats bit for bit, and one 64-bit counter per node does what USC's continuous weights need the two limbs of usc_acc.h for.
//
// Mapping: k_usc's streaming shape.  One wave per keypoint, blockDim.x / 64 independent waves per workgroup (spin_waves), the
// list in steps of 128 (shot_list_entry / shot_gather_entry), any length.  A wave owns D 64-bit counters of the dynamic LDS
// (1 224 B at W = 8 signed, 32 040 B at W = 44): cleared, fed by up to four 64-bit LDS integer atomic adds per neighbour, read
// out by the wave; the phases are ordered by SF_SHOT_SYNC, never a workgroup barrier.  W, the mode bits, the scale and min_cos are
// wave-uniform arguments (scalar registers).  No transcendental function, no table.
// Budget per keypoint: the 8 D B row (the HBM floor), 24 B keypoint + 24 B axis, per list entry 4 B index +
// 48 B record, 52 B (the records of a resident cloud come from L2), and up to four LDS atomics; float64 vector instructions per
// entry as counted in the build's ISA listing (profiles/spin_isa.md): 46, the root's expansion among them, 52 with the support angle.
// Surface points sit near beta = 0: the adds of a step pile onto few nodes, and same-address LDS atomics serialise -- the bound
// expected on curved surfaces.  Measured (tools/bench_spin.py, profiles/spin_bench.json) it does not show: a thin sphere's entries
// cost no more than a uniform cloud's, and the kernel sits nearest its row-write floor.  A per-lane pre-combination of same-node
// adds is therefore not built.
#include "common.h"
#include "device_util.h"
#include "host_stage.h"
#include "shot_core.h"

#include <cmath>

namespace {

#define SPIN_MAX_LIST (1 << 24) // a list this long or longer is refused (sf_usc's cap; the counters would stay below 2^56)
#define SPIN_SIGNED 1           // mode bits
#define SPIN_MIN_COS 2
#define SPIN_NORMALIZE 4

// One wave per keypoint, blockDim.x / 64 waves per workgroup, each with its own D counters of the dynamic LDS.
// axes: m x 3, by caller row; contrib (nullable): the contributing entries per keypoint, by caller row; err: set to 1 (a plain
// store) by a list of SPIN_MAX_LIST entries or more.
__global__ __launch_bounds__(256) void k_spin(const double *__restrict__ rec, const double *__restrict__ qx,
                                              const double *__restrict__ qy, const double *__restrict__ qz,
                                              const int64_t *__restrict__ offset, const int32_t *__restrict__ cnt,
                                              const int32_t *__restrict__ idx, const int32_t *__restrict__ qrow, int64_t m,
                                              const double *__restrict__ axes, double inv_bin, int W, int mode, double min_cos,
                                              int min_nb, double *__restrict__ out, int32_t *__restrict__ contrib,
                                              int *__restrict__ err)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long spin_lds[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nw = blockDim.x >> 6;
    const bool sgn = mode & SPIN_SIGNED, use_cos = mode & SPIN_MIN_COS;
    const int NV = sgn ? 2 * W + 1 : W + 1;
    const int D = (W + 1) * NV;
    const double Wd = (double)W;
    unsigned long long *const acc = spin_lds + (size_t)D * wave;
    const int64_t q = sf_xcd_block() * nw + wave;
    if (q >= m) return;
    const int64_t s = offset[q];
    const int k = sf_uniform(cnt[q]);
    const int64_t row = qrow ? qrow[q] : q;
    double *o = out + (int64_t)D * row;
    const double px = qx[q], py = qy[q], pz = qz[q];
    const double ax = axes[3 * row], ay = axes[3 * row + 1], az = axes[3 * row + 2];
    for (int b = lane; b < D; b += 64) acc[b] = 0ull;
    SF_SHOT_SYNC(); // (the cleared counters)

    int npos = 0;
    const int steps_end = k < SPIN_MAX_LIST ? k : 0; // (a list that is refused is not walked)
    for (int t0 = 0; t0 < steps_end; t0 += 128) {
        double cx[2], cy[2], cz[2], nx[2], ny[2], nz[2];
        int jj[2];
        bool on[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) jj[u] = shot_list_entry<true>(idx + s, t0 + 64 * u + lane, k); // (both indices before a record)
#pragma unroll
        for (int u = 0; u < 2; ++u) on[u] = shot_gather_entry(rec, jj[u], px, py, pz, cx[u], cy[u], cz[u], nx[u], ny[u], nz[u]);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const double d2 = (cx[u] * cx[u] + cy[u] * cy[u]) + cz[u] * cz[u];
            const double beta = (ax * cx[u] + ay * cy[u]) + az * cz[u];
            double a2 = d2 - beta * beta;
            a2 = a2 < 0.0 ? 0.0 : a2;
            const double uu = sqrt(a2) * inv_bin; // (the IEEE root: correctly rounded)
            const double t = (sgn ? beta : fabs(beta)) * inv_bin;
            // every test a positive one: a NaN contributes nothing
            bool at = on[u] && d2 > 0.0 && uu <= Wd && fabs(t) <= Wd; // (d2 == 0: the keypoint itself and its exact duplicates)
            if (use_cos) { // (wave-uniform) the support angle; without it the normals are not looked at
                const double c = (ax * nx[u] + ay * ny[u]) + az * nz[u];
                at = at && (sgn ? c : fabs(c)) >= min_cos;
            }
            npos += __popcll(__ballot(at));
            if (at) {
                const double vv = sgn ? t + Wd : t;
                const int iu = (int)uu, iv = (int)vv; // (0 <= uu <= W, 0 <= vv <= NV - 1: the truncation is the floor)
                const unsigned qu = (unsigned)((uu - (double)iu) * 65536.0); // (exact; 0 .. 65535)
                const unsigned qv = (unsigned)((vv - (double)iv) * 65536.0);
                const unsigned long long ru = 65536u - qu, rv = 65536u - qv; // (products of up to 2^32: 64 bits)
                unsigned long long *const node = acc + (iu * NV + iv);
                // a zero weight is not added: uu = W gives qu = 0 and vv = NV - 1 gives qv = 0, so no node outside the image is addressed
                atomicAdd(node, ru * rv);
                if (qu) atomicAdd(node + NV, (unsigned long long)qu * rv);
                if (qv) atomicAdd(node + 1, ru * qv);
                if (qu && qv) atomicAdd(node + NV + 1, (unsigned long long)qu * qv);
            }
        }
    }
    if (k >= SPIN_MAX_LIST) {
        if (lane == 0) *err = 1;
        npos = -1; // (the call fails: the row is not used)
    }
    if (contrib && lane == 0) contrib[row] = npos < 0 ? 0 : npos;
    if (!(npos > min_nb)) { // (min_nb arrives clamped into [-1, 2^31 - 1])
        for (int b = lane; b < D; b += 64) sf_store_stream(o + b, 0.0);
        return;
    }
    SF_SHOT_SYNC(); // (the adds)

    // ---- the row: one correctly rounded integer-to-double conversion per node, then an exact scaling by 2^-32 or (normalize)
    // one correctly rounded division by the exact double c 2^32 ----
    if (mode & SPIN_NORMALIZE) {
        const double den = (double)npos * 4294967296.0;
        for (int b = lane; b < D; b += 64) sf_store_stream(o + b, (double)acc[b] / den);
    } else {
        for (int b = lane; b < D; b += 64) sf_store_stream(o + b, (double)acc[b] * (1.0 / 4294967296.0));
    }
}

// Waves per workgroup for rows of D nodes: as many as keep the workgroup's LDS within 64 KiB (4 up to 2048, 2 above).
int spin_waves(int D) { return D <= 2048 ? 4 : 2; }

int spin_check_width(const char *who, int64_t W)
{
    if (W >= 1 && W <= SF_SPIN_MAX_WIDTH) return SF_OK;
    sf_set_error("%s: image_width = %lld outside [1, %d]", who, (long long)W, SF_SPIN_MAX_WIDTH);
    return SF_ERR_ARG;
}

} // namespace

// The scale of an image, on the host: bins per unit length, PCL's 1 / bin_size of bin_size = R / W / sqrt 2.
extern "C" int sf_spin_scale(double radius, int64_t image_width, double *inv_bin)
{
    SF_CHECK(sf_check_radius("sf_spin_scale", "radius", radius));
    SF_CHECK(spin_check_width("sf_spin_scale", image_width));
    if (!inv_bin) { sf_set_error("sf_spin_scale: null output"); return SF_ERR_ARG; }
    *inv_bin = ((double)image_width * sqrt(2.0)) / radius;
    return SF_OK;
}

extern "C" int sf_spin_images(sf_ctx *ctx, sf_cloud *c, sf_nbrs *nb, const double *axes, int64_t image_width, int signed_beta,
                              int use_min_cos, double min_cos, int normalize, int64_t min_nb, double *out, int32_t *contrib,
                              int flags)
{
    SF_CHECK(check_nbrs(ctx, c, nb, "sf_spin_images"));
    if (!axes || !out) { sf_set_error("sf_spin_images: null %s", axes ? "out" : "axes"); return SF_ERR_ARG; }
    SF_CHECK(spin_check_width("sf_spin_images", image_width));
    if (use_min_cos && !(min_cos >= -1.0 && min_cos <= 1.0)) {
        sf_set_error("sf_spin_images: min_cos must lie in [-1, 1] (got %g)", min_cos);
        return SF_ERR_ARG;
    }
    if (!(c->pop_begin == 0 && c->pop_end == c->n)) { sf_set_error("sf_spin_images: needs the whole cloud's grid, not a block of it"); return SF_ERR_UNSUPPORTED; }
    const int64_t m = nb->m;
    if (!(flags & SF_IN_DEVICE))
        for (int64_t i = 0; i < 3 * m; ++i)
            if (!std::isfinite(axes[i])) { sf_set_error("sf_spin_images: axis %lld is not finite", (long long)(i / 3)); return SF_ERR_ARG; }
    if (use_min_cos) { // (the support angle reads the neighbours' normals; positions alone suffice otherwise)
        if (!c->nrm_orig) { sf_set_error("sf_spin_images: min_cos needs normals, but the cloud has none"); return SF_ERR_STATE; }
        SF_CHECK(sf_cloud_ensure_sorted_normals(ctx, c));
    }
    double inv_bin = 0.0;
    SF_CHECK(sf_spin_scale(nb->radius, image_width, &inv_bin));
    const int W = (int)image_width;
    const int D = (W + 1) * (signed_beta ? 2 * W + 1 : W + 1);
    const int mode = (signed_beta ? SPIN_SIGNED : 0) | (use_min_cos ? SPIN_MIN_COS : 0) | (normalize ? SPIN_NORMALIZE : 0);
    sf_pool_guard guard(ctx);
    const double *daxes;
    double *dout;
    int32_t *dcontrib = nullptr;
    int *derr = nullptr;
    SF_CHECK(stage_in(guard, axes, (size_t)m * 3, flags, &daxes));
    SF_CHECK(guard.alloc(&derr, 1));
    SF_CHECK(stage_out(guard, out, (size_t)m * D, flags, &dout));
    if (contrib) SF_CHECK(stage_out(guard, contrib, (size_t)m, flags, &dcontrib));
    SF_HIP(hipMemsetAsync(derr, 0, sizeof(int), ctx->stream));
    const int nmin = (int)std::min<int64_t>(std::max<int64_t>(min_nb, -1), 2147483647LL);
    if (m) {
        const int wv = spin_waves(D);
        const size_t lds = (size_t)wv * D * sizeof(unsigned long long);
        sf_launch_timer t_(ctx, "k24_spin");
        hipLaunchKernelGGL(k_spin, dim3(sf_xcd_grid(sf_div_up(m, wv))), dim3(64 * wv), lds, ctx->stream, (const double *)c->rec,
                           (const double *)nb->qx, (const double *)nb->qy, (const double *)nb->qz, (const int64_t *)nb->offset,
                           (const int32_t *)nb->count, (const int32_t *)nb->idx, (const int32_t *)nb->qrow, m, daxes, inv_bin, W,
                           mode, use_min_cos ? min_cos : 0.0, nmin, dout, dcontrib, derr);
        SF_HIP(hipGetLastError());
    }
    SF_CHECK(finish_out(ctx, out, (size_t)m * D, flags, dout));
    if (contrib) SF_CHECK(finish_out(ctx, contrib, (size_t)m, flags, dcontrib));
    void *pin = nullptr; // (the error word is read back: the call always waits for its kernel)
    SF_CHECK(sf_ctx_pinned(ctx, &pin));
    SF_HIP(hipMemcpyAsync(pin, derr, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    SF_HIP(hipStreamSynchronize(ctx->stream));
    if (*(const int *)pin) {
        sf_set_error("sf_spin_images: a list of 2^24 entries or more");
        return SF_ERR_ARG;
    }
    return SF_OK;
}
