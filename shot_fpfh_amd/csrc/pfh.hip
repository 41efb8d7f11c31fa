// pfh.hip -- K22: Point Feature Histograms (Rusu, Blodow, Marton, Beetz 2008; pcl::PFHEstimation), the descriptor FPFH is the
// fast approximation of: per keypoint a histogram over S x S x S bins of the three Darboux angles of EVERY unordered pair of the
// entries of its list, k (k - 1) / 2 pairs for a list of k.  Rows of D = S^3 <= SF_PFH_MAX_BINS^3 doubles, the pair with bins
// (b1, b2, b3) of (theta, alpha, phi) at b1 + S b2 + S^2 b3 (PCL's order), row[b] = (100.0 count[b]) / (k (k - 1) / 2).
// The definition -- decided here, modelled on pcl::computePairFeatures -- is tests/pfh_numpy.py: which point of a pair is the
// source is a symmetric rule (so a row is a function of the cloud alone, not of the order of a list), bins by comparisons against
// tables computed once on the host (sf_pfh_tables), never atan2, acos or a division in the kernel; arithmetic unfused float64 in
// the statement's order.  Bin contents are integers: a row is exact whatever the order of the adds, and a call repeats bit for bit.
//
// Mapping: one wave per keypoint, blockDim.x / 64 independent waves per workgroup (pfh_waves), each with its own LDS: a stage of
// PFH_STAGE records (position and normal, 48 B, gathered from `rec` at the list's cell-sorted positions) and D 32-bit counters fed
// by LDS integer atomics.  The list is cut into chunks of 64 entries; a lane holds its entry of the chunk in registers and meets
//   * the other entries of the chunk by the cyclic scheme: entry (lane + j) mod r for j = 1 .. r / 2, the half round (r even,
//     j = r / 2) by the first r / 2 lanes only -- every unordered pair of the chunk once, the same work for every lane;
//   * every entry of every LATER chunk, one entry per round at a wave-uniform LDS address (a broadcast read).
// So a list of k entries takes about k^2 / 128 + k / 4 rounds of 64 pairs, 93 % of them with every lane at work at k = 110.
// A list of at most PFH_STAGE entries is staged once.  A longer one streams: per chunk the chunk itself in the first 64 slots, the
// later entries through the other PFH_STAGE - 64 in tiles -- the list is gathered k / 128 times over, 48 B per 64 pairs of a
// hundred float64 operations each.  Which of the two serves a keypoint is a wave-uniform test of its own list's length; both run
// the same rounds (pfh_rounds), so there is one pair body in the kernel.  The partner's record is three 16-byte LDS reads (a
// 48-byte stride puts the sixteen lanes of a read group on sixteen different four-bank slots: no conflict).
// The edge tables (3 (S + 1) doubles: q | ca | sa) are read at wave-uniform addresses through the scalar cache; with S a
// compile-time constant (SB = 5, the default) the edge loops unroll and the 12 interior values live in scalar registers for the
// whole kernel, SB = 0 is any S with the loads in the loop.
// Float64 issue is the floor: about a hundred vector float64 instructions per pair, nothing else comes close --
// 48 B of LDS per pair, and from HBM per keypoint the list (4 B + 48 B per entry, the records from L2) and the 8 D B row.
#include "common.h"
#include "device_util.h"
#include "host_stage.h"
#include "shot_core.h"

#include <cmath>

namespace {

#define PFH_STAGE 128     // records of a wave's LDS stage
#define PFH_TILE (PFH_STAGE - 64) // records of a tile of the streaming form (the stage without the chunk's 64 slots)
#define PFH_MAX_LIST 65536 // a list this long or longer is refused: k (k - 1) / 2 must stay below 2^32 (the 32-bit counters)

// doubles of LDS per wave: the stage, then D counters rounded up to whole 16 bytes (every wave's stage stays 16-byte aligned)
__host__ __device__ inline int pfh_wave_doubles(int D) { return PFH_STAGE * 6 + ((D + 3) / 4) * 2; }

__device__ inline void pfh_lds_read(const double *stage, int slot, double (&e)[6])
{
    const double2 *p = reinterpret_cast<const double2 *>(stage + 6 * slot);
    const double2 a = p[0], b = p[1], c = p[2];
    e[0] = a.x; e[1] = a.y; e[2] = b.x; e[3] = b.y; e[4] = c.x; e[5] = c.y;
}

// entries [t0, t0 + n) of a list into slots [slot0, slot0 + n) of the stage, n <= PFH_STAGE - slot0 (the caller's tiling)
__device__ inline void pfh_stage_entries(const double *__restrict__ rec, const int32_t *__restrict__ list, int t0, int n, int lane,
                                         double *stage, int slot0)
{
    for (int t = lane; t < n; t += 64) {
        const int j = SF_LIST_LOAD(list + t0 + t);
        const double2 *p = reinterpret_cast<const double2 *>(rec + 6 * (size_t)j);
        const double2 a = p[0], b = p[1], c = p[2];
        double2 *o = reinterpret_cast<double2 *>(stage + 6 * (slot0 + t));
        o[0] = a; o[1] = b; o[2] = c;
    }
}

// The bin of one pair: own entry A = s, partner T = t (x y z nx ny nz).  False: the pair is skipped (d2 == 0 or v2 == 0).
// tab: q[S + 1] | ca[S + 1] | sa[S + 1] (sf_pfh_tables), read at wave-uniform indices.
template <int SB>
__device__ inline bool pfh_pair_bin(const double (&A)[6], const double (&T)[6], sf_const_doubles tab, int S_, int &bin)
{
    const int S = SB ? SB : S_;
    const double dx = T[0] - A[0], dy = T[1] - A[1], dz = T[2] - A[2];
    const double d2 = (dx * dx + dy * dy) + dz * dz;
    const double as = (A[3] * dx + A[4] * dy) + A[5] * dz;
    const double at = -((T[3] * dx + T[4] * dy) + T[5] * dz);
    // the source: the larger |.|, then the larger signed value, then the point that comes first in (x, y, z) order (the sign of a
    // difference of two doubles is exact)
    const double fs = fabs(as), ft = fabs(at);
    const bool t_first = dx < 0.0 || (dx == 0.0 && (dy < 0.0 || (dy == 0.0 && dz < 0.0)));
    const bool tsrc = ft > fs || (ft == fs && (at > as || (at == as && t_first)));
    const double ex = tsrc ? -dx : dx, ey = tsrc ? -dy : dy, ez = tsrc ? -dz : dz;
    const double n1x = tsrc ? T[3] : A[3], n1y = tsrc ? T[4] : A[4], n1z = tsrc ? T[5] : A[5];
    const double n2x = tsrc ? A[3] : T[3], n2y = tsrc ? A[4] : T[4], n2z = tsrc ? A[5] : T[5];
    const double num3 = tsrc ? at : as;
    const double vx = ey * n1z - ez * n1y, vy = ez * n1x - ex * n1z, vz = ex * n1y - ey * n1x; // v = d x n1
    const double v2 = (vx * vx + vy * vy) + vz * vz;
    const double num2 = (vx * n2x + vy * n2y) + vz * n2z;
    const double wx = n1y * vz - n1z * vy, wy = n1z * vx - n1x * vz, wz = n1x * vy - n1y * vx; // w = n1 x v
    const double a = (wx * n2x + wy * n2y) + wz * n2z;
    double B = ((n1x * n2x + n1y * n2y) + n1z * n2z) * sqrt(v2); // (the IEEE root: correctly rounded)
    if (a == 0.0 && B == 0.0) B = 1.0;
    const double z3 = num3 * fabs(num3), z2 = num2 * fabs(num2);
    // theta = atan2(a, B) against the edges e[i]: X_i = sin(theta - e[i]) |(a, B)| >= 0; below the half turn (e[i] < 0) an edge is
    // passed by every theta >= 0 and by X_i, above it by theta >= 0 and X_i together, the edge at 0 (S even) by theta >= 0
    int b3 = 0, b2 = 0, lo = 0, hi = 0;
#pragma unroll
    for (int i = 1; i < S; ++i) {
        const double qi = tab[i];
        b3 += z3 >= qi * d2 ? 1 : 0;
        b2 += z2 >= qi * v2 ? 1 : 0;
        if (2 * i != S) {
            const int x = tab[S + 1 + i] * a - tab[2 * (S + 1) + i] * B >= 0.0 ? 1 : 0;
            if (2 * i < S) lo += x;
            else hi += x;
        }
    }
    const int below = (S - 1) / 2 + ((S & 1) ? 0 : 1); // edges with e[i] <= 0 among 1 .. S - 1
    const int b1 = a >= 0.0 ? below + hi : lo;
    bin = b1 + S * (b2 + S * b3); // (every count stays below S: bin < D)
    return d2 != 0.0 && v2 != 0.0;
}

// The rounds of one chunk against what the stage holds: the chunk's own r entries at slots chunk0 .. (n_intra = r / 2 rounds of
// the cyclic scheme; 0 when they have been run) and n_sweep later entries at slots sweep0 .. .  own: the lane's entry (lane < r).
template <int SB>
__device__ inline void pfh_rounds(const double *stage, unsigned *count, const double (&own)[6], int lane, int r, int chunk0,
                                  int n_intra, int sweep0, int n_sweep, sf_const_doubles tab, int S)
{
    for (int u = 0; u < n_intra + n_sweep; ++u) {
        const bool intra = u < n_intra;
        const int j = u + 1;
        int ps = lane + j; // (lane < r and j <= r / 2: below 2 r)
        ps = ps >= r ? ps - r : ps;
        const bool act = lane < r && !(intra && 2 * j == r && lane >= j); // (the half round: the first r / 2 lanes)
        const int slot = !act ? chunk0 : (intra ? chunk0 + ps : sweep0 + (u - n_intra)); // (an idle lane reads a slot that exists)
        double other[6];
        pfh_lds_read(stage, slot, other);
        int bin;
        const bool ok = pfh_pair_bin<SB>(own, other, tab, S, bin);
        if (act && ok) atomicAdd(&count[bin], 1u);
    }
}

// One wave per keypoint, blockDim.x / 64 waves per workgroup, each with pfh_wave_doubles(D) doubles of the dynamic LDS.
// SB: the bin count at compile time, 0: S_ at run time.  err: set to 1 (a plain store) by a list of PFH_MAX_LIST entries or more.
template <int SB>
__global__ __launch_bounds__(256) void k_pfh(const double *__restrict__ rec, const int64_t *__restrict__ offset,
                                             const int32_t *__restrict__ cnt, const int32_t *__restrict__ idx,
                                             const int32_t *__restrict__ qrow, int64_t m, const double *__restrict__ tab_, int S_,
                                             double *__restrict__ out, int *__restrict__ err)
{
    extern __shared__ __attribute__((aligned(16))) double pfh_lds[];
    const int S = SB ? SB : S_;
    const int D = S * S * S;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nw = blockDim.x >> 6;
    double *const stage = pfh_lds + (size_t)pfh_wave_doubles(D) * wave;
    unsigned *const count = reinterpret_cast<unsigned *>(stage + PFH_STAGE * 6);
    const int64_t q = sf_xcd_block() * nw + wave;
    if (q >= m) return;
    const int32_t *const list = idx + offset[q];
    const int k = sf_uniform(cnt[q]);
    const int64_t row = qrow ? qrow[q] : q;
    double *o = out + (int64_t)D * row;
    if (k < 2 || k >= PFH_MAX_LIST) { // (no pair, or a list that is not walked: the call fails, the row is not used)
        if (k >= PFH_MAX_LIST && lane == 0) *err = 1;
        for (int b = lane; b < D; b += 64) sf_store_stream(o + b, 0.0);
        return;
    }
    const sf_const_doubles tab = (sf_const_doubles)tab_;
    for (int b = lane; b < D; b += 64) count[b] = 0u;
    const bool fits = k <= PFH_STAGE; // (wave-uniform) the whole list in the stage, gathered once
    if (fits) pfh_stage_entries(rec, list, 0, k, lane, stage, 0);
    SF_SHOT_SYNC(); // (the cleared counters, the staged list)

    for (int c0 = 0; c0 < k; c0 += 64) {
        const int r = k - c0 < 64 ? k - c0 : 64;
        const int chunk0 = fits ? c0 : 0;
        if (!fits) {
            SF_SHOT_SYNC(); // (the reads of the chunk before)
            pfh_stage_entries(rec, list, c0, r, lane, stage, 0);
            SF_SHOT_SYNC();
        }
        double own[6];
        pfh_lds_read(stage, chunk0 + (lane < r ? lane : 0), own);
        int n_intra = r >> 1;
        int b0 = c0 + 64; // the first later entry; one pass when the list is staged, else a pass per tile
        do {
            int n_sweep = k - b0 > 0 ? k - b0 : 0;
            int sweep0 = b0;
            if (!fits) {
                n_sweep = n_sweep < PFH_TILE ? n_sweep : PFH_TILE;
                sweep0 = 64;
                SF_SHOT_SYNC(); // (the reads of the tile before)
                pfh_stage_entries(rec, list, b0, n_sweep, lane, stage, 64);
                SF_SHOT_SYNC();
            }
            pfh_rounds<SB>(stage, count, own, lane, r, chunk0, n_intra, sweep0, n_sweep, tab, S);
            n_intra = 0;
            b0 += fits ? PFH_MAX_LIST : PFH_TILE;
        } while (b0 < k);
    }
    SF_SHOT_SYNC(); // (the adds)

    // ---- the row: one exact product and one correctly rounded division per bin; P counts every pair, the skipped ones too ----
    const double P = (double)((unsigned)k * (unsigned)(k - 1) / 2u);
    for (int b = lane; b < D; b += 64) sf_store_stream(o + b, (100.0 * (double)count[b]) / P);
}

// Waves per workgroup for rows of D bins: as many as keep the workgroup's LDS within 64 KiB.
int pfh_waves(int D) { return 4 * 8 * pfh_wave_doubles(D) <= 65536 ? 4 : 2; }

int pfh_check_bins(const char *who, int64_t n_bins)
{
    if (n_bins >= 1 && n_bins <= SF_PFH_MAX_BINS) return SF_OK;
    sf_set_error("%s: n_bins = %lld outside [1, %d]", who, (long long)n_bins, SF_PFH_MAX_BINS);
    return SF_ERR_ARG;
}

} // namespace

// The tables of a bin count, on the host, S + 1 entries each (a kernel reads the interior ones, 1 .. S - 1):
// q = c |c| of c[i] = -1 + 2 i / S; ca, sa = cos, sin of e[i] = -pi + 2 pi i / S; g = the sign of e[i].
extern "C" int sf_pfh_tables(int64_t n_bins, double *q, double *ca, double *sa, int32_t *g)
{
    SF_CHECK(pfh_check_bins("sf_pfh_tables", n_bins));
    if (!q || !ca || !sa || !g) { sf_set_error("sf_pfh_tables: null output"); return SF_ERR_ARG; }
    const int S = (int)n_bins;
    const double pi = 3.141592653589793;
    for (int i = 0; i <= S; ++i) {
        double c = -1.0 + 2.0 * (double)i / (double)S;
        if (i == 0) c = -1.0;
        if (i == S) c = 1.0;
        if (2 * i == S) c = 0.0;
        q[i] = c * fabs(c);
        g[i] = (2 * i > S) - (2 * i < S);
        // every function value through the extended-precision libm, rounded once
        const double e = -pi + 2.0 * pi * (double)i / (double)S;
        ca[i] = g[i] ? (double)cosl(e) : 1.0;
        sa[i] = g[i] ? (double)sinl(e) : 0.0;
    }
    return SF_OK;
}

extern "C" int sf_pfh(sf_ctx *ctx, sf_cloud *c, sf_nbrs *nb, int64_t n_bins, double *out, int flags)
{
    SF_CHECK(check_nbrs(ctx, c, nb, "sf_pfh"));
    if (!out) { sf_set_error("sf_pfh: null out"); return SF_ERR_ARG; }
    SF_CHECK(pfh_check_bins("sf_pfh", n_bins));
    if (!(c->pop_begin == 0 && c->pop_end == c->n)) { sf_set_error("sf_pfh: needs the whole cloud's grid, not a block of it"); return SF_ERR_UNSUPPORTED; }
    SF_CHECK(sf_cloud_ensure_sorted_normals(ctx, c)); // (SF_ERR_STATE for a cloud without normals)
    const int S = (int)n_bins, D = S * S * S;
    const int64_t m = nb->m;
    std::vector<double> htab((size_t)3 * (S + 1));
    std::vector<int32_t> sign((size_t)S + 1);
    SF_CHECK(sf_pfh_tables(n_bins, &htab[0], &htab[S + 1], &htab[2 * (S + 1)], sign.data()));
    sf_pool_guard guard(ctx);
    double *dtab = nullptr, *dout;
    int *derr = nullptr;
    SF_CHECK(guard.alloc(&dtab, htab.size()));
    SF_CHECK(guard.alloc(&derr, 1));
    SF_CHECK(stage_out(guard, out, (size_t)m * D, flags, &dout));
    SF_HIP(hipMemsetAsync(derr, 0, sizeof(int), ctx->stream));
    SF_HIP(hipMemcpyAsync(dtab, htab.data(), htab.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (m) {
        const int wv = pfh_waves(D);
        const size_t lds = (size_t)wv * pfh_wave_doubles(D) * sizeof(double);
        const dim3 grid(sf_xcd_grid(sf_div_up(m, wv))), block(64 * wv);
        sf_launch_timer t_(ctx, "k22_pfh");
#define PFH_LAUNCH(SB)                                                                                                          \
    hipLaunchKernelGGL(k_pfh<SB>, grid, block, lds, ctx->stream, (const double *)c->rec, (const int64_t *)nb->offset,           \
                       (const int32_t *)nb->count, (const int32_t *)nb->idx, (const int32_t *)nb->qrow, m, (const double *)dtab, \
                       S, dout, derr)
        if (S == 5) PFH_LAUNCH(5);
        else PFH_LAUNCH(0);
#undef PFH_LAUNCH
        SF_HIP(hipGetLastError());
    }
    SF_CHECK(finish_out(ctx, out, (size_t)m * D, flags, dout));
    void *pin = nullptr; // (the table upload reads htab until the stream has passed it: the call always waits)
    SF_CHECK(sf_ctx_pinned(ctx, &pin));
    SF_HIP(hipMemcpyAsync(pin, derr, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    SF_HIP(hipStreamSynchronize(ctx->stream));
    if (*(const int *)pin) {
        sf_set_error("sf_pfh: a list of %d entries or more (its pairs would not fit the 32-bit counters)", PFH_MAX_LIST);
        return SF_ERR_ARG;
    }
    return SF_OK;
}
