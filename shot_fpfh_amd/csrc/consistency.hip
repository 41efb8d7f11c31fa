// consistency.hip -- K13: the geometric-consistency filter of a set of matches.
//
// No counterpart in the reference.  A rigid motion keeps lengths, so two matches i and j can both be true only if the scan side's
// |a_i - a_j| equals the reference side's |b_i - b_j| within the noise.  With, in unfused float64 and exactly this order,
//   dp(i,j) = sqrt(((ax_i - ax_j)^2 + (ay_i - ay_j)^2) + (az_i - az_j)^2),   dq(i,j) the same on b,
//   compat(i,j) = i != j  and  |dp - dq| <= distance_threshold  and  min(dp, dq) >= min_edge        (a NaN compares false),
//   degree[i] = #{ j : member[j] and compat(i,j) }                                                  (no mask: every column),
// the group is: deg over all columns; seed = the LOWEST index among the maxima of deg; member = compat(seed, .) with the seed
// itself; g = sum member; gdeg = degree over the member columns -- the definition of tests/consistency_numpy.py.  Every output is
// an integer decided in float64, so the device agrees with the statement exactly, whatever the order the pairs are visited in.
//
// k13_degree is the m^2 part: a thread owns a row (6 coordinates in registers), the columns go through LDS a tile at a time and
// every lane of a wave reads the SAME column (a broadcast read), so the inner loop is 16 float64 operations, two square roots and
// three compares per pair and nothing else.  The grid is 2-D, row blocks x column slices, so that a few thousand matches already
// fill the chip; a slice adds its count into the row's uint32 with one integer atomic, which is exact in any order.  A column
// outside the mask is staged as NaN: it is compatible with nothing, and the inner loop carries no mask test.
// The chain of sf_consistency_group (degree, arg-max, mark, count, masked degree) is queued on the stream; the host waits once.
#include "common.h"
#include "device_util.h"
#include "horn4.h"
#include "ransac.h" // the back half of K11, which with K9 (sf_ransac_score, match.hip) ranks K15's fits

namespace {

constexpr int K13_BLOCK = 256;          // rows of a block, one per thread
constexpr int K13_TILE = 128;           // columns staged through LDS at a time: 16 row blocks x 32 tiles at m = 4096, 2 blocks per CU
constexpr int K13_TARGET_BLOCKS = 4096; // column slices are cut until the grid has about this many blocks (16 per CU)
constexpr int K13_FOLD = 1024;          // threads of the single-block kernels

// the device info block (int64)
enum { IN_SEED = 0, IN_SEED_DEGREE = 1, IN_GROUP = 2, IN_STATUS = 3, IN_SIZE = 4 };

// (min(dp, dq) >= min_edge as two compares: the same decision, and false for a NaN like every comparison of the definition)
__device__ __forceinline__ bool k13_compat(double ax, double ay, double az, double bx, double by, double bz, double cax, double cay,
                                           double caz, double cbx, double cby, double cbz, double thr, double min_edge)
{
    const double ux = ax - cax, uy = ay - cay, uz = az - caz;
    const double vx = bx - cbx, vy = by - cby, vz = bz - cbz;
    const double dp = sqrt((ux * ux + uy * uy) + uz * uz);
    const double dq = sqrt((vx * vx + vy * vy) + vz * vz);
    return fabs(dp - dq) <= thr && dp >= min_edge && dq >= min_edge;
}

// grid: (row blocks, column slices).  Slice y counts columns [y, y + 1) * tiles_per_slice * K13_TILE of the rows of block x.
__global__ __launch_bounds__(K13_BLOCK) void k13_degree(const double *__restrict__ a, const double *__restrict__ b, int64_t m,
                                                        const unsigned char *__restrict__ member, double thr, double min_edge,
                                                        int tiles_per_slice, unsigned *__restrict__ degree)
{
    __shared__ __attribute__((aligned(16))) double col[K13_TILE * 6]; // per column: ax ay az bx by bz
    const double nan = __builtin_nan("");
    const int64_t i = (int64_t)blockIdx.x * K13_BLOCK + threadIdx.x;
    double ax = nan, ay = nan, az = nan, bx = nan, by = nan, bz = nan; // (a thread past the last row counts nothing)
    if (i < m) {
        ax = a[3 * i]; ay = a[3 * i + 1]; az = a[3 * i + 2];
        bx = b[3 * i]; by = b[3 * i + 1]; bz = b[3 * i + 2];
    }
    const int64_t tile0 = (int64_t)blockIdx.y * tiles_per_slice;
    unsigned count = 0;
    for (int t = 0; t < tiles_per_slice; ++t) {
        const int64_t j0 = (tile0 + t) * K13_TILE;
        if (j0 >= m) break; // (the same for the whole block)
        __syncthreads();    // the previous tile has been read by every wave
        for (int e = threadIdx.x; e < 6 * K13_TILE; e += K13_BLOCK) { // 3 K13_TILE doubles of a, then of b: coalesced
            const int side = e >= 3 * K13_TILE ? 1 : 0;
            const int r = e - side * 3 * K13_TILE, c = r / 3;
            const int64_t j = j0 + c;
            double v = nan;
            if (j < m && (!member || member[j])) v = (side ? b : a)[3 * j0 + r];
            col[6 * c + 3 * side + (r - 3 * c)] = v;
        }
        __syncthreads();
        const int lim = (int)(m - j0 < K13_TILE ? m - j0 : K13_TILE);
#pragma unroll 4
        for (int c = 0; c < lim; ++c) {
            const double *q = col + 6 * c; // one address for the whole wave: a broadcast read
            const bool ok = k13_compat(ax, ay, az, bx, by, bz, q[0], q[1], q[2], q[3], q[4], q[5], thr, min_edge);
            count += (ok && j0 + c != i) ? 1u : 0u;
        }
    }
    if (i < m && count) atomicAdd(&degree[i], count);
}

// One block: the first maximum of degree[0 .. m), as the 64-bit maximum of degree << 32 | ~index.
__global__ __launch_bounds__(K13_FOLD) void k13_argmax(const unsigned *__restrict__ degree, int64_t m, int64_t *__restrict__ info)
{
    __shared__ unsigned long long sh[K13_FOLD / SF_WAVE];
    unsigned long long best = 0; // (degree 0 at index 2^32 - 1: below every real entry, m <= 2^31 - 1)
    for (int64_t j = threadIdx.x; j < m; j += K13_FOLD) {
        const unsigned long long key = ((unsigned long long)degree[j] << 32) | (unsigned)~(unsigned)j;
        best = key > best ? key : best;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long y = __shfl_xor(best, off);
        best = y > best ? y : best;
    }
    if ((threadIdx.x & (SF_WAVE - 1)) == 0) sh[threadIdx.x / SF_WAVE] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < K13_FOLD / SF_WAVE; ++w) best = sh[w] > best ? sh[w] : best;
        info[IN_SEED] = (int64_t)(unsigned)~(unsigned)(best & 0xffffffffull);
        info[IN_SEED_DEGREE] = (int64_t)(best >> 32);
    }
}

// member[j] = compat(seed, j), and the seed itself; all zeros when no pair is compatible.  The seed is read from device memory.
__global__ __launch_bounds__(K13_BLOCK) void k13_mark(const double *__restrict__ a, const double *__restrict__ b, int64_t m, double thr,
                                                      double min_edge, const int64_t *__restrict__ info,
                                                      unsigned char *__restrict__ member)
{
    const int64_t j = (int64_t)blockIdx.x * K13_BLOCK + threadIdx.x;
    if (j >= m) return;
    const int64_t seed = info[IN_SEED];
    if (info[IN_SEED_DEGREE] == 0) { member[j] = 0; return; }
    const bool ok = k13_compat(a[3 * seed], a[3 * seed + 1], a[3 * seed + 2], b[3 * seed], b[3 * seed + 1], b[3 * seed + 2], a[3 * j],
                               a[3 * j + 1], a[3 * j + 2], b[3 * j], b[3 * j + 1], b[3 * j + 2], thr, min_edge);
    member[j] = (ok || j == seed) ? 1 : 0;
}

// One block: g = the number of members; the status (1: no compatible pair).
__global__ __launch_bounds__(K13_FOLD) void k13_count(const unsigned char *__restrict__ member, int64_t m, int64_t *__restrict__ info)
{
    __shared__ unsigned long long sh[K13_FOLD / SF_WAVE];
    unsigned long long n = 0;
    for (int64_t j = threadIdx.x; j < m; j += K13_FOLD) n += member[j] ? 1 : 0;
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off);
    if ((threadIdx.x & (SF_WAVE - 1)) == 0) sh[threadIdx.x / SF_WAVE] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < K13_FOLD / SF_WAVE; ++w) n += sh[w];
        info[IN_GROUP] = (int64_t)n;
        info[IN_STATUS] = info[IN_SEED_DEGREE] == 0 ? 1 : 0;
    }
}

int k13_check(const char *who, bool pointers, int64_t m, double thr, double min_edge)
{
    if (!pointers || m < 0) { sf_set_error("%s: bad argument", who); return SF_ERR_ARG; }
    if (m > 0x7fffffffll) { sf_set_error("%s: %lld matches, at most 2^31 - 1", who, (long long)m); return SF_ERR_ARG; }
    if (!(thr >= 0.0 && thr <= SF_DBL_MAX) || !(min_edge >= 0.0 && min_edge <= SF_DBL_MAX)) {
        sf_set_error("%s: distance_threshold %g and min_edge %g must be finite and not negative", who, thr, min_edge);
        return SF_ERR_ARG;
    }
    return SF_OK;
}

// degree_dev <- 0, then one launch: the slices add into it.
int k13_launch_degree(sf_ctx *ctx, const double *a, const double *b, int64_t m, const unsigned char *member, double thr,
                      double min_edge, unsigned *degree_dev)
{
    const int64_t row_blocks = sf_div_up(m, K13_BLOCK), tiles = sf_div_up(m, K13_TILE);
    const int64_t want = std::min<int64_t>(tiles, std::max<int64_t>(1, sf_div_up(K13_TARGET_BLOCKS, row_blocks)));
    const int tiles_per_slice = (int)sf_div_up(tiles, want);
    const int64_t slices = sf_div_up(tiles, tiles_per_slice); // <= K13_TARGET_BLOCKS
    SF_HIP(hipMemsetAsync(degree_dev, 0, (size_t)m * sizeof(unsigned), ctx->stream));
    SF_LAUNCH(ctx, "k13_degree", k13_degree, dim3((unsigned)row_blocks, (unsigned)slices), dim3(K13_BLOCK), a, b, m, member, thr,
              min_edge, tiles_per_slice, degree_dev);
    return SF_OK;
}


// ---- K14: second-order consistency (SC2, Chen et al. 2022) on the int8 matrix cores ----------------------------------------------
// C[i][j] = compat(i, j) as a byte matrix, m_pad x m_pad with m_pad = m rounded up to K14_T and the padding zero;
//   s2[i] = sum_j C[i][j] N[i][j],   N[i][j] = sum_k C[i][k] C[j][k]   (N = C C^T: both operands are ROWS of one matrix),
// twice the triangles through i in the compatibility graph -- the definition of tests/sc2_numpy.py.  Integers throughout.
//
// k14_matrix is k13_degree's loop with a store in place of the count: compat is symmetric bit for bit (the squares of negated
// differences are equal), so the thread that owns row i writes [c][i] and a wave's store is 64 consecutive bytes.
//
// k14_sc2 is the m^3 part, a K-loop GEMM on v_mfma_i32_32x32x32_i8.  A workgroup of 8 waves owns 256 x 256 outputs, a wave 64 x 128
// (2 x 4 accumulators of 32 x 32: 128 registers).  Per step the 64-byte K-chunk of the tile's 256 + 256 rows (32 KB) goes from
// global memory into one of two LDS buffers by LDS-DMA, four 1 KB instructions a wave.  The LDS image is lane-linear, row-major
// with 64-byte rows; slot p of row r holds the 16-byte chunk p ^ ((r >> 2) & 3) -- the permutation is applied to the SOURCE
// address of the DMA and to the fragment read alike -- so the 16 lanes of a fragment read (16 consecutive rows, one chunk) touch
// 16 different 16-byte bank groups: rows r and r + 4 would share theirs otherwise.  Operand layout as k_i8_min (match_i8.hip):
// lane (r31, h) holds bytes [16 h, 16 h + 16) of row r31 of the 32-deep step; accumulator register r is row (r & 3) + 8 (r >> 2) +
// 4 h, column r31.  Epilogue: acc x C[row][col], summed over the wave's four column blocks in registers and over the 32 lanes of
// a half by DPP, one integer atomicAdd per row and wave into s2 (zeroed in front).  Every s2 is below 2^30 at the cap.
// Only the tiles J >= I are computed: N is symmetric for ANY C, so tile (I, J) with J > I also adds, per column j, the sum over
// its rows of C[j][i] N[i][j] -- what tile (J, I) would have added to s2[j] -- from the same accumulators.
typedef int k14_i4 __attribute__((ext_vector_type(4)));
typedef int k14_i16 __attribute__((ext_vector_type(16)));
constexpr int K14_T = SF_SC2_TILE;          // outputs of a workgroup along either axis; m_pad is a multiple of it
constexpr int K14_KC = 64;                  // bytes of K per step and row
constexpr int K14_BUF = 2 * K14_T * K14_KC; // one LDS buffer: the row tile's 256 rows, then the column tile's
static_assert(K14_T == 256 && K14_T % K13_TILE == 0 && K14_T == K13_BLOCK, "the tile shapes below are written out for 256");

// grid: (m_pad / K13_BLOCK row blocks, column slices); every byte of the m_pad x m_pad matrix is written, the padding as zero
// (a row or column past m is NaN and compatible with nothing).
__global__ __launch_bounds__(K13_BLOCK) void k14_matrix(const double *__restrict__ a, const double *__restrict__ b, int64_t m,
                                                        int64_t m_pad, double thr, double min_edge, int tiles_per_slice,
                                                        unsigned char *__restrict__ cmat)
{
    __shared__ __attribute__((aligned(16))) double col[K13_TILE * 6];
    const double nan = __builtin_nan("");
    const int64_t i = (int64_t)blockIdx.x * K13_BLOCK + threadIdx.x; // < m_pad
    double ax = nan, ay = nan, az = nan, bx = nan, by = nan, bz = nan;
    if (i < m) {
        ax = a[3 * i]; ay = a[3 * i + 1]; az = a[3 * i + 2];
        bx = b[3 * i]; by = b[3 * i + 1]; bz = b[3 * i + 2];
    }
    const int64_t tile0 = (int64_t)blockIdx.y * tiles_per_slice;
    for (int t = 0; t < tiles_per_slice; ++t) {
        const int64_t j0 = (tile0 + t) * K13_TILE;
        if (j0 >= m_pad) break; // (the same for the whole block)
        __syncthreads();
        for (int e = threadIdx.x; e < 6 * K13_TILE; e += K13_BLOCK) {
            const int side = e >= 3 * K13_TILE ? 1 : 0;
            const int r = e - side * 3 * K13_TILE, c = r / 3;
            double v = nan;
            if (j0 + c < m) v = (side ? b : a)[3 * j0 + r];
            col[6 * c + 3 * side + (r - 3 * c)] = v;
        }
        __syncthreads();
#pragma unroll 4
        for (int c = 0; c < K13_TILE; ++c) { // (whole tiles: m_pad is a multiple of K13_TILE)
            const double *q = col + 6 * c;
            const bool ok = k13_compat(ax, ay, az, bx, by, bz, q[0], q[1], q[2], q[3], q[4], q[5], thr, min_edge);
            cmat[(j0 + c) * m_pad + i] = (ok && j0 + c != i) ? 1 : 0;
        }
    }
}

#define K14_DMA16(GPTR, LDS_DST)                                                                                    \
    {                                                                                                               \
        unsigned keep_;                                                                                             \
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\t"       \
                     "s_mov_b32 m0, %0"                                                                             \
                     : "=&s"(keep_)                                                                                 \
                     : "v"(GPTR), "s"(LDS_DST)                                                                      \
                     : "memory");                                                                                   \
    }
// the K-chunk [K0, K0 + K14_KC) of the 512 rows into buffer BUF: instruction u of wave w fills rows 16 (w + 8 u) .. + 15
#define K14_DMA(K0, BUF)                                                                                            \
    {                                                                                                               \
        const unsigned dst_ = lds_base + (unsigned)(BUF) * K14_BUF + 1024u * wave_u;                                \
        _Pragma("unroll") for (int u = 0; u < 4; ++u) K14_DMA16(src[u] + (K0), dst_ + 8192u * u)                    \
    }
#define K14_FRAG(ROW0, KS) (*reinterpret_cast<const k14_i4 *>(bp + (ROW0) * K14_KC + roff[KS]))

// grid: (row tiles, column tiles) of K14_T.  cmat: m_pad x m_pad bytes of 0 / 1 with zero padding; s2 (m uint32) is added to.
__global__ __launch_bounds__(512, 1) void k14_sc2(const unsigned char *__restrict__ cmat, int64_t m, int64_t m_pad,
                                                   unsigned *__restrict__ s2)
{
    __shared__ __attribute__((aligned(16))) unsigned char Ls[2 * K14_BUF];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r31 = lane & 31, h = lane >> 5;
    const int wr = wave >> 1, wc = wave & 1; // the wave's 64 rows x 128 columns of the tile
    if (blockIdx.y < blockIdx.x) return; // N = C C^T is symmetric whatever C is: tile (J, I) is served by tile (I, J)'s columns
    const bool mirror = blockIdx.y > blockIdx.x;
    const int64_t row_tile = (int64_t)blockIdx.x * K14_T, col_tile = (int64_t)blockIdx.y * K14_T;
    const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char *)Ls;
    const unsigned wave_u = (unsigned)__builtin_amdgcn_readfirstlane(wave);
    const unsigned char *src[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int P = 64 * (wave + 8 * u) + lane, row = P >> 2, c = (P & 3) ^ ((row >> 2) & 3);
        const int64_t grow = row < K14_T ? row_tile + row : col_tile + (row - K14_T);
        src[u] = cmat + grow * m_pad + 16 * c;
    }
    unsigned roff[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) roff[ks] = (unsigned)(r31 * K14_KC + (((2 * ks + h) ^ ((r31 >> 2) & 3)) * 16));
    k14_i16 acc[2][4];
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int bj = 0; bj < 4; ++bj)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[bi][bj][r] = 0;
    const int64_t nk = m_pad / K14_KC;
    K14_DMA(0, 0)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int64_t kc = 0; kc < nk; ++kc) {
        const int buf = (int)(kc & 1);
        if (kc + 1 < nk) K14_DMA((kc + 1) * K14_KC, buf ^ 1)
        const unsigned char *bp = Ls + buf * K14_BUF;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            k14_i4 fa[2], fb[4];
#pragma unroll
            for (int bi = 0; bi < 2; ++bi) fa[bi] = K14_FRAG(64 * wr + 32 * bi, ks);
#pragma unroll
            for (int bj = 0; bj < 4; ++bj) fb[bj] = K14_FRAG(K14_T + 128 * wc + 32 * bj, ks);
#pragma unroll
            for (int bi = 0; bi < 2; ++bi)
#pragma unroll
                for (int bj = 0; bj < 4; ++bj)
                    acc[bi][bj] = __builtin_amdgcn_mfma_i32_32x32x32_i8(fa[bi], fb[bj], acc[bi][bj], 0, 0, 0);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // this wave's DMA pieces of the next chunk have landed
        __syncthreads();
    }
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t row = row_tile + 64 * wr + 32 * bi + (r & 3) + 8 * (r >> 2) + 4 * h;
            const unsigned char *crow = cmat + row * m_pad + col_tile + 128 * wc + r31;
            int v = 0;
#pragma unroll
            for (int bj = 0; bj < 4; ++bj) v += acc[bi][bj][r] * (int)crow[32 * bj];
            v = sf_row16_sum(v);
            v += __shfl_xor(v, 16); // the two DPP rows of this 32-lane half
            if (r31 == 0 && row < m && v) atomicAdd(&s2[row], (unsigned)v);
        }
    if (!mirror) return; // (the same for the whole block)
    // the mirrored tile: s2[col] += sum_row C[col][row] N[row][col].  A lane owns a column; its rows of one accumulator are four
    // runs of four consecutive bytes of C's row `col`.  Summed over registers, then over the two lane halves.
#pragma unroll
    for (int bj = 0; bj < 4; ++bj) {
        const int64_t col = col_tile + 128 * wc + 32 * bj + r31;
        const unsigned char *ccol = cmat + col * m_pad + row_tile + 64 * wr + 4 * h;
        int v = 0;
#pragma unroll
        for (int bi = 0; bi < 2; ++bi)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const unsigned w = *reinterpret_cast<const unsigned *>(ccol + 32 * bi + 8 * q); // rows 8 q + 4 h + (0 .. 3)
#pragma unroll
                for (int e = 0; e < 4; ++e) v += acc[bi][bj][4 * q + e] * (int)((w >> (8 * e)) & 0xffu);
            }
        v += __shfl_xor(v, 32);
        if (h == 0 && col < m && v) atomicAdd(&s2[col], (unsigned)v);
    }
}
#undef K14_DMA
#undef K14_FRAG

int k14_check_count(const char *who, bool pointers, int64_t m)
{
    if (!pointers || m < 0) { sf_set_error("%s: bad argument", who); return SF_ERR_ARG; }
    if (m > SF_SC2_MAX_MATCHES) {
        sf_set_error("%s: %lld matches, at most %d (the byte matrix is m^2)", who, (long long)m, SF_SC2_MAX_MATCHES);
        return SF_ERR_ARG;
    }
    return SF_OK;
}

int64_t k14_pad(int64_t m) { return sf_div_up(m, K14_T) * K14_T; }

int k14_launch_matrix(sf_ctx *ctx, const double *a, const double *b, int64_t m, double thr, double min_edge, unsigned char *cmat)
{
    const int64_t m_pad = k14_pad(m), row_blocks = m_pad / K13_BLOCK, tiles = m_pad / K13_TILE;
    const int64_t want = std::min<int64_t>(tiles, std::max<int64_t>(1, sf_div_up(K13_TARGET_BLOCKS, row_blocks)));
    const int tiles_per_slice = (int)sf_div_up(tiles, want);
    const int64_t slices = sf_div_up(tiles, tiles_per_slice);
    SF_LAUNCH(ctx, "k14_matrix", k14_matrix, dim3((unsigned)row_blocks, (unsigned)slices), dim3(K13_BLOCK), a, b, m, m_pad, thr, min_edge,
              tiles_per_slice, cmat);
    return SF_OK;
}

// s2_dev <- 0, then one launch: the tiles add into it.
int k14_launch_sc2(sf_ctx *ctx, const unsigned char *cmat, int64_t m, unsigned *s2_dev)
{
    const int64_t m_pad = k14_pad(m), tiles = m_pad / K14_T; // <= 128
    SF_HIP(hipMemsetAsync(s2_dev, 0, (size_t)m * sizeof(unsigned), ctx->stream));
    SF_LAUNCH(ctx, "k14_sc2", k14_sc2, dim3((unsigned)tiles, (unsigned)tiles), dim3(512), cmat, m, m_pad, s2_dev);
    return SF_OK;
}


// ---- K15: SC2 registration -- one Kabsch fit per second-order seed, ranked by inliers over all matches ----------------------------
// The other half of SC2-PCR on the matrix K14 builds (the definition: tests/sc2_registration_numpy.py):
//   seeds   the n_seeds matches of the largest s2 > 0, s2 descending, position ascending (k15_seeds: an exact rank count, every
//           thread writes the one slot its rank names -- no atomic decides a position);
//   rows    row_s[j] = C[seed_s][j] sum_k C[seed_s][k] C[j][k] (k15_seed_rows: the thin integer GEMM below);
//   fits    consensus of a seed = the filter's rule on its row, Kabsch over the members (k15_fit, one workgroup a seed);
//   ranking K11's compaction, K9 and K11's first maximum (ransac.hip, match.hip), as they are.
//
// k15_seed_rows is k14_sc2 with a gathered, short row operand and a store in place of the sum.  A workgroup of 8 waves owns
// K15_TS = 64 seeds x 256 columns; wave w owns the 64 x 32 block of columns 32 w .. 32 w + 31 (2 accumulators).  Per step the
// 64-byte K-chunk of the 64 seed rows (source row = cmat row of the seed: the gather is in the DMA's source address and nowhere
// else) and of the tile's 256 column rows goes into one of two 20 KB LDS buffers by LDS-DMA, 20 instructions of 1 KB: waves
// 0 .. 3 issue three, the others two.  LDS image, bank permutation and operand layout are k14_sc2's.  N has no symmetry to use
// here (the row operand is a subset), and the grid is (seed tiles, column tiles) with the seed tile the fast axis: the seed
// tiles of one column tile are resident together and stream the same 256 rows of C.  A seed of -1 (or outside [0, m)) reads
// row 0 and multiplies by 0.
constexpr int K15_TS = SF_SC2_SEED_TILE;     // seeds of a workgroup
constexpr int K15_ROWS = K15_TS + K14_T;     // LDS rows of a buffer: the seed rows, then the column tile's
constexpr int K15_BUF = K15_ROWS * K14_KC;   // 20 KB
constexpr int K15_SEL = 1024;                // keys staged at a time by k15_seeds
constexpr int K15_FIT = 256;                 // threads of k15_fit
static_assert(K15_TS == 64 && K15_ROWS % 16 == 0 && K15_ROWS / 16 <= 24, "the DMA split below is written out for 64 + 256 rows");

// grid: blocks of 256 matches.  rank(i) = #{ j : (s2[j], -j) > (s2[i], -i) } as one 64-bit compare; seeds_dev was filled with -1.
__global__ __launch_bounds__(256) void k15_seeds(const unsigned *__restrict__ s2, int64_t m, int n_seeds, int *__restrict__ seeds)
{
    __shared__ unsigned long long keys[K15_SEL];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const unsigned long long mine = i < m ? (((unsigned long long)s2[i] << 32) | (unsigned)~(unsigned)i) : ~0ull;
    unsigned rank = 0;
    for (int64_t j0 = 0; j0 < m; j0 += K15_SEL) {
        __syncthreads();
        for (int e = threadIdx.x; e < K15_SEL; e += 256) {
            const int64_t j = j0 + e;
            keys[e] = j < m ? (((unsigned long long)s2[j] << 32) | (unsigned)~(unsigned)j) : 0ull; // (0: above nobody)
        }
        __syncthreads();
#pragma unroll 8
        for (int c = 0; c < K15_SEL; ++c) rank += keys[c] > mine ? 1u : 0u; // one address for the whole wave: a broadcast read
    }
    if (i < m && (mine >> 32) != 0 && rank < (unsigned)n_seeds) seeds[rank] = (int)i;
}

#define K15_FRAG(ROW0, KS) (*reinterpret_cast<const k14_i4 *>(bp + (ROW0) * K14_KC + roff[KS]))
// the K-chunk [K0, K0 + K14_KC) of the 320 rows into buffer BUF: instruction u of wave w fills rows 16 (w + 8 u) .. + 15
#define K15_DMA(K0, BUF)                                                                                            \
    {                                                                                                               \
        const unsigned dst_ = lds_base + (unsigned)(BUF) * K15_BUF + 1024u * wave_u;                                \
        K14_DMA16(src[0] + (K0), dst_)                                                                              \
        K14_DMA16(src[1] + (K0), dst_ + 8192u)                                                                      \
        if (wave_u < 4) K14_DMA16(src[2] + (K0), dst_ + 16384u)                                                     \
    }

// grid: (seed tiles of K15_TS, column tiles of K14_T).  rows: n_seeds x m_pad uint32, every entry of rows s < n_seeds written.
__global__ __launch_bounds__(512) void k15_seed_rows(const unsigned char *__restrict__ cmat, int64_t m, int64_t m_pad,
                                                     const int *__restrict__ seeds, int n_seeds, unsigned *__restrict__ rows)
{
    __shared__ __attribute__((aligned(16))) unsigned char Ls[2 * K15_BUF];
    __shared__ int seed_sh[K15_TS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r31 = lane & 31, h = lane >> 5;
    const int s0 = (int)blockIdx.x * K15_TS;
    const int64_t col_tile = (int64_t)blockIdx.y * K14_T;
    if (tid < K15_TS) {
        const int sd = s0 + tid < n_seeds ? seeds[s0 + tid] : -1;
        seed_sh[tid] = (sd >= 0 && sd < m) ? sd : -1;
    }
    __syncthreads();
    const unsigned lds_base = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char *)Ls;
    const unsigned wave_u = (unsigned)__builtin_amdgcn_readfirstlane(wave);
    const unsigned char *src[3];
#pragma unroll
    for (int u = 0; u < 3; ++u) {
        const int P = 64 * (wave + 8 * u) + lane, c = (P & 3) ^ ((P >> 4) & 3);
        const int row = (P >> 2) < K15_ROWS ? (P >> 2) : 0; // (waves 4 .. 7 have no third piece: never issued)
        int64_t grow;
        if (row < K15_TS) {
            const int sd = seed_sh[row];
            grow = sd >= 0 ? sd : 0;
        } else {
            grow = col_tile + (row - K15_TS);
        }
        src[u] = cmat + grow * m_pad + 16 * c;
    }
    unsigned roff[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) roff[ks] = (unsigned)(r31 * K14_KC + (((2 * ks + h) ^ ((r31 >> 2) & 3)) * 16));
    k14_i16 acc[2];
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[bi][r] = 0;
    const int64_t nk = m_pad / K14_KC;
    K15_DMA(0, 0)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int64_t kc = 0; kc < nk; ++kc) {
        const int buf = (int)(kc & 1);
        if (kc + 1 < nk) K15_DMA((kc + 1) * K14_KC, buf ^ 1)
        const unsigned char *bp = Ls + buf * K15_BUF;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const k14_i4 fb = K15_FRAG(K15_TS + 32 * wave, ks);
#pragma unroll
            for (int bi = 0; bi < 2; ++bi)
                acc[bi] = __builtin_amdgcn_mfma_i32_32x32x32_i8(K15_FRAG(32 * bi, ks), fb, acc[bi], 0, 0, 0);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // this wave's DMA pieces of the next chunk have landed
        __syncthreads();
    }
    const int64_t col = col_tile + 32 * wave + r31; // < m_pad
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rl = 32 * bi + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (s0 + rl >= n_seeds) continue;
            const int sd = seed_sh[rl];
            const unsigned cv = sd >= 0 ? (unsigned)cmat[(int64_t)sd * m_pad + col] : 0u;
            rows[(int64_t)(s0 + rl) * m_pad + col] = (unsigned)acc[bi][r] * cv; // 32 lanes: 128 consecutive bytes
        }
}
#undef K15_DMA
#undef K15_FRAG
#undef K14_DMA16

// NV sums over the block, the same total in every thread (sf_block_sum4, device_util.h)
template <int NV>
__device__ __forceinline__ void k15_block_sums(double (&v)[NV], double (&sh)[4][9])
{
    __syncthreads(); // (the previous use of sh has been read)
    sf_block_sum4_stage(v, sh);
#pragma unroll
    for (int q = 0; q < NV; ++q) v[q] = sf_block_sum4_at(sh, q);
}

// grid: one block a seed.  status: 0 a transform, 1 fewer than three members, 2 no unique rotation (sf_horn::rigid_from_moments,
// horn4.h: sf_horn::kabsch_rotation and the one rule K11's draws are held to), 3 no seed in this slot.
// sums (nullable): sf_ransac_refit_sums's layout (ransac.h), RS_SSR = 0.  member (nullable): n_seeds x m bytes.
__global__ __launch_bounds__(K15_FIT) void k15_fit(const double *__restrict__ a, const double *__restrict__ b, int64_t m, int64_t m_pad,
                                                   const int *__restrict__ seeds, const unsigned *__restrict__ rows, double share,
                                                   unsigned char *__restrict__ status, int *__restrict__ size, double *__restrict__ Rt,
                                                   double *__restrict__ sums, unsigned char *__restrict__ member)
{
    __shared__ double sh[4][9];
    __shared__ unsigned shu[K15_FIT / SF_WAVE];
    const int s = blockIdx.x, tid = threadIdx.x;
    int64_t sd = seeds[s];
    if (sd >= m) sd = -1;
    const unsigned *row = rows + (int64_t)s * m_pad;
    unsigned char *mem = member ? member + (int64_t)s * m : nullptr;
    unsigned top = 0;
    if (sd >= 0)
        for (int64_t j = tid; j < m; j += K15_FIT) top = row[j] > top ? row[j] : top;
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned y = __shfl_xor(top, off);
        top = y > top ? y : top;
    }
    if ((tid & (SF_WAVE - 1)) == 0) shu[tid / SF_WAVE] = top;
    __syncthreads();
    for (int w = 0; w < K15_FIT / SF_WAVE; ++w) top = shu[w] > top ? shu[w] : top;
    const double cut = share * (double)top;
    // pass 0: the members, their count and their sums (a thread takes positions tid, tid + 256, .. in ascending order)
    double v0[7];
#pragma unroll
    for (int q = 0; q < 7; ++q) v0[q] = 0.0;
    for (int64_t j = tid; j < m; j += K15_FIT) {
        const unsigned r = sd >= 0 ? row[j] : 0u;
        const bool in = sd >= 0 && (j == sd || (r >= 1u && (double)r >= cut));
        if (mem) mem[j] = in ? 1 : 0;
        if (!in) continue;
        sf_refit_add_pair(v0, a[3 * j], a[3 * j + 1], a[3 * j + 2], b[3 * j], b[3 * j + 1], b[3 * j + 2]);
    }
    k15_block_sums<7>(v0, sh);
    const double n = v0[0];
    const bool fit = n >= 3.0;
    double mean[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) mean[q] = n > 0.0 ? v0[1 + q] / n : 0.0;
    // pass 1: the centred cross-covariance over the same members (of any count: the sums are an output of their own)
    double v1[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) v1[q] = 0.0;
    if (sd >= 0)
        for (int64_t j = tid; j < m; j += K15_FIT) {
            const unsigned r = row[j];
            if (!(j == sd || (r >= 1u && (double)r >= cut))) continue;
            sf_refit_add_centred(v1, mean, a[3 * j], a[3 * j + 1], a[3 * j + 2], b[3 * j], b[3 * j + 1], b[3 * j + 2]);
        }
    k15_block_sums<9>(v1, sh);
    if (tid != 0) return;
    unsigned char st = sd < 0 ? 3 : (fit ? 0 : 1);
    double o[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) o[q] = 0.0;
    if (st == 0 && !sf_horn::rigid_from_moments(mean, v1, o)) st = 2;
    status[s] = st;
    size[s] = (int)n;
#pragma unroll
    for (int q = 0; q < 12; ++q) Rt[12 * (int64_t)s + q] = o[q];
    if (sums) {
        double *out = sums + RS_SIZE * (int64_t)s;
        out[RS_COUNT] = n;
#pragma unroll
        for (int q = 0; q < 6; ++q) { out[RS_ABAR + q] = mean[q]; out[RS_SUM_A + q] = v0[1 + q]; } // a, then b
#pragma unroll
        for (int q = 0; q < 9; ++q) out[RS_H + q] = v1[q];
        out[RS_SSR] = 0.0;
        out[RS_SPARE] = 0.0;
    }
}

// counts[i] <- -1 for the slots past the scored ones (tallies[0]): K11's first maximum never takes them
__global__ void k15_mask_tail(int64_t *__restrict__ counts, int n_seeds, const unsigned long long *__restrict__ tallies)
{
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < n_seeds && (unsigned long long)i >= tallies[0]) counts[i] = -1;
}

// the chain's result (sf_sc2_registration) from the tallies of the compaction and the winner of the first maximum
__global__ void k15_result(const unsigned long long *__restrict__ tallies, const int64_t *__restrict__ win, const int *__restrict__ seeds,
                           const int *__restrict__ size, int n_seeds, int64_t *__restrict__ out)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int64_t slot = win[1]; // the winner's position among the seeds
    out[0] = (int64_t)n_seeds - (int64_t)tallies[3];
    out[1] = (int64_t)tallies[1];
    out[2] = (int64_t)tallies[2];
    out[3] = (int64_t)tallies[0];
    out[4] = slot >= 0 ? (int64_t)seeds[slot] : -1;
    out[5] = win[2];
    out[6] = slot;
    out[7] = slot >= 0 ? (int64_t)size[slot] : 0;
}

int k15_check_seeds(const char *who, int64_t n_seeds)
{
    if (n_seeds < 1 || n_seeds > SF_SC2_MAX_SEEDS) {
        sf_set_error("%s: n_seeds %lld outside 1 .. %d", who, (long long)n_seeds, SF_SC2_MAX_SEEDS);
        return SF_ERR_ARG;
    }
    return SF_OK;
}

int k15_check_share(const char *who, double share)
{
    if (!(share > 0.0 && share <= 1.0)) { sf_set_error("%s: group_share %g outside (0, 1]", who, share); return SF_ERR_ARG; }
    return SF_OK;
}

int k15_launch_seeds(sf_ctx *ctx, const unsigned *s2, int64_t m, int n_seeds, int *seeds)
{
    SF_HIP(hipMemsetAsync(seeds, 0xff, (size_t)n_seeds * sizeof(int), ctx->stream)); // -1
    SF_LAUNCH(ctx, "k15_seeds", k15_seeds, dim3((unsigned)sf_div_up(m, 256)), dim3(256), s2, m, n_seeds, seeds);
    return SF_OK;
}

int k15_launch_seed_rows(sf_ctx *ctx, const unsigned char *cmat, int64_t m, const int *seeds, int n_seeds, unsigned *rows)
{
    const int64_t m_pad = k14_pad(m);
    SF_LAUNCH(ctx, "k15_seed_rows", k15_seed_rows, dim3((unsigned)sf_div_up(n_seeds, K15_TS), (unsigned)(m_pad / K14_T)), dim3(512), cmat, m,
              m_pad, seeds, n_seeds, rows);
    return SF_OK;
}

int k15_launch_fit(sf_ctx *ctx, const double *a, const double *b, int64_t m, const int *seeds, const unsigned *rows, int n_seeds,
                   double share, unsigned char *status, int *size, double *Rt, double *sums, unsigned char *member)
{
    SF_LAUNCH(ctx, "k15_fit", k15_fit, dim3((unsigned)n_seeds), dim3(K15_FIT), a, b, m, k14_pad(m), seeds, rows, share, status, size, Rt,
              sums, member);
    return SF_OK;
}
} // namespace

extern "C" int sf_consistency_degree(sf_ctx *ctx, const double *a_dev, const double *b_dev, int64_t m,
                                     const unsigned char *member_dev, double distance_threshold, double min_edge,
                                     unsigned *degree_dev)
{
    SF_CHECK(k13_check("sf_consistency_degree", ctx && a_dev && b_dev && degree_dev, m, distance_threshold, min_edge));
    if (m == 0) return SF_OK;
    SF_HIP(hipSetDevice(ctx->device));
    return k13_launch_degree(ctx, a_dev, b_dev, m, member_dev, distance_threshold, min_edge, degree_dev);
}

extern "C" int sf_consistency_group(sf_ctx *ctx, const double *a_dev, const double *b_dev, int64_t m, double distance_threshold,
                                    double min_edge, unsigned *degree_dev, unsigned char *member_dev, unsigned *group_degree_dev,
                                    int64_t *info)
{
    SF_CHECK(k13_check("sf_consistency_group", ctx && a_dev && b_dev && degree_dev && member_dev && group_degree_dev && info, m,
                       distance_threshold, min_edge));
    if (m == 0) return SF_OK;
    SF_HIP(hipSetDevice(ctx->device));
    sf_pool_guard tmp(ctx);
    int64_t *dinfo = nullptr;
    SF_CHECK(tmp.alloc(&dinfo, IN_SIZE));
    const dim3 one(1), fold(K13_FOLD);
    // queued back to back: nothing below waits for the device
    SF_CHECK(k13_launch_degree(ctx, a_dev, b_dev, m, nullptr, distance_threshold, min_edge, degree_dev));
    SF_LAUNCH(ctx, "k13_argmax", k13_argmax, one, fold, (const unsigned *)degree_dev, m, dinfo);
    SF_LAUNCH(ctx, "k13_mark", k13_mark, dim3((unsigned)sf_div_up(m, K13_BLOCK)), dim3(K13_BLOCK), a_dev, b_dev, m, distance_threshold,
              min_edge, (const int64_t *)dinfo, member_dev);
    SF_LAUNCH(ctx, "k13_count", k13_count, one, fold, (const unsigned char *)member_dev, m, dinfo);
    SF_CHECK(k13_launch_degree(ctx, a_dev, b_dev, m, member_dev, distance_threshold, min_edge, group_degree_dev));
    void *pin = nullptr;
    SF_CHECK(sf_ctx_pinned(ctx, &pin));
    int64_t *hi = (int64_t *)pin;
    SF_HIP(hipMemcpyAsync(hi, dinfo, IN_SIZE * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    SF_HIP(hipStreamSynchronize(ctx->stream)); // the one wait of the call
    for (int v = 0; v < IN_SIZE; ++v) info[v] = hi[v];
    if (info[IN_STATUS] != 0) info[IN_SEED] = -1; // no compatible pair: no seed, no group
    return SF_OK;
}

extern "C" int sf_consistency_matrix(sf_ctx *ctx, const double *a_dev, const double *b_dev, int64_t m, double distance_threshold,
                                     double min_edge, unsigned char *cmat_dev)
{
    SF_CHECK(k13_check("sf_consistency_matrix", ctx && a_dev && b_dev && cmat_dev, m, distance_threshold, min_edge));
    SF_CHECK(k14_check_count("sf_consistency_matrix", true, m));
    if (m == 0) return SF_OK;
    SF_HIP(hipSetDevice(ctx->device));
    return k14_launch_matrix(ctx, a_dev, b_dev, m, distance_threshold, min_edge, cmat_dev);
}

extern "C" int sf_consistency_sc2(sf_ctx *ctx, const unsigned char *cmat_dev, int64_t m, unsigned *s2_dev)
{
    SF_CHECK(k14_check_count("sf_consistency_sc2", ctx && cmat_dev && s2_dev, m));
    if (m == 0) return SF_OK;
    SF_HIP(hipSetDevice(ctx->device));
    return k14_launch_sc2(ctx, cmat_dev, m, s2_dev);
}

extern "C" int sf_consistency_sc2_group(sf_ctx *ctx, const double *a_dev, const double *b_dev, int64_t m, double distance_threshold,
                                        double min_edge, unsigned *s2_dev, unsigned char *member_dev, unsigned *group_degree_dev,
                                        int64_t *info)
{
    SF_CHECK(k13_check("sf_consistency_sc2_group", ctx && a_dev && b_dev && s2_dev && member_dev && group_degree_dev && info, m,
                       distance_threshold, min_edge));
    SF_CHECK(k14_check_count("sf_consistency_sc2_group", true, m)); // (before anything is allocated)
    if (m == 0) return SF_OK;
    SF_HIP(hipSetDevice(ctx->device));
    sf_pool_guard tmp(ctx);
    int64_t *dinfo = nullptr;
    unsigned char *cmat = nullptr;
    const int64_t m_pad = k14_pad(m);
    SF_CHECK(tmp.alloc(&dinfo, IN_SIZE));
    SF_CHECK(tmp.alloc(&cmat, (size_t)m_pad * (size_t)m_pad));
    const dim3 one(1), fold(K13_FOLD);
    // queued back to back: nothing below waits for the device.  The first maximum of s2 is K13's arg-max on another array; the
    // seed's row, its count and the degree inside the group are K13's own kernels, so they agree with the matrix bit for bit.
    SF_CHECK(k14_launch_matrix(ctx, a_dev, b_dev, m, distance_threshold, min_edge, cmat));
    SF_CHECK(k14_launch_sc2(ctx, cmat, m, s2_dev));
    SF_LAUNCH(ctx, "k13_argmax", k13_argmax, one, fold, (const unsigned *)s2_dev, m, dinfo);
    SF_LAUNCH(ctx, "k13_mark", k13_mark, dim3((unsigned)sf_div_up(m, K13_BLOCK)), dim3(K13_BLOCK), a_dev, b_dev, m, distance_threshold,
              min_edge, (const int64_t *)dinfo, member_dev);
    SF_LAUNCH(ctx, "k13_count", k13_count, one, fold, (const unsigned char *)member_dev, m, dinfo);
    SF_CHECK(k13_launch_degree(ctx, a_dev, b_dev, m, member_dev, distance_threshold, min_edge, group_degree_dev));
    void *pin = nullptr;
    SF_CHECK(sf_ctx_pinned(ctx, &pin));
    int64_t *hi = (int64_t *)pin;
    SF_HIP(hipMemcpyAsync(hi, dinfo, IN_SIZE * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    SF_HIP(hipStreamSynchronize(ctx->stream)); // the one wait of the call
    for (int v = 0; v < IN_SIZE; ++v) info[v] = hi[v];
    if (info[IN_STATUS] != 0) info[IN_SEED] = -1; // no consistent triple: no seed, no group
    return SF_OK;
}

extern "C" int sf_sc2_seeds(sf_ctx *ctx, const unsigned *s2_dev, int64_t m, int64_t n_seeds, int *seeds_dev)
{
    SF_CHECK(k14_check_count("sf_sc2_seeds", ctx && s2_dev && seeds_dev, m));
    SF_CHECK(k15_check_seeds("sf_sc2_seeds", n_seeds));
    if (m == 0) return SF_OK;
    SF_HIP(hipSetDevice(ctx->device));
    return k15_launch_seeds(ctx, s2_dev, m, (int)n_seeds, seeds_dev);
}

extern "C" int sf_sc2_seed_rows(sf_ctx *ctx, const unsigned char *cmat_dev, int64_t m, const int *seeds_dev, int64_t n_seeds,
                                unsigned *rows_dev)
{
    SF_CHECK(k14_check_count("sf_sc2_seed_rows", ctx && cmat_dev && seeds_dev && rows_dev, m));
    SF_CHECK(k15_check_seeds("sf_sc2_seed_rows", n_seeds));
    if (m == 0) return SF_OK;
    SF_HIP(hipSetDevice(ctx->device));
    return k15_launch_seed_rows(ctx, cmat_dev, m, seeds_dev, (int)n_seeds, rows_dev);
}

extern "C" int sf_sc2_seed_fits(sf_ctx *ctx, const double *a_dev, const double *b_dev, int64_t m, const int *seeds_dev,
                                const unsigned *rows_dev, int64_t n_seeds, double group_share, unsigned char *status_dev,
                                int *size_dev, double *Rt_dev, double *sums_dev, unsigned char *member_dev)
{
    SF_CHECK(k14_check_count("sf_sc2_seed_fits", ctx && a_dev && b_dev && seeds_dev && rows_dev && status_dev && size_dev && Rt_dev, m));
    SF_CHECK(k15_check_seeds("sf_sc2_seed_fits", n_seeds));
    SF_CHECK(k15_check_share("sf_sc2_seed_fits", group_share));
    if (m == 0) return SF_OK;
    SF_HIP(hipSetDevice(ctx->device));
    return k15_launch_fit(ctx, a_dev, b_dev, m, seeds_dev, rows_dev, (int)n_seeds, group_share, status_dev, size_dev, Rt_dev, sums_dev,
                          member_dev);
}

extern "C" int sf_sc2_registration(sf_ctx *ctx, const double *a_dev, const double *b_dev, int64_t m, double distance_threshold,
                                   double min_edge, int64_t n_seeds, double group_share, unsigned *s2_dev, int *seeds_dev,
                                   unsigned char *status_dev, int *size_dev, double *Rt_dev, int64_t *map_dev, int64_t *counts_dev,
                                   int64_t *result, double *best_Rt)
{
    SF_CHECK(k13_check("sf_sc2_registration", ctx && a_dev && b_dev && result && best_Rt, m, distance_threshold, min_edge));
    SF_CHECK(k14_check_count("sf_sc2_registration", true, m)); // (before anything is allocated)
    SF_CHECK(k15_check_seeds("sf_sc2_registration", n_seeds));
    SF_CHECK(k15_check_share("sf_sc2_registration", group_share));
    if (m == 0) return SF_OK;
    SF_HIP(hipSetDevice(ctx->device));
    sf_pool_guard tmp(ctx);
    const int ns = (int)n_seeds;
    const int64_t m_pad = k14_pad(m), nblocks = sf_k11_blocks(ns);
    unsigned char *cmat = nullptr;
    unsigned *rows = nullptr;
    double *Rt_all = nullptr, *dbest = nullptr;
    int *block_count = nullptr;
    int64_t *block_off = nullptr, *dwin = nullptr, *dres = nullptr;
    unsigned long long *tallies = nullptr;
    if (!s2_dev) SF_CHECK(tmp.alloc(&s2_dev, (size_t)m));
    if (!seeds_dev) SF_CHECK(tmp.alloc(&seeds_dev, (size_t)ns));
    if (!status_dev) SF_CHECK(tmp.alloc(&status_dev, (size_t)ns));
    if (!size_dev) SF_CHECK(tmp.alloc(&size_dev, (size_t)ns));
    if (!Rt_dev) SF_CHECK(tmp.alloc(&Rt_dev, (size_t)ns * 12));
    if (!map_dev) SF_CHECK(tmp.alloc(&map_dev, (size_t)ns));
    if (!counts_dev) SF_CHECK(tmp.alloc(&counts_dev, (size_t)ns));
    SF_CHECK(tmp.alloc(&cmat, (size_t)m_pad * (size_t)m_pad));
    SF_CHECK(tmp.alloc(&rows, (size_t)ns * (size_t)m_pad));
    SF_CHECK(tmp.alloc(&Rt_all, (size_t)ns * 12));
    SF_CHECK(tmp.alloc(&block_count, (size_t)nblocks));
    SF_CHECK(tmp.alloc(&block_off, (size_t)nblocks));
    SF_CHECK(tmp.alloc(&tallies, 4));
    SF_CHECK(tmp.alloc(&dwin, 4));
    SF_CHECK(tmp.alloc(&dbest, 12));
    SF_CHECK(tmp.alloc(&dres, 8));
    // queued back to back: nothing below waits for the device.  The compacted rows past the scored ones are zero transforms whose
    // counts are set to -1 before the first maximum, so K9 and K11's arg-max run over n_seeds slots without knowing how many count.
    SF_CHECK(k14_launch_matrix(ctx, a_dev, b_dev, m, distance_threshold, min_edge, cmat));
    SF_CHECK(k14_launch_sc2(ctx, cmat, m, s2_dev));
    SF_CHECK(k15_launch_seeds(ctx, s2_dev, m, ns, seeds_dev));
    SF_CHECK(k15_launch_seed_rows(ctx, cmat, m, seeds_dev, ns, rows));
    SF_CHECK(k15_launch_fit(ctx, a_dev, b_dev, m, seeds_dev, rows, ns, group_share, status_dev, size_dev, Rt_all, nullptr, nullptr));
    SF_HIP(hipMemsetAsync(Rt_dev, 0, (size_t)ns * 12 * sizeof(double), ctx->stream));
    SF_HIP(hipMemsetAsync(map_dev, 0xff, (size_t)ns * sizeof(int64_t), ctx->stream)); // -1
    SF_CHECK(sf_k11_compact(ctx, status_dev, Rt_all, ns, Rt_dev, map_dev, block_count, block_off, tallies));
    SF_CHECK(sf_ransac_score(ctx, a_dev, b_dev, m, Rt_dev, ns, distance_threshold, counts_dev, SF_IN_DEVICE | SF_OUT_DEVICE));
    SF_LAUNCH(ctx, "k15_mask_tail", k15_mask_tail, dim3((unsigned)sf_div_up(ns, 256)), dim3(256), counts_dev, ns,
              (const unsigned long long *)tallies);
    SF_CHECK(sf_k11_first_max(ctx, counts_dev, ns, map_dev, Rt_dev, dwin, dbest));
    SF_LAUNCH(ctx, "k15_result", k15_result, dim3(1), dim3(64), (const unsigned long long *)tallies, (const int64_t *)dwin,
              (const int *)seeds_dev, (const int *)size_dev, ns, dres);
    void *pin = nullptr;
    SF_CHECK(sf_ctx_pinned(ctx, &pin));
    int64_t *hr = (int64_t *)pin;
    double *hb = (double *)((char *)pin + 64);
    SF_HIP(hipMemcpyAsync(hr, dres, 8 * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    SF_HIP(hipMemcpyAsync(hb, dbest, 12 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    SF_HIP(hipStreamSynchronize(ctx->stream)); // the one wait of the call
    for (int v = 0; v < 8; ++v) result[v] = hr[v];
    memcpy(best_Rt, hb, 12 * sizeof(double));
    return SF_OK;
}
