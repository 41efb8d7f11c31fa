// select.hip -- K18: the exact rank-th smallest of n doubles resident in HBM, by radix selection on their bit patterns.
//
// Key order.  The sign bit is cleared; the remaining 63-bit pattern of a non-negative double orders like its value, -0.0 orders as
// zero, +inf orders above every finite value and the NaNs last: np.partition's order.  The all-ones pattern (what the trimmed ICP
// chain writes for a slot outside d_max, csrc/icp.hip) is the largest key of all.
//
// The 63 bits are taken in six digits of 11, 11, 11, 10, 10 and 10 bits, from the top.  Pass p is ONE launch of k_select_hist:
//   head   (p >= 1) every block repeats the PICK of pass p - 1 from that pass's finished histogram -- a parallel scan of its 2 048 or
//          1 024 bins, eight or four per thread, for the bucket that holds the rank -- and so knows (prefix, remaining rank) without a
//          launch of its own and without the host; block 0 leaves that state in device memory for the next launch;
//   body   a block-strided histogram of digit p over the keys whose higher digits equal the prefix: per-block LDS counters (32-bit:
//          a block sees n / gridDim keys, below 2^32 for any array that fits the device), merged into the pass's own global 64-bit
//          histogram with integer atomics.  A wave whose active lanes all carry one digit -- the rule once the prefix has narrowed
//          the keys down, and for all-equal keys from the first pass on -- adds its lane count once instead of 64 times to one bin.
// k_select_final picks from the last histogram and writes the result.  Integer counts do not depend on the order of the adds, so a
// call repeats bit for bit; there is no floating-point atomic.  Seven launches and one fill, no host wait in between.
//
// The rank is either given, or -- for the trimmed chain -- formed on the device by the first pick from the count n0 of keys that are
// not the all-ones pattern, which pass 0 counts beside its histogram: rank = min(n0, max(1, ceil(trim * n0))).
#include "common.h"
#include "select.h"

namespace {

constexpr int SEL_PASSES = 6;
constexpr int SEL_BLOCKS = 256;
constexpr int SEL_STRIDE = 2049; // counters per pass: 2 048 bins and, in pass 0, the count of keys that are not all ones
constexpr uint64_t SEL_KEY_MASK = 0x7fffffffffffffffull;
constexpr uint64_t SEL_NO_KEY = ~0ull;
__host__ __device__ constexpr int sel_bits(int pass) { return pass < 3 ? 11 : 10; }                          // 11 11 11 10 10 10
__host__ __device__ constexpr int sel_shift(int pass) { return pass < 3 ? 52 - 11 * pass : 50 - 10 * pass; } // 52 41 30 20 10 0

struct sel_state {
    unsigned long long prefix; // the digits found so far, most significant first
    long long rank;            // 1-based rank among the keys that carry the prefix
    long long below;           // keys that order below every key with the prefix
    long long n0;              // keys that are not the all-ones pattern
    long long rank0;           // the rank the selection started from
    long long bucket;          // keys in the bucket of the last pick
};

// the pick of one pass by all 256 threads of a block: the bucket b with  (keys in buckets < b) < rank <= (keys in buckets <= b)
__device__ inline sel_state pick_step(const unsigned long long *__restrict__ hist, int bits, sel_state s)
{
    __shared__ unsigned long long wave_total[4];
    __shared__ unsigned long long found[3];
    const int per = (1 << bits) >> 8; // 8 or 4 bins per thread
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long c[8], mine = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        c[j] = j < per ? hist[threadIdx.x * per + j] : 0ull;
        mine += c[j];
    }
    unsigned long long inc = mine; // inclusive scan over the wave
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long v = __shfl_up(inc, off);
        if (lane >= off) inc += v;
    }
    if (lane == 63) wave_total[wave] = inc;
    if (threadIdx.x == 0) found[0] = found[1] = found[2] = 0ull;
    __syncthreads();
    unsigned long long before = inc - mine;
    for (int w = 0; w < wave; ++w) before += wave_total[w];
    const unsigned long long r = (unsigned long long)s.rank;
    if (before < r && r <= before + mine) { // one thread at most; none for a rank of 0 (no key at all)
        unsigned long long b = before;
        bool done = false;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (!done && r <= b + c[j]) {
                found[0] = (unsigned long long)(threadIdx.x * per + j);
                found[1] = b;
                found[2] = c[j];
                done = true;
            }
            if (!done) b += c[j];
        }
    }
    __syncthreads();
    s.prefix = (s.prefix << bits) | found[0];
    s.rank -= (long long)found[1];
    s.below += (long long)found[1];
    s.bucket = (long long)found[2];
    __syncthreads(); // `found` may be written again by a later call
    return s;
}

// the state before the first pick: the given rank, or the trimmed chain's share of the n0 keys pass 0 counted
__device__ inline sel_state first_state(const unsigned long long *__restrict__ hist, int64_t rank, double trim)
{
    sel_state s = {0ull, (long long)rank, 0ll, (long long)hist[SEL_STRIDE - 1], 0ll, 0ll};
    if (trim > 0.0) {
        long long r = (long long)ceil(trim * (double)s.n0);
        if (r < 1) r = 1;
        s.rank = r < s.n0 ? r : s.n0;
    }
    s.rank0 = s.rank;
    return s;
}

__global__ __launch_bounds__(256) void k_select_hist(const uint64_t *__restrict__ keys, int64_t n, int pass, int64_t rank, double trim,
                                                     unsigned long long *__restrict__ hist /* SEL_PASSES x SEL_STRIDE, zero */,
                                                     sel_state *__restrict__ state /* SEL_PASSES */)
{
    __shared__ unsigned int bins[SEL_STRIDE];
    for (int b = threadIdx.x; b < SEL_STRIDE; b += 256) bins[b] = 0u;
    sel_state s = {0ull, 0ll, 0ll, 0ll, 0ll, 0ll};
    if (pass > 0) {
        s = pass == 1 ? first_state(hist, rank, trim) : state[pass - 1];
        s = pick_step(hist + (size_t)(pass - 1) * SEL_STRIDE, sel_bits(pass - 1), s);
        if (blockIdx.x == 0 && threadIdx.x == 0) state[pass] = s;
    }
    __syncthreads();
    const int shift = sel_shift(pass), above = pass > 0 ? sel_shift(pass - 1) : 63;
    const unsigned int digit_mask = (1u << sel_bits(pass)) - 1u;
    const int lane = threadIdx.x & 63;
    unsigned int real = 0;
    for (int64_t base = (int64_t)blockIdx.x * 256; base < n; base += (int64_t)gridDim.x * 256) { // uniform over the block
        const int64_t i = base + threadIdx.x;
        const uint64_t raw = i < n ? keys[i] : SEL_NO_KEY;
        const uint64_t key = raw & SEL_KEY_MASK;
        const bool take = i < n && (key >> above) == s.prefix; // (pass 0: key >> 63 = 0 = the empty prefix)
        const unsigned int digit = (unsigned int)(key >> shift) & digit_mask;
        real += raw != SEL_NO_KEY;
        const unsigned long long active = __ballot(take);
        if (active) {
            const int lead = __ffsll((long long)active) - 1;
            const unsigned int first = __shfl(digit, lead);
            if (__all(!take || digit == first)) {
                if (lane == lead) atomicAdd(&bins[first], (unsigned int)__popcll(active));
            } else if (take) {
                atomicAdd(&bins[digit], 1u);
            }
        }
    }
    if (pass == 0 && real) atomicAdd(&bins[SEL_STRIDE - 1], real);
    __syncthreads();
    unsigned long long *mine = hist + (size_t)pass * SEL_STRIDE;
    for (int b = threadIdx.x; b < SEL_STRIDE; b += 256)
        if (bins[b]) atomicAdd(&mine[b], (unsigned long long)bins[b]);
}

// the last pick, and the result: [0] the value (the key's pattern: a zero is +0.0), [1] keys that order below it, [2] keys that order
// at or below it, [3] 0, [4] n0, [5] the rank the selection started from; with a rank of 0 (the trimmed chain without a pair) all zero
__global__ __launch_bounds__(256) void k_select_final(const unsigned long long *__restrict__ hist, const sel_state *__restrict__ state,
                                                      double *__restrict__ res /* 8 */)
{
    sel_state s = pick_step(hist + (size_t)(SEL_PASSES - 1) * SEL_STRIDE, sel_bits(SEL_PASSES - 1), state[SEL_PASSES - 1]);
    if (threadIdx.x) return;
    const bool any = s.rank0 > 0;
    res[0] = any ? __longlong_as_double((long long)s.prefix) : 0.0;
    res[1] = any ? (double)s.below : 0.0;
    res[2] = any ? (double)(s.below + s.bucket) : 0.0;
    res[3] = 0.0;
    res[4] = (double)s.n0;
    res[5] = (double)s.rank0;
    res[6] = res[7] = 0.0;
}

} // namespace

int sf_select_launch(sf_ctx *ctx, const uint64_t *keys_dev, int64_t n, int64_t rank, double trim, double *res_dev)
{
    sf_pool_guard tmp(ctx);
    unsigned long long *work = nullptr; // the six histograms, then the states
    constexpr size_t hist_words = (size_t)SEL_PASSES * SEL_STRIDE;
    constexpr size_t state_words = (sizeof(sel_state) * SEL_PASSES + 7) / 8;
    SF_CHECK(tmp.alloc(&work, hist_words + state_words));
    SF_HIP(hipMemsetAsync(work, 0, (hist_words + state_words) * sizeof(unsigned long long), ctx->stream));
    sel_state *state = (sel_state *)(work + hist_words);
    const dim3 grid((unsigned)(sf_div_up(n, 256) < SEL_BLOCKS ? sf_div_up(n, 256) : SEL_BLOCKS)), block(256);
    for (int pass = 0; pass < SEL_PASSES; ++pass) {
        SF_LAUNCH(ctx, "i2_select_hist", k_select_hist, grid, block, keys_dev, n, pass, rank, trim, work, state);
    }
    SF_LAUNCH(ctx, "i2_select_final", k_select_final, dim3(1), block, (const unsigned long long *)work, (const sel_state *)state, res_dev);
    return SF_OK;
}

extern "C" int sf_select_kth(sf_ctx *ctx, const double *keys_dev, int64_t n, int64_t rank, double *out)
{
    const char *bad = nullptr;
    if (!ctx) bad = "ctx";
    else if (!keys_dev) bad = "keys_dev";
    else if (!out) bad = "out";
    else if (n < 1) bad = "n (must be at least 1)";
    else if (rank < 1 || rank > n) bad = "rank (must lie in 1 .. n)";
    if (bad) { sf_set_error("sf_select_kth: bad argument %s", bad); return SF_ERR_ARG; }
    SF_HIP(hipSetDevice(ctx->device));
    sf_pool_guard tmp(ctx);
    double *res = nullptr;
    SF_CHECK(tmp.alloc(&res, 8));
    SF_CHECK(sf_select_launch(ctx, (const uint64_t *)keys_dev, n, rank, 0.0, res));
    SF_HIP(hipMemcpyAsync(out, res, 4 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    SF_HIP(hipStreamSynchronize(ctx->stream));
    return SF_OK;
}
