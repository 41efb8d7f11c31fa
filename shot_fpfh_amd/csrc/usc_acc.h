// usc_acc.h -- the exact sums of K21 (usc.hip): a density weight as two integer limbs, and the two limb sums of a bin back as
// the correctly rounded double.  Host and device (tests/usc_acc_host_shim.hip builds it for the CPU).
//
// A weight w = 1 / c, c an integer in [1, 2^22), is a 53-bit mantissa times 2^e with e >= -74: a whole multiple of the unit
// 2^-75, at most 2^75 of them (w = 1).  That integer W (76 bits) is split at bit 40: lo = W mod 2^40, hi = W div 2^40 < 2^36.
// Over a list of fewer than 2^24 entries the sum of the lo limbs stays below 2^64 and the sum of the hi limbs below 2^60, so a
// bin is two 64-bit integer adds per neighbour, in any order, and nothing is ever rounded while it is being summed.
// At read-out the sum is S = hi 2^40 + lo, an integer below 2^100; usc_acc_round returns the double nearest to S 2^-75, ties to
// even, from the top 53 bits of S, the bit below them and a sticky bit for all the rest -- ONE rounding, which is what math.fsum
// of the same weights returns.  ((double)hi 2^40 + (double)lo would round each limb first, and the sum again.)
#pragma once
#include <cmath>
#include <cstdint>

#ifndef __host__
#define __host__
#define __device__
#endif

#define USC_ACC_UNIT_LOG2 75     // the limbs count units of 2^-75
#define USC_ACC_SPLIT 40         // W = hi 2^40 + lo
#define USC_ACC_MAX_LIST (1 << 24) // lists below this length cannot overflow a limb

// The two limbs of w.  False (limbs untouched) when w lies outside [2^-22, 1]; a NaN fails the first comparison.
__host__ __device__ inline bool usc_acc_split(double w, unsigned long long &lo, unsigned long long &hi)
{
    if (!(w >= 0x1p-22 && w <= 1.0)) return false;
    unsigned long long bits;
    __builtin_memcpy(&bits, &w, sizeof bits);
    const unsigned long long mant = (bits & 0x000fffffffffffffull) | 0x0010000000000000ull; // w = mant 2^(exp - 1075)
    const int shift = (int)(bits >> 52) - (1075 - USC_ACC_UNIT_LOG2);                       // W = mant << shift, 1 <= shift <= 23
    lo = (mant << shift) & ((1ull << USC_ACC_SPLIT) - 1ull); // (bits shifted out of the 64 lie above bit 40)
    hi = mant >> (USC_ACC_SPLIT - shift);
    return true;
}

// The double nearest to (hi 2^40 + lo) 2^-75, ties to even.  lo, hi: any 64-bit sums (S < 2^105).
__host__ __device__ inline double usc_acc_round(unsigned long long lo, unsigned long long hi)
{
    // S as two 64-bit words
    const unsigned long long add = hi << USC_ACC_SPLIT;
    const unsigned long long s0 = lo + add;
    const unsigned long long s1 = (hi >> (64 - USC_ACC_SPLIT)) + (s0 < add ? 1ull : 0ull);
    if ((s0 | s1) == 0ull) return 0.0;
    const int top = s1 ? 127 - __builtin_clzll(s1) : 63 - __builtin_clzll(s0); // position of the leading bit
    if (top <= 52) return ldexp((double)s0, -USC_ACC_UNIT_LOG2);               // 53 bits or fewer: exact
    // m54 = S >> k keeps 54 bits: the 53 of the result and the half bit; sticky: any bit of S below them
    const int k = top - 53;
    unsigned long long m54, rest;
    if (k == 0) {
        m54 = s0;
        rest = 0ull;
    } else if (k < 64) {
        m54 = (s0 >> k) | (s1 << (64 - k)); // (s1 << (64 - k): the bits of s1 that land in the low word; k >= 1)
        rest = s0 & ((1ull << k) - 1ull);
    } else {
        m54 = s1 >> (k - 64);
        rest = s0 | (s1 & ((1ull << (k - 64)) - 1ull));
    }
    unsigned long long m = m54 >> 1;
    if ((m54 & 1ull) && (rest != 0ull || (m & 1ull))) ++m; // (m = 2^53 after a carry is still exact as a double)
    return ldexp((double)m, k + 1 - USC_ACC_UNIT_LOG2);
}
