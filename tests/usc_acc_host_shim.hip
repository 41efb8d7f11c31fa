// The exact sums of K21 compiled for the HOST: extern "C" wrappers over usc_acc_split / usc_acc_round (csrc/usc_acc.h) and
// nothing else.  tests/test_usc_host.py builds this file with the library's own floating-point flags and compares it with
// fractions.Fraction without a GPU.
#include <cstdint>

#include "usc_acc.h"

// the limbs of one weight; 0 when it lies outside [2^-22, 1]
extern "C" int usc_acc_split_host(double w, unsigned long long *lo, unsigned long long *hi) { return usc_acc_split(w, *lo, *hi) ? 1 : 0; }

// the double nearest to (hi 2^40 + lo) 2^-75
extern "C" double usc_acc_round_host(unsigned long long lo, unsigned long long hi) { return usc_acc_round(lo, hi); }

// what a bin of the kernel does with n weights: the two limb sums, rounded once; *rejected: weights out of range (left out)
extern "C" double usc_acc_sum_host(const double *w, int64_t n, int64_t *rejected)
{
    unsigned long long sum_lo = 0, sum_hi = 0;
    *rejected = 0;
    for (int64_t i = 0; i < n; ++i) {
        unsigned long long lo, hi;
        if (usc_acc_split(w[i], lo, hi)) {
            sum_lo += lo;
            sum_hi += hi;
        } else {
            ++*rejected;
        }
    }
    return usc_acc_round(sum_lo, sum_hi);
}
