// The library's 3 x 3 eigensolver compiled for the HOST: an extern "C" wrapper over sf_eig::eigh3_lower and nothing else.
// tests/test_eigh3_host.py builds this file with the library's own floating-point flags and compares it with the oracle
// without a GPU.  Layouts are sf_eigh3's: lower = a11 a21 a31 a22 a32 a33, v[3 r + k] = component r of eigenvector k.
#include <cstdint>

#include "eigh3.h"

extern "C" void eigh3_host(const double *lower, int64_t m, double *w, double *v)
{
    for (int64_t i = 0; i < m; ++i) {
        const double *c = lower + 6 * i;
        const sf_eig::eig3 e = sf_eig::eigh3_lower(c[0], c[1], c[2], c[3], c[4], c[5]);
        w[3 * i + 0] = e.w1; w[3 * i + 1] = e.w2; w[3 * i + 2] = e.w3;
        double *o = v + 9 * i;
        o[0] = e.v11; o[1] = e.v12; o[2] = e.v13;
        o[3] = e.v21; o[4] = e.v22; o[5] = e.v23;
        o[6] = e.v31; o[7] = e.v32; o[8] = e.v33;
    }
}
