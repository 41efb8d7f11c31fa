// horn4.h -- the rotation R in SO(3) that maximises tr(R H) for a 3x3 cross-covariance H = sum (a - abar)(b - bbar)^T, i.e. what
// the reference's SVD Kabsch with its reflection fix returns (core/solvers.py:19-28), without an SVD.
//
// Horn (1987): with S = H, the unit quaternion q of R is the eigenvector of the LARGEST eigenvalue of the symmetric 4x4
//   N = [ Sxx+Syy+Szz   Syz-Szy        Szx-Sxz        Sxy-Syx      ]
//       [ .             Sxx-Syy-Szz    Sxy+Syx        Szx+Sxz      ]
//       [ .             .             -Sxx+Syy-Szz    Syz+Szy      ]
//       [ .             .              .             -Sxx-Syy+Szz  ]
// The eigenvalues of N are, with s1 >= s2 >= s3 the singular values of H and e = sign(det H),
//   s1 + s2 + e s3  >=  s1 - s2 - e s3  >=  -s1 + s2 - e s3  >=  -s1 - s2 + e s3,
// so the two largest give what decides whether the maximiser is unique:  gap = s2 + e s3 = (l1 - l2) / 2 and s1 = (l1 + l2) / 2.
// The eigenvector's condition is |N| / (l1 - l2) ~ s1 / gap -- the condition of the polar factor itself; going through H^T H
// would square it (a 3-point sample has s3 = 0 always).
//
// Method: cyclic Jacobi with a fixed number of sweeps on the ten entries of N (every rotation is written out on named scalars: no
// array is indexed at run time, everything stays in VGPRs, as in eigh3.h), then ONE first-order correction of the chosen eigenvector
// against the ORIGINAL N -- residual r = N q - l q, q += sum_j v_j (v_j . r) / (l - l_j) -- which takes out what the ~40
// rotations accumulated: what is left is the rounding of one 4x4 product over the gap.
#pragma once
#include <hip/hip_runtime.h>

#include "common.h"

namespace sf_horn {

struct rot3 {
    double r0, r1, r2, r3, r4, r5, r6, r7, r8; // row-major
    double gap, s1;                            // s2 + sign(det H) s3 and s1, from N's two largest eigenvalues
};

// a0 b0 + a1 b1 + a2 b2 + c to the last bit or two: exact products (fma) and error-free sums (Knuth's two-sum)
__host__ __device__ inline double dot3m1(double a0, double b0, double a1, double b1, double a2, double b2, double c)
{
    double s = c, err = 0.0;
#define SF_HORN_ACC(a, b)                                       \
    do {                                                        \
        const double p_ = (a) * (b), pe_ = fma((a), (b), -p_);  \
        const double t_ = s + p_, bb_ = t_ - s;                 \
        err += pe_ + ((s - (t_ - bb_)) + (p_ - bb_));           \
        s = t_;                                                 \
    } while (0)
    SF_HORN_ACC(a0, b0);
    SF_HORN_ACC(a1, b1);
    SF_HORN_ACC(a2, b2);
#undef SF_HORN_ACC
    return s + err;
}

#define SF_HORN_ROT(app, aqq, apq, arp, arq, asp, asq, v0p, v0q, v1p, v1q, v2p, v2q, v3p, v3q)                          \
    do {                                                                                                                 \
        if (fabs(apq) <= 8.673617379884035e-19 * (fabs(app) + fabs(aqq)) || !(fabs(apq) > 0.0)) { /* 2^-60 */            \
            apq = 0.0;                                                                                                   \
        } else {                                                                                                         \
            const double th_ = (aqq - app) / (2.0 * apq);                                                                \
            const double t_ = copysign(1.0, th_) / (fabs(th_) + sqrt(th_ * th_ + 1.0));                                  \
            const double c_ = 1.0 / sqrt(t_ * t_ + 1.0), s_ = t_ * c_, tau_ = s_ / (1.0 + c_);                           \
            double g_, h_;                                                                                               \
            app -= t_ * apq; aqq += t_ * apq; apq = 0.0;                                                                 \
            g_ = arp; h_ = arq; arp = g_ - s_ * (h_ + tau_ * g_); arq = h_ + s_ * (g_ - tau_ * h_);                      \
            g_ = asp; h_ = asq; asp = g_ - s_ * (h_ + tau_ * g_); asq = h_ + s_ * (g_ - tau_ * h_);                      \
            g_ = v0p; h_ = v0q; v0p = g_ - s_ * (h_ + tau_ * g_); v0q = h_ + s_ * (g_ - tau_ * h_);                      \
            g_ = v1p; h_ = v1q; v1p = g_ - s_ * (h_ + tau_ * g_); v1q = h_ + s_ * (g_ - tau_ * h_);                      \
            g_ = v2p; h_ = v2q; v2p = g_ - s_ * (h_ + tau_ * g_); v2q = h_ + s_ * (g_ - tau_ * h_);                      \
            g_ = v3p; h_ = v3q; v3p = g_ - s_ * (h_ + tau_ * g_); v3q = h_ + s_ * (g_ - tau_ * h_);                      \
        }                                                                                                                \
    } while (0)

// H row-major: h<i><j> = sum a_i b_j.  A non-finite H gives a non-finite (or zero) gap: the caller's `gap > tol * s1` is false.
__host__ __device__ inline rot3 kabsch_rotation(double h00, double h01, double h02, double h10, double h11, double h12,
                                                double h20, double h21, double h22)
{
    const double n00 = (h00 + h11) + h22, n01 = h12 - h21, n02 = h20 - h02, n03 = h01 - h10;
    const double n11 = (h00 - h11) - h22, n12 = h01 + h10, n13 = h20 + h02;
    const double n22 = (h11 - h00) - h22, n23 = h12 + h21;
    const double n33 = (h22 - h00) - h11;
    double a00 = n00, a01 = n01, a02 = n02, a03 = n03, a11 = n11, a12 = n12, a13 = n13, a22 = n22, a23 = n23, a33 = n33;
    double v00 = 1, v01 = 0, v02 = 0, v03 = 0, v10 = 0, v11 = 1, v12 = 0, v13 = 0;
    double v20 = 0, v21 = 0, v22 = 1, v23 = 0, v30 = 0, v31 = 0, v32 = 0, v33 = 1;
    for (int sweep = 0; sweep < 8; ++sweep) { // (quadratic convergence: 5 sweeps reach 2^-60 on a 4x4; 8 leave a margin)
        SF_HORN_ROT(a00, a11, a01, a02, a12, a03, a13, v00, v01, v10, v11, v20, v21, v30, v31);
        SF_HORN_ROT(a00, a22, a02, a01, a12, a03, a23, v00, v02, v10, v12, v20, v22, v30, v32);
        SF_HORN_ROT(a00, a33, a03, a01, a13, a02, a23, v00, v03, v10, v13, v20, v23, v30, v33);
        SF_HORN_ROT(a11, a22, a12, a01, a02, a13, a23, v01, v02, v11, v12, v21, v22, v31, v32);
        SF_HORN_ROT(a11, a33, a13, a01, a03, a12, a23, v01, v03, v11, v13, v21, v23, v31, v33);
        SF_HORN_ROT(a22, a33, a23, a02, a03, a12, a13, v02, v03, v12, v13, v22, v23, v32, v33);
    }
    // the largest eigenvalue (first maximum) and the largest of the other three
    int k = 0;
    double l1 = a00;
    if (a11 > l1) { k = 1; l1 = a11; }
    if (a22 > l1) { k = 2; l1 = a22; }
    if (a33 > l1) { k = 3; l1 = a33; }
    const double o0 = k == 0 ? a11 : a00, o1 = k <= 1 ? a22 : a11, o2 = k <= 2 ? a33 : a22;
    const double l2 = fmax(fmax(o0, o1), o2);
    double q0 = k == 0 ? v00 : (k == 1 ? v01 : (k == 2 ? v02 : v03));
    double q1 = k == 0 ? v10 : (k == 1 ? v11 : (k == 2 ? v12 : v13));
    double q2 = k == 0 ? v20 : (k == 1 ? v21 : (k == 2 ? v22 : v23));
    double q3 = k == 0 ? v30 : (k == 1 ? v31 : (k == 2 ? v32 : v33));
    // one correction against the original N
    const double y0 = ((n00 * q0 + n01 * q1) + n02 * q2) + n03 * q3;
    const double y1 = ((n01 * q0 + n11 * q1) + n12 * q2) + n13 * q3;
    const double y2 = ((n02 * q0 + n12 * q1) + n22 * q2) + n23 * q3;
    const double y3 = ((n03 * q0 + n13 * q1) + n23 * q2) + n33 * q3;
    const double lam = (((q0 * y0 + q1 * y1) + q2 * y2) + q3 * y3) / (((q0 * q0 + q1 * q1) + q2 * q2) + q3 * q3);
    const double e0 = y0 - lam * q0, e1 = y1 - lam * q1, e2 = y2 - lam * q2, e3 = y3 - lam * q3;
#define SF_HORN_FIX(j, lj, w0, w1, w2, w3)                                              \
    do {                                                                                \
        const double den_ = lam - (lj);                                                 \
        double cf_ = (((w0) * e0 + (w1) * e1) + (w2) * e2) + (w3) * e3;                 \
        cf_ = (k != (j) && den_ > 0.0) ? cf_ / den_ : 0.0;                              \
        d0 += cf_ * (w0); d1 += cf_ * (w1); d2 += cf_ * (w2); d3 += cf_ * (w3);         \
    } while (0)
    double d0 = 0.0, d1 = 0.0, d2 = 0.0, d3 = 0.0;
    SF_HORN_FIX(0, a00, v00, v10, v20, v30);
    SF_HORN_FIX(1, a11, v01, v11, v21, v31);
    SF_HORN_FIX(2, a22, v02, v12, v22, v32);
    SF_HORN_FIX(3, a33, v03, v13, v23, v33);
#undef SF_HORN_FIX
    q0 += d0; q1 += d1; q2 += d2; q3 += d3;
    const double nq = sqrt(((q0 * q0 + q1 * q1) + q2 * q2) + q3 * q3);
    q0 /= nq; q1 /= nq; q2 /= nq; q3 /= nq;
    const double xx = q1 * q1, yy = q2 * q2, zz = q3 * q3, xy = q1 * q2, xz = q1 * q3, yz = q2 * q3;
    const double wx = q0 * q1, wy = q0 * q2, wz = q0 * q3;
    const double m0 = 1.0 - 2.0 * (yy + zz), m1 = 2.0 * (xy - wz), m2 = 2.0 * (xz + wy);
    const double m3 = 2.0 * (xy + wz), m4 = 1.0 - 2.0 * (xx + zz), m5 = 2.0 * (yz - wx);
    const double m6 = 2.0 * (xz - wy), m7 = 2.0 * (yz + wx), m8 = 1.0 - 2.0 * (xx + yy);
    // |q|^2 and the nine entries are each a few roundings off: R^T R - I comes to 7 .. 8 x 2^-52.  One Newton-Schulz step
    // R <- R - R E / 2 with E = R^T R - I summed exactly (dot3m1) leaves what the final rounding of nine doubles leaves.
    const double e00 = dot3m1(m0, m0, m3, m3, m6, m6, -1.0), e11 = dot3m1(m1, m1, m4, m4, m7, m7, -1.0);
    const double e22 = dot3m1(m2, m2, m5, m5, m8, m8, -1.0), e01 = dot3m1(m0, m1, m3, m4, m6, m7, 0.0);
    const double e02 = dot3m1(m0, m2, m3, m5, m6, m8, 0.0), e12 = dot3m1(m1, m2, m4, m5, m7, m8, 0.0);
    rot3 R;
    R.r0 = m0 - 0.5 * ((m0 * e00 + m1 * e01) + m2 * e02);
    R.r1 = m1 - 0.5 * ((m0 * e01 + m1 * e11) + m2 * e12);
    R.r2 = m2 - 0.5 * ((m0 * e02 + m1 * e12) + m2 * e22);
    R.r3 = m3 - 0.5 * ((m3 * e00 + m4 * e01) + m5 * e02);
    R.r4 = m4 - 0.5 * ((m3 * e01 + m4 * e11) + m5 * e12);
    R.r5 = m5 - 0.5 * ((m3 * e02 + m4 * e12) + m5 * e22);
    R.r6 = m6 - 0.5 * ((m6 * e00 + m7 * e01) + m8 * e02);
    R.r7 = m7 - 0.5 * ((m6 * e01 + m7 * e11) + m8 * e12);
    R.r8 = m8 - 0.5 * ((m6 * e02 + m7 * e12) + m8 * e22);
    R.gap = 0.5 * (l1 - l2);
    R.s1 = 0.5 * (l1 + l2);
    return R;
}
#undef SF_HORN_ROT

// The rigid motion of a Kabsch fit from its moments: mean = {abar, bbar}, H the centred cross-covariance (row-major) ->
// o = {R row-major, t = bbar - R abar}.  false, and o as it was, when the rotation is not unique (gap <= 1e-6 s1: H = 0, collinear
// points, non-finite input) or an entry is not finite (the sum of the twelve magnitudes is finite iff all of them are: no NaN and
// no infinity ever reaches the scoring).  The one rule of K11's draws and K15's seeds.
__host__ __device__ inline bool rigid_from_moments(const double (&mean)[6], const double (&H)[9], double (&o)[12])
{
    const rot3 R = kabsch_rotation(H[0], H[1], H[2], H[3], H[4], H[5], H[6], H[7], H[8]);
    const double t0 = mean[3] - ((R.r0 * mean[0] + R.r1 * mean[1]) + R.r2 * mean[2]);
    const double t1 = mean[4] - ((R.r3 * mean[0] + R.r4 * mean[1]) + R.r5 * mean[2]);
    const double t2 = mean[5] - ((R.r6 * mean[0] + R.r7 * mean[1]) + R.r8 * mean[2]);
    const double mag = (((fabs(R.r0) + fabs(R.r1)) + (fabs(R.r2) + fabs(R.r3))) + ((fabs(R.r4) + fabs(R.r5)) + (fabs(R.r6) + fabs(R.r7)))) +
                       ((fabs(R.r8) + fabs(t0)) + (fabs(t1) + fabs(t2)));
    if (!(R.gap > 1e-6 * R.s1 && mag <= SF_DBL_MAX)) return false;
    o[0] = R.r0; o[1] = R.r1; o[2] = R.r2; o[3] = R.r3; o[4] = R.r4; o[5] = R.r5; o[6] = R.r6; o[7] = R.r7; o[8] = R.r8;
    o[9] = t0; o[10] = t1; o[11] = t2;
    return true;
}

} // namespace sf_horn
