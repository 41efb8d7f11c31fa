// shot_core.h -- what the SHOT kernels share, one definition each: the azimuth octant, the root / inverse-root pair, the atan /
// acos polynomials and their coefficient table, the geometry and the interpolation weights of one neighbour, the slots of the
// election tables and their tagging, the rule for who writes what, the gather of a chunk, the prologue of the register-held
// forms, the keypoint pick, the row epilogue, and the constants a launch is given.  Shared by K5 (shot.hip: 11 cosine bins, the
// tuned forms) and the serial SHOT with any number of cosine bins (shot_bins.hip).
#pragma once
#include "common.h"
#include "device_util.h"

// K4's launches (normals_lrf.hip): raw != 0 leaves the raw axes for a fused K5; skip_zero: frames of the serial variant
int sf_launch_shot_lrf(sf_ctx *ctx, sf_cloud *c, sf_nbrs *nb, int raw, int skip_zero, double *dlrf);
int sf_launch_lrf_from_cov(sf_ctx *ctx, const double *cov_dev, int64_t m, double *dlrf);

namespace {

#define SHOT_PI 3.141592653589793

__device__ inline int azimuth_octant(double x, double y) // get_azimuth_idx, shot.py:51-70
{
    const bool a = (y > 0.0) || ((y == 0.0) && (x < 0.0));
    const bool b = ((x > 0.0) || ((x == 0.0) && (y > 0.0))) != a;
    const bool c = ((x * y > 0.0) || (x == 0.0)) ? (fabs(x) < fabs(y)) : (fabs(x) > fabs(y));
    return 4 * (int)a + 2 * (int)b + (int)c;
}

// The same function for a whole wave with the special cases (a zero coordinate, |x| = |y|, a product that underflows)
// moved behind a wave-uniform test: off them the three bits are two sign tests and one magnitude comparison.
__device__ inline int azimuth_octant_wave(double x, double y)
{
    const double ax = fabs(x), ay = fabs(y);
    const bool special = !(fmin(ax, ay) > 1e-150) || ax == ay; // (also catches NaN)
    if (__ballot(special)) return azimuth_octant(x, y);
    const bool a = y > 0.0, xp = x > 0.0, lt = ax < ay;
    return 4 * (int)a + 2 * (int)(xp != a) + (int)(xp == a ? lt : !lt);
}

// A resolved slot holds the NEGATED value (values are >= 0, so the sign bit marks it); an unresolved key is
// the bit pattern of rho > 0 and an empty slot is +0.  Decoding is therefore max(-x, 0): one instruction.
__device__ inline unsigned long long tag_value(double v)
{
    return (unsigned long long)__double_as_longlong(v) | 0x8000000000000000ull;
}

__device__ inline double sf_dot3(double a0, double a1, double a2, double b0, double b1, double b2)
{
    return __builtin_fma(a2, b2, __builtin_fma(a1, b1, a0 * b0));
}

// sqrt(x) and 1/sqrt(x) together.  The root is ocml's own f64 sequence (v_rsq_f64 and three coupled Newton steps)
// minus its exponent pre/post-scaling, which only matters outside [1e-290, 1e290]: bit-identical to sqrt() there
// (tools/ubench/sqrt_check.hip: 0 differences in 1.6e7 inputs), 10 instructions instead of 22; the half-inverse
// the iteration carries along, refined once more, is 1/sqrt(x) to ~1 ulp for two more instructions.
__device__ inline void sf_sqrt_rsqrt_newton(double x, double &root, double &inv)
{
    const double y = __builtin_amdgcn_rsq(x);
    double g = x * y, h = 0.5 * y;
    double r = __builtin_fma(-h, g, 0.5);
    g = __builtin_fma(g, r, g);
    h = __builtin_fma(h, r, h);
    double d = __builtin_fma(-g, g, x);
    g = __builtin_fma(d, h, g);
    d = __builtin_fma(-g, g, x);
    g = __builtin_fma(d, h, g);
    r = __builtin_fma(-h, g, 0.5);
    h = __builtin_fma(h, r, h);
    root = g;
    inv = h + h;
}
// 2^-964 <= x < 2^963, i.e. 4.6e-291 .. 7.8e289, positive, finite, not NaN, tested on the exponent: one integer subtraction and
// comparison with 32-bit literals instead of two comparisons against 64-bit constants that each cost two scalar moves
__device__ inline bool sf_sqrt_fast_range(unsigned hi) { return hi - 0x03b00000u < 0x7c200000u - 0x03b00000u; }

__device__ inline void sf_sqrt_rsqrt(double x, double &root, double &inv)
{
    sf_sqrt_rsqrt_newton(x, root, inv);
    if (__ballot(!sf_sqrt_fast_range((unsigned)__double2hiint(x)))) { // (wave-uniform, never taken for real clouds)
        root = sqrt(x);
        inv = 1.0 / root;
    }
}

// The same pair for a WAVE-UNIFORM argument (the squared norm of a row: a sum of squares of weights, each 0 or >= 1e-19, so
// either 0 or far inside the fast range): the range test is two scalar instructions on the exponent instead of two vector
// comparisons against 64-bit literals (six vector instructions with their moves).
__device__ inline void sf_sqrt_rsqrt_uniform(double x, double &root, double &inv)
{
    if (sf_sqrt_fast_range((unsigned)__builtin_amdgcn_readfirstlane(__double2hiint(x)))) {
        sf_sqrt_rsqrt_newton(x, root, inv);
    } else {
        root = sqrt(x);
        inv = 1.0 / root;
    }
}

// ---- the frame of a fused SHOT kernel ---------------------------------------------------------------------------------
// K4's raw mode leaves, in the frame's final row-major layout [x y z] per component, the largest / smallest eigenvectors as
// returned (x, z) and y = cross(z, x) of THOSE.  The fused kernels count the sign votes (shot.py:40-45) from the neighbours they
// have gathered anyway and flip: x and z by their own vote, y when exactly one of the two flipped (every product of the cross
// product changes sign, so the rounded difference does too; a component that cancelled to zero stays +0, as -a + a does).  All of
// it is wave-uniform: the nine numbers arrive by scalar loads and a flip is a scalar xor (y: plus one vector "+ 0").
// (sign: 0 or the sign bit as a 64-bit mask, one scalar select per axis -- pinned, or the compiler distributes the select over
// the components; a flip is then ONE 64-bit scalar xor per component)
__device__ inline double shot_flip(double v, unsigned long long sign) { return __longlong_as_double(__double_as_longlong(v) ^ (long long)sign); }
// raw: the nine raw numbers; E: the finished frame.  Returns whether anything changed (the caller writes E back if so).
__device__ inline bool shot_finish_frame(const double (&raw)[9], int k, int xneg, int zneg, double (&E)[9])
{
    // coordinates are finite (checked at upload), so "not < 0" is ">= 0": flip when strictly more neighbours project negative
    const bool fx = xneg > k - xneg, fz = zneg > k - zneg;
    if (k == 0) { // shot.py:24-25
        E[0] = 1.0; E[1] = 0.0; E[2] = 0.0; E[3] = 0.0; E[4] = 1.0; E[5] = 0.0; E[6] = 0.0; E[7] = 0.0; E[8] = 1.0;
        return true;
    }
    unsigned long long sx = fx ? 0x8000000000000000ull : 0ull, sz = fz ? 0x8000000000000000ull : 0ull;
    asm volatile("" : "+s"(sx), "+s"(sz));
    const unsigned long long sy = sx ^ sz;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        E[3 * i + 0] = shot_flip(raw[3 * i + 0], sx);
        // (-a + a is +0: a component of y that cancelled stays +0 when y flips -- what "flipped + 0.0" would do, as integer
        // operations on the scalar unit: the vector add put y's three components into six vector registers for the whole
        // kernel, the difference between five and six waves per SIMD for the fused four-chunk form)
        unsigned long long yb = (unsigned long long)__double_as_longlong(raw[3 * i + 1]) ^ sy;
        yb = (yb << 1) ? yb : 0ull;
        E[3 * i + 1] = __longlong_as_double((long long)yb);
        E[3 * i + 2] = shot_flip(raw[3 * i + 2], sz);
    }
    return fx | fz;
}

// Phase markers for tools/k5_phases.py (an ANALYSIS build only, -DSF_K5_MARK_BUILD: scheduling barriers + an assembler
// comment; the shipped build compiles them to nothing): instruction counts per phase of the register-cached K5.
#ifdef SF_K5_MARK_BUILD
#define SF_K5_MARK(id, nch)                                                     \
    do {                                                                        \
        __builtin_amdgcn_sched_barrier(0);                                      \
        asm volatile("; K5MARK %0 %1" ::"n"(id), "n"(nch));                     \
        __builtin_amdgcn_sched_barrier(0);                                      \
    } while (0)
// (pure arithmetic sinks to its first use whatever barrier stands between: the values a phase produces are pinned in front
// of the next mark)
#define SF_K5_PIN(x) asm volatile("" : "+v"(x))
#else
#define SF_K5_MARK(id, nch) do { } while (0)
#define SF_K5_PIN(x) (void)(x)
#endif
// ids: 1 header+clear, 2 gather, 3 frame votes, 4 gate, 5 geometry (sub: 50 sqrt/rsqrt, 51 local coords + cosine, 52 cosine bin,
// 53 octant, 54 centre-ray cross/dot + neighbour octant, 55 lz/rho + packing), 6 election A (atomic max), 7 who-writes-what
// (key reads), 8 weights (sub: 80 atan fraction, 81 radial shells, 82 acos, 83 elevation + sum), 9 A store (CAS), 10 S3/S4 S6/S7
// adds, 11 S1 S9 elections + adds, 12 read-back + normalise + store

struct shot_kept {
    double rho, dc, tcross, tdot, lzr; // tcross / tdot: (lx, ly) against the octant's centre ray; lzr = lz / rho
    unsigned bins0, bins1;            // base | bcos << 9 | bth << 18 ; bins1: bit 31 = valid, bits 28-30 = election flags
};

// ---- short double-precision helpers for sweep 2 (coefficients: tools/fit_poly.py) ------------------------
// The interpolation weights are continuous in theta / phi, so these only have to be accurate, not
// correctly rounded: each is within ~2e-16 (absolute) of the libm value the reference uses, far inside the
// 1e-5 parity tolerance, at a quarter of the instruction count of ocml's atan2 / acos / sqrt / division.
__device__ inline double sf_rcp(double d) { return sf_rcp_fast(d); } // v_rcp_f64 + 2 Newton steps, ~1 ulp

__device__ inline double sf_sqrt_small(double x) // sqrt(x), 0 <= x <= 1/4, no denormal / huge handling
{
    const double y = __builtin_amdgcn_rsq(x);
    double g = x * y, h = 0.5 * y;
    const double r = __builtin_fma(-h, g, 0.5);
    g = __builtin_fma(g, r, g);
    h = __builtin_fma(h, r, h);
    const double d = __builtin_fma(-g, g, x);
    g = __builtin_fma(d, h, g);
    return x > 0.0 ? g : 0.0;
}


// The two polynomials' coefficients live in device memory (a 26-double table the context owns, reached through a kernel argument)
// and arrive by scalar loads -- sixteen dwords per instruction -- right where they are used.  As immediates every coefficient
// costs two s_mov_b32 in front of its FMA (the instruction takes one scalar operand, and keeping 24 of them live across the
// kernel is 48 scalar registers the kernel does not have): 96 scalar moves per keypoint, a quarter of its scalar instructions,
// and the scalar stream is what holds the vector pipe back at seven waves per SIMD (tools/pmc_k5.sh: vector instructions
// 783 -> 701 per keypoint bought nothing until the scalar ones followed).  (A __constant__ array with an initialiser is folded
// back into immediates by the compiler.)
#define SF_K_ATAN 1.2732395447351628  // 4 / pi
#define SF_K_ACOS 0.6366197723675814  // 2 / pi
#define SF_ATAN_TERMS 11
#define SF_ACOS_TERMS 13
#define SF_ACOS_AT 12 // (offset of the second table: both start on a 32-byte boundary)
static const double SF_SHOT_COEF[SF_ACOS_AT + SF_ACOS_TERMS + 1] = {
    // atan(t) / t / (pi/4) in s = t^2, highest power first
    0.021102961440831885 * SF_K_ATAN, -0.04345403041920663 * SF_K_ATAN, 0.05687431322104835 * SF_K_ATAN, -0.06640058350060206 * SF_K_ATAN,
    0.07689933264608774 * SF_K_ATAN,  -0.09090771637100807 * SF_K_ATAN, 0.11111106118508882 * SF_K_ATAN, -0.14285714179450393 * SF_K_ATAN,
    0.19999999998836118 * SF_K_ATAN,  -0.33333333333328347 * SF_K_ATAN, SF_K_ATAN, 0.0,
    // asin(r) / r / (pi/2) in s = r^2, highest power first
    0.028169218060881414 * SF_K_ACOS, -0.010749050339697808 * SF_K_ACOS, 0.01603551434914882 * SF_K_ACOS, 0.0078029494773533175 * SF_K_ACOS,
    0.011875494382636922 * SF_K_ACOS, 0.013929652902326633 * SF_K_ACOS,  0.017355259955786323 * SF_K_ACOS, 0.02237204763174451 * SF_K_ACOS,
    0.03038194736709848 * SF_K_ACOS,  0.044642857103423646 * SF_K_ACOS,  0.07500000000020764 * SF_K_ACOS,  0.1666666666666665 * SF_K_ACOS,
    SF_K_ACOS, 0.0};

// atan(t) / (pi/4) for 0 <= t <= tan(pi/8) (1 + 1e-3): the minimax polynomial of tools/fit_poly.py with 4/pi folded into its
// coefficients at compile time -- the azimuth weight is |dth| = angle / (pi/4), so the angle itself is never needed
// (passing a loaded coefficient through an empty asm with a scalar-register constraint keeps it the FMA's scalar operand; left
// alone the compiler selects the accumulate form v_fmac_f64, whose addend is the destination: two v_mov_b32 per coefficient)
__device__ inline double sf_scalar_operand(double c)
{
    asm("" : "+s"(c));
    return c;
}
typedef const __attribute__((address_space(4))) double *sf_const_doubles; // (read through the scalar cache: never written by a kernel)
__device__ inline double sf_atan_octant_fraction(double t, const double *__restrict__ coef_)
{
    sf_const_doubles coef = (sf_const_doubles)coef_;
    const double s = t * t;
    double p = coef[0];
#pragma unroll
    for (int i = 1; i < SF_ATAN_TERMS; ++i) p = __builtin_fma(p, s, sf_scalar_operand(coef[i]));
    return t * p;
}

// acos(|z|) / (pi/2) for |z| <= 1 (result in [0, 1]; |z| = 0 gives exactly 1, |z| = 1 exactly 0): the asin-form minimax
// polynomial with 2/pi folded into its coefficients.  The elevation weights are linear in phi / (pi/2) and symmetric about
// the equator -- acos(-z) = pi - acos(z) -- so the angle of |z| is all they need (shot_weights).
__device__ inline double sf_acos_abs_quadrants(double az, const double *__restrict__ coef_)
{
    sf_const_doubles coef = (sf_const_doubles)coef_;
    const bool big = az > 0.5;
    const double xb = __builtin_fma(-0.5, az, 0.5), xs = az * az; // (1 - |z|) / 2 is exact
    const double rb = sf_sqrt_small(fmin(xb, 0.25));
    const double x = big ? xb : xs;
    const double r = big ? rb : az;
    double p = coef[SF_ACOS_AT]; // asin(r) = r + r s R(s), s = r^2 <= 1/4
#pragma unroll
    for (int i = 1; i < SF_ACOS_TERMS; ++i) p = __builtin_fma(p, x, sf_scalar_operand(coef[SF_ACOS_AT + i]));
    const double as = r * p; // asin(r) / (pi/2)
    // |z| <= 1/2: 1 - as ;  |z| > 1/2: 2 as
    return big ? as + as : 1.0 - as;
}
// Radius-derived constants of the interpolation, computed once on the host (as kernel arguments they live in SGPRs;
// computed in the kernel the wave-uniform division 1 / (r/2) was a 14-instruction vector sequence per chunk)
struct shot_consts {
    double radius, half_r, q1, q3, inv_hr;
    const double *coef; // SF_SHOT_COEF in device memory
};

// The interpolation weights of one neighbour (shot.py:73-171, 244-298), reduced to what the elections consume:
//   vA   = S2 + S5 + S8 + S10 = (1 - |dc|) + current radial + current elevation + (1 - |dth|)
//   v_cd = S3's `outer` if the neighbour is in the inner shell, S4's `inner` if in the outer one (the other is 0)
//   v_ef = S6's `upper` if it is in the lower half space, S7's `lower` if in the upper one (the other is 0)
//   adth = |dth| (S9's value; S1's is |dc|, already in g)
// Written so that only the shell / half-space the neighbour is actually in gets evaluated: the centre of ITS bin is
// selected first, the distance to that centre computed once.  theta and phi enter as fractions of their bin size
// (sf_atan_octant_fraction, sf_acos_quadrants).  All weights are continuous in rho / phi / theta except at
// rho = r/2 (decided on rho itself, as the reference does) and phi = pi/2 (decided by the sign of z inside the
// reference's 1e-10 band), so last-bit differences of the short polynomial forms cannot flip a term.
__device__ inline void shot_weights(const shot_kept &g, const shot_consts &k, double &vA, double &v_cd, double &v_ef, double &adth)
{
    const bool z_pos = g.bins1 & 2u; // lz > 0, decided in shot_geometry
    const double rho = g.rho;
    const double adc = fabs(g.dc);
    // |dth|: angle off the octant's centre ray as a fraction of the octant, clipped to 1/2.  lx = ly = 0 has dot = 0:
    // the reference's atan2(0, 0) = 0 sits 3.5 octants from octant 0's start -> 1/2.
    SF_K5_MARK(80, 0);
    const bool fwd = g.tdot > 0.0;
    const double tq = fmin(fabs(g.tcross) * sf_rcp(fwd ? g.tdot : 1.0), 0.4146);
    const double at = fmin(sf_atan_octant_fraction(tq, k.coef), 0.5);
    adth = fwd ? at : 0.5;
    SF_K5_PIN(adth);
    // radial shells (interpolate_on_adjacent_husks): rho == r/2 belongs to neither and gets all three terms zero
    // The two shells mirror each other about rho = r/2: with s = |rho - r/2| the distance to the current shell's centre
    // is |s - r/4| and the distance "towards the other shell" (3r/4 - rho outside, rho - r/4 inside) is r/4 - s, in both.
    SF_K5_MARK(81, 0);
    const bool off_half = rho != k.half_r;
    const double ds = fabs(rho - k.half_r) - k.q1;
    const double cur = off_half ? 1.0 - fabs(ds) * k.inv_hr : 0.0;
    v_cd = off_half ? fmax(-ds, 0.0) * k.inv_hr : 0.0;
    { double curp = cur; SF_K5_PIN(curp); SF_K5_PIN(v_cd); }
    // elevation (interpolate_vertical_volumes).  With u = phi / (pi/2) the reference's terms are
    //   current = 1 - |u - 1/2| for phi < pi/2, 1 - |u - 3/2| for phi >= pi/2;
    //   lower  = [phi < pi/2 and (not near or z > 0) and phi >= pi/4] (u - 1/2), counted for z > 0 writers;
    //   upper  = [(phi > pi/2 or (near and z <= 0)) and phi <= 3pi/4] (3/2 - u), counted for z <= 0 writers
    // (near: |phi - pi/2| < 1e-10).  phi = acos(z) is symmetric about the equator, u(-z) = 2 - u(z), so in terms of
    // t = acos(|z|) / (pi/2) in [0, 1] all three are ONE expression per neighbour whatever the sign of z:
    //   current = 1 - |t - 1/2| ;  lower resp. upper = max(t - 1/2, 0), with the single exception the masks leave:
    //   a writer with z > 0 whose phi ROUNDS to pi/2 (t = 1 exactly) fails "phi < pi/2" and gets 0.
    SF_K5_MARK(82, 0);
    double t = sf_acos_abs_quadrants(fmin(fabs(g.lzr), 1.0), k.coef);
    SF_K5_PIN(t);
    SF_K5_MARK(83, 0);
    const double curv = 1.0 - fabs(t - 0.5);
    const bool side = !z_pos | (t < 1.0);
    v_ef = side ? fmax(t - 0.5, 0.0) : 0.0;
    vA = (((1.0 - adc) + cur) + curv) + (1.0 - adth);
}

// The waves of a K5 workgroup are independent (one keypoint and one LDS region each): what orders a wave's LDS phases is
// the in-order execution of its own LDS instructions, so the "barrier" is a compiler fence, never an s_barrier.
#define SF_SHOT_SYNC()                                                                                               \
    do {                                                                                                            \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");                                                      \
        __builtin_amdgcn_wave_barrier();                                                                            \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");                                                      \
    } while (0)

__device__ inline double shot_untag(unsigned long long x) { return fmax(-__longlong_as_double((long long)x), 0.0); }

// ---- the pieces every body of K5 shares: k_shot_cached, k_shot_team, k_shot_long (shot.hip), k_shot_bins (shot_bins.hip) ------
// N, where it appears: the number of cosine bins at compile time (11: the tuned forms), 0: a run-time value (k_shot_bins).

// The three slots of a neighbour -- its own bin (A: S2+S5+S8+S10), the neighbouring cosine bin (B: S1), the neighbouring octant
// (G: S9) -- in shot_kept.  11 bins: three 9-bit fields of bins0, bins1 = valid << 31 | (base & 3).  Any count (rows of up to
// 2 048 slots): bins0 = base | bcos << 16, bins1 = valid << 31 | bth << 2 | (base & 3).  Bits 0-1 of bins1, shell and half-space,
// are what shot_weights reads.
template <int N> __device__ inline void shot_pack(unsigned base, unsigned bcos, unsigned bth, shot_kept &o)
{
    o.bins0 = N ? base | (bcos << 9) | (bth << 18) : base | (bcos << 16);
    o.bins1 = 0x80000000u | (N ? 0u : bth << 2) | (base & 3u);
}
template <int N> __device__ inline unsigned shot_slot_a(const shot_kept &g) { return N ? g.bins0 & 511u : g.bins0 & 0xffffu; }
template <int N> __device__ inline unsigned shot_slot_b(const shot_kept &g) { return N ? (g.bins0 >> 9) & 511u : g.bins0 >> 16; }
template <int N> __device__ inline unsigned shot_slot_g(const shot_kept &g) { return N ? (g.bins0 >> 18) & 511u : (g.bins1 >> 2) & 0xfffu; }
__device__ inline unsigned long long shot_key(const shot_kept &g) { return (unsigned long long)__double_as_longlong(g.rho); }

// The geometry of one neighbour at non-zero distance: the five numbers shot_weights needs and its three slots.  With a run-time
// bin count (n, nd = (double)n) it returns false for a neighbour whose cosine bin is n (a clipped cosine of exactly +1 with n
// even: rint(n - 0.5) = n, the reference's IndexError), which then takes part in nothing; with 11 bins that cannot happen.
// The azimuth-neighbour decision uses the sign of the cross product with the octant's centre direction (no atan2); when that is
// not clearly non-zero it falls back to the reference's own expression, so the decision equals shot.py:283-288 in every case.
template <int N>
__device__ inline bool shot_geometry(double cx, double cy, double cz, double d2, double nx, double ny, double nz, const double *E,
                                     double half_r, int n_, double nd_, shot_kept &o)
{
    const int n = N ? N : n_;
    const double nd = N ? (double)N : nd_;
    double rho, inv_rho;
    SF_K5_MARK(50, 0);
    sf_sqrt_rsqrt(d2, rho, inv_rho);
    SF_K5_PIN(rho); SF_K5_PIN(inv_rho);
    SF_K5_MARK(51, 0);
    // (neighbors - point) @ eigenvectors and normals @ eigenvectors[:, 2] (shot.py:214-215) as the multiply-add chain an
    // FMA BLAS kernel runs over the inner index -- what the reference's NumPy does on any current x86 / OpenBLAS
    const double lx = sf_dot3(cx, cy, cz, E[0], E[3], E[6]);
    const double ly = sf_dot3(cx, cy, cz, E[1], E[4], E[7]);
    const double lz = sf_dot3(cx, cy, cz, E[2], E[5], E[8]);
    double cosine = sf_dot3(nx, ny, nz, E[2], E[5], E[8]);
    cosine = fmin(fmax(cosine, -1.0), 1.0);
    double lxp = lx, lyp = ly, lzp = lz;
    SF_K5_PIN(lxp); SF_K5_PIN(lyp); SF_K5_PIN(lzp); SF_K5_PIN(cosine);
    SF_K5_MARK(52, 0);
    // bin_dist = (cosine + 1.0) * n / 2.0 - 0.5 in that order, unfused (shot.py:386); rint rounds half to even (:387)
    const double cpos = (cosine + 1.0) * nd / 2.0 - 0.5;
    const double cf = rint(cpos);
    int ci = (int)cf; // 0 .. n (-0.5 rounds to -0)
    if (!N && ci >= n) return false;
    double dcp = cpos - cf;
    SF_K5_PIN(ci); SF_K5_PIN(dcp);
    SF_K5_MARK(53, 0);
    int ti = azimuth_octant_wave(lx, ly);
    SF_K5_PIN(ti);
    SF_K5_MARK(54, 0);
    const int pi_ = lz > 0.0 ? 1 : 0;
    const int ri = rho > half_r ? 1 : 0; // (radius / 2 is exact: the host passes that very double)
    const double dc = cpos - cf;
    const int sc = (dc > 0.0) - (dc < 0.0);
    int cin = ci + sc; // -1 .. n, wrapped as the reference's % n does (shot.py:401): n = 1 wraps onto itself
    cin = cin < 0 ? n - 1 : (cin >= n ? 0 : cin);
    // Offset from the octant's centre ray, in the octant's own frame: with a >= b the larger / smaller of |lx|, |ly|, the
    // point sits atan(b / a) in [0, pi/4] off the nearest axis and the centre ray pi/8 off it, so rotating (a, b) by
    // -pi/8 gives cross' / dot' = tan(angle off the centre).  Whether theta grows or shrinks with that angle alternates
    // from octant to octant (even octants: grows).
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
    {
        double crp = cross, dtp = dot;
        unsigned b0p = base, b1p = bcos, b2p = bth;
        SF_K5_PIN(crp); SF_K5_PIN(dtp); SF_K5_PIN(b0p); SF_K5_PIN(b1p); SF_K5_PIN(b2p);
    }
    SF_K5_MARK(55, 0);
    // lz / rho through the reciprocal, then one residual correction: acos has an unbounded derivative at +-1, so for a
    // neighbour on the frame's z axis a one-ulp error of the quotient would be a 1.5e-8 error of phi (the reference's
    // correctly rounded division gives exactly +-1 there)
    double lzr = lz * inv_rho;
    lzr = __builtin_fma(__builtin_fma(-lzr, rho, lz), inv_rho, lzr);
    o.rho = rho; o.dc = dc; o.tcross = cross; o.tdot = dot; o.lzr = lzr;
    shot_pack<N>(base, bcos, bth, o);
    return true;
}

// Who writes what, from the A keys read back after the election: the neighbour's own, the one of the other radial shell
// (slot ^ 1) and of the other half-space (slot ^ 2).  The winner of A (own == key) also writes S3/S4 when it is the farthest of
// its cell over BOTH shells -- every rho of the outer shell (odd) exceeds every rho of the inner one -- and S6/S7 when it is the
// farther of the two half-spaces' winners.  Equal distances there are a tie like any other (the larger caller index writes
// last): the body that sees `key == other_half` reports the keypoint and k_shot_tied computes the row, so what this rule
// answers on equality (z > 0) never reaches a caller.  The forms that hold their neighbours in registers keep the answers as
// flags of bins1, the streamed forms ask where they add.
__device__ inline bool shot_writes_cd(bool odd, unsigned long long other_shell) { return odd || other_shell == 0ull; }
__device__ inline bool shot_writes_ef(unsigned long long key, unsigned long long other_half, bool up)
{
    return key > other_half || (key == other_half && up);
}

// One chunk of a list: entry t of the k entries at `list` (NT: read past the caches, SF_LIST_LOAD), its record, its offset from
// the keypoint and its normal.  A lane past the end carries point 0's offset and returns false.
template <bool NT> __device__ inline int shot_list_entry(const int32_t *__restrict__ list, int t, int k)
{
    return t < k ? (NT ? SF_LIST_LOAD(list + t) : list[t]) : -1;
}
__device__ inline bool shot_gather_entry(const double *__restrict__ rec, int j, double px, double py, double pz, double &cx,
                                         double &cy, double &cz, double &nx, double &ny, double &nz)
{
    double x, y, z;
    sf_load_pn(rec, j < 0 ? 0 : j, x, y, z, nx, ny, nz);
    cx = x - px;
    cy = y - py;
    cz = z - pz;
    return j >= 0;
}
template <bool NT>
__device__ inline bool shot_gather64(const double *__restrict__ rec, const int32_t *__restrict__ list, int t, int k, double px,
                                     double py, double pz, double &cx, double &cy, double &cz, double &nx, double &ny, double &nz)
{
    return shot_gather_entry(rec, shot_list_entry<NT>(list, t, k), px, py, pz, cx, cy, cz, nx, ny, nz);
}

// One step of a streamed sweep: 128 neighbours gathered together, their geometry.  bins1 bit 31 marks a neighbour at non-zero
// distance whose bins are in range; pos: the lanes at non-zero distance, over: those of them in cosine bin n (N = 0 only).
template <int N, bool NT>
__device__ inline void shot_geometry128(const double *__restrict__ rec, const int32_t *__restrict__ list, int t0, int k, int lane,
                                        double px, double py, double pz, const double *E, double half_r, int n, double nd,
                                        shot_kept (&g)[2], unsigned long long (&pos)[2], unsigned long long (&over)[2])
{
    double cx[2], cy[2], cz[2], nx[2], ny[2], nz[2];
    int jj[2];
    bool on[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) jj[u] = shot_list_entry<NT>(list, t0 + 64 * u + lane, k); // (both indices requested before a record)
#pragma unroll
    for (int u = 0; u < 2; ++u) on[u] = shot_gather_entry(rec, jj[u], px, py, pz, cx[u], cy[u], cz[u], nx[u], ny[u], nz[u]);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        g[u].bins1 = 0u;
        const double d2 = (cx[u] * cx[u] + cy[u] * cy[u]) + cz[u] * cz[u];
        const bool at = on[u] && d2 > 0.0;
        bool bad = false;
        if (at) bad = !shot_geometry<N>(cx[u], cy[u], cz[u], d2, nx[u], ny[u], nz[u], E, half_r, n, nd, g[u]);
        pos[u] = __ballot(at);
        over[u] = __ballot(bad);
    }
}

// ---- the prologue of the forms that hold their chunks in registers (cached, team) ----
// the lanes of a chunk that hold one of the `rem` entries left, as a wave-uniform mask: votes and gate are mask arithmetic on
// the scalar unit (a ballot of a bare comparison is the comparison's own result register)
__device__ inline unsigned long long shot_chunk_mask(int rem) { return rem >= 64 ? ~0ull : (rem > 0 ? (1ull << rem) - 1ull : 0ull); }

// the sign votes of a chunk (shot.py:40-45): the neighbours that project negative on the raw x and z axes (the query itself
// votes ">= 0", as in the reference)
__device__ inline void shot_count_votes(double cx, double cy, double cz, const double (&raw)[9], unsigned long long onm, int &xneg,
                                        int &zneg)
{
    const double xo = sf_dot3(cx, cy, cz, raw[0], raw[3], raw[6]);
    const double zo = sf_dot3(cx, cy, cz, raw[2], raw[5], raw[8]);
    xneg += __popcll(__ballot(xo < 0.0) & onm);
    zneg += __popcll(__ballot(zo < 0.0) & onm);
}

// the gate of a chunk (shot.py:212): its neighbours at non-zero distance, as a mask (padding lanes carry point 0's offset: masked)
__device__ inline void shot_gate(double cx, double cy, double cz, unsigned long long onm, double &d2, unsigned long long &posm,
                                 int &npos)
{
    d2 = (cx * cx + cy * cy) + cz * cz;
    posm = __ballot(d2 > 0.0) & onm;
    npos += __popcll(posm);
}

// The keypoint of a wave (a team) of a launch over a selection `sel` (sf_dispatch::mid_sel / tail_sel, owner numbering) or over
// all m: false when it has none.
__device__ inline bool shot_pick_keypoint(int64_t &q, bool selected, const int32_t *__restrict__ sel, int64_t nsel,
                                          int64_t view_first, int64_t m)
{
    if (selected) {
        if (q >= nsel) return false;
        q = (int64_t)sf_uniform(sel[q]) - view_first;
        if (q < 0) return false;
    }
    return q < m;
}

// The scale of a row from its lanes' partial sums of squares (shot.py:301-305): 1 / norm when normalising, 1 otherwise, 0 for a
// row of zeros.  negated: for a row held as MINUS its values (the cached form's accumulator), minus that -- with "x * scale + 0"
// an empty slot then comes out +0 whatever the sign of the scale.  (The short root / inverse-root pair: ~1 ulp each, a third of
// sqrt() followed by a division.)
__device__ inline double shot_row_scale(double ss, int normalize, bool negated)
{
    double nrm, inv_nrm;
    sf_sqrt_rsqrt_uniform(sf_wave_sum(ss), nrm, inv_nrm);
    return nrm > 0.0 ? (normalize ? (negated ? -inv_nrm : inv_nrm) : (negated ? -1.0 : 1.0)) : (negated ? -0.0 : 0.0);
}

// ---- neighbours at EQUAL distance -----------------------------------------------------------------------------------------
// The contract: the ten statements see the neighbours at non-zero distance in ONE total order -- ascending rho,
// and among bit-equal rho ascending index in the caller's cloud array -- so the last writer of a bin is the farthest neighbour
// and, among equally far ones, the one with the largest caller index, in all ten statements alike.  The elections of the four
// bodies above compare rho alone; two holders of a winning key are told apart by whoever reaches the slot first.  So every body
// NOTICES such a meeting where it costs nothing -- the compare-and-swap or claim of a holder that finds the slot taken by another
// holder of its own key, and the comparison of the two half-spaces' winners that comes out equal -- and reports the keypoint
// (shot_report_tie); its row is then computed again by k_shot_tied, which holds the full order (rho, caller index) in every
// election.  A list without such a meeting takes the same instructions as before plus the tests of a wave-uniform flag; a list
// with one is walked nine more times by one wave (three tables, three sweeps each): what a tie costs.
// Which rows are computed again depends on the list alone (a tie either stands in it or does not), not on who won the race.
// (one pointer: the count, then the list -- every register a launch argument holds to the kernel's end is one the register-cached
// forms do not have; the list has room for the call's m keypoints, and a keypoint is reported at most once)
struct shot_ties {
    int32_t *buf; // [0]: how many keypoints were reported; [1 + i]: the i-th of them (processing slot)
};
__device__ inline unsigned long long shot_claimed(unsigned long long key) { return key | 0x8000000000000000ull; }
// (one lane of the wave -- of the team -- that served keypoint q calls this once)
__device__ inline void shot_report_tie(const shot_ties &T, int64_t q)
{
    T.buf[1 + atomicAdd(T.buf, 1)] = (int32_t)q;
}

// Rows of the reported keypoints under the full order.  One wave per keypoint, the list streamed 128 neighbours at a time, per
// table T = A (S2+S5+S8+S10, and S3/S4, S6/S7 off it), B (S1), G (S9) three sweeps: (a) the largest rho of every slot, (b) among
// the holders of that rho the largest caller index (perm[] of the cell-sorted position), (c) the one neighbour that holds both
// claims the slot (a bit: a list that was imported may name a point twice, both entries carry equal values) and writes.  S3/S4
// and S6/S7 go to vx as in the team form; between the half-spaces the pair (rho, index) decides.  The row is ((A + vx) + B) + G
// per bin in that order, whatever the order of the list: bit-identical however the keypoint is served.
// LDS per wave, S = 32 n slots: key (8 B), row (8 B), vx (8 B), top (4 B) per slot, S / 32 claim words.
// N: 11, or 0 for a run-time count n.  fused: the frames at `lrf` were written by a fused body, which leaves a frame that no vote
// flipped as K4 stored it and reads a y component of -0 as +0 (shot_finish_frame).
__host__ __device__ inline size_t shot_tied_words(int n) { return (size_t)112 * n + (size_t)((n + 1) >> 1); } // 8-byte words
template <int N>
__global__ __launch_bounds__(256) void k_shot_tied(const double *__restrict__ rec, const int32_t *__restrict__ perm,
                                                   const double *__restrict__ qx, const double *__restrict__ qy,
                                                   const double *__restrict__ qz, const int64_t *__restrict__ offset,
                                                   const int32_t *__restrict__ cnt, const int32_t *__restrict__ idx,
                                                   const int32_t *__restrict__ qrow, int64_t m, shot_consts K,
                                                   const double *__restrict__ lrf, int fused, int n_, int normalize,
                                                   double *__restrict__ out, shot_ties T)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long shot_tied_lds[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nw = blockDim.x >> 6;
    const int n = N ? N : n_;
    const double nd = (double)n;
    const int S = 32 * n;
    unsigned long long *const key = shot_tied_lds + shot_tied_words(n) * wave;
    double *const rowv = reinterpret_cast<double *>(key + S);
    double *const vx = rowv + S;
    unsigned *const top = reinterpret_cast<unsigned *>(vx + S);
    unsigned *const claim = top + S;
    int64_t nt = sf_uniform(T.buf[0]);
    nt = nt < m ? nt : m; // (one entry per keypoint at most: never more than m)
    for (int64_t t = (int64_t)blockIdx.x * nw + wave; t < nt; t += (int64_t)gridDim.x * nw) {
        const int64_t q = sf_uniform(T.buf[1 + t]);
        if (q < 0 || q >= m) continue;
        const int64_t s = offset[q];
        const int k = sf_uniform(cnt[q]);
        const int64_t row = qrow ? qrow[q] : q;
        double *o = out + (int64_t)S * row;
        const double px = qx[q], py = qy[q], pz = qz[q];
        double E[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) E[i] = lrf[9 * row + i];
        if (fused) {
#pragma unroll
            for (int i = 0; i < 3; ++i) E[3 * i + 1] = E[3 * i + 1] == 0.0 ? 0.0 : E[3 * i + 1];
        }
        for (int b = lane; b < 2 * S; b += 64) rowv[b] = 0.0; // (row and vx)
        // one sweep: f(geometry, caller index + 1) for every neighbour at non-zero distance whose bins are in range
        auto sweep = [&](auto f) {
            for (int t0 = 0; t0 < k; t0 += 128) {
                shot_kept g[2];
                unsigned long long pos[2], over[2];
                shot_geometry128<N, false>(rec, idx + s, t0, k, lane, px, py, pz, E, K.half_r, n, nd, g, pos, over);
#pragma unroll
                for (int u = 0; u < 2; ++u)
                    if (g[u].bins1 >> 31) f(g[u], (unsigned)perm[idx[s + t0 + 64 * u + lane]] + 1u);
            }
        };
        for (int table = 0; table < 3; ++table) {
            auto slot_of = [&](const shot_kept &g) {
                return table == 0 ? shot_slot_a<N>(g) : (table == 1 ? shot_slot_b<N>(g) : shot_slot_g<N>(g));
            };
            for (int b = lane; b < S; b += 64) { key[b] = 0ull; top[b] = 0u; }
            for (int b = lane; b < n; b += 64) claim[b] = 0u;
            SF_SHOT_SYNC();
            sweep([&](const shot_kept &g, unsigned me) { atomicMax(&key[slot_of(g)], shot_key(g)); });
            SF_SHOT_SYNC();
            sweep([&](const shot_kept &g, unsigned me) {
                const unsigned i = slot_of(g);
                if (key[i] == shot_key(g)) atomicMax(&top[i], me);
            });
            SF_SHOT_SYNC();
            sweep([&](const shot_kept &g, unsigned me) {
                const unsigned i = slot_of(g);
                const unsigned long long mine = shot_key(g);
                if (key[i] != mine || top[i] != me) return;
                const unsigned bit = 1u << (i & 31u);
                if (atomicOr(&claim[i >> 5], bit) & bit) return; // (the same point named twice)
                double vA, v_cd, v_ef, adth;
                shot_weights(g, K, vA, v_cd, v_ef, adth);
                if (table == 0) { // (bit 1 of a slot: z > 0, bit 0: outer shell)
                    rowv[i] = vA;
                    const unsigned long long other_half = key[i ^ 2u];
                    const bool far = mine > other_half || (mine == other_half && me > top[i ^ 2u]);
                    if (shot_writes_cd(i & 1u, key[i ^ 1u]) && v_cd != 0.0) unsafeAtomicAdd(&vx[i ^ 1u], v_cd);
                    if (far && v_ef != 0.0) unsafeAtomicAdd(&vx[i ^ 2u], v_ef);
                } else {
                    const double v = table == 1 ? fabs(g.dc) : adth;
                    if (v != 0.0) rowv[i] += v; // (one writer per slot)
                }
            });
            SF_SHOT_SYNC();
            if (table == 0) {
                for (int b = lane; b < S; b += 64) rowv[b] += vx[b];
                SF_SHOT_SYNC();
            }
        }
        double ss = 0.0;
        for (int b = lane; b < S; b += 64) ss += rowv[b] * rowv[b];
        const double scale = shot_row_scale(ss, normalize, false);
        for (int b = lane; b < S; b += 64) sf_store_stream(o + b, rowv[b] * scale);
        SF_SHOT_SYNC();
    }
}

// ---- host: what every K5 launch is given ----
// The radius-derived constants as the reference's own expressions (shot.py:95-117, 235), the polynomial coefficients (uploaded
// once per context), and min_nb clamped into [-1, 2^31 - 1]: a list holds fewer than 2^31 points, so "more than min_nb
// neighbours" is a 32-bit comparison in the kernels.
static inline int sf_shot_consts(sf_ctx *ctx, double r_, int64_t min_nb, shot_consts *K, int *min_nb32)
{
    if (!ctx->shot_coef) {
        SF_HIP(hipMalloc(&ctx->shot_coef, sizeof(SF_SHOT_COEF)));
        SF_HIP(hipMemcpy(ctx->shot_coef, SF_SHOT_COEF, sizeof(SF_SHOT_COEF), hipMemcpyHostToDevice));
    }
    *K = shot_consts{r_, r_ / 2, r_ / 4, r_ * 3 / 4, 1.0 / (r_ / 2), ctx->shot_coef};
    *min_nb32 = (int)std::min<int64_t>(std::max<int64_t>(min_nb, -1), 2147483647LL);
    return SF_OK;
}

// The report list of one call's K5 launches (m entries and the counter, zeroed), and the launch that computes the reported rows
// again (k_shot_tied; n: cosine bins at run time when N = 0).  The launch is unconditional -- the count stays on the device --
// and small: its waves walk the report list in strides and end at once when it is empty.
static inline int sf_shot_ties_begin(sf_ctx *ctx, sf_pool_guard &guard, int64_t m, shot_ties *T)
{
    SF_CHECK(guard.alloc(&T->buf, (size_t)m + 1));
    SF_HIP(hipMemsetAsync(T->buf, 0, sizeof(int32_t), ctx->stream));
    return SF_OK;
}
template <int N>
static inline int sf_shot_ties_finish(sf_ctx *ctx, sf_cloud *c, sf_nbrs *nb, const shot_consts &K, const double *dlrf, bool fused,
                                      int n, int normalize, double *dout, const shot_ties &T)
{
    const int w = n <= 16 ? 4 : (n <= 32 ? 2 : 1); // waves per workgroup: at most 57.6 KB of LDS
    const size_t lds = (size_t)w * shot_tied_words(n) * sizeof(unsigned long long);
    const int64_t blocks = std::min<int64_t>(sf_div_up(nb->m, w), 1024);
    sf_launch_timer t_(ctx, "k5_shot_ties");
    hipLaunchKernelGGL(k_shot_tied<N>, dim3((unsigned)blocks), dim3(64 * w), lds, ctx->stream, c->rec, (const int32_t *)c->perm, nb->qx,
                       nb->qy, nb->qz, nb->offset, nb->count, nb->idx, nb->qrow, nb->m, K, dlrf, (int)fused, n, normalize, dout, T);
    SF_HIP(hipGetLastError());
    return SF_OK;
}

} // namespace
