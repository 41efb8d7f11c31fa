// fpfh_mc.h -- K7 on the int8 matrix cores, as device functions: the pieces its forms share, each defined once, and the four
// bodies the kernels of fpfh.hip call (k_fpfh_mc, k_fpfh_mc_sparse, k_fpfh_mcl).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_util.h"

// --------------------------------------------------------------------------------------------------
// K7 on the matrix cores (uint8 table: at most 128 bins).
//
// fpfh[q][b] - spfh[q][b] = (1/k_q) sum_j w_j c_jb is, per keypoint, the product of a 1 x k row of weights with
// the k x 128 matrix of its neighbours' integer bin counts.  Done on the vector ALU it costs three instructions
// per count (extract, convert, FMA).  Here the weights are turned into 62-bit fixed point (scaled by the
// keypoint's largest weight) and cut into eight signed-byte limbs, and  R[limb][bin] = sum_j limb_j * (c_jb - 128)  is
// accumulated EXACTLY in int32 by v_mfma_i32_16x16x64_i8: A = limbs x 64 neighbours, B = 64 neighbours x 16 bins,
// the counts going from the table to the matrix unit as the bytes they are (the table stores count ^ 128, which
// read as int8 is count - 128; a padding bin holds -128, so its column is -128 * sum_j limb_j and cancels the bias).
// The sums are recombined in float64 once per keypoint:  sum_j w_j c_jb = 2^-S sum_i 2^(8i) (R[i][b] - R[i][pad]).
// The only rounding is in the fixed-point weights (2^-61 of the largest one) and in that final recombination.
//
// One wave per keypoint, 32 neighbours per step (v_mfma_i32_16x16x32_i8).  Layouts (tools/ubench: probed on the
// device): operand lane l holds row / column l % 16 and the 8 consecutive k of block l / 16, one per byte; the result
// lane holds column l % 16 and rows 4 (l / 16) .. + 3.  Per step the 32 rows (128 B each) reach LDS by LDS-DMA; the B
// operand of the MFMA for bins 16 bb .. 16 bb + 15 -- lane (a, kb): bin 16 bb + a of neighbours 8 kb .. 8 kb + 7, one
// per byte -- is exactly what ONE transposing read (ds_read_b64_tr_b8: 8 rows x 16 bytes per 16-lane group,
// delivered column-major) returns, so no byte shuffling is left to the vector pipe.
//
// Four bodies, one arithmetic: fpfh_mc_body (whole rows) and fpfh_mc_body_sparse (at most two live 16-bin blocks) hold a list of
// at most 255 points in registers, fpfh_mcl_body and fpfh_mcl_body_sparse walk a longer one twice.  A body keeps to itself its
// SCHEDULE -- which steps are requested up front, which vmcnt it waits on, where the limbs are written, one pass or two, the
// integer limb pairs of the short forms against the float64 ones of the long forms, own / k through the reciprocal or by
// division -- and the pieces of text that cost registers or lengthened an MFMA block as functions (profiles/k7_family_isa.md): its
// keypoint prologue (the own-count loads must stay in front of the first DMA statement, whose "memory" clobber pins them), its
// lane map, the loop of a whole-row step with its padding column, and in fpfh_mc_body the row epilogue.  Everything else is one of the functions below, and the rows of the four
// forms are equal bit for bit because of it: the additions of each recombination are ordered in ONE place.
// --------------------------------------------------------------------------------------------------
typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v2i_t __attribute__((ext_vector_type(2)));
typedef __amdgpu_buffer_rsrc_t fpfh_mc_rsrc_t;
#ifndef SF_MC_WPB
#define SF_MC_WPB 4 // waves (= keypoints in flight) per workgroup: 4.6 KB of LDS each
#endif
#define SF_MC_BPAD ((long)0x8080808080808080ull) // eight neighbours' padding bin as a B operand: -128 each

// Which bins of the descriptor the table's 128 columns are: column c = bin win_lo + c for c < win_len; the other bins of the
// nb3 are structurally empty (sf_spfh::win_lo) and the keypoint's row gets zeros there.  win_lo = 0, win_len = nb3 for tables
// of at most 128 bins.
struct sf_bin_window { int nb3, win_lo, win_len; };
__device__ __forceinline__ void fpfh_mc_zero_outside(double *__restrict__ o, const sf_bin_window &W, int lane)
{
    if (W.win_len != W.nb3) // (wave-uniform)
        for (int b = lane; b < W.nb3; b += 64)
            if (b < W.win_lo || b >= W.win_lo + W.win_len) sf_store_stream(o + b, 0.0);
}

// The keypoint's row leaves the wave as ONE run of 16-byte pieces.  A lane owns bins i0 and i1 = i0 + 16 (the layout the matrix
// core leaves the sums in): stored from there, a row is eight 128-byte runs issued by two instructions, and -- a row of 125
// doubles starting 1000 q bytes into the array -- every run straddles 32-byte sectors it shares with the run of the OTHER
// instruction: 1.37 GB of write requests for 1.0 GB of rows at C3 (WRITE_SIZE, profiles/r05_summary.md).  So the two values go
// through the wave's LDS region (free by now) and lane l stores the aligned piece l of the row, 16 bytes -- 8 at the row's two
// ends when the row starts on an odd multiple of 8: one instruction, 1000 contiguous bytes, two partial sectors per row.
// (A windowed table -- n_bins above 5 -- keeps the plain stores: its row has holes.)
__device__ __forceinline__ void fpfh_mc_store_row(double *__restrict__ o, int n, int i0, double v0, int i1, double v1,
                                                  double *stage /* this wave's, >= 128 doubles */, int lane)
{
    if (i0 < n) stage[i0] = v0;
    if (i1 < n) stage[i1] = v1;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int shift = (int)((reinterpret_cast<uintptr_t>(o) >> 3) & 1u); // (wave-uniform) the row starts in the middle of a piece
    const int e = 2 * lane - shift;
    const bool a_ok = e >= 0 && e < n, b_ok = e + 1 < n;
    const double a = a_ok ? stage[e] : 0.0, b = b_ok ? stage[e + 1] : 0.0;
    if (a_ok && b_ok) sf_store_stream2(o + e, a, b);
    else if (a_ok) sf_store_stream(o + e, a);
    else if (b_ok) sf_store_stream(o + e + 1, b);
}

// The row epilogue (of every form but fpfh_mc_body, which has it as text): zeros outside the window, then the lane's two bins o0, o1 (values r0, r1) -- staged through
// `rowbuf` (free once the last step's reads have returned; fpfh_mc_store_row brings its own fences) or by the two plain stores.
__device__ __forceinline__ void fpfh_mc_finish_row(double *__restrict__ out, int64_t q, const sf_bin_window &W, int o0, int o1,
                                                   double r0, double r1, unsigned *rowbuf, int lane)
{
    double *o = out + q * (int64_t)W.nb3;
    fpfh_mc_zero_outside(o, W, lane);
    o += W.win_lo;
    if (W.win_len == W.nb3 && W.win_len <= 126) { // (wave-uniform)
        fpfh_mc_store_row(o, W.win_len, o0, r0, o1, r1, reinterpret_cast<double *>(rowbuf), lane);
    } else {
        if (o0 < W.win_len) sf_store_stream(o + o0, r0);
        if (o1 < W.win_len) sf_store_stream(o + o1, r1);
    }
}

// ---- scalar pieces ------------------------------------------------------------------------------------------------
// weight of a neighbour, 1 / (k_j d_j) = rsqrt(d2 k_j^2): v_rsq_f64 and two Newton steps (~1 ulp; the weight is a continuous
// factor, no decision depends on its last bit) instead of sqrt + division (~35 instructions).  0 past the end of the list
// (!on) and at distance 0 (fpfh.py:110-114).
__device__ __forceinline__ double sf_fpfh_weight(double d2, double kd, bool on)
{
    const double xx = d2 * (kd * kd);
    const double y0 = __builtin_amdgcn_rsq(xx);
    const double y1 = __builtin_fma(0.5 * y0, __builtin_fma(-(xx * y0), y0, 1.0), y0);
    const double y2 = __builtin_fma(0.5 * y1, __builtin_fma(-(xx * y1), y1, 1.0), y1);
    return (on && d2 > 0.0) ? y2 : 0.0;
}

// 1 / k to ~1 ulp: v_rcp_f64 and two Newton steps
__device__ __forceinline__ double sf_fpfh_inv(double kd)
{
    double inv_k = __builtin_amdgcn_rcp(kd);
    inv_k = __builtin_fma(inv_k, __builtin_fma(-kd, inv_k, 1.0), inv_k);
    return __builtin_fma(inv_k, __builtin_fma(-kd, inv_k, 1.0), inv_k);
}

// fixed point: W = floor(w 2^S) < 2^62 with S = 61 - floor(log2 of the wave's largest weight) (wmax: the lane's largest)
__device__ __forceinline__ int fpfh_mc_exponent(double wmax)
{
    wmax = sf_wave_max_nonneg(wmax);
    const int e2 = wmax > 0.0 ? (int)((__double2hiint(wmax) >> 20) & 0x7ff) - 1023 : 0;
    return 61 - e2;
}

// what the limb sums of lane group g = kb are worth: limbs 4 g, 4 g + 1 as a pair 2^(32 g - S), limbs 4 g + 2, 4 g + 3 2^16 more
__device__ __forceinline__ void fpfh_mc_scales(int kb, int S, double &f0, double &f2)
{
    f0 = ldexp(1.0, 32 * kb - S); // 2^(8 (4 g) - S)
    f2 = f0 * 65536.0;
}

// count / k (the keypoint's own SPFH term, fpfh.py:88-90) of the short forms, through the reciprocal already at hand and one
// residual step -- the closing step of a division: correctly rounded for these small integers at a tenth of the instructions.
// `own`: the table's byte (count ^ 128).  (The long forms, whose counts pass 255, divide.)
__device__ __forceinline__ double fpfh_mc_own_term(unsigned own, double kd, double inv_k)
{
    const double c = (double)(own ^ 128u);
    const double s = c * inv_k;
    return __builtin_fma(__builtin_fma(-s, kd, c), inv_k, s);
}

// ---- LDS-DMA and the transposing read -------------------------------------------------------------------------------
// Staged rows: 128 B each, no padding -- the image is written by LDS-DMA (buffer_load_dwordx4 ... lds: a wave
// instruction writes its 64 lanes' 16-byte chunks back to back), so the bank spread comes from the SOURCE side:
// slot s of row r holds chunk s ^ f(r), f(r) = (r >> 1) & 7.  A transposing read of one 32-lane half (8 rows x 16
// bytes of block g and of block g + 1, same chunk) then touches all 64 banks once.
// THE DMA statement: every lane's 16 bytes at byte `voff` of the buffer go to LDS, the wave's 64 pieces back to back from
// `lds_addr` on (wave-uniform; m0 is saved and restored around it).  Its "memory" clobber keeps loads and stores on their side.
__device__ __forceinline__ void sf_lds_dma16(unsigned voff, fpfh_mc_rsrc_t rsrc, unsigned lds_addr)
{
    unsigned keep_;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
                 "buffer_load_dwordx4 %1, %2, 0 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep_)
                 : "v"(voff), "s"(rsrc), "s"(lds_addr)
                 : "memory");
}

// ONE transposing read: in its 16-lane group lane 2 q + p supplies the address of bytes 8 p .. 8 p + 7 of "row" q and receives
// column (lane & 15) of those eight 16-byte rows, one per byte -- an int8 MFMA operand as it is.
__device__ __forceinline__ long fpfh_mc_tr_read(const unsigned char *p)
{
    const v2i_t t = __builtin_amdgcn_ds_read_tr8_b64_v2i32((__attribute__((address_space(3))) v2i_t *)p);
    return (long)(((unsigned long long)(unsigned)t[1] << 32) | (unsigned)t[0]);
}

// ---- the list and its weights ---------------------------------------------------------
// the lane's entries of the keypoint's neighbour list, chunk by chunk (lane t of chunk c <-> neighbour 64 c + t; -1 past the
// end).  The kernel is instantiated for the longest list of the launch; the chunks past THIS keypoint's list -- the last
// one for nine keypoints in ten -- are skipped wave-uniformly: no index load, no gather, no weight.
template <int NKS>
__device__ __forceinline__ void fpfh_mc_list(const int32_t *__restrict__ idx, int64_t s, int k, int lane, int (&jv)[NKS])
{
#pragma unroll
    for (int c = 0; c < NKS; ++c) {
        const int t = c * 64 + lane;
        jv[c] = -1;
        if (c == 0 || c * 64 < k) jv[c] = t < k ? SF_LIST_LOAD(idx + s + t) : -1;
    }
}

// weights of all neighbours from their 32-byte records {x, y, z, k} (sf_fpfh_weight), the fixed-point exponent
// (fpfh_mc_exponent), and jv clamped to valid rows for the gathers that follow
// HI: lm[c] = the lanes of chunk c whose neighbour has more than 255 neighbours of its own (its bins are lo + 256 hi: the
// table of high bytes, fpfh_mc_hi)
// MOM: the pass also forms the weighted covariance of the keypoint's SHOT frame (shot.py:27-35: w = r - ||c||, the keypoint
// itself included): mom_out of lane 8 e, e = 1 .. 6, is c11 c21 c31 c22 c32 c33.  It walks the very pairs K6's sweep walks --
// same lane <-> entry assignment, the same doubles (the record is a copy of the cloud's), c and d2 formed by the same
// expressions -- and repeats k_spfh's moments() and epilogue operation by operation (sf_sqrt_fast, the FMAs, chunks in
// ascending order per lane, sf_wave_sum8, sf_rcp_fast), so the six numbers are K6's bit for bit.  K6 is bound by vector issue
// with no register to spare; this kernel had idle issue slots and 18 registers free: +111 vector instructions here for -140
// there (profiles/k7_moments_ab.md).  Done before the step loop: the accumulators are dead when the MFMA accumulators come to
// life.  The caller keeps mom_out to the end of the kernel: a store from here sits in front of the step loop's vmcnt(0) wait.
template <int NKS, bool HI, bool MOM = false>
__device__ __forceinline__ int fpfh_mc_weights(const double *__restrict__ p4, double px, double py, double pz, int k,
                                               int (&jv)[NKS], double (&wv)[NKS], unsigned long long (&lm)[NKS],
                                               double mom_radius, double &mom_out)
{
    double gx[NKS], gy[NKS], gz[NKS], gk[NKS];
#pragma unroll
    for (int c = 0; c < NKS; ++c) {
        gx[c] = gy[c] = gz[c] = gk[c] = 0.0;
        if (c == 0 || c * 64 < k) {
            const int j = jv[c] < 0 ? 0 : jv[c];
            const double2 *pp = reinterpret_cast<const double2 *>(p4 + 4 * (size_t)j); // {x, y}, {z, k}: one 32-byte record
            const double2 u0 = pp[0], u1 = pp[1];
            gx[c] = u0.x; gy[c] = u0.y; gz[c] = u1.x; gk[c] = u1.y;
        }
    }
    SF_HEAD_PRIO_DROP(); // (raised at the kernel's start; the up-front DMA statements and the record loads have been issued)
    double wmax = 0.0;
    double ws = 0, a11 = 0, a21 = 0, a31 = 0, a22 = 0, a32 = 0, a33 = 0;
#pragma unroll
    for (int c = 0; c < NKS; ++c) {
        wv[c] = 0.0;
        if (c == 0 || c * 64 < k) {
            const double cx = gx[c] - px, cy = gy[c] - py, cz = gz[c] - pz;
            const double d2 = (cx * cx + cy * cy) + cz * cz;
            if (MOM && jv[c] >= 0) { // (k_spfh's moments(), spfh.hip)
                const double w = mom_radius - sf_sqrt_fast(d2);
                ws += w;
                const double wx = cx * w, wy = cy * w, wz = cz * w;
                a11 = __builtin_fma(cx, wx, a11); a21 = __builtin_fma(cy, wx, a21); a31 = __builtin_fma(cz, wx, a31);
                a22 = __builtin_fma(cy, wy, a22); a32 = __builtin_fma(cz, wy, a32); a33 = __builtin_fma(cz, wz, a33);
            }
            const double kd = gk[c];
            wv[c] = sf_fpfh_weight(d2, kd, jv[c] >= 0);
            wmax = fmax(wmax, wv[c]);
            if (HI) lm[c] = __ballot(wv[c] > 0.0 && kd > 255.0);
        } else if (HI) {
            lm[c] = 0ull;
        }
        jv[c] = jv[c] < 0 ? 0 : jv[c];
    }
    if (MOM) { // (k_spfh's epilogue)
        const double part[8] = {ws, a11, a21, a31, a22, a32, a33, 0.0};
        const double tot = sf_wave_sum8(part); // lanes 8 i .. 8 i + 7 hold the sum of part[i]
        const double iw = sf_rcp_fast(sf_read_lane(tot, 0));
        mom_out = tot * iw; // lanes 8 e, e = 1 .. 6: c11 c21 c31 c22 c32 c33 (the caller stores them)
    }
    return fpfh_mc_exponent(wmax);
}

// The part of sum_j w_j c_jb that the byte table does not hold: 256 sum_{j long} w_j hi_jb for the two bins this lane
// writes, in float64, neighbour after neighbour in list order (the same order on every rank and in every form, so the rows
// stay reproducible bit for bit).  Wave-uniform loop over the set bits of the masks: a keypoint without long neighbours --
// every keypoint of a cloud without long lists -- executes nothing.
template <int NKS>
__device__ __forceinline__ void fpfh_mc_hi(const uint8_t *__restrict__ hi, const int (&jv)[NKS], const double (&wv)[NKS],
                                           const unsigned long long (&lm)[NKS], int o0, int o1, double &c0, double &c1)
{
#pragma unroll
    for (int c = 0; c < NKS; ++c) {
        unsigned long long mk = lm[c];
        while (mk) { // four long neighbours per round: their eight byte loads are in flight together
            int t[4];
            bool on[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                on[u] = mk != 0ull;
                t[u] = on[u] ? __builtin_ctzll(mk) : t[0];
                mk &= mk - 1; // (0 stays 0)
            }
            unsigned b0[4], b1[4];
            double w[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = __builtin_amdgcn_readlane(jv[c], t[u]);
                const uint8_t *r = hi + (size_t)j * 128;
                b0[u] = r[o0];
                b1[u] = r[o1];
                const double wu = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(wv[c]), t[u]),
                                                   __builtin_amdgcn_readlane(__double2loint(wv[c]), t[u]));
                w[u] = on[u] ? wu * 256.0 : 0.0;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) { // (list order: the same sums on every rank and in every form)
                c0 = __builtin_fma(w[u], (double)b0[u], c0);
                c1 = __builtin_fma(w[u], (double)b1[u], c1);
            }
        }
    }
}

// This lane's weight as EIGHT signed-byte limbs: W = floor(w 2^S) < 2^62 is written in the signed-digit form
// W = sum_i d_i 256^i, d_i in [-128, 127] -- add 0x80 to every byte of W with carries, then flip every byte's top bit --
// which is what an int8 MFMA operand wants, 8 bits per limb instead of 7.  The limbs of neighbour t are the 8 bytes at
// abuf + 8 t: one ds_write_b64 per lane; the A operand (row = limb, k = neighbour) comes back through the same
// transposing read as the B operand (fpfh_mc_a_operand).
__device__ __forceinline__ void fpfh_mc_limbs(unsigned char *abuf, int lane, double w, int S)
{
    const double x = ldexp(w, S - 32); // < 2^30
    const unsigned hi = (unsigned)x;
    const unsigned lo = (unsigned)ldexp(x - (double)hi, 32);
    const unsigned long long W = ((unsigned long long)hi << 32) | lo;
    const unsigned long long D = (W + 0x8080808080808080ull) ^ 0x8080808080808080ull; // (hi < 2^30: no carry out)
    *reinterpret_cast<unsigned long long *>(abuf + 8 * lane) = D;
}

// A operand of a step (32 neighbours: 32 (st & 1) .. of the chunk whose limbs are in abuf): lane (a, kb) wants limb a of
// neighbours 8 kb .. 8 kb + 7, one per byte.  In its 16-lane group lane 2 q + p supplies the address of "row" q = one
// neighbour's 8 limb bytes for p = 0 and of 8 zero bytes (abuf + 512) for p = 1 -- limbs 8 .. 15 do not exist -- and
// receives column a of those eight 16-byte rows.
__device__ __forceinline__ long fpfh_mc_a_operand(const unsigned char *abuf, int a, int kb, int st)
{
    return fpfh_mc_tr_read((a & 1) ? abuf + 512 : abuf + 8 * (32 * (st & 1) + 8 * kb + (a >> 1)));
}

// ---- recombination: lane (a, g) holds rows (limbs) 4g .. 4g+3 of column a of an accumulator --------------------------
// A lane's four limb rows of one bin, SHORT lists: combined in INTEGER arithmetic first: |R| <= 128 * 128 * 255 < 2^22, so
// (R[r+1] << 8) + R[r] and the same combination of the padding column stay below 2^30.01, and their difference --
// (sum_j d_j c_jb of limb r + 1) 2^8 + (that of limb r), each at most 128 * 255 * 255 -- is below 2^31: it fits an
// int32 exactly (two's-complement wrap-around of an intermediate is harmless).  Two shift-adds and a subtraction per
// pair of limbs instead of a subtraction, a conversion and a float64 FMA per limb.
__device__ __forceinline__ double fpfh_mc_part(const v4i &acc, const v4i &pad, double f0, double f2)
{
    const int e01 = ((acc[1] << 8) + acc[0]) - ((pad[1] << 8) + pad[0]);
    const int e23 = ((acc[3] << 8) + acc[2]) - ((pad[3] << 8) + pad[2]);
    return __builtin_fma((double)e23, f2, (double)e01 * f0);
}

// ... LONG lists: the limb pairs formed in float64 (the integer shift-adds would overflow; on a short list the two give the
// same bits)
__device__ __forceinline__ double fpfh_mcl_pair(int hi_limb, int lo_limb, int pad_hi, int pad_lo)
{
    return __builtin_fma((double)hi_limb - (double)pad_hi, 256.0, (double)lo_limb - (double)pad_lo); // exact: < 2^41
}
__device__ __forceinline__ double fpfh_mcl_part(const v4i &acc, const v4i &pad, double f0, double f2)
{
    return __builtin_fma(fpfh_mcl_pair(acc[3], acc[2], pad[3], pad[2]), f2, fpfh_mcl_pair(acc[1], acc[0], pad[1], pad[0]) * f0);
}

// Sum over the four limb groups g = kb of the FULL form, transposing as we go: after the exchange with lane ^ 32 a lane keeps
// only the blocks bb = 4 (kb >> 1) + {0..3}, after the one with lane ^ 16 only bb = 4 (kb >> 1) + 2 (kb & 1) + {0, 1} -- the two
// bins it writes (v0, v1).  gfx950's lane-swap instructions do the exchange AND the selection in one go, without the LDS
// (sf_lane_swap): a + b is "my half's block plus the partner's" in both halves.  The order of the additions -- g + (g ^ 2)
// first, then the two halves of that -- is the contract every form keeps.
__device__ __forceinline__ void fpfh_mc_reduce_full(const double (&part)[8], double &v0, double &v1)
{
    double keep[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        double a_ = part[u], b_ = part[4 + u];
        sf_lane_swap<32>(a_, b_);
        keep[u] = a_ + b_;
    }
    double a0 = keep[0], b0_ = keep[2], a1 = keep[1], b1_ = keep[3];
    sf_lane_swap<16>(a0, b0_);
    sf_lane_swap<16>(a1, b1_);
    v0 = a0 + b0_;
    v1 = a1 + b1_;
}

// The same sum of the TWO-BLOCK form, in the SAME order, so that the rounding, hence every bit of the row, is the full form's:
// after the 32-swap the lower half of the wave holds block b0's pair sums and the upper half block b1's, after the 16-swap both
// rows of a half hold the total; every lane needs both totals for the row it helps write, the other half's through one more
// 32-swap.  v0, v1: the sums of the lane's bins of blocks bb0, bb0 + 1 -- a dead block's are exactly 0.
__device__ __forceinline__ void fpfh_mc_reduce_pair(double part0, double part1, int bb0, int b0, int b1, double &v0, double &v1)
{
    sf_lane_swap<32>(part0, part1);
    double v = part0 + part1; // lanes 0..31: block b0, groups (g, g + 2) ; lanes 32..63: block b1
    double w = v;
    sf_lane_swap<16>(v, w);
    const double tot = v + w; // all four groups; lanes 0..31: bin 16 b0 + a, lanes 32..63: bin 16 b1 + a
    double tot0 = tot, tot1 = tot;
    sf_lane_swap<32>(tot0, tot1); // (after the swap tot0 is block b0's total in both halves, tot1 block b1's)
    v0 = bb0 == b0 ? tot0 : (bb0 == b1 ? tot1 : 0.0);
    v1 = bb0 + 1 == b0 ? tot0 : (bb0 + 1 == b1 ? tot1 : 0.0);
}

// The two callers of the DMA statement, as MACROS: they expand in a body next to its jv[], rsrc, lds_rows and lane maps.  (As
// __forceinline__ functions they cost k_fpfh_mc<3> and <4> 24 and 39 spilled registers and k_fpfh_mc_sparse<3> and <4> two to
// four registers, as does a function around the loop of a whole-row step: profiles/k7_family_isa.md.)
// They take from the body that expands them: jv[], lane, rsrc, lds_rows, and dma_chunk (ROWS) or d_row, dma_chunk16, ROW_BYTES
// (PAIR).  ST must be a constant after unrolling: jv[] stays in registers.  CLAMP: the list entries may still be -1 (short forms).
// Whole rows: the 32 rows of step ST (neighbours 32 ST .. + 31 = lanes 32 (ST & 1) .. of chunk ST >> 1), 4 instructions of
// 64 x 16 bytes, 4 KB.
#define SF_MC_DMA_ROWS(ST, CLAMP)                                                                                    \
    {                                                                                                               \
        _Pragma("unroll") for (int u = 0; u < 4; ++u) {                                                             \
            const int jr0 = __shfl(jv[(ST) >> 1], 32 * ((ST) & 1) + 8 * u + (lane >> 3));                           \
            const int jr = (CLAMP) && jr0 < 0 ? 0 : jr0; /* idle slots of the last step fetch row 0 */              \
            sf_lds_dma16((unsigned)jr * 128u + 16u * (unsigned)(dma_chunk ^ ((u & 1) << 2)), rsrc, lds_rows + 1024u * u); \
        }                                                                                                           \
    }
// Two live chunks: ONE instruction for the 32 rows of step ST, into quarter ST & 3 of the row buffer (NCH: chunks jv[] holds).
#define SF_MC_DMA_PAIR(ST, NCH, CLAMP)                                                                               \
    {                                                                                                               \
        const int jr0 = __shfl(jv[((ST) >> 1) < (NCH) ? ((ST) >> 1) : 0], 32 * ((ST) & 1) + d_row);                 \
        const int jr = (CLAMP) && jr0 < 0 ? 0 : jr0;                                                                \
        sf_lds_dma16((unsigned)jr * ROW_BYTES + dma_chunk16, rsrc, lds_rows + 1024u * (unsigned)((ST) & 3));        \
    }

// acc += A x B on the matrix core: B a transposing read (fpfh_mc_tr_read) or the constant padding operand
__device__ __forceinline__ v4i fpfh_mc_mfma(long A, long B, v4i acc) { return __builtin_amdgcn_mfma_i32_16x16x32_i8(A, B, acc, 0, 0, 0); }

// The two live chunks of the step's quarter at `rb`: two reads, three MFMAs (blocks b0, b1, and the padding column).
__device__ __forceinline__ void fpfh_mc_step_pair(long A, const unsigned char *rb, int rd0, int rd1, v4i &acc0, v4i &acc1, v4i &accp)
{
    const long B0 = fpfh_mc_tr_read(rb + rd0), B1 = fpfh_mc_tr_read(rb + rd1);
    accp = fpfh_mc_mfma(A, SF_MC_BPAD, accp);
    acc0 = fpfh_mc_mfma(A, B0, acc0);
    acc1 = fpfh_mc_mfma(A, B1, acc1);
}

// PADC: the padding column that removes the -128 bias comes from an MFMA against a constant operand (as in the sparse form)
// instead of column 127 of the table -- for a window of 128 real bins (n_bins = 8), which leaves no padding column.
template <int NKS, bool HI, bool PADC = false>
__device__ __forceinline__ void fpfh_mc_body(const double *__restrict__ rec, const int64_t *__restrict__ offset,
                                             const int32_t *__restrict__ cnt, const int32_t *__restrict__ idx,
                                             int64_t nbrs_begin, const int32_t *__restrict__ kp_pos, sf_bin_window W,
                                             const uint8_t *__restrict__ counts, unsigned table_bytes,
                                             const double *__restrict__ p4, double *__restrict__ out, int64_t q,
                                             unsigned *rowbuf /* 4 KB */, unsigned char *abuf /* 576 B */,
                                             const uint8_t *__restrict__ hi, int limit)
{
    const int lane = threadIdx.x & 63;
    const int64_t i = kp_pos ? (int64_t)kp_pos[q] : nbrs_begin + q;
    const int64_t slot = i - nbrs_begin;
    const int64_t s = offset[slot];
    const int k = cnt[slot];
    if (sf_uniform(k) > limit) return; // (a keypoint whose own list exceeds this form: the second launch, launch_fpfh_mc)
    const double px = rec[6 * i + 0], py = rec[6 * i + 1], pz = rec[6 * i + 2];
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(counts), 0, (int)table_bytes, 0x00020000);
    const int a = lane & 15, kb = lane >> 4;
    // (the keypoint's own counts of the two bins this lane writes, requested with the list: see the sparse form)
    const unsigned own0 = counts[i * 128 + 16 * (4 * (kb >> 1) + 2 * (kb & 1)) + a], own1 = counts[i * 128 + 16 * (4 * (kb >> 1) + 2 * (kb & 1)) + a + 16];
    if (lane == 0) *reinterpret_cast<unsigned long long *>(abuf + 512) = 0ull; // the "limbs 8 .. 15" every A operand reads
    // Lane map of the full form (own text in both full bodies: as a function it lengthened their MFMA blocks).  Reads: in its
    // group (k block kb) lane 2 q + p supplies the address of row 8 kb + q, bytes 8 p .. + 7 of chunk bb (slot bb ^ f(row),
    // f(row) = (row >> 1) & 7), and receives bin 16 bb + a of those eight rows -- exactly its B operand.  DMA: lane l of
    // instruction u fills slot l & 7 of row 8 u + (l >> 3) with chunk (l & 7) ^ f(row): dma_chunk, ^ 4 for u = 1, 3.
    const int frow = ((a >> 2) & 3) | ((kb & 1) << 2);
    const int rd_base = (8 * kb + (a >> 1)) * 128 + 8 * (a & 1); // bytes
    int xoff[8];
#pragma unroll
    for (int bb = 0; bb < 8; ++bb) xoff[bb] = rd_base + 16 * (bb ^ frow);
    const int dma_chunk = (lane & 7) ^ ((lane >> 4) & 3);
    const unsigned lds_rows = (unsigned)__builtin_amdgcn_readfirstlane(
        (int)(unsigned)(size_t)(__attribute__((address_space(3))) unsigned *)rowbuf);
    int jv[NKS];
    double wv[NKS];
    unsigned long long lm[NKS];
    fpfh_mc_list<NKS>(idx, s, k, lane, jv);
    SF_MC_DMA_ROWS(0, true) // in flight while the weights are computed
    double mom_unused = 0.0;
    const int S = fpfh_mc_weights<NKS, HI>(p4, px, py, pz, k, jv, wv, lm, 0.0, mom_unused);

    v4i acc[8]; // acc[bb]: column a = bin 16 bb + a, rows = limbs 4 kb .. 4 kb + 3
#pragma unroll
    for (int bb = 0; bb < 8; ++bb) acc[bb] = v4i{0, 0, 0, 0};
    v4i accp = v4i{0, 0, 0, 0};

#pragma unroll
    for (int st = 0; st < 2 * NKS; ++st) {
        if (st * 32 < k) { // wave-uniform
            if (st > 0) SF_MC_DMA_ROWS(st, true) // (step 0 was issued before the weights were computed)
            if ((st & 1) == 0) fpfh_mc_limbs(abuf, lane, wv[st >> 1], S); // the two steps of a chunk use the lower / upper 32 columns
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the DMA pieces have landed
            __builtin_amdgcn_wave_barrier(); // both buffers are private to the wave; LDS operations of a wave stay in order
            const long A = fpfh_mc_a_operand(abuf, a, kb, st); // row a = limb a (rows 8 .. 15: zero)
            const unsigned char *rb = reinterpret_cast<const unsigned char *>(rowbuf);
#pragma unroll
            for (int bb = 0; bb < 8; ++bb) acc[bb] = fpfh_mc_mfma(A, fpfh_mc_tr_read(rb + xoff[bb]), acc[bb]);
            if (PADC) accp = fpfh_mc_mfma(A, SF_MC_BPAD, accp);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // reads done before the next step's DMA overwrites the rows
            __builtin_amdgcn_wave_barrier();
        }
    }
    // ---- recombination: lane (a, g) holds rows (limbs) 4g .. 4g+3 of column a of acc[bb]; bin = 16 bb + a ----
    int rp[4]; // the padding column: the constant operand's, or column 15 of bb = 7 (bin 127) of the table
#pragma unroll
    for (int r = 0; r < 4; ++r) rp[r] = PADC ? accp[r] : __builtin_amdgcn_update_dpp(0, acc[7][r], 0x150 + 15, 0xf, 0xf, false);
    const v4i rpad = v4i{rp[0], rp[1], rp[2], rp[3]};
    double f0, f2;
    fpfh_mc_scales(kb, S, f0, f2);
    const double kd = (double)k, inv_k = sf_fpfh_inv(kd);
    // partial sums over this lane's four limbs, for its eight bins
    double part[8];
#pragma unroll
    for (int bb = 0; bb < 8; ++bb) part[bb] = fpfh_mc_part(acc[bb], rpad, f0, f2);
    double vsel0, vsel1;
    fpfh_mc_reduce_full(part, vsel0, vsel1);
    {
        const int bb0 = 4 * (kb >> 1) + 2 * (kb & 1);
        const int b0 = 16 * bb0 + a, b1 = b0 + 16;
        // (own text of fpfh_mc_finish_row, the zeros first: through the function k_fpfh_mc<1, 2, 4>'s MFMA blocks grew)
        double *o = out + q * (int64_t)W.nb3;
        fpfh_mc_zero_outside(o, W, lane);
        o += W.win_lo;
        const double s0 = fpfh_mc_own_term(own0, kd, inv_k), s1 = fpfh_mc_own_term(own1, kd, inv_k);
        double h0 = 0.0, h1 = 0.0;
        if (HI) fpfh_mc_hi<NKS>(hi, jv, wv, lm, b0, b1, h0, h1);
        const double r0 = s0 + (HI ? vsel0 + h0 : vsel0) * inv_k, r1 = s1 + (HI ? vsel1 + h1 : vsel1) * inv_k;
        if (W.win_len == W.nb3 && W.win_len <= 126) { // (wave-uniform)
            fpfh_mc_store_row(o, W.win_len, b0, r0, b1, r1, reinterpret_cast<double *>(rowbuf), lane);
        } else {
            if (b0 < W.win_len) sf_store_stream(o + b0, r0);
            if (b1 < W.win_len) sf_store_stream(o + b1, r1);
        }
    }
}

// --------------------------------------------------------------------------------------------------
// The same contraction when at most TWO of the table's eight 16-bin blocks hold any count (blocks b0, b1; K6 keeps the OR
// of the non-empty blocks of every row it writes).  Per step of 32 neighbours ONE LDS-DMA instruction fetches the two live
// 16-byte chunks of each row (lane l: row l >> 1 ... see the mapping below) instead of four instructions for the whole
// rows, two transposing reads + two MFMAs replace eight, and the padding column that removes the -128 bias is an MFMA
// against a constant operand (every byte 0x80) instead of a column read from the table.  Results are those of the full
// kernel bit for bit: the integer sums of the live bins are the same sums, and a dead bin's sum is exactly its bias.
// --------------------------------------------------------------------------------------------------
// PACKED: the two chunks come from K6's packed copy of the table (`rows`: 32 bytes per row = {chunk b0, chunk b1}) instead
// of the table itself (`rows` = counts, 128 bytes per row): four rows per cache line for the gather.
template <int NKS, bool PACKED, bool HI, bool MOM = false>
__device__ __forceinline__ void fpfh_mc_body_sparse(const double *__restrict__ rec, const int64_t *__restrict__ offset,
                                                    const int32_t *__restrict__ cnt, const int32_t *__restrict__ idx,
                                                    int64_t nbrs_begin, const int32_t *__restrict__ kp_pos, sf_bin_window W,
                                                    const uint8_t *__restrict__ counts, const uint8_t *__restrict__ rows,
                                                    unsigned rows_bytes, const double *__restrict__ p4,
                                                    double *__restrict__ out, int64_t q, int b0, int b1,
                                                    unsigned *rowbuf /* 4 KB: four steps of 1 KB */, unsigned char *abuf /* 576 B */,
                                                    const uint8_t *__restrict__ hi, int limit, double mom_radius = 0.0,
                                                    double *__restrict__ cov = nullptr /* MOM: 6 doubles per query */)
{
    const int lane = threadIdx.x & 63;
    const int64_t i = kp_pos ? (int64_t)kp_pos[q] : nbrs_begin + q;
    const int64_t slot = i - nbrs_begin;
    const int64_t s = offset[slot];
    const int k = cnt[slot];
    if (sf_uniform(k) > limit) return; // (the second launch's keypoint)
    const double px = rec[6 * i + 0], py = rec[6 * i + 1], pz = rec[6 * i + 2];
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(rows), 0, (int)rows_bytes, 0x00020000);
    const int a = lane & 15, kb = lane >> 4;
    // the keypoint's own counts of the two bins this lane writes: requested HERE, with the list -- the "memory" clobbers of the
    // DMA statements below pin a load where it is written, and at the end of the kernel (where the values are used) it was a
    // memory round trip of its own on every wave's critical path
    const int bb0 = 4 * (kb >> 1) + 2 * (kb & 1);
    const int o0 = 16 * bb0 + a, o1 = o0 + 16; // as in the full kernel
    const unsigned own0 = counts[i * 128 + o0], own1 = counts[i * 128 + o1];
    if (lane == 0) *reinterpret_cast<unsigned long long *>(abuf + 512) = 0ull; // the "limbs 8 .. 15" every A operand reads
    // LDS image of a step: 64 pieces of 16 bytes, piece P = 32 (kb >> 1) + 16 u + 8 (kb & 1) + q holds chunk b_u of row
    // 8 kb + q -- the DMA writes its lanes' pieces back to back, so lane P fetches exactly that; the 32 pieces a
    // transposing read of block u touches per half-wave then lie in 32 different 8-byte bank pairs.
    const int d_u = (lane >> 4) & 1, d_row = 16 * (lane >> 5) + (lane & 15); // = 8 (2 (P >> 5) + ((P >> 3) & 1)) + (P & 7)
    const unsigned dma_chunk16 = PACKED ? 16u * (unsigned)d_u : 16u * (unsigned)(d_u ? b1 : b0);
    constexpr unsigned ROW_BYTES = PACKED ? 32u : 128u;
    const int rd_piece = 32 * (kb >> 1) + 8 * (kb & 1) + (a >> 1); // + 16 u ; bytes 8 (a & 1) .. of the piece
    const int rd0 = 16 * rd_piece + 8 * (a & 1), rd1 = rd0 + 256;
    const unsigned lds_rows = (unsigned)__builtin_amdgcn_readfirstlane(
        (int)(unsigned)(size_t)(__attribute__((address_space(3))) unsigned *)rowbuf);
    int jv[NKS];
    double wv[NKS];
    unsigned long long lm[NKS];
    fpfh_mc_list<NKS>(idx, s, k, lane, jv);
    // The image of a step is 1 KB, so the 4 KB row buffer holds FOUR steps: the rows of the first two chunks (128
    // neighbours -- the whole list for nine keypoints in ten) are all requested here, in flight while the weights are
    // computed, and the step loop below never waits on memory again; only a third / fourth chunk re-uses the buffer.
    SF_MC_DMA_PAIR(0, NKS, true)
    if (32 < k) SF_MC_DMA_PAIR(1, NKS, true)
    if (NKS >= 2 && 64 < k) SF_MC_DMA_PAIR(2, NKS, true)
    if (NKS >= 2 && 96 < k) SF_MC_DMA_PAIR(3, NKS, true)
    double mom = 0.0;
    const int S = fpfh_mc_weights<NKS, HI, MOM>(p4, px, py, pz, k, jv, wv, lm, mom_radius, mom);

    v4i acc0 = v4i{0, 0, 0, 0}, acc1 = v4i{0, 0, 0, 0}, accp = v4i{0, 0, 0, 0}; // blocks b0, b1, and the padding column

#pragma unroll
    for (int st = 0; st < 2 * NKS; ++st) {
        if (st * 32 < k) { // wave-uniform
            if (st >= 4) SF_MC_DMA_PAIR(st, NKS, true) // (steps 0 .. 3 were requested up front; by now their regions have been consumed)
            if ((st & 1) == 0) fpfh_mc_limbs(abuf, lane, wv[st >> 1], S);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the DMA pieces have landed
            __builtin_amdgcn_wave_barrier();
            const long A = fpfh_mc_a_operand(abuf, a, kb, st); // row a = limb a (rows 8 .. 15: zero)
            const unsigned char *rb = reinterpret_cast<const unsigned char *>(rowbuf);
            fpfh_mc_step_pair(A, rb, rd0 + 1024 * (st & 3), rd1 + 1024 * (st & 3), acc0, acc1, accp);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // reads done before the next step's DMA overwrites the pieces
            __builtin_amdgcn_wave_barrier();
        }
    }
    // ---- recombination: lane (a, g) holds limbs 4g .. 4g + 3 of bin 16 b_u + a in acc_u, and of the padding column in accp
    //      (every column of accp is the same sum) ----
    double f0, f2;
    fpfh_mc_scales(kb, S, f0, f2);
    const double kd = (double)k, inv_k = sf_fpfh_inv(kd);
    const double part0 = fpfh_mc_part(acc0, accp, f0, f2), part1 = fpfh_mc_part(acc1, accp, f0, f2);
    double v0, v1;
    fpfh_mc_reduce_pair(part0, part1, bb0, b0, b1, v0, v1);
    if (MOM && (lane & 7) == 0 && lane >= 8 && lane < 56) cov[6 * q + (lane >> 3) - 1] = mom;
    {
        const double s0 = fpfh_mc_own_term(own0, kd, inv_k), s1 = fpfh_mc_own_term(own1, kd, inv_k);
        double h0 = 0.0, h1 = 0.0;
        if (HI) fpfh_mc_hi<NKS>(hi, jv, wv, lm, o0, o1, h0, h1);
        const double r0 = s0 + (HI ? v0 + h0 : v0) * inv_k, r1 = s1 + (HI ? v1 + h1 : v1) * inv_k;
        fpfh_mc_finish_row(out, q, W, o0, o1, r0, r1, rowbuf, lane);
    }
}

// --------------------------------------------------------------------------------------------------
// The matrix-core contraction for lists of MORE than 255 points.  Nothing in the arithmetic above is tied to 255 neighbours but
// the registers that hold a list
// and the int32 recombination: |limb x (count - 128)| <= 2^14 per neighbour, so the int32 accumulators hold EXACT sums for any
// list a byte table can have (k <= 65 535 -> < 2^30).  So: a first pass over the list finds the largest weight (the fixed-point
// exponent), the second walks it in super-chunks of SC x 64 neighbours -- index loads, record gathers and weights of a
// super-chunk at once, then its 2 SC steps of 32 neighbours through the same LDS-DMA / transposing reads / MFMAs -- and the
// limb sums are recombined once, in float64 (fpfh_mcl_part).  A list of at most SC x 64 points keeps entries and weights in registers between the passes.
// High bytes of neighbours that have more than 255 neighbours of their own: fpfh_mc_hi per super-chunk, list order.
// The sparse and the full form mirror each other operation by operation, as the short forms do: same bits.
// --------------------------------------------------------------------------------------------------
template <int SC>
__device__ __forceinline__ void fpfh_mcl_load(const int32_t *__restrict__ idx, const double *__restrict__ p4, int64_t s, int k,
                                              int base, int lane, double px, double py, double pz, int (&jv)[SC], double (&wv)[SC],
                                              unsigned long long (&lm)[SC])
{
#pragma unroll
    for (int c = 0; c < SC; ++c) {
        const int t = base + 64 * c + lane;
        jv[c] = (base + 64 * c < k && t < k) ? SF_LIST_LOAD(idx + s + t) : -1;
    }
    double2 u0[SC], u1[SC];
#pragma unroll
    for (int c = 0; c < SC; ++c) {
        u0[c] = u1[c] = make_double2(0.0, 0.0);
        if (base + 64 * c < k) { // (wave-uniform)
            const double2 *pp = reinterpret_cast<const double2 *>(p4 + 4 * (size_t)(jv[c] < 0 ? 0 : jv[c]));
            u0[c] = pp[0];
            u1[c] = pp[1];
        }
    }
#pragma unroll
    for (int c = 0; c < SC; ++c) {
        const double cx = u0[c].x - px, cy = u0[c].y - py, cz = u1[c].x - pz;
        const double d2 = (cx * cx + cy * cy) + cz * cz;
        const double kd = u1[c].y;
        const bool on = jv[c] >= 0;
        wv[c] = sf_fpfh_weight(d2, kd, on); // (weight 0 past the end and at distance 0: all limbs 0)
        lm[c] = __ballot(wv[c] > 0.0 && kd > 255.0);
        jv[c] = on ? jv[c] : 0; // (past the end of the list row 0 is fetched, under weight 0)
    }
}

template <bool PACKED, int SC>
__device__ __forceinline__ void fpfh_mcl_body_sparse(const double *__restrict__ rec, const int64_t *__restrict__ offset,
                                                     const int32_t *__restrict__ cnt, const int32_t *__restrict__ idx,
                                                     int64_t nbrs_begin, const int32_t *__restrict__ kp_pos, sf_bin_window W,
                                                     const uint8_t *__restrict__ counts, const uint8_t *__restrict__ rows,
                                                     unsigned rows_bytes, const double *__restrict__ p4,
                                                     double *__restrict__ out, int64_t q, int b0, int b1,
                                                     unsigned *rowbuf /* 4 KB: four steps of 1 KB */, unsigned char *abuf /* 576 B */,
                                                     const uint8_t *__restrict__ hi, int limit)
{
    const int lane = threadIdx.x & 63;
    const int64_t i = kp_pos ? (int64_t)kp_pos[q] : nbrs_begin + q;
    const int64_t slot = i - nbrs_begin;
    const int k = sf_uniform(cnt[slot]);
    if (k <= limit) return; // (the main launch's keypoint)
    const int64_t s = offset[slot];
    const double px = rec[6 * i + 0], py = rec[6 * i + 1], pz = rec[6 * i + 2];
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(rows), 0, (int)rows_bytes, 0x00020000);
    const int a = lane & 15, kb = lane >> 4;
    const int bb0 = 4 * (kb >> 1) + 2 * (kb & 1);
    const int o0 = 16 * bb0 + a, o1 = o0 + 16; // the two bins this lane writes, as in the short forms
    unsigned own0 = (unsigned)counts[i * 128 + o0] ^ 128u, own1 = (unsigned)counts[i * 128 + o1] ^ 128u;
    if (k > 255) { own0 += 256u * (unsigned)hi[i * 128 + o0]; own1 += 256u * (unsigned)hi[i * 128 + o1]; }
    if (lane == 0) *reinterpret_cast<unsigned long long *>(abuf + 512) = 0ull; // the "limbs 8 .. 15" every A operand reads
    // LDS image of a step and the DMA's lane mapping: fpfh_mc_body_sparse
    const int d_u = (lane >> 4) & 1, d_row = 16 * (lane >> 5) + (lane & 15);
    const unsigned dma_chunk16 = PACKED ? 16u * (unsigned)d_u : 16u * (unsigned)(d_u ? b1 : b0);
    constexpr unsigned ROW_BYTES = PACKED ? 32u : 128u;
    const int rd_piece = 32 * (kb >> 1) + 8 * (kb & 1) + (a >> 1);
    const int rd0 = 16 * rd_piece + 8 * (a & 1), rd1 = rd0 + 256;
    const unsigned lds_rows = (unsigned)__builtin_amdgcn_readfirstlane(
        (int)(unsigned)(size_t)(__attribute__((address_space(3))) unsigned *)rowbuf);
    int jv[SC];
    double wv[SC];
    unsigned long long lm[SC];
    // ---- pass 0: the largest weight -> the fixed-point exponent ----
    double wmax = 0.0;
    for (int base = 0; base < k; base += 64 * SC) {
        fpfh_mcl_load<SC>(idx, p4, s, k, base, lane, px, py, pz, jv, wv, lm);
#pragma unroll
        for (int c = 0; c < SC; ++c) wmax = fmax(wmax, wv[c]);
    }
    const int S = fpfh_mc_exponent(wmax);

    v4i acc0 = v4i{0, 0, 0, 0}, acc1 = v4i{0, 0, 0, 0}, accp = v4i{0, 0, 0, 0}; // blocks b0, b1, and the padding column
    double h0 = 0.0, h1 = 0.0;
    for (int base = 0; base < k; base += 64 * SC) {
        if (k > 64 * SC) fpfh_mcl_load<SC>(idx, p4, s, k, base, lane, px, py, pz, jv, wv, lm); // (else: still held from pass 0)
        const int left = k - base;
        const int nst = left >= 64 * SC ? 2 * SC : (left + 31) >> 5; // steps of this super-chunk (wave-uniform)
        // The 4 KB row buffer holds four steps: up to four are in flight, and a step's slot is refilled as soon as its reads
        // have returned -- the loop waits for the OLDEST request only (vector-memory requests complete in order).
#pragma unroll
        for (int st = 0; st < 4; ++st)
            if (st < nst) SF_MC_DMA_PAIR(st, SC, false)
#pragma unroll
        for (int st = 0; st < 2 * SC; ++st) {
            if (st < nst) { // wave-uniform
                if ((st & 1) == 0) fpfh_mc_limbs(abuf, lane, wv[st >> 1], S);
                if (st + 3 < nst) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
                else if (st + 2 < nst) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
                else if (st + 1 < nst) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
                else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __builtin_amdgcn_wave_barrier();
                const long A = fpfh_mc_a_operand(abuf, a, kb, st);
                const unsigned char *rb = reinterpret_cast<const unsigned char *>(rowbuf);
                fpfh_mc_step_pair(A, rb, rd0 + 1024 * (st & 3), rd1 + 1024 * (st & 3), acc0, acc1, accp);
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // reads done before the slot is refilled
                __builtin_amdgcn_wave_barrier();
                if (st + 4 < nst) SF_MC_DMA_PAIR(st + 4, SC, false)
            }
        }
        fpfh_mc_hi<SC>(hi, jv, wv, lm, o0, o1, h0, h1);
    }
    // ---- recombination: fpfh_mc_body_sparse's, the limb pairs formed in float64 ----
    double f0, f2;
    fpfh_mc_scales(kb, S, f0, f2);
    const double kd = (double)k, inv_k = sf_fpfh_inv(kd);
    double v0, v1;
    fpfh_mc_reduce_pair(fpfh_mcl_part(acc0, accp, f0, f2), fpfh_mcl_part(acc1, accp, f0, f2), bb0, b0, b1, v0, v1);
    {
        const double r0 = (double)own0 / kd + (v0 + h0) * inv_k, r1 = (double)own1 / kd + (v1 + h1) * inv_k; // spfh[kp] + sum / len(neighbourhood)  (fpfh.py:109-115)
        fpfh_mc_finish_row(out, q, W, o0, o1, r0, r1, rowbuf, lane);
    }
}

// ... and on a table with more than two live blocks: whole 128-byte rows, one step (4 KB) in LDS at a time, eight MFMAs per step
template <int SC, bool PADC = false>
__device__ __forceinline__ void fpfh_mcl_body(const double *__restrict__ rec, const int64_t *__restrict__ offset,
                                              const int32_t *__restrict__ cnt, const int32_t *__restrict__ idx,
                                              int64_t nbrs_begin, const int32_t *__restrict__ kp_pos, sf_bin_window W,
                                              const uint8_t *__restrict__ counts, unsigned table_bytes,
                                              const double *__restrict__ p4, double *__restrict__ out, int64_t q,
                                              unsigned *rowbuf /* 4 KB */, unsigned char *abuf /* 576 B */,
                                              const uint8_t *__restrict__ hi, int limit)
{
    const int lane = threadIdx.x & 63;
    const int64_t i = kp_pos ? (int64_t)kp_pos[q] : nbrs_begin + q;
    const int64_t slot = i - nbrs_begin;
    const int k = sf_uniform(cnt[slot]);
    if (k <= limit) return; // (the main launch's keypoint)
    const int64_t s = offset[slot];
    const double px = rec[6 * i + 0], py = rec[6 * i + 1], pz = rec[6 * i + 2];
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(counts), 0, (int)table_bytes, 0x00020000);
    const int a = lane & 15, kb = lane >> 4;
    const int bb0 = 4 * (kb >> 1) + 2 * (kb & 1);
    const int o0 = 16 * bb0 + a, o1 = o0 + 16;
    unsigned own0 = (unsigned)counts[i * 128 + o0] ^ 128u, own1 = (unsigned)counts[i * 128 + o1] ^ 128u;
    if (k > 255) { own0 += 256u * (unsigned)hi[i * 128 + o0]; own1 += 256u * (unsigned)hi[i * 128 + o1]; }
    if (lane == 0) *reinterpret_cast<unsigned long long *>(abuf + 512) = 0ull;
    // (lane map of the full form: fpfh_mc_body)
    const int frow = ((a >> 2) & 3) | ((kb & 1) << 2);
    const int rd_base = (8 * kb + (a >> 1)) * 128 + 8 * (a & 1); // bytes
    int xoff[8];
#pragma unroll
    for (int bb = 0; bb < 8; ++bb) xoff[bb] = rd_base + 16 * (bb ^ frow);
    const int dma_chunk = (lane & 7) ^ ((lane >> 4) & 3);
    const unsigned lds_rows = (unsigned)__builtin_amdgcn_readfirstlane(
        (int)(unsigned)(size_t)(__attribute__((address_space(3))) unsigned *)rowbuf);
    int jv[SC];
    double wv[SC];
    unsigned long long lm[SC];
    double wmax = 0.0;
    for (int base = 0; base < k; base += 64 * SC) {
        fpfh_mcl_load<SC>(idx, p4, s, k, base, lane, px, py, pz, jv, wv, lm);
#pragma unroll
        for (int c = 0; c < SC; ++c) wmax = fmax(wmax, wv[c]);
    }
    const int S = fpfh_mc_exponent(wmax);
    v4i acc[8];
#pragma unroll
    for (int bb = 0; bb < 8; ++bb) acc[bb] = v4i{0, 0, 0, 0};
    v4i accp = v4i{0, 0, 0, 0};
    double h0 = 0.0, h1 = 0.0;
    for (int base = 0; base < k; base += 64 * SC) {
        if (k > 64 * SC) fpfh_mcl_load<SC>(idx, p4, s, k, base, lane, px, py, pz, jv, wv, lm);
        const int left = k - base;
        const int nst = left >= 64 * SC ? 2 * SC : (left + 31) >> 5;
#pragma unroll
        for (int st = 0; st < 2 * SC; ++st) {
            if (st < nst) { // wave-uniform
                SF_MC_DMA_ROWS(st, false)
                if ((st & 1) == 0) fpfh_mc_limbs(abuf, lane, wv[st >> 1], S);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __builtin_amdgcn_wave_barrier();
                const long A = fpfh_mc_a_operand(abuf, a, kb, st);
                const unsigned char *rb = reinterpret_cast<const unsigned char *>(rowbuf);
#pragma unroll
                for (int bb = 0; bb < 8; ++bb) acc[bb] = fpfh_mc_mfma(A, fpfh_mc_tr_read(rb + xoff[bb]), acc[bb]);
                if (PADC) accp = fpfh_mc_mfma(A, SF_MC_BPAD, accp);
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_wave_barrier();
            }
        }
        fpfh_mc_hi<SC>(hi, jv, wv, lm, o0, o1, h0, h1);
    }
    // ---- recombination: fpfh_mc_body's, the limb pairs formed in float64 ----
    int rp[4]; // the padding column: the constant operand's, or column 15 of bb = 7 (bin 127) of the table
#pragma unroll
    for (int r = 0; r < 4; ++r) rp[r] = PADC ? accp[r] : __builtin_amdgcn_update_dpp(0, acc[7][r], 0x150 + 15, 0xf, 0xf, false);
    const v4i rpad = v4i{rp[0], rp[1], rp[2], rp[3]};
    double f0, f2;
    fpfh_mc_scales(kb, S, f0, f2);
    const double kd = (double)k, inv_k = sf_fpfh_inv(kd);
    double part[8];
#pragma unroll
    for (int bb = 0; bb < 8; ++bb) part[bb] = fpfh_mcl_part(acc[bb], rpad, f0, f2);
    double vsel0, vsel1;
    fpfh_mc_reduce_full(part, vsel0, vsel1);
    {
        const double r0 = (double)own0 / kd + (vsel0 + h0) * inv_k, r1 = (double)own1 / kd + (vsel1 + h1) * inv_k;
        fpfh_mc_finish_row(out, q, W, o0, o1, r0, r1, rowbuf, lane);
    }
}

#undef SF_MC_DMA_ROWS
#undef SF_MC_DMA_PAIR
