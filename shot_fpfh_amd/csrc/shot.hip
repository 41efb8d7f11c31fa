// shot.hip -- K5, the SHOT descriptor (register-cached, team and streaming forms) and its entry points.
//
// Replaces: compute_single_shot_descriptor  shot.py:175-306; ShotMultiprocessor's drivers shot_parallelization.py:135-312;
//           the serial compute_shot_descriptor shot.py:310-499; get_azimuth_idx shot.py:51-70.
// Mapping: one wave per keypoint (the wave holds the whole neighbourhood, 64 neighbours per register chunk); lists above 255
// points: a team of waves per keypoint, streamed beyond 3 072.  Neighbours are gathered from the cell-sorted AoS records.
// All bin-deciding arithmetic is float64 with FMA contraction off.  HBM roofline, algorithmic bytes: the 352 x 8 = 2816 B row
// + 24 B keypoint + 72 B frame per keypoint.  (Until round 6: the body of descriptors.hip; K3 / K4: normals_lrf.hip.)
#include "common.h"
#include "device_util.h"
#include "host_stage.h"
#include "shot_core.h"
#include <hip/amd_detail/amd_hip_unsafe_atomics.h>

namespace {


// --------------------------------------------------------------------------------------------------
// K5: SHOT descriptor.
//
// The reference accumulates with ten NumPy fancy-index statements "D[idx] += val" (shot.py:244-298).
// With duplicate indices NumPy keeps only the LAST write of each statement, and neighbours are
// ordered by ascending rho (shot.py:218), so per statement and bin the neighbour with the LARGEST rho
// wins and the ten per-statement winners are summed.  The ten statements use five distinct writer
// keys: A = (ci,ti,pi,ri) [S2,S5,S8,S10], B = (ci+-1,ti,pi,ri) [S1], G = (ci,ti+-1,pi,ri) [S9],
// CD = (ci,ti,pi) [S3 -> radial bin 1, S4 -> radial bin 0], EF = (ci,ti,ri) [S6 -> elevation bin 1,
// S7 -> elevation bin 0].  Sweep 1 elects winners with 64-bit LDS atomicMax on the bit pattern of rho
// (positive doubles order like unsigned integers); sweep 2 lets each winner overwrite its slot with its
// value, tagged by the sign bit (all values are >= 0) so that later lanes cannot mistake it for a key.
// One wave per keypoint: the register-cached form (k_shot_cached, 5.5 KB of LDS, two phases) takes every list of at most
// 255 points, the streamed form (k_shot_long) the longer ones.
// --------------------------------------------------------------------------------------------------
// (the helpers that do not depend on the number of cosine bins -- octant, roots, polynomials, weights, slot tags -- are in
// shot_core.h, shared with the serial SHOT of any bin count, shot_bins.hip)

// get_azimuth_idx as an elementwise function (shot.py:51-70): the very device function K5 bins with
__global__ void k_azimuth_idx(const double *__restrict__ x, const double *__restrict__ y, int64_t n, int64_t *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = azimuth_octant(x[i], y[i]);
}

#ifndef SF_SHOT_WPB
#define SF_SHOT_WPB 2 // waves (= keypoints) per workgroup: 1.61 / 1.54 / 1.55 / 1.80 ms at C3 for 1 / 2 / 4 / 8
#endif

// Slot numbers of the cached form's LDS tables (round 6).  Bin b = ((cosine * 8 + azimuth) * 2 + half-space) * 2 + shell lives
// in slot b ^ (2 (b >> 5)).  With slot = b the bank pair of an 8-byte slot is b mod 32 = (azimuth, half-space, shell) WHATEVER
// the cosine bin -- and the 32 lanes an LDS pass serves hold neighbours that follow each other in the cell-sorted order, i.e.
// that lie in the same direction from the keypoint: same octant, same half-space, same shell, told apart by the cosine bin of
// their normals alone.  Their 64-bit election atomics met in a handful of bank pairs (SQ_LDS_BANK_CONFLICT 312 cycles per wave,
// half of the LDS pipe's active cycles; 239 cycles per wave waiting behind an LDS instruction).  XOR-ing bits 1-4 with the
// cosine bin puts the eleven cosine bins of one direction into eleven bank pairs: 206 conflict cycles, 105 waiting, K5 -2 %
// (tools/pmc_k5.sh and tools/ab_libs.sh, same box, three rounds).  Measured beside it: XOR with 3 x the cosine bin, which also
// spreads the shell bit (148 conflict cycles, but the row read-out then has to exchange the halves of its pairs: +10 vector
// instructions per keypoint, and the kernel is bound by those -- 1 % slower than this form); the shell bit moved to the top of
// the slot number (slot = cell + 176 shell: no change, 288 cycles -- the shell does not tell the lanes of a pass apart).
// The XOR stays inside the cosine bin's 32 slots, keeps a pair of adjacent bins adjacent and in order, and commutes with the
// ^ 1 / ^ 2 that reach the other shell / half-space; bit 1 of a slot number is no longer the half-space (bins1 carries it).
// All three 9-bit fields of bins0 at once.  (The team form keeps the plain numbering: with the two more registers the re-mapped
// read-out of its four tables takes, its fused instantiations drop from eight waves per SIMD to seven.)
__device__ inline unsigned shot_swz3(unsigned b)
{
    return b ^ ((b >> 4) & 0x783C1Eu); // every 9-bit field f becomes f ^ (2 (f >> 5))
}

template <int NCH, bool FUSED>
__device__ __forceinline__ void shot_cached_body(const double *__restrict__ rec,
                                                 const double *__restrict__ qx, const double *__restrict__ qy,
                                                 const double *__restrict__ qz, const int64_t *__restrict__ offset,
                                                 const int32_t *__restrict__ cnt, const int32_t *__restrict__ idx,
                                                 const int32_t *__restrict__ qrow, const shot_consts &K,
                                                 double *__restrict__ lrf, int normalize, int64_t min_nb,
                                                 double *__restrict__ out, int64_t q, unsigned long long *slot,
                                                 const shot_ties &ties)
{
    // FUSED: `lrf` holds the raw axes written by k_shot_lrf(raw = 1); the sign votes (shot.py:40-45) are taken
    // here from the gathered neighbours and the finished frame is written back before it is used.
    // LDS: 704 election slots (5.5 KB per wave), used twice.  Phase 1 elects and resolves the writers of
    // S2+S5+S8+S10 (A, 352 slots), S3/S4 (CD, 176) and S6/S7 (EF, 176); phase 2 those of S1 (B, 352) and S9
    // (G, 352).  Halving the footprint (it was 11 KB with all five tables live at once) is what lets the
    // register file, not LDS, set the occupancy.  A CD / EF slot carries ONE value plus a flag in bit 62
    // (unused by doubles below 2.0): the S3/S4 pair of a winner has a single non-zero member, selected by
    // the winner's radial bin, and likewise S6/S7 by its elevation bin.
    SF_K5_MARK(1, NCH);
    unsigned long long *const sA = slot;
    const int lane = threadIdx.x & 63;
    const int64_t s = offset[q];
    const int k = cnt[q];
    const int64_t row = qrow ? qrow[q] : q;
    double *o = out + (int64_t)SF_SHOT_LEN * row;
    const double px = qx[q], py = qy[q], pz = qz[q];

    // (only the election / accumulator half: sX is cleared before each of its two uses; 16 bytes per lane and store)
    for (int b = lane; b < 176; b += 64) reinterpret_cast<ulonglong2 *>(slot)[b] = make_ulonglong2(0ull, 0ull);

    SF_K5_MARK(2, NCH);
    // one gather for all chunks
    double cx[NCH], cy[NCH], cz[NCH], nx[NCH], ny[NCH], nz[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) // (padding lanes carry point 0's offset; they are masked by `onm` below)
        shot_gather64<true>(rec, idx + s, c * 64 + lane, k, px, py, pz, cx[c], cy[c], cz[c], nx[c], ny[c], nz[c]);
    SF_K5_MARK(3, NCH);
    unsigned long long onm[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) onm[c] = shot_chunk_mask(k - 64 * c);
    double E[9];
    if (FUSED) {
        double *lr = lrf + 9 * row;
        double raw[9];
        // Scalar loads, by reading the nine numbers through the constant address space: this wave is the only one that touches
        // this frame, it reads it here and writes it below, so the scalar cache never holds a stale copy of it -- but the
        // compiler, seeing stores to `lrf` in the same kernel, proves that for one of the two inlined bodies only and loads the
        // other's frame into vector registers (every flip below then costs vector instructions).  The pin keeps all nine loads
        // in front of the votes (left alone the scheduler sinks the y loads to their first use: a scalar-memory round trip of
        // their own in the middle of the kernel).  (The same lines stand in k_shot_team: as a function of shot_core.h they
        // cost k_shot_cached<1, true> four scalar registers and k_shot_team<3, 16, true> two -- profiles/k5_family_isa.md.)
        sf_const_doubles clr = (sf_const_doubles)lr;
#pragma unroll
        for (int i = 0; i < 9; ++i) raw[i] = clr[i];
#pragma unroll
        for (int i = 0; i < 9; ++i) asm volatile("" : "+s"(raw[i]));
        int xneg = 0, zneg = 0;
#pragma unroll
        for (int c = 0; c < NCH; ++c) shot_count_votes(cx[c], cy[c], cz[c], raw, onm[c], xneg, zneg);
        if (shot_finish_frame(raw, k, xneg, zneg, E) && lane == 0) {
#pragma unroll
            for (int i = 0; i < 9; ++i) lr[i] = E[i]; // (streamed past the L2 like the rows: no difference)
        }
    } else {
#pragma unroll
        for (int i = 0; i < 9; ++i) E[i] = lrf[9 * row + i];
    }

    SF_K5_MARK(4, NCH);
    double d2[NCH];
    unsigned long long posm[NCH];
    int npos = 0;
#pragma unroll
    for (int c = 0; c < NCH; ++c) shot_gate(cx[c], cy[c], cz[c], onm[c], d2[c], posm[c], npos);
    if (!(npos > (int)min_nb)) { // (launch_shot passes min_nb clamped into [-1, 2^31 - 1]: a scalar 32-bit comparison)
        for (int b = lane; b < SF_SHOT_LEN; b += 64) o[b] = 0.0;
        return;
    }
    SF_SHOT_SYNC();
    // Election and accumulation.  sA (352 slots) first elects the writers of S2+S5+S8+S10 by rho, then becomes the
    // ACCUMULATOR of the row: its winners store their (negated) value, and every other statement's winner adds its own
    // (negated) value to the bin it feeds with an LDS float64 atomic add -- the LDS pipe does the additions, the bins are
    // never assembled by the vector ALU.  Every wave of the workgroup (SF_SHOT_WPB of them, one keypoint each) works in its
    // OWN LDS region and never waits for another; a wave's LDS instructions execute in program order, so the order of the
    // additions into a bin -- hence every bit of the row -- is the same in every run, whatever the workgroup size.
    // S3/S4 and S6/S7 need no election of their own: their writer is the farthest neighbour of a cell (cosine, azimuth,
    // half-space) over BOTH radial shells, resp. of a cell (cosine, azimuth, shell) over both half-spaces -- i.e. the
    // farther of the two S2 winners of bins base ^ 1, resp. base ^ 2.  Those two keys are read back after the election,
    // next to the bin's own, and compared: three plain reads replace two 64-bit LDS atomic maxima and two
    // compare-and-swaps per neighbour (the LDS pipe was 77 % busy, more than half of it bank
    // conflicts of the random 8-byte atomics -- tools/pmc_k5.sh).  sX (352 slots) serves S1 (B), then S9 (G).
    unsigned long long *const sX = slot + 352;
    double *const acc = reinterpret_cast<double *>(slot);
    // (a claimed sX slot holds its key with the sign bit set -- no rho has it -- so a second holder of that key knows what it met)
    constexpr unsigned WON_A = 1u << 28, WON_CD = 1u << 29, WON_EF = 1u << 30; // flags kept in bins1 (bit 31 = valid)
    // bit 27: this neighbour met another holder of its winning key (shot_core.h); the wave reports the keypoint if any did.  (A bit
    // of a register the chunk holds anyway: the scalar stream is what holds this kernel back, and a lane mask kept to the end is
    // two scalar registers it lacks.)
    constexpr unsigned MET = 1u << 27;
    shot_kept g[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        g[c].bins1 = 0u;
        SF_K5_MARK(5, NCH);
        // (a branch per chunk on purpose: calling the geometry for all lanes puts the chunks' chains into one basic block, the
        // scheduler interleaves them and the kernel needs 87 registers instead of 70 -- 5 waves per SIMD, 1.72 ms; capped at
        // 72 / 80 registers it spills / runs 1.62 ms)
        if (__builtin_amdgcn_inverse_ballot_w64(posm[c])) {
            shot_geometry<11>(cx[c], cy[c], cz[c], d2[c], nx[c], ny[c], nz[c], E, K.half_r, 11, 11.0, g[c]);
            g[c].bins0 = shot_swz3(g[c].bins0);
            SF_K5_MARK(6, NCH);
            atomicMax(&sA[shot_slot_a<11>(g[c])], shot_key(g[c]));
        }
    }
    SF_SHOT_SYNC();
    SF_K5_MARK(7, NCH);
    // who writes what (all reads of the keys come before the first winner replaces its key by a value)
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        if (__builtin_amdgcn_inverse_ballot_w64(posm[c])) {
            const unsigned long long key = shot_key(g[c]);
            const unsigned iA = shot_slot_a<11>(g[c]);
            const bool up = g[c].bins1 & 2u, odd = g[c].bins1 & 1u; // (z > 0; outer shell -- iA is a SLOT number: shot_swz3)
            const unsigned long long own = sA[iA], other_shell = sA[iA ^ 1u], other_half = sA[iA ^ 2u];
            unsigned f = 0u;
            if (own == key) {
                f = WON_A;
                if (shot_writes_cd(odd, other_shell)) f |= WON_CD;
                if (shot_writes_ef(key, other_half, up)) f |= WON_EF;
                if (key == other_half) f |= MET;
            }
            g[c].bins1 |= f;
        }
    }
    // the winners of A store; every neighbour keeps what its other statements may have to add
    double v_cd[NCH], v_ef[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        v_cd[c] = 0.0;
        v_ef[c] = 0.0;
        SF_K5_MARK(8, NCH);
        if (__builtin_amdgcn_inverse_ballot_w64(posm[c])) {
            const unsigned long long key = shot_key(g[c]);
            const unsigned iA = shot_slot_a<11>(g[c]);
            double vA, adth;
            shot_weights(g[c], K, vA, v_cd[c], v_ef[c], adth);
            SF_K5_MARK(9, NCH);
            g[c].tdot = adth;
            // compare-and-swap, not a plain store: two neighbours at exactly the same distance hold the same key, and the ADDS
            // below must come from one of them only.  Their values differ unless they are one point named twice (another
            // direction, another normal): the holder that finds the slot taken reports the tie, and the row is computed again
            // under the full order (rho, caller index) by k_shot_tied
            const bool lost = (g[c].bins1 & WON_A) && atomicCAS(&sA[iA], key, tag_value(vA)) != key;
            if (lost) g[c].bins1 = (g[c].bins1 & ~WON_A) | MET; // (WON_CD / WON_EF are read under WON_A only)
        }
    }
    SF_SHOT_SYNC();
    SF_K5_MARK(10, NCH);
    // S3/S4 and S6/S7: the writer adds into the bin with the OTHER radial / elevation bit than its own
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        if (g[c].bins1 & WON_A) {
            const unsigned iA = shot_slot_a<11>(g[c]);
            if ((g[c].bins1 & WON_CD) && v_cd[c] != 0.0) unsafeAtomicAdd(&acc[iA ^ 1u], -v_cd[c]);
            if ((g[c].bins1 & WON_EF) && v_ef[c] != 0.0) unsafeAtomicAdd(&acc[iA ^ 2u], -v_ef[c]);
        }
    }
    SF_SHOT_SYNC();
    SF_K5_MARK(11, NCH);
    // S1 (value |dc|) and S9 (value |dth|): elect in sX, add into the accumulator
#pragma unroll
    for (int stmt = 0; stmt < 2; ++stmt) {
        for (int b = lane; b < 176; b += 64) reinterpret_cast<ulonglong2 *>(sX)[b] = make_ulonglong2(0ull, 0ull);
        SF_SHOT_SYNC();
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            if (__builtin_amdgcn_inverse_ballot_w64(posm[c]))
                atomicMax(&sX[stmt ? shot_slot_g<11>(g[c]) : shot_slot_b<11>(g[c])], shot_key(g[c]));
        }
        SF_SHOT_SYNC();
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            if (__builtin_amdgcn_inverse_ballot_w64(posm[c])) {
                const unsigned long long key = shot_key(g[c]);
                const unsigned iW = stmt ? shot_slot_g<11>(g[c]) : shot_slot_b<11>(g[c]);
                const double val = stmt ? g[c].tdot : fabs(g[c].dc); // S1's range mask is always true for cf in 0..10
                const unsigned long long was = atomicCAS(&sX[iW], key, shot_claimed(key));
                if (was == key && val != 0.0) unsafeAtomicAdd(&acc[iW], -val);
                if (was == shot_claimed(key)) g[c].bins1 |= MET;
            }
        }
        SF_SHOT_SYNC();
    }
    SF_K5_MARK(12, NCH);
    // every slot of the accumulator is +0 (nothing written) or minus the bin's value: the row is acc * (-scale) + 0 (the sum
    // of squares does not see the sign; the "+ 0" makes an empty slot +0 whatever the sign of the scale).
    // A lane takes PAIRS of adjacent bins -- (2 l, 2 l + 1) of each third of the row -- so that the row leaves in three
    // 16-byte-per-lane store instructions instead of six 8-byte ones (and is read back in three LDS instructions): a wave's
    // slot is held until its stores are acknowledged, and the row is issued at the very end of the wave's work -- leaving
    // five of the six store instructions out (timing only) made the kernel 14 % faster, halving their number 1-1.5 %.
    double2 vals[3];
    double ss = 0.0;
#pragma unroll
    for (int u = 0; u < 3; ++u) {
        const int b = 2 * lane + 128 * u;
        // bins b, b + 1 are the slots b ^ g, (b ^ g) + 1 with g = 2 (b >> 5) = 2 (lane >> 4) + 8 u: an aligned pair, in order
        const int sb = ((2 * lane) ^ (2 * (lane >> 4)) ^ (8 * u)) + 128 * u;
        vals[u] = b < 352 ? *reinterpret_cast<const double2 *>(acc + sb) : make_double2(0.0, 0.0);
        ss += vals[u].x * vals[u].x;
        ss += vals[u].y * vals[u].y;
    }
    const double nscale = shot_row_scale(ss, normalize, true);
#pragma unroll
    for (int u = 0; u < 3; ++u) {
        const int b = 2 * lane + 128 * u;
        if (b < 352) sf_store_stream2(o + b, __builtin_fma(vals[u].x, nscale, 0.0), __builtin_fma(vals[u].y, nscale, 0.0));
    }
    unsigned met = 0u;
#pragma unroll
    for (int c = 0; c < NCH; ++c) met |= g[c].bins1;
    if (__ballot((met & MET) != 0u) && lane == 0) shot_report_tie(ties, q);
}


// --------------------------------------------------------------------------------------------------
// K5 for lists of ANY length (the keypoints whose own list exceeds the register-cached form: dense regions, and the
// reference's default configuration -- a support subsampled at radius / 10 puts 300-500 voxels' points into a ball on a
// surface scan).  Same arithmetic as the cached form (shot_geometry / shot_weights: the short polynomial forms, the octant
// fast path, S3/S4 and S6/S7 writers read off the S2 election), streamed: the list is swept three times, 128 neighbours in
// flight -- (V) sign votes of the frame + the gate, (1) geometry -> the three elections (64-bit LDS atomic max on rho's bit
// pattern for S2.., S1, S9), (2) geometry again -> weights -> every elected writer claims its (statement, bin) once (a bit
// per slot: two neighbours at exactly the same distance hold the same key; the second to come has met a tie, whose order is
// (rho, caller index) -- the keypoint is reported and k_shot_tied computes its row, shot_core.h) and ADDS its value into a
// float64 accumulator row with ds_add_f64.  LDS per wave: 3 x 352 keys + 352 accumulators + 3 x 352 claim bits = 11.4 KB.  A wave's LDS
// instructions execute in program order and no two lanes of one instruction target the same slot (one claimed writer per
// statement and bin), so every bit of the row is reproducible.  (Until round 4 this was `k_shot`, a two-sweep kernel on
// libm's atan2 / acos with five election tables: 2.3x the time per neighbour of the cached form.)
// --------------------------------------------------------------------------------------------------
#ifndef SF_SHOT_LONG_WPB
#define SF_SHOT_LONG_WPB 2
#endif
struct shot_long_lds {
    unsigned long long keyA[352], keyB[352], keyG[352];
    double acc[352];
    unsigned claim[3][12];
};

template <bool FUSED, bool SEL>
__global__ __launch_bounds__(64 * SF_SHOT_LONG_WPB) void k_shot_long(const double *__restrict__ rec,
                                             const double *__restrict__ qx, const double *__restrict__ qy,
                                             const double *__restrict__ qz, const int64_t *__restrict__ offset,
                                             const int32_t *__restrict__ cnt, const int32_t *__restrict__ idx,
                                             const int32_t *__restrict__ qrow,
                                             int64_t m, shot_consts K, double *__restrict__ lrf, int normalize,
                                             int64_t min_nb, double *__restrict__ out, const int32_t *__restrict__ sel,
                                             int64_t nsel, int64_t view_first, int lo, shot_ties ties)
{
    __shared__ __attribute__((aligned(16))) shot_long_lds lds_all[SF_SHOT_LONG_WPB];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    shot_long_lds &L = lds_all[wave];
    int64_t q = sf_xcd_block() * SF_SHOT_LONG_WPB + wave;
    if (!shot_pick_keypoint(q, SEL, sel, nsel, view_first, m)) return;
    const int64_t s = offset[q];
    const int k = sf_uniform(cnt[q]);
    if (k <= lo) return; // (a list the team form of another launch holds: launch_shot)
    const int64_t row = qrow ? qrow[q] : q;
    double *o = out + (int64_t)SF_SHOT_LEN * row;
    const double px = qx[q], py = qy[q], pz = qz[q];
    {
        unsigned long long *w = reinterpret_cast<unsigned long long *>(&L);
        for (int b = lane; b < (int)(sizeof(shot_long_lds) / 8); b += 64) w[b] = 0ull;
    }
    double raw[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (FUSED) {
        const double *lr = lrf + 9 * row;
#pragma unroll
        for (int i = 0; i < 9; ++i) raw[i] = lr[i];
    }
    // ---- sweep V: gate (shot.py:212, 306) and the frame's sign votes (shot.py:40-45) ----
    int npos = 0, xneg = 0, zneg = 0;
    for (int t0 = 0; t0 < k; t0 += 128) {
        int jj[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int t = t0 + 64 * u + lane;
            jj[u] = t < k ? idx[s + t] : -1;
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            double x, y, z;
            sf_load_xyz(rec, jj[u] < 0 ? 0 : jj[u], x, y, z);
            const double cx = x - px, cy = y - py, cz = z - pz;
            const bool on = jj[u] >= 0;
            npos += __popcll(__ballot(on && ((cx * cx + cy * cy) + cz * cz) > 0.0));
            if (FUSED) {
                xneg += __popcll(__ballot(on && sf_dot3(cx, cy, cz, raw[0], raw[3], raw[6]) < 0.0));
                zneg += __popcll(__ballot(on && sf_dot3(cx, cy, cz, raw[2], raw[5], raw[8]) < 0.0));
            }
        }
    }
    double E[9];
    if (FUSED) { // (the frame is written whether or not the descriptor passes the gate, as in the cached form)
        if (shot_finish_frame(raw, k, xneg, zneg, E) && lane == 0) {
#pragma unroll
            for (int i = 0; i < 9; ++i) lrf[9 * row + i] = E[i];
        }
    } else {
#pragma unroll
        for (int i = 0; i < 9; ++i) E[i] = lrf[9 * row + i];
    }
    if (!((int64_t)npos > min_nb)) {
        for (int b = lane; b < SF_SHOT_LEN; b += 64) o[b] = 0.0;
        return;
    }
    SF_SHOT_SYNC(); // (the cleared tables)
    // one step of a sweep (shot_geometry128 with 11 bins; the list is read through the caches: it is swept three times)
    auto geometry128 = [&](int t0, shot_kept (&g)[2]) {
        unsigned long long pos[2], over[2];
        shot_geometry128<11, false>(rec, idx + s, t0, k, lane, px, py, pz, E, K.half_r, 11, 11.0, g, pos, over);
    };
    // ---- sweep 1: the three elections ----
    for (int t0 = 0; t0 < k; t0 += 128) {
        shot_kept g[2];
        geometry128(t0, g);
#pragma unroll
        for (int u = 0; u < 2; ++u)
            if (g[u].bins1 >> 31) {
                atomicMax(&L.keyA[shot_slot_a<11>(g[u])], shot_key(g[u]));
                atomicMax(&L.keyB[shot_slot_b<11>(g[u])], shot_key(g[u]));
                atomicMax(&L.keyG[shot_slot_g<11>(g[u])], shot_key(g[u]));
            }
    }
    SF_SHOT_SYNC();
    // ---- sweep 2: every elected writer claims its slot and adds its value ----
    // true for exactly one of the neighbours holding the winning key; another holder that comes later has met a tie (its
    // values are its own: shot_core.h) and the row is computed again by k_shot_tied
    bool tie = false;
    auto claim = [&](int table, unsigned slot_) -> bool {
        const unsigned bit = 1u << (slot_ & 31u);
        const bool first = (atomicOr(&L.claim[table][slot_ >> 5], bit) & bit) == 0u;
        tie |= !first;
        return first;
    };
    for (int t0 = 0; t0 < k; t0 += 128) {
        shot_kept g[2];
        geometry128(t0, g);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (g[u].bins1 >> 31) {
                const unsigned long long key = shot_key(g[u]);
                const unsigned iA = shot_slot_a<11>(g[u]), iB = shot_slot_b<11>(g[u]), iG = shot_slot_g<11>(g[u]);
                // (bit 1 of a slot: z > 0, bit 0: outer shell)
                const unsigned long long own = L.keyA[iA], other_shell = L.keyA[iA ^ 1u], other_half = L.keyA[iA ^ 2u];
                const bool winB = L.keyB[iB] == key, winG = L.keyG[iG] == key;
                double vA, v_cd, v_ef, adth;
                shot_weights(g[u], K, vA, v_cd, v_ef, adth);
                tie |= own == key && other_half == key;
                if (own == key && claim(0, iA)) {
                    unsafeAtomicAdd(&L.acc[iA], vA);
                    if (shot_writes_cd(iA & 1u, other_shell) && v_cd != 0.0) unsafeAtomicAdd(&L.acc[iA ^ 1u], v_cd);
                    if (shot_writes_ef(key, other_half, iA & 2u) && v_ef != 0.0) unsafeAtomicAdd(&L.acc[iA ^ 2u], v_ef);
                }
                const double adc = fabs(g[u].dc);
                if (winB && claim(1, iB) && adc != 0.0) unsafeAtomicAdd(&L.acc[iB], adc);
                if (winG && claim(2, iG) && adth != 0.0) unsafeAtomicAdd(&L.acc[iG], adth);
            }
        }
    }
    SF_SHOT_SYNC();
    // (six values held across the norm: read twice from LDS, through a loop shared with k_shot_bins, the kernel took 117
    // registers instead of 115 -- profiles/k5_family_isa.md)
    double vals[6];
    double ss = 0.0;
#pragma unroll
    for (int u = 0; u < 6; ++u) {
        const int b = lane + 64 * u;
        const double v = b < 352 ? L.acc[b] : 0.0;
        vals[u] = v;
        ss += v * v;
    }
    const double scale = shot_row_scale(ss, normalize, false);
#pragma unroll
    for (int u = 0; u < 6; ++u) {
        const int b = lane + 64 * u;
        if (b < 352) sf_store_stream(o + b, vals[u] * scale);
    }
    if (__ballot(tie) && lane == 0) shot_report_tie(ties, q);
}

template <int NCH, bool FUSED>
__global__ __launch_bounds__(64 * SF_SHOT_WPB) void k_shot_cached(const double *__restrict__ rec,
                                                    const double *__restrict__ qx, const double *__restrict__ qy,
                                                    const double *__restrict__ qz, const int64_t *__restrict__ offset,
                                                    const int32_t *__restrict__ cnt, const int32_t *__restrict__ idx,
                                                    const int32_t *__restrict__ qrow,
                                                    int64_t m, shot_consts K, double *__restrict__ lrf,
                                                    int normalize, int64_t min_nb, double *__restrict__ out, int limit,
                                                    const int32_t *__restrict__ sel, int64_t nsel, int64_t view_first,
                                                    shot_ties ties)
{
    __shared__ __attribute__((aligned(16))) unsigned long long slots[SF_SHOT_WPB][704];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    unsigned long long *const slot = slots[wave];
    int64_t q = sf_xcd_block() * SF_SHOT_WPB + wave;
    // (sel: the launch of the lists that need more chunks than the bulk, sf_dispatch::mid_sel)
    if (!shot_pick_keypoint(q, sel != nullptr, sel, nsel, view_first, m)) return;
    // (a keypoint whose own list is longer than this launch's form holds belongs to the second launch: launch_shot)
    if (sf_uniform(cnt[q]) > limit) return;
    // The kernel is instantiated for the LONGEST list of the launch (a 1M-point uniform cloud at 110 neighbours on average
    // has one of 160+), but nearly every keypoint fits one chunk less: a wave-uniform branch picks the body that
    // matches THIS keypoint, so the gather, votes and distance tests of an empty last chunk are never issued.
    if (NCH >= 3 && sf_uniform(cnt[q]) <= 64 * (NCH - 1)) {
        shot_cached_body<(NCH >= 3 ? NCH - 1 : NCH), FUSED>(rec, qx, qy, qz, offset, cnt, idx, qrow, K, lrf, normalize, min_nb, out, q, slot, ties);
        return;
    }
    shot_cached_body<NCH, FUSED>(rec, qx, qy, qz, offset, cnt, idx, qrow, K, lrf, normalize, min_nb, out, q, slot, ties);
}

// --------------------------------------------------------------------------------------------------
// K5 for lists of 256 .. 64 NCH NW points (round 5): a TEAM of waves -- one workgroup -- per keypoint.  The register-cached
// form's work, spread over waves: a list of n chunks is served by a = ceil(n / NCH) waves (the workgroup's other waves end at
// once; a barrier waits for the surviving waves only), wave w holding the chunks w, w + a, w + 2a of the list in registers:
// ONE gather, the geometry evaluated ONCE (the streaming form evaluates it twice, once to elect and once to add, because no
// single wave can keep 12 registers per chunk for a list of any length), the election tables are the workgroup's.  All three
// elections (S2.., S1, S9) run in one phase on three key tables; the winners then replace their key by their value (one
// compare-and-swap claims the slot and stores) and the S3/S4 and S6/S7 writers store into a value table of their own (two
// addends per slot at most: commutative), so the row is the sum of the four tables in a fixed order -- every bit of it
// independent of how the waves were scheduled and of the team's size AS LONG AS no two neighbours hold the same winning key:
// which of two such holders claims first is a race between waves.  The one that finds the slot taken raises a flag, the
// keypoint is reported and k_shot_tied computes its row under the order (rho, caller index) -- shot_core.h.  Four
// workgroup barriers per keypoint.  LDS: 4 x 352 x 8 B + 256 B = 11.3 KB per team.
// --------------------------------------------------------------------------------------------------
#ifndef SF_TEAM_NCH
#define SF_TEAM_NCH 3 // 70 registers: seven waves per SIMD (tools/ab_long.sh: 2 / 3 / 4 chunks per wave)
#endif
struct shot_team_lds {
    unsigned long long keyA[352], keyB[352], keyG[352]; // keys (rho's bit pattern), then tagged values: S2+S5+S8+S10, S1, S9
    double vx[352];                                      // S3/S4 + S6/S7 by destination bin (two addends at most: see below)
    __attribute__((aligned(16))) int red[16][4];         // per wave: gate count and the two sign votes; [0][3]: a tie was met
};

template <int NCH, int NW, bool FUSED>
__global__ __launch_bounds__(64 * NW) void k_shot_team(const double *__restrict__ rec, const double *__restrict__ qx,
                                                       const double *__restrict__ qy, const double *__restrict__ qz,
                                                       const int64_t *__restrict__ offset, const int32_t *__restrict__ cnt,
                                                       const int32_t *__restrict__ idx, const int32_t *__restrict__ qrow,
                                                       int64_t m, shot_consts K, double *__restrict__ lrf, int normalize,
                                                       int64_t min_nb, double *__restrict__ out,
                                                       const int32_t *__restrict__ sel, int64_t nsel, int64_t view_first,
                                                       int lo, shot_ties ties)
{
    __shared__ __attribute__((aligned(16))) shot_team_lds L;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    int64_t q = sf_xcd_block();
    if (!shot_pick_keypoint(q, sel != nullptr, sel, nsel, view_first, m)) return;
    const int k = sf_uniform(cnt[q]);
    if (k <= lo || k > 64 * NCH * NW) return; // (another launch's list: launch_shot)
    const int nact = (((k + 63) >> 6) + NCH - 1) / NCH; // waves that hold a part of this list
    if (wave >= nact) return;
    const int nthr = 64 * nact;
    const int64_t s = offset[q];
    const int64_t row = qrow ? qrow[q] : q;
    double *o = out + (int64_t)SF_SHOT_LEN * row;
    const double px = qx[q], py = qy[q], pz = qz[q];
    {
        ulonglong2 *w = reinterpret_cast<ulonglong2 *>(&L);
        for (int b = threadIdx.x; b < 704; b += nthr) w[b] = make_ulonglong2(0ull, 0ull);
    }
    // this wave's chunks of the list: chunk w + a c of the list is its chunk c
    double cx[NCH], cy[NCH], cz[NCH], nx[NCH], ny[NCH], nz[NCH];
    unsigned long long onm[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const int first = 64 * (wave + nact * c);
        cx[c] = cy[c] = cz[c] = nx[c] = ny[c] = nz[c] = 0.0;
        onm[c] = 0ull;
        if (first < k) { // (wave-uniform)
            shot_gather64<true>(rec, idx + s, first + lane, k, px, py, pz, cx[c], cy[c], cz[c], nx[c], ny[c], nz[c]);
            onm[c] = shot_chunk_mask(k - first);
        }
    }
    double raw[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    int xneg = 0, zneg = 0;
    if (FUSED) { // (read by every wave of the team before the barriers below, written back by one lane after them)
        // (scalar loads through the constant address space, pinned: see shot_cached_body)
        sf_const_doubles clr = (sf_const_doubles)(lrf + 9 * row);
#pragma unroll
        for (int i = 0; i < 9; ++i) raw[i] = clr[i];
#pragma unroll
        for (int i = 0; i < 9; ++i) asm volatile("" : "+s"(raw[i]));
#pragma unroll
        for (int c = 0; c < NCH; ++c)
            if (onm[c]) shot_count_votes(cx[c], cy[c], cz[c], raw, onm[c], xneg, zneg);
    }
    double d2[NCH];
    unsigned long long posm[NCH];
    int npos = 0;
#pragma unroll
    for (int c = 0; c < NCH; ++c) shot_gate(cx[c], cy[c], cz[c], onm[c], d2[c], posm[c], npos);
    if (lane == 0) {
        L.red[wave][0] = npos;
        L.red[wave][1] = xneg;
        L.red[wave][2] = zneg;
        L.red[wave][3] = 0;
    }
    __syncthreads(); // the cleared tables, the waves' counts
    npos = xneg = zneg = 0;
    for (int w = 0; w < nact; ++w) {
        const int4 part = *reinterpret_cast<const int4 *>(L.red[w]);
        npos += sf_uniform(part.x);
        xneg += sf_uniform(part.y);
        zneg += sf_uniform(part.z);
    }
    double E[9];
    if (FUSED) {
        if (shot_finish_frame(raw, k, xneg, zneg, E) && threadIdx.x == 0) {
#pragma unroll
            for (int i = 0; i < 9; ++i) lrf[9 * row + i] = E[i];
        }
    } else {
#pragma unroll
        for (int i = 0; i < 9; ++i) E[i] = lrf[9 * row + i];
    }
    if (!(npos > (int)min_nb)) { // (the same for every wave of the team)
        for (int b = threadIdx.x; b < SF_SHOT_LEN; b += nthr) o[b] = 0.0;
        return;
    }
    constexpr unsigned WON_B = 1u << 26, WON_G = 1u << 27, WON_A = 1u << 28, WON_CD = 1u << 29, WON_EF = 1u << 30;
    constexpr unsigned TIE = 1u << 25; // this lane met another holder of its winning key (shot_core.h)
    // ---- the three elections ----
    shot_kept g[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        g[c].bins1 = 0u;
        if (__builtin_amdgcn_inverse_ballot_w64(posm[c])) {
            shot_geometry<11>(cx[c], cy[c], cz[c], d2[c], nx[c], ny[c], nz[c], E, K.half_r, 11, 11.0, g[c]);
            atomicMax(&L.keyA[shot_slot_a<11>(g[c])], shot_key(g[c]));
            atomicMax(&L.keyB[shot_slot_b<11>(g[c])], shot_key(g[c]));
            atomicMax(&L.keyG[shot_slot_g<11>(g[c])], shot_key(g[c]));
        }
    }
    __syncthreads();
    // ---- who writes what: every key is read before the first winner replaces one by its value ----
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        if (__builtin_amdgcn_inverse_ballot_w64(posm[c])) {
            const unsigned long long key = shot_key(g[c]);
            const unsigned iA = shot_slot_a<11>(g[c]);
            const bool up = iA & 2u, odd = iA & 1u; // (bit 1 of a slot: z > 0, bit 0: outer shell)
            const unsigned long long own = L.keyA[iA], other_shell = L.keyA[iA ^ 1u], other_half = L.keyA[iA ^ 2u];
            unsigned f = 0u;
            if (own == key) {
                f = WON_A;
                if (shot_writes_cd(odd, other_shell)) f |= WON_CD;
                if (shot_writes_ef(key, other_half, up)) f |= WON_EF;
                if (other_half == key) f |= TIE;
            }
            if (L.keyB[shot_slot_b<11>(g[c])] == key) f |= WON_B;
            if (L.keyG[shot_slot_g<11>(g[c])] == key) f |= WON_G;
            g[c].bins1 |= f;
        }
    }
    __syncthreads();
    // ---- the winners' values: one claimed writer per slot ----
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        if (__builtin_amdgcn_inverse_ballot_w64(posm[c])) {
            const unsigned long long key = shot_key(g[c]);
            const unsigned iA = shot_slot_a<11>(g[c]);
            double vA, v_cd, v_ef, adth;
            shot_weights(g[c], K, vA, v_cd, v_ef, adth);
            const unsigned f = g[c].bins1;
            // (a holder of a winning key whose compare-and-swap finds the slot taken has met a tie: which of the two got there
            // first is a race between waves, and the row is computed again under the full order by k_shot_tied)
            bool met = f & TIE;
            if (f & WON_A) {
                if (atomicCAS(&L.keyA[iA], key, tag_value(vA)) == key) {
                    // (a bin receives at most one S3/S4 value -- from the winner of bin ^ 1 -- and one S6/S7 value -- from the
                    // winner of bin ^ 2: two addends into a slot that starts at +0 give the same sum in either order)
                    if ((f & WON_CD) && v_cd != 0.0) unsafeAtomicAdd(&L.vx[iA ^ 1u], v_cd);
                    if ((f & WON_EF) && v_ef != 0.0) unsafeAtomicAdd(&L.vx[iA ^ 2u], v_ef);
                } else {
                    met = true;
                }
            }
            if (f & WON_B) met |= atomicCAS(&L.keyB[shot_slot_b<11>(g[c])], key, tag_value(fabs(g[c].dc))) != key;
            if (f & WON_G) met |= atomicCAS(&L.keyG[shot_slot_g<11>(g[c])], key, tag_value(adth)) != key;
            if (met) L.red[0][3] = 1;
        }
    }
    __syncthreads();
    // ---- the row: wave 0 sums the four tables in a fixed order, takes the norm, scales and stores (the other waves are done:
    //      with three writers, each repeating the sums and the norm for a third of the stores, the launch took 6 % longer --
    //      the team is bound by the vector instructions it issues, like the cached form) ----
    if (wave != 0) return;
    if (L.red[0][3] && lane == 0) shot_report_tie(ties, q);
    double2 vals[3];
    double ss = 0.0;
#pragma unroll
    for (int u = 0; u < 3; ++u) {
        const int b = 2 * lane + 128 * u;
        vals[u] = make_double2(0.0, 0.0);
        if (b < 352) {
            const ulonglong2 a = *reinterpret_cast<const ulonglong2 *>(L.keyA + b);
            const ulonglong2 bb = *reinterpret_cast<const ulonglong2 *>(L.keyB + b);
            const ulonglong2 gg = *reinterpret_cast<const ulonglong2 *>(L.keyG + b);
            const double2 vx = *reinterpret_cast<const double2 *>(L.vx + b);
            vals[u].x = ((shot_untag(a.x) + vx.x) + shot_untag(bb.x)) + shot_untag(gg.x);
            vals[u].y = ((shot_untag(a.y) + vx.y) + shot_untag(bb.y)) + shot_untag(gg.y);
        }
        ss += vals[u].x * vals[u].x;
        ss += vals[u].y * vals[u].y;
    }
    const double scale = shot_row_scale(ss, normalize, false);
#pragma unroll
    for (int u = 0; u < 3; ++u) {
        const int b = 2 * lane + 128 * u;
        if (b < 352) sf_store_stream2(o + b, vals[u].x * scale, vals[u].y * scale);
    }
}

} // namespace

// launch K5 on resident buffers; FUSED: dlrf holds raw axes (k_shot_lrf raw mode) and receives the frames.
// Dispatch by list length, per keypoint (sf_nbrs_dispatch): the register-cached form of the main launch leaves out the
// keypoints whose own list exceeds it, and the team and streaming forms serve exactly those in launches of their own.
template <bool FUSED>
static int launch_shot_as(sf_ctx *ctx, sf_cloud *c, sf_nbrs *nb, double *dlrf, int normalize, int64_t min_nb_, double *dout)
{
    const int64_t m = nb->m;
    if (!m) return SF_OK;
    shot_consts K;
    int nmin;
    SF_CHECK(sf_shot_consts(ctx, nb->radius, min_nb_, &K, &nmin));
    const int64_t min_nb = nmin;
    const sf_dispatch d = sf_nbrs_dispatch(nb);
    const int32_t *const none = nullptr;
    // neighbours at equal distance: every form reports the keypoints whose elections met one, k_shot_tied computes their rows
    // again under the order (rho, caller index) -- shot_core.h
    sf_pool_guard tmp(ctx);
    shot_ties ties;
    SF_CHECK(sf_shot_ties_begin(ctx, tmp, m, &ties));
    const dim3 block(64 * SF_SHOT_WPB), block_streaming(64 * SF_SHOT_LONG_WPB);
#define SF_SHOT_ARGS c->rec, nb->qx, nb->qy, nb->qz, nb->offset, nb->count, nb->idx, nb->qrow, m, K, dlrf, normalize, min_nb, dout
    // the cached form over all m (sel = none) or over a selection; the streaming form likewise; the team of NW waves
#define SF_SHOT_CACHED(NAME, N, COUNT, LIMIT, SELP)                                                                  \
    SF_LAUNCH(ctx, NAME, (k_shot_cached<N, FUSED>), dim3(sf_xcd_grid(sf_div_up(COUNT, SF_SHOT_WPB))), block, SF_SHOT_ARGS, LIMIT, SELP, (int64_t)(COUNT), d.view_first, ties)
#define SF_SHOT_STREAM(NAME, SEL, COUNT, SELP, LO)                                                                    \
    SF_LAUNCH(ctx, NAME, (k_shot_long<FUSED, SEL>), dim3(sf_xcd_grid(sf_div_up(COUNT, SF_SHOT_LONG_WPB))), block_streaming, SF_SHOT_ARGS, SELP, (int64_t)(COUNT), d.view_first, LO, ties)
#define SF_SHOT_TEAM(NW)                                                                                              \
    SF_LAUNCH(ctx, "k5_shot_tail", (k_shot_team<SF_TEAM_NCH, NW, FUSED>), dim3(sf_xcd_grid(d.n_tail)), dim3(64 * NW), SF_SHOT_ARGS, d.tail_sel, d.n_tail, d.view_first, 255, ties)
    if (d.chunks == 1) { SF_SHOT_CACHED("k5_shot", 1, m, d.limit, none); }
    else if (d.chunks == 2) { SF_SHOT_CACHED("k5_shot", 2, m, d.limit, none); }
    else if (d.chunks == 3) { SF_SHOT_CACHED("k5_shot", 3, m, d.limit, none); }
    else if (d.chunks == 4) { SF_SHOT_CACHED("k5_shot", 4, m, d.limit, none); }
    else { SF_SHOT_STREAM("k5_shot", false, m, none, 0); }
    // the few lists that need more chunks than the bulk: the same form, four chunks
    if (d.n_mid) { SF_SHOT_CACHED("k5_shot_mid", 4, d.n_mid, 255, d.mid_sel); }
    if (d.n_tail) {
        // Lists above 255 points: a team of waves per keypoint while the list fits the team's registers (the longest list of
        // the search decides which team sizes are launched at all; every launch walks the selection and takes its own lengths),
        // the streaming form beyond.  Team size: the smallest that holds the longest list of the search (a shorter list uses as many
        // of the team's waves as it needs).
        const int64_t longest = nb->max_count > 255 ? nb->max_count : INT64_MAX; // (unknown: every form is launched)
        int64_t covered;
        if (longest <= 64 * SF_TEAM_NCH * 4) { SF_SHOT_TEAM(4); covered = 64 * SF_TEAM_NCH * 4; }
        else if (longest <= 64 * SF_TEAM_NCH * 8) { SF_SHOT_TEAM(8); covered = 64 * SF_TEAM_NCH * 8; }
        else { SF_SHOT_TEAM(16); covered = 64 * SF_TEAM_NCH * 16; }
        if (longest > covered) { SF_SHOT_STREAM("k5_shot_tail_stream", true, d.n_tail, d.tail_sel, (int)covered); }
    }
#undef SF_SHOT_TEAM
#undef SF_SHOT_STREAM
#undef SF_SHOT_CACHED
#undef SF_SHOT_ARGS
    return sf_shot_ties_finish<11>(ctx, c, nb, K, dlrf, FUSED, 11, normalize, dout, ties);
}

static int launch_shot(sf_ctx *ctx, sf_cloud *c, sf_nbrs *nb, double *dlrf, int normalize, int64_t min_nb, double *dout, bool fused)
{
    return fused ? launch_shot_as<true>(ctx, c, nb, dlrf, normalize, min_nb, dout)
                 : launch_shot_as<false>(ctx, c, nb, dlrf, normalize, min_nb, dout);
}

extern "C" int sf_shot(sf_ctx *ctx, sf_cloud *c, sf_nbrs *nb, const double *lrf, int normalize, int64_t min_nb,
                       double *out, int flags)
{
    SF_CHECK(check_nbrs(ctx, c, nb, "sf_shot"));
    if (!lrf || !out) { sf_set_error("sf_shot: null lrf/out"); return SF_ERR_ARG; }
    SF_CHECK(sf_cloud_ensure_sorted_normals(ctx, c));
    const int64_t m = nb->m;
    sf_pool_guard tmp(ctx);
    const double *dlrf;
    double *dout;
    SF_CHECK(stage_in(tmp, lrf, (size_t)m * 9, flags, &dlrf));
    SF_CHECK(stage_out(tmp, out, (size_t)m * SF_SHOT_LEN, flags, &dout));
    SF_CHECK(launch_shot(ctx, c, nb, const_cast<double *>(dlrf), normalize, min_nb, dout, false));
    SF_CHECK(finish_out(ctx, out, (size_t)m * SF_SHOT_LEN, flags, dout));
    return stage_sync(ctx, flags);
}

extern "C" int sf_azimuth_idx(sf_ctx *ctx, const double *x, const double *y, int64_t n, int64_t *idx, int flags)
{
    if (!ctx || !x || !y || !idx || n < 0) { sf_set_error("sf_azimuth_idx: bad argument"); return SF_ERR_ARG; }
    SF_HIP(hipSetDevice(ctx->device));
    sf_pool_guard tmp(ctx);
    const double *dx, *dy;
    SF_CHECK(stage_in(tmp, x, (size_t)n, flags, &dx));
    SF_CHECK(stage_in(tmp, y, (size_t)n, flags, &dy));
    int64_t *dout;
    SF_CHECK(stage_out(tmp, idx, (size_t)n, flags, &dout));
    if (n) { SF_LAUNCH(ctx, "k5_azimuth_idx", k_azimuth_idx, dim3((unsigned)sf_div_up(n, 256)), dim3(256), dx, dy, n, dout); }
    SF_CHECK(finish_out(ctx, idx, (size_t)n, flags, dout));
    return stage_sync(ctx, flags);
}

// compute_shot_descriptor, the reference's serial variant (shot.py:310-499): the frame of a keypoint is computed on its
// neighbours at NON-ZERO distance only (the keypoint itself and its duplicates are dropped first, :361-363) and the
// descriptor is always normalised (:496-497).  K4 with skip_zero, then the plain K5.
extern "C" int sf_shot_serial(sf_ctx *ctx, sf_cloud *c, sf_nbrs *nb, int64_t min_nb, double *out, int flags)
{
    SF_CHECK(check_nbrs(ctx, c, nb, "sf_shot_serial"));
    if (!out) { sf_set_error("sf_shot_serial: null out"); return SF_ERR_ARG; }
    SF_CHECK(sf_cloud_ensure_sorted_normals(ctx, c));
    const int64_t m = nb->m;
    sf_pool_guard guard(ctx);
    double *dlrf = nullptr, *dout;
    SF_CHECK(guard.alloc(&dlrf, (size_t)m * 9));
    SF_CHECK(stage_out(guard, out, (size_t)m * SF_SHOT_LEN, flags, &dout));
    SF_CHECK(sf_launch_shot_lrf(ctx, c, nb, 0, 1, dlrf));
    SF_CHECK(launch_shot(ctx, c, nb, dlrf, 1, min_nb, dout, false));
    SF_CHECK(finish_out(ctx, out, (size_t)m * SF_SHOT_LEN, flags, dout));
    return stage_sync_out(ctx, flags);
}

// Frames by `frames(dlrf)` (raw axes), then the fused K5, which votes on the neighbours it gathers anyway (the streaming K5
// votes too: no list is too long for the fused path).  lrf: where the frames go, or null.
template <class F>
static int shot_fused(sf_ctx *ctx, sf_cloud *c, sf_nbrs *nb, F frames, int normalize, int64_t min_nb, double *lrf, double *out,
                      int flags)
{
    SF_CHECK(sf_cloud_ensure_sorted_normals(ctx, c));
    const int64_t m = nb->m;
    const bool out_dev = flags & SF_OUT_DEVICE;
    sf_pool_guard tmp(ctx);
    double *dlrf = lrf, *dout;
    if (!out_dev || !lrf) SF_CHECK(tmp.alloc(&dlrf, (size_t)m * 9)); // frames wanted on the host, or not wanted at all: scratch on the device
    SF_CHECK(stage_out(tmp, out, (size_t)m * SF_SHOT_LEN, flags, &dout));
    SF_CHECK(frames(dlrf));
    SF_CHECK(launch_shot(ctx, c, nb, dlrf, normalize, min_nb, dout, true));
    if (lrf) SF_CHECK(finish_out(ctx, lrf, (size_t)m * 9, flags, dlrf));
    SF_CHECK(finish_out(ctx, out, (size_t)m * SF_SHOT_LEN, flags, dout));
    return stage_sync_out(ctx, flags);
}

// Single-scale SHOT in one go (shot_parallelization.py:135-183: frames and descriptor from the SAME search):
// K4 without its vote sweep, then the fused K5.
extern "C" int sf_shot_single_scale(sf_ctx *ctx, sf_cloud *c, sf_nbrs *nb, int normalize, int64_t min_nb, double *lrf,
                                    double *out, int flags)
{
    SF_CHECK(check_nbrs(ctx, c, nb, "sf_shot_single_scale"));
    if (!out) { sf_set_error("sf_shot_single_scale: null out"); return SF_ERR_ARG; }
    return shot_fused(ctx, c, nb, [&](double *dlrf) { return sf_launch_shot_lrf(ctx, c, nb, 1, 0, dlrf); }, normalize, min_nb, lrf, out, flags);
}

// sf_shot_single_scale with the frame moments already computed by sf_spfh_compute_moments on the SAME lists (self
// search; lists of any length: launch_shot dispatches per keypoint): eigen-solves only, then the fused K5.  cov: m x 6 on the device.
extern "C" int sf_shot_from_moments(sf_ctx *ctx, sf_cloud *c, sf_nbrs *nb, const double *cov_dev, int normalize, int64_t min_nb,
                                    double *lrf, double *out, int flags)
{
    SF_CHECK(check_nbrs(ctx, c, nb, "sf_shot_from_moments"));
    if (!out || !cov_dev) { sf_set_error("sf_shot_from_moments: null argument"); return SF_ERR_ARG; }
    if (nb->qrow) {
        sf_set_error("sf_shot_from_moments: needs a self search");
        return SF_ERR_UNSUPPORTED;
    }
    return shot_fused(ctx, c, nb, [&](double *dlrf) { return sf_launch_lrf_from_cov(ctx, cov_dev, nb->m, dlrf); }, normalize, min_nb, lrf, out, flags);
}

extern "C" int sf_shot_from_raw_lrf(sf_ctx *ctx, sf_cloud *c, sf_nbrs *nb, double *lrf_dev, int normalize, int64_t min_nb,
                                    double *out_dev)
{
    SF_CHECK(check_nbrs(ctx, c, nb, "sf_shot_from_raw_lrf"));
    if (!lrf_dev || !out_dev) { sf_set_error("sf_shot_from_raw_lrf: null argument"); return SF_ERR_ARG; }
    SF_CHECK(sf_cloud_ensure_sorted_normals(ctx, c));
    return launch_shot(ctx, c, nb, lrf_dev, normalize, min_nb, out_dev, true);
}

