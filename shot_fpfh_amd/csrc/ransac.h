// ransac.h -- what ransac.hip (K11) lends to the other estimators that rank fitted transforms (K15, consistency.hip): the layout
// of the refit sums and the back half of K11 (order-preserving compaction, first maximum).  Stated at the definitions.
#pragma once
#include "common.h"

// the 24 doubles of sf_ransac_refit_sums, which sf_sc2_seed_fits writes per seed too
enum { RS_COUNT = 0, RS_ABAR = 1, RS_BBAR = 4, RS_H = 7, RS_SSR = 16, RS_SUM_A = 17, RS_SUM_B = 20, RS_SPARE = 23, RS_SIZE = 24 };

#ifdef __HIPCC__
// One pair (p, q) into the accumulators of a Kabsch fit, the order and the expressions of every kernel that forms one.
// Pass 0: the count, sum p, sum q.  Pass 1: the nine products centred with mean = {pbar, qbar}, row-major.
template <int NV>
__device__ __forceinline__ void sf_refit_add_pair(double (&acc)[NV], double px, double py, double pz, double qx, double qy, double qz)
{
    acc[0] += 1.0;
    acc[1] += px; acc[2] += py; acc[3] += pz;
    acc[4] += qx; acc[5] += qy; acc[6] += qz;
}
template <int NV>
__device__ __forceinline__ void sf_refit_add_centred(double (&acc)[NV], const double (&mean)[6], double px, double py, double pz,
                                                     double qx, double qy, double qz)
{
    const double ux = px - mean[0], uy = py - mean[1], uz = pz - mean[2];
    const double vx = qx - mean[3], vy = qy - mean[4], vz = qz - mean[5];
    acc[0] += ux * vx; acc[1] += ux * vy; acc[2] += ux * vz;
    acc[3] += uy * vx; acc[4] += uy * vy; acc[5] += uy * vz;
    acc[6] += uz * vx; acc[7] += uz * vy; acc[8] += uz * vz;
}
#endif

int64_t sf_k11_blocks(int64_t n);
int sf_k11_compact(sf_ctx *ctx, const unsigned char *status, const double *Rt_all, int64_t n, double *Rt_out, int64_t *map,
                   int *block_count, int64_t *block_off, unsigned long long *tallies);
int sf_k11_first_max(sf_ctx *ctx, const int64_t *counts, int64_t n, const int64_t *map, const double *Rt, int64_t *win, double *best_rt);
