// select.h -- the device-side entry of K18's radix selection (select.hip) for the chains that keep its result on the device.
#pragma once
#include "common.h"

// Queues the selection over keys_dev[0..n) (bit patterns of doubles, ordered with the sign bit cleared) on ctx->stream and leaves
// res_dev[8]: [0] the value, [1] keys below it, [2] keys at or below it, [3] 0, [4] n0 = the keys that are not all ones, [5] the rank
// used.  trim == 0: the given rank (1 .. n).  trim in (0, 1): rank = min(n0, max(1, ceil(trim * n0))) formed on the device; with
// n0 == 0 the rank is 0 and res_dev[0..3] are zero.  No host wait.
int sf_select_launch(sf_ctx *ctx, const uint64_t *keys_dev, int64_t n, int64_t rank, double trim, double *res_dev);
