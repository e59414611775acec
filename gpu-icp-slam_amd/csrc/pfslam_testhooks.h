/*
 * pfslam_testhooks.h -- NOT part of the installed interface (include/pfslam.h).  Entry points that exist only so that
 * tests/ can check device-side arithmetic against the oracle; exported from libpfslam_hip.so, declared here.
 */
#ifndef PFSLAM_TESTHOOKS_H
#define PFSLAM_TESTHOOKS_H
#include "../../include/pfslam.h"
#ifdef __cplusplus
extern "C" {
#endif
/* evaluate the bit-reproducible math specification (pf_math.h) on the device.
 * which: 0 sincos (out: n x {sin, cos}), 1 erfcinv, 2 asin, 3 rsqrt, 4 sqrt_rn, 5 x / 0.025f,
 *        6 sub-cell index of x on the 0.025 m lattice (out: n x {sub_index, sub_index_fast or INT_MIN when not safe}, int bits),
 *        8 the same as 6 on the lattice of resolution in_host[0] (in_host[0] is also query 0) */
int pfslam_debug_math(pfslam_handle *h, int which, const float *in_host, int n, float *out_host);
/* pfslam_search_wide's and pfslam_search_best's frontier buffers hold `nodes` nodes each from the next call on (0 = the default, 2^22; at least 4), so that a small
 * window is cut into many batches.  Results do not depend on it. */
int pfslam_debug_search_frontier(pfslam_handle *h, int nodes);
#ifdef __cplusplus
}
#endif
#endif
