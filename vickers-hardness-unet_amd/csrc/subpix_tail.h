// The tail of a vk_subpix_quad record, written by one thread: what vk_subpix_refine (subpix.hip) and vk_kp_refine (keypoints.hip) share,
// so that the two calls leave the same bytes for the same vertices.  IEEE float64 with contraction off, as include/vk_unet.h states it.
#pragma once
#include "vk_common.h"

#include <math.h>

#pragma clang fp contract(off)

namespace vk {

// a record with valid == 0: label, area, and zeros in every other field
__device__ __forceinline__ void sp_write_invalid(vk_subpix_quad* __restrict__ dst, const char* __restrict__ rec) {
  dst->label = reinterpret_cast<const int*>(rec)[0];
  dst->area = reinterpret_cast<const int*>(rec)[1];
  dst->valid = 0;
  dst->reserved = 0;
  for (int q = 0; q < 4; ++q) { dst->flags[q] = 0; dst->iters[q] = 0; }
  for (int q = 0; q < 8; ++q) { dst->v[q] = 0.0; dst->vs[q] = 0.0; }
  dst->d1 = 0.0;
  dst->d2 = 0.0;
  dst->d_mean = 0.0;
}

// vx, vy, fl, it: the four vertices (LDS or registers); affine: [batch][3] or null
__device__ __forceinline__ void sp_write_record(vk_subpix_quad* __restrict__ dst, const char* __restrict__ rec, const double* __restrict__ affine,
                                                int b, const double* vx, const double* vy, const int* fl, const int* it) {
#pragma clang fp contract(off)
  double ox = 0.0, oy = 0.0, inv = 1.0;
  if (affine) { ox = affine[3 * (size_t)b]; oy = affine[3 * (size_t)b + 1]; inv = affine[3 * (size_t)b + 2]; }
  dst->label = reinterpret_cast<const int*>(rec)[0];
  dst->area = reinterpret_cast<const int*>(rec)[1];
  dst->valid = 1;
  dst->reserved = 0;
  for (int q = 0; q < 4; ++q) {
    dst->flags[q] = fl[q];
    dst->iters[q] = it[q];
    dst->v[2 * q] = vx[q];
    dst->v[2 * q + 1] = vy[q];
    dst->vs[2 * q] = (vx[q] - ox) * inv;
    dst->vs[2 * q + 1] = (vy[q] - oy) * inv;
  }
  // the geometry records' rule: the longest of the six pairs (the first on a tie), then the other two vertices
  double dmax = -1.0;
  int i1 = 0, j1 = 1;
  for (int a = 0; a < 4; ++a)
    for (int c = a + 1; c < 4; ++c) {
      const double ddx = vx[a] - vx[c], ddy = vy[a] - vy[c];
      const double d = sqrt(ddx * ddx + ddy * ddy);
      if (d > dmax) { dmax = d; i1 = a; j1 = c; }
    }
  int r0 = -1, r1 = -1;
  for (int q = 0; q < 4; ++q)
    if (q != i1 && q != j1) { if (r0 < 0) r0 = q; else r1 = q; }
  const double ex = vx[r0] - vx[r1], ey = vy[r0] - vy[r1];
  const double d1 = dmax * inv;
  const double d2 = sqrt(ex * ex + ey * ey) * inv;
  dst->d1 = d1;
  dst->d2 = d2;
  dst->d_mean = 0.5 * (d1 + d2);
}

}  // namespace vk
