// The sigmoid pieces of one logit, shared by the pixel-wise loss kernels (seg_loss.hip, kp_loss.hip): one implementation, so a term
// that both files evaluate gives the same bits in either.
#pragma once
#include <math.h>

#include "vk_common.h"

namespace vk {

// sigmoid pieces of one logit without overflow: e = exp(-|x|), l1p = log1p(e), p = sigmoid(x), omp = 1 - p
struct SlSig {
  float e, l1p, p, omp;
};
__device__ __forceinline__ SlSig sl_sigmoid(float x) {
  SlSig s;
  s.e = expf(-fabsf(x));
  s.l1p = log1pf(s.e);
  const float r = 1.f / (1.f + s.e);
  s.p = x >= 0.f ? r : s.e * r;
  s.omp = x >= 0.f ? s.e * r : r;
  return s;
}

}  // namespace vk
