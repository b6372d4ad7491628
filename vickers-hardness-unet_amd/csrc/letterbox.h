// Letterbox geometry shared by the single-plane (prepost.hip) and class-plane (multiclass_post.hip) pre/post-processing kernels:
// the launch parameters, OpenCV's INTER_LINEAR source coordinates and the sigmoid, restated once so that every kernel rounds alike.
// Files that include this switch floating-point contraction off (the arithmetic must match the scalar CPU code).
#pragma once
#include "vk_common.h"

namespace vk {

struct LbParams {
  int h, w, stride, S, nh, nw, top, left, pad;
  int window;                   // post-processing: stage the transformed source window in LDS (large outputs)
  double scale_x, scale_y;      // 1 / (dst / src) in double, computed on the host as cv::resize does
};

// cv::resize linear coordinates: index of the left/top sample and the float weight of the right/bottom one
__device__ __forceinline__ void lin_coord(int d, double scale, int src, int& s, float& f) {
#pragma clang fp contract(off)
  const double t = ((double)d + 0.5) * scale;
  float fv = (float)(t - 0.5);
  int sv = (int)floorf(fv);
  fv -= (float)sv;
  if (sv < 0) { fv = 0.f; sv = 0; }
  if (sv >= src - 1) { fv = 0.f; sv = src - 1; }
  s = sv;
  f = fv;
}

__device__ __forceinline__ float sigmoidf(float x) {
#pragma clang fp contract(off)
  return 1.f / (1.f + expf(-x));
}

static inline int fill_params(const vk_letterbox_desc* d, LbParams& p, bool forward, const char* who) {
  VK_CHECK_ARG(d != nullptr, "%s: null descriptor", who);
  VK_CHECK_ARG(d->h > 0 && d->w > 0 && d->size > 0 && d->nh > 0 && d->nw > 0, "%s: non-positive size", who);
  VK_CHECK_ARG(d->top >= 0 && d->left >= 0 && d->top + d->nh <= d->size && d->left + d->nw <= d->size,
               "%s: the %dx%d resized image at (%d,%d) does not fit the %d-pixel square", who, d->nh, d->nw, d->top, d->left, d->size);
  VK_CHECK_ARG(d->h <= 16384 && d->w <= 16384 && d->size <= 16384, "%s: image side above 16384", who);
  VK_CHECK_ARG(d->pad_value >= 0 && d->pad_value <= 255, "%s: pad_value outside 0..255", who);
  p.h = d->h; p.w = d->w; p.stride = d->src_stride; p.S = d->size; p.nh = d->nh; p.nw = d->nw;
  p.top = d->top; p.left = d->left; p.pad = d->pad_value;
  p.window = 1;
  if (forward) {   // original -> resized
    p.scale_x = 1.0 / ((double)d->nw / (double)d->w);
    p.scale_y = 1.0 / ((double)d->nh / (double)d->h);
  } else {         // resized crop -> original
    p.scale_x = 1.0 / ((double)d->w / (double)d->nw);
    p.scale_y = 1.0 / ((double)d->h / (double)d->nh);
  }
  return VK_OK;
}

}  // namespace vk
