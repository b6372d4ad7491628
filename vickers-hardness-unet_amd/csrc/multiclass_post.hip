// Inference post-processing of a C-class logit map [C][S][S] (fp32 class planes), the class-plane counterparts of prepost.hip's
// k_letterbox_mask / k_letterbox_post, with the same descriptor, coordinate mapping and arithmetic:
//
//   k_letterbox_post_multi<MC_LABELS>  argmax over the classes at the model's resolution (ties to the lowest index), crop,
//                                      INTER_NEAREST to uint8 [h][w]: decide, then resize, as predict_mask does (infer_pth_gui.py:50-53)
//   k_letterbox_post_multi<MC_MASKS>   per class (sigmoid >= thresh) * 255, crop, INTER_NEAREST to uint8 [C][h][w]
//   k_letterbox_prob_multi<false>      per class sigmoid, crop, INTER_LINEAR (a copy when the crop has the original size), clip [0,1]
//                                      -> fp32 [C][h][w]
//   k_letterbox_prob_multi<true>       the same with softmax over the classes at each source pixel: shift by the max, expf, sum in
//                                      class order, divide
//
// Labels / masks: a thread owns 4 consecutive pixels of one output row and writes them in every class plane (4-byte stores when the
// width allows, lanes along x); each output pixel reads one source pixel per class, so there is nothing to share.
// Probabilities: a bilinear upsample reads every source pixel from ~4 x (scale^2) output pixels (about 6 x 6 at 3072 x 2048 from a
// 512 crop), so evaluating the class transform at every tap repeats the expf (and, for softmax, the 2 C loads of the normaliser) tens
// of times.  As in k_letterbox_post, a workgroup owns a 256 x 16 block of the output and transforms the source window of that block
// ONCE into LDS (softmax: max and sum over the C planes first, then one class plane at a time), then interpolates from LDS; windows
// above PM_WIN samples (strong reductions, small outputs) fall back to per-tap evaluation.  The numbers are the same either way.
// With C == 1 every mode reproduces the single-plane kernels bit for bit (same expressions, contraction off).
#include "letterbox.h"

#pragma clang fp contract(off)

namespace vk {

enum { MC_LABELS = 0, MC_MASKS = 1, MC_SIGMOID = 2, MC_SOFTMAX = 3 };

// softmax normaliser of one source pixel: max over the classes and the class-order sum of expf(x_c - max)
__device__ __forceinline__ void softmax_norm(const float* __restrict__ px, size_t plane, int C, float& m, float& s) {
#pragma clang fp contract(off)
  m = px[0];
  for (int c = 1; c < C; ++c) m = fmaxf(m, px[(size_t)c * plane]);
  s = 0.f;
  for (int c = 0; c < C; ++c) s += expf(px[(size_t)c * plane] - m);
}

template <int MODE>
__global__ __launch_bounds__(256) void k_letterbox_post_multi(const LbParams p, int C, const float* __restrict__ logits,
                                                              float thresh, void* __restrict__ outv) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int y = blockIdx.y * 4 + wave;
  const int x0 = blockIdx.x * 256 + lane * 4;
  if (y >= p.h || x0 >= p.w) return;
  const size_t plane = (size_t)p.S * p.S, oplane = (size_t)p.h * p.w;
  const float* base = logits + (size_t)p.top * p.S + p.left;
  const bool vec = (p.w & 3) == 0 && (reinterpret_cast<uintptr_t>(outv) & 15) == 0;      // x0 + 3 < w, aligned vector stores
  const bool same = p.nh == p.h && p.nw == p.w;

  if (MODE == MC_LABELS || MODE == MC_MASKS) {
    // nearest source pixel of each of the 4 outputs (resizeNN from the nh x nw crop to h x w)
    int sy = y, sx[4];
    if (!same) sy = min((int)floor((double)y * p.scale_y), p.nh - 1);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int x = min(x0 + j, p.w - 1);
      sx[j] = same ? x : min((int)floor((double)x * p.scale_x), p.nw - 1);
    }
    const float* row = base + (size_t)sy * p.S;
    auto store = [&](uint8_t* out, const uint32_t* m) {
      if (vec) {
        *reinterpret_cast<uint32_t*>(out) = m[0] | (m[1] << 8) | (m[2] << 16) | (m[3] << 24);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (x0 + j < p.w) out[j] = (uint8_t)m[j];
      }
    };
    uint8_t* out = reinterpret_cast<uint8_t*>(outv) + (size_t)y * p.w + x0;
    if (MODE == MC_LABELS) {
      float best[4];
      uint32_t arg[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) { best[j] = row[sx[j]]; arg[j] = 0; }
      for (int c = 1; c < C; ++c) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float v = row[(size_t)c * plane + sx[j]];
          if (v > best[j]) { best[j] = v; arg[j] = (uint32_t)c; }         // strict: ties keep the lowest index
        }
      }
      store(out, arg);
    } else {
      for (int c = 0; c < C; ++c) {
        uint32_t m[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) m[j] = sigmoidf(row[(size_t)c * plane + sx[j]]) >= thresh ? 255u : 0u;
        store(out + (size_t)c * oplane, m);
      }
    }
  }
}

constexpr int PM_BW = 256, PM_BH = 16, PM_WIN = 4096;

// the transform of class c at one source pixel, evaluated in place (the fallback for windows above PM_WIN)
template <bool SOFTMAX>
__device__ __forceinline__ float prob_at(const float* __restrict__ px, size_t plane, int C, int c) {
#pragma clang fp contract(off)
  const float l = px[(size_t)c * plane];
  if (!SOFTMAX) return sigmoidf(l);
  float m, s;
  softmax_norm(px, plane, C, m, s);
  return expf(l - m) / s;
}

// the 4 x 4 outputs of one thread in class plane c from a tap function; UNROLL = false for the per-tap fallback, whose taps each
// carry the C-plane softmax normaliser (one copy of that code instead of 64)
template <bool UNROLL, typename Tap>
__device__ __forceinline__ void interp_store(const LbParams& p, bool same, bool vec, int x0, int y0, const int* sx, const int* sx1,
                                             const float* fx, const int* sy, const int* sy1, const float* fy, float* dst_plane, Tap tap) {
#pragma clang fp contract(off)
  constexpr int kUnroll = UNROLL ? 4 : 1;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int y = y0 + i;
    if (y >= p.h) break;
    float o[4];
#pragma unroll kUnroll
    for (int j = 0; j < 4; ++j) {
      float v;
      if (same) {
        v = tap(sy[i], sx[j]);
      } else {
        const float a0 = 1.f - fx[j], a1 = fx[j], b0 = 1.f - fy[i], b1 = fy[i];
        const float h0 = tap(sy[i], sx[j]) * a0 + tap(sy[i], sx1[j]) * a1;
        const float h1 = tap(sy1[i], sx[j]) * a0 + tap(sy1[i], sx1[j]) * a1;
        v = h0 * b0 + h1 * b1;
      }
      o[j] = fminf(fmaxf(v, 0.f), 1.f);
    }
    float* dst = dst_plane + (size_t)y * p.w + x0;
    if (vec) {
      *reinterpret_cast<f32x4_t*>(dst) = f32x4_t{o[0], o[1], o[2], o[3]};
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (x0 + j < p.w) dst[j] = o[j];
    }
  }
}

template <bool SOFTMAX>
__global__ __launch_bounds__(256) void k_letterbox_prob_multi(const LbParams p, int C, const float* __restrict__ logits,
                                                              float* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ float win[PM_WIN];                        // class plane c of the window, transformed
  __shared__ float nrm[SOFTMAX ? 2 : 1][SOFTMAX ? PM_WIN : 1];      // softmax: max and sum over the classes per window sample
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int bx0 = blockIdx.x * PM_BW, by0 = blockIdx.y * PM_BH;
  const int bx1 = min(bx0 + PM_BW, p.w) - 1, by1 = min(by0 + PM_BH, p.h) - 1;      // last pixel of this block (inclusive)
  const size_t plane = (size_t)p.S * p.S, oplane = (size_t)p.h * p.w;
  const float* base = logits + (size_t)p.top * p.S + p.left;
  const bool same = p.nh == p.h && p.nw == p.w;

  // source window of the block (coordinates are monotone in the destination index)
  int wx0 = bx0, wx1 = bx1, wy0 = by0, wy1 = by1;
  if (!same) {
    float f;
    lin_coord(bx0, p.scale_x, p.nw, wx0, f);
    lin_coord(bx1, p.scale_x, p.nw, wx1, f);
    lin_coord(by0, p.scale_y, p.nh, wy0, f);
    lin_coord(by1, p.scale_y, p.nh, wy1, f);
    wx1 = min(wx1 + 1, p.nw - 1);
    wy1 = min(wy1 + 1, p.nh - 1);
  }
  const int nx = wx1 - wx0 + 1, ny = wy1 - wy0 + 1;
  const bool windowed = nx * ny <= PM_WIN;            // workgroup-uniform

  // this thread's 4 pixels in 4 rows, their taps and weights
  const int x0 = bx0 + lane * 4;
  const bool active = x0 < p.w;
  int sx[4], sx1[4], sy[4], sy1[4];
  float fx[4], fy[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int x = min(x0 + j, p.w - 1), y = min(by0 + wave * 4 + j, p.h - 1);
    sx[j] = sx1[j] = x;
    sy[j] = sy1[j] = y;
    fx[j] = fy[j] = 0.f;
    if (!same) {
      lin_coord(x, p.scale_x, p.nw, sx[j], fx[j]);
      sx1[j] = min(sx[j] + 1, p.nw - 1);
      lin_coord(y, p.scale_y, p.nh, sy[j], fy[j]);
      sy1[j] = min(sy[j] + 1, p.nh - 1);
    }
  }
  const bool vec = (p.w & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;      // x0 + 3 < w, aligned vector stores

  if (SOFTMAX && windowed) {
    for (int i = threadIdx.x; i < nx * ny; i += 256) {
      float m, s;
      softmax_norm(base + (size_t)(wy0 + i / nx) * p.S + wx0 + i % nx, plane, C, m, s);
      nrm[0][i] = m;
      nrm[SOFTMAX ? 1 : 0][i] = s;
    }
  }
  for (int c = 0; c < C; ++c) {
    const float* bc = base + (size_t)c * plane;
    if (windowed) {
      __syncthreads();                                 // the normalisers are written / the previous plane is read
      for (int i = threadIdx.x; i < nx * ny; i += 256) {
        const float l = bc[(size_t)(wy0 + i / nx) * p.S + wx0 + i % nx];
        win[i] = SOFTMAX ? expf(l - nrm[0][i]) / nrm[SOFTMAX ? 1 : 0][i] : sigmoidf(l);
      }
      __syncthreads();
    }
    if (!active) continue;
    float* dst = out + (size_t)c * oplane;
    if (windowed)
      interp_store<true>(p, same, vec, x0, by0 + wave * 4, sx, sx1, fx, sy, sy1, fy, dst,
                         [&](int ty, int tx) { return win[(ty - wy0) * nx + (tx - wx0)]; });
    else
      interp_store<false>(p, same, vec, x0, by0 + wave * 4, sx, sx1, fx, sy, sy1, fy, dst,
                          [&](int ty, int tx) { return prob_at<SOFTMAX>(base + (size_t)ty * p.S + tx, plane, C, c); });
  }
}

static int mc_post(const char* who, const vk_letterbox_desc* d, int C, const float* logits, void* out, int mode, float thresh,
                   double out_bytes_per_pixel, void* stream) {
  LbParams p;
  int rc = fill_params(d, p, false, who);
  if (rc != VK_OK) return rc;
  VK_CHECK_ARG(C >= 1 && C <= 16, "%s: C = %d outside [1, 16]", who, C);
  VK_CHECK_ARG(logits && out, "%s: null buffer", who);
  hipStream_t st = (hipStream_t)stream;
  const double px = (double)d->h * d->w, src = fmin((double)d->nh * d->nw, px);
  vkh::ProfScope ps(who, st, 0.0, 4.0 * C * src + out_bytes_per_pixel * px);
  const dim3 block(256);
  if (mode == MC_LABELS || mode == MC_MASKS) {
    const dim3 grid((d->w + 255) / 256, (d->h + 3) / 4);
    if (mode == MC_LABELS) hipLaunchKernelGGL(k_letterbox_post_multi<MC_LABELS>, grid, block, 0, st, p, C, logits, thresh, out);
    else hipLaunchKernelGGL(k_letterbox_post_multi<MC_MASKS>, grid, block, 0, st, p, C, logits, thresh, out);
  } else {
    const dim3 grid((d->w + PM_BW - 1) / PM_BW, (d->h + PM_BH - 1) / PM_BH);
    if (mode == MC_SOFTMAX) hipLaunchKernelGGL(k_letterbox_prob_multi<true>, grid, block, 0, st, p, C, logits, (float*)out);
    else hipLaunchKernelGGL(k_letterbox_prob_multi<false>, grid, block, 0, st, p, C, logits, (float*)out);
  }
  VK_CHECK_HIP(hipGetLastError());
  return VK_OK;
}

}  // namespace vk

using namespace vk;

extern "C" int vk_letterbox_postprocess_labels(const vk_letterbox_desc* d, int C, const float* logits, uint8_t* labels_hw, void* stream) {
  return mc_post("vk_letterbox_postprocess_labels", d, C, logits, labels_hw, MC_LABELS, 0.f, 1.0, stream);
}

extern "C" int vk_letterbox_postprocess_mask_multi(const vk_letterbox_desc* d, int C, const float* logits, float thresh, uint8_t* masks_chw,
                                                   void* stream) {
  return mc_post("vk_letterbox_postprocess_mask_multi", d, C, logits, masks_chw, MC_MASKS, thresh, 1.0 * C, stream);
}

extern "C" int vk_letterbox_postprocess_prob_multi(const vk_letterbox_desc* d, int C, int mode, const float* logits, float* probs_chw,
                                                   void* stream) {
  VK_CHECK_ARG(mode == VK_LOSS_MULTILABEL || mode == VK_LOSS_MULTICLASS, "vk_letterbox_postprocess_prob_multi: mode %d is neither "
               "multilabel (%d) nor multiclass (%d)", mode, VK_LOSS_MULTILABEL, VK_LOSS_MULTICLASS);
  VK_CHECK_ARG(mode != VK_LOSS_MULTICLASS || C >= 2, "vk_letterbox_postprocess_prob_multi: multiclass needs C >= 2 (got %d)", C);
  return mc_post("vk_letterbox_postprocess_prob_multi", d, C, logits, probs_chw, mode == VK_LOSS_MULTICLASS ? MC_SOFTMAX : MC_SIGMOID,
                 0.f, 4.0 * C, stream);
}
