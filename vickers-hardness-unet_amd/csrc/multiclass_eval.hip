// Validation metrics of a multi-label / multi-class model on the device: per (image, class) counts tp, fp, fn, tn and the
// reference's thresholded Dice / IoU (train.py:230-255 `dice_coef`, :259-281 `iou_coef`) generalised per class.
//
//   multilabel : pred_c = sigmoid(x_c) > threshold (x_c > threshold for probabilities), target fp32 [N][C][HW] in {0, 1};
//                another target value is a bad label: that (pixel, class) is skipped.
//   multiclass : pred = argmax_c x_c (ties to the lowest index), target int64 [N][HW]; a label outside [0, C) is a bad label:
//                the pixel is skipped.
//
// k_seg_counts_multi reads the logits (and the target) once.  Lanes run along the pixel axis; for every class a wave counts its 64 x VEC
// pixels with ballots (popcount(ballot(pred == c)), ballot(t == c), ballot(both), ballot(valid)): wave-uniform scalar counts, added
// once per step into lane c of four accumulator registers (no per-thread [C] array indexed at run time, no per-pixel LDS histogram
// atomics that would all hit the background bin).  A workgroup adds its four waves through LDS and issues one int64 atomic per
// (image, class, count).  The counts are integers: the result does not depend on the order of the atomics.
// k_seg_finalize_multi (one workgroup, as k_seg_finalize) turns them into fp / fn / tn and the scores.
#include "vk_common.h"

namespace vk {

constexpr int kMcMaxClasses = 16;
constexpr int kMcCounts = 4;   // per (image, class): tp, predicted, target, valid

__device__ __forceinline__ uint32_t popc(uint64_t m) { return (uint32_t)__popcll(m); }

// VEC: pixels per lane per step (4: 16-byte loads of every class plane; 1: the scalar path when HW % 4 != 0 or a plane is not aligned).
// MODE: VK_LOSS_MULTILABEL or VK_LOSS_MULTICLASS.
template <int VEC, int MODE, bool FROM_LOGITS>
__global__ __launch_bounds__(256) void k_seg_counts_multi(int C, int HW, const float* __restrict__ logits,
                                                          const void* __restrict__ target, float thr,
                                                          unsigned long long* __restrict__ counts, int* __restrict__ bad_labels) {
  const int img = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* x = logits + (size_t)img * C * HW;
  // lane c of the wave holds class c's four counters; a class's counts of one step (scalars from the ballots) are added into them
  // once per step, so only four scalar counters are live at a time whatever C is
  uint32_t acc[kMcCounts] = {0, 0, 0, 0};
  uint32_t bad = 0;
  auto flush = [&](int c, const uint32_t* n) {
#pragma unroll
    for (int k = 0; k < kMcCounts; ++k) acc[k] += lane == c ? n[k] : 0u;
  };
  // wave-uniform loop over chunks of 64 * VEC pixels: the trip count is the same in every lane, so the ballots see every lane and
  // the counts stay scalar; lanes past HW are masked out through `inb`
  const int chunk = 64 * VEC;
  for (int base = (blockIdx.x * 4 + wave) * chunk; base < HW; base += gridDim.x * 4 * chunk) {
    const int p0 = base + lane * VEC;
    bool inb[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) inb[e] = p0 + e < HW;
    if (MODE == VK_LOSS_MULTICLASS) {
      const int64_t* t = reinterpret_cast<const int64_t*>(target) + (size_t)img * HW;
      int64_t tv[VEC];
      float best[VEC] = {};
      int arg[VEC] = {};
      if constexpr (VEC == 4) {
        if (inb[0]) {                     // HW % 4 == 0 on this path: a lane's four pixels are all in or all out
          const u32x4_t a = *reinterpret_cast<const u32x4_t*>(t + p0), b = *reinterpret_cast<const u32x4_t*>(t + p0 + 2);
          tv[0] = (int64_t)(((uint64_t)a[1] << 32) | a[0]);
          tv[1] = (int64_t)(((uint64_t)a[3] << 32) | a[2]);
          tv[2] = (int64_t)(((uint64_t)b[1] << 32) | b[0]);
          tv[3] = (int64_t)(((uint64_t)b[3] << 32) | b[2]);
        } else {
#pragma unroll
          for (int e = 0; e < VEC; ++e) tv[e] = 0;
        }
      } else {
        tv[0] = inb[0] ? t[p0] : 0;
      }
      for (int c = 0; c < C; ++c) {
        float v[VEC];
        if constexpr (VEC == 4) {
          const f32x4_t q = inb[0] ? *reinterpret_cast<const f32x4_t*>(x + (size_t)c * HW + p0) : f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int e = 0; e < VEC; ++e) v[e] = q[e];
        } else {
          v[0] = inb[0] ? x[(size_t)c * HW + p0] : 0.f;
        }
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          if (c == 0 || v[e] > best[e]) { best[e] = v[e]; arg[e] = c; }     // strict: ties keep the lowest index
        }
      }
      uint64_t vm[VEC];
      int tl[VEC];
      uint32_t nvalid = 0;
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const bool valid = inb[e] && tv[e] >= 0 && tv[e] < C;
        vm[e] = __ballot(valid);
        nvalid += popc(vm[e]);
        bad += popc(__ballot(inb[e] && !valid));
        tl[e] = (int)tv[e];
      }
      for (int c = 0; c < C; ++c) {
        uint32_t n[kMcCounts] = {0, 0, 0, nvalid};
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          const uint64_t pm = __ballot(arg[e] == c) & vm[e], tm = __ballot(tl[e] == c) & vm[e];
          n[0] += popc(pm & tm);
          n[1] += popc(pm);
          n[2] += popc(tm);
        }
        flush(c, n);
      }
    } else {
      const float* t = reinterpret_cast<const float*>(target) + (size_t)img * C * HW;
      for (int c = 0; c < C; ++c) {
        float v[VEC], tv[VEC];
        if constexpr (VEC == 4) {
          const f32x4_t zero = {0.f, 0.f, 0.f, 0.f};
          const f32x4_t q = inb[0] ? *reinterpret_cast<const f32x4_t*>(x + (size_t)c * HW + p0) : zero;
          const f32x4_t r = inb[0] ? *reinterpret_cast<const f32x4_t*>(t + (size_t)c * HW + p0) : zero;
#pragma unroll
          for (int e = 0; e < VEC; ++e) { v[e] = q[e]; tv[e] = r[e]; }
        } else {
          v[0] = inb[0] ? x[(size_t)c * HW + p0] : 0.f;
          tv[0] = inb[0] ? t[(size_t)c * HW + p0] : 0.f;
        }
        uint32_t n[kMcCounts] = {0, 0, 0, 0};
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          const float pv = FROM_LOGITS ? 1.f / (1.f + expf(-v[e])) : v[e];   // as k_seg_counts
          const bool one = tv[e] == 1.f, valid = inb[e] && (one || tv[e] == 0.f);
          const uint64_t vm = __ballot(valid);
          const uint64_t pm = __ballot(pv > thr) & vm, tm = __ballot(one) & vm;
          bad += popc(__ballot(inb[e] && !valid));
          n[0] += popc(pm & tm);
          n[1] += popc(pm);
          n[2] += popc(tm);
          n[3] += popc(vm);
        }
        flush(c, n);
      }
    }
  }
  __shared__ uint32_t red[4][kMcMaxClasses][kMcCounts];
  __shared__ uint32_t red_bad[4];
  if (lane < C) {
#pragma unroll
    for (int k = 0; k < kMcCounts; ++k) red[wave][lane][k] = acc[k];
  }
  if (lane == 0) red_bad[wave] = bad;
  __syncthreads();
  if (threadIdx.x < C * kMcCounts) {
    const int c = threadIdx.x / kMcCounts, k = threadIdx.x % kMcCounts;
    const unsigned long long s = (unsigned long long)red[0][c][k] + red[1][c][k] + red[2][c][k] + red[3][c][k];
    if (s) atomicAdd(counts + ((size_t)img * C + c) * kMcCounts + k, s);
  }
  if (threadIdx.x == 0) {
    const int b = (int)(red_bad[0] + red_bad[1] + red_bad[2] + red_bad[3]);
    if (b) atomicAdd(bad_labels, b);
  }
}

// Scores per (image, class) in fp32 with the reference's operation order (k_seg_finalize's): I = tp, card = (tp + fp) + (tp + fn),
// dice = (2 I + eps) / (card + eps), iou = (I + eps) / ((card - I) + eps).  Batch score of a class: mean over images in fp64, rounded
// once, summed in k_seg_finalize's order (thread j takes images j, j + 64, ...; the 64 partials are added in j order), so C == 1
// reproduces vk_seg_metrics bit for bit.  Overall score: mean of the class scores in fp64, rounded once.
// out = [mean dice, mean iou, dice_c[C], iou_c[C], per_image[N][C][2]]; stats (optional) = [4][N][C] {tp, fp, fn, tn}.
__global__ __launch_bounds__(64) void k_seg_finalize_multi(int n, int C, const unsigned long long* __restrict__ counts, float eps,
                                                             float* __restrict__ out, int64_t* __restrict__ stats) {
  __shared__ double acc[kMcMaxClasses][2][64];
  __shared__ float cls[2][kMcMaxClasses];
  float* per_image = out + 2 + 2 * C;
  for (int c = 0; c < C; ++c) {
    double d = 0.0, u = 0.0;
    for (int i = threadIdx.x; i < n; i += 64) {
      const unsigned long long* q = counts + ((size_t)i * C + c) * kMcCounts;
      const int64_t tp = (int64_t)q[0], fp = (int64_t)q[1] - tp, fn = (int64_t)q[2] - tp, tn = (int64_t)q[3] - tp - fp - fn;
      if (stats) {
        const size_t o = (size_t)i * C + c, nc = (size_t)n * C;
        stats[o] = tp;
        stats[nc + o] = fp;
        stats[2 * nc + o] = fn;
        stats[3 * nc + o] = tn;
      }
      const float I = (float)tp;
      const float card = (float)(tp + fp) + (float)(tp + fn);
      const float dice = (2.f * I + eps) / (card + eps);
      const float iou = (I + eps) / ((card - I) + eps);
      per_image[((size_t)i * C + c) * 2] = dice;
      per_image[((size_t)i * C + c) * 2 + 1] = iou;
      d += (double)dice;
      u += (double)iou;
    }
    acc[c][0][threadIdx.x] = d;
    acc[c][1][threadIdx.x] = u;
  }
  __syncthreads();
  if (threadIdx.x < 2 * C) {
    const int c = threadIdx.x >> 1, k = threadIdx.x & 1;
    double s = 0.0;
    for (int j = 0; j < 64; ++j) s += acc[c][k][j];      // fixed order
    const float m = (float)(s / (double)n);
    out[2 + k * C + c] = m;
    cls[k][c] = m;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    double s = 0.0;
    for (int c = 0; c < C; ++c) s += (double)cls[threadIdx.x][c];
    out[threadIdx.x] = (float)(s / (double)C);
  }
}

template <int VEC>
static void launch_counts(int mode, bool from_logits, dim3 grid, hipStream_t st, int C, int HW, const float* logits,
                          const void* target, float thr, unsigned long long* counts, int* bad) {
  if (mode == VK_LOSS_MULTICLASS)
    hipLaunchKernelGGL((k_seg_counts_multi<VEC, VK_LOSS_MULTICLASS, true>), grid, dim3(256), 0, st, C, HW, logits, target, thr, counts, bad);
  else if (from_logits)
    hipLaunchKernelGGL((k_seg_counts_multi<VEC, VK_LOSS_MULTILABEL, true>), grid, dim3(256), 0, st, C, HW, logits, target, thr, counts, bad);
  else
    hipLaunchKernelGGL((k_seg_counts_multi<VEC, VK_LOSS_MULTILABEL, false>), grid, dim3(256), 0, st, C, HW, logits, target, thr, counts, bad);
}

}  // namespace vk

extern "C" size_t vk_seg_metrics_multi_workspace_bytes(int n_images, int C) {
  return n_images > 0 && C > 0 ? (size_t)n_images * C * vk::kMcCounts * sizeof(unsigned long long) : 0;
}

extern "C" int vk_seg_metrics_multi(int mode, int n_images, int C, size_t per_image, const float* logits, const void* target,
                                    int from_logits, float threshold, float eps, void* workspace, size_t workspace_bytes,
                                    int64_t* stats, float* out, int* bad_labels, void* stream) {
  using namespace vk;
  VK_CHECK_ARG(mode == VK_LOSS_MULTILABEL || mode == VK_LOSS_MULTICLASS, "vk_seg_metrics_multi: mode %d is neither multilabel (%d) "
               "nor multiclass (%d)", mode, VK_LOSS_MULTILABEL, VK_LOSS_MULTICLASS);
  VK_CHECK_ARG(C >= 1 && C <= kMcMaxClasses, "vk_seg_metrics_multi: C = %d outside [1, %d]", C, kMcMaxClasses);
  VK_CHECK_ARG(mode != VK_LOSS_MULTICLASS || C >= 2, "vk_seg_metrics_multi: multiclass needs C >= 2 (got %d)", C);
  VK_CHECK_ARG(n_images >= 1 && n_images <= 65535, "vk_seg_metrics_multi: n_images = %d outside [1, 65535]", n_images);
  VK_CHECK_ARG(per_image >= 1 && per_image <= (size_t)(INT32_MAX / kMcMaxClasses), "vk_seg_metrics_multi: per_image = %zu outside [1, %d]",
               per_image, INT32_MAX / kMcMaxClasses);
  VK_CHECK_ARG(logits && target && workspace && out && bad_labels, "vk_seg_metrics_multi: null buffer");
  VK_CHECK_ARG(workspace_bytes >= vk_seg_metrics_multi_workspace_bytes(n_images, C), "vk_seg_metrics_multi: workspace too small "
               "(%zu < %zu)", workspace_bytes, vk_seg_metrics_multi_workspace_bytes(n_images, C));
  VK_CHECK_ARG(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)target & (mode == VK_LOSS_MULTICLASS ? 7 : 3)) == 0 &&
               ((uintptr_t)logits & 3) == 0 && ((uintptr_t)stats & 7) == 0, "vk_seg_metrics_multi: misaligned buffer");
  hipStream_t st = (hipStream_t)stream;
  const int HW = (int)per_image;
  const double tbytes = mode == VK_LOSS_MULTICLASS ? 8.0 : 4.0 * C;
  vkh::ProfScope ps_("seg_metrics_multi", st, 0.0, (4.0 * C + tbytes) * (double)n_images * (double)HW);
  unsigned long long* counts = (unsigned long long*)workspace;
  VK_CHECK_HIP(hipMemsetAsync(counts, 0, vk_seg_metrics_multi_workspace_bytes(n_images, C), st));
  VK_CHECK_HIP(hipMemsetAsync(bad_labels, 0, sizeof(int), st));
  const bool vec = HW % 4 == 0 && (((uintptr_t)logits | (uintptr_t)target) & 15) == 0;
  // enough workgroups to fill the chip across the batch (about 2048 in all), each with at least ~4 steps of 1024 * VEC pixels
  const size_t per_wg = (size_t)256 * (vec ? 4 : 1) * 4;
  unsigned bx = (unsigned)((per_image + per_wg - 1) / per_wg);
  const unsigned cap = (unsigned)((2048 + n_images - 1) / n_images);
  if (bx > cap) bx = cap;
  if (bx < 1) bx = 1;
  const dim3 grid(bx, (unsigned)n_images);
  if (vec) launch_counts<4>(mode, from_logits != 0, grid, st, C, HW, logits, target, threshold, counts, bad_labels);
  else launch_counts<1>(mode, from_logits != 0, grid, st, C, HW, logits, target, threshold, counts, bad_labels);
  hipLaunchKernelGGL(k_seg_finalize_multi, dim3(1), dim3(64), 0, st, n_images, C, (const unsigned long long*)counts, eps, out, stats);
  VK_CHECK_HIP(hipGetLastError());
  return VK_OK;
}
