// Threshold sweep of the validation metrics: every threshold's Dice / IoU / precision-recall point from ONE pass over prediction and
// target (the reference's dice_coef / iou_coef, train.py:230-281, evaluate one hand-picked threshold per call).
//
//   pass 1, k_sweep_hist: per plane (one class map of one image) a histogram of the prediction over the threshold grid, split by
//     target value: hist[plane][t][b], t in {0, 1}, b = #{k : pv > thr[k]} in [0, K].  Its suffix sums are the exact integer counts
//     {I, P, T} of k_seg_counts for every threshold at once.  HBM-bound: 8 B per element (5 B with uint8 targets), nothing written
//     but the histogram.
//   pass 2, k_sweep_suffix / k_sweep_mean / k_sweep_summary: suffix sums, then k_seg_finalize_multi's expressions per threshold, the
//     micro-averaged precision / recall / F1 / IoU / FPR curve, AP, ROC-AUC and the best thresholds.  Small and latency-bound.
//
// The end bins.  A trained network's map is saturated almost everywhere, so nearly every element lands in bin 0 or bin K and an LDS
// histogram would serialise its atomics on two addresses per target value.  Those four (target, end bin) cases are classified first
// (two compares against thr[0] and thr[K-1]) and counted in registers; only the remainder searches the thresholds (in LDS) and does
// an integer LDS atomic into the workgroup's histogram, which leaves as one integer global atomic per non-zero bin: integers only, so
// the result does not depend on any order.  (One histogram per workgroup, not one per wave: four copies cost four times the zeroing
// and flushing and a quarter of the resident workgroups at K = 1024; profiles/sweep/README.md has both measured.)
//
// Whatever arrives as a device array may hold garbage (thresholds out of order, groups out of range, negative bins): every index
// formed from such a value is bounded by construction, so the result is then meaningless but no access leaves its buffer.
#include "vk_common.h"

#include <math.h>

#pragma clang fp contract(off)

namespace vk {

constexpr int kSweepMaxK = 1024;
constexpr int kSweepMaxClasses = 16;
constexpr int kSweepMaxPlanes = 1 << 20;
constexpr int kSweepMaxImages = 65535;

// ------------------------------------------------------------------------------------------------ pass 1: histogram
template <typename TT> struct SweepTarget;
template <> struct SweepTarget<float> {
  static __device__ __forceinline__ void load4(const float* p, float* v) {
    const f32x4_t q = *reinterpret_cast<const f32x4_t*>(p);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = q[e];
  }
};
template <> struct SweepTarget<uint8_t> {
  static __device__ __forceinline__ void unpack(uint32_t w, float* v) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (float)((w >> (8 * e)) & 0xffu);
  }
  static __device__ __forceinline__ void load4(const uint8_t* p, float* v) { unpack(*reinterpret_cast<const uint32_t*>(p), v); }
};

// VEC elements per thread and step: 4 (one 16-byte load of each fp32 tensor; a 4-byte load of a uint8 target), 1 (any alignment, any
// length).  The vector path needs per_plane % 4 == 0, so it has no tail.  A target value (uint8 or fp32) is compared as a float: every
// uint8 is exact there.  (16 elements per step with one 16-byte load of a uint8 target measured slower than this: profiles/sweep.)
template <typename TT, int VEC, bool FROM_LOGITS>
__global__ __launch_bounds__(256) void k_sweep_hist(size_t per_plane, size_t stride, unsigned bx, const float* __restrict__ pred,
                                                    const TT* __restrict__ target, int K, const float* __restrict__ thr_dev,
                                                    int has_ignore, float ignore_value, int* __restrict__ hist, int* __restrict__ bad_out) {
  extern __shared__ int smem[];
  const int B = K + 1;
  float* thr = reinterpret_cast<float*>(smem);              // [K]
  int* h = smem + K;                                        // [2][B], shared by the four waves
  __shared__ int sbad;
  const int tid = threadIdx.x;
  for (int i = tid; i < K; i += 256) thr[i] = thr_dev[i];
  for (int i = tid; i < 2 * B; i += 256) h[i] = 0;
  if (tid == 0) sbad = 0;
  __syncthreads();
  const size_t plane = blockIdx.x / bx;
  const unsigned chunk = blockIdx.x % bx;
  const float* p = pred + plane * stride;
  const TT* t = target + plane * stride;
  const float thr_lo = thr[0], thr_hi = thr[K - 1];
  uint32_t c_lo0 = 0, c_lo1 = 0, c_hi0 = 0, c_hi1 = 0, badc = 0;
  auto one = [&](float x, float tv) {
    const float pv = FROM_LOGITS ? 1.f / (1.f + expf(-x)) : x;          // as k_seg_counts
    const bool ign = has_ignore && tv == ignore_value;
    const bool pos = tv == 1.f, valid = !ign && (pos || tv == 0.f);
    badc += (!ign && !valid) ? 1u : 0u;
    const bool above = pv > thr_lo;                                     // NaN: false, bin 0
    const bool hi = above && pv > thr_hi, lo = !above;
    c_lo0 += (valid && lo && !pos) ? 1u : 0u;
    c_lo1 += (valid && lo && pos) ? 1u : 0u;
    c_hi0 += (valid && hi && !pos) ? 1u : 0u;
    c_hi1 += (valid && hi && pos) ? 1u : 0u;
    if (valid && above && !hi) {
      // #{k : thr[k] < pv}: every probe index is in [0, K) whatever thr holds
      int lo_i = 0, n = K;
      while (n > 0) {
        const int half = n >> 1, mid = lo_i + half;
        if (thr[mid] < pv) { lo_i = mid + 1; n -= half + 1; } else { n = half; }
      }
      atomicAdd(h + (pos ? B : 0) + lo_i, 1);
    }
  };
  const size_t nstep = per_plane / VEC, step = (size_t)bx * 256;
  auto load = [&](size_t i, float* pv, float* tv) {
    if constexpr (VEC == 4) {
      SweepTarget<float>::load4(p + 4 * i, pv);
      SweepTarget<TT>::load4(t + 4 * i, tv);
    } else {
      pv[0] = p[i];
      tv[0] = (float)t[i];
    }
  };
  for (size_t i = (size_t)chunk * 256 + tid; i < nstep; i += step) {
    float pv[VEC], tv[VEC];
    load(i, pv, tv);
#pragma unroll
    for (int e = 0; e < VEC; ++e) one(pv[e], tv[e]);
  }
  if (c_lo0) atomicAdd(h, (int)c_lo0);
  if (c_lo1) atomicAdd(h + B, (int)c_lo1);
  if (c_hi0) atomicAdd(h + K, (int)c_hi0);
  if (c_hi1) atomicAdd(h + B + K, (int)c_hi1);
  if (badc) atomicAdd(&sbad, (int)badc);
  __syncthreads();
  int* out = hist + plane * 2 * (size_t)B;
  for (int i = tid; i < 2 * B; i += 256) {
    const int s = h[i];
    if (s) atomicAdd(out + i, s);
  }
  if (tid == 0 && sbad) atomicAdd(bad_out, sbad);
}

template <typename TT, int VEC>
static void launch_hist(bool from_logits, unsigned grid, size_t lds, hipStream_t st, size_t per_plane, size_t stride, unsigned bx,
                        const float* pred, const void* target, int K, const float* thr_dev, int has_ignore, float ignore_value, int* hist,
                        int* bad) {
  if (from_logits)
    hipLaunchKernelGGL((k_sweep_hist<TT, VEC, true>), dim3(grid), dim3(256), lds, st, per_plane, stride, bx, pred, (const TT*)target, K,
                       thr_dev, has_ignore, ignore_value, hist, bad);
  else
    hipLaunchKernelGGL((k_sweep_hist<TT, VEC, false>), dim3(grid), dim3(256), lds, st, per_plane, stride, bx, pred, (const TT*)target, K,
                       thr_dev, has_ignore, ignore_value, hist, bad);
}

// ------------------------------------------------------------------------------------------------ pass 2: curves
// One workgroup per plane: suffix sums of the two histogram rows in int64, then per threshold k the counts and k_seg_finalize_multi's
// scores.  stats [K][4][N][C] {tp, fp, fn, tn}, per_image [K][N][C][2] {dice, iou}: row k has vk_seg_metrics_multi's layout.
__global__ __launch_bounds__(256) void k_sweep_suffix(int N, int C, int K, const int* __restrict__ hist, float eps,
                                                      int64_t* __restrict__ stats, float* __restrict__ per_image) {
#pragma clang fp contract(off)
  const int plane = blockIdx.x, n = plane / C, c = plane % C, tid = threadIdx.x;
  const int B = K + 1, CH = (B + 255) / 256;
  const int* h0 = hist + (size_t)plane * 2 * B;
  const int* h1 = h0 + B;
  __shared__ long long ca[256], ci[256];
  const int b0 = tid * CH < B ? tid * CH : B, b1 = b0 + CH < B ? b0 + CH : B;
  long long sa = 0, si = 0;
  for (int b = b0; b < b1; ++b) { sa += (long long)h0[b] + (long long)h1[b]; si += (long long)h1[b]; }
  ca[tid] = sa;
  ci[tid] = si;
  __syncthreads();
  long long P = 0, I = 0, valid = 0, T = 0;        // P, I: the bins above this thread's chunk
  for (int j = 0; j < 256; ++j) {
    valid += ca[j];
    T += ci[j];
    if (j > tid) { P += ca[j]; I += ci[j]; }
  }
  const size_t nc = (size_t)N * C, o = (size_t)n * C + c;
  for (int b = b1 - 1; b >= b0; --b) {
    if (b < K) {                                   // threshold k = b: the bins above b
      const int64_t tp = I, fp = P - I, fn = T - I, tn = valid - tp - fp - fn;
      int64_t* s = stats + (size_t)b * 4 * nc + o;
      s[0] = tp;
      s[nc] = fp;
      s[2 * nc] = fn;
      s[3 * nc] = tn;
      const float If = (float)tp;
      const float card = (float)(tp + fp) + (float)(tp + fn);
      const float dice = (2.f * If + eps) / (card + eps);
      const float iou = (If + eps) / ((card - If) + eps);
      per_image[((size_t)b * nc + o) * 2] = dice;
      per_image[((size_t)b * nc + o) * 2 + 1] = iou;
    }
    P += (long long)h0[b] + (long long)h1[b];
    I += (long long)h1[b];
  }
}

// Numbers the images of every group in ascending image index and lists them group by group: rank[i] = #{i' < i : group[i'] == group[i]},
// cnt[g], start[g] = sum of cnt below g, order[start[g] + rank[i]] = i.  One workgroup; cnt is zeroed by the host.  An image whose
// group is outside [0, G) belongs to no group.  The running counts are read back with atomics (they are updated with atomics).
__global__ __launch_bounds__(1024) void k_sweep_group_order(int N, int G, const int* __restrict__ group, int* cnt, int* start, int* rank,
                                                             int* order) {
  __shared__ int sg[1024];
  const int tid = threadIdx.x;
  for (int base = 0; base < N; base += 1024) {
    const int i = base + tid;
    int g = i < N ? group[i] : -1;
    if (g < 0 || g >= G) g = -1;
    sg[tid] = g;
    __syncthreads();
    int r = 0;
    if (g >= 0) {
      for (int j = 0; j < tid; ++j) r += sg[j] == g ? 1 : 0;
      rank[i] = atomicAdd(cnt + g, 0) + r;
    } else if (i < N) {
      rank[i] = -1;
    }
    __syncthreads();
    if (g >= 0) atomicAdd(cnt + g, 1);
    __syncthreads();
  }
  const int CH = (G + 1023) / 1024;
  const int g0 = tid * CH < G ? tid * CH : G, g1 = g0 + CH < G ? g0 + CH : G;
  int s = 0;
  for (int g = g0; g < g1; ++g) s += atomicAdd(cnt + g, 0);
  sg[tid] = s;
  __syncthreads();
  int pre = 0;
  for (int j = 0; j < tid; ++j) pre += sg[j];
  for (int g = g0; g < g1; ++g) {
    start[g] = pre;
    pre += atomicAdd(cnt + g, 0);
  }
  __syncthreads();
  for (int i = tid; i < N; i += 1024) {
    const int g = group[i], r = rank[i];
    if (g >= 0 && g < G && r >= 0) {
      const int pos = start[g] + r;
      if (pos >= 0 && pos < N) order[pos] = i;
    }
  }
}

// Workgroup (k, g): the mean over the images of group g (order == NULL: all N images, in index order) of the per-image scores at
// threshold k, per class, in k_seg_finalize's order: worker j takes members j, j + 64, ... in fp64, the 64 partials are added in j
// order, the quotient is rounded once; the overall score is the fp64 mean of the rounded class scores.  Outputs are [g][K][C] and
// [g][K].  MICRO (all images only): the int64 counts pooled over the images and the micro-averaged curve point in fp64.
template <bool MICRO>
__global__ __launch_bounds__(64) void k_sweep_mean(int N, int C, int K, const float* __restrict__ per_image,
                                                   const int64_t* __restrict__ stats, const int* __restrict__ order,
                                                   const int* __restrict__ start, const int* __restrict__ cnt, float* __restrict__ dice_out,
                                                   float* __restrict__ iou_out, float* __restrict__ mdice_out, float* __restrict__ miou_out,
                                                   int64_t* __restrict__ micro_stats, double* __restrict__ micro) {
#pragma clang fp contract(off)
  __shared__ double acc[2][64];
  __shared__ long long macc[4][64];
  __shared__ float cls[2][kSweepMaxClasses];
  const int k = blockIdx.x, g = blockIdx.y, tid = threadIdx.x;
  int m0 = 0, n = N;
  if (order) {
    m0 = start[g];
    n = cnt[g];
    if (m0 < 0 || n < 0 || m0 > N || n > N - m0) { m0 = 0; n = 0; }
  }
  const size_t nc = (size_t)N * C, kc = (size_t)K * C;
  for (int c = 0; c < C; ++c) {
    double d = 0.0, u = 0.0;
    long long q[4] = {0, 0, 0, 0};
    for (int m = tid; m < n; m += 64) {
      int i = order ? order[m0 + m] : m;
      if (i < 0 || i >= N) i = 0;
      const size_t o = (size_t)i * C + c;
      d += (double)per_image[((size_t)k * nc + o) * 2];
      u += (double)per_image[((size_t)k * nc + o) * 2 + 1];
      if (MICRO) {
#pragma unroll
        for (int e = 0; e < 4; ++e) q[e] += stats[((size_t)k * 4 + e) * nc + o];
      }
    }
    __syncthreads();                 // the previous class's partials have been read
    acc[0][tid] = d;
    acc[1][tid] = u;
    if (MICRO) {
#pragma unroll
      for (int e = 0; e < 4; ++e) macc[e][tid] = q[e];
    }
    __syncthreads();
    if (tid < 2) {
      double s = 0.0;
      for (int j = 0; j < 64; ++j) s += acc[tid][j];        // fixed order
      const float m = (float)(s / (double)n);
      (tid ? iou_out : dice_out)[((size_t)g * K + k) * C + c] = m;
      cls[tid][c] = m;
    }
    if (MICRO && tid == 2) {
      long long s[4] = {0, 0, 0, 0};
      for (int j = 0; j < 64; ++j) {
#pragma unroll
        for (int e = 0; e < 4; ++e) s[e] += macc[e][j];
      }
      const long long tp = s[0], fp = s[1], fn = s[2], tn = s[3];
      const size_t o = (size_t)k * C + c;
#pragma unroll
      for (int e = 0; e < 4; ++e) micro_stats[e * kc + o] = s[e];
      micro[o] = tp + fp == 0 ? 1.0 : (double)tp / (double)(tp + fp);                             // precision
      micro[kc + o] = tp + fn == 0 ? 1.0 : (double)tp / (double)(tp + fn);                        // recall
      micro[2 * kc + o] = 2 * tp + fp + fn == 0 ? 1.0 : (double)(2 * tp) / (double)(2 * tp + fp + fn);   // f1
      micro[3 * kc + o] = tp + fp + fn == 0 ? 1.0 : (double)tp / (double)(tp + fp + fn);          // iou
      micro[4 * kc + o] = fp + tn == 0 ? 0.0 : (double)fp / (double)(fp + tn);                    // false-positive rate
    }
  }
  __syncthreads();
  if (tid < 2) {
    double s = 0.0;
    for (int c = 0; c < C; ++c) s += (double)cls[tid][c];
    (tid ? miou_out : mdice_out)[(size_t)g * K + k] = (float)(s / (double)C);
  }
}

// Epoch score of the reference's validate (train.py:518-529): the mean over the batches of the batch means, as the float64 value
// (sum over g ascending of (double)score_g) / G.  Entry e of the K * C class scores and of the K overall scores alike.
__global__ __launch_bounds__(256) void k_sweep_epoch(int G, int per_group, const float* __restrict__ score, double* __restrict__ out) {
#pragma clang fp contract(off)
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= per_group) return;
  double s = 0.0;
  for (int g = 0; g < G; ++g) s += (double)score[(size_t)g * per_group + e];
  out[e] = s / (double)G;
}

// Per class: AP = sum_k (recall_k - recall_{k+1}) precision_k with recall_K = 0; ROC-AUC by the trapezoid rule over the points (1, 1),
// (fpr_k, recall_k) for k ascending, (0, 0), each step ((x_prev - x) * (y_prev + y)) * 0.5; the first k of the best mean Dice, mean
// IoU and micro F1.  Threads C and C + 1: the first k of the best overall mean Dice / IoU.
__global__ __launch_bounds__(64) void k_sweep_summary(int C, int K, const float* __restrict__ dice, const float* __restrict__ iou,
                                                      const float* __restrict__ mdice, const float* __restrict__ miou,
                                                      const double* __restrict__ micro, double* __restrict__ ap, double* __restrict__ auc,
                                                      int* __restrict__ best_dice, int* __restrict__ best_iou, int* __restrict__ best_f1,
                                                      int* __restrict__ best_mean) {
#pragma clang fp contract(off)
  const int c = threadIdx.x;
  const size_t kc = (size_t)K * C;
  if (c < C) {
    const double* prec = micro + c;
    const double* rec = micro + kc + c;
    const double* f1 = micro + 2 * kc + c;
    const double* fpr = micro + 4 * kc + c;
    double a = 0.0, area = 0.0, xp = 1.0, yp = 1.0;
    int bd = 0, bu = 0, bf = 0;
    for (int k = 0; k < K; ++k) {
      const size_t o = (size_t)k * C;
      const double rn = k + 1 < K ? rec[o + C] : 0.0;
      a += (rec[o] - rn) * prec[o];
      area += ((xp - fpr[o]) * (yp + rec[o])) * 0.5;
      xp = fpr[o];
      yp = rec[o];
      if (dice[o + c] > dice[(size_t)bd * C + c]) bd = k;
      if (iou[o + c] > iou[(size_t)bu * C + c]) bu = k;
      if (f1[o] > f1[(size_t)bf * C]) bf = k;
    }
    area += ((xp - 0.0) * (yp + 0.0)) * 0.5;
    ap[c] = a;
    auc[c] = area;
    best_dice[c] = bd;
    best_iou[c] = bu;
    best_f1[c] = bf;
  } else if (c < C + 2) {
    const float* v = c == C ? mdice : miou;
    int b = 0;
    for (int k = 1; k < K; ++k) {
      if (v[k] > v[b]) b = k;
    }
    best_mean[c - C] = b;
  }
}

static bool sweep_dims_ok(int N, int C, int K, int G) {
  return N >= 1 && N <= kSweepMaxImages && C >= 1 && C <= kSweepMaxClasses && K >= 1 && K <= kSweepMaxK && G >= 0 && G <= N;
}

static size_t sweep_round8(size_t b) { return (b + 7) & ~(size_t)7; }

static void sweep_layout(int N, int C, int K, int G, vk_sweep_layout* L) {
  const size_t n = (size_t)N, c = (size_t)C, k = (size_t)K, g = (size_t)G;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    const size_t o = off;
    off += sweep_round8(bytes);
    return o;
  };
  L->stats = take(k * 4 * n * c * 8);
  L->per_image = take(k * n * c * 2 * 4);
  L->dice = take(k * c * 4);
  L->iou = take(k * c * 4);
  L->mean_dice = take(k * 4);
  L->mean_iou = take(k * 4);
  L->micro_stats = take(4 * k * c * 8);
  L->micro = take(5 * k * c * 8);
  L->ap = take(c * 8);
  L->auc = take(c * 8);
  L->best_dice = take(c * 4);
  L->best_iou = take(c * 4);
  L->best_f1 = take(c * 4);
  L->best_mean = take(2 * 4);
  L->group_dice = take(g * k * c * 4);
  L->group_iou = take(g * k * c * 4);
  L->group_mean_dice = take(g * k * 4);
  L->group_mean_iou = take(g * k * 4);
  L->epoch_dice = take(g ? k * c * 8 : 0);
  L->epoch_iou = take(g ? k * c * 8 : 0);
  L->epoch_mean_dice = take(g ? k * 8 : 0);
  L->epoch_mean_iou = take(g ? k * 8 : 0);
  L->total_bytes = off;
  L->workspace_bytes = g ? (2 * n + 2 * g) * 4 : 0;
}

}  // namespace vk

extern "C" int vk_sweep_curves_layout(int n_images, int C, int K, int n_groups, vk_sweep_layout* layout) {
  using namespace vk;
  VK_CHECK_ARG(layout, "vk_sweep_curves_layout: null layout");
  VK_CHECK_ARG(sweep_dims_ok(n_images, C, K, n_groups), "vk_sweep_curves_layout: N = %d outside [1, %d], C = %d outside [1, %d], "
               "K = %d outside [1, %d] or G = %d outside [0, N]", n_images, kSweepMaxImages, C, kSweepMaxClasses, K, kSweepMaxK, n_groups);
  sweep_layout(n_images, C, K, n_groups, layout);
  return VK_OK;
}

extern "C" size_t vk_sweep_curves_out_bytes(int n_images, int C, int K, int n_groups) {
  using namespace vk;
  if (!sweep_dims_ok(n_images, C, K, n_groups)) return 0;
  vk_sweep_layout L;
  sweep_layout(n_images, C, K, n_groups, &L);
  return L.total_bytes;
}

extern "C" int vk_sweep_hist(int n_planes, size_t per_plane, size_t plane_stride, const float* pred, const void* target, int target_u8,
                             int from_logits, int has_ignore, int ignore_index, int K, const float* thr_host, const float* thr_dev,
                             int accumulate, int32_t* hist, int* bad, void* stream) {
  using namespace vk;
  VK_CHECK_ARG(K >= 1 && K <= kSweepMaxK, "vk_sweep_hist: K = %d outside [1, %d]", K, kSweepMaxK);
  VK_CHECK_ARG(n_planes >= 1 && n_planes <= kSweepMaxPlanes, "vk_sweep_hist: n_planes = %d outside [1, %d]", n_planes, kSweepMaxPlanes);
  VK_CHECK_ARG(per_plane >= 1 && per_plane <= (size_t)INT32_MAX, "vk_sweep_hist: per_plane = %zu outside [1, 2^31)", per_plane);
  if (plane_stride == 0) plane_stride = per_plane;
  VK_CHECK_ARG(plane_stride >= per_plane && plane_stride <= (size_t)INT32_MAX, "vk_sweep_hist: plane_stride = %zu outside [per_plane, 2^31)",
               plane_stride);
  VK_CHECK_ARG(pred && target && thr_host && thr_dev && hist && bad, "vk_sweep_hist: null buffer");
  VK_CHECK_ARG((((uintptr_t)pred | (uintptr_t)thr_dev | (uintptr_t)hist | (uintptr_t)bad) & 3) == 0 &&
               (target_u8 || ((uintptr_t)target & 3) == 0), "vk_sweep_hist: misaligned buffer");
  for (int k = 0; k < K; ++k) {
    VK_CHECK_ARG(isfinite(thr_host[k]), "vk_sweep_hist: threshold %d is not finite", k);
    VK_CHECK_ARG(k == 0 || thr_host[k] > thr_host[k - 1], "vk_sweep_hist: thresholds are not strictly ascending at %d", k);
  }
  hipStream_t st = (hipStream_t)stream;
  const size_t tb = target_u8 ? 1 : 4;
  vkh::ProfScope ps_("sweep_hist", st, 0.0, (4.0 + (double)tb) * (double)n_planes * (double)per_plane);
  const size_t B = (size_t)K + 1;
  if (!accumulate) {
    VK_CHECK_HIP(hipMemsetAsync(hist, 0, (size_t)n_planes * 2 * B * sizeof(int32_t), st));
    VK_CHECK_HIP(hipMemsetAsync(bad, 0, sizeof(int), st));
  }
  const uintptr_t pa = (uintptr_t)pred, ta = (uintptr_t)target;
  int vec = 1;
  if (target_u8) {
    if (per_plane % 4 == 0 && plane_stride % 4 == 0 && (pa & 15) == 0 && (ta & 3) == 0) vec = 4;
  } else if (per_plane % 4 == 0 && plane_stride % 4 == 0 && ((pa | ta) & 15) == 0) {
    vec = 4;
  }
  // workgroups spread over the planes, about 4096 in all; none so small that zeroing and flushing its 2 (K + 1) LDS bins outweighs
  // its share of the plane
  size_t per_wg = (size_t)256 * vec * 4;
  if (per_wg < 8 * B) per_wg = 8 * B;
  size_t bx = (per_plane + per_wg - 1) / per_wg;
  const size_t cap = (4096 + (size_t)n_planes - 1) / (size_t)n_planes;
  if (bx > cap) bx = cap;
  if (bx < 1) bx = 1;
  const unsigned grid = (unsigned)(bx * (size_t)n_planes);
  const size_t lds = ((size_t)K + 2 * B) * 4;
  const float ign = (float)ignore_index;
  const bool fl = from_logits != 0;
  const int hi = has_ignore ? 1 : 0;
  if (target_u8) {
    if (vec == 4) launch_hist<uint8_t, 4>(fl, grid, lds, st, per_plane, plane_stride, (unsigned)bx, pred, target, K, thr_dev, hi, ign, hist, bad);
    else launch_hist<uint8_t, 1>(fl, grid, lds, st, per_plane, plane_stride, (unsigned)bx, pred, target, K, thr_dev, hi, ign, hist, bad);
  } else {
    if (vec == 4) launch_hist<float, 4>(fl, grid, lds, st, per_plane, plane_stride, (unsigned)bx, pred, target, K, thr_dev, hi, ign, hist, bad);
    else launch_hist<float, 1>(fl, grid, lds, st, per_plane, plane_stride, (unsigned)bx, pred, target, K, thr_dev, hi, ign, hist, bad);
  }
  VK_CHECK_HIP(hipGetLastError());
  return VK_OK;
}

extern "C" int vk_sweep_curves(int n_images, int C, int K, const int32_t* hist, const int32_t* group, int n_groups, float eps,
                               void* workspace, size_t workspace_bytes, void* out, size_t out_bytes, void* stream) {
  using namespace vk;
  VK_CHECK_ARG(sweep_dims_ok(n_images, C, K, n_groups), "vk_sweep_curves: N = %d outside [1, %d], C = %d outside [1, %d], "
               "K = %d outside [1, %d] or G = %d outside [0, N]", n_images, kSweepMaxImages, C, kSweepMaxClasses, K, kSweepMaxK, n_groups);
  VK_CHECK_ARG(hist && out, "vk_sweep_curves: null buffer");
  VK_CHECK_ARG((group != nullptr) == (n_groups > 0), "vk_sweep_curves: group and n_groups must be given together");
  vk_sweep_layout L;
  sweep_layout(n_images, C, K, n_groups, &L);
  VK_CHECK_ARG(out_bytes >= L.total_bytes, "vk_sweep_curves: out too small (%zu < %zu)", out_bytes, L.total_bytes);
  VK_CHECK_ARG(((uintptr_t)out & 7) == 0 && ((uintptr_t)hist & 3) == 0 && ((uintptr_t)group & 3) == 0, "vk_sweep_curves: misaligned buffer");
  VK_CHECK_ARG(n_groups == 0 || (workspace && workspace_bytes >= L.workspace_bytes), "vk_sweep_curves: workspace too small (%zu < %zu)",
               workspace ? workspace_bytes : (size_t)0, L.workspace_bytes);
  VK_CHECK_ARG(n_groups == 0 || ((uintptr_t)workspace & 7) == 0, "vk_sweep_curves: workspace must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int N = n_images, G = n_groups;
  vkh::ProfScope ps_("sweep_curves", st, 0.0, 8.0 * N * C * (K + 1) + 40.0 * N * C * K);
  char* o = (char*)out;
  int64_t* stats = (int64_t*)(o + L.stats);
  float* per_image = (float*)(o + L.per_image);
  float* dice = (float*)(o + L.dice);
  float* iou = (float*)(o + L.iou);
  float* mdice = (float*)(o + L.mean_dice);
  float* miou = (float*)(o + L.mean_iou);
  double* micro = (double*)(o + L.micro);
  hipLaunchKernelGGL(k_sweep_suffix, dim3((unsigned)(N * C)), dim3(256), 0, st, N, C, K, hist, eps, stats, per_image);
  hipLaunchKernelGGL(k_sweep_mean<true>, dim3((unsigned)K, 1), dim3(64), 0, st, N, C, K, (const float*)per_image, (const int64_t*)stats,
                     (const int*)nullptr, (const int*)nullptr, (const int*)nullptr, dice, iou, mdice, miou,
                     (int64_t*)(o + L.micro_stats), micro);
  hipLaunchKernelGGL(k_sweep_summary, dim3(1), dim3(64), 0, st, C, K, (const float*)dice, (const float*)iou, (const float*)mdice,
                     (const float*)miou, (const double*)micro, (double*)(o + L.ap), (double*)(o + L.auc), (int*)(o + L.best_dice),
                     (int*)(o + L.best_iou), (int*)(o + L.best_f1), (int*)(o + L.best_mean));
  if (G > 0) {
    int* cnt = (int*)workspace;
    int* start = cnt + G;
    int* rank = start + G;
    int* order = rank + N;
    VK_CHECK_HIP(hipMemsetAsync(workspace, 0, L.workspace_bytes, st));
    hipLaunchKernelGGL(k_sweep_group_order, dim3(1), dim3(1024), 0, st, N, G, group, cnt, start, rank, order);
    float* gd = (float*)(o + L.group_dice);
    float* gu = (float*)(o + L.group_iou);
    float* gmd = (float*)(o + L.group_mean_dice);
    float* gmu = (float*)(o + L.group_mean_iou);
    hipLaunchKernelGGL(k_sweep_mean<false>, dim3((unsigned)K, (unsigned)G), dim3(64), 0, st, N, C, K, (const float*)per_image,
                       (const int64_t*)stats, (const int*)order, (const int*)start, (const int*)cnt, gd, gu, gmd, gmu, (int64_t*)nullptr,
                       (double*)nullptr);
    const int kc = K * C;
    hipLaunchKernelGGL(k_sweep_epoch, dim3((unsigned)((kc + 255) / 256)), dim3(256), 0, st, G, kc, (const float*)gd, (double*)(o + L.epoch_dice));
    hipLaunchKernelGGL(k_sweep_epoch, dim3((unsigned)((kc + 255) / 256)), dim3(256), 0, st, G, kc, (const float*)gu, (double*)(o + L.epoch_iou));
    hipLaunchKernelGGL(k_sweep_epoch, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, st, G, K, (const float*)gmd, (double*)(o + L.epoch_mean_dice));
    hipLaunchKernelGGL(k_sweep_epoch, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, st, G, K, (const float*)gmu, (double*)(o + L.epoch_mean_iou));
  }
  VK_CHECK_HIP(hipGetLastError());
  return VK_OK;
}
