// The fused optimizer (DESIGN.md sections 4, 10 and 24): AdamW, the GradScaler checks and the global gradient norm.
//   vk_adamw_step / vk_adamw_step_amp ......... the whole flat buffer in one grid-stride launch (k_adamw_flat); step-dependent values
//                                               from the host, or resolved on the device by k_adamw_prepare
//   vk_adamw_step_amp_segments / _groups ...... the listed tensors only, one workgroup per chunk of VK_ADAMW_SEGMENT_CHUNK elements of
//                                               one segment (k_adamw_table), hyper-parameters per segment from a by-value table of groups
//   vk_amp_check_inf / vk_amp_unscale_check ... GradScaler's inf check / unscale over the one flat gradient buffer
//   vk_grad_norm_segments ..................... L2 or max norm of the gradient over the listed segments only, and torch's clip
//                                               coefficient of it, in two launches without atomics
//   vk_avg_update / vk_avg_swap ............... EMA / SWA of up to four flat ranges in one grid-stride launch (k_avg_ranges), the weight
//                                               resolved on the device (avg_prepare); the in-place exchange of average and model
//   vk_adamw_step_amp_avg ..................... vk_adamw_step_amp with the average updated by the same launch (k_adamw_flat<.., true>)
// The update arithmetic is written once, in adamw_elem, and the averaging rule once, in avg_elem; every entry point runs them, so they
// agree bit for bit by construction.
// Reference operators replaced: AdamW (train.py:449, 606), GradScaler's unscale and inf check (train.py:441-445).
#include <math.h>

#include "vk_common.h"

namespace vk {

// ------------------------------------------------------------------------------------------------
// K15: AdamW (torch/optim/adam.py's single-tensor path: decoupled decay, bias-corrected).  One element, and the definition of the
// update: every rounding below is one fp32 operation, the fused multiply-adds are explicit and contraction is off, so the bits do not
// depend on what an optimiser pass chooses to fuse.
//   gi   = g * factor                                   (rounded)
//   m'   = fma(fma(g, factor, -m), 1 - beta1, m)        m + (g*factor - m)(1 - beta1): the inner product is not rounded
//   v'   = fma(gi, (1 - beta2) * gi, v * beta2)         both products rounded, then one fused add
//   p'   = fma(p, fma(-lr, wd, 1), -(step_size * (m' / (sqrt(v') / bc2_sqrt + eps))))
// with step_size = lr / (1 - beta1^t) and bc2_sqrt = sqrt(1 - beta2^t), both formed in double and rounded once.  Returns p'.
__device__ __forceinline__ float adamw_elem(size_t i, float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                            float* __restrict__ v, float lr, float beta1, float beta2, float eps, float wd, float step_size,
                                            float bc2_sqrt, float inv_scale) {
#pragma clang fp contract(off)
  const float gr = g[i];
  const float gi = gr * inv_scale;
  const float keep = __builtin_fmaf(-lr, wd, 1.f);                                  // 1 - lr*wd
  float mi = m[i];
  mi = __builtin_fmaf(__builtin_fmaf(gr, inv_scale, -mi), 1.f - beta1, mi);        // m + (gi - m)*(1 - beta1)
  const float vi = __builtin_fmaf(gi, (1.f - beta2) * gi, v[i] * beta2);          // v*beta2 + (1 - beta2)*gi*gi
  const float denom = sqrtf(vi) / bc2_sqrt + eps;
  const float pi = __builtin_fmaf(p[i], keep, -(step_size * (mi / denom)));        // p*(1 - lr*wd) - step*(m / denom)
  p[i] = pi;
  m[i] = mi;
  v[i] = vi;
  return pi;
}

// The averaging rule: a the average, p the current value, w the weight of this update.  w == 1 is a copy, exactly
// (the first SWA sample, decay 0); otherwise the difference is rounded once and the fused multiply-add once.  Returns a'.
__device__ __forceinline__ float avg_elem(float a, float p, float w) {
#pragma clang fp contract(off)
  if (w == 1.f) return p;
  const float d = p - a;
  return __builtin_fmaf(d, w, a);
}

// The weight of the update that follows `*count` updates, by thread 0 of a prepare kernel: st[0] = skip flag; taken: *count = t =
// *count + 1 and st[1] = w, formed in double and rounded once (EMA: 1 - decay_t, decay_t = decay or timm's min(decay, (1 + t) / (10 + t));
// SWA: 1 / t).  Skipped: neither *count nor st[1] is written.
__device__ __forceinline__ void avg_prepare(vk_avg_rule rule, int* __restrict__ count, bool skip, float* __restrict__ st) {
  st[0] = skip ? 1.f : 0.f;
  if (skip) return;
  const int t = *count + 1;
  *count = t;
  double w;
  if (rule.kind == VK_AVG_SWA) {
    w = 1.0 / (double)t;
  } else {
    double d = (double)rule.decay;
    if (rule.warmup) d = fmin(d, (1.0 + (double)t) / (10.0 + (double)t));
    w = 1.0 - d;
  }
  st[1] = (float)w;
}

struct AdamwGroupTable {
  vk_adamw_group g[VK_ADAMW_MAX_GROUPS];      // 8 x 20 bytes, passed by value: an LR scheduler changes lr from the host every epoch
};

// a null table is group 0 everywhere; a bad entry reads group 0, never past the kernel argument
__device__ __forceinline__ int group_of(const int32_t* __restrict__ seg_group, int s, int ngroups) {
  const int gi = seg_group ? seg_group[s] : 0;
  return (unsigned)gi < (unsigned)ngroups ? gi : 0;
}

// the bias corrections of step t (t < 1 counts as 1): step_size = lr / (1 - beta1^t), bc2_sqrt = sqrt(1 - beta2^t)
__device__ __forceinline__ void adamw_bias_corrections(const vk_adamw_group& h, int t, float* step_size, float* bc2_sqrt) {
  const double bc1 = 1.0 - pow((double)h.beta1, (double)(t > 0 ? t : 1));
  const double bc2 = 1.0 - pow((double)h.beta2, (double)(t > 0 ? t : 1));
  *step_size = (float)((double)h.lr / bc1);
  *bc2_sqrt = (float)sqrt(bc2);
}

// the gradient factor inv_scale / *grad_scale (* *clip_coef): a quotient or a product is formed in double and rounded once
__device__ __forceinline__ float adamw_grad_factor(float inv_scale, const float* grad_scale, const float* clip_coef) {
  if (!grad_scale && !clip_coef) return inv_scale;
  const double f = grad_scale ? (double)inv_scale / (double)*grad_scale : (double)inv_scale;
  return (float)(clip_coef ? f * (double)*clip_coef : f);
}

// One workgroup: resolves the GradScaler protocol on the device (no host round trip, train.py:443-445).  The body of both prepare
// kernels; skip is *found_inf != 0.
//   st[0] = skip flag, st[3] = gradient factor;
//   with a segment table: st[4 + 2s], st[5 + 2s] = the bias corrections of segment s from its group and its tensor's counter
//   steps[seg[s][2]], and st[1] = st[2] = 0; without one (seg null, nseg 1): st[1], st[2] = those of the one counter steps[0];
//   a counter advances only when the step is taken (torch: optimizer.step() is not called on an overflow).
__device__ __forceinline__ void adamw_prepare(int nseg, const int64_t* __restrict__ seg, const int32_t* __restrict__ seg_group,
                                              int* __restrict__ steps, const float* __restrict__ grad_scale, bool skip,
                                              const float* __restrict__ clip_coef, const AdamwGroupTable& hp, int ngroups, float inv_scale,
                                              float* __restrict__ st) {
  if (threadIdx.x == 0) {
    st[0] = skip ? 1.f : 0.f;
    if (seg) st[1] = st[2] = 0.f;
    st[3] = adamw_grad_factor(inv_scale, grad_scale, clip_coef);
  }
  for (int s = threadIdx.x; s < nseg; s += blockDim.x) {
    int* const cnt = steps + (seg ? seg[3 * (size_t)s + 2] : 0);
    int t = *cnt;
    if (!skip) {
      t += 1;
      *cnt = t;
    }
    float* const out = seg ? st + 4 + 2 * s : st + 1;
    adamw_bias_corrections(hp.g[group_of(seg_group, s, ngroups)], t, out, out + 1);
  }
}

__global__ __launch_bounds__(256) void k_adamw_prepare(int nseg, const int64_t* __restrict__ seg, const int32_t* __restrict__ seg_group,
                                                       int* __restrict__ steps, const float* __restrict__ grad_scale,
                                                       const float* __restrict__ found_inf, const float* __restrict__ clip_coef,
                                                       AdamwGroupTable hp, int ngroups, float inv_scale, float* __restrict__ st) {
  adamw_prepare(nseg, seg, seg_group, steps, grad_scale, found_inf && *found_inf != 0.f, clip_coef, hp, ngroups, inv_scale, st);
}

// The same, and the weight of the average's update under the same skip test (vk_adamw_step_amp_avg: one counter, no segment table).
__global__ __launch_bounds__(256) void k_adamw_prepare_avg(int* __restrict__ steps, const float* __restrict__ grad_scale,
                                                           const float* __restrict__ found_inf, AdamwGroupTable hp, float inv_scale,
                                                           float* __restrict__ st, vk_avg_rule rule, int* __restrict__ avg_count,
                                                           float* __restrict__ avg_st) {
  const bool skip = found_inf && *found_inf != 0.f;
  adamw_prepare(1, nullptr, nullptr, steps, grad_scale, skip, nullptr, hp, 1, inv_scale, st);
  if (threadIdx.x == 0) avg_prepare(rule, avg_count, skip, avg_st);
}

// The weight alone (vk_avg_update).
__global__ void k_avg_prepare(vk_avg_rule rule, int* __restrict__ count, const float* __restrict__ found_inf, float* __restrict__ st) {
  if (threadIdx.x == 0) avg_prepare(rule, count, found_inf && *found_inf != 0.f, st);
}

// Where k_adamw_flat takes what depends on the step: from the scratch k_adamw_prepare wrote (st, vk_adamw_step_amp), or, with st null,
// from the host's values and its int flag (vk_adamw_step, whose ABI has no device scratch).
struct AdamwStepValues {
  const float* st;
  const int* found_inf;
  float step_size, bc2_sqrt, factor;
};

// What k_adamw_flat<.., true> takes besides: the average of the parameters, the scratch avg_prepare wrote, and one extra range that gets
// the averaging rule alone.  Empty without the flag, so that instantiation keeps the code it had.
template <bool AVG>
struct AdamwFlatAvg {};
template <>
struct AdamwFlatAvg<true> {
  float* avg;
  const float* st;
  float* extra_avg;
  const float* extra_src;
  size_t extra_n;
};

// The whole buffer: a grid-stride loop over [0, n), optionally emitting the 16-bit working copy.  AVG: each element then moves its
// average toward the value just written, and the loop runs on over the extra range.
template <typename LT, bool AVG>
__global__ void k_adamw_flat(size_t n, float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                             float lr, float beta1, float beta2, float eps, float wd, AdamwStepValues sv, LT* lowp, AdamwFlatAvg<AVG> av) {
  if (sv.st) {
    if (sv.st[0] != 0.f) return;
    sv.step_size = sv.st[1];
    sv.bc2_sqrt = sv.st[2];
    sv.factor = sv.st[3];
  } else if (sv.found_inf && *sv.found_inf) {
    return;
  }
  float w = 0.f;
  if constexpr (AVG) w = av.st[1];
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float pi = adamw_elem(i, p, g, m, v, lr, beta1, beta2, eps, wd, sv.step_size, sv.bc2_sqrt, sv.factor);
    if (lowp) st1(lowp + i, pi);
    if constexpr (AVG) av.avg[i] = avg_elem(av.avg[i], pi, w);
  }
  if constexpr (AVG) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < av.extra_n; i += (size_t)gridDim.x * blockDim.x)
      av.extra_avg[i] = avg_elem(av.extra_avg[i], av.extra_src[i], w);
  }
}

// Up to VK_AVG_MAX_RANGES flat ranges in one grid-stride launch (vk_avg_update, vk_avg_swap).  Per range: scalar accesses up to the first
// 16-byte boundary of avg, 16-byte accesses, a scalar tail; a range whose avg and src sit at different offsets from a 16-byte boundary is
// scalar throughout.  SWAP: avg and src exchange their values (both read, then both written); otherwise avg moves toward src by st[1].
struct AvgRanges {
  float* avg[VK_AVG_MAX_RANGES];
  float* src[VK_AVG_MAX_RANGES];
  size_t n[VK_AVG_MAX_RANGES];
  int count;
};

template <bool SWAP>
__global__ __launch_bounds__(256) void k_avg_ranges(AvgRanges r, const float* __restrict__ st) {
  float w = 0.f;
  if constexpr (!SWAP) {
    if (st[0] != 0.f) return;
    w = st[1];
  }
  const size_t gid = blockIdx.x * (size_t)blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  for (int k = 0; k < r.count; ++k) {
    float* const a = r.avg[k];
    float* const s = r.src[k];
    const size_t n = r.n[k];
    const uint32_t mis = (uint32_t)((uintptr_t)a & 15u);
    const size_t to_boundary = ((16u - mis) & 15u) >> 2;
    const size_t head = mis == (uint32_t)((uintptr_t)s & 15u) ? (to_boundary < n ? to_boundary : n) : n;
    const size_t nvec = (n - head) >> 2;
    const size_t tail_at = head + 4 * nvec;
    f32x4_t* const a4 = reinterpret_cast<f32x4_t*>(a + head);
    f32x4_t* const s4 = reinterpret_cast<f32x4_t*>(s + head);
    for (size_t i = gid; i < nvec; i += stride) {
      const f32x4_t x = a4[i], y = s4[i];
      if constexpr (SWAP) {
        a4[i] = y;
        s4[i] = x;
      } else {
        a4[i] = f32x4_t{avg_elem(x[0], y[0], w), avg_elem(x[1], y[1], w), avg_elem(x[2], y[2], w), avg_elem(x[3], y[3], w)};
      }
    }
    // the scalar elements: [0, head) and [tail_at, n), one per thread in grid-stride order (a scalar range may be long)
    const size_t nscalar = head + (n - tail_at);
    for (size_t j = gid; j < nscalar; j += stride) {
      const size_t i = j < head ? j : tail_at + (j - head);
      const float x = a[i], y = s[i];
      if constexpr (SWAP) {
        a[i] = y;
        s[i] = x;
      } else {
        a[i] = avg_elem(x, y, w);
      }
    }
  }
}

// The listed tensors: workgroup b owns chunk blocks[b].y of segment blocks[b].x (a table built once per set of segments: no search per
// element), with the five values of that segment's group, so the padding between tensors and the tensors not listed are never touched.
__global__ __launch_bounds__(256) void k_adamw_table(const int64_t* __restrict__ seg, const int32_t* __restrict__ seg_group,
                                                     const int2* __restrict__ blocks, float* __restrict__ p, const float* __restrict__ g,
                                                     float* __restrict__ m, float* __restrict__ v, AdamwGroupTable hp, int ngroups,
                                                     const float* __restrict__ st) {
  if (st[0] != 0.f) return;
  const int2 b = blocks[blockIdx.x];
  const int64_t begin = seg[3 * (size_t)b.x] + (int64_t)b.y * VK_ADAMW_SEGMENT_CHUNK;
  const int64_t end = min(begin + (int64_t)VK_ADAMW_SEGMENT_CHUNK, seg[3 * (size_t)b.x + 1]);
  const vk_adamw_group h = hp.g[group_of(seg_group, b.x, ngroups)];
  const float step_size = st[4 + 2 * b.x], bc2_sqrt = st[5 + 2 * b.x], inv_scale = st[3];
  for (int64_t i = begin + threadIdx.x; i < end; i += blockDim.x)
    (void)adamw_elem((size_t)i, p, g, m, v, h.lr, h.beta1, h.beta2, h.eps, h.weight_decay, step_size, bc2_sqrt, inv_scale);
}

// ------------------------------------------------------------------------------------------------
// K16: GradScaler's checks
__global__ void k_check_inf(size_t n, const float* __restrict__ g, int* found) {
  bool bad = false;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    bad |= !isfinite(g[i]);
  if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(found, 1);
}

// GradScaler form (torch._amp_foreach_non_finite_check_and_unscale_ over the ONE flat gradient buffer):
// g *= *inv_scale (skipped when the factor is exactly 1: GradScaler's check-only call passes a dummy 1.0), *found_inf = 1.0f if any
// element is inf / nan.  16-byte accesses; n4 = n / 4 (the flat buffer is padded to a multiple of 64 elements).
__global__ __launch_bounds__(256) void k_amp_unscale_check(size_t n4, float* __restrict__ g, const float* __restrict__ inv_scale,
                                                           float* __restrict__ found_inf) {
  const float inv = inv_scale ? *inv_scale : 1.f;
  const bool scale = inv != 1.f;
  bool bad = false;
  f32x4_t* g4 = reinterpret_cast<f32x4_t*>(g);
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    f32x4_t v = g4[i];
    bad |= !(isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]) && isfinite(v[3]));
    if (scale) {
      v = v * inv;
      g4[i] = v;
    }
  }
  if (__any(bad) && (threadIdx.x & 63) == 0) *found_inf = 1.f;     // every writer stores the same value
}

// ------------------------------------------------------------------------------------------------ gradient norm
// One accumulator type for both norms.  L2: the sum of (double)g * (double)g, each product exact.  INF: the largest |g|, where a NaN wins
// over everything (torch.linalg.vector_norm; fmax would drop it) and stays once taken.
template <int KIND>
struct NormAcc {
  static __device__ __forceinline__ double elem(double acc, float g) {
    const double a = (double)g;
    if (KIND == VK_NORM_L2) return __builtin_fma(a, a, acc);       // a * a is exact in double, so the fused and the plain form agree
    return join(acc, __builtin_fabs(a));
  }
  static __device__ __forceinline__ double join(double x, double y) {
    if (KIND == VK_NORM_L2) return x + y;
    return (y > x || y != y) ? y : x;
  }
};

// Fixed-order fold of one value per thread of a 256-thread workgroup: xor butterfly inside each wave (both partners add the same two
// values, so every lane holds the same bits), then the four wave values through LDS as (w0 + w1) + (w2 + w3).  Valid in thread 0.
template <int KIND>
__device__ __forceinline__ double block_fold(double v, double* lds4) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = NormAcc<KIND>::join(v, __shfl_xor(v, o, 64));
  if ((threadIdx.x & 63) == 0) lds4[threadIdx.x >> 6] = v;
  __syncthreads();
  return NormAcc<KIND>::join(NormAcc<KIND>::join(lds4[0], lds4[1]), NormAcc<KIND>::join(lds4[2], lds4[3]));
}

// Workgroup b reads chunk blocks[b].y of segment blocks[b].x: scalar loads up to the first 16-byte boundary, 16-byte loads, scalar tail.
// Every thread takes its elements in a fixed order, so partials[b] has the same bits on every call; it is a plain store.
template <int KIND>
__global__ __launch_bounds__(256) void k_grad_norm_partials(const int64_t* __restrict__ seg, const int2* __restrict__ blocks,
                                                            const float* __restrict__ g, double* __restrict__ partials) {
  __shared__ double lds4[4];
  const int2 b = blocks[blockIdx.x];
  const int64_t begin = seg[3 * (size_t)b.x] + (int64_t)b.y * VK_ADAMW_SEGMENT_CHUNK;
  const int64_t end = min(begin + (int64_t)VK_ADAMW_SEGMENT_CHUNK, seg[3 * (size_t)b.x + 1]);
  const int len = end > begin ? (int)(end - begin) : 0;
  const float* const base = g + begin;
  const int head = min(len, (int)(((16u - (uint32_t)((uintptr_t)base & 15u)) & 15u) >> 2));
  const int nvec = (len - head) >> 2;
  const int tail = len - head - 4 * nvec;
  double acc = 0.0;
  if ((int)threadIdx.x < head) acc = NormAcc<KIND>::elem(acc, base[threadIdx.x]);
  // a chunk holds at most kVecs 16-byte vectors per thread: all of them are requested before the first is used (one workgroup then has
  // its whole 16 KiB in flight); a vector past the end is read as zeros, which change neither a sum of squares nor a maximum of |g|
  constexpr int kVecs = VK_ADAMW_SEGMENT_CHUNK / (4 * 256);
  static_assert(kVecs * 4 * 256 == VK_ADAMW_SEGMENT_CHUNK, "a chunk is a whole number of 16-byte vectors per thread");
  const f32x4_t* const b4 = reinterpret_cast<const f32x4_t*>(base + head);
  f32x4_t x[kVecs];
#pragma unroll
  for (int k = 0; k < kVecs; ++k) {
    const int i = (int)threadIdx.x + 256 * k;
    x[k] = i < nvec ? b4[i] : f32x4_t{0.f, 0.f, 0.f, 0.f};
  }
#pragma unroll
  for (int k = 0; k < kVecs; ++k) {
    acc = NormAcc<KIND>::elem(acc, x[k][0]);
    acc = NormAcc<KIND>::elem(acc, x[k][1]);
    acc = NormAcc<KIND>::elem(acc, x[k][2]);
    acc = NormAcc<KIND>::elem(acc, x[k][3]);
  }
  if ((int)threadIdx.x < tail) acc = NormAcc<KIND>::elem(acc, base[head + 4 * nvec + threadIdx.x]);
  acc = block_fold<KIND>(acc, lds4);
  if (threadIdx.x == 0) partials[blockIdx.x] = acc;
}

// One 256-thread workgroup: thread t folds partials t, t + 256, ... in order, then the fixed tree.  out[0] = total norm of
// inv_scale * grad, out[1] = torch's clip coefficient max_norm / (total + 1e-6) clamped to at most 1, a NaN kept.
template <int KIND>
__global__ __launch_bounds__(256) void k_grad_norm_finalize(int n, const double* __restrict__ partials, float inv_scale, float max_norm,
                                                            float* __restrict__ out) {
  __shared__ double lds4[4];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) acc = NormAcc<KIND>::join(acc, partials[i]);
  acc = block_fold<KIND>(acc, lds4);
  if (threadIdx.x != 0) return;
  const double total = (KIND == VK_NORM_L2 ? sqrt(acc) : acc) * __builtin_fabs((double)inv_scale);
  const double c = (double)max_norm / (total + 1e-6);
  out[0] = (float)total;
  out[1] = (float)(c < 1.0 ? c : (c != c ? c : 1.0));
}

}  // namespace vk

// =================================================================================================
// C ABI wrappers
// =================================================================================================
using namespace vk;

// groups_host[0 .. n_groups) and group 0 again in the unused entries
static AdamwGroupTable group_table(const vk_adamw_group* groups_host, int n_groups) {
  AdamwGroupTable hp;
  for (int i = 0; i < VK_ADAMW_MAX_GROUPS; ++i) hp.g[i] = groups_host[i < n_groups ? i : 0];
  return hp;
}

// k_adamw_flat over [0, n) with the 16-bit copy of lowp_dtype (none: a null pointer or VK_F32)
template <bool AVG>
static void launch_adamw_flat(hipStream_t st, size_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                              const vk_adamw_group& h, const AdamwStepValues& sv, void* lowp_copy, vk_dtype lowp_dtype,
                              const AdamwFlatAvg<AVG>& av) {
  const dim3 grid(grid_for(n)), block(256);
  if (!lowp_copy || lowp_dtype == VK_F32) {
    hipLaunchKernelGGL((k_adamw_flat<float, AVG>), grid, block, 0, st, n, param, grad, exp_avg, exp_avg_sq, h.lr, h.beta1, h.beta2, h.eps,
                       h.weight_decay, sv, (float*)nullptr, av);
  } else if (lowp_dtype == VK_BF16) {
    hipLaunchKernelGGL((k_adamw_flat<bf16_t, AVG>), grid, block, 0, st, n, param, grad, exp_avg, exp_avg_sq, h.lr, h.beta1, h.beta2, h.eps,
                       h.weight_decay, sv, (bf16_t*)lowp_copy, av);
  } else {
    hipLaunchKernelGGL((k_adamw_flat<f16_t, AVG>), grid, block, 0, st, n, param, grad, exp_avg, exp_avg_sq, h.lr, h.beta1, h.beta2, h.eps,
                       h.weight_decay, sv, (f16_t*)lowp_copy, av);
  }
}

// the rule's own argument checks (every entry point that takes one)
static bool avg_rule_ok(const char* who, vk_avg_rule rule) {
  if (rule.kind != VK_AVG_EMA && rule.kind != VK_AVG_SWA) {
    vkh::set_error("%s: unknown averaging kind %d", who, rule.kind);
    return false;
  }
  if (!(rule.decay >= 0.f && rule.decay < 1.f)) {       // false for a NaN too
    vkh::set_error("%s: decay must be a number in [0, 1)", who);
    return false;
  }
  return true;
}

// ranges_host -> the by-value table of k_avg_ranges (empty ranges dropped); false and the error string on a bad one
static bool avg_ranges(const char* who, int n_ranges, const vk_avg_range* ranges_host, AvgRanges* out, size_t* longest) {
  if (n_ranges < 1 || n_ranges > VK_AVG_MAX_RANGES || !ranges_host) {
    vkh::set_error("%s: %d ranges (1..%d are supported, in a non-null array)", who, n_ranges, VK_AVG_MAX_RANGES);
    return false;
  }
  *out = AvgRanges{};
  *longest = 0;
  for (int k = 0; k < n_ranges; ++k) {
    const vk_avg_range& q = ranges_host[k];
    if (q.n == 0) continue;
    if (!q.avg || !q.src || (((uintptr_t)q.avg | (uintptr_t)q.src) & 3u)) {
      vkh::set_error("%s: range %d has a null or misaligned pointer", who, k);
      return false;
    }
    out->avg[out->count] = q.avg;
    out->src[out->count] = const_cast<float*>(q.src);
    out->n[out->count] = q.n;
    ++out->count;
    if (q.n > *longest) *longest = q.n;
  }
  return true;
}

extern "C" int vk_adamw_step(size_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float lr, float beta1,
                             float beta2, float eps, float weight_decay, int step, float inv_scale, const int* found_inf,
                             void* lowp_copy, vk_dtype lowp_dtype, void* stream) {
  VK_CHECK_ARG(n > 0 && param && grad && exp_avg && exp_avg_sq && step >= 1, "vk_adamw_step: bad argument");
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  const AdamwStepValues sv = {nullptr, found_inf, (float)((double)lr / bc1), (float)sqrt(bc2), inv_scale};
  hipStream_t st = (hipStream_t)stream;
  vkh::ProfScope ps_("adamw", st, 0.0, (double)n * 28.0);
  launch_adamw_flat<false>(st, n, param, grad, exp_avg, exp_avg_sq, {lr, beta1, beta2, eps, weight_decay}, sv, lowp_copy, lowp_dtype, {});
  VK_CHECK_HIP(hipGetLastError());
  return VK_OK;
}

extern "C" int vk_adamw_step_amp(size_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float lr, float beta1,
                                 float beta2, float eps, float weight_decay, int* step_count, float inv_scale, const float* grad_scale,
                                 const float* found_inf, float* scratch4, void* lowp_copy, vk_dtype lowp_dtype, void* stream) {
  VK_CHECK_ARG(n > 0 && param && grad && exp_avg && exp_avg_sq && step_count && scratch4, "vk_adamw_step_amp: bad argument");
  const vk_adamw_group h = {lr, beta1, beta2, eps, weight_decay};
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_adamw_prepare, dim3(1), dim3(256), 0, st, 1, (const int64_t*)nullptr, (const int32_t*)nullptr, step_count, grad_scale,
                     found_inf, (const float*)nullptr, group_table(&h, 1), 1, inv_scale, scratch4);
  vkh::ProfScope ps_("adamw", st, 0.0, (double)n * 28.0);
  launch_adamw_flat<false>(st, n, param, grad, exp_avg, exp_avg_sq, h, {scratch4, nullptr, 0.f, 0.f, 0.f}, lowp_copy, lowp_dtype, {});
  VK_CHECK_HIP(hipGetLastError());
  return VK_OK;
}

extern "C" int vk_adamw_step_amp_avg(size_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float lr, float beta1,
                                     float beta2, float eps, float weight_decay, int* step_count, float inv_scale, const float* grad_scale,
                                     const float* found_inf, float* scratch4, void* lowp_copy, vk_dtype lowp_dtype, float* avg,
                                     int* avg_count, vk_avg_rule rule, float* avg_scratch2, float* extra_avg, const float* extra_src,
                                     size_t extra_n, void* stream) {
  VK_CHECK_ARG(n > 0 && param && grad && exp_avg && exp_avg_sq && step_count && scratch4, "vk_adamw_step_amp_avg: bad argument");
  VK_CHECK_ARG(avg && avg_count && avg_scratch2, "vk_adamw_step_amp_avg: null average, counter or scratch");
  VK_CHECK_ARG(extra_n == 0 || (extra_avg && extra_src), "vk_adamw_step_amp_avg: null extra range");
  if (!avg_rule_ok("vk_adamw_step_amp_avg", rule)) return VK_ERR_ARG;
  const vk_adamw_group h = {lr, beta1, beta2, eps, weight_decay};
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_adamw_prepare_avg, dim3(1), dim3(256), 0, st, step_count, grad_scale, found_inf, group_table(&h, 1), inv_scale,
                     scratch4, rule, avg_count, avg_scratch2);
  vkh::ProfScope ps_("adamw_avg", st, 0.0, (double)n * 36.0 + (double)extra_n * 12.0);
  const AdamwFlatAvg<true> av = {avg, avg_scratch2, extra_avg, extra_src, extra_n};
  launch_adamw_flat<true>(st, n, param, grad, exp_avg, exp_avg_sq, h, {scratch4, nullptr, 0.f, 0.f, 0.f}, lowp_copy, lowp_dtype, av);
  VK_CHECK_HIP(hipGetLastError());
  return VK_OK;
}

// the grid of k_avg_ranges: one thread per 16-byte vector of the longest range, at most 2,048 workgroups
static dim3 avg_grid(size_t longest) { return dim3(grid_for((longest + 3) / 4, 256, 2048)); }

extern "C" int vk_avg_update(int n_ranges, const vk_avg_range* ranges_host, vk_avg_rule rule, int* count, const float* found_inf,
                             float* scratch2, void* stream) {
  AvgRanges r;
  size_t longest;
  if (!avg_ranges("vk_avg_update", n_ranges, ranges_host, &r, &longest)) return VK_ERR_ARG;
  VK_CHECK_ARG(count && scratch2, "vk_avg_update: null counter or scratch");
  if (!avg_rule_ok("vk_avg_update", rule)) return VK_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_avg_prepare, dim3(1), dim3(64), 0, st, rule, count, found_inf, scratch2);
  double elems = 0.0;
  for (int k = 0; k < r.count; ++k) elems += (double)r.n[k];
  vkh::ProfScope ps_("avg_update", st, 0.0, elems * 12.0);
  if (r.count) hipLaunchKernelGGL(k_avg_ranges<false>, avg_grid(longest), dim3(256), 0, st, r, (const float*)scratch2);
  VK_CHECK_HIP(hipGetLastError());
  return VK_OK;
}

extern "C" int vk_avg_swap(int n_ranges, const vk_avg_range* ranges_host, void* stream) {
  AvgRanges r;
  size_t longest;
  if (!avg_ranges("vk_avg_swap", n_ranges, ranges_host, &r, &longest)) return VK_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  double elems = 0.0;
  for (int k = 0; k < r.count; ++k) elems += (double)r.n[k];
  vkh::ProfScope ps_("avg_swap", st, 0.0, elems * 16.0);
  if (r.count) hipLaunchKernelGGL(k_avg_ranges<true>, avg_grid(longest), dim3(256), 0, st, r, (const float*)nullptr);
  VK_CHECK_HIP(hipGetLastError());
  return VK_OK;
}

extern "C" int vk_adamw_segment_blocks(int n_segments, const int64_t* seg, int32_t* blocks, int capacity) {
  VK_CHECK_ARG(n_segments >= 1 && seg && (capacity >= 0), "vk_adamw_segment_blocks: bad argument");
  int64_t rows = 0;
  for (int s = 0; s < n_segments; ++s) {
    const int64_t b = seg[3 * s], e = seg[3 * s + 1];
    VK_CHECK_ARG(0 <= b && b < e && seg[3 * s + 2] >= 0, "vk_adamw_segment_blocks: bad segment %d [%lld, %lld)", s, (long long)b, (long long)e);
    const int64_t chunks = (e - b + VK_ADAMW_SEGMENT_CHUNK - 1) / VK_ADAMW_SEGMENT_CHUNK;
    for (int64_t c = 0; c < chunks; ++c, ++rows) {
      VK_CHECK_ARG(rows < (1 << 30), "vk_adamw_segment_blocks: too many blocks");
      if (blocks && rows < capacity) {
        blocks[2 * rows] = s;
        blocks[2 * rows + 1] = (int32_t)c;
      }
    }
  }
  VK_CHECK_ARG(!blocks || rows <= capacity, "vk_adamw_segment_blocks: %lld rows do not fit in %d", (long long)rows, capacity);
  return (int)rows;
}

// prepare + k_adamw_table over the block table; seg_group null: every segment is group 0
static void launch_adamw_table(hipStream_t st, const char* tag, int n_segments, const int64_t* segments, const int32_t* seg_group,
                               int n_blocks, const int32_t* blocks, float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                               const AdamwGroupTable& hp, int n_groups, int* step_counts, float inv_scale, const float* grad_scale,
                               const float* found_inf, const float* clip_coef, float* scratch) {
  hipLaunchKernelGGL(k_adamw_prepare, dim3(1), dim3(256), 0, st, n_segments, segments, seg_group, step_counts, grad_scale, found_inf,
                     clip_coef, hp, n_groups, inv_scale, scratch);
  vkh::ProfScope ps_(tag, st, 0.0, (double)n_blocks * VK_ADAMW_SEGMENT_CHUNK * 28.0);
  hipLaunchKernelGGL(k_adamw_table, dim3((unsigned)n_blocks), dim3(256), 0, st, segments, seg_group, (const int2*)blocks, param, grad,
                     exp_avg, exp_avg_sq, hp, n_groups, (const float*)scratch);
}

extern "C" int vk_adamw_step_amp_segments(int n_segments, const int64_t* segments, int n_blocks, const int32_t* blocks, float* param,
                                          const float* grad, float* exp_avg, float* exp_avg_sq, float lr, float beta1, float beta2, float eps,
                                          float weight_decay, int* step_counts, float inv_scale, const float* grad_scale,
                                          const float* found_inf, float* scratch, void* stream) {
  VK_CHECK_ARG(n_segments >= 1 && n_blocks >= 1 && segments && blocks && param && grad && exp_avg && exp_avg_sq && step_counts && scratch,
               "vk_adamw_step_amp_segments: bad argument");
  const vk_adamw_group h = {lr, beta1, beta2, eps, weight_decay};
  launch_adamw_table((hipStream_t)stream, "adamw_segments", n_segments, segments, nullptr, n_blocks, blocks, param, grad, exp_avg,
                     exp_avg_sq, group_table(&h, 1), 1, step_counts, inv_scale, grad_scale, found_inf, nullptr, scratch);
  VK_CHECK_HIP(hipGetLastError());
  return VK_OK;
}

extern "C" int vk_adamw_step_groups(int n_segments, const int64_t* segments, const int32_t* segment_group, int n_blocks,
                                    const int32_t* blocks, float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                                    int n_groups, const vk_adamw_group* groups_host, int* step_counts, float inv_scale,
                                    const float* grad_scale, const float* found_inf, const float* clip_coef, float* scratch,
                                    void* stream) {
  VK_CHECK_ARG(n_segments >= 1 && n_blocks >= 1 && segments && segment_group && blocks && param && grad && exp_avg && exp_avg_sq &&
                   groups_host && step_counts && scratch,
               "vk_adamw_step_groups: bad argument");
  VK_CHECK_ARG(n_groups >= 1 && n_groups <= VK_ADAMW_MAX_GROUPS, "vk_adamw_step_groups: %d groups (1..%d are supported)", n_groups,
               VK_ADAMW_MAX_GROUPS);
  launch_adamw_table((hipStream_t)stream, "adamw_groups", n_segments, segments, segment_group, n_blocks, blocks, param, grad, exp_avg,
                     exp_avg_sq, group_table(groups_host, n_groups), n_groups, step_counts, inv_scale, grad_scale, found_inf, clip_coef,
                     scratch);
  VK_CHECK_HIP(hipGetLastError());
  return VK_OK;
}

extern "C" int vk_amp_unscale_check(size_t n, float* grad, const float* inv_scale, float* found_inf, void* stream) {
  VK_CHECK_ARG(n > 0 && grad && found_inf, "vk_amp_unscale_check: null argument");
  VK_CHECK_ARG((n & 3) == 0 && ((uintptr_t)grad & 15) == 0, "vk_amp_unscale_check: the gradient buffer must be 16-byte aligned with n %% 4 == 0");
  vkh::ProfScope ps_("amp_unscale_check", (hipStream_t)stream, 0.0, (double)n * 4.0);
  hipLaunchKernelGGL(k_amp_unscale_check, dim3(grid_for(n / 4)), dim3(256), 0, (hipStream_t)stream, n / 4, grad, inv_scale, found_inf);
  VK_CHECK_HIP(hipGetLastError());
  return VK_OK;
}

extern "C" int vk_amp_check_inf(size_t n, const float* grad, int* found_inf, void* stream) {
  VK_CHECK_ARG(n > 0 && grad && found_inf, "vk_amp_check_inf: null argument");
  hipLaunchKernelGGL(k_check_inf, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, n, grad, found_inf);
  VK_CHECK_HIP(hipGetLastError());
  return VK_OK;
}

extern "C" int vk_grad_norm_segments(int n_segments, const int64_t* segments, int n_blocks, const int32_t* blocks, const float* grad,
                                     int norm_kind, float inv_scale, float max_norm, double* partials, float* out, void* stream) {
  VK_CHECK_ARG(n_segments >= 1 && n_blocks >= 1 && segments && blocks && grad && partials && out, "vk_grad_norm_segments: bad argument");
  VK_CHECK_ARG(norm_kind == VK_NORM_L2 || norm_kind == VK_NORM_INF, "vk_grad_norm_segments: unknown norm kind %d", norm_kind);
  VK_CHECK_ARG(max_norm >= 0.f, "vk_grad_norm_segments: max_norm must be a number >= 0");      // false for a NaN too
  hipStream_t st = (hipStream_t)stream;
  vkh::ProfScope ps_("grad_norm", st, 0.0, (double)n_blocks * VK_ADAMW_SEGMENT_CHUNK * 4.0);
  const dim3 grid((unsigned)n_blocks), block(256);
  if (norm_kind == VK_NORM_L2) {
    hipLaunchKernelGGL(k_grad_norm_partials<VK_NORM_L2>, grid, block, 0, st, segments, (const int2*)blocks, grad, partials);
    hipLaunchKernelGGL(k_grad_norm_finalize<VK_NORM_L2>, dim3(1), block, 0, st, n_blocks, (const double*)partials, inv_scale, max_norm, out);
  } else {
    hipLaunchKernelGGL(k_grad_norm_partials<VK_NORM_INF>, grid, block, 0, st, segments, (const int2*)blocks, grad, partials);
    hipLaunchKernelGGL(k_grad_norm_finalize<VK_NORM_INF>, dim3(1), block, 0, st, n_blocks, (const double*)partials, inv_scale, max_norm, out);
  }
  VK_CHECK_HIP(hipGetLastError());
  return VK_OK;
}
