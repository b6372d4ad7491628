// Param groups and global-norm gradient clipping for the fused AdamW.
//   vk_adamw_step_groups ..... vk_adamw_step_amp_segments with the five hyper-parameters taken per segment from a small by-value table
//                              of groups, and an optional device-resident clip coefficient folded into the gradient factor
//   vk_grad_norm_segments .... L2 or max norm of the gradient over the listed segments only, and torch's clip coefficient of it, in two
//                              launches without atomics: one double per workgroup, then one workgroup that folds them in a fixed order
// Both walk the block table of vk_adamw_segment_blocks (one workgroup per chunk of VK_ADAMW_SEGMENT_CHUNK elements of one segment), so
// the padding between tensors and the tensors that are not listed are never touched.
#include "vk_common.h"

namespace vk {

struct AdamwGroupTable {
  vk_adamw_group g[VK_ADAMW_MAX_GROUPS];      // 8 x 20 bytes, passed by value: an LR scheduler changes lr from the host every epoch
};

__device__ __forceinline__ int group_of(const int32_t* __restrict__ seg_group, int s, int ngroups) {
  const int gi = seg_group[s];
  return (unsigned)gi < (unsigned)ngroups ? gi : 0;      // a bad table reads group 0, never past the kernel argument
}

// k_adamw_prepare_segments with the bias corrections taken from each segment's group.  st[0] = skip flag, st[3] = gradient factor,
// st[4 + 2s], st[5 + 2s] = lr_g / (1 - beta1_g^t), sqrt(1 - beta2_g^t) of segment s's counter.  The factor without a clip coefficient is
// k_adamw_prepare's expression; with one, the product is formed in double and rounded once.
__global__ __launch_bounds__(256) void k_adamw_prepare_groups(int nseg, const int64_t* __restrict__ seg, const int32_t* __restrict__ seg_group,
                                                              int* __restrict__ steps, const float* __restrict__ grad_scale,
                                                              const float* __restrict__ found_inf, const float* __restrict__ clip_coef,
                                                              AdamwGroupTable hp, int ngroups, float inv_scale, float* __restrict__ st) {
  const bool skip = found_inf && *found_inf != 0.f;
  if (threadIdx.x == 0) {
    st[0] = skip ? 1.f : 0.f;
    st[1] = st[2] = 0.f;
    float factor;
    if (clip_coef) {
      const double f = grad_scale ? (double)inv_scale / (double)*grad_scale : (double)inv_scale;
      factor = (float)(f * (double)*clip_coef);
    } else {
      factor = grad_scale ? (float)((double)inv_scale / (double)*grad_scale) : inv_scale;
    }
    st[3] = factor;
  }
  for (int s = threadIdx.x; s < nseg; s += blockDim.x) {
    int* const cnt = steps + seg[3 * (size_t)s + 2];
    int t = *cnt;
    if (!skip) {
      t += 1;
      *cnt = t;
    }
    const vk_adamw_group h = hp.g[group_of(seg_group, s, ngroups)];
    // k_adamw_prepare_segments' four lines (kept there as they stand: routed through a shared helper that kernel schedules differently)
    const double bc1 = 1.0 - pow((double)h.beta1, (double)(t > 0 ? t : 1));
    const double bc2 = 1.0 - pow((double)h.beta2, (double)(t > 0 ? t : 1));
    st[4 + 2 * s] = (float)((double)h.lr / bc1);
    st[5 + 2 * s] = (float)sqrt(bc2);
  }
}

// k_adamw_segments with its group's five values: the same adamw_elem, hence the same bits for the same values
__global__ __launch_bounds__(256) void k_adamw_groups(const int64_t* __restrict__ seg, const int32_t* __restrict__ seg_group,
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

using namespace vk;

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
  AdamwGroupTable hp;
  for (int i = 0; i < VK_ADAMW_MAX_GROUPS; ++i) hp.g[i] = groups_host[i < n_groups ? i : 0];
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_adamw_prepare_groups, dim3(1), dim3(256), 0, st, n_segments, segments, segment_group, step_counts, grad_scale,
                     found_inf, clip_coef, hp, n_groups, inv_scale, scratch);
  vkh::ProfScope ps_("adamw_groups", st, 0.0, (double)n_blocks * VK_ADAMW_SEGMENT_CHUNK * 28.0);
  hipLaunchKernelGGL(k_adamw_groups, dim3((unsigned)n_blocks), dim3(256), 0, st, segments, segment_group, (const int2*)blocks, param, grad,
                     exp_avg, exp_avg_sq, hp, n_groups, (const float*)scratch);
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
