// Object-level validation: which indentations were found, and how far off are their diagonals.
//
//   vk_inst_contingency, k_inst_contingency: ONE pass over two slot maps (vk_geom_slot_map's output for the prediction and for the
//     ground truth) that counts, per image, the pixels of every (pred slot, GT slot) pair.  HBM-bound: 8 B per pixel read, nothing
//     written but the table.  Integer atomics only, so the table does not depend on any order.
//   vk_inst_match, k_inst_match + k_inst_totals: row / column sums, the unique IoU > 1/2 candidate of every pred slot, the statistics of
//     the matched pairs at K IoU thresholds, then the epoch totals, one image after the other.  Small and latency-bound.
//
// The atomics budget of the contingency kernel.  A pixel's pair is one key, i * (Mg + 1) + j; key 0 is (none, none).
//   1. a lane that holds equal keys (the usual case: 4 pixels of one 16-byte load) offers one (key, count); runs of equal keys over
//      neighbouring lanes are found with one shuffle and one __ballot and leave through their first lane, as in k_geom_runs_area;
//   2. that lane does ONE integer LDS atomic into the workgroup's table, an open-addressed hash of 4096 keys: a workgroup reads 2048
//      pixels, so the table is at most half full and a probe always ends;
//   3. the workgroup leaves with one integer global atomic per key it holds;
//   4. key 0 is never counted: a map is mostly background, and counting it would send every wave to one address.  The [0][0] cell is
//      h * w minus the rest: the image's first workgroup adds h * w, every workgroup subtracts what it counted (one more atomic).
// A slot value outside [0, M) becomes index 0 before it is used, so no value read from a map can address the table.
#include "vk_common.h"

#include <math.h>

#pragma clang fp contract(off)

namespace vk {

constexpr int kInstMaxSlots = 256;
constexpr int kInstMaxK = 16;
constexpr int kInstChunk = 2048;        // pixels per workgroup
constexpr int kInstHashLog = 12;
constexpr int kInstHash = 1 << kInstHashLog;

// ------------------------------------------------------------------------------------------------ the contingency table
__device__ __forceinline__ void inst_hash_add(uint32_t* keys, int* cnts, uint32_t key, int count) {
  uint32_t hh = (key * 2654435761u) >> (32 - kInstHashLog);
  for (int probe = 0; probe < kInstHash; ++probe) {
    uint32_t k = keys[hh];
    if (k == 0u) k = atomicCAS(keys + hh, 0u, key);       // 0 = empty (key 0 is never stored); returns what was there
    if (k == 0u || k == key) {
      atomicAdd(cnts + hh, count);
      return;
    }
    hh = (hh + 1) & (kInstHash - 1);
  }
}

// VEC pixels per lane and step: 4 (one 16-byte load of each map; n % 4 == 0, both maps 16-byte aligned) or 1 (anything).
template <int VEC>
__global__ __launch_bounds__(256) void k_inst_contingency(int n, int Mp, int Mg, const int32_t* __restrict__ pred,
                                                          const int32_t* __restrict__ gt, int32_t* __restrict__ table) {
  __shared__ uint32_t keys[kInstHash];
  __shared__ int cnts[kInstHash];
  __shared__ int s_counted;
  const int tid = threadIdx.x, lane = tid & 63;
  for (int i = tid; i < kInstHash; i += 256) { keys[i] = 0u; cnts[i] = 0; }
  if (tid == 0) s_counted = 0;
  __syncthreads();
  const int b = blockIdx.y;
  const int32_t* p = pred + (size_t)b * n;
  const int32_t* g = gt + (size_t)b * n;
  const int cols = Mg + 1;
  auto key_of = [&](int ps, int gs) -> int {
    const int i = (unsigned)ps < (unsigned)Mp ? ps + 1 : 0;
    const int j = (unsigned)gs < (unsigned)Mg ? gs + 1 : 0;
    return i * cols + j;
  };
  const int base = blockIdx.x * kInstChunk;
#pragma unroll
  for (int it = 0; it < kInstChunk / (256 * VEC); ++it) {
    const int e0 = base + (it * 256 + tid) * VEC;          // < 2^30 + 2048
    int k[VEC];
    if constexpr (VEC == 4) {
      if (e0 < n) {
        const i32x4_t pv = *reinterpret_cast<const i32x4_t*>(p + e0);
        const i32x4_t gv = *reinterpret_cast<const i32x4_t*>(g + e0);
#pragma unroll
        for (int e = 0; e < 4; ++e) k[e] = key_of(pv[e], gv[e]);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) k[e] = 0;
      }
    } else {
      k[0] = e0 < n ? key_of(p[e0], g[e0]) : 0;
    }
    bool uniform = true;
#pragma unroll
    for (int e = 1; e < VEC; ++e) uniform = uniform && k[e] == k[0];
    const int ukey = uniform ? k[0] : -1;                  // -1: this lane's pixels differ, it counts them itself
    const int left = __shfl_up(ukey, 1, 64);
    const bool joins = lane > 0 && ukey > 0 && left == ukey;
    const unsigned long long m = __ballot(joins);
    if (ukey > 0 && !joins) {
      int len = 1;
      if (lane < 63) {
        const unsigned long long rest = ~(m >> (lane + 1));      // first lane above that does not join ends the run
        len += __builtin_ctzll(rest);
      }
      inst_hash_add(keys, cnts, (uint32_t)ukey, len * VEC);
    } else if (ukey < 0) {
      int cur = k[0], c = 1;
#pragma unroll
      for (int e = 1; e < VEC; ++e) {
        if (k[e] == cur) { ++c; continue; }
        if (cur > 0) inst_hash_add(keys, cnts, (uint32_t)cur, c);
        cur = k[e];
        c = 1;
      }
      if (cur > 0) inst_hash_add(keys, cnts, (uint32_t)cur, c);
    }
  }
  __syncthreads();
  int32_t* out = table + (size_t)b * (size_t)(Mp + 1) * cols;
  const uint32_t cells = (uint32_t)((Mp + 1) * cols);
  int counted = 0;
  for (int i = tid; i < kInstHash; i += 256) {
    const uint32_t key = keys[i];
    if (key != 0u && key < cells) {
      const int c = cnts[i];
      atomicAdd(out + key, c);
      counted += c;
    }
  }
  if (counted) atomicAdd(&s_counted, counted);
  __syncthreads();
  if (tid == 0) {
    const int delta = (blockIdx.x == 0 ? n : 0) - s_counted;
    if (delta) atomicAdd(out, delta);
  }
}

// ------------------------------------------------------------------------------------------------ matching
struct InstThr {
  double v[kInstMaxK];
};

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const int u = __shfl_xor(v, o, 64); v = u > v ? u : v; }
  return v;
}

// One workgroup per image.  Row i of the table is pred slot i - 1, column j GT slot j - 1; index 0 is "none".
__global__ __launch_bounds__(256) void k_inst_match(int Mp, int Mg, const int32_t* __restrict__ table_b, const int32_t* __restrict__ n_pred,
                                                    const int32_t* __restrict__ n_gt, int K, const InstThr thr,
                                                    const char* __restrict__ diag_p, size_t stride_p, const char* __restrict__ diag_g,
                                                    size_t stride_g, int32_t* __restrict__ pair_gt, double* __restrict__ pair_iou,
                                                    double* __restrict__ pair_derr, vk_inst_stats* __restrict__ per_image) {
#pragma clang fp contract(off)
  __shared__ int Ap[kInstMaxSlots + 1], Ag[kInstMaxSlots + 1];
  __shared__ int cand[kInstMaxSlots];
  __shared__ double s_iou[kInstMaxSlots], s_dp[kInstMaxSlots], s_dg[kInstMaxSlots];
  __shared__ int s_split, s_merge;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int rows = Mp + 1, cols = Mg + 1;
  const int32_t* T = table_b + (size_t)b * rows * cols;
  const int cp = n_pred[b], cg = n_gt[b];
  const int npu = cp < 0 ? 0 : (cp > Mp ? Mp : cp), ngu = cg < 0 ? 0 : (cg > Mg ? Mg : cg);
  if (tid == 0) { s_split = 0; s_merge = 0; }
  __syncthreads();
  // rows: a wave per row (sum, and how many GT slots the pred slot touches)
  int merges = 0;
  for (int i = wave; i < rows; i += 4) {
    int s = 0, touched = 0;
    for (int j = lane; j < cols; j += 64) {
      const int v = T[(size_t)i * cols + j];
      s += v;
      touched += (j >= 1 && j <= ngu && v > 0) ? 1 : 0;
    }
    s = wave_sum_i(s);
    touched = wave_sum_i(touched);
    if (lane == 0) {
      Ap[i] = s;
      if (i >= 1 && i <= npu && touched >= 2) ++merges;
    }
  }
  if (lane == 0 && merges) atomicAdd(&s_merge, merges);
  // columns: a thread per column
  int splits = 0;
  for (int j = tid; j < cols; j += 256) {
    int s = 0, touched = 0;
    for (int i = 0; i < rows; ++i) {
      const int v = T[(size_t)i * cols + j];
      s += v;
      touched += (i >= 1 && i <= npu && v > 0) ? 1 : 0;
    }
    Ag[j] = s;
    if (j >= 1 && j <= ngu && touched >= 2) ++splits;
  }
  if (splits) atomicAdd(&s_split, splits);
  __syncthreads();
  // the candidate of every pred slot: 3 I > Ap + Ag in int64, i.e. IoU > 1/2 exactly; at most one per row and per column
  for (int s = wave; s < Mp; s += 4) {
    const int i = s + 1;
    int best = -1;
    if (s < npu) {
      const long long ap = Ap[i];
      for (int j = 1 + lane; j <= ngu; j += 64) {
        const long long I = T[(size_t)i * cols + j];
        if (3 * I > ap + (long long)Ag[j]) best = j - 1 > best ? j - 1 : best;
      }
      best = wave_max_i(best);
    }
    if (lane == 0) {
      double iou = 0.0, dp = 0.0, dg = 0.0, derr = 0.0;
      if (best >= 0) {
        const long long I = T[(size_t)i * cols + best + 1];
        const long long U = (long long)Ap[i] + (long long)Ag[best + 1] - I;
        iou = (double)I / (double)U;
        if (diag_p && diag_g) {
          dp = *reinterpret_cast<const double*>(diag_p + ((size_t)b * Mp + s) * stride_p);
          dg = *reinterpret_cast<const double*>(diag_g + ((size_t)b * Mg + best) * stride_g);
          derr = dp - dg;
        }
      }
      cand[s] = best;
      s_iou[s] = iou;
      s_dp[s] = dp;
      s_dg[s] = dg;
      const size_t o = (size_t)b * Mp + s;
      pair_gt[o] = best;
      pair_iou[o] = iou;
      pair_derr[o] = derr;
    }
  }
  __syncthreads();
  // thread k: the matched pairs at threshold k, in ascending pred slot order, every sum sequential
  if (tid < K) {
    const double t = thr.v[tid];
    const bool has_d = diag_p && diag_g;
    long long tp = 0, n_rel = 0;
    double sum_iou = 0.0, sum_abs = 0.0, sum_rel = 0.0, sum_srel = 0.0, sum_hv = 0.0, mx = 0.0;
    for (int s = 0; s < npu; ++s) {
      if (cand[s] < 0 || !(s_iou[s] > t)) continue;
      ++tp;
      sum_iou += s_iou[s];
      if (has_d) {
        const double dp = s_dp[s], dg = s_dg[s];
        const double e = dp - dg, a = fabs(e);
        sum_abs += a;
        if (a > mx) mx = a;
        if (dg > 0.0 && dp > 0.0) {
          ++n_rel;
          sum_rel += a / dg;
          sum_srel += e / dg;
          const double r = dg / dp;
          sum_hv += r * r - 1.0;
        }
      }
    }
    vk_inst_stats o;
    o.tp = tp;
    o.fp = (long long)npu - tp;
    o.fn = (long long)ngu - tp;
    o.n_rel = n_rel;
    o.n_pred_used = npu;
    o.n_gt_used = ngu;
    o.n_split = s_split;
    o.n_merge = s_merge;
    o.overflow_pred = cp > Mp ? 1 : 0;
    o.overflow_gt = cg > Mg ? 1 : 0;
    o.n_images = 1;
    o.sum_iou = sum_iou;
    o.sum_abs_d = sum_abs;
    o.sum_rel_d = sum_rel;
    o.sum_signed_rel_d = sum_srel;
    o.sum_hv_rel = sum_hv;
    o.max_abs_d = mx;
    per_image[(size_t)b * K + tid] = o;
  }
}

// Thread k: totals[k] (+)= image 0, then image 1, ...: one flat sequence, whatever the batches were.
__global__ __launch_bounds__(64) void k_inst_totals(int batch, int K, const vk_inst_stats* __restrict__ per_image, int accumulate,
                                                    vk_inst_stats* __restrict__ totals) {
#pragma clang fp contract(off)
  const int k = threadIdx.x;
  if (k >= K) return;
  vk_inst_stats t;
  if (accumulate) {
    t = totals[k];
  } else {
    t.tp = t.fp = t.fn = t.n_rel = t.n_pred_used = t.n_gt_used = t.n_split = t.n_merge = t.overflow_pred = t.overflow_gt = t.n_images = 0;
    t.sum_iou = t.sum_abs_d = t.sum_rel_d = t.sum_signed_rel_d = t.sum_hv_rel = t.max_abs_d = 0.0;
  }
  for (int b = 0; b < batch; ++b) {
    const vk_inst_stats s = per_image[(size_t)b * K + k];
    t.tp += s.tp;
    t.fp += s.fp;
    t.fn += s.fn;
    t.n_rel += s.n_rel;
    t.n_pred_used += s.n_pred_used;
    t.n_gt_used += s.n_gt_used;
    t.n_split += s.n_split;
    t.n_merge += s.n_merge;
    t.overflow_pred += s.overflow_pred;
    t.overflow_gt += s.overflow_gt;
    t.n_images += s.n_images;
    t.sum_iou += s.sum_iou;
    t.sum_abs_d += s.sum_abs_d;
    t.sum_rel_d += s.sum_rel_d;
    t.sum_signed_rel_d += s.sum_signed_rel_d;
    t.sum_hv_rel += s.sum_hv_rel;
    if (s.max_abs_d > t.max_abs_d) t.max_abs_d = s.max_abs_d;
  }
  totals[k] = t;
}

}  // namespace vk

using namespace vk;

extern "C" int vk_inst_contingency(int batch, int h, int w, const int32_t* pred_slots, const int32_t* gt_slots, int Mp, int Mg,
                                   int32_t* table, void* stream) {
  VK_CHECK_ARG(batch >= 1 && batch <= 65535, "vk_inst_contingency: batch %d outside 1..65535", batch);
  VK_CHECK_ARG(h >= 1 && w >= 1, "vk_inst_contingency: map size %dx%d", h, w);
  VK_CHECK_ARG((size_t)h * (size_t)w < ((size_t)1 << 30), "vk_inst_contingency: more than 2^30 pixels per map");
  VK_CHECK_ARG(Mp >= 1 && Mp <= kInstMaxSlots, "vk_inst_contingency: Mp = %d outside 1..%d", Mp, kInstMaxSlots);
  VK_CHECK_ARG(Mg >= 1 && Mg <= kInstMaxSlots, "vk_inst_contingency: Mg = %d outside 1..%d", Mg, kInstMaxSlots);
  VK_CHECK_ARG(pred_slots && gt_slots && table, "vk_inst_contingency: null buffer");
  VK_CHECK_ARG((((uintptr_t)pred_slots | (uintptr_t)gt_slots | (uintptr_t)table) & 3) == 0, "vk_inst_contingency: misaligned buffer");
  hipStream_t st = (hipStream_t)stream;
  const int n = h * w;
  vkh::ProfScope ps_("inst_contingency", st, 0.0, 8.0 * (double)batch * (double)n);
  VK_CHECK_HIP(hipMemsetAsync(table, 0, (size_t)batch * (size_t)(Mp + 1) * (size_t)(Mg + 1) * sizeof(int32_t), st));
  const dim3 grid((unsigned)((n + kInstChunk - 1) / kInstChunk), (unsigned)batch);
  const bool vec = (w % 4 == 0) && ((((uintptr_t)pred_slots | (uintptr_t)gt_slots) & 15) == 0);
  if (vec) hipLaunchKernelGGL(k_inst_contingency<4>, grid, dim3(256), 0, st, n, Mp, Mg, pred_slots, gt_slots, table);
  else hipLaunchKernelGGL(k_inst_contingency<1>, grid, dim3(256), 0, st, n, Mp, Mg, pred_slots, gt_slots, table);
  VK_CHECK_HIP(hipGetLastError());
  return VK_OK;
}

extern "C" int vk_inst_match(int batch, int Mp, int Mg, const int32_t* table, const int32_t* n_pred, const int32_t* n_gt, int K,
                             const double* iou_thresholds, const void* diag_pred, size_t diag_pred_stride, const void* diag_gt,
                             size_t diag_gt_stride, int32_t* pair_gt, double* pair_iou, double* pair_derr, vk_inst_stats* per_image,
                             vk_inst_stats* totals, int accumulate, void* stream) {
  VK_CHECK_ARG(batch >= 1 && batch <= 65535, "vk_inst_match: batch %d outside 1..65535", batch);
  VK_CHECK_ARG(Mp >= 1 && Mp <= kInstMaxSlots, "vk_inst_match: Mp = %d outside 1..%d", Mp, kInstMaxSlots);
  VK_CHECK_ARG(Mg >= 1 && Mg <= kInstMaxSlots, "vk_inst_match: Mg = %d outside 1..%d", Mg, kInstMaxSlots);
  VK_CHECK_ARG(K >= 1 && K <= kInstMaxK, "vk_inst_match: K = %d outside 1..%d", K, kInstMaxK);
  VK_CHECK_ARG(table && n_pred && n_gt && iou_thresholds && pair_gt && pair_iou && pair_derr && per_image && totals,
               "vk_inst_match: null buffer");
  InstThr thr;
  for (int k = 0; k < kInstMaxK; ++k) thr.v[k] = 2.0;
  for (int k = 0; k < K; ++k) {
    const double t = iou_thresholds[k];
    VK_CHECK_ARG(isfinite(t), "vk_inst_match: threshold %d is not finite", k);
    VK_CHECK_ARG(t >= 0.5 && t < 1.0, "vk_inst_match: threshold %d = %g outside [0.5, 1)", k, t);
    VK_CHECK_ARG(k == 0 || t > iou_thresholds[k - 1], "vk_inst_match: thresholds are not strictly ascending at %d", k);
    thr.v[k] = t;
  }
  VK_CHECK_ARG((((uintptr_t)table | (uintptr_t)n_pred | (uintptr_t)n_gt | (uintptr_t)pair_gt) & 3) == 0 &&
               (((uintptr_t)pair_iou | (uintptr_t)pair_derr | (uintptr_t)per_image | (uintptr_t)totals) & 7) == 0,
               "vk_inst_match: misaligned buffer");
  const bool has_d = diag_pred && diag_gt;
  if (has_d) {
    VK_CHECK_ARG((((uintptr_t)diag_pred | (uintptr_t)diag_gt) & 7) == 0 && diag_pred_stride >= 8 && diag_gt_stride >= 8 &&
                 diag_pred_stride % 8 == 0 && diag_gt_stride % 8 == 0,
                 "vk_inst_match: diagonals must be 8-byte aligned float64 with a byte stride that is a multiple of 8");
  }
  hipStream_t st = (hipStream_t)stream;
  vkh::ProfScope ps_("inst_match", st, 0.0, 8.0 * (double)batch * (double)(Mp + 1) * (double)(Mg + 1));
  hipLaunchKernelGGL(k_inst_match, dim3((unsigned)batch), dim3(256), 0, st, Mp, Mg, table, n_pred, n_gt, K, thr,
                     has_d ? (const char*)diag_pred : (const char*)nullptr, diag_pred_stride, has_d ? (const char*)diag_gt : (const char*)nullptr,
                     diag_gt_stride, pair_gt, pair_iou, pair_derr, per_image);
  hipLaunchKernelGGL(k_inst_totals, dim3(1), dim3(64), 0, st, batch, K, (const vk_inst_stats*)per_image, accumulate ? 1 : 0, totals);
  VK_CHECK_HIP(hipGetLastError());
  return VK_OK;
}
