// Per-plane pixel losses of a keypoint head (vk_kp_loss): every plane of logits fp32 [N][C][HW] against a target fp32 [N][C][HW] in
// [0, 1] follows one of three rules, given as two disjoint bit masks
//   heat     CornerNet's penalty-reduced focal loss: an entry is positive iff y >= pos_threshold;
//            positive -(1 - p)^alpha log p, negative -(1 - y)^beta p^alpha log(1 - p); the plane's sum over (N, HW) divided by
//            max(number of positives, 1); `heat` is the mean over the heat planes
//   bce      torch's BCEWithLogitsLoss(pos_weight): the mean over the N HW entries of all BCE planes together
//   neither  the plane is not read; its gradient is 0 (accumulate = 0) or left as it is (accumulate = 1)
// total = w_heat heat + w_bce bce.  The launches and their shape are those of vk_seg_loss (seg_loss.hip):
//   reduce    one pass over x and y; per workgroup one fp64 partial sum and one integer count of positives (no fp atomics)
//   finalize  one workgroup adds the rows in a fixed order (bit-reproducible), writes the values and one gradient coefficient per plane
//   backward  one pass writing (or adding) grad_scale * d total / dx; skipped when no gradient is asked for
// A thread owns 4 consecutive pixels with 16-byte loads / stores when HW % 4 == 0 and the buffers are 16-byte aligned; otherwise the
// same code runs with one pixel per thread.  log p = -(max(-x, 0) + l1p), log(1 - p) = -(max(x, 0) + l1p), 1 - p is SlSig::omp; the
// integer powers are left-to-right fp32 products.
#include <math.h>

#include "sl_sigmoid.h"
#include "vk_common.h"

namespace vk {

constexpr int kKpMaxC = 16;
constexpr int kKpCoef = 16;          // doubles: the gradient coefficient of plane c

struct KpParams {
  unsigned heat, bce;
  int alpha, beta;
  float thr;
  int has_pw;
  float pw[kKpMaxC];
};

// q^k by left-to-right products: 1, q, q q, (q q) q, ...
__device__ __forceinline__ float kp_pow(float q, int k) {
  if (k == 0) return 1.f;
  float r = q;
  for (int i = 1; i < k; ++i) r *= q;
  return r;
}

__device__ __forceinline__ float kp_pwm1(const KpParams& s, int c) {
  float v = 0.f;
  if (s.has_pw) {
#pragma unroll
    for (int j = 0; j < kKpMaxC; ++j)
      if (j == c) v = s.pw[j] - 1.f;
  }
  return v;
}

template <int V> __device__ __forceinline__ void kp_load(const float* p, float* f) {
  if constexpr (V == 4) {
    const f32x4_t v = *reinterpret_cast<const f32x4_t*>(p);
    f[0] = v[0]; f[1] = v[1]; f[2] = v[2]; f[3] = v[3];
  } else {
    f[0] = *p;
  }
}
template <int V> __device__ __forceinline__ void kp_store(float* p, const float* f) {
  if constexpr (V == 4) *reinterpret_cast<f32x4_t*>(p) = f32x4_t{f[0], f[1], f[2], f[3]};
  else *p = f[0];
}

// value of one heat entry; *pos: whether it is a positive
__device__ __forceinline__ float kp_heat_val(float x, float y, const SlSig& g, const KpParams& s, bool* pos) {
  *pos = y >= s.thr;
  if (*pos) return kp_pow(g.omp, s.alpha) * (fmaxf(-x, 0.f) + g.l1p);
  return kp_pow(1.f - y, s.beta) * kp_pow(g.p, s.alpha) * (fmaxf(x, 0.f) + g.l1p);
}

// its derivative: positive alpha p omp^alpha log p - omp^(alpha + 1), negative (1 - y)^beta (p^(alpha + 1) - alpha p^alpha omp log(1 - p))
__device__ __forceinline__ float kp_heat_grad(float x, float y, const SlSig& g, const KpParams& s) {
  const float fa = (float)s.alpha;
  if (y >= s.thr) {
    const float oa = kp_pow(g.omp, s.alpha);
    return -(fa * g.p * oa * (fmaxf(-x, 0.f) + g.l1p) + oa * g.omp);
  }
  const float pa = kp_pow(g.p, s.alpha);
  return kp_pow(1.f - y, s.beta) * (pa * g.p + fa * pa * g.omp * (fmaxf(x, 0.f) + g.l1p));
}

// block (bx, plane = n C + c): the sum and the positives of class c, row n nbx + bx; psum and pcnt are [plane c][row]
template <int V>
__global__ __launch_bounds__(256) void k_kp_reduce(KpParams s, int C, int HW, int nbx, int rows, const float* __restrict__ x,
                                                   const float* __restrict__ y, double* __restrict__ psum,
                                                   long long* __restrict__ pcnt) {
  const int plane = blockIdx.y, c = plane % C, n = plane / C;
  const bool heat = (s.heat >> c) & 1u, bce = (s.bce >> c) & 1u;
  if (!heat && !bce) return;                                  // a plane without a rule: nothing is read
  const float* xp = x + (size_t)plane * HW;
  const float* yp = y + (size_t)plane * HW;
  const float pwm1 = kp_pwm1(s, c);
  double acc = 0.0;
  int cnt = 0;
  for (int i = (blockIdx.x * 256 + threadIdx.x) * V; i < HW; i += nbx * 256 * V) {
    float xv[V], yv[V];
    kp_load<V>(xp + i, xv);
    kp_load<V>(yp + i, yv);
    float f = 0.f;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const float xx = xv[j], yy = yv[j];
      const SlSig g = sl_sigmoid(xx);
      if (heat) {
        bool pos;
        f += kp_heat_val(xx, yy, g, s, &pos);
        cnt += pos ? 1 : 0;
      } else {
        const float spn = fmaxf(-xx, 0.f) + g.l1p;             // softplus(-x)
        f += fmaxf(xx, 0.f) - xx * yy + g.l1p + pwm1 * yy * spn;
      }
    }
    acc += (double)f;
  }
  __shared__ double red[4];
  __shared__ int redn[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double v = wave_sum_d(acc);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if (lane == 0) { red[wave] = v; redn[wave] = cnt; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const size_t at = (size_t)c * rows + n * nbx + blockIdx.x;
    psum[at] = ((red[0] + red[1]) + red[2]) + red[3];
    pcnt[at] = (long long)redn[0] + redn[1] + redn[2] + redn[3];
  }
}

// 16 waves: wave w adds the rows of plane w (lanes stride the rows, then a fixed butterfly)
__global__ __launch_bounds__(1024) void k_kp_finalize(KpParams s, float w_heat, float w_bce, int N, int C, int HW, int rows,
                                                      const double* __restrict__ psum, const long long* __restrict__ pcnt,
                                                      double* __restrict__ coef, float* __restrict__ loss_out,
                                                      int64_t* __restrict__ positives) {
  __shared__ double tot[kKpMaxC];
  __shared__ long long npos[kKpMaxC];
  const int lane = threadIdx.x & 63, c = threadIdx.x >> 6;
  const unsigned ruled = s.heat | s.bce;
  double v = 0.0;
  long long k = 0;
  if (c < C && ((ruled >> c) & 1u)) {
    for (int r = lane; r < rows; r += 64) {
      v += psum[(size_t)c * rows + r];
      k += pcnt[(size_t)c * rows + r];
    }
  }
  v = wave_sum_d(v);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) k += __shfl_xor(k, o, 64);
  if (lane == 0) { tot[c] = v; npos[c] = k; }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const int n_heat = __popc(s.heat), n_bce = __popc(s.bce);
  const double all_bce = (double)N * HW * n_bce;
  double heat = 0.0, bce = 0.0;
  for (int q = 0; q < kKpMaxC; ++q) {
    double kq = 0.0;
    long long pq = 0;
    if (q < C && ((s.heat >> q) & 1u)) {
      pq = npos[q];
      const double den = pq > 0 ? (double)pq : 1.0;
      heat += tot[q] / den;
      kq = (double)w_heat / ((double)n_heat * den);
    } else if (q < C && ((s.bce >> q) & 1u)) {
      bce += tot[q];
      kq = (double)w_bce / all_bce;
    }
    coef[q] = kq;
    if (positives) positives[q] = (int64_t)pq;
  }
  heat = n_heat ? heat / n_heat : 0.0;
  bce = n_bce ? bce / all_bce : 0.0;
  loss_out[0] = (float)((n_heat ? (double)w_heat * heat : 0.0) + (n_bce ? (double)w_bce * bce : 0.0));
  loss_out[1] = (float)heat;
  loss_out[2] = (float)bce;
  for (int q = 3; q < 8; ++q) loss_out[q] = 0.f;
}

template <int V>
__global__ __launch_bounds__(256) void k_kp_bwd(KpParams s, int C, int HW, int nbx, const float* __restrict__ x,
                                                const float* __restrict__ y, const double* __restrict__ coef, float grad_scale,
                                                int accumulate, float* __restrict__ dl) {
  const int plane = blockIdx.y, c = plane % C;
  const bool heat = (s.heat >> c) & 1u, bce = (s.bce >> c) & 1u;
  const size_t base = (size_t)plane * HW;
  if (!heat && !bce) {                                        // nothing is read: zeros, or the plane is left as it is
    if (accumulate) return;
    float z[V];
#pragma unroll
    for (int j = 0; j < V; ++j) z[j] = 0.f;
    for (int i = (blockIdx.x * 256 + threadIdx.x) * V; i < HW; i += nbx * 256 * V) kp_store<V>(dl + base + i, z);
    return;
  }
  const float k = (float)coef[c], pwm1 = kp_pwm1(s, c);
  for (int i = (blockIdx.x * 256 + threadIdx.x) * V; i < HW; i += nbx * 256 * V) {
    float xv[V], yv[V], o[V];
    kp_load<V>(x + base + i, xv);
    kp_load<V>(y + base + i, yv);
    if (accumulate) kp_load<V>(dl + base + i, o);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const float xx = xv[j], yy = yv[j];
      const SlSig g = sl_sigmoid(xx);
      const float v = heat ? k * kp_heat_grad(xx, yy, g, s) : k * (g.p - yy - pwm1 * yy * g.omp);
      const float sv = __fmul_rn(v, grad_scale);                 // rounded before it is added: old + g, not a fused multiply-add
      o[j] = accumulate ? __fadd_rn(o[j], sv) : sv;
    }
    kp_store<V>(dl + base + i, o);
  }
}

// loss_out float[16]: [0, 8) as vk_seg_loss leaves them (zeros without a seg part), [8, 11) = {total, heat, bce} as vk_kp_loss leaves
// them -> [0] += total, [8] heat, [9] bce, [10] total
__global__ void k_kp_combine(float* __restrict__ lo) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const float t = lo[8], h = lo[9], b = lo[10];
  lo[0] += t;
  lo[8] = h;
  lo[9] = b;
  lo[10] = t;
}

}  // namespace vk

// =================================================================================================
// C ABI
// =================================================================================================
using namespace vk;

namespace {
int kp_nbx(int N, int C, int HW) {
  int cap = HW / 2048;
  if (cap < 1) cap = 1;
  if (cap > 64) cap = 64;
  int want = 2048 / (N * C);
  if (want < 1) want = 1;
  return want < cap ? want : cap;
}

bool kp_finite(float v) { return v == v && v - v == 0.f; }

bool kp_shape_ok(int N, int C, int HW) {
  return N >= 1 && C >= 1 && C <= kKpMaxC && HW >= 1 && HW <= (1 << 28) && (int64_t)N * C <= 65535 &&
         (int64_t)N * C * HW <= (int64_t)0x7fffffff;
}
}  // namespace

namespace vk {
// every field of the configuration and the shape; the text goes to vk_last_error_string
bool kp_check(const vk_kp_loss_cfg* c, int N, int C, int HW, const char* who) {
#define KP_REQ(cond, ...)                        \
  do {                                           \
    if (!(cond)) {                               \
      vkh::set_error(__VA_ARGS__);               \
      return false;                              \
    }                                            \
  } while (0)
  KP_REQ(c, "%s: null configuration", who);
  KP_REQ(c->struct_size == sizeof(vk_kp_loss_cfg), "%s: struct_size %u, this library expects %zu", who, c->struct_size,
         sizeof(vk_kp_loss_cfg));
  KP_REQ(C >= 1 && C <= kKpMaxC, "%s: planes must be 1..16 (got %d)", who, C);
  KP_REQ((c->heat_planes | c->bce_planes) != 0, "%s: both plane masks are empty", who);
  KP_REQ((c->heat_planes & c->bce_planes) == 0, "%s: the plane masks overlap (heat 0x%x, bce 0x%x)", who, c->heat_planes, c->bce_planes);
  KP_REQ(((c->heat_planes | c->bce_planes) >> C) == 0, "%s: a plane mask (heat 0x%x, bce 0x%x) names a plane >= C = %d", who,
         c->heat_planes, c->bce_planes, C);
  KP_REQ(kp_finite(c->w_heat) && kp_finite(c->w_bce), "%s: a term weight is not finite", who);
  KP_REQ(c->alpha >= 0 && c->alpha <= VK_KP_LOSS_MAX_EXP && c->beta >= 0 && c->beta <= VK_KP_LOSS_MAX_EXP,
         "%s: exponents alpha = %d, beta = %d outside 0..%d", who, c->alpha, c->beta, VK_KP_LOSS_MAX_EXP);
  KP_REQ(c->pos_threshold > 0.f && c->pos_threshold <= 1.f, "%s: pos_threshold %g outside (0, 1]", who, (double)c->pos_threshold);
  KP_REQ(c->has_pos_weight == 0 || c->has_pos_weight == 1, "%s: has_pos_weight must be 0 or 1", who);
  if (c->has_pos_weight)
    for (int i = 0; i < C; ++i)
      KP_REQ(kp_finite(c->pos_weight[i]) && c->pos_weight[i] > 0.f, "%s: pos_weight[%d] is not finite and positive", who, i);
  KP_REQ(N >= 1 && HW >= 1 && HW <= (1 << 28) && (int64_t)N * C <= 65535, "%s: bad shape N=%d C=%d HW=%d", who, N, C, HW);
  KP_REQ((int64_t)N * C * HW <= (int64_t)0x7fffffff, "%s: N C HW = %lld entries, at most 2^31 - 1", who, (long long)N * C * HW);
  return true;
#undef KP_REQ
}

bool kp_check_workspace(int N, int C, int HW, const void* workspace, size_t workspace_bytes, const char* who) {
  const size_t need = vk_kp_loss_workspace_bytes(N, C, HW);
  if (!workspace) {
    vkh::set_error("%s: null argument", who);
    return false;
  }
  if (((uintptr_t)workspace & 7) != 0 || workspace_bytes < need) {
    vkh::set_error("%s: workspace too small or misaligned (%zu bytes, needs %zu)", who, workspace_bytes, need);
    return false;
  }
  return true;
}

int kp_combine(float* loss_out, hipStream_t st) {
  hipLaunchKernelGGL(k_kp_combine, dim3(1), dim3(64), 0, st, loss_out);
  VK_CHECK_HIP(hipGetLastError());
  return VK_OK;
}
}  // namespace vk

extern "C" size_t vk_kp_loss_cfg_size(void) { return sizeof(vk_kp_loss_cfg); }

extern "C" size_t vk_kp_loss_workspace_bytes(int N, int C, int HW) {
  if (!kp_shape_ok(N, C, HW)) return 0;
  const size_t cells = (size_t)C * N * kp_nbx(N, C, HW);
  return kKpCoef * sizeof(double) + cells * (sizeof(double) + sizeof(long long));
}

extern "C" int vk_kp_loss(const vk_kp_loss_cfg* cfg, int N, int C, int HW, const float* logits, const float* target, void* workspace,
                          size_t workspace_bytes, float* loss_out, int64_t* positives, float* dlogits, float grad_scale, int accumulate,
                          void* stream) {
  if (!kp_check(cfg, N, C, HW, "vk_kp_loss")) return VK_ERR_ARG;
  VK_CHECK_ARG(kp_finite(grad_scale), "vk_kp_loss: grad_scale is not finite");
  VK_CHECK_ARG(accumulate == 0 || accumulate == 1, "vk_kp_loss: accumulate must be 0 or 1");
  VK_CHECK_ARG(logits && target && loss_out, "vk_kp_loss: null argument");
  if (!kp_check_workspace(N, C, HW, workspace, workspace_bytes, "vk_kp_loss")) return VK_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  KpParams s;
  s.heat = cfg->heat_planes;
  s.bce = cfg->bce_planes;
  s.alpha = cfg->alpha;
  s.beta = cfg->beta;
  s.thr = cfg->pos_threshold;
  s.has_pw = cfg->has_pos_weight;
  for (int i = 0; i < kKpMaxC; ++i) s.pw[i] = (s.has_pw && i < C) ? cfg->pos_weight[i] : 1.f;
  const int nbx = kp_nbx(N, C, HW), rows = N * nbx;
  double* coef = (double*)workspace;
  double* psum = coef + kKpCoef;
  long long* pcnt = (long long*)(psum + (size_t)C * rows);
  const bool vec = HW % 4 == 0 && (((uintptr_t)logits | (uintptr_t)target | (uintptr_t)dlogits) & 15) == 0;
  const double ruled = (double)N * HW * __builtin_popcount(s.heat | s.bce), rest = (double)N * HW * C - ruled;
  vkh::ProfScope ps_("kp_loss", st, 0.0, 8.0 * ruled + (dlogits ? (accumulate ? 16.0 : 12.0) * ruled + (accumulate ? 0.0 : 4.0 * rest) : 0.0));
  const dim3 grid((unsigned)nbx, (unsigned)(N * C));
  if (vec) hipLaunchKernelGGL(k_kp_reduce<4>, grid, dim3(256), 0, st, s, C, HW, nbx, rows, logits, target, psum, pcnt);
  else hipLaunchKernelGGL(k_kp_reduce<1>, grid, dim3(256), 0, st, s, C, HW, nbx, rows, logits, target, psum, pcnt);
  hipLaunchKernelGGL(k_kp_finalize, dim3(1), dim3(1024), 0, st, s, cfg->w_heat, cfg->w_bce, N, C, HW, rows, (const double*)psum,
                     (const long long*)pcnt, coef, loss_out, positives);
  if (dlogits) {
    if (vec) hipLaunchKernelGGL(k_kp_bwd<4>, grid, dim3(256), 0, st, s, C, HW, nbx, logits, target, (const double*)coef, grad_scale, accumulate, dlogits);
    else hipLaunchKernelGGL(k_kp_bwd<1>, grid, dim3(256), 0, st, s, C, HW, nbx, logits, target, (const double*)coef, grad_scale, accumulate, dlogits);
  }
  VK_CHECK_HIP(hipGetLastError());
  return VK_OK;
}
