// Configurable segmentation loss (vk_seg_loss): a weighted sum of at most one term of each kind
//   pix      BCE-with-logits (binary, multilabel) or cross-entropy (multiclass): label smoothing, pos_weight, mean over all / valid
//   focal    smp focal_loss_with_logits (per class plane against [t == c] in multiclass mode)
//   dice, jaccard, tversky   region scores from the per-class sums I = sum p y, P = sum p, T = sum y over (N, HW)
//   mcc      (binary) Matthews correlation from the same sums and the valid count: no pass of its own
// with one ignore_index for the whole sum, over logits fp32 [N][C][HW] (class planes), 1 <= C <= 16.  p = sigmoid(x) (binary,
// multilabel: target fp32 [N][C][HW]) or softmax over the classes (multiclass: target int64 [N][HW]).
// Three launches whatever the number of terms:
//   reduce    one pass over x and the target; per workgroup a row of fp64 partial sums (no fp atomics)
//   finalize  one workgroup adds the rows in a fixed order (bit-reproducible), evaluates every term and folds the region terms'
//             gradient into two coefficients per class: d(sum of region terms)/dp = m (a_c y + b_c)
//   backward  one pass writing dlogits = grad_scale * d total / dx (skipped when no gradient is asked for)
// A thread owns 4 consecutive pixels and walks the class planes with 16-byte loads / stores when HW % 4 == 0 and the buffers are
// 16-byte aligned; otherwise the same code runs with one pixel per thread.
#include <math.h>

#include "sl_sigmoid.h"      // SlSig, sl_sigmoid: shared with kp_loss.hip
#include "vk_common.h"

namespace vk {

constexpr int kSlMaxC = 16;
constexpr int kSlCoef = 64;          // doubles: [0,16) a_c, [16,32) b_c, [32] pixel-term scale, [33] focal scale, [34] bad labels
constexpr unsigned kSlPix = 1u, kSlFocal = 2u, kSlDice = 4u, kSlJaccard = 8u, kSlTversky = 16u, kSlMcc = 32u;

// what the two passes over the pixels need of the configuration
struct SlParams {
  unsigned terms;
  int has_ignore, ignore;
  float sf;                          // label smoothing of the pixel term
  int has_pw;
  float pw[kSlMaxC];
  int f_has_alpha;
  float f_alpha, f_gamma;
  int f_gmode;                       // 0, 1, 2: gamma is that integer (no powf); 3: general
};

// q^gamma and gamma q^(gamma - 1) for q in [0, 1].  The general case goes through one hardware log2 and two exp2 (absolute error
// of a few 2^-24 on values <= 1; q = 0 gives 0 and 0 for gamma > 1): powf twice per element made the pass instruction-bound.
__device__ __forceinline__ void sl_pow(float q, float gamma, int gmode, float* qg, float* dqg) {
  if (gmode == 0) { *qg = 1.f; *dqg = 0.f; }
  else if (gmode == 1) { *qg = q; *dqg = 1.f; }
  else if (gmode == 2) { *qg = q * q; *dqg = 2.f * q; }
  else {
    const float lq = __builtin_amdgcn_logf(q);
    *qg = __builtin_amdgcn_exp2f(gamma * lq);
    *dqg = gamma * __builtin_amdgcn_exp2f((gamma - 1.f) * lq);
  }
}

// focal term of one logit against y: value (1 - e^-b)^gamma b aw and its derivative, b = BCE-with-logits(x, y)
__device__ __forceinline__ void sl_focal(float x, float y, const SlSig& g, const SlParams& s, float* val, float* grad) {
  const float b = fmaxf(x, 0.f) - x * y + g.l1p;
  const float q = -expm1f(-b);
  const float pt = expf(-b);
  const float aw = s.f_has_alpha ? s.f_alpha * y + (1.f - s.f_alpha) * (1.f - y) : 1.f;
  float qg, dqg;
  sl_pow(q, s.f_gamma, s.f_gmode, &qg, &dqg);
  *val = qg * b * aw;
  *grad = aw * (qg + dqg * pt * b) * (g.p - y);
}

__device__ __forceinline__ float sl_pwm1(const SlParams& s, int c) {
  float v = 0.f;
  if (s.has_pw) {
#pragma unroll
    for (int j = 0; j < kSlMaxC; ++j)
      if (j == c) v = s.pw[j] - 1.f;
  }
  return v;
}

template <int V> __device__ __forceinline__ void sl_load(const float* p, float* f) {
  if constexpr (V == 4) {
    const f32x4_t v = *reinterpret_cast<const f32x4_t*>(p);
    f[0] = v[0]; f[1] = v[1]; f[2] = v[2]; f[3] = v[3];
  } else {
    f[0] = *p;
  }
}
template <int V> __device__ __forceinline__ void sl_store(float* p, const float* f) {
  if constexpr (V == 4) *reinterpret_cast<f32x4_t*>(p) = f32x4_t{f[0], f[1], f[2], f[3]};
  else *p = f[0];
}
typedef long long sl_i64x2_t __attribute__((ext_vector_type(2)));
template <int V> __device__ __forceinline__ void sl_load_labels(const int64_t* p, int64_t* l) {
  if constexpr (V == 4) {
    const sl_i64x2_t a = *reinterpret_cast<const sl_i64x2_t*>(p), b = *reinterpret_cast<const sl_i64x2_t*>(p + 2);
    l[0] = a[0]; l[1] = a[1]; l[2] = b[0]; l[3] = b[1];
  } else {
    l[0] = *p;
  }
}

// ---------------------------------------------------------------------------------------------- binary / multilabel
// block (bx, plane = n C + c): columns {pix, focal, valid, I, P, T} of class c, row n nbx + bx; part is [column][row]
template <int V>
__global__ __launch_bounds__(256) void k_sl_sig_reduce(SlParams s, int C, int HW, int nbx, int rows, const float* __restrict__ x,
                                                       const float* __restrict__ y, double* __restrict__ part) {
  const int plane = blockIdx.y, c = plane % C, n = plane / C;
  const float* xp = x + (size_t)plane * HW;
  const float* yp = y + (size_t)plane * HW;
  const float pwm1 = sl_pwm1(s, c), ign = (float)s.ignore;
  const bool focal = (s.terms & kSlFocal) != 0;
  double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = (blockIdx.x * 256 + threadIdx.x) * V; i < HW; i += nbx * 256 * V) {
    float xv[V], yv[V];
    sl_load<V>(xp + i, xv);
    sl_load<V>(yp + i, yv);
    float f[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < V; ++j) {
      if (s.has_ignore && yv[j] == ign) continue;
      const float xx = xv[j], yy = yv[j];
      const SlSig g = sl_sigmoid(xx);
      const float ys = yy + s.sf * (1.f - 2.f * yy);
      const float spn = fmaxf(-xx, 0.f) + g.l1p;             // softplus(-x)
      f[0] += fmaxf(xx, 0.f) - xx * ys + g.l1p + pwm1 * ys * spn;
      if (focal) {
        float fv, fg;
        sl_focal(xx, yy, g, s, &fv, &fg);
        f[1] += fv;
      }
      f[2] += 1.f;
      f[3] += g.p * yy;
      f[4] += g.p;
      f[5] += yy;
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) acc[q] += (double)f[q];
  }
  __shared__ double red[4][6];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < 6; ++q) {
    const double v = wave_sum_d(acc[q]);
    if (lane == 0) red[wave][q] = v;
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int q = threadIdx.x;
    part[(size_t)(c * 6 + q) * rows + n * nbx + blockIdx.x] = ((red[0][q] + red[1][q]) + red[2][q]) + red[3][q];
  }
}

template <int V>
__global__ __launch_bounds__(256) void k_sl_sig_bwd(SlParams s, int C, int HW, int nbx, const float* __restrict__ x,
                                                    const float* __restrict__ y, const double* __restrict__ coef, float grad_scale,
                                                    float* __restrict__ dl) {
  const int plane = blockIdx.y, c = plane % C;
  const float ka = (float)coef[c], kb = (float)coef[kSlMaxC + c], kpix = (float)coef[32], kfoc = (float)coef[33];
  const float pwm1 = sl_pwm1(s, c), ign = (float)s.ignore;
  const bool focal = (s.terms & kSlFocal) != 0;
  const size_t base = (size_t)plane * HW;
  for (int i = (blockIdx.x * 256 + threadIdx.x) * V; i < HW; i += nbx * 256 * V) {
    float xv[V], yv[V], o[V];
    sl_load<V>(x + base + i, xv);
    sl_load<V>(y + base + i, yv);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      o[j] = 0.f;
      if (s.has_ignore && yv[j] == ign) continue;
      const float xx = xv[j], yy = yv[j];
      const SlSig g = sl_sigmoid(xx);
      const float ys = yy + s.sf * (1.f - 2.f * yy);
      float v = kpix * (g.p - ys - pwm1 * ys * g.omp) + (ka * yy + kb) * g.p * g.omp;
      if (focal) {
        float fv, fg;
        sl_focal(xx, yy, g, s, &fv, &fg);
        v = fmaf(kfoc, fg, v);
      }
      o[j] = v * grad_scale;
    }
    sl_store<V>(dl + base + i, o);
  }
}

// ---------------------------------------------------------------------------------------------- multiclass
// block (bx, n): columns {pix, focal, valid, bad, I[C], P[C], T[C]}, row n nbx + bx.  CM: compile-time bound of C.
template <int CM, int V>
__global__ __launch_bounds__(256) void k_sl_mc_reduce(SlParams s, int C, int HW, int nbx, int rows, const float* __restrict__ x,
                                                      const int64_t* __restrict__ t, double* __restrict__ part) {
  const int n = blockIdx.y;
  const float* xn = x + (size_t)n * C * HW;
  const int64_t* tn = t + (size_t)n * HW;
  const bool focal = (s.terms & kSlFocal) != 0;
  const float sfc = s.sf / (float)C;
  double pix = 0.0, foc = 0.0, I[CM], Ps[CM];
  int valid = 0, bad = 0, Ts[CM];
#pragma unroll
  for (int c = 0; c < CM; ++c) { I[c] = 0.0; Ps[c] = 0.0; Ts[c] = 0; }
  for (int i = (blockIdx.x * 256 + threadIdx.x) * V; i < HW; i += nbx * 256 * V) {
    float xv[CM][V];
    int64_t lab[V];
    sl_load_labels<V>(tn + i, lab);
    // planes >= C: the last plane again (no branch around a load), then -inf
#pragma unroll
    for (int c = 0; c < CM; ++c) {
      sl_load<V>(xn + (size_t)(c < C ? c : C - 1) * HW + i, xv[c]);
#pragma unroll
      for (int j = 0; j < V; ++j) xv[c][j] = c < C ? xv[c][j] : -INFINITY;
    }
    float fpix = 0.f, ffoc = 0.f;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const int64_t l = lab[j];
      const bool ign = s.has_ignore && l == (int64_t)s.ignore, inr = l >= 0 && l < C;
      bad += !ign && !inr ? 1 : 0;                    // neither a class nor ignore_index: counted, adds nothing
      if (ign || !inr) continue;
      const int label = (int)l;
      ++valid;
      float m = xv[0][j];
#pragma unroll
      for (int c = 1; c < CM; ++c) m = fmaxf(m, xv[c][j]);
      float ex[CM], ssum = 0.f, sumx = 0.f, xl = 0.f;
#pragma unroll
      for (int c = 0; c < CM; ++c) {
        ex[c] = c < C ? expf(xv[c][j] - m) : 0.f;
        ssum += ex[c];
        if (c < C) sumx += xv[c][j];
        if (c == label) xl = xv[c][j];
      }
      const float lse = m + logf(ssum), inv = 1.f / ssum;
      fpix += (1.f - s.sf) * (lse - xl) + sfc * ((float)C * lse - sumx);
      // [c == label] by integer arithmetic: sixteen compare masks held across the loops below would not fit the scalar registers
#pragma unroll
      for (int c = 0; c < CM; ++c) {
        const int hit = 1 - (int)min((unsigned)abs(label - c), 1u);
        const float p = ex[c] * inv;
        Ps[c] += (double)p;
        I[c] += (double)(p * (float)hit);
        Ts[c] += hit;
      }
    }
    if (focal) {       // a loop nest of its own: one body holding both would be too large to unroll
#pragma unroll
      for (int c = 0; c < CM; ++c) {
        if (c < C) {
#pragma unroll
          for (int j = 0; j < V; ++j) {
            const int64_t l = lab[j];
            const bool ok = !(s.has_ignore && l == (int64_t)s.ignore) && l >= 0 && l < C;
            float fv, fg;
            sl_focal(xv[c][j], l == c ? 1.f : 0.f, sl_sigmoid(xv[c][j]), s, &fv, &fg);
            ffoc += ok ? fv : 0.f;
          }
        }
      }
    }
    pix += (double)fpix;
    foc += (double)ffoc;
  }
  __shared__ double red[4][3 * CM + 4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  {
    const double a = wave_sum_d(pix), b = wave_sum_d(foc), c = wave_sum_d((double)valid), d = wave_sum_d((double)bad);
    if (lane == 0) { red[wave][0] = a; red[wave][1] = b; red[wave][2] = c; red[wave][3] = d; }
  }
#pragma unroll
  for (int c = 0; c < CM; ++c) {
    if (c < C) {
      const double a = wave_sum_d(I[c]), b = wave_sum_d(Ps[c]), d = wave_sum_d((double)Ts[c]);
      if (lane == 0) { red[wave][4 + c] = a; red[wave][4 + C + c] = b; red[wave][4 + 2 * C + c] = d; }
    }
  }
  __syncthreads();
  const int Q = 3 * C + 4;
  if ((int)threadIdx.x < Q) {
    const int q = threadIdx.x;
    part[(size_t)q * rows + n * nbx + blockIdx.x] = ((red[0][q] + red[1][q]) + red[2][q]) + red[3][q];
  }
}

// dx_k = kpix (p_k - (1 - sf) [k = t] - sf / C) + p_k (G_k - sum_c G_c p_c) + kfoc focal'_k,  G_k = a_k [k = t] + b_k
template <int CM, int V>
__global__ __launch_bounds__(256) void k_sl_mc_bwd(SlParams s, int C, int HW, int nbx, const float* __restrict__ x,
                                                   const int64_t* __restrict__ t, const double* __restrict__ coef, float grad_scale,
                                                   float* __restrict__ dl) {
  const int n = blockIdx.y;
  const float* xn = x + (size_t)n * C * HW;
  float* dn = dl + (size_t)n * C * HW;
  const int64_t* tn = t + (size_t)n * HW;
  const bool focal = (s.terms & kSlFocal) != 0;
  float ka[CM], kb[CM];
#pragma unroll
  for (int c = 0; c < CM; ++c) { ka[c] = c < C ? (float)coef[c] : 0.f; kb[c] = c < C ? (float)coef[kSlMaxC + c] : 0.f; }
  const float kpix = (float)coef[32], kfoc = (float)coef[33], sfc = s.sf / (float)C;
  for (int i = (blockIdx.x * 256 + threadIdx.x) * V; i < HW; i += nbx * 256 * V) {
    float xv[CM][V];
    int64_t lab[V];
    sl_load_labels<V>(tn + i, lab);
    // planes >= C: the last plane again (no branch around a load), then -inf
#pragma unroll
    for (int c = 0; c < CM; ++c) {
      sl_load<V>(xn + (size_t)(c < C ? c : C - 1) * HW + i, xv[c]);
#pragma unroll
      for (int j = 0; j < V; ++j) xv[c][j] = c < C ? xv[c][j] : -INFINITY;
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const int64_t l = lab[j];
      const bool ok = !(s.has_ignore && l == (int64_t)s.ignore) && l >= 0 && l < C;
      const int label = ok ? (int)l : -1;
      float m = xv[0][j];
#pragma unroll
      for (int c = 1; c < CM; ++c) m = fmaxf(m, xv[c][j]);
      float p[CM], ssum = 0.f;
#pragma unroll
      for (int c = 0; c < CM; ++c) {
        p[c] = c < C ? expf(xv[c][j] - m) : 0.f;
        ssum += p[c];
      }
      const float inv = 1.f / ssum;
      float pg = 0.f;
#pragma unroll
      for (int c = 0; c < CM; ++c) {
        p[c] *= inv;
        pg = fmaf(p[c], (c == label ? ka[c] : 0.f) + kb[c], pg);
      }
#pragma unroll
      for (int c = 0; c < CM; ++c) {
        const float hit = c == label ? 1.f : 0.f;
        float v = kpix * (p[c] - (1.f - s.sf) * hit - sfc) + p[c] * (hit * ka[c] + kb[c] - pg);
        if (focal && c < C) {
          float fv, fg;
          sl_focal(xv[c][j], hit, sl_sigmoid(xv[c][j]), s, &fv, &fg);
          v = fmaf(kfoc, fg, v);
        }
        xv[c][j] = ok ? v * grad_scale : 0.f;        // an ignored (or bad) pixel gets exactly 0
      }
    }
#pragma unroll
    for (int c = 0; c < CM; ++c)
      if (c < C) sl_store<V>(dn + (size_t)c * HW + i, xv[c]);
  }
}

// ---------------------------------------------------------------------------------------------- finalize
// 16 waves: wave w adds the rows of columns w, w + 16, ... (lanes stride the rows, then a fixed butterfly): no barrier per column.
__global__ __launch_bounds__(1024) void k_sl_finalize(vk_seg_loss_cfg cfg, int N, int C, int HW, int rows, const double* __restrict__ part,
                                                      double* __restrict__ coef, float* __restrict__ loss_out) {
  __shared__ double tot[6 * kSlMaxC];
  const bool mc = cfg.mode == VK_LOSS_MULTICLASS;
  const int ncols = mc ? 3 * C + 4 : 6 * C;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int q = wave; q < ncols; q += 16) {
    const double* col = part + (size_t)q * rows;
    double v = 0.0;
    for (int r = lane; r < rows; r += 64) v += col[r];
    v = wave_sum_d(v);
    if (lane == 0) tot[q] = v;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  // sums of class c: I, P, T
#define SL_I(c) tot[mc ? 4 + (c) : (c) * 6 + 3]
#define SL_P(c) tot[mc ? 4 + C + (c) : (c) * 6 + 4]
#define SL_T(c) tot[mc ? 4 + 2 * C + (c) : (c) * 6 + 5]
  double pixs = 0.0, focs = 0.0, valid = 0.0, bad = 0.0, all;
  if (mc) {
    pixs = tot[0]; focs = tot[1]; valid = tot[2]; bad = tot[3];
    all = (double)N * HW;
  } else {
    for (int c = 0; c < C; ++c) { pixs += tot[c * 6]; focs += tot[c * 6 + 1]; valid += tot[c * 6 + 2]; }
    all = (double)N * C * HW;
  }
  const unsigned terms = cfg.terms;
  const double den_pix = cfg.pix_denom_valid ? valid : all;
  const bool has_pix = (terms & kSlPix) && den_pix > 0.0, has_foc = (terms & kSlFocal) && valid > 0.0;
  const double v_pix = has_pix ? pixs / den_pix : 0.0;
  const double v_foc = has_foc ? focs / valid : 0.0;
  for (int c = 0; c < kSlMaxC; ++c) { coef[c] = 0.0; coef[kSlMaxC + c] = 0.0; }
  double v_dice = 0.0, v_jac = 0.0, v_tv = 0.0;
  for (int k = 0; k < 3; ++k) {
    if (!(terms & (kSlDice << k))) continue;
    const double w = k == 0 ? cfg.w_dice : k == 1 ? cfg.w_jaccard : cfg.w_tversky;
    const double smooth = k == 0 ? cfg.dice_smooth : k == 1 ? cfg.jaccard_smooth : cfg.tversky_smooth;
    const double eps = k == 0 ? cfg.dice_eps : k == 1 ? cfg.jaccard_eps : cfg.tversky_eps;
    const int logl = k == 0 ? cfg.dice_log : k == 1 ? cfg.jaccard_log : cfg.tversky_log;
    unsigned cmask = k == 0 ? cfg.dice_classes : k == 1 ? cfg.jaccard_classes : cfg.tversky_classes;
    if (cmask == 0) cmask = (1u << C) - 1u;
    const double al = cfg.tversky_alpha, be = cfg.tversky_beta;
    // score = num / max(den, eps): num = nI I + smooth, den = dI I + dP P + dT T + smooth
    const double nI = k == 0 ? 2.0 : 1.0;
    const double dI = k == 0 ? 0.0 : k == 1 ? -1.0 : 1.0 - al - be;
    const double dP = k == 2 ? al : 1.0, dT = k == 2 ? be : 1.0;
    const int K = __popc(cmask);
    double mean = 0.0;
    for (int c = 0; c < C; ++c) {
      if (!((cmask >> c) & 1u) || !(SL_T(c) > 0.0)) continue;
      const double num = nI * SL_I(c) + smooth, raw = dI * SL_I(c) + dP * SL_P(c) + dT * SL_T(c) + smooth;
      const double score = num / (raw > eps ? raw : eps);
      mean += logl ? -log(score > eps ? score : eps) : 1.0 - score;
    }
    mean /= K;
    double outer = w / K;
    if (k == 2) {
      const double g = cfg.tversky_gamma;
      outer *= g == 1.0 ? 1.0 : g * pow(mean, g - 1.0);
      mean = g == 1.0 ? mean : pow(mean, g);
    }
    if (k == 0) v_dice = mean;
    else if (k == 1) v_jac = mean;
    else v_tv = mean;
    for (int c = 0; c < C; ++c) {
      if (!((cmask >> c) & 1u) || !(SL_T(c) > 0.0)) continue;
      const double num = nI * SL_I(c) + smooth, raw = dI * SL_I(c) + dP * SL_P(c) + dT * SL_T(c) + smooth;
      const double cl = raw > eps ? 1.0 : 0.0, den = raw > eps ? raw : eps;
      const double score = num / den;
      const double dls = outer * (logl ? (score > eps ? -1.0 / score : 0.0) : -1.0);     // d(weighted term) / d score_c
      const double nd2 = num / (den * den) * cl;
      coef[c] += dls * (nI / den - nd2 * dI);            // multiplies y
      coef[kSlMaxC + c] += dls * (-nd2 * dP);            // constant in y
    }
  }
  // mcc (binary, C == 1): tp = I + eps, fp = P - I + eps, fn = T - I + eps, tn = M - P - T + I + eps.  The four factors under the
  // root are A = P + 2 eps, B = T + 2 eps, Cn = M - T + 2 eps, D = M - P + 2 eps: none depends on I, and d num / dI = M + 4 eps,
  // d num / dP = -B, so d loss / dp = m (a y + b) with a = -(M + 4 eps) / den, b = B / den + (num / den) (1 / A - 1 / D) / 2.
  double v_mcc = 0.0;
  if ((terms & kSlMcc) && valid > 0.0) {
    const double e = cfg.mcc_eps, I = SL_I(0), P = SL_P(0), T = SL_T(0), M = valid;
    const double tp = I + e, fp = P - I + e, fn = T - I + e, tn = M - P - T + I + e;
    const double A = tp + fp, B = tp + fn, Cn = tn + fp, D = tn + fn;
    const double num = tp * tn - fp * fn, den = sqrt(A * B * Cn * D);
    v_mcc = 1.0 - num / den;
    coef[0] += cfg.w_mcc * (-(M + 4.0 * e) / den);
    coef[kSlMaxC] += cfg.w_mcc * (B / den + 0.5 * (num / den) * (1.0 / A - 1.0 / D));
  }
#undef SL_I
#undef SL_P
#undef SL_T
  coef[32] = has_pix ? (double)cfg.w_pix / den_pix : 0.0;
  coef[33] = has_foc ? (double)cfg.w_focal / valid : 0.0;
  coef[34] = bad;
  const double total = (terms & kSlPix ? cfg.w_pix * v_pix : 0.0) + (terms & kSlFocal ? cfg.w_focal * v_foc : 0.0) +
                       (terms & kSlDice ? cfg.w_dice * v_dice : 0.0) + (terms & kSlJaccard ? cfg.w_jaccard * v_jac : 0.0) +
                       (terms & kSlTversky ? cfg.w_tversky * v_tv : 0.0) + (terms & kSlMcc ? cfg.w_mcc * v_mcc : 0.0);
  const float nan = __builtin_nanf("");
  const bool isbad = bad > 0.0;
  loss_out[0] = isbad ? nan : (float)total;
  loss_out[1] = isbad ? nan : (float)v_pix;
  loss_out[2] = isbad ? nan : (float)v_foc;
  loss_out[3] = isbad ? nan : (float)v_dice;
  loss_out[4] = isbad ? nan : (float)v_jac;
  loss_out[5] = isbad ? nan : (float)v_tv;
  loss_out[6] = (float)bad;
  loss_out[7] = (float)v_mcc;          // binary only: never beside bad labels; 0 without the term
}

}  // namespace vk

// =================================================================================================
// C ABI
// =================================================================================================
using namespace vk;

namespace {
int sl_nbx(int mode_mc, int N, int C, int HW) {
  int cap = HW / 2048;
  if (cap < 1) cap = 1;
  if (cap > 64) cap = 64;
  const int units = mode_mc ? N : N * C;
  int want = (mode_mc ? 1024 : 2048) / units;
  if (want < 1) want = 1;
  return want < cap ? want : cap;
}

bool finite_f(float v) { return v == v && v - v == 0.f; }

// every field against the mode and C; the text goes to vk_last_error_string
bool sl_check_cfg(const vk_seg_loss_cfg* c, int C, const char* who) {
#define SL_REQ(cond, ...)                        \
  do {                                           \
    if (!(cond)) {                               \
      vkh::set_error(__VA_ARGS__);               \
      return false;                              \
    }                                            \
  } while (0)
  SL_REQ(c, "%s: null configuration", who);
  SL_REQ(c->struct_size == sizeof(vk_seg_loss_cfg), "%s: struct_size %u, this library expects %zu", who, c->struct_size,
         sizeof(vk_seg_loss_cfg));
  SL_REQ(C >= 1 && C <= kSlMaxC, "%s: classes must be 1..16 (got %d)", who, C);
  SL_REQ(c->mode == VK_LOSS_BINARY || c->mode == VK_LOSS_MULTILABEL || c->mode == VK_LOSS_MULTICLASS, "%s: bad mode %d", who, c->mode);
  SL_REQ(c->mode != VK_LOSS_BINARY || C == 1, "%s: mode binary needs C == 1 (got %d)", who, C);
  SL_REQ(c->mode != VK_LOSS_MULTICLASS || C >= 2, "%s: mode multiclass needs C >= 2 (got %d)", who, C);
  SL_REQ(c->terms != 0 && (c->terms & ~63u) == 0, "%s: terms 0x%x: at least one of the six kinds, no other bit", who, c->terms);
  SL_REQ(finite_f(c->w_pix) && finite_f(c->w_focal) && finite_f(c->w_dice) && finite_f(c->w_jaccard) && finite_f(c->w_tversky),
         "%s: a term weight is not finite", who);
  if (c->terms & kSlPix) {
    SL_REQ(c->pix_smooth >= 0.f && c->pix_smooth <= 1.f, "%s: smooth_factor %g outside [0, 1]", who, (double)c->pix_smooth);
    SL_REQ(c->pix_denom_valid == 0 || c->pix_denom_valid == 1, "%s: pix_denom_valid must be 0 or 1", who);
    SL_REQ(!c->has_pos_weight || c->mode != VK_LOSS_MULTICLASS, "%s: pos_weight belongs to the BCE term, not to cross-entropy", who);
    if (c->has_pos_weight)
      for (int i = 0; i < C; ++i) SL_REQ(finite_f(c->pos_weight[i]), "%s: pos_weight[%d] is not finite", who, i);
  }
  if (c->terms & kSlFocal) {
    SL_REQ(finite_f(c->focal_gamma) && (c->focal_gamma == 0.f || c->focal_gamma >= 1.f),
           "%s: focal gamma %g: 0 or >= 1 (the derivative is unbounded in between)", who, (double)c->focal_gamma);
    SL_REQ(!c->focal_has_alpha || finite_f(c->focal_alpha), "%s: focal alpha is not finite", who);
  }
  for (int k = 0; k < 3; ++k) {
    if (!(c->terms & (kSlDice << k))) continue;
    const char* nm = k == 0 ? "dice" : k == 1 ? "jaccard" : "tversky";
    const float smooth = k == 0 ? c->dice_smooth : k == 1 ? c->jaccard_smooth : c->tversky_smooth;
    const float eps = k == 0 ? c->dice_eps : k == 1 ? c->jaccard_eps : c->tversky_eps;
    const unsigned cm = k == 0 ? c->dice_classes : k == 1 ? c->jaccard_classes : c->tversky_classes;
    SL_REQ(finite_f(smooth) && smooth >= 0.f, "%s: %s smooth %g must be finite and >= 0", who, nm, (double)smooth);
    SL_REQ(finite_f(eps) && eps > 0.f, "%s: %s eps %g must be > 0", who, nm, (double)eps);
    SL_REQ((cm >> C) == 0, "%s: %s classes mask 0x%x names a class >= C = %d", who, nm, cm, C);
  }
  if (c->terms & kSlMcc) {
    SL_REQ(c->mode == VK_LOSS_BINARY, "%s: the mcc term needs mode binary", who);
    SL_REQ(finite_f(c->w_mcc), "%s: a term weight is not finite", who);
    SL_REQ(finite_f(c->mcc_eps) && c->mcc_eps > 0.f, "%s: mcc eps %g must be > 0", who, (double)c->mcc_eps);
  }
  if (c->terms & kSlTversky) {
    SL_REQ(finite_f(c->tversky_alpha) && finite_f(c->tversky_beta), "%s: tversky alpha / beta not finite", who);
    SL_REQ(finite_f(c->tversky_gamma) && c->tversky_gamma >= 1.f, "%s: tversky gamma %g must be >= 1", who, (double)c->tversky_gamma);
  }
  return true;
#undef SL_REQ
}
}  // namespace

extern "C" size_t vk_seg_loss_cfg_size(void) { return sizeof(vk_seg_loss_cfg); }

extern "C" size_t vk_seg_loss_workspace_bytes(int N, int C, int HW) {
  if (N < 1 || C < 1 || C > kSlMaxC || HW < 1) return 0;
  const size_t sg = (size_t)6 * C * N * sl_nbx(0, N, C, HW), mc = (size_t)(3 * C + 4) * N * sl_nbx(1, N, C, HW);
  return (kSlCoef + (sg > mc ? sg : mc)) * sizeof(double);
}

extern "C" int vk_seg_loss(const vk_seg_loss_cfg* cfg, int N, int C, int HW, const float* logits, const void* target, void* workspace,
                           size_t workspace_bytes, float* loss_out, float* dlogits, float grad_scale, void* stream) {
  if (!sl_check_cfg(cfg, C, "vk_seg_loss")) return VK_ERR_ARG;
  VK_CHECK_ARG(N >= 1 && HW >= 1 && HW <= (1 << 28) && (int64_t)N * C <= 65535 && (int64_t)N * C * HW < ((int64_t)1 << 40),
               "vk_seg_loss: bad shape N=%d C=%d HW=%d", N, C, HW);
  VK_CHECK_ARG(finite_f(grad_scale), "vk_seg_loss: grad_scale is not finite");
  VK_CHECK_ARG(logits && target && workspace && loss_out, "vk_seg_loss: null argument");
  VK_CHECK_ARG(((uintptr_t)workspace & 7) == 0 && workspace_bytes >= vk_seg_loss_workspace_bytes(N, C, HW),
               "vk_seg_loss: workspace too small or misaligned (%zu bytes, needs %zu)", workspace_bytes,
               vk_seg_loss_workspace_bytes(N, C, HW));
  hipStream_t st = (hipStream_t)stream;
  const bool mc = cfg->mode == VK_LOSS_MULTICLASS;
  SlParams s;
  s.terms = cfg->terms;
  s.has_ignore = cfg->has_ignore;
  s.ignore = cfg->ignore_index;
  s.sf = (cfg->terms & kSlPix) ? cfg->pix_smooth : 0.f;
  s.has_pw = (cfg->terms & kSlPix) && cfg->has_pos_weight;
  for (int i = 0; i < kSlMaxC; ++i) s.pw[i] = (s.has_pw && i < C) ? cfg->pos_weight[i] : 1.f;
  s.f_has_alpha = cfg->focal_has_alpha;
  s.f_alpha = cfg->focal_alpha;
  s.f_gamma = cfg->focal_gamma;
  s.f_gmode = cfg->focal_gamma == 0.f ? 0 : cfg->focal_gamma == 1.f ? 1 : cfg->focal_gamma == 2.f ? 2 : 3;
  const int nbx = sl_nbx(mc, N, C, HW), rows = N * nbx;
  double* coef = (double*)workspace;
  double* part = coef + kSlCoef;
  const bool vec = HW % 4 == 0 && (((uintptr_t)logits | (uintptr_t)target | (uintptr_t)dlogits) & 15) == 0;
  const double px = (double)N * HW, tb = mc ? 8.0 * px : 4.0 * px * C, xb = 4.0 * px * C;
  vkh::ProfScope ps_("seg_loss", st, 0.0, (xb + tb) * (dlogits ? 2.0 : 1.0) + (dlogits ? xb : 0.0));
  if (!mc) {
    const dim3 grid((unsigned)nbx, (unsigned)(N * C));
    const float* y = (const float*)target;
    if (vec) hipLaunchKernelGGL(k_sl_sig_reduce<4>, grid, dim3(256), 0, st, s, C, HW, nbx, rows, logits, y, part);
    else hipLaunchKernelGGL(k_sl_sig_reduce<1>, grid, dim3(256), 0, st, s, C, HW, nbx, rows, logits, y, part);
    hipLaunchKernelGGL(k_sl_finalize, dim3(1), dim3(1024), 0, st, *cfg, N, C, HW, rows, (const double*)part, coef, loss_out);
    if (dlogits) {
      if (vec) hipLaunchKernelGGL(k_sl_sig_bwd<4>, grid, dim3(256), 0, st, s, C, HW, nbx, logits, y, (const double*)coef, grad_scale, dlogits);
      else hipLaunchKernelGGL(k_sl_sig_bwd<1>, grid, dim3(256), 0, st, s, C, HW, nbx, logits, y, (const double*)coef, grad_scale, dlogits);
    }
  } else {
    const dim3 grid((unsigned)nbx, (unsigned)N);
    const int64_t* t = (const int64_t*)target;
#define SL_MC(CM, V)                                                                                                              \
  do {                                                                                                                            \
    hipLaunchKernelGGL((k_sl_mc_reduce<CM, V>), grid, dim3(256), 0, st, s, C, HW, nbx, rows, logits, t, part);                    \
    hipLaunchKernelGGL(k_sl_finalize, dim3(1), dim3(1024), 0, st, *cfg, N, C, HW, rows, (const double*)part, coef, loss_out);     \
    if (dlogits)                                                                                                                  \
      hipLaunchKernelGGL((k_sl_mc_bwd<CM, V>), grid, dim3(256), 0, st, s, C, HW, nbx, logits, t, (const double*)coef, grad_scale, \
                         dlogits);                                                                                                \
  } while (0)
    if (C <= 4) { if (vec) SL_MC(4, 4); else SL_MC(4, 1); }
    else if (C <= 8) { if (vec) SL_MC(8, 4); else SL_MC(8, 1); }
    else { if (vec) SL_MC(16, 4); else SL_MC(16, 1); }
#undef SL_MC
  }
  VK_CHECK_HIP(hipGetLastError());
  return VK_OK;
}
