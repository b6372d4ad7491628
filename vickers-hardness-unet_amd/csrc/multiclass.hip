// Multi-class / multi-label segmentation: the 16 -> C head (1 <= C <= 16) and the two losses smp pairs with it.
//   head forward   : logits[n][c][y][x] = bias[c] + sum_{r,s,ch} W[c][r][s][ch] a[n][y+r-1][x+s-1][ch], a = relu(bn(z)) on load
//   head backward  : dy = conv^T(dlogits) (+ the fused BatchNorm+ReLU backward reduce of the head's input layer), dW, db
//   multi-label    : BCEWithLogitsLoss() + smp DiceLoss("multilabel")    (sigmoid per channel, target fp32 [N][C][H][W])
//   multi-class    : CrossEntropyLoss() + smp DiceLoss("multiclass")     (softmax over channels, target int64 [N][H][W])
// The binary model (C = 1) keeps its own kernels in elementwise.hip; nothing here runs for it.  Logits and dlogits are fp32 NCHW
// (class planes), the head input is the 16-channel NHWC tensor of decoder.blocks.4.conv2.  Every reduction that feeds a weight
// gradient or a loss value goes through per-workgroup partials added in a fixed order: the same inputs give the same bits.
#include <math.h>

#include "vk_common.h"

namespace vk {

typedef float f32x2_t __attribute__((ext_vector_type(2)));
constexpr int kMaxClasses = 16;
constexpr int kHaloPx = 18 * 18;

// ---- head forward: 16x16 pixel tile per workgroup; the 18x18x16 activated halo is staged in LDS as fp32 (as in k_head_fwd), a thread
// computes its pixel for every class with packed FMAs (one f32x2 accumulator per class: C independent chains).  The filter is read
// through uniform addresses with compile-time offsets (scalar loads).
template <typename T>
__global__ __launch_bounds__(256) void k_head_fwd_multi(int N, int H, int W, int C, int tiles_x, int tiles_y, const T* __restrict__ z,
                                                        const float* __restrict__ scale, const float* __restrict__ shift, int relu,
                                                        const float* __restrict__ w, const float* __restrict__ bias,
                                                        float* __restrict__ logits) {
  constexpr int VE = ElemTraits<T>::kVec, VPP = 16 / VE;
  constexpr int PS = 20;
  __shared__ __attribute__((aligned(16))) float tile[kHaloPx * PS];
  const int tid = threadIdx.x;
  int bt = blockIdx.x;
  const int tx0 = bt % tiles_x;
  bt /= tiles_x;
  const int ty0 = bt % tiles_y;
  const int n = bt / tiles_y;
  const int y0 = ty0 * 16, x0 = tx0 * 16;
  const bool affine = scale != nullptr;
  const int vec = tid % VPP;
  float sc[VE], sh[VE];
#pragma unroll
  for (int j = 0; j < VE; ++j) { sc[j] = affine ? scale[vec * VE + j] : 1.f; sh[j] = affine ? shift[vec * VE + j] : 0.f; }
  constexpr int NHV = (kHaloPx * VPP + 255) / 256;
  u32x4_t raw[NHV];
  bool inb[NHV];
#pragma unroll
  for (int i = 0; i < NHV; ++i) {
    const int v = tid + i * 256;
    const int hp = v / VPP;
    const int hy = hp / 18, hx = hp - hy * 18;
    const int y = y0 - 1 + hy, x = x0 - 1 + hx;
    inb[i] = v < kHaloPx * VPP && (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
    raw[i] = u32x4_t{0, 0, 0, 0};
    if (inb[i]) raw[i] = *reinterpret_cast<const u32x4_t*>(z + (((size_t)n * H + y) * W + x) * 16 + vec * VE);
  }
#pragma unroll
  for (int i = 0; i < NHV; ++i) {
    const int v = tid + i * 256;
    if (v >= kHaloPx * VPP) continue;
    const int hp = v / VPP;
    float f[VE];
    Vec16<T>::unpack(raw[i], f);
#pragma unroll
    for (int j = 0; j < VE; ++j) {
      if (affine) {
        f[j] = fmaf(f[j], sc[j], sh[j]);
        if (relu) f[j] = fmaxf(f[j], 0.f);
      }
      if (!inb[i]) f[j] = 0.f;
    }
#pragma unroll
    for (int j = 0; j < VE; j += 4) *reinterpret_cast<f32x4_t*>(&tile[hp * PS + vec * VE + j]) = f32x4_t{f[j], f[j + 1], f[j + 2], f[j + 3]};
  }
  __syncthreads();
  const int ty = tid >> 4, tx = tid & 15;
  f32x2_t acc[kMaxClasses];
#pragma unroll
  for (int c = 0; c < kMaxClasses; ++c) acc[c] = f32x2_t{c < C ? bias[c] : 0.f, 0.f};
  // taps in a rolled loop: per tap and class the 16 filter values are one scalar load (all 144 C of them would not fit)
#pragma unroll 1
  for (int tap = 0; tap < 9; ++tap) {
    const int r = tap / 3, s = tap - 3 * r;
    const float* a = &tile[((ty + r) * 18 + tx + s) * PS];
    f32x4_t av[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) av[q] = *reinterpret_cast<const f32x4_t*>(a + 4 * q);
#pragma unroll
    for (int c = 0; c < kMaxClasses; ++c) {
      if (c < C) {
        const float* wt = w + (c * 9 + tap) * 16;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          acc[c] = __builtin_elementwise_fma(f32x2_t{av[q][0], av[q][1]}, f32x2_t{wt[4 * q], wt[4 * q + 1]}, acc[c]);
          acc[c] = __builtin_elementwise_fma(f32x2_t{av[q][2], av[q][3]}, f32x2_t{wt[4 * q + 2], wt[4 * q + 3]}, acc[c]);
        }
      }
    }
  }
  const int y = y0 + ty, x = x0 + tx;
  if (y < H && x < W) {
#pragma unroll
    for (int c = 0; c < kMaxClasses; ++c)
      if (c < C) logits[(((size_t)n * C + c) * H + y) * W + x] = acc[c][0] + acc[c][1];
  }
}

// ---- head backward, data + weights in one pass.  Persistent workgroups walk 16x16 tiles; per tile the C planes of the dlogits halo
// and the activated input of the tile's 256 pixels are staged in LDS (fp32), then
//   * data gradient, thread = pixel: dy[px][ch] = sum_{c,tap} W[c][tap][ch] dl[c][px + (1-r, 1-s)] (9 C FMAs per channel), rounded to
//     T, masked by the ReLU of the head's input layer and summed into its BatchNorm-backward sums (as k_head_dgrad does);
//   * weight gradient, thread = (class, tap) pair x pixel group: dW[c][tap][0..15] += dl[c][px + (1-r, 1-s)] a[px][0..15] — the
//     lanes of one group read the same activation row (LDS broadcast);
//   * bias gradient: db[c] += dl[c][px].
// The workgroup's dW / db go to its row of `part` (144 C + C floats), in a fixed order; k_head_multi_reduce adds the rows in order.
template <typename T>
__global__ __launch_bounds__(256) void k_head_bwd_multi(int N, int H, int W, int C, int tiles_x, int tiles_y, int ntiles,
                                                        const T* __restrict__ z, const float* __restrict__ scale,
                                                        const float* __restrict__ shift, int relu, const float* __restrict__ w,
                                                        const float* __restrict__ dl, T* __restrict__ dy, const T* __restrict__ bnr_z,
                                                        const float* __restrict__ bnr_scale, const float* __restrict__ bnr_shift,
                                                        double* bnr_sums, float* __restrict__ part) {
  constexpr int VE = ElemTraits<T>::kVec, VPP = 16 / VE;
  constexpr int PS = 20;                                     // floats per staged pixel (16 + 4 pad)
  __shared__ __attribute__((aligned(16))) float as[256 * PS];
  __shared__ float dls[kMaxClasses * kHaloPx];
  __shared__ float bred[4][32];
  __shared__ float gred[4][kMaxClasses];
  const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15, lane = tid & 63, wave = tid >> 6;
  const bool affine = scale != nullptr;
  const int P = 9 * C, G = 256 / P;                          // (class, tap) pairs and pixel groups of the weight gradient
  const bool wg = tid < P * G;
  const int wp = wg ? tid % P : 0, wgroup = wg ? tid / P : 0;
  const int wc = wp / 9, wtap = wp - wc * 9, wr = wtap / 3, ws = wtap - wr * 3;
  float sc[16], sh[16], bsc[16], bsh[16], s1[16], s2[16], gw[16], gb[kMaxClasses];
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    sc[j] = affine ? scale[j] : 1.f;
    sh[j] = affine ? shift[j] : 0.f;
    bsc[j] = bnr_z ? bnr_scale[j] : 1.f;
    bsh[j] = bnr_z ? bnr_shift[j] : 0.f;
    s1[j] = 0.f; s2[j] = 0.f; gw[j] = 0.f;
  }
#pragma unroll
  for (int c = 0; c < kMaxClasses; ++c) gb[c] = 0.f;
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    int bt = t;
    const int tx0 = bt % tiles_x;
    bt /= tiles_x;
    const int ty0 = bt % tiles_y;
    const int n = bt / tiles_y;
    const int y0 = ty0 * 16, x0 = tx0 * 16;
    const int y = y0 + ty, x = x0 + tx;
    const bool inb = y < H && x < W;
    const size_t off = (((size_t)n * H + (inb ? y : 0)) * W + (inb ? x : 0)) * 16;
    float zf[16];
    {
      u32x4_t zr[VPP];
#pragma unroll
      for (int v = 0; v < VPP; ++v) zr[v] = *reinterpret_cast<const u32x4_t*>(z + off + v * VE);
      float a[16];
#pragma unroll
      for (int v = 0; v < VPP; ++v) Vec16<T>::unpack(zr[v], a + v * VE);
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        if (affine) {
          a[j] = fmaf(a[j], sc[j], sh[j]);
          if (relu) a[j] = fmaxf(a[j], 0.f);
        }
        if (!inb) a[j] = 0.f;                  // pixels outside the map add nothing to dW
      }
#pragma unroll
      for (int j = 0; j < 16; j += 4) *reinterpret_cast<f32x4_t*>(&as[tid * PS + j]) = f32x4_t{a[j], a[j + 1], a[j + 2], a[j + 3]};
      if (bnr_z) {
        if (bnr_z != z) {
#pragma unroll
          for (int v = 0; v < VPP; ++v) zr[v] = *reinterpret_cast<const u32x4_t*>(bnr_z + off + v * VE);
        }
#pragma unroll
        for (int v = 0; v < VPP; ++v) Vec16<T>::unpack(zr[v], zf + v * VE);
      }
    }
    for (int i = tid; i < C * kHaloPx; i += 256) {
      const int c = i / kHaloPx, hp = i - c * kHaloPx;
      const int hy = hp / 18, hx = hp - hy * 18;
      const int yy = y0 - 1 + hy, xx = x0 - 1 + hx;
      dls[i] = ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W) ? dl[(((size_t)n * C + c) * H + yy) * W + xx] : 0.f;
    }
    __syncthreads();
    // ---- data gradient (thread = pixel)
    float o[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) o[j] = 0.f;
#pragma unroll
    for (int c = 0; c < kMaxClasses; ++c)
      if (c < C) gb[c] += dls[c * kHaloPx + (ty + 1) * 18 + tx + 1];
#pragma unroll 1
    for (int p = 0; p < P; ++p) {    // (class, tap) pairs in a rolled loop: one scalar load of 16 filter values each
      const int c = p / 9, tap = p - 9 * c, r = tap / 3, s = tap - 3 * r;
      const float dv = dls[c * kHaloPx + (ty + 2 - r) * 18 + tx + 2 - s];   // halo origin (y0-1, x0-1): pixel + (1 - r, 1 - s)
      const float* wt = w + p * 16;
#pragma unroll
      for (int j = 0; j < 16; ++j) o[j] = fmaf(dv, wt[j], o[j]);
    }
    if (inb) {
#pragma unroll
      for (int v = 0; v < VPP; ++v) {
        u32x4_t pk = Vec16<T>::pack(o + v * VE);
        if (bnr_z) {       // g = dy * [relu(bn(z)) > 0]; sums over the stored values
          float g[VE];
          Vec16<T>::unpack(pk, g);
#pragma unroll
          for (int j = 0; j < VE; ++j) {
            if (!(fmaf(zf[v * VE + j], bsc[v * VE + j], bsh[v * VE + j]) > 0.f)) g[j] = 0.f;
            s1[v * VE + j] += g[j];
            s2[v * VE + j] += g[j] * zf[v * VE + j];
          }
          pk = Vec16<T>::pack(g);
        }
        *reinterpret_cast<u32x4_t*>(dy + off + v * VE) = pk;
      }
    }
    // ---- weight gradient (thread = (class, tap) pair of one pixel group)
    if (wg) {
      const float* d = dls + wc * kHaloPx + (2 - wr) * 18 + 2 - ws;
      for (int px = wgroup; px < 256; px += G) {
        const float dv = d[(px >> 4) * 18 + (px & 15)];
        const float* a = &as[px * PS];
#pragma unroll
        for (int j = 0; j < 16; j += 4) {
          const f32x4_t av = *reinterpret_cast<const f32x4_t*>(a + j);
          gw[j] = fmaf(dv, av[0], gw[j]);
          gw[j + 1] = fmaf(dv, av[1], gw[j + 1]);
          gw[j + 2] = fmaf(dv, av[2], gw[j + 2]);
          gw[j + 3] = fmaf(dv, av[3], gw[j + 3]);
        }
      }
    }
    __syncthreads();                 // the staged tiles are rewritten by the next iteration
  }
  if (bnr_z) {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const float a = wave_sum(s1[j]), b = wave_sum(s2[j]);
      if (lane == 0) { bred[wave][j] = a; bred[wave][16 + j] = b; }
    }
  }
#pragma unroll
  for (int c = 0; c < kMaxClasses; ++c) {
    if (c < C) {
      const float v = wave_sum(gb[c]);
      if (lane == 0) gred[wave][c] = v;
    }
  }
  float* red = as;                   // [G][P][16] (P G <= 256): the pair partials, then added over the groups in order
  if (wg) {
#pragma unroll
    for (int j = 0; j < 16; ++j) red[tid * 16 + j] = gw[j];
  }
  __syncthreads();
  if (bnr_z && tid < 32) {
    const float v = bred[0][tid] + bred[1][tid] + bred[2][tid] + bred[3][tid];
    atomicAdd(bnr_sums + (size_t)(blockIdx.x % VK_STATS_REPLICAS) * 32 + tid, (double)v);   // [replica][2][16]
  }
  const int nout = 145 * C;
  float* row = part + (size_t)blockIdx.x * nout;
  for (int o = tid; o < 144 * C; o += 256) {
    float v = 0.f;
    for (int g = 0; g < G; ++g) v += red[g * P * 16 + o];
    row[o] = v;
  }
  if (tid < C) row[144 * C + tid] = gred[0][tid] + gred[1][tid] + gred[2][tid] + gred[3][tid];
}

// dw[0 .. 144 C) / db[0 .. C) += sum of the nb rows of `part` in a fixed order: 16 lanes per output each add every 16th row, then the
// 16 lane sums in lane order
__global__ __launch_bounds__(256) void k_head_multi_reduce(int nb, int C, const float* __restrict__ part, float* dw, float* db) {
  const int nout = 145 * C;
  const int o = blockIdx.x * 16 + (threadIdx.x & 15), l = threadIdx.x >> 4;
  __shared__ float red[16][17];
  float s = 0.f;
  if (o < nout)
    for (int b = l; b < nb; b += 16) s += part[(size_t)b * nout + o];
  red[l][threadIdx.x & 15] = s;
  __syncthreads();
  if (l == 0 && o < nout) {
    float v = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) v += red[j][threadIdx.x & 15];
    if (o < 144 * C) dw[o] += v;
    else db[o - 144 * C] += v;
  }
}

// ------------------------------------------------------------------------------------------------ losses
// Per-workgroup partial rows of fp64 sums, then ONE workgroup adds the rows of every quantity in a fixed order (thread-strided,
// then a fixed tree) and writes loss_out plus the per-class gradient coefficients coef[0..16) (multiplies the target / one-hot),
// coef[16..32) (constant term), coef[32] (weight of the pixel-wise term / its count), coef[33] (bad labels).

// ordered sum over rows [0, nrows) of column q of part[row * ld + q] by the 256 threads of the workgroup (result in every thread)
__device__ double ordered_sum(const double* part, int nrows, int ld, int q, double* lds) {
  double s = 0.0;
  for (int r = threadIdx.x; r < nrows; r += 256) s += part[(size_t)r * ld + q];
  lds[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) lds[threadIdx.x] += lds[threadIdx.x + w];
    __syncthreads();
  }
  const double v = lds[0];
  __syncthreads();
  return v;
}

// ---- multi-label: block (bx, plane = n C + c) sums {bce, p y, p, y} over its share of the plane
__global__ __launch_bounds__(256) void k_ml_reduce(int HW, int nbx, const float* __restrict__ x, const float* __restrict__ y,
                                                   double* __restrict__ part) {
  const int plane = blockIdx.y;
  const float* xp = x + (size_t)plane * HW;
  const float* yp = y + (size_t)plane * HW;
  double bce = 0.0, py = 0.0, ps = 0.0, ys = 0.0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += nbx * 256) {
    const float xv = xp[i], yv = yp[i];
    bce += (double)(fmaxf(xv, 0.f) - xv * yv + log1pf(expf(-fabsf(xv))));
    const float p = 1.f / (1.f + expf(-xv));
    py += (double)(p * yv);
    ps += (double)p;
    ys += (double)yv;
  }
  __shared__ double red[4][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double a = wave_sum_d(bce), b = wave_sum_d(py), c = wave_sum_d(ps), d = wave_sum_d(ys);
  if (lane == 0) { red[wave][0] = a; red[wave][1] = b; red[wave][2] = c; red[wave][3] = d; }
  __syncthreads();
  if (threadIdx.x < 4) {
    const int q = threadIdx.x;
    part[((size_t)plane * nbx + blockIdx.x) * 4 + q] = ((red[0][q] + red[1][q]) + red[2][q]) + red[3][q];
  }
}

// Dice of one class from its sums (smp soft_dice_score, smooth 0): loss term, and the two gradient coefficients of d(term)/dp_i =
// ky * t_i + k0 (eps clamp: the cardinality's gradient is cut when it binds)
__device__ void dice_class(double I, double Ps, double Ts, double wscale, double* term, double* ky, double* k0) {
  const double eps = 1e-7;
  const double card = Ps + Ts;
  const double den = card > eps ? card : eps;
  const double mask = Ts > 0.0 ? 1.0 : 0.0;
  *term = (1.0 - 2.0 * I / den) * mask;
  *ky = -2.0 * wscale * mask / den;
  *k0 = card > eps ? 2.0 * wscale * mask * I / (den * den) : 0.0;
}

__global__ __launch_bounds__(256) void k_ml_finalize(int N, int C, int nbx, double count, const double* __restrict__ part,
                                                     double* __restrict__ coef, float* loss_out, float w_bce, float w_dice) {
  __shared__ double lds[256];
  __shared__ double cls[kMaxClasses][3];
  const int rows = N * C * nbx;
  const double bce_sum = ordered_sum(part, rows, 4, 0, lds);
  for (int c = 0; c < C; ++c) {
    for (int q = 1; q < 4; ++q) {
      // rows of class c: plane n C + c, block bx -> row (n C + c) nbx + bx; visited in (n, bx) order
      double s = 0.0;
      for (int r = threadIdx.x; r < N * nbx; r += 256) {
        const int n = r / nbx, bx = r - n * nbx;
        s += part[(((size_t)n * C + c) * nbx + bx) * 4 + q];
      }
      lds[threadIdx.x] = s;
      __syncthreads();
      for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) lds[threadIdx.x] += lds[threadIdx.x + w];
        __syncthreads();
      }
      if (threadIdx.x == 0) cls[c][q - 1] = lds[0];
      __syncthreads();
    }
  }
  if (threadIdx.x == 0) {
    const double bce = bce_sum / count;
    double dice = 0.0;
    for (int c = 0; c < C; ++c) {
      double term, ky, k0;
      dice_class(cls[c][0], cls[c][1], cls[c][2], (double)w_dice / C, &term, &ky, &k0);
      dice += term;
      coef[c] = ky;
      coef[kMaxClasses + c] = k0;
    }
    dice /= C;
    coef[32] = (double)w_bce / count;
    coef[33] = 0.0;
    loss_out[0] = (float)(w_bce * bce + w_dice * dice);
    loss_out[1] = (float)bce;
    loss_out[2] = (float)dice;
    loss_out[3] = 0.f;
  }
}

__global__ __launch_bounds__(256) void k_ml_bwd(int C, int HW, int nbx, const float* __restrict__ x, const float* __restrict__ y,
                                                const double* __restrict__ coef, float grad_scale, float* __restrict__ dl) {
  const int plane = blockIdx.y, c = plane % C;
  const float ky = (float)coef[c], k0 = (float)coef[kMaxClasses + c], invc = (float)coef[32];
  const size_t base = (size_t)plane * HW;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += nbx * 256) {
    const float xv = x[base + i], yv = y[base + i];
    const float p = 1.f / (1.f + expf(-xv));
    const float g = (p - yv) * invc + (ky * yv + k0) * p * (1.f - p);
    dl[base + i] = g * grad_scale;
  }
}

// ---- multi-class: block (bx, n) sums {ce, bad labels, I[C], P[C], T[C]} over its share of image n's pixels
__device__ __forceinline__ bool softmax_px(int C, const float* __restrict__ xp, size_t stride, float* p, float* lse, float* xl, int label) {
  float xv[kMaxClasses];
  float m = -INFINITY;
#pragma unroll
  for (int c = 0; c < kMaxClasses; ++c) {
    xv[c] = c < C ? xp[c * stride] : -INFINITY;
    m = fmaxf(m, xv[c]);
  }
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < kMaxClasses; ++c) {
    p[c] = c < C ? expf(xv[c] - m) : 0.f;
    s += p[c];
  }
  const float inv = 1.f / s;
  *xl = 0.f;
#pragma unroll
  for (int c = 0; c < kMaxClasses; ++c) {
    p[c] *= inv;
    if (c == label) *xl = xv[c];
  }
  *lse = m + logf(s);
  return label >= 0 && label < C;
}

__global__ __launch_bounds__(256) void k_mc_reduce(int C, int HW, int nbx, const float* __restrict__ x, const int64_t* __restrict__ t,
                                                   double* __restrict__ part) {
  const int n = blockIdx.y;
  const int Q = 3 * C + 2;
  const float* xn = x + (size_t)n * C * HW;
  const int64_t* tn = t + (size_t)n * HW;
  double ce = 0.0, bad = 0.0, I[kMaxClasses], Ps[kMaxClasses], Ts[kMaxClasses];
#pragma unroll
  for (int c = 0; c < kMaxClasses; ++c) { I[c] = 0.0; Ps[c] = 0.0; Ts[c] = 0.0; }
  for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += nbx * 256) {
    const int64_t lab = tn[i];
    const int label = (lab >= 0 && lab < C) ? (int)lab : -1;
    float p[kMaxClasses], lse, xl;
    if (!softmax_px(C, xn + i, (size_t)HW, p, &lse, &xl, label)) {
      bad += 1.0;                    // out-of-range label: reported through coef[33] / loss_out[3], the pixel adds nothing
      continue;
    }
    ce += (double)(lse - xl);
#pragma unroll
    for (int c = 0; c < kMaxClasses; ++c) {
      if (c < C) {
        Ps[c] += (double)p[c];
        if (c == label) { I[c] += (double)p[c]; Ts[c] += 1.0; }
      }
    }
  }
  __shared__ double red[4][3 * kMaxClasses + 2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  {
    const double a = wave_sum_d(ce), b = wave_sum_d(bad);
    if (lane == 0) { red[wave][0] = a; red[wave][1] = b; }
  }
#pragma unroll
  for (int c = 0; c < kMaxClasses; ++c) {
    if (c < C) {
      const double a = wave_sum_d(I[c]), b = wave_sum_d(Ps[c]), d = wave_sum_d(Ts[c]);
      if (lane == 0) { red[wave][2 + c] = a; red[wave][2 + C + c] = b; red[wave][2 + 2 * C + c] = d; }
    }
  }
  __syncthreads();
  for (int q = threadIdx.x; q < Q; q += 256)
    part[((size_t)n * nbx + blockIdx.x) * Q + q] = ((red[0][q] + red[1][q]) + red[2][q]) + red[3][q];
}

__global__ __launch_bounds__(256) void k_mc_finalize(int N, int C, int nbx, double count, const double* __restrict__ part,
                                                     double* __restrict__ coef, float* loss_out, float w_ce, float w_dice) {
  __shared__ double lds[256];
  __shared__ double tot[3 * kMaxClasses + 2];
  const int Q = 3 * C + 2, rows = N * nbx;
  for (int q = 0; q < Q; ++q) {
    const double v = ordered_sum(part, rows, Q, q, lds);
    if (threadIdx.x == 0) tot[q] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double bad = tot[1];
    const double ce = tot[0] / count;
    double dice = 0.0;
    for (int c = 0; c < C; ++c) {
      double term, ky, k0;
      dice_class(tot[2 + c], tot[2 + C + c], tot[2 + 2 * C + c], (double)w_dice / C, &term, &ky, &k0);
      dice += term;
      coef[c] = ky;
      coef[kMaxClasses + c] = k0;
    }
    dice /= C;
    coef[32] = (double)w_ce / count;
    coef[33] = bad;
    const float nan = __builtin_nanf("");
    loss_out[0] = bad > 0.0 ? nan : (float)(w_ce * ce + w_dice * dice);
    loss_out[1] = bad > 0.0 ? nan : (float)ce;
    loss_out[2] = bad > 0.0 ? nan : (float)dice;
    loss_out[3] = (float)bad;
  }
}

// dx_k = w_ce (p_k - [k = t]) / count + p_k (g_k - sum_j p_j g_j),  g_k = d(w_dice dice)/dp_k = ky_k [k = t] + k0_k
__global__ __launch_bounds__(256) void k_mc_bwd(int C, int HW, int nbx, const float* __restrict__ x, const int64_t* __restrict__ t,
                                                const double* __restrict__ coef, float grad_scale, float* __restrict__ dl) {
  const int n = blockIdx.y;
  const float* xn = x + (size_t)n * C * HW;
  float* dn = dl + (size_t)n * C * HW;
  const int64_t* tn = t + (size_t)n * HW;
  float ky[kMaxClasses], k0[kMaxClasses];
#pragma unroll
  for (int c = 0; c < kMaxClasses; ++c) { ky[c] = c < C ? (float)coef[c] : 0.f; k0[c] = c < C ? (float)coef[kMaxClasses + c] : 0.f; }
  const float invc = (float)coef[32];
  for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += nbx * 256) {
    const int64_t lab = tn[i];
    const int label = (lab >= 0 && lab < C) ? (int)lab : -1;
    float p[kMaxClasses], lse, xl;
    const bool ok = softmax_px(C, xn + i, (size_t)HW, p, &lse, &xl, label);
    float g[kMaxClasses], pg = 0.f;
#pragma unroll
    for (int c = 0; c < kMaxClasses; ++c) {
      g[c] = (c == label ? ky[c] : 0.f) + k0[c];
      pg = fmaf(p[c], g[c], pg);
    }
#pragma unroll
    for (int c = 0; c < kMaxClasses; ++c) {
      if (c < C) {
        const float v = (p[c] - (c == label ? 1.f : 0.f)) * invc + p[c] * (g[c] - pg);
        dn[(size_t)c * HW + i] = ok ? v * grad_scale : 0.f;
      }
    }
  }
}

}  // namespace vk

// =================================================================================================
// C ABI wrappers
// =================================================================================================
using namespace vk;

#define DISPATCH_T(dt, CALL)                         \
  switch (dt) {                                      \
    case VK_F32: { using T = float; CALL; } break;   \
    case VK_BF16: { using T = bf16_t; CALL; } break; \
    case VK_F16: { using T = f16_t; CALL; } break;   \
    default: vkh::set_error("bad dtype %d", (int)dt); return VK_ERR_ARG; \
  }

extern "C" int vk_head_fwd_multi(vk_dtype dtype, int N, int H, int W, int C, const vk_src* src, const float* w, const float* bias,
                                 float* logits, void* stream) {
  VK_CHECK_ARG(src && src->ptr && w && bias && logits, "vk_head_fwd_multi: null argument");
  VK_CHECK_ARG(src->C == 16 && !src->up, "vk_head_fwd_multi: head input must have 16 channels, no upsample");
  VK_CHECK_ARG(N >= 1 && H >= 1 && W >= 1 && C >= 1 && C <= kMaxClasses, "vk_head_fwd_multi: bad shape N=%d H=%d W=%d C=%d", N, H, W, C);
  hipStream_t st = (hipStream_t)stream;
  vkh::ProfScope ps_("head_fwd_multi", st, 2.0 * 144.0 * C * N * H * W,
                     (double)N * H * W * (16.0 * (dtype == VK_F32 ? 4.0 : 2.0) + 4.0 * C));
  const int tx = (W + 15) / 16, ty = (H + 15) / 16;
  DISPATCH_T(dtype, hipLaunchKernelGGL(k_head_fwd_multi<T>, dim3((unsigned)(N * tx * ty)), dim3(256), 0, st, N, H, W, C, tx, ty,
                                       (const T*)src->ptr, src->scale, src->shift, src->relu, w, bias, logits));
  VK_CHECK_HIP(hipGetLastError());
  return VK_OK;
}

extern "C" size_t vk_head_multi_workspace_bytes(int C) {
  return C >= 1 && C <= kMaxClasses ? (size_t)1024 * 145 * C * sizeof(float) : 0;
}

extern "C" int vk_head_bwd_multi(vk_dtype dtype, int N, int H, int W, int C, const vk_src* src, const float* w, const float* dlogits,
                                 void* dy, float* dw, float* dbias, const vk_bnr* bnr, void* workspace, size_t workspace_bytes,
                                 void* stream) {
  VK_CHECK_ARG(src && src->ptr && w && dlogits && dy && dw && dbias && workspace, "vk_head_bwd_multi: null argument");
  VK_CHECK_ARG(src->C == 16 && !src->up, "vk_head_bwd_multi: head input must have 16 channels, no upsample");
  VK_CHECK_ARG(N >= 1 && H >= 1 && W >= 1 && C >= 1 && C <= kMaxClasses, "vk_head_bwd_multi: bad shape N=%d H=%d W=%d C=%d", N, H, W, C);
  VK_CHECK_ARG(!bnr || (bnr->z && bnr->scale && bnr->shift && bnr->sums), "vk_head_bwd_multi: incomplete vk_bnr");
  const size_t row = (size_t)145 * C * sizeof(float);
  VK_CHECK_ARG(workspace_bytes >= row, "vk_head_bwd_multi: workspace of %zu bytes is below one row (%zu)", workspace_bytes, row);
  hipStream_t st = (hipStream_t)stream;
  const int tx = (W + 15) / 16, ty = (H + 15) / 16;
  const int ntiles = N * tx * ty;
  const double eb = dtype == VK_F32 ? 4.0 : 2.0;
  int nb = ntiles < 1024 ? ntiles : 1024;
  if ((size_t)nb > workspace_bytes / row) nb = (int)(workspace_bytes / row);
  vkh::ProfScope ps_("head_bwd_multi", st, 4.0 * 144.0 * C * N * H * W, (double)N * H * W * (16.0 * eb * 2.0 + 4.0 * C));
  DISPATCH_T(dtype, hipLaunchKernelGGL(k_head_bwd_multi<T>, dim3((unsigned)nb), dim3(256), 0, st, N, H, W, C, tx, ty, ntiles,
                                       (const T*)src->ptr, src->scale, src->shift, src->relu, w, dlogits, (T*)dy,
                                       (const T*)(bnr ? bnr->z : nullptr), bnr ? bnr->scale : nullptr, bnr ? bnr->shift : nullptr,
                                       bnr ? bnr->sums : nullptr, (float*)workspace));
  hipLaunchKernelGGL(k_head_multi_reduce, dim3((unsigned)((145 * C + 15) / 16)), dim3(256), 0, st, nb, C, (const float*)workspace, dw, dbias);
  VK_CHECK_HIP(hipGetLastError());
  return VK_OK;
}

namespace {
int loss_nbx(int HW) {
  const int n = HW / 4096;
  return n < 1 ? 1 : (n > 64 ? 64 : n);
}
constexpr size_t kCoefBytes = 64 * sizeof(double);
}  // namespace

extern "C" size_t vk_multi_loss_workspace_bytes(int N, int C, int HW) {
  if (N < 1 || C < 1 || C > kMaxClasses || HW < 1) return 0;
  const size_t nbx = (size_t)loss_nbx(HW);
  const size_t ml = (size_t)N * C * nbx * 4, mc = (size_t)N * nbx * (3 * C + 2);
  return kCoefBytes + (ml > mc ? ml : mc) * sizeof(double);
}

extern "C" int vk_multilabel_loss(int N, int C, int HW, const float* logits, const float* target, void* workspace, size_t workspace_bytes,
                                  float* loss_out, float* dlogits, float grad_scale, float w_bce, float w_dice, void* stream) {
  VK_CHECK_ARG(logits && target && workspace && loss_out, "vk_multilabel_loss: null argument");
  VK_CHECK_ARG(N >= 1 && HW >= 1 && C >= 1 && C <= kMaxClasses, "vk_multilabel_loss: bad shape N=%d C=%d HW=%d", N, C, HW);
  VK_CHECK_ARG(workspace_bytes >= vk_multi_loss_workspace_bytes(N, C, HW), "vk_multilabel_loss: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const double count = (double)N * C * HW;
  vkh::ProfScope ps_("multilabel_loss", st, 0.0, count * (dlogits ? 20.0 : 8.0));
  const int nbx = loss_nbx(HW);
  double* coef = (double*)workspace;
  double* part = (double*)((char*)workspace + kCoefBytes);
  hipLaunchKernelGGL(k_ml_reduce, dim3((unsigned)nbx, (unsigned)(N * C)), dim3(256), 0, st, HW, nbx, logits, target, part);
  hipLaunchKernelGGL(k_ml_finalize, dim3(1), dim3(256), 0, st, N, C, nbx, count, (const double*)part, coef, loss_out, w_bce, w_dice);
  if (dlogits)
    hipLaunchKernelGGL(k_ml_bwd, dim3((unsigned)nbx, (unsigned)(N * C)), dim3(256), 0, st, C, HW, nbx, logits, target, (const double*)coef,
                       grad_scale, dlogits);
  VK_CHECK_HIP(hipGetLastError());
  return VK_OK;
}

extern "C" int vk_multiclass_loss(int N, int C, int HW, const float* logits, const int64_t* target, void* workspace, size_t workspace_bytes,
                                  float* loss_out, float* dlogits, float grad_scale, float w_ce, float w_dice, void* stream) {
  VK_CHECK_ARG(logits && target && workspace && loss_out, "vk_multiclass_loss: null argument");
  VK_CHECK_ARG(N >= 1 && HW >= 1 && C >= 1 && C <= kMaxClasses, "vk_multiclass_loss: bad shape N=%d C=%d HW=%d", N, C, HW);
  VK_CHECK_ARG(workspace_bytes >= vk_multi_loss_workspace_bytes(N, C, HW), "vk_multiclass_loss: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const double count = (double)N * HW;
  vkh::ProfScope ps_("multiclass_loss", st, 0.0, count * ((dlogits ? 12.0 : 4.0) * C + (dlogits ? 16.0 : 8.0)));
  const int nbx = loss_nbx(HW);
  double* coef = (double*)workspace;
  double* part = (double*)((char*)workspace + kCoefBytes);
  hipLaunchKernelGGL(k_mc_reduce, dim3((unsigned)nbx, (unsigned)N), dim3(256), 0, st, C, HW, nbx, logits, target, part);
  hipLaunchKernelGGL(k_mc_finalize, dim3(1), dim3(256), 0, st, N, C, nbx, count, (const double*)part, coef, loss_out, w_ce, w_dice);
  if (dlogits)
    hipLaunchKernelGGL(k_mc_bwd, dim3((unsigned)nbx, (unsigned)N), dim3(256), 0, st, C, HW, nbx, logits, target, (const double*)coef,
                       grad_scale, dlogits);
  VK_CHECK_HIP(hipGetLastError());
  return VK_OK;
}
