// Pointwise (1x1) convolutions — the Bottleneck conv1 / conv3 and the downsample shortcuts of the resnet50 encoder (reference:
// smp.Unet("resnet50") behind train.py:372) — as MFMA GEMMs over NHWC pixels (vk_conv1x1_fwd / vk_conv1x1_wgrad in vk_unet.h).
//
//   forward         y [m][k]  (+)= sum_c V[in(m)][c] * w [k][c]     m: output pixel, in(m) = the input pixel at stride s
//   data gradient   dx[out(m)][c] (+)= sum_k dz[m][k] * wt[c][k]   m: dz pixel, out(m) = the dx pixel at stride s (the others: 0)
//   weight gradient dw[k][c]  += sum_m dz[m][k] * V[in(m)][c]      split over pixels, partial tiles reduced in a fixed order
//
// V is the producer's BatchNorm scale / shift and ReLU applied while the operand is staged (the vk_src convention).  Forward and
// data gradient are the same kernel: both reduction operands are rows with the reduction dimension contiguous ("NT" GEMM), staged
// through LDS as [row][256 bytes] (four MFMA k-steps) with the next stage's global loads in flight in registers while the current
// stage's MFMAs run.  The weight gradient reduces over pixels, i.e. over the OUTER dimension of both operands: its loader writes the
// 16-byte channel vectors of a pixel transposed into the same [channel][pixels] LDS image, and the MFMA loop is the forward's.
// Every 16-bit layer runs v_mfma_f32_16x16x32_{bf16,f16}; fp32 runs v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 sums).
#include <algorithm>

#include "conv_host.h"

namespace vk {
namespace {

constexpr int kTile = 64;               // GEMM tile: 64 rows x 64 columns per workgroup, 4 waves of 32 x 32
constexpr int kRowB = 256;              // reduction bytes per LDS row and stage (4 MFMA k-steps of 64 bytes)
constexpr int kLdsRow = kRowB + 16;     // padded row: the 16 rows a lane group reads sit in distinct bank groups
constexpr int kOpBytes = kTile * kLdsRow;

struct Fwd1x1 {
  const void* x;          // GEMM-row source: NHWC [N][H][W][Cred]
  const float* scale;     // [Cred] or null
  const float* shift;
  int relu;
  const void* w;          // [Kout][Cred]
  void* y;                // NHWC [N][Ho][Wo][Kout]
  double* stats;          // [VK_STATS_REPLICAS][2][Kout] or null
  int Cred, Kout;
  int M;                  // GEMM rows: N * Hg * Wg
  int Hg, Wg;             // GEMM-row grid
  int H, W, Ho, Wo;       // input / output grids
  int in_s, out_s;        // log2 of the stride applied to the input (forward) / output (data gradient) pixel coordinates
  int accumulate;
};

struct Wg1x1 {
  const void* dz;         // [N][Ho][Wo][K]
  const void* x;          // [N][H][W][C]
  const float* scale;
  const float* shift;
  int relu;
  float* dw;              // [K][C] fp32, += (one split)
  float* part;            // [splits][K][C] fp32 partial tiles (several splits), or null
  int K, C, P;            // P = N * Ho * Wo
  int Ho, Wo, H, W, s;
  int px_per_split;       // a multiple of the stage's pixel count
};

template <typename T>
__device__ __forceinline__ u32x4_t transform(u32x4_t v, const float* __restrict__ scale, const float* __restrict__ shift, int relu, int c0) {
  constexpr int VE = ElemTraits<T>::kVec;
  float sc[VE], sh[VE];
  if (scale) {
#pragma unroll
    for (int q = 0; q < VE / 4; ++q) {
      const f32x4_t a = *reinterpret_cast<const f32x4_t*>(scale + c0 + 4 * q);
      const f32x4_t b = *reinterpret_cast<const f32x4_t*>(shift + c0 + 4 * q);
#pragma unroll
      for (int j = 0; j < 4; ++j) { sc[4 * q + j] = a[j]; sh[4 * q + j] = b[j]; }
    }
  } else {
#pragma unroll
    for (int j = 0; j < VE; ++j) { sc[j] = 1.f; sh[j] = 0.f; }
  }
  return AffineRelu<T>::run(v, sc, sh, relu != 0);
}

// the 4 x (2 x 2) MFMAs of one stage: wave tile rows [wm, wm + 32) of A, [wn, wn + 32) of B; `chunks` valid 64-byte k-steps
template <typename T>
__device__ __forceinline__ void mma_stage(const char* As, const char* Bs, int wm, int wn, int lane, int chunks, f32x4_t (&acc)[2][2]) {
  const int ro = (lane & 15) * kLdsRow + (lane >> 4) * 16;
  for (int c = 0; c < chunks; ++c) {
    const u32x4_t a0 = *reinterpret_cast<const u32x4_t*>(As + wm * kLdsRow + ro + c * 64);
    const u32x4_t a1 = *reinterpret_cast<const u32x4_t*>(As + (wm + 16) * kLdsRow + ro + c * 64);
    const u32x4_t b0 = *reinterpret_cast<const u32x4_t*>(Bs + wn * kLdsRow + ro + c * 64);
    const u32x4_t b1 = *reinterpret_cast<const u32x4_t*>(Bs + (wn + 16) * kLdsRow + ro + c * 64);
    acc[0][0] = Mma<T>::run(a0, b0, acc[0][0]);
    acc[0][1] = Mma<T>::run(a0, b1, acc[0][1]);
    acc[1][0] = Mma<T>::run(a1, b0, acc[1][0]);
    acc[1][1] = Mma<T>::run(a1, b1, acc[1][1]);
  }
}

// ------------------------------------------------------------------------------------------------ forward / data gradient
template <typename T>
__global__ __launch_bounds__(256) void k_conv1x1_fwd(Fwd1x1 p) {
  constexpr int EB = ElemTraits<T>::kBytes, VE = ElemTraits<T>::kVec;
  constexpr int VPR = kRowB / 16;                 // 16-byte vectors per row and stage
  constexpr int RPP = 256 / VPR;                  // rows per loader pass
  constexpr int LPT = kTile / RPP;                // loader passes (vectors per thread per operand)
  __shared__ __attribute__((aligned(16))) char smem[2 * kOpBytes];
  char* const As = smem;
  char* const Bs = smem + kOpBytes;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.x * kTile, n0 = blockIdx.y * kTile;
  const int lv = tid % VPR;
  const int HWg = p.Hg * p.Wg;
  const char* a_ptr[LPT];
  const char* b_ptr[LPT];
#pragma unroll
  for (int i = 0; i < LPT; ++i) {
    const int row = tid / VPR + i * RPP;
    const int m = m0 + row;
    a_ptr[i] = nullptr;
    if (m < p.M) {
      const int n = m / HWg, r = m - n * HWg, hg = r / p.Wg, wg = r - hg * p.Wg;
      const int64_t pix = ((int64_t)n * p.H + (hg << p.in_s)) * p.W + (wg << p.in_s);
      a_ptr[i] = (const char*)p.x + pix * p.Cred * EB;
    }
    const int k = n0 + row;
    b_ptr[i] = k < p.Kout ? (const char*)p.w + (int64_t)k * p.Cred * EB : nullptr;
  }
  const int CB = p.Cred * EB;
  const int nst = (CB + kRowB - 1) / kRowB;
  u32x4_t ra[LPT], rb[LPT];
  auto load = [&](int s) {
    const int cb = s * kRowB + lv * 16;
    const bool cok = cb < CB;
#pragma unroll
    for (int i = 0; i < LPT; ++i) {
      ra[i] = u32x4_t{0, 0, 0, 0};
      rb[i] = u32x4_t{0, 0, 0, 0};
      if (cok && a_ptr[i]) {
        ra[i] = *reinterpret_cast<const u32x4_t*>(a_ptr[i] + cb);
        if (p.scale || p.relu) ra[i] = transform<T>(ra[i], p.scale, p.shift, p.relu, cb / EB);
      }
      if (cok && b_ptr[i]) rb[i] = *reinterpret_cast<const u32x4_t*>(b_ptr[i] + cb);
    }
  };
  f32x4_t acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;
  load(0);
  for (int s = 0; s < nst; ++s) {
#pragma unroll
    for (int i = 0; i < LPT; ++i) {
      const int row = tid / VPR + i * RPP;
      *reinterpret_cast<u32x4_t*>(As + row * kLdsRow + lv * 16) = ra[i];
      *reinterpret_cast<u32x4_t*>(Bs + row * kLdsRow + lv * 16) = rb[i];
    }
    __syncthreads();
    if (s + 1 < nst) load(s + 1);                 // next stage's global loads run under this stage's MFMAs
    const int rem = CB - s * kRowB;
    mma_stage<T>(As, Bs, wm, wn, lane, rem >= kRowB ? 4 : (rem + 63) / 64, acc);
    __syncthreads();
  }
  // epilogue: the fp32 tile through LDS ([64 rows][64 floats], padded rows), then whole 16-byte output vectors per thread
  float* const Cs = reinterpret_cast<float*>(smem);
  constexpr int CROW = kLdsRow / 4;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) Cs[(wm + 16 * i + (lane >> 4) * 4 + e) * CROW + wn + 16 * j + (lane & 15)] = acc[i][j][e];
  __syncthreads();
  constexpr int VPO = kTile / VE;                 // output vectors per tile row
  constexpr int OPT = kTile * VPO / 256;          // output vectors per thread
  const int cv = tid % VPO;
  const int col = n0 + cv * VE;
  float s1[VE], s2[VE];
#pragma unroll
  for (int j = 0; j < VE; ++j) { s1[j] = 0.f; s2[j] = 0.f; }
  T* const y = (T*)p.y;
#pragma unroll
  for (int q = 0; q < OPT; ++q) {
    const int row = tid / VPO + q * (256 / VPO);
    const int m = m0 + row;
    if (m >= p.M || col >= p.Kout) continue;
    const int n = m / HWg, r = m - n * HWg, hg = r / p.Wg, wg = r - hg * p.Wg;
    const int oh = hg << p.out_s, ow = wg << p.out_s;
    const int64_t pix = ((int64_t)n * p.Ho + oh) * p.Wo + ow;
    u32x4_t* gp = reinterpret_cast<u32x4_t*>(y + pix * p.Kout + col);
    float f[VE];
#pragma unroll
    for (int j = 0; j < VE; ++j) f[j] = Cs[row * CROW + cv * VE + j];
    if (p.accumulate) {
      float o[VE];
      Vec16<T>::unpack(*gp, o);
#pragma unroll
      for (int j = 0; j < VE; ++j) f[j] += o[j];
    }
    const u32x4_t v = Vec16<T>::pack(f);
    Vec16<T>::unpack(v, f);                        // statistics of the stored (rounded) values
#pragma unroll
    for (int j = 0; j < VE; ++j) { s1[j] += f[j]; s2[j] += f[j] * f[j]; }
    *gp = v;
    if (p.out_s && !p.accumulate) {                // stride-2 data gradient: the pixels no output tap reaches are zero
      const u32x4_t z = u32x4_t{0, 0, 0, 0};
      if (ow + 1 < p.Wo) *reinterpret_cast<u32x4_t*>(y + (pix + 1) * p.Kout + col) = z;
      if (oh + 1 < p.Ho) {
        *reinterpret_cast<u32x4_t*>(y + (pix + p.Wo) * p.Kout + col) = z;
        if (ow + 1 < p.Wo) *reinterpret_cast<u32x4_t*>(y + (pix + p.Wo + 1) * p.Kout + col) = z;
      }
    }
  }
  if (p.stats) {
    __syncthreads();                               // Cs is read above; the partial sums reuse the LDS behind it
    float* red = reinterpret_cast<float*>(smem + kTile * kLdsRow);
#pragma unroll
    for (int j = 0; j < VE; ++j) { red[(tid * VE + j) * 2] = s1[j]; red[(tid * VE + j) * 2 + 1] = s2[j]; }
    __syncthreads();
    if (tid < kTile && n0 + tid < p.Kout) {
      const int c = tid / VE, j = tid % VE;
      float a = 0.f, b = 0.f;
      for (int t = c; t < 256; t += VPO) { a += red[(t * VE + j) * 2]; b += red[(t * VE + j) * 2 + 1]; }
      double* sp = p.stats + (size_t)(blockIdx.x % VK_STATS_REPLICAS) * 2 * p.Kout;
      atomicAdd(sp + n0 + tid, (double)a);
      atomicAdd(sp + p.Kout + n0 + tid, (double)b);
    }
  }
}

// ------------------------------------------------------------------------------------------------ weight gradient
template <typename T>
__global__ __launch_bounds__(256) void k_conv1x1_wgrad(Wg1x1 p) {
  constexpr int EB = ElemTraits<T>::kBytes, VE = ElemTraits<T>::kVec;
  constexpr int VPP = kTile / VE;                 // 16-byte channel vectors per pixel of a 64-channel tile
  constexpr int PPP = 256 / VPP;                  // pixels per loader pass
  constexpr int PS = kRowB / EB;                  // pixels per stage
  constexpr int LPT = PS / PPP;                   // loader passes
  __shared__ __attribute__((aligned(16))) char smem[2 * kOpBytes];
  char* const As = smem;                          // [dz channel k][pixels]
  char* const Bs = smem + kOpBytes;               // [input channel c][pixels]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tiles_c = (p.C + kTile - 1) / kTile;
  const int k0 = (blockIdx.x / tiles_c) * kTile, c0 = (blockIdx.x % tiles_c) * kTile;
  const int split = blockIdx.y;
  const int p_begin = split * p.px_per_split;
  const int p_end = min(p.P, p_begin + p.px_per_split);
  const int cv = tid % VPP;                       // this thread's channel vector (the same in every pass)
  const int kk = k0 + cv * VE, cc = c0 + cv * VE;
  const bool k_ok = kk < p.K, c_ok = cc < p.C;
  float sc[VE], sh[VE];
#pragma unroll
  for (int j = 0; j < VE; ++j) {
    sc[j] = (p.scale && c_ok) ? p.scale[cc + j] : 1.f;
    sh[j] = (p.shift && c_ok) ? p.shift[cc + j] : 0.f;
  }
  const bool tf = p.scale || p.relu;
  const int HWo = p.Ho * p.Wo;
  const T* dz = (const T*)p.dz;
  const T* x = (const T*)p.x;
  u32x4_t ra[LPT], rb[LPT];
  auto load = [&](int pb) {
#pragma unroll
    for (int i = 0; i < LPT; ++i) {
      const int m = pb + tid / VPP + i * PPP;
      ra[i] = u32x4_t{0, 0, 0, 0};
      rb[i] = u32x4_t{0, 0, 0, 0};
      if (m < p_end) {
        if (k_ok) ra[i] = *reinterpret_cast<const u32x4_t*>(dz + (int64_t)m * p.K + kk);
        if (c_ok) {
          int64_t pix = m;
          if (p.s) {
            const int n = m / HWo, r = m - n * HWo, ho = r / p.Wo, wo = r - ho * p.Wo;
            pix = ((int64_t)n * p.H + (ho << p.s)) * p.W + (wo << p.s);
          }
          rb[i] = *reinterpret_cast<const u32x4_t*>(x + pix * p.C + cc);
          if (tf) rb[i] = AffineRelu<T>::run(rb[i], sc, sh, p.relu != 0);
        }
      }
    }
  };
  // transposed store: element j of the vector of pixel pp goes to row (cv*VE + j), column pp
  auto store = [&]() {
#pragma unroll
    for (int i = 0; i < LPT; ++i) {
      const int pp = tid / VPP + i * PPP;
      if constexpr (EB == 4) {
#pragma unroll
        for (int j = 0; j < VE; ++j) {
          *reinterpret_cast<uint32_t*>(As + (cv * VE + j) * kLdsRow + pp * 4) = ra[i][j];
          *reinterpret_cast<uint32_t*>(Bs + (cv * VE + j) * kLdsRow + pp * 4) = rb[i][j];
        }
      } else {
#pragma unroll
        for (int j = 0; j < VE; ++j) {
          const uint32_t wa = ra[i][j >> 1], wb = rb[i][j >> 1];
          *reinterpret_cast<uint16_t*>(As + (cv * VE + j) * kLdsRow + pp * 2) = (uint16_t)((j & 1) ? wa >> 16 : wa);
          *reinterpret_cast<uint16_t*>(Bs + (cv * VE + j) * kLdsRow + pp * 2) = (uint16_t)((j & 1) ? wb >> 16 : wb);
        }
      }
    }
  };
  f32x4_t acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;
  if (p_begin < p_end) {
    load(p_begin);
    for (int pb = p_begin; pb < p_end; pb += PS) {
      store();
      __syncthreads();
      if (pb + PS < p_end) load(pb + PS);
      const int rem = (p_end - pb) * EB;            // valid reduction bytes of this stage (the rest of the rows is zero)
      mma_stage<T>(As, Bs, wm, wn, lane, rem >= kRowB ? 4 : (rem + 63) / 64, acc);
      __syncthreads();
    }
  }
  // D[row = k][col = c]: one split writes its partial tile (or adds into dw when it is the only one) — no atomics, same bits every run
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int c = c0 + wn + 16 * j + (lane & 15);
      if (c >= p.C) continue;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int k = k0 + wm + 16 * i + (lane >> 4) * 4 + e;
        if (k >= p.K) continue;
        const size_t o = (size_t)k * p.C + c;
        if (p.part) p.part[(size_t)split * p.K * p.C + o] = acc[i][j][e];
        else p.dw[o] += acc[i][j][e];
      }
    }
}

// dw[i] += sum over splits s = 0, 1, ... of part[s][i] (fixed order)
__global__ __launch_bounds__(256) void k_conv1x1_wgrad_reduce(const float* __restrict__ part, int splits, size_t n, float* __restrict__ dw) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    float a = 0.f;
    for (int s = 0; s < splits; ++s) a += part[(size_t)s * n + i];
    dw[i] += a;
  }
}

// ------------------------------------------------------------------------------------------------ host
int check_1x1(const vk_conv_desc* d, const char* who) {
  VK_CHECK_ARG(d, "%s: null descriptor", who);
  if (d->R != 1 || d->S != 1 || d->pad != 0 || (d->stride != 1 && d->stride != 2) || d->src1.ptr || d->src0.up) {
    vkh::set_error("%s: only R = S = 1, pad 0, stride 1 or 2, one source without upsampling (got R=%d S=%d pad=%d stride=%d)", who, d->R, d->S,
                   d->pad, d->stride);
    return VK_ERR_UNSUPPORTED;
  }
  VK_CHECK_ARG(d->dtype == VK_F32 || d->dtype == VK_BF16 || d->dtype == VK_F16, "%s: bad dtype", who);
  const int ve = d->dtype == VK_F32 ? 4 : 8;
  VK_CHECK_ARG(d->src0.ptr, "%s: src0.ptr is null", who);
  VK_CHECK_ARG(d->N >= 1 && d->H >= 1 && d->W >= 1 && d->Ho >= 1 && d->Wo >= 1, "%s: empty tensor", who);
  VK_CHECK_ARG(d->src0.C >= ve && d->src0.C % ve == 0 && d->K >= ve && d->K % ve == 0, "%s: channels C=%d K=%d must be multiples of %d", who,
               d->src0.C, d->K, ve);
  VK_CHECK_ARG(!d->src0.scale == !d->src0.shift, "%s: scale and shift go together", who);
  VK_CHECK_ARG((((uintptr_t)d->src0.scale | (uintptr_t)d->src0.shift) & 15) == 0, "%s: scale / shift must be 16-byte aligned", who);
  const int s = d->stride;
  if (!d->transposed)
    VK_CHECK_ARG(d->Ho == (d->H - 1) / s + 1 && d->Wo == (d->W - 1) / s + 1, "%s: output %dx%d does not match input %dx%d at stride %d", who,
                 d->Ho, d->Wo, d->H, d->W, s);
  else
    VK_CHECK_ARG(d->H == (d->Ho - 1) / s + 1 && d->W == (d->Wo - 1) / s + 1, "%s: gradient %dx%d does not match output %dx%d at stride %d", who,
                 d->H, d->W, d->Ho, d->Wo, s);
  VK_CHECK_ARG((size_t)d->N * d->H * d->W < (1ull << 31) && (size_t)d->N * d->Ho * d->Wo < (1ull << 31), "%s: too many pixels", who);
  return VK_OK;
}

}  // namespace

int conv1x1_fwd_impl(const vk_conv_desc* d, const void* w, void* y, int accumulate, double* stats, hipStream_t st) {
  const int rc = check_1x1(d, d && d->transposed ? "vk_conv1x1_fwd (data gradient)" : "vk_conv1x1_fwd");
  if (rc != VK_OK) return rc;
  VK_CHECK_ARG(w && y, "vk_conv1x1_fwd: null argument");
  const int eb = d->dtype == VK_F32 ? 4 : 2;
  Fwd1x1 p;
  p.x = d->src0.ptr; p.scale = d->src0.scale; p.shift = d->src0.shift; p.relu = d->src0.relu;
  p.w = w; p.y = y; p.stats = stats;
  p.Cred = d->src0.C; p.Kout = d->K;
  p.H = d->H; p.W = d->W; p.Ho = d->Ho; p.Wo = d->Wo;
  const int sl = d->stride == 2 ? 1 : 0;
  if (!d->transposed) { p.Hg = d->Ho; p.Wg = d->Wo; p.in_s = sl; p.out_s = 0; }
  else { p.Hg = d->H; p.Wg = d->W; p.in_s = 0; p.out_s = sl; }
  p.M = d->N * p.Hg * p.Wg;
  p.accumulate = accumulate;
  dim3 grid((unsigned)((p.M + kTile - 1) / kTile), (unsigned)((p.Kout + kTile - 1) / kTile));
  const double flops = 2.0 * p.M * (double)p.Cred * p.Kout;
  const double bytes = ((double)p.M * p.Cred + (double)p.M * p.Kout * (accumulate ? 2.0 : 1.0) + (double)p.Kout * p.Cred) * eb +
                       (d->transposed && sl && !accumulate ? 3.0 * p.M * p.Kout * eb : 0.0);
  static const char* const tags[2][2] = {{"conv1x1_fwd_f32", "conv1x1_fwd_16b"}, {"conv1x1_dgrad_f32", "conv1x1_dgrad_16b"}};
  const char* const tag = tags[d->transposed ? 1 : 0][eb == 2 ? 1 : 0];
  return dispatch_dtype(d->dtype, [&](auto e) { return vkh::launch<k_conv1x1_fwd<decltype(e)>>(grid, dim3(256), 0, st, tag, {}, flops, bytes, p); });
}

int conv1x1_wgrad_impl(const vk_conv_desc* d, const void* dz, float* dw, void* workspace, size_t workspace_bytes, hipStream_t st) {
  const int rc = check_1x1(d, "vk_conv1x1_wgrad");
  if (rc != VK_OK) return rc;
  VK_CHECK_ARG(dz && dw && !d->transposed, "vk_conv1x1_wgrad: null argument or transposed descriptor");
  const int eb = d->dtype == VK_F32 ? 4 : 2;
  Wg1x1 p;
  p.dz = dz; p.x = d->src0.ptr; p.scale = d->src0.scale; p.shift = d->src0.shift; p.relu = d->src0.relu;
  p.dw = dw; p.part = nullptr;
  p.K = d->K; p.C = d->src0.C; p.P = d->N * d->Ho * d->Wo;
  p.Ho = d->Ho; p.Wo = d->Wo; p.H = d->H; p.W = d->W; p.s = d->stride == 2 ? 1 : 0;
  const int PS = kRowB / eb;
  const int tiles = ((p.K + kTile - 1) / kTile) * ((p.C + kTile - 1) / kTile);
  // split the pixels so that the grid fills the chip about twice; at least 4 stages per split, bounded by the workspace
  const size_t tile_bytes = (size_t)p.K * p.C * sizeof(float);
  int splits = (512 + tiles - 1) / tiles;
  splits = std::min(splits, std::max(1, (p.P + 4 * PS - 1) / (4 * PS)));
  const size_t fit = workspace ? workspace_bytes / tile_bytes : 0;
  splits = (int)std::min<size_t>((size_t)splits, fit);
  if (splits < 2) splits = 1;
  int stages = (p.P + PS - 1) / PS;
  const int per = (stages + splits - 1) / splits;
  splits = (stages + per - 1) / per;                    // no empty split
  p.px_per_split = per * PS;
  if (splits > 1) {
    VK_CHECK_ARG(((uintptr_t)workspace & 15) == 0, "vk_conv1x1_wgrad: workspace must be 16-byte aligned");
    p.part = (float*)workspace;
  }
  const double flops = 2.0 * p.P * (double)p.K * p.C;
  const double bytes = ((double)p.P * p.K + (double)d->N * d->H * d->W * p.C / (p.s ? 4.0 : 1.0)) * eb +
                       (double)tile_bytes * (splits > 1 ? 2.0 * splits + 2.0 : 2.0);
  const char* const tag = eb == 2 ? "conv1x1_wgrad_16b" : "conv1x1_wgrad_f32";
  dim3 grid((unsigned)tiles, (unsigned)splits);
  {
    const int rc = dispatch_dtype(d->dtype, [&](auto e) { return vkh::launch<k_conv1x1_wgrad<decltype(e)>>(grid, dim3(256), 0, st, tag, {}, flops, bytes, p); });
    if (rc != VK_OK) return rc;
  }
  if (splits > 1) {
    const size_t n = (size_t)p.K * p.C;
    const unsigned blocks = (unsigned)std::min<size_t>((n + 255) / 256, 1024);
    hipLaunchKernelGGL(k_conv1x1_wgrad_reduce, dim3(blocks), dim3(256), 0, st, (const float*)p.part, splits, n, dw);
    VK_CHECK_HIP(hipGetLastError());
  }
  return VK_OK;
}

}  // namespace vk

extern "C" int vk_conv1x1_fwd(const vk_conv_desc* d, const void* w, void* y, int accumulate, double* stats, void* stream) {
  return vk::conv1x1_fwd_impl(d, w, y, accumulate, stats, (hipStream_t)stream);
}

extern "C" int vk_conv1x1_wgrad(const vk_conv_desc* d, const void* dz, float* dw, void* workspace, size_t workspace_bytes, void* stream) {
  return vk::conv1x1_wgrad_impl(d, dz, dw, workspace, workspace_bytes, (hipStream_t)stream);
}
