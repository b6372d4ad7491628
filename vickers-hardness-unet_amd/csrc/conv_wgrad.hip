// Weight gradient of the convolutions (replaces ATen conv backward-weight behind loss.backward(),
// reference train.py:443/:448):
//
//   dW[k][tap][c] += sum_{pixels m in this split}  dz[m][k] * V[m @ tap][c]
//
// A GEMM whose reduction runs over pixels.  Both operands are pixel-major in HBM (NHWC), i.e.
// "K-strided" for the MFMA; they are staged as they lie ([pixel][channel], 16-byte vectors, BN+ReLU /
// upsample / concat applied to V on the way) and the transposition happens in the LDS read:
//   16-bit : ds_read_b64_tr_b16 (4 pixels x 16 channels per 16-lane group, two reads per fragment)
//   fp32   : ds_read_b32, lane = (channel, pixel-in-group) — already the 16x16x4 operand layout.
// Split-K over pixel ranges (grid.z): every split stores its partial tile into a slab of the caller's workspace and
// k_wgrad_slab_reduce (wgrad_halo.hip) adds the splits in a fixed order -> bit-reproducible gradients (fp32 atomics into
// the flat gradient buffer only when no workspace is given).
// Two wave layouts: big tiles split the output tile over the 4 waves; small-channel layers
// (K or C <= 32: decoder blocks 3/4, stem) give every wave the whole tile on its own 32-pixel slice.
#include <stdlib.h>

#include <string>

#include "conv_host.h"

namespace vk {

struct WgradParams {
  Src s0, s1;
  const void* dz;
  uint32_t dz_bytes;
  float* dw;
  float* slab;            // [splits][K * RS * C] partial results (nullptr: fp32 atomics into dw)
  int N, H, W, Ho, Wo, K, R, S, slog, pad;
  int C, M, RS, mps, ctiles, stem, cin;      // stem: the x4 layout; cin = its real channels (1..4), dW is [64][7][7][cin]
  FastDiv div_hw, div_w, div_ct, div_s;
};

template <typename T, int BMW, int BNW, bool WSPLIT>
struct WgradCfg {
  using Tr = ElemTraits<T>;
  static constexpr int VE = Tr::kVec;
  static constexpr int EB = Tr::kBytes;
  static constexpr int PX = WSPLIT ? 128 : 32;                 // pixels per chunk
  static constexpr int ZV = BMW / VE, VV = BNW / VE;            // vectors per pixel row
  static constexpr int ZPASS = (PX * ZV + 255) / 256, VPASS = (PX * VV + 255) / 256;
  // row pads chosen so that the transposed / b32 fragment reads are bank-conflict free
  static constexpr int zpad(int ch) { return EB == 2 ? (((ch * 2 / 32) % 2 == 0) ? 32 : 0) : ((ch % 32 == 0) ? 64 : 0); }
  static constexpr int ZSB = BMW * EB + zpad(BMW);
  static constexpr int VSB = BNW * EB + zpad(BNW);
  static constexpr int STAGE = PX * (ZSB + VSB);
  static constexpr int WGK = WSPLIT ? 1 : 2, WGC = WSPLIT ? 1 : 2;
  static constexpr int WK = BMW / WGK, WC = BNW / WGC;
  static constexpr int TK = WK / 16, TCc = WC / 16;
  static constexpr int SMEM = 2 * STAGE;
  static_assert(TK >= 1 && TCc >= 1, "tile too small");
};

template <typename T, int BMW, int BNW, bool WSPLIT>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(const WgradParams p) {
  using Cfg = WgradCfg<T, BMW, BNW, WSPLIT>;
  constexpr int VE = Cfg::VE, EB = Cfg::EB, PX = Cfg::PX, ZV = Cfg::ZV, VV = Cfg::VV;
  constexpr int ZPASS = Cfg::ZPASS, VPASS = Cfg::VPASS, ZSB = Cfg::ZSB, VSB = Cfg::VSB, STAGE = Cfg::STAGE;
  constexpr int TK = Cfg::TK, TCc = Cfg::TCc;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int k0 = blockIdx.x * BMW;
  const int tap = (int)fdiv(blockIdx.y, p.div_ct);
  const int ct = blockIdx.y - tap * p.ctiles;
  const int c0 = ct * BNW;                       // channel in concat space
  const int r = (int)fdiv((uint32_t)tap, p.div_s), s = tap - r * p.S;
  const int mbeg = blockIdx.z * p.mps;
  const int mend = min(p.M, mbeg + p.mps);
  const int nch = (mend - mbeg + PX - 1) / PX;
  if (nch <= 0) return;

  const bool first = c0 < p.s0.C;
  const Src& sd = first ? p.s0 : p.s1;
  const int cl0 = first ? c0 : c0 - p.s0.C;
  const __amdgpu_buffer_rsrc_t rsv = make_rsrc(sd.ptr, sd.bytes);
  const __amdgpu_buffer_rsrc_t rsz = make_rsrc(p.dz, p.dz_bytes);
  const int up = sd.up;
  const int Hs = p.H >> up, Ws = p.W >> up;
  const int HoWo = p.Ho * p.Wo;
  const bool affine = sd.scale != nullptr;
  const bool relu = sd.relu != 0;

  // V-vector channel of this thread is fixed for the whole kernel -> scale/shift loaded once
  float sc[VPASS][VE], sh[VPASS][VE];
#pragma unroll
  for (int i = 0; i < VPASS; ++i) {
    const int v = tid + i * 256;
    const int vec = v % VV;
#pragma unroll
    for (int j = 0; j < VE; ++j) { sc[i][j] = 1.f; sh[i][j] = 0.f; }
    if (affine && v < PX * VV) {
#pragma unroll
      for (int j = 0; j < VE; ++j) {
        sc[i][j] = sd.scale[cl0 + vec * VE + j];
        sh[i][j] = sd.shift[cl0 + vec * VE + j];
      }
    }
  }

  u32x4_t zreg[ZPASS], vreg[VPASS];
  uint32_t vmask = 0;

  auto load_chunk = [&](int ch) {
    const int mb = mbeg + ch * PX;
#pragma unroll
    for (int i = 0; i < ZPASS; ++i) {
      const int v = tid + i * 256;
      const int px = v / ZV, vec = v % ZV;
      const int m = mb + px;
      const bool ok = (v < PX * ZV) && (m < mend) && (k0 + vec * VE < p.K);
      const uint32_t off = (uint32_t)(m * p.K + k0 + vec * VE) * (uint32_t)EB;
      zreg[i] = buf_load16(rsz, ok ? off : kOOB);
    }
    vmask = 0;
#pragma unroll
    for (int i = 0; i < VPASS; ++i) {
      const int v = tid + i * 256;
      const int px = v / VV, vec = v % VV;
      const int m = mb + px;
      bool ok = (v < PX * VV) && (m < mend);
      const int n = (int)fdiv((uint32_t)m, p.div_hw);
      const int rem = m - n * HoWo;
      const int pp = (int)fdiv((uint32_t)rem, p.div_w);
      const int q = rem - pp * p.Wo;
      uint32_t off;
      if (!p.stem) {
        const int h = (pp << p.slog) - p.pad + r;
        const int w = (q << p.slog) - p.pad + s;
        ok = ok && (unsigned)h < (unsigned)p.H && (unsigned)w < (unsigned)p.W;
        off = (uint32_t)(((n * Hs + (h >> up)) * Ws + (w >> up)) * sd.C + cl0 + vec * VE) * (uint32_t)EB;
        vreg[i] = buf_load16(rsv, ok ? off : kOOB);
      } else {
        // stem: "tap" = filter row, "channels" = 8 pixels x 4 channels along W
        constexpr int PPV = VE / 4;
        const int h = 2 * pp - 3 + tap;
        const int wb = 2 * q - 3 + vec * PPV;
        const bool okh = ok && (unsigned)h < (unsigned)p.H;
        const uint32_t rowoff = (uint32_t)((n * p.H + h) * p.W) * 4u * (uint32_t)EB;
        if (PPV == 1) {
          const bool o0 = okh && (unsigned)wb < (unsigned)p.W;
          vreg[i] = buf_load16(rsv, o0 ? rowoff + (uint32_t)wb * 4u * EB : kOOB);
        } else {
          const bool o0 = okh && (unsigned)wb < (unsigned)p.W;
          const bool o1 = okh && (unsigned)(wb + 1) < (unsigned)p.W;
          const u32x2_t lo = __builtin_amdgcn_raw_buffer_load_b64(rsv, o0 ? rowoff + (uint32_t)wb * 4u * EB : kOOB, 0, 0);
          const u32x2_t hi = __builtin_amdgcn_raw_buffer_load_b64(rsv, o1 ? rowoff + (uint32_t)(wb + 1) * 4u * EB : kOOB, 0, 0);
          vreg[i] = u32x4_t{lo[0], lo[1], hi[0], hi[1]};
        }
      }
      vmask |= (ok ? 1u : 0u) << i;
    }
  };

  auto store_chunk = [&](int stage) {
    char* Zs = smem + stage * STAGE;
    char* Vs = Zs + PX * ZSB;
#pragma unroll
    for (int i = 0; i < ZPASS; ++i) {
      const int v = tid + i * 256;
      if (v < PX * ZV) *reinterpret_cast<u32x4_t*>(Zs + (v / ZV) * ZSB + (v % ZV) * 16) = zreg[i];
    }
#pragma unroll
    for (int i = 0; i < VPASS; ++i) {
      const int v = tid + i * 256;
      u32x4_t x = vreg[i];
      if (affine) {
        float f[VE];
        Vec16<T>::unpack(x, f);
#pragma unroll
        for (int j = 0; j < VE; ++j) {
          f[j] = fmaf(f[j], sc[i][j], sh[i][j]);
          if (relu) f[j] = fmaxf(f[j], 0.f);
        }
        x = Vec16<T>::pack(f);
        if (!((vmask >> i) & 1u)) x = u32x4_t{0, 0, 0, 0};
      }
      if (v < PX * VV) *reinterpret_cast<u32x4_t*>(Vs + (v / VV) * VSB + (v % VV) * 16) = x;
    }
  };

  const int wk0 = WSPLIT ? 0 : (wave >> 1) * Cfg::WK;
  const int wc0 = WSPLIT ? 0 : (wave & 1) * Cfg::WC;
  const int wpx = WSPLIT ? wave * 32 : 0;        // this wave's pixel slice inside the chunk
  f32x4_t acc[TK][TCc];
#pragma unroll
  for (int a = 0; a < TK; ++a)
#pragma unroll
    for (int b = 0; b < TCc; ++b) acc[a][b] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  auto compute = [&](int stage) {
    const char* Zs = smem + stage * STAGE + wpx * ZSB;
    const char* Vs = smem + stage * STAGE + PX * ZSB + wpx * VSB;
    if (EB == 2) {
      // lane j of 16-lane group g supplies row (pixel) 4g + (j>>2) [+16 for the second read], columns 4*(j&3)..+3
      const int g = lane >> 4, j = lane & 15;
      const int prow = 4 * g + (j >> 2);
      const int cofs = 4 * (j & 3) * 2;
      u32x4_t zf[TK], vf[TCc];
      typedef __attribute__((address_space(3))) s16x4_t* lds_s16x4_ptr;
#pragma unroll
      for (int a = 0; a < TK; ++a) {
        const char* b0 = Zs + prow * ZSB + (wk0 + a * 16) * 2 + cofs;
        const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(b0));
        const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(b0 + 16 * ZSB));
        const u32x2_t l2 = __builtin_bit_cast(u32x2_t, lo), h2 = __builtin_bit_cast(u32x2_t, hi);
        zf[a] = u32x4_t{l2[0], l2[1], h2[0], h2[1]};
      }
#pragma unroll
      for (int b = 0; b < TCc; ++b) {
        const char* b0 = Vs + prow * VSB + (wc0 + b * 16) * 2 + cofs;
        const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(b0));
        const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(b0 + 16 * VSB));
        const u32x2_t l2 = __builtin_bit_cast(u32x2_t, lo), h2 = __builtin_bit_cast(u32x2_t, hi);
        vf[b] = u32x4_t{l2[0], l2[1], h2[0], h2[1]};
      }
#pragma unroll
      for (int a = 0; a < TK; ++a)
#pragma unroll
        for (int b = 0; b < TCc; ++b) acc[a][b] = Mma<T>::run(zf[a], vf[b], acc[a][b]);
    } else {
      const int i = lane & 15, kg = lane >> 4;
#pragma unroll
      for (int st = 0; st < 8; ++st) {
        float zf[TK], vf[TCc];
#pragma unroll
        for (int a = 0; a < TK; ++a)
          zf[a] = *reinterpret_cast<const float*>(Zs + (4 * st + kg) * ZSB + (wk0 + a * 16 + i) * 4);
#pragma unroll
        for (int b = 0; b < TCc; ++b)
          vf[b] = *reinterpret_cast<const float*>(Vs + (4 * st + kg) * VSB + (wc0 + b * 16 + i) * 4);
#pragma unroll
        for (int a = 0; a < TK; ++a)
#pragma unroll
          for (int b = 0; b < TCc; ++b)
            acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(zf[a], vf[b], acc[a][b], 0, 0, 0);
      }
    }
  };

  load_chunk(0);
  store_chunk(0);
  __syncthreads();
  for (int ch = 0; ch < nch; ++ch) {
    const bool more = ch + 1 < nch;
    if (more) load_chunk(ch + 1);
    compute(ch & 1);
    if (more) store_chunk((ch + 1) & 1);
    __syncthreads();
  }

  // ---- epilogue: dW[k][tap][c] (stem: [k][r][s][cin], padding columns dropped): this split's slab, or fp32 atomics ----
  // (WSPLIT layouts give every wave the whole tile on its own pixel slice: their four partial tiles are added through LDS first)
  float* const out = p.slab ? p.slab + (size_t)blockIdx.z * ((size_t)p.K * (p.stem ? 49 * p.cin : p.RS * p.C)) : p.dw;
  if (WSPLIT && p.slab) {
    float* red = reinterpret_cast<float*>(smem);           // [wave][TK][TCc][64 lanes][4]: at most 4 * 4 * 4 * 256 * 4 B = 64 KB <= 2 * STAGE
    static_assert(4 * TK * TCc * 1024 <= Cfg::SMEM || !WSPLIT, "wave-partial tiles must fit the staging buffers");
#pragma unroll
    for (int a = 0; a < TK; ++a)
#pragma unroll
      for (int b = 0; b < TCc; ++b) *reinterpret_cast<f32x4_t*>(red + (((wave * TK + a) * TCc + b) * 64 + lane) * 4) = acc[a][b];
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int a = 0; a < TK; ++a)
#pragma unroll
        for (int b = 0; b < TCc; ++b) {
          f32x4_t t = acc[a][b];
#pragma unroll
          for (int w = 1; w < 4; ++w) t = t + *reinterpret_cast<const f32x4_t*>(red + (((w * TK + a) * TCc + b) * 64 + lane) * 4);
          acc[a][b] = t;
        }
    } else {
      return;
    }
  }
#pragma unroll
  for (int a = 0; a < TK; ++a)
#pragma unroll
    for (int b = 0; b < TCc; ++b) {
      const int cc = c0 + wc0 + b * 16 + (lane & 15);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int k = k0 + wk0 + a * 16 + (lane >> 4) * 4 + e;
        if (k >= p.K) continue;
        float* dst = nullptr;
        if (!p.stem) {
          if (cc < p.C) dst = out + ((size_t)k * p.RS + tap) * p.C + cc;
        } else {
          const int sx = cc >> 2, ci = cc & 3;
          if (sx < 7 && ci < p.cin) dst = out + (((size_t)k * 7 + tap) * 7 + sx) * p.cin + ci;
        }
        if (!dst) continue;
        if (p.slab) *dst = acc[a][b][e];
        else atomicAdd(dst, acc[a][b][e]);
      }
    }
}

int launch_slab_reduce(size_t n4, int splits, const float* slab, float* dw, hipStream_t st);     // wgrad_halo.hip

// ------------------------------------------------------------------------------------------------ host
template <typename T, int BMW, int BNW, bool WSPLIT>
static int launch_w(WgradParams p, void* workspace, size_t workspace_bytes, hipStream_t st) {
  using Cfg = WgradCfg<T, BMW, BNW, WSPLIT>;
  p.ctiles = (p.C + BNW - 1) / BNW;
  p.div_ct = vkh::make_fastdiv((uint32_t)p.ctiles);
  const int ktiles = (p.K + BMW - 1) / BMW;
  const int out_tiles = ktiles * p.ctiles * p.RS;
  // split the pixel reduction so that ~4 workgroups per CU exist, each with at least 8 chunks
  int chunks = (p.M + Cfg::PX - 1) / Cfg::PX;
  int splits = (1024 + out_tiles - 1) / out_tiles;
  if (splits > chunks / 8) splits = chunks / 8;
  if (splits < 1) splits = 1;
  // reproducible mode: the splits' partial results go to a slab in the workspace ([splits][K * RS * C] floats) and are added in split order
  const size_t out_elems = (size_t)p.K * (p.stem ? (size_t)49 * p.cin : (size_t)p.RS * p.C);
  const bool use_slab = workspace && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0 && out_elems % 4 == 0 && workspace_bytes >= out_elems * 4 &&
                        (reinterpret_cast<uintptr_t>(p.dw) & 15) == 0 && !getenv("VK_WGRAD_ATOMICS");
  if (use_slab) {
    const size_t cap = workspace_bytes / (out_elems * 4);
    if ((size_t)splits > cap) splits = (int)cap;
  }
  int cps = (chunks + splits - 1) / splits;
  p.mps = cps * Cfg::PX;
  splits = (p.M + p.mps - 1) / p.mps;
  p.slab = use_slab ? (float*)workspace : nullptr;
  dim3 grid(ktiles, p.ctiles * p.RS, splits);
  static const std::string tag_c = std::string("wgrad_") + (sizeof(T) == 4 ? "f32" : "16b") + "_" + std::to_string(BMW) + "x" + std::to_string(BNW);
  static const std::string tag_s = std::string("wgrad_stem_") + (sizeof(T) == 4 ? "f32" : "16b");
  const double rsc = p.stem ? 49.0 * p.cin : (double)p.RS * p.C;
  const double eb = sizeof(T);
  const double bytes = ((double)p.N * p.H * p.W * (p.stem ? p.cin : p.C) + (double)p.M * p.K) * eb + (double)p.K * rsc * 4.0;
  const int rc = vkh::launch<conv_wgrad_kernel<T, BMW, BNW, WSPLIT>>(grid, dim3(256), Cfg::SMEM, st, (p.stem ? tag_s : tag_c).c_str(),
                                                                     {":H%d_K%d_C%d_R%d_s%d", {p.H, p.K, p.C, p.R, splits}}, 2.0 * (double)p.M * p.K * rsc, bytes, p);
  if (rc != VK_OK || !use_slab) return rc;
  return launch_slab_reduce(out_elems / 4, splits, p.slab, p.dw, st);
}

template <typename T>
static int launch_w_shape(const WgradParams& p, int cmin, void* ws, size_t wsb, hipStream_t st) {
  // cmin = smallest per-source channel count (a c-tile must not straddle the concat boundary)
  if (p.K >= 128 && cmin % 128 == 0) return launch_w<T, 128, 128, false>(p, ws, wsb, st);
  if (p.K >= 64 && cmin % 64 == 0) return launch_w<T, 64, 64, false>(p, ws, wsb, st);
  if (p.K >= 64 && cmin % 32 == 0) return launch_w<T, 64, 32, true>(p, ws, wsb, st);
  if (p.K >= 32 && cmin % 64 == 0) return launch_w<T, 32, 64, true>(p, ws, wsb, st);
  if (p.K >= 32 && cmin % 32 == 0) return launch_w<T, 32, 32, true>(p, ws, wsb, st);
  if (cmin % 32 == 0) return launch_w<T, 16, 32, true>(p, ws, wsb, st);
  return launch_w<T, 16, 16, true>(p, ws, wsb, st);
}

static int dispatch_w(vk_dtype dt, const WgradParams& p, int cmin, void* ws, size_t wsb, hipStream_t st) {
  return dispatch_dtype(dt, [&](auto e) { return launch_w_shape<decltype(e)>(p, cmin, ws, wsb, st); }, true);
}

int wgrad_halo_try(const vk_conv_desc* d, const void* dz, float* dw, void* workspace, size_t workspace_bytes, hipStream_t st);

int conv_wgrad_impl(const vk_conv_desc* d, const void* dz, float* dw, void* workspace, size_t workspace_bytes, hipStream_t st) {
  VK_CHECK_ARG(d && dz && dw && d->src0.ptr, "vk_conv_wgrad: null argument");
  VK_CHECK_ARG(!d->transposed, "vk_conv_wgrad: descriptor must describe the forward convolution");
  {
    const int rc = wgrad_halo_try(d, dz, dw, workspace, workspace_bytes, st);      // 3x3 stride-1 layers with enough pixels per output tile
    if (rc != VK_ERR_UNSUPPORTED) return rc;
  }
  const int eb = d->dtype == VK_F32 ? 4 : 2;
  const int C = d->src0.C + (d->src1.ptr ? d->src1.C : 0);
  VK_CHECK_ARG(d->K % 16 == 0 && C % 16 == 0, "vk_conv_wgrad: K=%d, C=%d must be multiples of 16", d->K, C);
  VK_CHECK_ARG(d->stride == 1 || d->stride == 2, "vk_conv_wgrad: stride %d unsupported", d->stride);
  const size_t in_bytes = (size_t)d->N * d->H * d->W * C * eb, dz_bytes = (size_t)d->N * d->Ho * d->Wo * d->K * eb;
  VK_CHECK_ARG(in_bytes < (1ull << 31) && dz_bytes < (1ull << 31), "vk_conv_wgrad: tensor too large for 32-bit offsets");
  WgradParams p;
  p.s0 = make_src(d->src0, d->N, d->H, d->W, eb);
  p.s1 = make_src1(d, eb);
  p.dz = dz;
  p.dz_bytes = (uint32_t)dz_bytes;
  p.dw = dw;
  p.slab = nullptr;
  p.N = d->N; p.H = d->H; p.W = d->W; p.Ho = d->Ho; p.Wo = d->Wo; p.K = d->K; p.R = d->R; p.S = d->S;
  p.slog = d->stride == 2 ? 1 : 0;
  p.pad = d->pad;
  p.C = C;
  p.M = d->N * d->Ho * d->Wo;
  p.RS = d->R * d->S;
  p.stem = 0; p.cin = 0;
  p.div_hw = vkh::make_fastdiv((uint32_t)(d->Ho * d->Wo));
  p.div_w = vkh::make_fastdiv((uint32_t)d->Wo);
  p.div_s = vkh::make_fastdiv((uint32_t)d->S);
  int cmin = d->src0.C;
  if (d->src1.ptr && d->src1.C < cmin) cmin = d->src1.C;
  if (d->src1.ptr) {
    // tiles must not straddle the concat boundary: use the gcd-like granularity of both sources
    int g = 128;
    while (g > 16 && (d->src0.C % g || d->src1.C % g)) g >>= 1;
    cmin = g;
  }
  return dispatch_w(d->dtype, p, cmin, workspace, workspace_bytes, st);
}

// ---- stem (7x7 stride 2, cin->64, 1 <= cin <= 4) weight gradient for the 16-bit types: one workgroup stages a 4 x 32 output-pixel tile of dz
// and the 13 x 72 input pixels under it ONCE and accumulates all seven filter rows from them (the tap-by-tap kernel above
// streams dz once per filter row: 7 passes over the 268 MB tensor).
//   dW[k][r][s][c] = sum_px dz[px][k] * x4[2y + r - 3][2x + s - 3][c]
// GEMM view per filter row r: A = dz^T (k x pixels), B[px][v] with v = (s, c) = the 64 contiguous bytes starting at input pixel
// (2y + r - 3, 2x - 3): overlapping windows of the staged rows, read by ds_read_b64_tr_b16 with per-lane addresses.
// Wave w owns output channels 16w..16w+15 and all 7 x 2 (s-half) tiles: 56 accumulator registers.  Persistent workgroups,
// double-buffered LDS, next tile's loads in flight (registers) under the MFMAs.  fp32 atomics at the end (as above).
struct StemWgParams {
  const void* x4;
  const void* dz;
  const void* z;          // BNA form: dz is the masked upstream gradient g, the operand is a*g + b*z + c (BatchNorm backward apply, folded in)
  const float* coef;      // [3][64]: a, b, c
  float* dw;
  float* slab;            // [gridDim.x][64 * 49 * cin] per-workgroup partial results (nullptr: fp32 atomics into dw)
  uint32_t x_bytes, dz_bytes;
  int N, H, W, Ho, Wo, tiles_x, tiles_y, ntiles;
  int cin;                // channels of x4 that are data: dW is KRSC [64][7][7][cin], the columns ci >= cin are dropped
};

// BNA (r04): the stem's BatchNorm-backward apply pass exists only to feed this kernel (the stem has no data gradient): instead of
// reading g and z (2 x 268 MB at bs 32), writing dz and reading it again here, the kernel reads g and z itself and forms
// dz = a*g + b*z + c (same fp32 expression and rounding as k_bn_bwd_apply) while staging — the 805 MB pass and its launch go
template <typename T, bool BNA>
__global__ __launch_bounds__(256) void k_stem_wgrad(const StemWgParams p) {
  static_assert(sizeof(T) == 2, "16-bit types only");
  constexpr int ZSB = 160;                   // dz pixel row: 64 k x 2 B + 32 pad (conflict-free transposed reads)
  constexpr int XW = 72, XROWS = 13;         // staged input: 13 rows x 72 pixels x 8 B
  constexpr int Z_BYTES = 128 * ZSB, X_BYTES = XROWS * XW * 8;
  constexpr int STAGE = (Z_BYTES + X_BYTES + 255) / 256 * 256;
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];
  typedef __attribute__((address_space(3))) s16x4_t* lds_s16x4_ptr;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const __amdgpu_buffer_rsrc_t rsx = make_rsrc(p.x4, p.x_bytes);
  const __amdgpu_buffer_rsrc_t rsz = make_rsrc(p.dz, p.dz_bytes);

  u32x4_t zr[4], zr_n[4];
  u32x4_t qr[BNA ? 4 : 1], qr_n[BNA ? 4 : 1];       // BNA: the z vectors beside the g vectors
  uint32_t okm = 0, okm_n = 0;                       // BNA: which of the four vectors lie inside the image (c must not leak into the padding)
  u32x2_t xr[4], xr_n[4];
  const __amdgpu_buffer_rsrc_t rsq = make_rsrc(BNA ? p.z : p.dz, p.dz_bytes);
  float ca[8], cb[8], cc[8];                         // this thread's 8 channels: vec = tid & 7 in every vector it stages
  if (BNA) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      ca[j] = p.coef[(tid & 7) * 8 + j];
      cb[j] = p.coef[64 + (tid & 7) * 8 + j];
      cc[j] = p.coef[128 + (tid & 7) * 8 + j];
    }
  }
  auto fetch = [&](int t, u32x4_t (&zv)[4], u32x4_t (&qv)[BNA ? 4 : 1], uint32_t& okv, u32x2_t (&xv)[4]) {
    int bt = t;
    const int tx = bt % p.tiles_x;
    bt /= p.tiles_x;
    const int ty = bt % p.tiles_y;
    const int n = bt / p.tiles_y;
    const int y0 = ty * 4, x0 = tx * 32;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int idx = tid + i * 256;
      const int px = idx >> 3, vec = idx & 7;
      const int y = y0 + (px >> 5), x = x0 + (px & 31);
      const bool ok = y < p.Ho && x < p.Wo;
      const uint32_t off = ok ? (uint32_t)(((n * p.Ho + y) * p.Wo + x) * 64 + vec * 8) * 2u : kOOB;
      zv[i] = buf_load16(rsz, off);
      if (BNA) {
        qv[i] = buf_load16(rsq, off);
        if (i == 0) okv = 0;
        okv |= (ok ? 1u : 0u) << i;
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int idx = tid + i * 256;
      const int ry = idx / XW, rx = idx - ry * XW;
      const int iy = 2 * y0 - 3 + ry, ix = 2 * x0 - 3 + rx;
      const bool ok = idx < XROWS * XW && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
      xv[i] = __builtin_amdgcn_raw_buffer_load_b64(rsx, ok ? (uint32_t)(((n * p.H + iy) * p.W + ix) * 4) * 2u : kOOB, 0, 0);
    }
  };
  auto stage = [&](int st, const u32x4_t (&zv)[4], const u32x4_t (&qv)[BNA ? 4 : 1], uint32_t okv, const u32x2_t (&xv)[4]) {
    char* Zs = smem + st * STAGE;
    char* Xs = Zs + Z_BYTES;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int idx = tid + i * 256;
      u32x4_t v = zv[i];
      if (BNA) {
        float g[8], zf[8], o[8];
        Vec16<T>::unpack(zv[i], g);
        Vec16<T>::unpack(qv[i], zf);
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = fmaf(ca[j], g[j], fmaf(cb[j], zf[j], cc[j]));
        v = Vec16<T>::pack(o);
        if (!((okv >> i) & 1u)) v = u32x4_t{0, 0, 0, 0};
      }
      *reinterpret_cast<u32x4_t*>(Zs + (idx >> 3) * ZSB + (idx & 7) * 16) = v;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int idx = tid + i * 256;
      if (idx < XROWS * XW) *reinterpret_cast<u32x2_t*>(Xs + idx * 8) = xv[i];
    }
  };

  f32x4_t acc[7][2];
#pragma unroll
  for (int r = 0; r < 7; ++r)
#pragma unroll
    for (int h = 0; h < 2; ++h) acc[r][h] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  // transposed-read lane geometry: lane j of 16-lane group g supplies pixel 4g + (j >> 2), elements 4 (j & 3) .. +3
  const int pl = 4 * (lane >> 4) + ((lane & 15) >> 2), q = lane & 3;
  const int lane_z = pl * ZSB + (wave * 16 + 4 * q) * 2;
  const int lane_x = (2 * pl + q) * 8;

  int t = blockIdx.x;
  if (t < p.ntiles) {
    fetch(t, zr, qr, okm, xr);
    stage(0, zr, qr, okm, xr);
  }
  __syncthreads();
  for (int it = 0; t < p.ntiles; t += gridDim.x, ++it) {
    const bool has_next = t + (int)gridDim.x < p.ntiles;
    if (has_next) fetch(t + gridDim.x, zr_n, qr_n, okm_n, xr_n);
    const char* Zs = smem + (it & 1) * STAGE;
    const char* Xs = Zs + Z_BYTES;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {                       // one output row = 32 pixels of reduction
      const char* zb = Zs + lane_z + (32 * ks) * ZSB;
      const u32x2_t zl = __builtin_bit_cast(u32x2_t, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(zb)));
      const u32x2_t zh = __builtin_bit_cast(u32x2_t, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(zb + 16 * ZSB)));
      const u32x4_t zf = u32x4_t{zl[0], zl[1], zh[0], zh[1]};
#pragma unroll
      for (int r = 0; r < 7; ++r)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const char* xb = Xs + lane_x + ((2 * ks + r) * XW + 4 * h) * 8;
          const u32x2_t xl = __builtin_bit_cast(u32x2_t, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(xb)));
          const u32x2_t xh = __builtin_bit_cast(u32x2_t, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(xb + 32 * 8)));
          acc[r][h] = Mma<T>::run(zf, u32x4_t{xl[0], xl[1], xh[0], xh[1]}, acc[r][h]);
        }
    }
    if (has_next) {
      stage((it + 1) & 1, zr_n, qr_n, okm_n, xr_n);        // that buffer was last read one iteration ago, before the barrier below
#pragma unroll
      for (int i = 0; i < 4; ++i) { zr[i] = zr_n[i]; xr[i] = xr_n[i]; }
    }
    __syncthreads();
  }
  // D[row = (lane >> 4) * 4 + e -> k][col = lane & 15 -> (s - 4h, c)]
#pragma unroll
  for (int r = 0; r < 7; ++r)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int sx = 4 * h + ((lane & 15) >> 2), ci = lane & 3;
      if (sx < 7 && ci < p.cin) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int k = wave * 16 + (lane >> 4) * 4 + e;
          const size_t off = (((size_t)k * 7 + r) * 7 + sx) * p.cin + ci;
          if (p.slab) p.slab[(size_t)blockIdx.x * (64 * 49 * p.cin) + off] = acc[r][h][e];       // every workgroup writes all 3,136 cin elements
          else atomicAdd(p.dw + off, acc[r][h][e]);
        }
      }
    }
}

int stem_wgrad_impl(vk_dtype dt, int N, int H, int W, int cin, const void* x4, const void* dz, float* dw, void* workspace, size_t workspace_bytes,
                    hipStream_t st, const void* bn_z = nullptr, const float* bn_coef = nullptr) {
  VK_CHECK_ARG(x4 && dz && dw, "vk_stem_wgrad: null argument");
  VK_CHECK_ARG(cin >= 1 && cin <= 4, "vk_stem_wgrad_c: cin=%d is outside 1..4", cin);
  const int eb = dt == VK_F32 ? 4 : 2;
  const bool tile = dt != VK_F32 && !getenv("VK_STEM_WGRAD_TAPS") && (size_t)N * (H / 2) * (W / 2) * 64 * 2 < (1ull << 31);
  if (bn_z && !tile) return VK_ERR_UNSUPPORTED;        // the folded BatchNorm apply lives in the 16-bit tile kernel only
  if (tile) {
    StemWgParams q;
    q.x4 = x4; q.dz = dz; q.dw = dw; q.z = bn_z; q.coef = bn_coef;
    q.N = N; q.H = H; q.W = W; q.Ho = H / 2; q.Wo = W / 2; q.cin = cin;
    q.x_bytes = (uint32_t)((size_t)N * H * W * 4 * 2);
    q.dz_bytes = (uint32_t)((size_t)N * q.Ho * q.Wo * 64 * 2);
    q.tiles_x = (q.Wo + 31) / 32; q.tiles_y = (q.Ho + 3) / 4;
    q.ntiles = N * q.tiles_y * q.tiles_x;
    int nb = q.ntiles < 512 ? q.ntiles : 512;
    const size_t out_elems = (size_t)64 * 49 * cin;        // 3,136 cin: a multiple of 4 for every cin (the reduce adds 16-byte vectors)
    q.slab = nullptr;
    if (workspace && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0 && (reinterpret_cast<uintptr_t>(dw) & 15) == 0 &&
        workspace_bytes >= out_elems * 4 && !getenv("VK_WGRAD_ATOMICS")) {
      const size_t cap = workspace_bytes / (out_elems * 4);
      if ((size_t)nb > cap) nb = (int)cap;
      q.slab = (float*)workspace;
    }
    const double flops = 2.0 * (double)N * q.Ho * q.Wo * 64.0 * 49.0 * cin;
    const double bytes = ((double)N * H * W * 4 + (double)N * q.Ho * q.Wo * 64 * (bn_z ? 2 : 1)) * 2.0 + 64.0 * 49 * cin * 4;
    auto stem = [&](auto e) {
      using T = decltype(e);
      if (bn_z) return vkh::launch<k_stem_wgrad<T, true>>(dim3((unsigned)nb), dim3(256), 0, st, "wgrad_stem_16b_bn", {}, flops, bytes, q);
      return vkh::launch<k_stem_wgrad<T, false>>(dim3((unsigned)nb), dim3(256), 0, st, "wgrad_stem_16b", {}, flops, bytes, q);
    };
    const int rc = dt == VK_BF16 ? stem(bf16_t()) : stem(f16_t());
    if (rc != VK_OK || !q.slab) return rc;
    return launch_slab_reduce(out_elems / 4, nb, q.slab, dw, st);
  }
  WgradParams p;
  p.s0 = plain_src(x4, 4, N, H, W, eb);
  p.s1 = no_src();
  p.dz = dz;
  p.dz_bytes = (uint32_t)((size_t)N * (H / 2) * (W / 2) * 64 * eb);
  p.dw = dw;
  p.slab = nullptr;
  p.N = N; p.H = H; p.W = W; p.Ho = H / 2; p.Wo = W / 2; p.K = 64; p.R = 7; p.S = 1;
  p.slog = 1; p.pad = 3;
  p.C = 32;
  p.M = N * p.Ho * p.Wo;
  p.RS = 7;
  p.stem = 1; p.cin = cin;
  p.div_hw = vkh::make_fastdiv((uint32_t)(p.Ho * p.Wo));
  p.div_w = vkh::make_fastdiv((uint32_t)p.Wo);
  p.div_s = vkh::make_fastdiv(1);
  return dispatch_dtype(dt, [&](auto e) { return launch_w<decltype(e), 64, 32, true>(p, workspace, workspace_bytes, st); });
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Data gradient of the stem (the gradient of the model's input): the transpose of the 7x7 stride-2 pad-3 convolution, 64 -> cin
// channels (1 <= cin <= 4), in the space-to-depth form.  Output pixel (2i + u, 2j + v) receives dz[i - 1 + wy][j - 1 + wx][k] * w[k][r][s][c] with
// r = u + 5 - 2 wy, s = v + 5 - 2 wx (a tap exists where 0 <= r, s <= 6: 3 rows for u = 0, 4 for u = 1), so every 2x2 output block
// (i, j) reads the same 4x4 window of dz.  One GEMM:  M = N * Ho * Wo blocks, K = 16 window positions x 64 channels, N = 4 cin outputs
// (u, v, c) -> column uv * cin + c, padded to 16 (four channels fill it exactly), against a re-packed weight matrix of which 49 / 64 taps are non-zero.
//   A (dz): lane (m = lane & 15, q = lane >> 4) holds block j0 + m, channels grp * 4 VE + q VE .. + VE - 1 of one window position:
//           ONE 16-byte NHWC load per lane and MFMA step (16-bit: one 16x16x32; fp32: four 16x16x4, Mma<float>'s k permutation);
//   B (weights): the same (window, group, lane) geometry, built once per workgroup in LDS from the fp32 KRSC master weights;
//   D: lane holds output (u, v, c) = lane & 15 of blocks j0 + 4q .. 4q + 3.
// BNA: dz = a*g + b*z + c is formed while loading (k_bn_bwd_apply's fp32 expression), zero outside the image: no dz pass.
// Workgroup: 4 waves on block rows 4 ty .. 4 ty + 3 of one 16-block column strip (their windows overlap: L1 / L2 reuse).
struct StemDgParams {
  const void* g;
  const void* z;
  const float* coef;      // [3][64] (BNA)
  const float* w;         // fp32 KRSC [64][7][7][cin]
  float* dx;              // fp32 NCHW [N][cin][H][W]
  int N, H, W, Ho, Wo, tiles_x, tiles_y, ntiles, cin;
};

template <typename T, bool BNA>
__global__ __launch_bounds__(256) void k_stem_dgrad(const StemDgParams p) {
  constexpr int VE = ElemTraits<T>::kVec;
  constexpr int CPG = 4 * VE;            // channels per MFMA step: 32 (16-bit), 16 (fp32)
  constexpr int NG = 64 / CPG;
  __shared__ u32x4_t Bs[16 * NG * 64];   // [window][group][lane]: 32 KB (16-bit) / 64 KB (fp32)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m = lane & 15, q = lane >> 4;
  for (int sl = tid; sl < 16 * NG * 64; sl += 256) {
    const int ln = sl & 63, grp = (sl >> 6) % NG, win = sl / (64 * NG);
    const int n = ln & 15, wy = win >> 2, wx = win & 3;
    const int uv = n / p.cin, c = n - p.cin * uv;
    const int r = (uv >> 1) + 5 - 2 * wy, s = (uv & 1) + 5 - 2 * wx;
    const bool tap = n < 4 * p.cin && r >= 0 && r <= 6 && s >= 0 && s <= 6;
    float f[VE];
#pragma unroll
    for (int j = 0; j < VE; ++j) {
      const int k = grp * CPG + (ln >> 4) * VE + j;
      f[j] = tap ? p.w[((k * 7 + r) * 7 + s) * p.cin + c] : 0.f;
    }
    Bs[sl] = Vec16<T>::pack(f);
  }
  float ca[NG][VE], cb[NG][VE], cc[NG][VE];
  if (BNA) {
#pragma unroll
    for (int grp = 0; grp < NG; ++grp)
#pragma unroll
      for (int j = 0; j < VE; ++j) {
        const int k = grp * CPG + q * VE + j;
        ca[grp][j] = p.coef[k];
        cb[grp][j] = p.coef[64 + k];
        cc[grp][j] = p.coef[128 + k];
      }
  }
  __syncthreads();
  const T* g = (const T*)p.g;
  const T* z = (const T*)p.z;
  const int uv = m / p.cin, c = m - p.cin * uv;      // this lane's output column m = uv * cin + c (a store only where m < 4 cin)
  for (int t = blockIdx.x; t < p.ntiles; t += gridDim.x) {
    const int tx = t % p.tiles_x, ty = (t / p.tiles_x) % p.tiles_y, nimg = t / (p.tiles_x * p.tiles_y);
    const int i = ty * 4 + wave, j0 = tx * 16;
    f32x4_t acc = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int wy = 0; wy < 4; ++wy) {
      const int oy = i - 1 + wy;
      const bool row_ok = oy >= 0 && oy < p.Ho;
#pragma unroll
      for (int wx = 0; wx < 4; ++wx) {
        const int ox = j0 + m - 1 + wx;
        const bool ok = row_ok && ox >= 0 && ox < p.Wo;
        const size_t pix = ((size_t)nimg * p.Ho + (ok ? oy : 0)) * p.Wo + (ok ? ox : 0);
#pragma unroll
        for (int grp = 0; grp < NG; ++grp) {
          const size_t e = pix * 64 + grp * CPG + q * VE;
          u32x4_t a = u32x4_t{0, 0, 0, 0};
          if (ok) {
            a = *reinterpret_cast<const u32x4_t*>(g + e);
            if (BNA) {
              float gf[VE], zf[VE], o[VE];
              Vec16<T>::unpack(a, gf);
              Vec16<T>::unpack(*reinterpret_cast<const u32x4_t*>(z + e), zf);
#pragma unroll
              for (int jj = 0; jj < VE; ++jj) o[jj] = fmaf(ca[grp][jj], gf[jj], fmaf(cb[grp][jj], zf[jj], cc[grp][jj]));
              a = Vec16<T>::pack(o);
            }
          }
          acc = Mma<T>::run(a, Bs[((wy * 4 + wx) * NG + grp) * 64 + lane], acc);
        }
      }
    }
    if (m < 4 * p.cin) {
      float* dst = p.dx + (((size_t)nimg * p.cin + c) * p.H + 2 * i + (uv >> 1)) * p.W + (uv & 1);
#pragma unroll
      for (int e = 0; e < 4; ++e) dst[2 * (j0 + 4 * q + e)] = acc[e];
    }
  }
}

static int stem_dgrad_impl(vk_dtype dt, int N, int H, int W, int cin, const void* g, const void* z, const float* coef, const float* w, float* dx,
                           hipStream_t st) {
  VK_CHECK_ARG(g && w && dx && (!coef || z), "vk_stem_dgrad: null argument");
  VK_CHECK_ARG(cin >= 1 && cin <= 4, "vk_stem_dgrad_c: cin=%d is outside 1..4", cin);
  VK_CHECK_ARG(N >= 1 && H >= 8 && W >= 32 && H % 8 == 0 && W % 32 == 0, "vk_stem_dgrad: H=%d W=%d (need H %% 8 == 0, W %% 32 == 0)", H, W);
  VK_CHECK_ARG(dt == VK_F32 || dt == VK_BF16 || dt == VK_F16, "vk_stem_dgrad: bad dtype");
  StemDgParams q;
  q.g = g; q.z = z; q.coef = coef; q.w = w; q.dx = dx;
  q.N = N; q.H = H; q.W = W; q.Ho = H / 2; q.Wo = W / 2; q.cin = cin;
  q.tiles_x = q.Wo / 16; q.tiles_y = q.Ho / 4;
  q.ntiles = N * q.tiles_x * q.tiles_y;
  const int cap = dt == VK_F32 ? 512 : 1024;            // persistent: every workgroup builds the weight table once
  const int nb = q.ntiles < cap ? q.ntiles : cap;
  const double eb = dt == VK_F32 ? 4.0 : 2.0;
  const double flops = 2.0 * (double)N * q.Ho * q.Wo * 1024.0 * 16.0;
  const double bytes = (double)N * q.Ho * q.Wo * 64 * eb * (coef ? 2.0 : 1.0) + (double)N * cin * H * W * 4.0;
  return dispatch_dtype(dt, [&](auto e) {
    using T = decltype(e);
    if (coef) return vkh::launch<k_stem_dgrad<T, true>>(dim3((unsigned)nb), dim3(256), 0, st, "stem_dgrad_bn", {}, flops, bytes, q);
    return vkh::launch<k_stem_dgrad<T, false>>(dim3((unsigned)nb), dim3(256), 0, st, "stem_dgrad", {}, flops, bytes, q);
  });
}

}  // namespace vk

extern "C" int vk_stem_dgrad_c(vk_dtype dtype, int N, int H, int W, int cin, const void* g, const void* z, const float* coef_abc, const float* w_krsc,
                               float* dx, void* stream) {
  return vk::stem_dgrad_impl(dtype, N, H, W, cin, g, z, coef_abc, w_krsc, dx, (hipStream_t)stream);
}
extern "C" int vk_stem_dgrad(vk_dtype dtype, int N, int H, int W, const void* g, const void* z, const float* coef_abc, const float* w_krsc3,
                             float* dx, void* stream) {
  return vk_stem_dgrad_c(dtype, N, H, W, 3, g, z, coef_abc, w_krsc3, dx, stream);
}

extern "C" int vk_conv_wgrad(const vk_conv_desc* d, const void* dz, float* dw, void* workspace, size_t workspace_bytes, void* stream) {
  return vk::conv_wgrad_impl(d, dz, dw, workspace, workspace_bytes, (hipStream_t)stream);
}
extern "C" int vk_stem_wgrad_c(vk_dtype dtype, int N, int H, int W, int cin, const void* x4, const void* dz, float* dw_krsc, void* workspace,
                               size_t workspace_bytes, void* stream) {
  return vk::stem_wgrad_impl(dtype, N, H, W, cin, x4, dz, dw_krsc, workspace, workspace_bytes, (hipStream_t)stream);
}
extern "C" int vk_stem_wgrad(vk_dtype dtype, int N, int H, int W, const void* x4, const void* dz, float* dw_krsc3, void* workspace,
                             size_t workspace_bytes, void* stream) {
  return vk_stem_wgrad_c(dtype, N, H, W, 3, x4, dz, dw_krsc3, workspace, workspace_bytes, stream);
}
extern "C" int vk_stem_wgrad_bn_c(vk_dtype dtype, int N, int H, int W, int cin, const void* x4, const void* g, const void* z, const float* coef_abc,
                                  float* dw_krsc, void* workspace, size_t workspace_bytes, void* stream) {
  VK_CHECK_ARG(z && coef_abc, "vk_stem_wgrad_bn: null argument");
  return vk::stem_wgrad_impl(dtype, N, H, W, cin, x4, g, dw_krsc, workspace, workspace_bytes, (hipStream_t)stream, z, coef_abc);
}
extern "C" int vk_stem_wgrad_bn(vk_dtype dtype, int N, int H, int W, const void* x4, const void* g, const void* z, const float* coef_abc,
                                float* dw_krsc3, void* workspace, size_t workspace_bytes, void* stream) {
  return vk_stem_wgrad_bn_c(dtype, N, H, W, 3, x4, g, z, coef_abc, dw_krsc3, workspace, workspace_bytes, stream);
}
