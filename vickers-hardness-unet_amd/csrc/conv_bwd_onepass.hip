// One-pass backward of the small-channel decoder convolutions (dec4.conv2: 16 -> 16 at full resolution, dec3.conv2: 32 -> 32 at half):
// BatchNorm-backward apply + data gradient (with the fused BN+ReLU-backward reduce of the layer below) + weight gradient in ONE kernel.
//
// The three launches it replaces move 8 T (T = one N*H*W*K tensor pass): the apply reads g, z and writes dz; the data gradient reads
// dz, z1 and writes g1; the weight gradient reads dz, z1 again.  dz has two readers, so folding the apply into each of them would still
// move 7 T.  Here dz is formed ONCE, in LDS, and both gradients are computed from that image: g, z, z1 in, g1 out = 4 T (+ 2/16 halo
// columns and 2/RS halo rows).  The structure is conv3x3_stream_kernel's (conv_halo.hip) with wgrad_stream_kernel's (wgrad_halo.hip)
// accumulators beside it:
//   * a wave owns a strip of 16 columns x RS rows and walks down it; per output row it requests ONE row each of g, z and z1, 18 pixels
//     wide, three rows ahead (register queue with compile-time indices), and has no workgroup barrier in the row loop;
//   * row j becomes two LDS images in the wave's private rings (4 slots each, pixel-major with the 48 / 96-byte pixel stride of the
//     streaming kernel: conflict-free for its ds_read_b128 fragments; for the transposed reads 96 bytes is conflict-free too, 48 bytes
//     is 2-way on three of the eight pixels of a 32-lane group — the 16-channel kernel is HBM-bound, a second image would only add writes): dz = pack(fmaf(a, g, fmaf(b, z, c))) — k_bn_bwd_apply's fp32 expression, rounded to T before any use — and
//     V = relu(z1 * scale + shift) as the forward's operand transform rounds it; both zero outside the image AFTER the transform;
//   * data gradient: the MODE 2 row of conv3x3_stream_kernel, operand for operand (taps ascending, one chain per accumulator), then its
//     epilogue: g1 = y * [V > 0] stored, sum g1 and sum g1 * z1 in fp32 over the rows of one STREAMING-kernel strip (RSsum, which
//     divides this kernel's taller strip), then fp64 atomics into the 32 replicas.  g1 and the sums are bit for bit what
//     vk_bn_bwd_apply + vk_conv_dgrad_fused leave;
//   * weight gradient: every second row one K = 32 MFMA step over (2 rows x 16 pixels) per tap and 16 x 16 tile, fragments by the
//     LDS-transposing reads from the SAME two images (dz pixels 1..16 of the 18, V pixels s..s+15), K x 9 x C fp32 accumulators per
//     wave for the whole strip; the four waves of a workgroup add their tiles in LDS in wave order, every workgroup writes one slab
//     and k_wgrad_slab_reduce adds the slabs in a fixed order: run-to-run reproducible.
#include <stdlib.h>

#include <string>
#include <type_traits>

#include "conv_host.h"

namespace vk {

int launch_slab_reduce(size_t n4, int splits, const float* slab, float* dw, hipStream_t st);      // wgrad_halo.hip

struct OnePassParams {
  const void *g, *z, *z1, *w;
  void* y;
  const float *coef, *scale, *shift, *bnr_scale, *bnr_shift;
  double* sums;
  float* slab;
  int N, H, W, RS, RSsum, relu;
  uint32_t w_bytes, t_bytes, t1_bytes;                    // filter, g / z, z1 / y (t1 = t except in the upsampled form)
};

template <int CK>
struct OnePassCfg {
  static constexpr int NSTEP = CK == 16 ? 5 : 9;
  static constexpr int APS = CK == 16 ? 48 : 96;           // LDS pixel stride (StreamCfg)
  static constexpr int VPP = CK / 8;
  static constexpr int NVEC = 18 * VPP;
  static constexpr int NLD = (NVEC + 63) / 64;
  static constexpr int ROWB = CK == 16 ? 1024 : 2048;
  static constexpr int V_OFF = 4 * ROWB, ZERO_OFF = 8 * ROWB;
  static constexpr int WAVE_LDS = 8 * ROWB + 64;           // dz ring, V ring, a zero line (the non-existent 10th tap at C = 16)
  static constexpr int RED = CK * 9 * CK * 4;
  static constexpr int SMEM = 4 * WAVE_LDS > RED ? 4 * WAVE_LDS : RED;
  static_assert(18 * APS <= ROWB && NLD <= 2, "row image");
};

template <typename T, int CK>
__global__ __launch_bounds__(256, (CK == 16 ? 2 : 1)) void conv_bwd_onepass_kernel(const OnePassParams p) {
  using Cfg = OnePassCfg<CK>;
  constexpr int NSTEP = Cfg::NSTEP, APS = Cfg::APS, VPP = Cfg::VPP, NVEC = Cfg::NVEC, NLD = Cfg::NLD, ROWB = Cfg::ROWB;
  constexpr int VE = 8, TC = CK / 16;
  static_assert(sizeof(T) == 2, "16-bit element types");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  typedef __attribute__((address_space(3))) s16x4_t* lds_s16x4_ptr;
  const int RS = p.RS;                                     // strip height: a multiple of 8
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  char* const ring = smem + wave * Cfg::WAVE_LDS;          // dz rows
  char* const vring = ring + Cfg::V_OFF;                   // V rows
  const int strips_x = (p.W + 15) / 16, strips_y = (p.H + RS - 1) / RS;
  int sid = (int)blockIdx.x * 4 + wave;
  const bool active = sid < p.N * strips_y * strips_x;
  const int strip = sid;
  const int sx = sid % strips_x;
  sid /= strips_x;
  const int sy = sid % strips_y;
  const int n = sid / strips_y;
  const int x0 = sx * 16, ys = sy * RS, ye = min(p.H, ys + RS);
  const int li = lane & 15, kg = lane >> 4;

  f32x4_t wacc[9][TC][TC];                                 // weight gradient of the strip: [tap][k tile][c tile]
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int a = 0; a < TC; ++a)
#pragma unroll
      for (int b = 0; b < TC; ++b) wacc[t][a][b] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  if (active) {
    const __amdgpu_buffer_rsrc_t rsg = make_rsrc(p.g, p.t_bytes);
    const __amdgpu_buffer_rsrc_t rsz = make_rsrc(p.z, p.t_bytes);
    const __amdgpu_buffer_rsrc_t rs1 = make_rsrc(p.z1, p.t_bytes);
    const __amdgpu_buffer_rsrc_t rsw = make_rsrc(p.w, p.w_bytes);

    // ---- the data-gradient filter: registers, for the whole strip (conv3x3_stream_kernel with flip: plain [C][9][16] at 16 channels,
    // halo pack [9][C][4 swizzled 16-byte pieces] at 32)
    u32x4_t wf[NSTEP][TC];
#pragma unroll
    for (int st = 0; st < NSTEP; ++st)
#pragma unroll
      for (int a = 0; a < TC; ++a) {
        const int row = a * 16 + li;
        uint32_t off;
        bool ok = true;
        if (CK == 16) {
          const int tap = 2 * st + (kg >> 1);
          ok = tap < 9;
          off = (uint32_t)(((row * 9 + (8 - tap)) * 16 + (kg & 1) * VE) * 2);
        } else {
          const int pos = kg ^ (((row >> 2) & 1) << 1);
          off = (uint32_t)((((8 - st) * CK + row) * 4 + pos) * 16);
        }
        wf[st][a] = buf_load16(rsw, ok ? off : kOOB);
      }
    if (lane < 4) *reinterpret_cast<u32x4_t*>(ring + Cfg::ZERO_OFF + lane * 16) = u32x4_t{0, 0, 0, 0};

    // ---- staging geometry of this lane (fixed for the strip; the lane map of conv3x3_stream_kernel): vector v -> pixel hx, piece hv
    int st_off[NLD], ld_col[NLD];
    bool xok[NLD];
#pragma unroll
    for (int q = 0; q < NLD; ++q) {
      const int v = lane + 64 * q;
      int hx = v / VPP, hv = v % VPP;
      if (VPP == 4) {
        if ((hx | 3) < 18) hx = (hx & ~3) | ((hx & 1) << 1) | ((hx >> 1) & 1);
      } else {
        if ((v | 15) < NVEC) { hx = (v & 7) | ((v >> 4) << 3); hv = (v >> 3) & 1; }
      }
      const int xs = x0 - 1 + hx;
      xok[q] = v < NVEC && (unsigned)xs < (unsigned)p.W;
      ld_col[q] = xs * CK + hv * VE;
      st_off[q] = v < NVEC ? hx * APS + hv * 16 : -1;
    }
    // the 8 channels of this lane's vector(s): VPP = 4: piece lane % 4 for both; VPP = 2: one vector per lane, piece from the map above
    static_assert(VPP == 4 || NLD == 1, "C = 16: one staged vector per lane");
    const int hvl = VPP == 4 ? lane % VPP : (((lane | 15) < NVEC) ? (lane >> 3) & 1 : lane % VPP);
    const bool aff = p.scale != nullptr, relu = p.relu != 0;
    float sc[VE], sh[VE], ca[VE], cb[VE], cc[VE];
#pragma unroll
    for (int j = 0; j < VE; ++j) {
      sc[j] = aff ? p.scale[hvl * VE + j] : 1.f;
      sh[j] = aff ? p.shift[hvl * VE + j] : 0.f;
      ca[j] = p.coef[hvl * VE + j];
      cb[j] = p.coef[CK + hvl * VE + j];
      cc[j] = p.coef[2 * CK + hvl * VE + j];
    }
    struct RowQ {
      u32x4_t g[NLD], z[NLD], v[NLD];
    };
    auto issue = [&](int j, RowQ& r) {                     // request row j of g, z, z1 (zeros outside the map)
      const bool rok = (unsigned)j < (unsigned)p.H;
#pragma unroll
      for (int q = 0; q < NLD; ++q) {
        const uint32_t off = (rok && xok[q]) ? (uint32_t)(((n * p.H + j) * p.W) * CK + ld_col[q]) * 2u : kOOB;
        r.g[q] = buf_load16(rsg, off);
        r.z[q] = buf_load16(rsz, off);
        r.v[q] = buf_load16(rs1, off);
      }
    };
    auto write_row = [&](int j, const RowQ& r) {
      const bool rok = (unsigned)j < (unsigned)p.H;
      const int slot = (j & 3) * ROWB;
#pragma unroll
      for (int q = 0; q < NLD; ++q) {
        if (st_off[q] < 0) continue;
        float gf[VE], zf[VE], o[VE];
        Vec16<T>::unpack(r.g[q], gf);
        Vec16<T>::unpack(r.z[q], zf);
#pragma unroll
        for (int e = 0; e < VE; ++e) o[e] = fmaf(ca[e], gf[e], fmaf(cb[e], zf[e], cc[e]));
        u32x4_t dz = Vec16<T>::pack(o);
        u32x4_t v = r.v[q];
        if (aff) v = AffineRelu<T>::run(v, sc, sh, relu);
        if (!(rok && xok[q])) {                            // zero padding applies AFTER the transforms (c and shift must not leak)
          dz = u32x4_t{0, 0, 0, 0};
          v = u32x4_t{0, 0, 0, 0};
        }
        *reinterpret_cast<u32x4_t*>(ring + slot + st_off[q]) = dz;
        *reinterpret_cast<u32x4_t*>(vring + slot + st_off[q]) = v;
      }
    };

    // ---- data-gradient fragment reads (conv3x3_stream_kernel)
    int fr_r16[CK == 16 ? NSTEP : 1], fr_off16[CK == 16 ? NSTEP : 1];
    if (CK == 16) {
#pragma unroll
      for (int st = 0; st < NSTEP; ++st) {
        const int tap = 2 * st + (kg >> 1);
        const int r = tap / 3, sxx = tap - r * 3;
        fr_r16[st] = tap < 9 ? r : -100;
        fr_off16[st] = (li + sxx) * APS + (kg & 1) * 16;
      }
    }
    const int fr_base32 = kg * 16;
    // ---- weight-gradient fragment reads (wgrad_stream_kernel): lane j of 16-lane group g supplies pixel 4 g + (j >> 2), channels
    // 4 (j & 3) ..; dz pixel px is ring pixel px + 1, V pixel px under filter column s is ring pixel px + s
    const int lane_t = (4 * kg + (li >> 2)) * APS + (4 * (lane & 3)) * 2;
    auto tr = [](const char* q) { return __builtin_bit_cast(u32x2_t, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(q))); };

    // ---- output side of the data gradient
    const int xo = x0 + li;
    const bool x_ok = xo < p.W;
    float bsc[TC][4], bsh[TC][4], s1[TC][4], s2[TC][4];
#pragma unroll
    for (int a = 0; a < TC; ++a)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int ch = a * 16 + kg * 4 + e;
        bsc[a][e] = p.bnr_scale[ch];
        bsh[a][e] = p.bnr_shift[ch];
        s1[a][e] = 0.f; s2[a][e] = 0.f;
      }
    auto round_t = [&](float (&f)[4]) {                    // to T and back: everything downstream sees the stored values
      float g[8] = {f[0], f[1], f[2], f[3], 0.f, 0.f, 0.f, 0.f};
      const u32x4_t pk = Vec16<T>::pack(g);
      Vec16<T>::unpack(pk, g);
#pragma unroll
      for (int e = 0; e < 4; ++e) f[e] = g[e];
      return u32x2_t{pk[0], pk[1]};
    };
    // 32-bit byte offsets; lanes and rows that must not touch memory get the out-of-range offset (loads answer zeros, stores are skipped)
    const uint32_t lane_ob = x_ok ? (uint32_t)(((n * p.H) * p.W + xo) * CK + kg * 4) * 2u : kOOB;
    const uint32_t row_ob = (uint32_t)(p.W * CK * 2);
    auto out_off = [&](int a, int y) -> uint32_t { return lane_ob + (uint32_t)y * row_ob + (uint32_t)(a * 32); };
    u32x2_t zq[2][TC];
    auto z_issue = [&](int y, u32x2_t (&z)[TC]) {
      const bool ok = y < p.H;
#pragma unroll
      for (int a = 0; a < TC; ++a) z[a] = __builtin_amdgcn_raw_buffer_load_b64(rs1, ok ? out_off(a, y) : kOOB, 0, 0);
    };
    auto finish = [&](int a, float (&f)[4], uint32_t boff, bool counted, u32x2_t zr) {
      float zf[8];
      Vec16<T>::unpack(u32x4_t{zr[0], zr[1], 0u, 0u}, zf);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (!counted || !(fmaf(zf[e], bsc[a][e], bsh[a][e]) > 0.f)) f[e] = 0.f;      // pixels outside the map add nothing
        s1[a][e] += f[e];
        s2[a][e] += f[e] * zf[e];
      }
      const u32x2_t pk = round_t(f);
      if ((int32_t)boff >= 0) *reinterpret_cast<u32x2_t*>((char*)p.y + boff) = pk;
    };

    // ---- the row pipeline: source row j lives in queue set j & 3 until it is written to ring slot j & 3 (ys is a multiple of 8)
    RowQ pre[4];
    issue(ys - 1, pre[3]);
    issue(ys, pre[0]);
    issue(ys + 1, pre[1]);
    issue(ys + 2, pre[2]);
    z_issue(ys, zq[0]);
    write_row(ys - 1, pre[3]);
    issue(ys + 3, pre[3]);
    write_row(ys, pre[0]);
    auto row = [&](int y, auto ph_c) {
      constexpr int PH = decltype(ph_c)::value;            // y & 3
      write_row(y + 1, pre[(PH + 1) & 3]);
      issue(y + 4, pre[PH & 3]);                           // row y + 4 shares the slot of row y, written one iteration ago
      z_issue(y + 1, zq[(PH & 1) ^ 1]);
      // ---- data gradient of row y: dz rows y - 1 .. y + 1
      f32x4_t acc[TC];
#pragma unroll
      for (int a = 0; a < TC; ++a) acc[a] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int st = 0; st < NSTEP; ++st) {
        int addr;
        if (CK == 16) {
          const int vrow = y - 1 + fr_r16[st];
          addr = fr_r16[st] < 0 ? Cfg::ZERO_OFF : (vrow & 3) * ROWB + fr_off16[st];
        } else {
          const int r = st / 3, sxx = st - r * 3;
          addr = ((y - 1 + r) & 3) * ROWB + (li + sxx) * APS + fr_base32;
        }
        const u32x4_t xf = *reinterpret_cast<const u32x4_t*>(ring + addr);
#pragma unroll
        for (int a = 0; a < TC; ++a) acc[a] = Mma<T>::run(wf[st][a], xf, acc[a]);
      }
      // every MFMA of the row stays in front of every accumulator read of its epilogue (the r03 hazard)
      __builtin_amdgcn_sched_barrier(0);
      const bool y_ok = y < p.H;
#pragma unroll
      for (int a = 0; a < TC; ++a) {
        float f[4] = {acc[a][0], acc[a][1], acc[a][2], acc[a][3]};
        (void)round_t(f);
        finish(a, f, y_ok ? out_off(a, y) : kOOB, x_ok && y_ok, zq[PH & 1][a]);
      }
      // ---- weight gradient of rows y - 1, y (every second row): dz rows y - 1, y against V rows y - 2 + r, y - 1 + r
      if constexpr ((PH & 1) == 1) {
        constexpr int SL = (PH + 3) & 3, SH = PH & 3;       // slots of rows y - 1, y
        u32x4_t zf[TC];
#pragma unroll
        for (int a = 0; a < TC; ++a) {
          const u32x2_t lo = tr(ring + SL * ROWB + APS + lane_t + a * 32), hi = tr(ring + SH * ROWB + APS + lane_t + a * 32);
          zf[a] = u32x4_t{lo[0], lo[1], hi[0], hi[1]};
        }
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          const int slo = ((PH + 2 + r) & 3) * ROWB, shi = ((PH + 3 + r) & 3) * ROWB;      // rows y - 2 + r, y - 1 + r
#pragma unroll
          for (int s_ = 0; s_ < 3; ++s_) {
            u32x4_t vf[TC];
#pragma unroll
            for (int b = 0; b < TC; ++b) {
              const u32x2_t lo = tr(vring + slo + s_ * APS + lane_t + b * 32), hi = tr(vring + shi + s_ * APS + lane_t + b * 32);
              vf[b] = u32x4_t{lo[0], lo[1], hi[0], hi[1]};
            }
#pragma unroll
            for (int a = 0; a < TC; ++a)
#pragma unroll
              for (int b = 0; b < TC; ++b) wacc[r * 3 + s_][a][b] = Mma<T>::run(zf[a], vf[b], wacc[r * 3 + s_][a][b]);
          }
        }
      }
    };
    // BN+ReLU-backward sums: 16 lanes of a row hold the same channels -> DPP row sum, one lane per row adds them.  The fp32 partials
    // cover RSsum rows — the strip height the streaming data gradient would take for this map — and go to fp64 there, not at the end
    // of this kernel's (taller) strip: the sums, and with them conv1's BatchNorm-backward coefficients, keep the bits of the three
    // launches (an fp32 partial over another span differs in its last bits, and the cancelling S_gz - mu S_g magnifies that)
    double* const sp = p.sums + (size_t)(strip % VK_STATS_REPLICAS) * 2 * CK;
    auto flush_sums = [&]() {
#pragma unroll
      for (int a = 0; a < TC; ++a)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float u = row16_sum(s1[a][e]), v = row16_sum(s2[a][e]);
          const int ch = a * 16 + kg * 4 + e;
          if (li == 0) {
            atomicAdd(sp + ch, (double)u);
            atomicAdd(sp + CK + ch, (double)v);
          }
          s1[a][e] = 0.f; s2[a][e] = 0.f;
        }
    };
    // rows at or beyond H inside the last group of four run on zero rows and store nothing; dz rows of the neighbouring strips (ys - 1,
    // ys + RS) only ever enter the data gradient: the weight-gradient pairs are (ys, ys + 1) .. (ys + RS - 2, ys + RS - 1)
    const int RSsum = p.RSsum;                             // a multiple of 8 that divides RS
    for (int yb = ys, left = RSsum; yb < ye; yb += 4) {
      row(yb, std::integral_constant<int, 0>{});
      row(yb + 1, std::integral_constant<int, 1>{});
      row(yb + 2, std::integral_constant<int, 2>{});
      row(yb + 3, std::integral_constant<int, 3>{});
      left -= 4;
      if (left == 0 || yb + 4 >= ye) {
        flush_sums();
        left = RSsum;
      }
    }
  }

  // ---- the four waves add their weight-gradient tiles in wave order; one slab per workgroup
  __syncthreads();                                           // every wave is done with its rings
  float* const red = reinterpret_cast<float*>(smem);
#pragma unroll 1
  for (int phase = 0; phase < 4; ++phase) {
    if (wave == phase) {
#pragma unroll
      for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int a = 0; a < TC; ++a)
#pragma unroll
          for (int b = 0; b < TC; ++b)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int k = a * 16 + kg * 4 + e, c = b * 16 + li;
              float* dst = red + (k * 9 + t) * CK + c;
              if (phase > 0) *dst += wacc[t][a][b][e];
              else *dst = wacc[t][a][b][e];
            }
    }
    __syncthreads();
  }
  float* const slab = p.slab + (size_t)blockIdx.x * CK * 9 * CK;
  for (int i = tid; i < CK * 9 * CK / 4; i += 256) *reinterpret_cast<f32x4_t*>(slab + i * 4) = *reinterpret_cast<const f32x4_t*>(red + i * 4);
}

template <typename T, int CK>
static int launch_onepass(OnePassParams p, float* dw, size_t slab_bytes, hipStream_t st) {
  using Cfg = OnePassCfg<CK>;
  // strip height: the tallest of 32-256 rows that still gives every resident wave a strip, i.e. ONE round of the grid (2 workgroups per CU
  // at 16 channels, 1 at 32: 2,048 / 1,024 waves).  Measured at bs 32 (profiles/onepass/strip_height.log): 16 channels at 512^2
  // 333 / 281 / 256 / 250 us at 32 / 64 / 128 / 256 rows, 32 channels at 256^2 264 / 215 / 190 / 328 us at 32 / 64 / 128 / 256 — every
  // further round pays the prologue, the sums' atomics and the workgroup's slab again.  VK_STREAM_RS overrides (tests / sweeps).
  const char* e_rs = getenv("VK_STREAM_RS");
  int RS = 256;
  if (e_rs) {
    RS = atoi(e_rs);
  } else {
    const long per_row_block = (long)p.N * ((p.W + 15) / 16), resident = CK == 16 ? 2048 : 1024;
    while (RS > 32 && per_row_block * ((p.H + RS - 1) / RS) < resident) RS >>= 1;
  }
  RS = (RS + 7) & ~7;
  if (RS < 8) RS = 8;
  // span of one fp32 partial of the BN-backward sums: the streaming kernel's strip height (stream_strip_rows states the invariant)
  int RSsum = RS;
  if (!e_rs) {
    RSsum = stream_strip_rows(p.N, p.H, p.W);
    if (RS < RSsum) RS = RSsum;                            // both are 32 << n: RSsum divides RS
  }
  p.RSsum = RSsum;
  p.RS = RS;
  const long strips = (long)p.N * ((p.H + RS - 1) / RS) * ((p.W + 15) / 16);
  const long nwg = (strips + 3) / 4;
  if ((size_t)nwg * CK * 9 * CK * sizeof(float) > slab_bytes) return VK_ERR_UNSUPPORTED;
  static const std::string tag = std::string("bwd_onepass_16b_c") + std::to_string(CK);
  const double px = (double)p.N * p.H * p.W;
  const int rc = vkh::launch<conv_bwd_onepass_kernel<T, CK>>(dim3((unsigned)nwg), dim3(256), Cfg::SMEM, st, tag.c_str(), {}, 2.0 * 2.0 * px * CK * 9.0 * CK,
                                                             4.0 * px * CK * 2.0 + 9.0 * CK * CK * (2.0 + 4.0), p);
  if (rc != VK_OK) return rc;
  return launch_slab_reduce((size_t)CK * 9 * CK / 4, (int)nwg, p.slab, dw, st);
}

// ---- the upsampled-source form (dec4.conv1: 32 channels at half resolution, nearest x2, -> 16 channels at full resolution).  The three
// launches it replaces move 6.5 T (T = one N*H*W*16 pass): apply g, z -> dz; data gradient dz, z1 (T/2) -> g1 (T/2) behind the 2x2
// pooling; weight gradient dz, z1.  Here g, z, z1 in and g1 out = 3 T.  Same pipeline as conv_bwd_onepass_kernel with these differences:
//   * dz (16 channels, 48-byte pixels) is requested and written every row; V = relu(z1 * scale + shift) comes from the HALF-resolution
//     source, 10 pixels x 32 channels per source row, one source row per two output rows, each source pixel written to its two halo
//     columns (wgrad_stream_kernel<T, 16, true>): the V image is 18 full-resolution pixels of 96 bytes, four source rows deep;
//   * data gradient: the MODE 3 row of conv3x3_stream_kernel<T, 16, 2, false, 3>, operand for operand (five two-tap steps, two output
//     tiles), every full-resolution value rounded to T, the four of a 2x2 block added as ((prev + pn) + f) + cn, then that kernel's
//     finish on the odd rows: mask [bn(z1) > 0], sums, store from the even lanes into [N][H/2][W/2][32];
//   * weight gradient: K = 16 x C = 32; on odd rows y = 2m + 1 the pairs (dz rows y - 1, y) against V rows (y - 2 + r, y - 1 + r), i.e.
//     source rows (m - 1, m), (m, m), (m, m + 1) for r = 0, 1, 2: three transposed reads per filter column and channel tile feed six MFMAs.
struct OnePassUpCfg {
  static constexpr int NSTEP = 5, APS = 48, ROWB = 1024;   // dz image (StreamCfg<T, 16, false>)
  static constexpr int VSB = 96, VROW = 18 * VSB;          // V image (WsCfg<T, 16, true>)
  static constexpr int V_OFF = 4 * ROWB, ZERO_OFF = V_OFF + 4 * VROW;
  // per-channel constants of the wave, read from LDS where they are used (in registers they would not leave room for two workgroups
  // per CU): a, b, c [16] each, scale, shift [32] each, bnr scale, bnr shift [32] each
  static constexpr int TAB_OFF = ZERO_OFF + 64, TAB_SC = 48, TAB_SH = 80, TAB_BSC = 112, TAB_BSH = 144, TAB_N = 176;
  static constexpr int WAVE_LDS = TAB_OFF + TAB_N * 4;
  static constexpr int K = 16, C = 32;
  static constexpr int RED = K * 9 * C * 4;
  static constexpr int SMEM = 4 * WAVE_LDS > RED ? 4 * WAVE_LDS : RED;
  static_assert(18 * APS <= ROWB && WAVE_LDS % 16 == 0, "row images");
};

template <typename T>
__global__ __launch_bounds__(256, 2) void conv_bwd_onepass_up_kernel(const OnePassParams p) {
  using Cfg = OnePassUpCfg;
  constexpr int NSTEP = Cfg::NSTEP, APS = Cfg::APS, ROWB = Cfg::ROWB, VSB = Cfg::VSB, VROW = Cfg::VROW;
  constexpr int VE = 8, TC = 2, K = Cfg::K, C = Cfg::C;
  static_assert(sizeof(T) == 2, "16-bit element types");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  typedef __attribute__((address_space(3))) s16x4_t* lds_s16x4_ptr;
  const int RS = p.RS;                                     // strip height: a multiple of 8
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  char* const ring = smem + wave * Cfg::WAVE_LDS;          // dz rows: row j in slot j & 3
  char* const vring = ring + Cfg::V_OFF;                   // V source rows: row m in slot m & 3
  const int strips_x = (p.W + 15) / 16, strips_y = (p.H + RS - 1) / RS;
  int sid = (int)blockIdx.x * 4 + wave;
  const bool active = sid < p.N * strips_y * strips_x;
  const int strip = sid;
  const int sx = sid % strips_x;
  sid /= strips_x;
  const int sy = sid % strips_y;
  const int n = sid / strips_y;
  const int x0 = sx * 16, ys = sy * RS, ye = min(p.H, ys + RS);
  const int li = lane & 15, kg = lane >> 4;
  const int Hs = p.H >> 1, Ws = p.W >> 1;                  // H, W even (host)

  f32x4_t wacc[9][TC];                                     // weight gradient of the strip: [tap][c tile], k = 4 kg + e, c = 16 b + li
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int b = 0; b < TC; ++b) wacc[t][b] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  if (active) {
    const __amdgpu_buffer_rsrc_t rsg = make_rsrc(p.g, p.t_bytes);
    const __amdgpu_buffer_rsrc_t rsz = make_rsrc(p.z, p.t_bytes);
    const __amdgpu_buffer_rsrc_t rs1 = make_rsrc(p.z1, p.t1_bytes);
    const __amdgpu_buffer_rsrc_t rsw = make_rsrc(p.w, p.w_bytes);

    // ---- the data-gradient filter: registers, for the whole strip (conv3x3_stream_kernel at C = 16 with flip: plain [32][9][16])
    u32x4_t wf[NSTEP][TC];
#pragma unroll
    for (int st = 0; st < NSTEP; ++st)
#pragma unroll
      for (int a = 0; a < TC; ++a) {
        const int tap = 2 * st + (kg >> 1);
        const uint32_t off = (uint32_t)((((a * 16 + li) * 9 + (8 - tap)) * 16 + (kg & 1) * VE) * 2);
        wf[st][a] = buf_load16(rsw, tap < 9 ? off : kOOB);
      }
    if (lane < 4) *reinterpret_cast<u32x4_t*>(ring + Cfg::ZERO_OFF + lane * 16) = u32x4_t{0, 0, 0, 0};

    // ---- staging geometry of this lane (fixed for the strip).  g, z: 36 vectors, the 16-channel lane map of conv3x3_stream_kernel
    int d_off, d_col;
    bool d_xok;
    int hvd;
    {
      int hx = lane >> 1;
      hvd = lane & 1;
      if ((lane | 15) < 36) { hx = (lane & 7) | ((lane >> 4) << 3); hvd = (lane >> 3) & 1; }
      const int xs = x0 - 1 + hx;
      d_xok = lane < 36 && (unsigned)xs < (unsigned)p.W;
      d_col = xs * K + hvd * VE;
      d_off = lane < 36 ? hx * APS + hvd * 16 : -1;
    }
    // V: 40 vectors, source pixel lane >> 2 (source column x0 / 2 - 1 + pixel), piece lane & 3 (wgrad_stream_kernel)
    const int vj = lane >> 2;
    const int vcs = (x0 >> 1) - 1 + vj;
    const bool v_lane = lane < 40, v_xok = v_lane && (unsigned)vcs < (unsigned)Ws;
    const int v_col = vcs * C + (lane & 3) * VE;
    const bool aff = p.scale != nullptr, relu = p.relu != 0;
    float* const tab = reinterpret_cast<float*>(ring + Cfg::TAB_OFF);
    for (int i = lane; i < Cfg::TAB_N; i += 64) {
      float v;
      if (i < Cfg::TAB_SC) v = p.coef[i];
      else if (i < Cfg::TAB_SH) v = aff ? p.scale[i - Cfg::TAB_SC] : 1.f;
      else if (i < Cfg::TAB_BSC) v = aff ? p.shift[i - Cfg::TAB_SH] : 0.f;
      else if (i < Cfg::TAB_BSH) v = p.bnr_scale[i - Cfg::TAB_BSC];
      else v = p.bnr_shift[i - Cfg::TAB_BSH];
      tab[i] = v;
    }
    const float* const tab_d = tab + hvd * VE;             // a, b, c of this lane's 8 dz channels
    const float* const tab_v = tab + (lane & 3) * VE;      // scale, shift of this lane's 8 source channels
    const float* const tab_o = tab + kg * 4;               // bnr scale, shift of this lane's 4 + 4 output channels
    auto ld8 = [](const float* q, float (&o)[VE]) {
      const f32x4_t lo = *reinterpret_cast<const f32x4_t*>(q), hi = *reinterpret_cast<const f32x4_t*>(q + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) { o[e] = lo[e]; o[4 + e] = hi[e]; }
    };
    struct RowQ {
      u32x4_t g, z;
    };
    auto issue = [&](int j, RowQ& r) {                     // request row j of g and z (zeros outside the map)
      const bool ok = (unsigned)j < (unsigned)p.H && d_xok;
      const uint32_t off = ok ? (uint32_t)(((n * p.H + j) * p.W) * K + d_col) * 2u : kOOB;
      r.g = buf_load16(rsg, off);
      r.z = buf_load16(rsz, off);
    };
    auto issue_v = [&](int m, u32x4_t& r) {                // request source row m of z1
      const bool ok = (unsigned)m < (unsigned)Hs && v_xok;
      r = buf_load16(rs1, ok ? (uint32_t)(((n * Hs + m) * Ws) * C + v_col) * 2u : kOOB);
    };
    auto write_row = [&](int j, const RowQ& r) {
      if (d_off < 0) return;
      float gf[VE], zf[VE], o[VE], ca[VE], cb[VE], cc[VE];
      ld8(tab_d, ca);
      ld8(tab_d + K, cb);
      ld8(tab_d + 2 * K, cc);
      Vec16<T>::unpack(r.g, gf);
      Vec16<T>::unpack(r.z, zf);
#pragma unroll
      for (int e = 0; e < VE; ++e) o[e] = fmaf(ca[e], gf[e], fmaf(cb[e], zf[e], cc[e]));
      u32x4_t dz = Vec16<T>::pack(o);
      if (!((unsigned)j < (unsigned)p.H && d_xok)) dz = u32x4_t{0, 0, 0, 0};      // zero padding applies AFTER the transform (c must not leak)
      *reinterpret_cast<u32x4_t*>(ring + (j & 3) * ROWB + d_off) = dz;
    };
    auto write_v = [&](int m, const u32x4_t& r) {          // source pixel j -> halo columns 2 j - 1, 2 j
      if (!v_lane) return;
      u32x4_t x = r;
      if (aff) {
        float sc[VE], sh[VE];
        ld8(tab_v + Cfg::TAB_SC, sc);
        ld8(tab_v + Cfg::TAB_SH, sh);
        x = AffineRelu<T>::run(x, sc, sh, relu);
      }
      if (!((unsigned)m < (unsigned)Hs && v_xok)) x = u32x4_t{0, 0, 0, 0};       // the shift must not leak either
      char* const dst = vring + (m & 3) * VROW + (lane & 3) * 16;
      if (vj > 0) *reinterpret_cast<u32x4_t*>(dst + (2 * vj - 1) * VSB) = x;
      if (vj < 9) *reinterpret_cast<u32x4_t*>(dst + (2 * vj) * VSB) = x;
    };

    // ---- data-gradient fragment reads (conv3x3_stream_kernel, C = 16)
    int fr_r16[NSTEP], fr_off16[NSTEP];
#pragma unroll
    for (int st = 0; st < NSTEP; ++st) {
      const int tap = 2 * st + (kg >> 1);
      const int r = tap / 3, sxx = tap - r * 3;
      fr_r16[st] = tap < 9 ? r : -100;
      fr_off16[st] = (li + sxx) * APS + (kg & 1) * 16;
    }
    // ---- weight-gradient fragment reads (wgrad_stream_kernel): lane j of 16-lane group g supplies pixel 4 g + (j >> 2), channels
    // 4 (j & 3) ..; dz pixel px is ring pixel px + 1, V pixel px under filter column s is halo column px + s
    const int lane_z = (4 * kg + (li >> 2) + 1) * APS + (4 * (lane & 3)) * 2;
    const int lane_v = (4 * kg + (li >> 2)) * VSB + (4 * (lane & 3)) * 2;
    auto tr = [](const char* q) { return __builtin_bit_cast(u32x2_t, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(q))); };

    // ---- output side of the data gradient: the pooled pixel (y >> 1, xo >> 1) of [N][H/2][W/2][32], stored by the even lanes
    const int xo = x0 + li;
    const bool lane_stores = xo < p.W && (li & 1) == 0;
    float s1[TC][4], s2[TC][4], prev[TC][4];
#pragma unroll
    for (int a = 0; a < TC; ++a)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        s1[a][e] = 0.f; s2[a][e] = 0.f; prev[a][e] = 0.f;
      }
    auto round_t = [&](float (&f)[4]) {                    // to T and back: everything downstream sees the stored values
      float g[8] = {f[0], f[1], f[2], f[3], 0.f, 0.f, 0.f, 0.f};
      const u32x4_t pk = Vec16<T>::pack(g);
      Vec16<T>::unpack(pk, g);
#pragma unroll
      for (int e = 0; e < 4; ++e) f[e] = g[e];
      return u32x2_t{pk[0], pk[1]};
    };
    // 32-bit byte offsets; lanes and rows that must not touch memory get the out-of-range offset (loads answer zeros, stores are skipped)
    const uint32_t lane_ob = lane_stores ? (uint32_t)(((n * Hs) * Ws + (xo >> 1)) * C + kg * 4) * 2u : kOOB;
    const uint32_t row_ob = (uint32_t)(Ws * C * 2);
    auto out_off = [&](int a, int y) -> uint32_t { return lane_ob + (uint32_t)(y >> 1) * row_ob + (uint32_t)(a * 32); };
    u32x2_t zq[2][TC];
    auto z_issue = [&](int y, u32x2_t (&z)[TC]) {
      const bool ok = y < p.H;
#pragma unroll
      for (int a = 0; a < TC; ++a) z[a] = __builtin_amdgcn_raw_buffer_load_b64(rs1, ok ? out_off(a, y) : kOOB, 0, 0);
    };
    auto finish = [&](int a, float (&f)[4], uint32_t boff, bool counted, u32x2_t zr) {
      float zf[8];
      Vec16<T>::unpack(u32x4_t{zr[0], zr[1], 0u, 0u}, zf);
      const f32x4_t bsc = *reinterpret_cast<const f32x4_t*>(tab_o + Cfg::TAB_BSC + a * 16);
      const f32x4_t bsh = *reinterpret_cast<const f32x4_t*>(tab_o + Cfg::TAB_BSH + a * 16);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (!counted || !(fmaf(zf[e], bsc[e], bsh[e]) > 0.f)) f[e] = 0.f;            // pixels outside the map add nothing
        s1[a][e] += f[e];
        s2[a][e] += f[e] * zf[e];
      }
      const u32x2_t pk = round_t(f);
      if ((int32_t)boff >= 0) *reinterpret_cast<u32x2_t*>((char*)p.y + boff) = pk;
    };

    // ---- the row pipeline.  g / z row j lives in queue set j & 3 until it is written to ring slot j & 3; source row m lives in set
    // m & 1 until row 2 m - 1 writes it (ys is a multiple of 8, so the set indices are compile-time in the phase of y)
    RowQ pre[4];
    u32x4_t vq[2], v0, v1;
    const int ss = ys >> 1;
    issue(ys - 1, pre[3]);
    issue(ys, pre[0]);
    issue_v(ss - 1, v0);
    issue_v(ss, v1);
    issue(ys + 1, pre[1]);
    issue(ys + 2, pre[2]);
    issue_v(ss + 1, vq[1]);
    issue_v(ss + 2, vq[0]);
    z_issue(ys + 1, zq[0]);
    write_row(ys - 1, pre[3]);
    issue(ys + 3, pre[3]);
    write_row(ys, pre[0]);
    write_v(ss - 1, v0);
    write_v(ss, v1);
    auto row = [&](int y, auto ph_c) {
      constexpr int PH = decltype(ph_c)::value;            // y & 3
      write_row(y + 1, pre[(PH + 1) & 3]);
      issue(y + 4, pre[PH & 3]);                           // row y + 4 shares the slot of row y, written one iteration ago
      constexpr int ZC = (PH >> 1) & 1;                    // set holding this row pair's z1
      if constexpr ((PH & 1) == 1) {
        constexpr int VS = ((PH + 1) >> 1) & 1;            // set of source row m + 1 = (y + 1) >> 1
        const int m1 = (y + 1) >> 1;
        write_v(m1, vq[VS]);
        issue_v(m1 + 2, vq[VS]);
        z_issue(y + 2, zq[ZC ^ 1]);
      }
      // ---- data gradient of row y: dz rows y - 1 .. y + 1
      f32x4_t acc[TC];
#pragma unroll
      for (int a = 0; a < TC; ++a) acc[a] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int st = 0; st < NSTEP; ++st) {
        const int vrow = y - 1 + fr_r16[st];
        const int addr = fr_r16[st] < 0 ? Cfg::ZERO_OFF : (vrow & 3) * ROWB + fr_off16[st];
        const u32x4_t xf = *reinterpret_cast<const u32x4_t*>(ring + addr);
#pragma unroll
        for (int a = 0; a < TC; ++a) acc[a] = Mma<T>::run(wf[st][a], xf, acc[a]);
      }
      // every MFMA of the row stays in front of every accumulator read of its epilogue (the r03 hazard)
      __builtin_amdgcn_sched_barrier(0);
      const bool y_ok = y < p.H;
#pragma unroll
      for (int a = 0; a < TC; ++a) {
        float f[4] = {acc[a][0], acc[a][1], acc[a][2], acc[a][3]};
        (void)round_t(f);
        // rows pair up inside the strip; the four ROUNDED values are added in the streaming kernel's order:
        // (row 2q, col 2c), (2q, 2c + 1), (2q + 1, 2c), (2q + 1, 2c + 1)
        if constexpr ((PH & 1) == 0) {
#pragma unroll
          for (int e = 0; e < 4; ++e) prev[a][e] = f[e];
        } else {
          float t[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float pn = dpp_f<0xB1>(prev[a][e]), cn = dpp_f<0xB1>(f[e]);      // the odd neighbour column
            t[e] = ((prev[a][e] + pn) + f[e]) + cn;
          }
          (void)round_t(t);
          finish(a, t, y_ok ? out_off(a, y) : kOOB, lane_stores && y_ok, zq[ZC][a]);
        }
      }
      // ---- weight gradient of rows y - 1, y (odd y = 2 m + 1): source rows m - 1, m, m + 1
      if constexpr ((PH & 1) == 1) {
        constexpr int SL = (PH + 3) & 3, SH = PH & 3;       // dz slots of rows y - 1, y
        const u32x2_t zlo = tr(ring + SL * ROWB + lane_z), zhi = tr(ring + SH * ROWB + lane_z);
        const u32x4_t zf = u32x4_t{zlo[0], zlo[1], zhi[0], zhi[1]};
        const int m = y >> 1;
        const char* const Va = vring + ((m - 1) & 3) * VROW + lane_v;
        const char* const Vb = vring + (m & 3) * VROW + lane_v;
        const char* const Vc = vring + ((m + 1) & 3) * VROW + lane_v;
#pragma unroll
        for (int s_ = 0; s_ < 3; ++s_)
#pragma unroll
          for (int b = 0; b < TC; ++b) {
            const u32x2_t va = tr(Va + s_ * VSB + b * 32), vb = tr(Vb + s_ * VSB + b * 32), vc = tr(Vc + s_ * VSB + b * 32);
            wacc[s_][b] = Mma<T>::run(zf, u32x4_t{va[0], va[1], vb[0], vb[1]}, wacc[s_][b]);
            wacc[3 + s_][b] = Mma<T>::run(zf, u32x4_t{vb[0], vb[1], vb[0], vb[1]}, wacc[3 + s_][b]);
            wacc[6 + s_][b] = Mma<T>::run(zf, u32x4_t{vb[0], vb[1], vc[0], vc[1]}, wacc[6 + s_][b]);
          }
      }
    };
    // BN+ReLU-backward sums: as in conv_bwd_onepass_kernel, the fp32 partials cover RSsum rows — the strip of the streaming data
    // gradient — and go to fp64 there
    double* const sp = p.sums + (size_t)(strip % VK_STATS_REPLICAS) * 2 * C;
    auto flush_sums = [&]() {
#pragma unroll
      for (int a = 0; a < TC; ++a)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float u = row16_sum(s1[a][e]), v = row16_sum(s2[a][e]);
          const int ch = a * 16 + kg * 4 + e;
          if (li == 0) {
            atomicAdd(sp + ch, (double)u);
            atomicAdd(sp + C + ch, (double)v);
          }
          s1[a][e] = 0.f; s2[a][e] = 0.f;
        }
    };
    // rows at or beyond H inside the last group of four run on zero rows and store nothing (H is even: a row pair is inside or outside)
    const int RSsum = p.RSsum;                             // a multiple of 8 that divides RS
    for (int yb = ys, left = RSsum; yb < ye; yb += 4) {
      row(yb, std::integral_constant<int, 0>{});
      row(yb + 1, std::integral_constant<int, 1>{});
      row(yb + 2, std::integral_constant<int, 2>{});
      row(yb + 3, std::integral_constant<int, 3>{});
      left -= 4;
      if (left == 0 || yb + 4 >= ye) {
        flush_sums();
        left = RSsum;
      }
    }
  }

  // ---- the four waves add their weight-gradient tiles in wave order; one slab per workgroup
  __syncthreads();                                           // every wave is done with its rings
  float* const red = reinterpret_cast<float*>(smem);
#pragma unroll 1
  for (int phase = 0; phase < 4; ++phase) {
    if (wave == phase) {
#pragma unroll
      for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int b = 0; b < TC; ++b)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float* dst = red + ((kg * 4 + e) * 9 + t) * C + b * 16 + li;
            if (phase > 0) *dst += wacc[t][b][e];
            else *dst = wacc[t][b][e];
          }
    }
    __syncthreads();
  }
  float* const slab = p.slab + (size_t)blockIdx.x * K * 9 * C;
  for (int i = tid; i < K * 9 * C / 4; i += 256) *reinterpret_cast<f32x4_t*>(slab + i * 4) = *reinterpret_cast<const f32x4_t*>(red + i * 4);
}

template <typename T>
static int launch_onepass_up(OnePassParams p, float* dw, size_t slab_bytes, hipStream_t st) {
  using Cfg = OnePassUpCfg;
  // strip height: launch_onepass's rule at two workgroups per CU — the tallest of 32-256 rows that still gives each of the 2,048
  // resident waves a strip.  Measured at bs 32, 512^2 (profiles/onepass_up/strip_height.log): 395 / 326 / 292 / 288 us at 32 / 64 / 128 /
  // 256 rows against 451 us for the three launches.  The fp32 partials of the BN-backward sums span launch_stream's strip.
  // VK_STREAM_RS overrides both (tests / sweeps).
  const char* e_rs = getenv("VK_STREAM_RS");
  const long per_row_block = (long)p.N * ((p.W + 15) / 16);
  int RS = 256;
  if (e_rs) {
    RS = atoi(e_rs);
  } else {
    while (RS > 32 && per_row_block * ((p.H + RS - 1) / RS) < 2048) RS >>= 1;
  }
  RS = (RS + 7) & ~7;
  if (RS < 8) RS = 8;
  int RSsum = RS;
  if (!e_rs) {
    RSsum = stream_strip_rows(p.N, p.H, p.W);
    if (RS < RSsum) RS = RSsum;                            // both are 32 << n: RSsum divides RS
  }
  p.RSsum = RSsum;
  p.RS = RS;
  const long strips = (long)p.N * ((p.H + RS - 1) / RS) * ((p.W + 15) / 16);
  const long nwg = (strips + 3) / 4;
  if ((size_t)nwg * Cfg::K * 9 * Cfg::C * sizeof(float) > slab_bytes) return VK_ERR_UNSUPPORTED;
  const double px = (double)p.N * p.H * p.W;
  const int rc = vkh::launch<conv_bwd_onepass_up_kernel<T>>(dim3((unsigned)nwg), dim3(256), Cfg::SMEM, st, "bwd_onepass_16b_c32up_k16", {},
                                                            2.0 * 2.0 * px * Cfg::K * 9.0 * Cfg::C, 3.0 * px * Cfg::K * 2.0 + 9.0 * Cfg::K * Cfg::C * (2.0 + 4.0), p);
  if (rc != VK_OK) return rc;
  return launch_slab_reduce((size_t)Cfg::K * 9 * Cfg::C / 4, (int)nwg, p.slab, dw, st);
}

}  // namespace vk

extern "C" int vk_conv_bwd_onepass(const vk_conv_desc* d, const void* g, const void* z, const float* coef_abc, const void* w_dgrad, void* y,
                                   const vk_bnr* bnr, float* dw, void* workspace, size_t workspace_bytes, void* stream) {
  VK_CHECK_ARG(d && g && z && coef_abc && w_dgrad && y && bnr && dw, "vk_conv_bwd_onepass: null argument");
  // shapes outside the kernel: before any launch
  if (d->dtype != VK_BF16 && d->dtype != VK_F16) return VK_ERR_UNSUPPORTED;
  if (d->R != 3 || d->S != 3 || d->stride != 1 || d->pad != 1 || d->transposed || d->H != d->Ho || d->W != d->Wo) return VK_ERR_UNSUPPORTED;
  const bool up = d->src0.up != 0;
  if (d->src1.ptr) return VK_ERR_UNSUPPORTED;
  if (up ? (d->src0.C != 32 || d->K != 16 || ((d->H | d->W) & 1)) : (d->src0.C != d->K || (d->K != 16 && d->K != 32))) return VK_ERR_UNSUPPORTED;
  if ((size_t)d->N * d->H * d->W * d->K * 2 >= (1ull << 31)) return VK_ERR_UNSUPPORTED;
  if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15)) return VK_ERR_UNSUPPORTED;
  VK_CHECK_ARG(d->src0.ptr && d->N > 0 && d->H > 0 && d->W > 0, "vk_conv_bwd_onepass: empty descriptor");
  VK_CHECK_ARG((d->src0.scale != nullptr) == (d->src0.shift != nullptr), "vk_conv_bwd_onepass: scale and shift come together");
  VK_CHECK_ARG(bnr->z == d->src0.ptr && !bnr->mask && !bnr->accumulate && bnr->sums && bnr->scale && bnr->shift,
               "vk_conv_bwd_onepass: bnr must describe the layer's own input (z = src0.ptr, scale, shift, sums; no mask, no accumulate)");
  vk::OnePassParams p;
  p.g = g; p.z = z; p.z1 = d->src0.ptr; p.w = w_dgrad; p.y = y;
  p.coef = coef_abc; p.scale = d->src0.scale; p.shift = d->src0.shift; p.relu = d->src0.relu;
  p.bnr_scale = bnr->scale; p.bnr_shift = bnr->shift; p.sums = bnr->sums;
  p.slab = (float*)workspace;
  p.N = d->N; p.H = d->H; p.W = d->W; p.RS = 0;
  p.t_bytes = (uint32_t)((size_t)d->N * d->H * d->W * d->K * 2);
  p.t1_bytes = up ? (uint32_t)((size_t)d->N * (d->H / 2) * (d->W / 2) * d->src0.C * 2) : p.t_bytes;
  p.w_bytes = (uint32_t)((size_t)d->K * 9 * d->src0.C * 2);
  hipStream_t st = (hipStream_t)stream;
  if (up) return d->dtype == VK_BF16 ? vk::launch_onepass_up<vk::bf16_t>(p, dw, workspace_bytes, st) : vk::launch_onepass_up<vk::f16_t>(p, dw, workspace_bytes, st);
  if (d->dtype == VK_BF16)
    return d->K == 16 ? vk::launch_onepass<vk::bf16_t, 16>(p, dw, workspace_bytes, st) : vk::launch_onepass<vk::bf16_t, 32>(p, dw, workspace_bytes, st);
  return d->K == 16 ? vk::launch_onepass<vk::f16_t, 16>(p, dw, workspace_bytes, st) : vk::launch_onepass<vk::f16_t, 32>(p, dw, workspace_bytes, st);
}
