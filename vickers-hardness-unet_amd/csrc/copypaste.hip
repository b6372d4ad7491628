// Instance copy-paste on the device: a compose step between the letterboxed uint8 store and vk_augment_batch.
//
//   k_cp_boxes : once per bank — bounding box and area of every slot of a vk_geom_slot_map result.  A wave owns one row piece of 64
//        pixels, so the lanes of one slot are a ballot: first / last set bit and popcount are that slot's x range and count in the
//        piece (the per-wave reduction).  The wave's leader adds them to the workgroup's table in LDS, and the table goes out with
//        integer min / max / add atomics: no order to depend on.
//   k_cp_alpha : once per bank — kept = (slot >= 0) and the 7 x 7 binomial of kept with a gain of 8, as uint8.  64 x 16 tiles with a
//        3-pixel apron in LDS, rows first, then columns: the 49 taps never come from global memory.
//   k_cp_paste : per step — every output pixel starts as its base pixel and takes the records of its sample in list order: a
//        fixed-point bilinear gather out of the donor box (turned by d4), blended by the donor's alpha; the mask takes the donor's kept
//        bit at the nearest tap.  A wave owns 256 pixels of one row (4 per lane: 12-byte and 4-byte loads and stores where S % 4 == 0),
//        so the test "this record's box misses my pixels" is the same in every lane and a record that misses costs a few scalar
//        compares.  The records of the sample are read into LDS once per workgroup.  No atomics, no workspace: a pixel depends on the
//        stores alone.
// All arithmetic is integer and follows tests/copypaste_ref.py: the outputs are the same bytes.
#include "vk_common.h"

namespace vk {

static_assert(sizeof(vk_cp_rec) == 40, "vk_cp_rec layout");
constexpr int CP_REC_INTS = sizeof(vk_cp_rec) / 4;

// ------------------------------------------------------------------------------------------------ boxes
constexpr int CPB_W = 64, CPB_H = 16;       // tile of one workgroup; a wave owns CPB_H / 4 rows of it

__global__ __launch_bounds__(256) void k_cp_boxes_init(int total, int h, int w, int* __restrict__ boxes) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  int* b = boxes + (size_t)i * 5;
  b[0] = w; b[1] = h; b[2] = -1; b[3] = -1; b[4] = 0;
}

__global__ __launch_bounds__(256) void k_cp_boxes(int h, int w, int max_slots, const int* __restrict__ slots, int* __restrict__ boxes) {
  __shared__ int tab[VK_CP_MAX_SLOTS][5];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (t < max_slots) {
    tab[t][0] = w; tab[t][1] = h; tab[t][2] = -1; tab[t][3] = -1; tab[t][4] = 0;
  }
  __syncthreads();
  const int xs = blockIdx.x * CPB_W, x = xs + lane;
  const int* map = slots + (size_t)blockIdx.z * h * w;
  for (int rr = 0; rr < CPB_H / 4; ++rr) {
    const int y = blockIdx.y * CPB_H + wave * (CPB_H / 4) + rr;            // the same in every lane
    int s = -1;
    if (x < w && y < h) s = map[(size_t)y * w + x];
    bool active = s >= 0 && s < max_slots;
    unsigned long long left = __ballot(active);
    while (left) {
      const int leader = __ffsll((long long)left) - 1;
      const int cs = __shfl(s, leader, 64);
      const bool mine = active && s == cs;
      const unsigned long long bm = __ballot(mine);                        // never empty: the leader is in it
      if (lane == leader) {
        atomicMin(&tab[cs][0], xs + __ffsll((long long)bm) - 1);
        atomicMin(&tab[cs][1], y);
        atomicMax(&tab[cs][2], xs + 63 - __clzll((long long)bm));
        atomicMax(&tab[cs][3], y);
        atomicAdd(&tab[cs][4], __popcll(bm));
      }
      active = active && !mine;
      left &= ~bm;
    }
  }
  __syncthreads();
  if (t < max_slots && tab[t][4] > 0) {
    int* b = boxes + ((size_t)blockIdx.z * max_slots + t) * 5;
    atomicMin(b + 0, tab[t][0]);
    atomicMin(b + 1, tab[t][1]);
    atomicMax(b + 2, tab[t][2]);
    atomicMax(b + 3, tab[t][3]);
    atomicAdd(b + 4, tab[t][4]);
  }
}

// ------------------------------------------------------------------------------------------------ alpha
constexpr int CPA_W = 64, CPA_H = 16, CPA_R = 3;
constexpr int CPA_TW = CPA_W + 2 * CPA_R, CPA_TH = CPA_H + 2 * CPA_R;      // 70 x 22 with the apron
constexpr int CPA_PITCH = 72;

__global__ __launch_bounds__(256) void k_cp_alpha(int h, int w, const int* __restrict__ slots, uint8_t* __restrict__ kept,
                                                  uint8_t* __restrict__ alpha) {
  __shared__ uint8_t kt[CPA_TH][CPA_PITCH];       // kept, with the apron
  __shared__ uint8_t ht[CPA_TH][CPA_W];           // row sums: at most 64
  const int t = threadIdx.x;
  const int xs = blockIdx.x * CPA_W, ys = blockIdx.y * CPA_H;
  const size_t plane = (size_t)blockIdx.z * h * w;
  const int* map = slots + plane;
  for (int e = t; e < CPA_TH * CPA_TW; e += 256) {
    const int ry = e / CPA_TW, rx = e - ry * CPA_TW;
    const int gy = ys + ry - CPA_R, gx = xs + rx - CPA_R;
    int v = 0;
    if ((unsigned)gy < (unsigned)h && (unsigned)gx < (unsigned)w) v = map[(size_t)gy * w + gx] >= 0;
    kt[ry][rx] = (uint8_t)v;
  }
  __syncthreads();
  for (int e = t; e < CPA_TH * CPA_W; e += 256) {
    const int ry = e >> 6, cx = e & 63;
    const uint8_t* r = &kt[ry][cx];
    ht[ry][cx] = (uint8_t)(r[0] + 6 * r[1] + 15 * r[2] + 20 * r[3] + 15 * r[4] + 6 * r[5] + r[6]);
  }
  __syncthreads();
  const int lx = t & 63, gx = xs + lx;
  if (gx >= w) return;
  for (int rr = 0; rr < CPA_H / 4; ++rr) {
    const int ly = (t >> 6) * (CPA_H / 4) + rr, gy = ys + ly;
    if (gy >= h) break;
    const int acc = ht[ly][lx] + 6 * ht[ly + 1][lx] + 15 * ht[ly + 2][lx] + 20 * ht[ly + 3][lx] + 15 * ht[ly + 4][lx] + 6 * ht[ly + 5][lx] +
                    ht[ly + 6][lx];                                       // 0..4096
    const size_t o = plane + (size_t)gy * w + gx;
    kept[o] = kt[ly + CPA_R][lx + CPA_R];
    alpha[o] = (uint8_t)min(255, (acc * 2040 + 2048) >> 12);
  }
}

// ------------------------------------------------------------------------------------------------ paste
constexpr int CP_PX = 4;                    // pixels per lane
constexpr int CP_SEG = 64 * CP_PX;          // pixels per wave: one piece of one row
constexpr int CP_ROWS = 4;                  // waves (rows) per workgroup

// Source coordinate of destination index i on one axis: ((2 i + 1) * t * 256) / (2 d) - 128 clipped to [0, (t - 1) * 256], t the
// source length (<= 4096), d the destination length (<= 8192), 0 <= i < d.  The product passes 2^32, so t * 128 = a * d + r is taken
// apart once per record: floor((2 i + 1) (a d + r) / d) = (2 i + 1) a + floor((2 i + 1) r / d), with (2 i + 1) r < 2^14 * 2^13 and the
// whole below t * 256 <= 2^20.
struct AxisMap {
  uint32_t a, r, d;
  int hi;
};
__device__ __forceinline__ AxisMap axis_map(int t, int d) {
  AxisMap m;
  m.d = (uint32_t)d;
  m.a = (uint32_t)(t * 128) / m.d;
  m.r = (uint32_t)(t * 128) - m.a * m.d;
  m.hi = (t - 1) * 256;
  return m;
}
__device__ __forceinline__ int axis_src(int i, const AxisMap& m) {
  const uint32_t o = 2u * (uint32_t)i + 1u;
  const int q = (int)(o * m.a + (o * m.r) / m.d);
  return min(max(q - 128, 0), m.hi);
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_cp_paste(int S, int n_items, const uint8_t* __restrict__ images, const uint8_t* __restrict__ masks,
                                                  const uint8_t* __restrict__ kept, const uint8_t* __restrict__ alpha,
                                                  const int* __restrict__ base_index, const int* __restrict__ recs,
                                                  const int* __restrict__ counts, uint8_t* __restrict__ out_rgb,
                                                  uint8_t* __restrict__ out_mask) {
  __shared__ int rl[VK_CP_MAX_PASTES * CP_REC_INTS];
  const int n = blockIdx.z, t = threadIdx.x;
  const int cnt = min(max(counts[n], 0), VK_CP_MAX_PASTES);
  if (t < cnt * CP_REC_INTS) rl[t] = recs[(size_t)n * (VK_CP_MAX_PASTES * CP_REC_INTS) + t];
  __syncthreads();
  const int lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int y = blockIdx.y * CP_ROWS + wave, xs = blockIdx.x * CP_SEG;
  const int x = xs + lane * CP_PX;
  if (y >= S || x >= S) return;
  const int item = min(max(base_index[n], 0), n_items - 1);               // a bad index can never leave the stores
  const size_t SS = (size_t)S * S;
  const size_t src = (size_t)item * SS + (size_t)y * S + x, dst = (size_t)n * SS + (size_t)y * S + x;
  const int npx = VEC ? CP_PX : min(CP_PX, S - x);
  int cur[CP_PX][3], m[CP_PX];
  if (VEC) {
    const uint32_t* p = (const uint32_t*)(images + src * 3);
    const uint32_t w0 = p[0], w1 = p[1], w2 = p[2], wm = *(const uint32_t*)(masks + src);
    const uint32_t b[12] = {w0 & 255, (w0 >> 8) & 255, (w0 >> 16) & 255, w0 >> 24, w1 & 255, (w1 >> 8) & 255, (w1 >> 16) & 255, w1 >> 24,
                            w2 & 255, (w2 >> 8) & 255, (w2 >> 16) & 255, w2 >> 24};
#pragma unroll
    for (int q = 0; q < CP_PX; ++q) {
      cur[q][0] = (int)b[3 * q]; cur[q][1] = (int)b[3 * q + 1]; cur[q][2] = (int)b[3 * q + 2];
      m[q] = (int)((wm >> (8 * q)) & 255);
    }
  } else {
#pragma unroll
    for (int q = 0; q < CP_PX; ++q) {
      cur[q][0] = cur[q][1] = cur[q][2] = m[q] = 0;
      if (q < npx) {
        const uint8_t* p = images + (src + q) * 3;
        cur[q][0] = p[0]; cur[q][1] = p[1]; cur[q][2] = p[2];
        m[q] = masks[src + q];
      }
    }
  }
  for (int r = 0; r < cnt; ++r) {
    const int* rc = rl + r * CP_REC_INTS;
    const int dx0 = rc[6], dy0 = rc[7], dw = rc[8], dh = rc[9];
    const int j = y - dy0;
    if (j < 0 || j >= dh || dx0 >= xs + CP_SEG || dx0 + dw <= xs) continue;        // the same in every lane of the wave
    const int donor = rc[0], sx0 = rc[1], sy0 = rc[2], sw = rc[3], sh = rc[4], d4 = rc[5];
    const int k = d4 & 3;
    const int tw = (k & 1) ? sh : sw, th = (k & 1) ? sw : sh;
    // T[ty][tx] = P[cy + ay tx + by ty][cx + ax tx + bx ty]: numpy's rot90 by k quarter turns, after the mirror when d4 & 4
    int ax = (k == 0) - (k == 2), bx = (k == 3) - (k == 1), cx = (k == 1 || k == 2) ? sw - 1 : 0;
    const int ay = (k == 1) - (k == 3), by = (k == 0) - (k == 2), cy = (k == 2 || k == 3) ? sh - 1 : 0;
    if (d4 & 4) { ax = -ax; bx = -bx; cx = sw - 1 - cx; }
    const int o0 = (sy0 + cy) * S + sx0 + cx, dX = ay * S + ax, dY = by * S + bx;
    const AxisMap mu = axis_map(tw, dw), mv = axis_map(th, dh);
    const int V = axis_src(j, mv);
    const int y0 = V >> 8, fy = V & 255, y1 = min(y0 + 1, th - 1), ky = min((V + 128) >> 8, th - 1);
    const size_t dbase = (size_t)donor * SS;
    const uint8_t* dimg = images + dbase * 3;
    const uint8_t* dal = alpha + dbase;
    const uint8_t* dkp = kept + dbase;
    const int r0 = o0 + y0 * dY, r1 = o0 + y1 * dY, rk = o0 + ky * dY;
#pragma unroll
    for (int q = 0; q < CP_PX; ++q) {
      const int i = x + q - dx0;
      if (q >= npx || i < 0 || i >= dw) continue;
      const int U = axis_src(i, mu);
      const int x0 = U >> 8, fx = U & 255, x1 = min(x0 + 1, tw - 1), kx = min((U + 128) >> 8, tw - 1);
      const int o00 = r0 + x0 * dX, o01 = r0 + x1 * dX, o10 = r1 + x0 * dX, o11 = r1 + x1 * dX;
      const int gx = 256 - fx, gy = 256 - fy;
      const int a = ((dal[o00] * gx + dal[o01] * fx) * gy + (dal[o10] * gx + dal[o11] * fx) * fy + 32768) >> 16;
      m[q] |= dkp[rk + kx * dX];
      if (a == 0) continue;                 // (0 val + 255 cur + 127) / 255 = cur: the margin and the corners of a box cost no colour taps
      const uint8_t *p00 = dimg + (size_t)o00 * 3, *p01 = dimg + (size_t)o01 * 3, *p10 = dimg + (size_t)o10 * 3, *p11 = dimg + (size_t)o11 * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int val = ((p00[c] * gx + p01[c] * fx) * gy + (p10[c] * gx + p11[c] * fx) * fy + 32768) >> 16;
        cur[q][c] = (a * val + (255 - a) * cur[q][c] + 127) / 255;
      }
    }
  }
  if (VEC) {
    uint32_t b[12];
#pragma unroll
    for (int q = 0; q < CP_PX; ++q) {
      b[3 * q] = (uint32_t)cur[q][0]; b[3 * q + 1] = (uint32_t)cur[q][1]; b[3 * q + 2] = (uint32_t)cur[q][2];
    }
    uint32_t* o = (uint32_t*)(out_rgb + dst * 3);
    o[0] = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
    o[1] = b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24);
    o[2] = b[8] | (b[9] << 8) | (b[10] << 16) | (b[11] << 24);
    *(uint32_t*)(out_mask + dst) = (uint32_t)m[0] | ((uint32_t)m[1] << 8) | ((uint32_t)m[2] << 16) | ((uint32_t)m[3] << 24);
  } else {
#pragma unroll
    for (int q = 0; q < CP_PX; ++q) {
      if (q < npx) {
        uint8_t* o = out_rgb + (dst + q) * 3;
        o[0] = (uint8_t)cur[q][0]; o[1] = (uint8_t)cur[q][1]; o[2] = (uint8_t)cur[q][2];
        out_mask[dst + q] = (uint8_t)m[q];
      }
    }
  }
}

static bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }

static int check_maps(const char* who, int batch, int h, int w) {
  VK_CHECK_ARG(batch >= 1 && batch <= 65535, "%s: batch %d outside 1..65535", who, batch);
  VK_CHECK_ARG(h >= 1 && h <= 16384 && w >= 1 && w <= 16384, "%s: map size %d x %d outside 1..16384", who, h, w);
  return VK_OK;
}

}  // namespace vk

using namespace vk;

extern "C" int vk_cp_boxes(int batch, int h, int w, const int32_t* slots, int max_slots, int32_t* boxes, void* stream) {
  int rc = check_maps("vk_cp_boxes", batch, h, w);
  if (rc != VK_OK) return rc;
  VK_CHECK_ARG(max_slots >= 1 && max_slots <= VK_CP_MAX_SLOTS, "vk_cp_boxes: max_slots %d outside 1..%d", max_slots, VK_CP_MAX_SLOTS);
  VK_CHECK_ARG(slots && boxes, "vk_cp_boxes: null buffer");
  VK_CHECK_ARG(aligned4(slots) && aligned4(boxes), "vk_cp_boxes: misaligned buffer");
  hipStream_t st = (hipStream_t)stream;
  const int total = batch * max_slots;
  vkh::ProfScope ps("cp_boxes", st, 0.0, (double)batch * h * w * 4.0 + (double)total * 20.0);
  hipLaunchKernelGGL(k_cp_boxes_init, dim3((total + 255) / 256), dim3(256), 0, st, total, h, w, boxes);
  hipLaunchKernelGGL(k_cp_boxes, dim3((w + CPB_W - 1) / CPB_W, (h + CPB_H - 1) / CPB_H, batch), dim3(256), 0, st, h, w, max_slots, slots, boxes);
  VK_CHECK_HIP(hipGetLastError());
  return VK_OK;
}

extern "C" int vk_cp_alpha(int batch, int h, int w, const int32_t* slots, uint8_t* kept, uint8_t* alpha, void* stream) {
  int rc = check_maps("vk_cp_alpha", batch, h, w);
  if (rc != VK_OK) return rc;
  VK_CHECK_ARG(slots && kept && alpha, "vk_cp_alpha: null buffer");
  VK_CHECK_ARG(aligned4(slots), "vk_cp_alpha: misaligned buffer");
  hipStream_t st = (hipStream_t)stream;
  vkh::ProfScope ps("cp_alpha", st, 0.0, (double)batch * h * w * 6.0);
  hipLaunchKernelGGL(k_cp_alpha, dim3((w + CPA_W - 1) / CPA_W, (h + CPA_H - 1) / CPA_H, batch), dim3(256), 0, st, h, w, slots, kept, alpha);
  VK_CHECK_HIP(hipGetLastError());
  return VK_OK;
}

extern "C" int vk_cp_paste(int n, int S, int n_items, const uint8_t* images_rgb, const uint8_t* masks, const uint8_t* kept,
                           const uint8_t* alpha, const int32_t* base_index_dev, const int32_t* counts_host, const vk_cp_rec* recs_host,
                           void* recs_dev, uint8_t* out_rgb, uint8_t* out_mask, void* stream) {
  VK_CHECK_ARG(n >= 1 && n <= 65535, "vk_cp_paste: batch %d outside 1..65535", n);
  VK_CHECK_ARG(S >= 1 && S <= VK_CP_MAX_SIDE, "vk_cp_paste: S = %d outside 1..%d", S, VK_CP_MAX_SIDE);
  VK_CHECK_ARG(n_items >= 1, "vk_cp_paste: no items");
  VK_CHECK_ARG(images_rgb && masks && kept && alpha && base_index_dev && counts_host && recs_host && recs_dev && out_rgb && out_mask,
               "vk_cp_paste: null buffer");
  VK_CHECK_ARG(aligned4(images_rgb) && aligned4(masks) && aligned4(kept) && aligned4(alpha) && aligned4(base_index_dev) && aligned4(recs_dev) &&
                   aligned4(out_rgb) && aligned4(out_mask) && aligned4(counts_host) && aligned4(recs_host),
               "vk_cp_paste: misaligned buffer");
  double donor_bytes = 0.0;
  for (int k = 0; k < n; ++k) {
    const int c = counts_host[k];
    VK_CHECK_ARG(c >= 0 && c <= VK_CP_MAX_PASTES, "vk_cp_paste: sample %d: count %d outside 0..%d", k, c, VK_CP_MAX_PASTES);
    for (int r = 0; r < c; ++r) {
      const vk_cp_rec& q = recs_host[(size_t)k * VK_CP_MAX_PASTES + r];
      VK_CHECK_ARG(q.donor >= 0 && q.donor < n_items, "vk_cp_paste: sample %d record %d: donor %d outside 0..%d", k, r, q.donor, n_items - 1);
      VK_CHECK_ARG(q.sw >= 1 && q.sh >= 1 && q.sx0 >= 0 && q.sy0 >= 0 && q.sx0 <= S - q.sw && q.sy0 <= S - q.sh,
                   "vk_cp_paste: sample %d record %d: donor box %d x %d at (%d, %d) not inside the %d-pixel image", k, r, q.sw, q.sh, q.sx0,
                   q.sy0, S);
      VK_CHECK_ARG(q.d4 >= 0 && q.d4 <= 7, "vk_cp_paste: sample %d record %d: d4 %d outside 0..7", k, r, q.d4);
      VK_CHECK_ARG(q.dw >= 1 && q.dw <= 2 * S && q.dh >= 1 && q.dh <= 2 * S, "vk_cp_paste: sample %d record %d: destination size %d x %d outside 1..%d",
                   k, r, q.dw, q.dh, 2 * S);
      VK_CHECK_ARG(q.dx0 >= -2 * S && q.dx0 <= 2 * S && q.dy0 >= -2 * S && q.dy0 <= 2 * S,
                   "vk_cp_paste: sample %d record %d: destination origin (%d, %d) outside +-%d", k, r, q.dx0, q.dy0, 2 * S);
      donor_bytes += 5.0 * q.sw * q.sh;
    }
  }
  hipStream_t st = (hipStream_t)stream;
  const size_t rec_bytes = (size_t)n * VK_CP_MAX_PASTES * sizeof(vk_cp_rec);
  VK_CHECK_HIP(hipMemcpyAsync(recs_dev, recs_host, rec_bytes, hipMemcpyHostToDevice, st));
  VK_CHECK_HIP(hipMemcpyAsync((char*)recs_dev + rec_bytes, counts_host, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, st));
  vkh::ProfScope ps("cp_paste", st, 0.0, (double)n * S * S * 8.0 + donor_bytes);            // 4 bytes read, 4 written per pixel
  const dim3 grid((S + CP_SEG - 1) / CP_SEG, (S + CP_ROWS - 1) / CP_ROWS, n);
  const int* rd = (const int*)recs_dev;
  const int* cd = (const int*)((const char*)recs_dev + rec_bytes);
  if (S % 4 == 0)
    hipLaunchKernelGGL(k_cp_paste<true>, grid, dim3(256), 0, st, S, n_items, images_rgb, masks, kept, alpha, base_index_dev, rd, cd, out_rgb, out_mask);
  else
    hipLaunchKernelGGL(k_cp_paste<false>, grid, dim3(256), 0, st, S, n_items, images_rgb, masks, kept, alpha, base_index_dev, rd, cd, out_rgb,
                       out_mask);
  VK_CHECK_HIP(hipGetLastError());
  return VK_OK;
}
