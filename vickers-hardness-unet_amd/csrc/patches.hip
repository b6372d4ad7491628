// Native-resolution patch training on the device: the training-side half of vk.tiling.  The micrographs stay in HBM at
// their own size (uint8 BGR, one ragged store; masks binarised in a second one) and every step cuts n random S x S patches out of them:
//
//   k_patch_rowcount + k_patch_rowscan : once per dataset — rowcum[item][r] = foreground pixels of rows 0..r (int32, integer sums: no
//        atomics, no order to depend on).  One wave per mask row (dword loads, byte compare, popcount), then one workgroup per item
//        scanning its h row counts in place.
//   k_patch_origins : per step, one wave per sample — the k-th foreground pixel of the item in raster order (row: binary search in
//        rowcum; column: ballot / popcount prefix over 64-pixel pieces of that row), minus the drawn offset, clamped per axis
//        (L >= S: into the image; L < S: the image centred in the patch, as PadIfNeeded does).
//   k_patch_crop : per step — 64 x 4 pixel tiles of the patch.  General path: inverse-mapped bilinear (image) / nearest (mask) gather
//        in the SOURCE image, aug_geom's operation order with the zoom inserted; taps outside the image read 0.  Copy path (no
//        rotation, zoom 1): each wave stages the source row of its tile row in LDS with aligned dword loads.  Both paths leave the
//        tile's RGB bytes in LDS at the byte alignment of their destination, and the tile goes out as whole dwords (bytes only at
//        the two ends of a row that is not dword-aligned, S odd).
// The results are the uint8 RGB [n][S][S][3] / mask {0,1} [n][S][S] buffers vk_augment_batch reads.  Arithmetic is float32 with
// contraction off and follows tests/patches_ref.py operation by operation: outputs are bit-identical to it.  Every byte offset is
// 64-bit (the real store is 1.96 GB).
#include <stdlib.h>

#include "vk_common.h"

#pragma clang fp contract(off)

namespace vk {

struct PatchItem {      // = vk_patch_item
  long long img_off, msk_off;
  int h, w;
  long long row_off;
};
static_assert(sizeof(PatchItem) == sizeof(vk_patch_item) && sizeof(PatchItem) == 32, "vk_patch_item layout");

struct PatchParams {    // = vk_patch_params
  int item, k, oy, ox;
  float zoom, cos_a, sin_a;
  int reserved;
};
static_assert(sizeof(PatchParams) == sizeof(vk_patch_params) && sizeof(PatchParams) == 32, "vk_patch_params layout");

// non-zero bytes of a dword
__device__ __forceinline__ int nonzero_bytes(uint32_t v) {
  v |= v >> 4;
  v |= v >> 2;
  v |= v >> 1;
  return __popc(v & 0x01010101u);
}

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// One wave per mask row: bytes up to the first dword boundary and behind the last one are read as bytes, everything between as
// dwords — no load touches a byte outside the row.  grid (ceil(max_h / 4), n_items); rows at or below h leave at once.
__global__ __launch_bounds__(256) void k_patch_rowcount(const PatchItem* __restrict__ items, const uint8_t* __restrict__ masks,
                                                        int* __restrict__ rowcum) {
  const PatchItem it = items[blockIdx.y];
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= it.h) return;
  const uint8_t* p = masks + (size_t)it.msk_off + (size_t)r * it.w;
  const int head = min((int)((4 - ((uintptr_t)p & 3)) & 3), it.w);
  const int ndw = (it.w - head) >> 2, tail = it.w - head - 4 * ndw;
  int c = 0;
  if (lane < head) c += p[lane] != 0;
  const uint32_t* q = (const uint32_t*)(p + head);
  for (int i = lane; i < ndw; i += 64) c += nonzero_bytes(q[i]);
  if (lane < tail) c += p[head + 4 * ndw + lane] != 0;
  c = wave_sum_i(c);
  if (lane == 0) rowcum[(size_t)it.row_off + r] = c;
}

// One workgroup per item: inclusive scan of its h row counts, in place.  Thread t owns rows [t * per, (t + 1) * per).
__global__ __launch_bounds__(256) void k_patch_rowscan(const PatchItem* __restrict__ items, int* __restrict__ rowcum) {
  __shared__ int part[256];
  const PatchItem it = items[blockIdx.x];
  int* rc = rowcum + (size_t)it.row_off;
  const int t = threadIdx.x, per = (it.h + 255) >> 8;
  const int lo = min(t * per, it.h), hi = min(lo + per, it.h);
  int s = 0;
  for (int r = lo; r < hi; ++r) s += rc[r];
  part[t] = s;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    const int v = t >= off ? part[t - off] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int run = part[t] - s;                                   // rows before this thread's
  for (int r = lo; r < hi; ++r) {
    run += rc[r];
    rc[r] = run;
  }
}

__device__ __forceinline__ int clamp_origin(int o, int L, int S) { return L >= S ? min(max(o, 0), L - S) : -((S - L) / 2); }

// One wave per sample; every lane walks the same path, lane 0 writes.
__global__ __launch_bounds__(64) void k_patch_origins(int S, const PatchItem* __restrict__ items, const uint8_t* __restrict__ masks,
                                                      const int* __restrict__ rowcum, const PatchParams* __restrict__ params,
                                                      int* __restrict__ origins) {
  const int n = blockIdx.x, lane = threadIdx.x;
  const PatchParams p = params[n];
  const PatchItem it = items[p.item];
  const int* rc = rowcum + (size_t)it.row_off;
  const int count = rc[it.h - 1];
  int y0 = p.oy, x0 = p.ox;
  if (p.k >= 0 && count > 0) {
    const int k = min(p.k, count - 1);
    int lo = 0, hi = it.h - 1;                             // first row with rowcum[row] > k
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (rc[mid] > k) hi = mid; else lo = mid + 1;
    }
    const int py = lo;
    int rank = k - (py > 0 ? rc[py - 1] : 0), px = 0;      // rank of the pixel among the row's foreground
    const uint8_t* row = masks + (size_t)it.msk_off + (size_t)py * it.w;
    for (int xb = 0; xb < it.w; xb += 64) {
      const int x = xb + lane;
      const bool fg = x < it.w && row[x] != 0;
      const unsigned long long m = __ballot(fg);
      const int cnt = __popcll(m);
      if (rank < cnt) {
        const int before = __popcll(m & ((1ull << lane) - 1ull));
        const unsigned long long hit = __ballot(fg && before == rank);
        px = xb + (hit ? __ffsll((long long)hit) - 1 : 0);
        break;
      }
      rank -= cnt;
    }
    y0 = py - p.oy;
    x0 = px - p.ox;
  }
  if (lane == 0) {
    origins[2 * n] = clamp_origin(y0, it.h, S);
    origins[2 * n + 1] = clamp_origin(x0, it.w, S);
  }
}

constexpr int PT_W = 64, PT_H = 4;
constexpr int PT_OUT_PITCH = 200;       // bytes per LDS row of the outgoing tile: 3 + 192 used, a multiple of 4
constexpr int PT_SRC_DW = 52;           // dwords per LDS row of the staged source row (copy path): 49 used

__global__ __launch_bounds__(256) void k_patch_crop(int S, int force_general, const PatchItem* __restrict__ items,
                                                    const uint8_t* __restrict__ images, const uint8_t* __restrict__ masks,
                                                    const PatchParams* __restrict__ params, const int* __restrict__ origins,
                                                    uint8_t* __restrict__ rgb, uint8_t* __restrict__ mout) {
#pragma clang fp contract(off)
  __shared__ uint32_t out_dw[PT_H][PT_OUT_PITCH / 4];
  __shared__ uint32_t src_dw[PT_H][PT_SRC_DW];
  const int n = blockIdx.z;
  const PatchParams p = params[n];
  const PatchItem it = items[p.item];
  const int y0 = origins[2 * n], x0 = origins[2 * n + 1];
  const uint8_t* img = images + (size_t)it.img_off;
  const uint8_t* msk = masks + (size_t)it.msk_off;
  const int h = it.h, w = it.w;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int xs = blockIdx.x * PT_W, x = xs + tx, y = blockIdx.y * PT_H + ty;
  const int npx = min(PT_W, S - xs);                       // pixels of this tile's rows
  const bool row_in = y < S, in = row_in && x < S;
  // destination of this wave's row: RGB bytes [g, g + 3 * npx), mask bytes at mrow
  uint8_t* g = rgb + (((size_t)n * S + (size_t)min(y, S - 1)) * S + xs) * 3;
  uint8_t* mrow = mout + ((size_t)n * S + (size_t)min(y, S - 1)) * S + xs;
  const int ga = (int)((uintptr_t)g & 3);
  uint8_t* ob = (uint8_t*)out_dw[ty] + ga + 3 * tx;        // this pixel's bytes in the outgoing tile
  int r = 0, gg = 0, b = 0, m = 0;
  const bool copy = !force_general && p.cos_a == 1.f && p.sin_a == 0.f && p.zoom == 1.f;     // uniform over the workgroup
  if (copy) {
    // rows of the window straight from the source: the part of this tile row that lies in the image, as aligned dwords
    const int sy = y0 + y;
    const int xa = max(x0 + xs, 0), xb = min(x0 + xs + npx, w);
    const bool have = row_in && (unsigned)sy < (unsigned)h && xa < xb;
    int sa = 0;
    if (have) {
      const uint8_t* s = img + ((size_t)sy * w + xa) * 3;
      sa = (int)((uintptr_t)s & 3);
      const int ndw = (sa + (xb - xa) * 3 + 3) >> 2;       // <= 49; the store is padded to whole dwords (vk_patch_index checks it)
      if (tx < ndw) src_dw[ty][tx] = ((const uint32_t*)(s - sa))[tx];
    }
    __syncthreads();
    const int sx = x0 + x;
    if (in && have && sx >= xa && sx < xb) {
      const uint8_t* t = (const uint8_t*)src_dw[ty] + sa + 3 * (sx - xa);
      b = t[0]; gg = t[1]; r = t[2];
      m = msk[(size_t)sy * w + sx] != 0;
    }
  } else if (in) {
    const float c = (float)S * 0.5f - 0.5f;
    const float dx = (float)x - c, dy = (float)y - c;
    const float cx = (float)x0 + c, cy = (float)y0 + c;
    const float u = ((p.cos_a * dx - p.sin_a * dy) * p.zoom) + cx;
    const float v = ((p.sin_a * dx + p.cos_a * dy) * p.zoom) + cy;
    const float u0f = floorf(u), v0f = floorf(v);
    const float wx = u - u0f, wy = v - v0f;
    const int u0 = (int)u0f, v0 = (int)v0f;
    float t[4][3];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int yy = v0 + (q >> 1), xx = u0 + (q & 1);
      if ((unsigned)yy < (unsigned)h && (unsigned)xx < (unsigned)w) {
        const uint8_t* s = img + ((size_t)yy * w + xx) * 3;
        t[q][0] = (float)s[0]; t[q][1] = (float)s[1]; t[q][2] = (float)s[2];
      } else {
        t[q][0] = t[q][1] = t[q][2] = 0.f;
      }
    }
    const float w0x = 1.f - wx, w0y = 1.f - wy;
    int val[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float top = t[0][ch] * w0x + t[1][ch] * wx;
      const float bot = t[2][ch] * w0x + t[3][ch] * wx;
      const float f = top * w0y + bot * wy;
      val[ch] = min(max((int)rintf(f), 0), 255);
    }
    b = val[0]; gg = val[1]; r = val[2];
    const int xi = (int)floorf(u + 0.5f), yi = (int)floorf(v + 0.5f);
    if ((unsigned)yi < (unsigned)h && (unsigned)xi < (unsigned)w) m = msk[(size_t)yi * w + xi] != 0;
  }
  if (in) {
    ob[0] = (uint8_t)r; ob[1] = (uint8_t)gg; ob[2] = (uint8_t)b;      // BGR -> RGB
    mrow[tx] = (uint8_t)m;
  }
  __syncthreads();
  if (!row_in) return;
  // dword i of the LDS row is the destination dword at g - ga + 4 * i; whole dwords where all four bytes belong to the row
  const int nb = 3 * npx, ndw = (ga + nb + 3) >> 2;
  if (tx < ndw) {
    const int lo = 4 * tx, hi = lo + 4;
    if (lo >= ga && hi <= ga + nb) {
      ((uint32_t*)(g - ga))[tx] = out_dw[ty][tx];
    } else {
      const uint8_t* ts = (const uint8_t*)out_dw[ty];
      for (int j = max(lo, ga); j < min(hi, ga + nb); ++j) (g - ga)[j] = ts[j];
    }
  }
}

static size_t round4(size_t v) { return (v + 3) & ~(size_t)3; }

}  // namespace vk

using namespace vk;

extern "C" int vk_patch_index(int n_items, const vk_patch_item* items_host, void* items_dev, size_t images_bytes, const uint8_t* masks,
                              size_t masks_bytes, int32_t* rowcum, size_t rowcum_len, void* stream) {
  VK_CHECK_ARG(n_items >= 1 && n_items <= 65535, "vk_patch_index: %d items outside 1..65535", n_items);
  VK_CHECK_ARG(items_host && items_dev && masks && rowcum, "vk_patch_index: null buffer");
  VK_CHECK_ARG(((uintptr_t)masks & 3) == 0 && ((uintptr_t)rowcum & 3) == 0, "vk_patch_index: masks / rowcum not 4-byte aligned");
  int max_h = 0;
  for (int i = 0; i < n_items; ++i) {
    const vk_patch_item& it = items_host[i];
    VK_CHECK_ARG(it.h >= 1 && it.h <= 16384 && it.w >= 1 && it.w <= 16384, "vk_patch_index: item %d: size %dx%d outside 1..16384", i, it.h, it.w);
    VK_CHECK_ARG(it.img_off >= 0 && it.msk_off >= 0 && it.row_off >= 0, "vk_patch_index: item %d: negative offset", i);
    VK_CHECK_ARG((it.img_off & 3) == 0 && (it.msk_off & 3) == 0, "vk_patch_index: item %d: offsets must be multiples of 4", i);
    VK_CHECK_ARG((size_t)it.img_off + round4((size_t)it.h * it.w * 3) <= images_bytes,
                 "vk_patch_index: item %d: the image (padded to whole dwords) ends behind the %zu-byte store", i, images_bytes);
    VK_CHECK_ARG((size_t)it.msk_off + (size_t)it.h * it.w <= masks_bytes, "vk_patch_index: item %d: the mask ends behind the %zu-byte store", i,
                 masks_bytes);
    VK_CHECK_ARG((size_t)it.row_off + (size_t)it.h <= rowcum_len, "vk_patch_index: item %d: its rows end behind the %zu-entry row table", i,
                 rowcum_len);
    max_h = it.h > max_h ? it.h : max_h;
  }
  hipStream_t st = (hipStream_t)stream;
  VK_CHECK_HIP(hipMemcpyAsync(items_dev, items_host, (size_t)n_items * sizeof(vk_patch_item), hipMemcpyHostToDevice, st));
  vkh::ProfScope ps("patch_index", st, 0.0, (double)masks_bytes + 12.0 * (double)rowcum_len);
  hipLaunchKernelGGL(k_patch_rowcount, dim3((max_h + 3) / 4, n_items), dim3(256), 0, st, (const PatchItem*)items_dev, masks, rowcum);
  hipLaunchKernelGGL(k_patch_rowscan, dim3(n_items), dim3(256), 0, st, (const PatchItem*)items_dev, rowcum);
  VK_CHECK_HIP(hipGetLastError());
  return VK_OK;
}

extern "C" int vk_patch_batch(int n, int size, int n_items, const void* items_dev, const uint8_t* images, const uint8_t* masks,
                              const int32_t* rowcum, const vk_patch_params* params_host, void* params_dev, int flags, int32_t* origins,
                              uint8_t* patches_rgb, uint8_t* patches_mask, void* stream) {
  VK_CHECK_ARG(n >= 1 && n <= 65535, "vk_patch_batch: batch %d outside 1..65535", n);
  VK_CHECK_ARG(size >= 1 && size <= 16384, "vk_patch_batch: patch size %d outside 1..16384", size);
  VK_CHECK_ARG(n_items >= 1, "vk_patch_batch: no items");
  VK_CHECK_ARG((flags & ~VK_PATCH_FORCE_GENERAL) == 0, "vk_patch_batch: unknown flags 0x%x", flags);
  VK_CHECK_ARG(items_dev && images && masks && rowcum && params_host && params_dev && origins && patches_rgb && patches_mask,
               "vk_patch_batch: null buffer");
  VK_CHECK_ARG(((uintptr_t)images & 3) == 0, "vk_patch_batch: the image store is not 4-byte aligned");
  for (int i = 0; i < n; ++i) {
    const vk_patch_params& p = params_host[i];
    VK_CHECK_ARG(p.item >= 0 && p.item < n_items, "vk_patch_batch: sample %d: item %d outside 0..%d", i, p.item, n_items - 1);
    VK_CHECK_ARG(p.zoom >= 0.25f && p.zoom <= 4.f, "vk_patch_batch: sample %d: zoom %g outside 0.25..4", i, (double)p.zoom);
    VK_CHECK_ARG(fabsf(p.cos_a * p.cos_a + p.sin_a * p.sin_a - 1.f) < 1e-3f, "vk_patch_batch: sample %d: (cos, sin) not a rotation", i);
    VK_CHECK_ARG(p.oy >= 0 && p.oy <= 16384 && p.ox >= 0 && p.ox <= 16384, "vk_patch_batch: sample %d: offset (%d, %d) outside 0..16384", i, p.oy, p.ox);
  }
  hipStream_t st = (hipStream_t)stream;
  VK_CHECK_HIP(hipMemcpyAsync(params_dev, params_host, (size_t)n * sizeof(vk_patch_params), hipMemcpyHostToDevice, st));
  {
    vkh::ProfScope ps("patch_origins", st, 0.0, (double)n * (sizeof(vk_patch_params) + sizeof(vk_patch_item) + 8.0));
    hipLaunchKernelGGL(k_patch_origins, dim3(n), dim3(64), 0, st, size, (const PatchItem*)items_dev, masks, rowcum, (const PatchParams*)params_dev,
                       origins);
  }
  {
    vkh::ProfScope ps("patch_crop", st, 0.0, (double)n * size * size * 8.0);      // 4 bytes read, 4 written per pixel
    hipLaunchKernelGGL(k_patch_crop, dim3((size + PT_W - 1) / PT_W, (size + PT_H - 1) / PT_H, n), dim3(256), 0, st, size,
                       (flags & VK_PATCH_FORCE_GENERAL) ? 1 : 0, (const PatchItem*)items_dev, images, masks, (const PatchParams*)params_dev,
                       origins, patches_rgb, patches_mask);
  }
  VK_CHECK_HIP(hipGetLastError());
  return VK_OK;
}
