// Vertex heatmaps: vk_kp_targets, vk_kp_peaks, vk_kp_refine.
//
//   k_kp_targets : vertex records -> a float32 heatmap.  A workgroup (256 lanes) owns 64 x 16 tiles of one map, a lane four pixels of a
//        row.  Per round every lane reads one vertex (256 per round, ascending (slot, q)), converts it to 1/16-pixel fixed point and
//        tests its disc against the tile's rectangle; the hits are compacted with a ballot per wave into a list in LDS, relative to
//        the tile's origin, so everything after it is int32.  Then every lane walks the list (broadcast LDS reads): a vertex whose
//        rows cannot reach the wave's four rows is skipped on wave-uniform values, the others cost two subtractions per pixel and a
//        table read where D < table_len.  More vertices than a round holds (4 x max_components > 256) are further rounds.  The result
//        is a maximum over table values above 0.0f, which does not depend on the order.  Stores: one 16-byte store per lane where
//        base, stride and width allow it, four 4-byte stores otherwise; the values are the same registers.
//        The table is read from memory (the default: 15.1 us against 28.1 us for 32 maps of 512 x 512 at sigma 2, where staging 36.9 KB
//        per 4 KB tile loses) or staged in LDS (VK_KP_TABLE_LDS, up to VK_KP_TABLE_LDS_MAX entries); profiles/keypoints/README.md.
//   k_kp_mark / k_kp_scan / k_kp_emit : heatmap -> the list of its local maxima in raster order, without atomics.  A workgroup owns
//        1,024 consecutive raster pixels, a lane four of them.  mark: tests p >= min_peak first (almost every pixel of a heatmap
//        fails it), then the window; leaves a 4-bit mask per lane and a count per workgroup in the workspace.  scan: one workgroup
//        per map, the exclusive prefix of the counts (a running carry over chunks of 256) and counts[b].  emit: the ordered prefix
//        inside the workgroup (wave scan, then the waves' totals) and the records below max_peaks.
//   k_kp_refine  : one workgroup per (map, slot), wave k refines vertex k.  The lanes stride over the search window, each keeping its
//        best (value, raster index); the wave's best is the maximum under the total order (larger value, then smaller index), so
//        the shuffle tree's shape changes no bit.  The parabola and the centroid are evaluated by every lane on broadcast loads;
//        the centroid's sums are one sequential loop.  The record tail is subpix_tail.h, shared with vk_subpix_refine.
//
// No transcendental and no float atomic runs on the device.  Float64 with contraction off where include/vk_unet.h states it.  Every
// index into a map is formed from coordinates clipped to it; every table index is below table_len; slots are below max_components.
#include "vk_common.h"
#include "subpix_tail.h"

#include <math.h>

#pragma clang fp contract(off)

namespace vk {

static_assert(sizeof(vk_kp_peak) == 16 && sizeof(vk_kp_params) == 32, "vk_kp_peak / vk_kp_params layout");
constexpr int KP_TW = 64, KP_TH = 16;                        // the tile of k_kp_targets
constexpr int KP_LIST = 256;                                 // vertices per round: one per lane
constexpr int KP_CHUNK = 1024;                               // raster pixels per workgroup of the peak kernels

// ------------------------------------------------------------------------------------------------ targets
template <bool VEC, bool TAB_LDS>
__global__ __launch_bounds__(256) void k_kp_targets(int h, int w, int tiles_x, int64_t ntiles, const char* __restrict__ recs, size_t stride,
                                                    size_t vert_off, int vert_type, int valid_off, const int32_t* __restrict__ counts, int M,
                                                    const float* __restrict__ table, int table_len, int R16, float* __restrict__ out,
                                                    size_t image_stride) {
#pragma clang fp contract(off)
  extern __shared__ float s_table[];                        // TAB_LDS: table_len floats
  __shared__ int s_x[KP_LIST], s_y[KP_LIST];
  __shared__ int s_wcnt[4];
  const int b = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int cnt = counts[b];
  const int used = cnt < 0 ? 0 : (cnt > M ? M : cnt);
  const int nv = 4 * used;
  const float* tab = table;
  if (TAB_LDS) {
    for (int e = t; e < table_len; e += 256) s_table[e] = table[e];
    tab = s_table;                                           // published by the first barrier of the first round; not read without one
  }
  const char* base = recs + (size_t)b * M * stride;
  float* img = out + (size_t)b * image_stride;
  const int ly = t >> 4, lx = (t & 15) * 4;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int ty = (int)(tile / tiles_x), tx = (int)(tile - (int64_t)ty * tiles_x);
    const int xs = tx * KP_TW, ys = ty * KP_TH;
    const int64_t X0 = 16 * (int64_t)xs, Y0 = 16 * (int64_t)ys;
    const int x_hi = 16 * (min(xs + KP_TW, w) - 1 - xs), y_hi = 16 * (min(ys + KP_TH, h) - 1 - ys);      // the tile's last pixel, relative
    float best[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int r0 = 0; r0 < nv; r0 += KP_LIST) {
      // one vertex per lane
      const int e = r0 + t;
      bool hit = false;
      int rx = 0, ry = 0;
      if (e < nv) {
        const char* rec = base + (size_t)(e >> 2) * stride;
        const int q = e & 3;
        bool ok = valid_off < 0 || *reinterpret_cast<const int*>(rec + valid_off) != 0;
        int64_t X = 0, Y = 0;
        if (vert_type == VK_KP_VERT_I32) {
          const int* p = reinterpret_cast<const int*>(rec + vert_off);
          X = 16 * (int64_t)p[2 * q];
          Y = 16 * (int64_t)p[2 * q + 1];
        } else {
          const double* p = reinterpret_cast<const double*>(rec + vert_off);
          const double vx = p[2 * q], vy = p[2 * q + 1];
          if (fabs(vx) <= 1048576.0 && fabs(vy) <= 1048576.0) {            // a NaN fails
            X = (int64_t)floor(vx * 16.0 + 0.5);
            Y = (int64_t)floor(vy * 16.0 + 0.5);
          } else {
            ok = false;
          }
        }
        const int64_t RX = X - X0, RY = Y - Y0;                              // |.| < 2^36: no overflow
        if (ok) {
          const int64_t gx = RX < 0 ? -RX : (RX > x_hi ? RX - x_hi : 0), gy = RY < 0 ? -RY : (RY > y_hi ? RY - y_hi : 0);
          if (gx <= R16 && gy <= R16 && gx * gx + gy * gy < table_len) {          // the squares only of values up to 192
            hit = true;
            rx = (int)RX;                                                      // within R16 of the tile: |.| <= 16 * 63 + 192
            ry = (int)RY;
          }
        }
      }
      const unsigned long long bm = __ballot(hit);
      if (lane == 0) s_wcnt[wave] = __popcll(bm);
      __syncthreads();                                                         // also: the list of the round before has been read
      int off = 0, total = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int c = s_wcnt[k];
        if (k < wave) off += c;
        total += c;
      }
      if (hit) {
        const int pos = off + __popcll(bm & ((1ull << lane) - 1ull));
        s_x[pos] = rx;
        s_y[pos] = ry;
      }
      __syncthreads();
      const int py = 16 * ly;
      const int wy0 = 16 * (4 * wave), wy1 = 16 * (4 * wave + 3);              // the wave's rows
      for (int j = 0; j < total; ++j) {
        const int vx = __builtin_amdgcn_readfirstlane(s_x[j]), vy = __builtin_amdgcn_readfirstlane(s_y[j]);
        if (vy < wy0 - R16 || vy > wy1 + R16) continue;                        // wave-uniform: a scalar branch
        const int dy = py - vy;
        if (dy < -R16 || dy > R16) continue;
        const int dy2 = dy * dy;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int dx = 16 * (lx + q) - vx;
          const int D = dx * dx + dy2;                                         // |dx| <= 16 * 63 + 192, |dy| <= 192: below 2^21
          if (D < table_len) {
            const float v = tab[D];
            if (v > best[q]) best[q] = v;
          }
        }
      }
      __syncthreads();                                                         // s_wcnt and the list are written again
    }
    const int gy = ys + ly, gx = xs + lx;
    if (gy < h && gx < w) {
      float* o = img + (size_t)gy * w + gx;
      if (VEC) {
        f32x4_t v4 = {best[0], best[1], best[2], best[3]};
        *reinterpret_cast<f32x4_t*>(o) = v4;
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (gx + q < w) o[q] = best[q];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ peaks
// the rule of include/vk_unet.h for pixel idx of one map; a NaN is no peak and suppresses none
__device__ __forceinline__ bool kp_is_peak(const float* __restrict__ m, int h, int w, int64_t idx, double min_peak, int r) {
  const float p = m[idx];
  if (!((double)p >= min_peak)) return false;
  const int y = (int)(idx / w), x = (int)(idx - (int64_t)y * w);
  const int y0 = max(y - r, 0), y1 = min(y + r, h - 1), x0 = max(x - r, 0), x1 = min(x + r, w - 1);
  for (int j = y0; j <= y1; ++j) {
    const float* row = m + (size_t)j * w;
    for (int i = x0; i <= x1; ++i) {
      const float q = row[i];
      if (q > p) return false;
      if (q == p && (j < y || (j == y && i < x))) return false;
    }
  }
  return true;
}

__global__ __launch_bounds__(256) void k_kp_mark(int h, int w, int nb, const float* __restrict__ heat, size_t image_stride, double min_peak, int r,
                                                 int32_t* __restrict__ blk_cnt, uint8_t* __restrict__ masks) {
  __shared__ int s_w[4];
  const int j = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
  const float* m = heat + (size_t)b * image_stride;
  const int64_t n = (int64_t)h * w, first = (int64_t)j * KP_CHUNK + 4 * t;
  int mask = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q)
    if (first + q < n && kp_is_peak(m, h, w, first + q, min_peak, r)) mask |= 1 << q;
  masks[((size_t)b * nb + j) * 256 + t] = (uint8_t)mask;
  int c = __popc(mask);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((t & 63) == 0) s_w[t >> 6] = c;
  __syncthreads();
  if (t == 0) blk_cnt[(size_t)b * nb + j] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// in place: blk[b][j] becomes the number of peaks before workgroup j; counts[b] the number of all
__global__ __launch_bounds__(256) void k_kp_scan(int nb, int32_t* __restrict__ blk, int32_t* __restrict__ counts) {
  __shared__ int s[256];
  const int b = blockIdx.x, t = threadIdx.x;
  int32_t* a = blk + (size_t)b * nb;
  int carry = 0;
  for (int base = 0; base < nb; base += 256) {
    const int v = base + t < nb ? a[base + t] : 0;
    s[t] = v;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
      const int add = t >= o ? s[t - o] : 0;
      __syncthreads();
      s[t] += add;
      __syncthreads();
    }
    if (base + t < nb) a[base + t] = carry + s[t] - v;
    carry += s[255];
    __syncthreads();
  }
  if (t == 0) counts[b] = carry;
}

__global__ __launch_bounds__(256) void k_kp_emit(int w, int nb, const float* __restrict__ heat, size_t image_stride, int max_peaks,
                                                 const int32_t* __restrict__ blk_off, const uint8_t* __restrict__ masks,
                                                 vk_kp_peak* __restrict__ out) {
  __shared__ int s_w[4];
  const int j = blockIdx.x, b = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int mask = masks[((size_t)b * nb + j) * 256 + t];
  const int c = __popc(mask);
  int inc = c;                                                // inclusive prefix inside the wave
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(inc, o, 64);
    if (lane >= o) inc += u;
  }
  if (lane == 63) s_w[wave] = inc;
  __syncthreads();
  int pos = blk_off[(size_t)b * nb + j] + inc - c;
  for (int k = 0; k < wave; ++k) pos += s_w[k];
  if (mask == 0) return;
  const float* m = heat + (size_t)b * image_stride;
  const int64_t first = (int64_t)j * KP_CHUNK + 4 * t;
#pragma unroll
  for (int q = 0; q < 4; ++q)
    if (mask & (1 << q)) {
      if (pos < max_peaks) {                                   // pos >= 0: a sum of counts
        const int64_t idx = first + q;                        // below h * w: mark set the bit
        const int y = (int)(idx / w);
        vk_kp_peak rec;
        rec.x = (int)(idx - (int64_t)y * w);
        rec.y = y;
        rec.value = m[idx];
        rec.reserved = 0;
        out[(size_t)b * max_peaks + pos] = rec;
      }
      ++pos;
    }
}

// ------------------------------------------------------------------------------------------------ refine
struct KpBest {
  float v;
  int idx;                                                    // raster index inside the clipped window; -1: none yet
};
__device__ __forceinline__ bool kp_better(float v, int idx, const KpBest& o) {
  if (idx < 0) return false;
  if (o.idx < 0) return true;
  return v > o.v || (v == o.v && idx < o.idx);
}

__global__ __launch_bounds__(256) void k_kp_refine(const vk_kp_params P, int h, int w, const float* __restrict__ heat, size_t image_stride,
                                                   const char* __restrict__ recs, size_t stride, size_t box_off, int valid_off,
                                                   const int32_t* __restrict__ counts, int M, const double* __restrict__ affine,
                                                   vk_subpix_quad* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double s_vx[4], s_vy[4];
  __shared__ int s_fl[4], s_it[4], s_px[4], s_py[4];
  const int slot = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cnt = counts[b];
  const int used = cnt < 0 ? 0 : (cnt > M ? M : cnt);
  if (slot >= used) return;                                    // the whole workgroup, before any barrier
  const char* rec = recs + ((size_t)b * M + slot) * stride;
  const int* box = reinterpret_cast<const int*>(rec + box_off);
  const int valid = valid_off >= 0 ? (*reinterpret_cast<const int*>(rec + valid_off) != 0 ? 1 : 0) : 1;
  vk_subpix_quad* dst = out + (size_t)b * M + slot;
  if (!valid) {
    if (tid == 0) sp_write_invalid(dst, rec);
    return;
  }
  const float* map = heat + (size_t)b * image_stride;
  const int sx = box[2 * wave], sy = box[2 * wave + 1];
  const int S = P.search;
  // the search window clipped to the map, in int64: a corner may be any int32
  const int64_t lx0 = (int64_t)sx - S, lx1 = (int64_t)sx + S, ly0 = (int64_t)sy - S, ly1 = (int64_t)sy + S;
  const int x0 = (int)(lx0 < 0 ? 0 : lx0), y0 = (int)(ly0 < 0 ? 0 : ly0);
  const int x1 = (int)(lx1 > w - 1 ? w - 1 : lx1), y1 = (int)(ly1 > h - 1 ? h - 1 : ly1);
  KpBest best{0.0f, -1};
  int ww = 0;
  if (lx0 <= w - 1 && lx1 >= 0 && ly0 <= h - 1 && ly1 >= 0) {    // wave-uniform: some pixel is inside
    ww = x1 - x0 + 1;
    const int n = ww * (y1 - y0 + 1);                          // at most 63 * 63
    for (int e = lane; e < n; e += 64) {
      const int j = e / ww, i = e - j * ww;
      const float p = map[(size_t)(y0 + j) * w + (x0 + i)];
      if (p == p && kp_better(p, e, best)) { best.v = p; best.idx = e; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(best.v, o, 64);
      const int oi = __shfl_xor(best.idx, o, 64);
      if (kp_better(ov, oi, best)) { best.v = ov; best.idx = oi; }
    }
  }
  double qx = (double)sx, qy = (double)sy;
  int flags = 0, iters = 0, px = -1, py = -1;
  if (best.idx < 0 || (double)best.v < P.min_peak) {
    flags = VK_KP_NO_PEAK;
  } else {
    py = y0 + best.idx / ww;
    px = x0 + best.idx % ww;
    iters = 1;
    if (px == lx0 || px == lx1 || py == ly0 || py == ly1) flags |= VK_KP_AT_EDGE;
    const double c = (double)best.v;
    if (P.method == VK_KP_PARABOLA) {
      double ox = 0.0, oy = 0.0;
      if (px > 0 && px < w - 1) {
        const double l = (double)map[(size_t)py * w + (px - 1)], r = (double)map[(size_t)py * w + (px + 1)];
        const double den = (l - c) + (r - c);
        if (den < 0.0) ox = 0.5 * (l - r) / den;
      }
      if (py > 0 && py < h - 1) {
        const double l = (double)map[(size_t)(py - 1) * w + px], r = (double)map[(size_t)(py + 1) * w + px];
        const double den = (l - c) + (r - c);
        if (den < 0.0) oy = 0.5 * (l - r) / den;
      }
      qx = (double)px + ox;
      qy = (double)py + oy;
    } else {
      const double fl = P.floor_frac * c;
      const int cw = P.cwin;
      const int cx0 = max(px - cw, 0), cx1 = min(px + cw, w - 1), cy0 = max(py - cw, 0), cy1 = min(py + cw, h - 1);
      double sw = 0.0, sxx = 0.0, syy = 0.0;
      for (int j = cy0; j <= cy1; ++j)
        for (int i = cx0; i <= cx1; ++i) {
          const double d = (double)map[(size_t)j * w + i] - fl;
          const double g = d > 0.0 ? d : 0.0;                  // a NaN gives 0
          sw = sw + g;
          sxx = sxx + g * (double)(i - px);
          syy = syy + g * (double)(j - py);
        }
      qx = (double)px;
      qy = (double)py;
      if (sw > 0.0) {                                          // no weight at all: the peak pixel itself
        qx = (double)px + sxx / sw;
        qy = (double)py + syy / sw;
      }
    }
  }
  if (lane == 0) { s_vx[wave] = qx; s_vy[wave] = qy; s_fl[wave] = flags; s_it[wave] = iters; s_px[wave] = px; s_py[wave] = py; }
  __syncthreads();
  if (tid != 0) return;
  // two vertices on one peak pixel: neither is believed
  int shared = 0;
  for (int a = 0; a < 4; ++a)
    for (int c = a + 1; c < 4; ++c)
      if (s_it[a] && s_it[c] && s_px[a] == s_px[c] && s_py[a] == s_py[c]) shared |= (1 << a) | (1 << c);
  for (int q = 0; q < 4; ++q)
    if (shared & (1 << q)) {
      s_fl[q] |= VK_KP_SHARED;
      s_it[q] = 0;
      s_vx[q] = (double)box[2 * q];
      s_vy[q] = (double)box[2 * q + 1];
    }
  sp_write_record(dst, rec, affine, b, s_vx, s_vy, s_fl, s_it);
}

// ------------------------------------------------------------------------------------------------ host checks
static int kp_check_maps(const char* fn, int batch, int h, int w, size_t image_stride) {
  VK_CHECK_ARG(batch >= 1 && batch <= 65535, "%s: batch %d outside 1..65535", fn, batch);
  VK_CHECK_ARG(h >= 1 && w >= 1, "%s: map size %dx%d", fn, h, w);
  VK_CHECK_ARG((size_t)h * (size_t)w <= ((size_t)1 << 30), "%s: more than 2^30 pixels per map", fn);
  VK_CHECK_ARG(image_stride >= (size_t)h * (size_t)w && image_stride <= ((size_t)1 << 40), "%s: image stride %zu below h * w = %zu (or above 2^40)",
               fn, image_stride, (size_t)h * (size_t)w);
  return VK_OK;
}

static int kp_root(int table_len) {                            // R16 with table_len == R16^2 + 1, or 0
  for (int r = 1; r <= VK_KP_MAX_RADIUS16; ++r)
    if (r * r + 1 == table_len) return r;
  return 0;
}

}  // namespace vk

using namespace vk;

extern "C" int vk_kp_targets(int batch, int h, int w, const void* records, size_t record_stride, size_t vert_offset, int vert_type,
                             int valid_offset, const int32_t* counts, int max_components, const float* table, int table_len, float* out,
                             size_t image_stride, int flags, void* stream) {
  const char* fn = "vk_kp_targets";
  const int rc = kp_check_maps(fn, batch, h, w, image_stride);
  if (rc != VK_OK) return rc;
  VK_CHECK_ARG(max_components >= 1 && max_components <= 4096, "vk_kp_targets: max_components = %d outside 1..4096", max_components);
  VK_CHECK_ARG(records && counts && table && out, "vk_kp_targets: null buffer");
  VK_CHECK_ARG(vert_type == VK_KP_VERT_I32 || vert_type == VK_KP_VERT_F64, "vk_kp_targets: vertex type %d is neither int32 nor float64", vert_type);
  const size_t va = vert_type == VK_KP_VERT_F64 ? 8 : 4, vbytes = 8 * va;
  VK_CHECK_ARG(record_stride % va == 0 && vert_offset % va == 0 && record_stride <= ((size_t)1 << 20) && vert_offset <= record_stride &&
                   vert_offset + vbytes <= record_stride,
               "vk_kp_targets: record stride %zu / vertex offset %zu: multiples of %zu with the eight coordinates inside the record", record_stride,
               vert_offset, va);
  VK_CHECK_ARG(valid_offset == -1 || (valid_offset >= 0 && valid_offset % 4 == 0 && (size_t)valid_offset + 4 <= record_stride),
               "vk_kp_targets: valid offset %d is neither -1 nor an int inside the record", valid_offset);
  const int R16 = kp_root(table_len);
  VK_CHECK_ARG(R16 >= 1, "vk_kp_targets: table_len = %d is not R16 * R16 + 1 with R16 in 1..%d", table_len, VK_KP_MAX_RADIUS16);
  VK_CHECK_ARG(flags == 0 || flags == VK_KP_TABLE_MEMORY || flags == VK_KP_TABLE_LDS, "vk_kp_targets: flags = %d", flags);
  VK_CHECK_ARG(flags != VK_KP_TABLE_LDS || table_len <= VK_KP_TABLE_LDS_MAX, "vk_kp_targets: a table of %d entries does not fit the LDS path (%d)",
               table_len, VK_KP_TABLE_LDS_MAX);
  VK_CHECK_ARG((((uintptr_t)records) & (va - 1)) == 0 && (((uintptr_t)counts | (uintptr_t)table | (uintptr_t)out) & 3) == 0,
               "vk_kp_targets: misaligned buffer");
  hipStream_t st = (hipStream_t)stream;
  vkh::ProfScope ps_("kp_targets", st, 0.0, (double)batch * (double)h * (double)w * 4.0);       // 4 bytes written per pixel
  const int tiles_x = (w + KP_TW - 1) / KP_TW;
  const int64_t ntiles = (int64_t)tiles_x * ((h + KP_TH - 1) / KP_TH);
  const dim3 grid((unsigned)(ntiles < (1 << 20) ? ntiles : (1 << 20)), (unsigned)batch);
  const bool vec = ((uintptr_t)out & 15) == 0 && image_stride % 4 == 0 && w % 4 == 0;
  const bool lds = flags == VK_KP_TABLE_LDS;                  // the default is the table in memory: profiles/keypoints/README.md
  const size_t dyn = lds ? (size_t)table_len * 4 : 0;
#define KP_LAUNCH(V, T)                                                                                                                          \
  hipLaunchKernelGGL((k_kp_targets<V, T>), grid, dim3(256), dyn, st, h, w, tiles_x, ntiles, (const char*)records, record_stride, vert_offset,   \
                     vert_type, valid_offset, counts, max_components, table, table_len, R16, out, image_stride)
  if (vec && lds) KP_LAUNCH(true, true);
  else if (vec) KP_LAUNCH(true, false);
  else if (lds) KP_LAUNCH(false, true);
  else KP_LAUNCH(false, false);
#undef KP_LAUNCH
  VK_CHECK_HIP(hipGetLastError());
  return VK_OK;
}

extern "C" size_t vk_kp_peaks_workspace_bytes(int batch, int h, int w) {
  if (batch < 1 || batch > 65535 || h < 1 || w < 1 || (size_t)h * (size_t)w > ((size_t)1 << 30)) return 0;
  return VK_KP_PEAKS_WS_BYTES(batch, h, w);
}

extern "C" int vk_kp_peaks(int batch, int h, int w, const float* heat, size_t image_stride, double min_peak, int nms_radius, int max_peaks,
                           vk_kp_peak* out, int32_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
  const char* fn = "vk_kp_peaks";
  const int rc = kp_check_maps(fn, batch, h, w, image_stride);
  if (rc != VK_OK) return rc;
  VK_CHECK_ARG(isfinite(min_peak), "vk_kp_peaks: min_peak is not finite");
  VK_CHECK_ARG(nms_radius >= 1 && nms_radius <= VK_KP_MAX_NMS, "vk_kp_peaks: nms_radius = %d outside 1..%d", nms_radius, VK_KP_MAX_NMS);
  VK_CHECK_ARG(max_peaks >= 1 && max_peaks <= 4096, "vk_kp_peaks: max_peaks = %d outside 1..4096", max_peaks);
  VK_CHECK_ARG(heat && out && counts && workspace, "vk_kp_peaks: null buffer");
  VK_CHECK_ARG(workspace_bytes >= VK_KP_PEAKS_WS_BYTES(batch, h, w), "vk_kp_peaks: workspace of %zu bytes, %zu needed", workspace_bytes,
               (size_t)VK_KP_PEAKS_WS_BYTES(batch, h, w));
  VK_CHECK_ARG((((uintptr_t)heat | (uintptr_t)out | (uintptr_t)counts | (uintptr_t)workspace) & 3) == 0, "vk_kp_peaks: misaligned buffer");
  hipStream_t st = (hipStream_t)stream;
  vkh::ProfScope ps_("kp_peaks", st, 0.0, (double)batch * (double)h * (double)w * 4.0);         // every pixel read once
  const int nb = (int)(((size_t)h * w + KP_CHUNK - 1) / KP_CHUNK);
  int32_t* blk = (int32_t*)workspace;
  uint8_t* masks = (uint8_t*)workspace + (size_t)batch * nb * 4;
  hipLaunchKernelGGL(k_kp_mark, dim3((unsigned)nb, (unsigned)batch), dim3(256), 0, st, h, w, nb, heat, image_stride, min_peak, nms_radius, blk, masks);
  hipLaunchKernelGGL(k_kp_scan, dim3((unsigned)batch), dim3(256), 0, st, nb, blk, counts);
  hipLaunchKernelGGL(k_kp_emit, dim3((unsigned)nb, (unsigned)batch), dim3(256), 0, st, w, nb, heat, image_stride, max_peaks, (const int32_t*)blk,
                     (const uint8_t*)masks, out);
  VK_CHECK_HIP(hipGetLastError());
  return VK_OK;
}

extern "C" int vk_kp_refine(const vk_kp_params* params, int batch, int h, int w, const float* heat, size_t image_stride, const void* records,
                            size_t record_stride, size_t box_offset, int valid_offset, const int32_t* counts, int max_components,
                            const double* affine, vk_subpix_quad* out, void* stream) {
  VK_CHECK_ARG(params, "vk_kp_refine: null parameters");
  const vk_kp_params& p = *params;
  VK_CHECK_ARG(p.method == VK_KP_PARABOLA || p.method == VK_KP_CENTROID, "vk_kp_refine: method %d is neither parabola nor centroid", p.method);
  VK_CHECK_ARG(p.search >= 1 && p.search <= VK_KP_MAX_SEARCH, "vk_kp_refine: search = %d outside 1..%d", p.search, VK_KP_MAX_SEARCH);
  VK_CHECK_ARG(p.cwin >= 1 && p.cwin <= VK_KP_MAX_CWIN, "vk_kp_refine: cwin = %d outside 1..%d", p.cwin, VK_KP_MAX_CWIN);
  VK_CHECK_ARG(isfinite(p.min_peak), "vk_kp_refine: min_peak is not finite");
  VK_CHECK_ARG(p.floor_frac >= 0.0 && p.floor_frac < 1.0, "vk_kp_refine: floor_frac = %g outside [0, 1)", p.floor_frac);
  const int rc = kp_check_maps("vk_kp_refine", batch, h, w, image_stride);
  if (rc != VK_OK) return rc;
  VK_CHECK_ARG(max_components >= 1 && max_components <= 4096, "vk_kp_refine: max_components = %d outside 1..4096", max_components);
  VK_CHECK_ARG(heat && records && counts && out, "vk_kp_refine: null buffer");
  VK_CHECK_ARG(record_stride % 4 == 0 && box_offset % 4 == 0 && box_offset >= 8 && record_stride <= ((size_t)1 << 20) && box_offset <= record_stride &&
                   box_offset + 32 <= record_stride,
               "vk_kp_refine: record stride %zu / box offset %zu: multiples of 4 with label, area and box[8] inside the record", record_stride,
               box_offset);
  VK_CHECK_ARG(valid_offset == -1 || (valid_offset >= 8 && valid_offset % 4 == 0 && (size_t)valid_offset + 4 <= record_stride),
               "vk_kp_refine: valid offset %d is neither -1 nor an int inside the record", valid_offset);
  VK_CHECK_ARG((((uintptr_t)heat | (uintptr_t)records | (uintptr_t)counts) & 3) == 0 && (((uintptr_t)out | (uintptr_t)affine) & 7) == 0,
               "vk_kp_refine: misaligned buffer");
  hipStream_t st = (hipStream_t)stream;
  vkh::ProfScope ps_("kp_refine", st, 0.0, (double)batch * (double)max_components * (double)sizeof(vk_subpix_quad));
  hipLaunchKernelGGL(k_kp_refine, dim3((unsigned)max_components, (unsigned)batch), dim3(256), 0, st, p, h, w, heat, image_stride, (const char*)records,
                     record_stride, box_offset, valid_offset, counts, max_components, affine, out);
  VK_CHECK_HIP(hipGetLastError());
  return VK_OK;
}
