// Second-pass inference on one window per indentation: vk_zoom_windows, vk_zoom_gather, vk_zoom_merge.
//
//   k_zoom_windows : one workgroup walks the B x M first-pass slots in chunks of 256.  A thread derives its slot's window in float64
//        (the corners through the first pass's affine row, their mean, the half extent, the clamped scale, the origin); a ballot per
//        wave and four wave totals in LDS give every window its place in ascending (map, slot) order, without atomics.
//   k_zoom_gather  : the hot path.  One workgroup per 32 x 8 output tile of one window (blockIdx.z = window).  The value of an output
//        pixel is the mean of the source image over the square of side f = max(s, 1) around the pixel's centre, separable: per axis
//        source pixel i weighs min(b, i + 1) - max(a, i).  Two forms of one kernel template.  Direct (the default, no LDS): every
//        thread takes the two nested sums of its pixel from memory.  Staged (VK_ZOOM_STAGED): the part of the tile's source footprint
//        that lies in the image goes to LDS as aligned dwords (each holds at least one byte of its row, so no load leaves the pages
//        of the image), the horizontal pass leaves one float64 row sum per (footprint row, output column, channel) in LDS, the
//        vertical pass adds them up; a footprint beyond the LDS (s above about 5) takes the direct sums.  Both forms do the same
//        float64 operations in the same order: columns ascending within a row, rows ascending, one division by f * f; then rint,
//        clamp, and the float32 normalisation of k_letterbox_pre / k_tile_pre.  The direct form is the default because it measured
//        faster: above scale 1 the squares of neighbouring output pixels tile the source, so staging shares
//        no tap and saves no arithmetic, while it costs two barriers, byte reads from LDS and all but two workgroups per CU.
//   k_zoom_merge   : one thread per first-pass slot: binary search of its window, the integer containment test on the second pass's
//        polygons, the acceptance rules, and a copy of either the second pass's record or the first pass's.
// The arithmetic is spelt out in include/vk_unet.h and mirrored by tests/zoom_ref.py.  Every tap is checked against the image's h and
// w before it is read, every byte offset is 64-bit, and nothing depends on the launch shape.
#include "vk_common.h"

#include <math.h>

#pragma clang fp contract(off)

namespace vk {

static_assert(sizeof(vk_zoom_window) == 40 && sizeof(vk_zoom_image) == 24 && sizeof(vk_zoom_params) == 32, "vk_zoom_* layouts");
static_assert(sizeof(vk_subpix_quad) == 200, "vk_subpix_quad layout");

// ------------------------------------------------------------------------------------------------ windows
__global__ __launch_bounds__(256) void k_zoom_windows(const vk_zoom_params P, int B, const char* __restrict__ recs, size_t stride,
                                                      size_t box_off, int valid_off, const int32_t* __restrict__ counts, int M,
                                                      const double* __restrict__ affine, const int32_t* __restrict__ sizes,
                                                      vk_zoom_window* __restrict__ windows, int32_t* __restrict__ n_windows) {
#pragma clang fp contract(off)
  __shared__ int s_wave[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long total = (long long)B * M;
  int base = 0;                                                // windows found in the chunks before this one (uniform)
  for (long long c0 = 0; c0 < total; c0 += 256) {
    const long long e = c0 + tid;
    bool have = false;
    vk_zoom_window W{0, 0, 0, 0, 0.0, 0.0, 0.0};
    if (e < total) {
      const int b = (int)(e / M), t = (int)(e - (long long)b * M);
      const int cnt = counts[b];
      const int used = cnt < 0 ? 0 : (cnt > M ? M : cnt);
      const char* rec = recs + (size_t)e * stride;
      if (t < used && (valid_off < 0 || *reinterpret_cast<const int*>(rec + valid_off) != 0)) {
        const int* box = reinterpret_cast<const int*>(rec + box_off);
        double ox = 0.0, oy = 0.0, inv = 1.0;
        if (affine) { ox = affine[3 * (size_t)b]; oy = affine[3 * (size_t)b + 1]; inv = affine[3 * (size_t)b + 2]; }
        double sx[4], sy[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          sx[q] = ((double)box[2 * q] - ox) * inv;
          sy[q] = ((double)box[2 * q + 1] - oy) * inv;
        }
        const double cx = (((sx[0] + sx[1]) + sx[2]) + sx[3]) * 0.25;
        const double cy = (((sy[0] + sy[1]) + sy[2]) + sy[3]) * 0.25;
        double ext = 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const double dx = fabs(sx[q] - cx), dy = fabs(sy[q] - cy);
          ext = dx > ext ? dx : ext;
          ext = dy > ext ? dy : ext;
        }
        const double S = (double)P.S;
        const double raw = (P.margin * (2.0 * ext)) / S;
        double s = raw;
        int status = 0;
        if (!(raw >= P.s_min)) { s = P.s_min; status |= VK_ZOOM_SCALE_CLAMPED_LO; }
        if (raw > P.s_max) { s = P.s_max; status |= VK_ZOOM_SCALE_CLAMPED_HI; }
        const double X0 = (cx + 0.5) - (S * s) * 0.5;
        const double Y0 = (cy + 0.5) - (S * s) * 0.5;
        const double h = (double)sizes[2 * (size_t)b], w = (double)sizes[2 * (size_t)b + 1];
        if (!(X0 >= 0.0 && Y0 >= 0.0 && X0 + S * s <= w && Y0 + S * s <= h)) status |= VK_ZOOM_CLIPPED;
        W.map = b; W.slot = t; W.status = status; W.pad = 0; W.X0 = X0; W.Y0 = Y0; W.s = s;
        have = true;
      }
    }
    const unsigned long long m = __ballot(have);
    if (lane == 0) s_wave[wave] = __popcll(m);
    __syncthreads();
    int before = base, chunk = 0;
    for (int k = 0; k < 4; ++k) {
      if (k < wave) before += s_wave[k];
      chunk += s_wave[k];
    }
    const int pos = before + __popcll(m & ((1ull << lane) - 1ull));
    if (have && pos < P.max_windows) windows[pos] = W;
    base += chunk;
    __syncthreads();                                           // s_wave is written again by the next chunk
  }
  if (tid == 0) *n_windows = base < P.max_windows ? base : P.max_windows;
}

// ------------------------------------------------------------------------------------------------ gather
constexpr int ZT_W = 32, ZT_H = 8;
constexpr int ZT_SRC_DW = 6016;         // dwords of staged source bytes
constexpr int ZT_HROWS = 53;            // footprint rows of row sums: 53 * 32 * 3 doubles
constexpr double ZT_MAX_ORIGIN = 1073741824.0;

__device__ __forceinline__ void z_span(double O, int x, double s, double f, double& a, double& b) {
#pragma clang fp contract(off)
  a = (O + ((double)x + 0.5) * s) - f * 0.5;
  b = a + f;
}

__device__ __forceinline__ double z_weight(double a, double b, int i) {
#pragma clang fp contract(off)
  const double lo = a > (double)i ? a : (double)i;
  const double hi = b < (double)(i + 1) ? b : (double)(i + 1);
  return hi - lo;
}

__device__ __forceinline__ void z_store(float* __restrict__ o, size_t plane, const double* v, double ff) {
#pragma clang fp contract(off)
  const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    int q = (int)rint(v[2 - k] / ff);                          // RGB plane k = BGR channel 2 - k
    q = q < 0 ? 0 : (q > 255 ? 255 : q);
    const float f = (float)q / 255.f;
    o[k * plane] = (f - mean[k]) / stdv[k];
  }
}

template <bool STAGED>
__global__ __launch_bounds__(256) void k_zoom_gather(int S, int n_images, int pad, const vk_zoom_window* __restrict__ windows,
                                                     const vk_zoom_image* __restrict__ images, float* __restrict__ out) {
#pragma clang fp contract(off)
  const int n = blockIdx.z, tid = threadIdx.x;
  const vk_zoom_window W = windows[n];
  const int tx = tid & (ZT_W - 1), ty = tid / ZT_W;
  const int xs = blockIdx.x * ZT_W, ys = blockIdx.y * ZT_H;
  const int x = xs + tx, y = ys + ty;
  const bool in = x < S && y < S;
  const size_t plane = (size_t)S * S;
  float* o = out + (size_t)n * 3 * plane + (size_t)(in ? y : 0) * S + (in ? x : 0);
  const double dpad = (double)pad;
  const bool ok = W.map >= 0 && W.map < n_images && W.s >= 0.25 && W.s <= 64.0 && fabs(W.X0) <= ZT_MAX_ORIGIN &&
                  fabs(W.Y0) <= ZT_MAX_ORIGIN;                 // uniform over the workgroup; a NaN fails
  if (!ok) {
    const double v[3] = {dpad, dpad, dpad};
    if (in) z_store(o, plane, v, 1.0);
    return;
  }
  const vk_zoom_image img = images[W.map];
  const uint8_t* __restrict__ src = reinterpret_cast<const uint8_t*>(img.ptr);
  const int h = img.h, w = img.w;
  const size_t rstride = (size_t)img.stride;
  const double s = W.s, f = s > 1.0 ? s : 1.0, ff = f * f;
  double ax, bx, ay, by;
  z_span(W.X0, x, s, f, ax, bx);
  z_span(W.Y0, y, s, f, ay, by);
  const int i0 = (int)floor(ax), i1 = (int)floor(bx), j0 = (int)floor(ay), j1 = (int)floor(by);
  // the tile's footprint: z_span is monotonic in x, so every pixel's taps lie in [c0, c1] x [r0, r1]
  double ta, tb, ua, ub;
  z_span(W.X0, xs, s, f, ta, ub);
  z_span(W.X0, min(xs + ZT_W, S) - 1, s, f, ua, tb);
  const int c0 = (int)floor(ta), c1 = (int)floor(tb);
  z_span(W.Y0, ys, s, f, ta, ub);
  z_span(W.Y0, min(ys + ZT_H, S) - 1, s, f, ua, tb);
  const int r0 = (int)floor(ta), r1 = (int)floor(tb);
  const int xa = max(c0, 0), xb = min(c1 + 1, w), ya = max(r0, 0), yb = min(r1 + 1, h);   // the part of it inside the image
  const int nbytes = xb > xa ? (xb - xa) * 3 : 0, nrow = (yb > ya && nbytes > 0) ? yb - ya : 0;
  const int pitch = (nbytes + 6) >> 2;                         // dwords per staged row, whatever its alignment
  const int FH = r1 - r0 + 1;
  double tot[3] = {0.0, 0.0, 0.0};
  bool done = false;
  if constexpr (STAGED) {
    if (FH <= ZT_HROWS && (long long)nrow * pitch <= ZT_SRC_DW) {               // uniform over the workgroup
      __shared__ uint32_t s_src[ZT_SRC_DW];
      __shared__ double s_h[ZT_HROWS * ZT_W * 3];
      done = true;
      for (int e = tid; e < nrow * pitch; e += 256) {
        const int r = e / pitch, d = e - r * pitch;
        const uint8_t* p = src + (size_t)(ya + r) * rstride + (size_t)xa * 3;
        const int sa = (int)((uintptr_t)p & 3);
        if (d < ((sa + nbytes + 3) >> 2)) s_src[e] = reinterpret_cast<const uint32_t*>(p - sa)[d];
      }
      __syncthreads();
      // horizontal pass: one (footprint row, output column) per item
      for (int e = tid; e < FH * ZT_W; e += 256) {
        const int fr = e / ZT_W, cx = e & (ZT_W - 1), xx = xs + cx;
        if (xx >= S) continue;
        const int row = r0 + fr;
        const bool row_in = row >= ya && row < yb && nrow > 0;
        const uint8_t* rp = nullptr;
        if (row_in) {
          const int sa = (int)((uintptr_t)(src + (size_t)row * rstride + (size_t)xa * 3) & 3);
          rp = reinterpret_cast<const uint8_t*>(s_src + (size_t)(row - ya) * pitch) + sa;
        }
        double a, b;
        z_span(W.X0, xx, s, f, a, b);
        const int k0 = (int)floor(a), k1 = (int)floor(b);
        double r[3] = {0.0, 0.0, 0.0};
        for (int i = k0; i <= k1; ++i) {
          const double wx = z_weight(a, b, i);
          double p0 = dpad, p1 = dpad, p2 = dpad;
          if (row_in && i >= xa && i < xb) {
            const uint8_t* t = rp + 3 * (i - xa);
            p0 = (double)t[0]; p1 = (double)t[1]; p2 = (double)t[2];
          }
          r[0] = r[0] + wx * p0;
          r[1] = r[1] + wx * p1;
          r[2] = r[2] + wx * p2;
        }
        double* hs = s_h + (size_t)e * 3;
        hs[0] = r[0]; hs[1] = r[1]; hs[2] = r[2];
      }
      __syncthreads();
      if (in) {
        for (int j = j0; j <= j1; ++j) {
          const double wy = z_weight(ay, by, j);
          const double* hs = s_h + ((size_t)(j - r0) * ZT_W + tx) * 3;
          tot[0] = tot[0] + wy * hs[0];
          tot[1] = tot[1] + wy * hs[1];
          tot[2] = tot[2] + wy * hs[2];
        }
      }
    }
  }
  if (!done && in) {
    for (int j = j0; j <= j1; ++j) {
      const double wy = z_weight(ay, by, j);
      const bool row_in = j >= 0 && j < h;
      const uint8_t* rp = src + (size_t)(row_in ? j : 0) * rstride;
      double r[3] = {0.0, 0.0, 0.0};
      for (int i = i0; i <= i1; ++i) {
        const double wx = z_weight(ax, bx, i);
        double p0 = dpad, p1 = dpad, p2 = dpad;
        if (row_in && i >= 0 && i < w) {
          const uint8_t* t = rp + (size_t)i * 3;
          p0 = (double)t[0]; p1 = (double)t[1]; p2 = (double)t[2];
        }
        r[0] = r[0] + wx * p0;
        r[1] = r[1] + wx * p1;
        r[2] = r[2] + wx * p2;
      }
      tot[0] = tot[0] + wy * r[0];
      tot[1] = tot[1] + wy * r[1];
      tot[2] = tot[2] + wy * r[2];
    }
  }
  if (in) z_store(o, plane, tot, ff);
}

// ------------------------------------------------------------------------------------------------ merge
__global__ __launch_bounds__(256) void k_zoom_merge(int S, double agree, int n, const vk_zoom_window* __restrict__ windows,
                                                    const char* __restrict__ recs2, size_t stride2, size_t box_off2, int valid_off2,
                                                    const int32_t* __restrict__ counts2, int M2, const vk_subpix_quad* __restrict__ quads2,
                                                    int B, int M, const int32_t* __restrict__ counts,
                                                    const vk_subpix_quad* __restrict__ coarse, vk_subpix_quad* __restrict__ out,
                                                    int32_t* __restrict__ status, double* __restrict__ scale) {
#pragma clang fp contract(off)
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)B * M) return;
  const int b = (int)(e / M), t = (int)(e - (long long)b * M);
  const int cnt = counts[b];
  const int used = cnt < 0 ? 0 : (cnt > M ? M : cnt);
  if (t >= used) {
    status[e] = VK_ZOOM_NO_WINDOW;
    scale[e] = 0.0;
    return;
  }
  // the window of (b, t): the list is sorted by (map, slot)
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const long long key = (long long)windows[mid].map * M + windows[mid].slot;
    if (key < e) lo = mid + 1; else hi = mid;
  }
  const bool found = lo < n && windows[lo].map == b && windows[lo].slot == t;
  if (!found) {
    out[e] = coarse[e];
    status[e] = VK_ZOOM_NO_WINDOW;
    scale[e] = 0.0;
    return;
  }
  const int k = lo;
  const int wbits = windows[k].status;
  scale[e] = windows[k].s;
  const int c2 = counts2[k];
  const int used2 = c2 < 0 ? 0 : (c2 > M2 ? M2 : c2);
  int target = -1, best_area = 0;
  const long long P = (long long)S;
  for (int u = 0; u < used2; ++u) {
    const char* rec = recs2 + ((size_t)k * M2 + u) * stride2;
    if (valid_off2 >= 0 && *reinterpret_cast<const int*>(rec + valid_off2) == 0) continue;
    if (quads2[(size_t)k * M2 + u].valid == 0) continue;
    const int* box = reinterpret_cast<const int*>(rec + box_off2);
    bool all_pos = true, all_neg = true;
    for (int q = 0; q < 4; ++q) {
      const int q1 = (q + 1) & 3;
      const long long axd = 2ll * box[2 * q], ayd = 2ll * box[2 * q + 1];
      const long long bxd = 2ll * box[2 * q1], byd = 2ll * box[2 * q1 + 1];
      const long long cr = (bxd - axd) * (P - ayd) - (byd - ayd) * (P - axd);
      all_pos = all_pos && cr >= 0;
      all_neg = all_neg && cr <= 0;
    }
    if (!(all_pos || all_neg)) continue;
    const int area = reinterpret_cast<const int*>(rec)[1];
    if (target < 0 || area > best_area) { target = u; best_area = area; }
  }
  int st;
  if (target < 0) {
    st = VK_ZOOM_NO_TARGET;
  } else {
    const vk_subpix_quad* q2 = quads2 + (size_t)k * M2 + target;
    const int fl = (q2->flags[0] | q2->flags[1]) | (q2->flags[2] | q2->flags[3]);
    const double dc = coarse[e].d_mean;
    if (fl & VK_ZOOM_FAIL_MASK) st = VK_ZOOM_REFINE_FAILED;
    else if (!(fabs(q2->d_mean - dc) <= agree * dc)) st = VK_ZOOM_DISAGREES;
    else st = VK_ZOOM_ZOOMED;
  }
  if (st == VK_ZOOM_ZOOMED) {
    vk_subpix_quad r = quads2[(size_t)k * M2 + target];
    r.label = coarse[e].label;
    r.area = coarse[e].area;
    out[e] = r;
  } else {
    out[e] = coarse[e];
  }
  status[e] = st | wbits;
}

}  // namespace vk

using namespace vk;

static int zoom_check_records(const char* who, size_t record_stride, size_t box_offset, int valid_offset) {
  VK_CHECK_ARG(record_stride % 4 == 0 && box_offset % 4 == 0 && box_offset >= 8 && box_offset + 32 <= record_stride,
               "%s: record stride %zu / box offset %zu: multiples of 4 with label, area and box[8] inside the record", who, record_stride,
               box_offset);
  VK_CHECK_ARG(valid_offset == -1 || (valid_offset >= 8 && valid_offset % 4 == 0 && (size_t)valid_offset + 4 <= record_stride),
               "%s: valid offset %d is neither -1 nor an int inside the record", who, valid_offset);
  return VK_OK;
}

extern "C" int vk_zoom_windows(const vk_zoom_params* params, int batch, const void* records, size_t record_stride, size_t box_offset,
                               int valid_offset, const int32_t* counts, int max_components, const double* affine, const int32_t* sizes,
                               vk_zoom_window* windows, int32_t* n_windows, void* stream) {
  VK_CHECK_ARG(params, "vk_zoom_windows: null parameters");
  const vk_zoom_params p = *params;
  VK_CHECK_ARG(p.S >= 1 && p.S <= 16384, "vk_zoom_windows: S = %d outside 1..16384", p.S);
  VK_CHECK_ARG(p.s_min >= 0.25 && p.s_min <= p.s_max && p.s_max <= 64.0, "vk_zoom_windows: s_min = %g, s_max = %g: need 0.25 <= s_min <= s_max <= 64",
               p.s_min, p.s_max);
  VK_CHECK_ARG(p.margin >= 1.0 && p.margin <= 8.0, "vk_zoom_windows: margin = %g outside [1, 8]", p.margin);
  VK_CHECK_ARG(p.max_windows >= 1 && p.max_windows <= 65535, "vk_zoom_windows: max_windows = %d outside 1..65535", p.max_windows);
  VK_CHECK_ARG(batch >= 1 && batch <= 65535, "vk_zoom_windows: batch %d outside 1..65535", batch);
  VK_CHECK_ARG(max_components >= 1 && max_components <= 4096, "vk_zoom_windows: max_components = %d outside 1..4096", max_components);
  VK_CHECK_ARG(records && counts && sizes && windows && n_windows, "vk_zoom_windows: null buffer");
  if (int rc = zoom_check_records("vk_zoom_windows", record_stride, box_offset, valid_offset)) return rc;
  VK_CHECK_ARG((((uintptr_t)records | (uintptr_t)counts | (uintptr_t)sizes | (uintptr_t)n_windows) & 3) == 0 &&
                   (((uintptr_t)windows | (uintptr_t)affine) & 7) == 0,
               "vk_zoom_windows: misaligned buffer");
  hipStream_t st = (hipStream_t)stream;
  vkh::ProfScope ps_("zoom_windows", st, 0.0, (double)batch * (double)max_components * (double)(record_stride + sizeof(vk_zoom_window)));
  hipLaunchKernelGGL(k_zoom_windows, dim3(1), dim3(256), 0, st, p, batch, (const char*)records, record_stride, box_offset, valid_offset, counts,
                     max_components, affine, sizes, windows, n_windows);
  VK_CHECK_HIP(hipGetLastError());
  return VK_OK;
}

extern "C" int vk_zoom_gather(int n, int S, const vk_zoom_window* windows, int n_images, const vk_zoom_image* images_host, void* images_dev,
                              int pad_value, int flags, float* out, void* stream) {
  VK_CHECK_ARG(n >= 1 && n <= 65535, "vk_zoom_gather: %d windows outside 1..65535", n);
  VK_CHECK_ARG(S >= 1 && S <= 16384, "vk_zoom_gather: S = %d outside 1..16384", S);
  VK_CHECK_ARG(n_images >= 1 && n_images <= 65535, "vk_zoom_gather: %d images outside 1..65535", n_images);
  VK_CHECK_ARG(pad_value >= 0 && pad_value <= 255, "vk_zoom_gather: pad_value outside 0..255");
  VK_CHECK_ARG((flags & ~VK_ZOOM_STAGED) == 0, "vk_zoom_gather: unknown flags 0x%x", flags);
  VK_CHECK_ARG(windows && images_host && images_dev && out, "vk_zoom_gather: null buffer");
  VK_CHECK_ARG((((uintptr_t)windows | (uintptr_t)images_dev) & 7) == 0 && ((uintptr_t)out & 3) == 0, "vk_zoom_gather: misaligned buffer");
  for (int i = 0; i < n_images; ++i) {
    const vk_zoom_image& im = images_host[i];
    VK_CHECK_ARG(im.ptr != 0, "vk_zoom_gather: image %d: null address", i);
    VK_CHECK_ARG(im.h >= 1 && im.h <= 16384 && im.w >= 1 && im.w <= 16384, "vk_zoom_gather: image %d: size %dx%d outside 1..16384", i, im.h, im.w);
    VK_CHECK_ARG(im.stride >= 3 * (int64_t)im.w && im.stride <= ((int64_t)1 << 31), "vk_zoom_gather: image %d: row stride %lld below 3 * w", i,
                 (long long)im.stride);
  }
  hipStream_t st = (hipStream_t)stream;
  VK_CHECK_HIP(hipMemcpyAsync(images_dev, images_host, (size_t)n_images * sizeof(vk_zoom_image), hipMemcpyHostToDevice, st));
  vkh::ProfScope ps_("zoom_gather", st, 0.0, (double)n * S * S * 12.0);
  const dim3 grid((S + ZT_W - 1) / ZT_W, (S + ZT_H - 1) / ZT_H, n);
  if (flags & VK_ZOOM_STAGED)
    hipLaunchKernelGGL(k_zoom_gather<true>, grid, dim3(256), 0, st, S, n_images, pad_value, windows, (const vk_zoom_image*)images_dev, out);
  else
    hipLaunchKernelGGL(k_zoom_gather<false>, grid, dim3(256), 0, st, S, n_images, pad_value, windows, (const vk_zoom_image*)images_dev, out);
  VK_CHECK_HIP(hipGetLastError());
  return VK_OK;
}

extern "C" int vk_zoom_merge(int S, double agree, int n, const vk_zoom_window* windows, const void* records2, size_t record_stride2,
                             size_t box_offset2, int valid_offset2, const int32_t* counts2, int max_components2,
                             const vk_subpix_quad* quads2, int batch, int max_components, const int32_t* counts,
                             const vk_subpix_quad* coarse, vk_subpix_quad* out, int32_t* status, double* scale, void* stream) {
  VK_CHECK_ARG(S >= 1 && S <= 16384, "vk_zoom_merge: S = %d outside 1..16384", S);
  VK_CHECK_ARG(agree >= 0.0 && agree <= 1.7976931348623157e308, "vk_zoom_merge: agree = %g is not a finite number >= 0", agree);
  VK_CHECK_ARG(n >= 0 && n <= 65535, "vk_zoom_merge: %d windows outside 0..65535", n);
  VK_CHECK_ARG(batch >= 1 && batch <= 65535, "vk_zoom_merge: batch %d outside 1..65535", batch);
  VK_CHECK_ARG(max_components >= 1 && max_components <= 4096, "vk_zoom_merge: max_components = %d outside 1..4096", max_components);
  VK_CHECK_ARG(counts && coarse && out && status && scale, "vk_zoom_merge: null buffer");
  VK_CHECK_ARG(((uintptr_t)counts & 3) == 0 && ((uintptr_t)status & 3) == 0 && (((uintptr_t)coarse | (uintptr_t)out | (uintptr_t)scale) & 7) == 0,
               "vk_zoom_merge: misaligned buffer");
  if (n > 0) {
    VK_CHECK_ARG(windows && records2 && counts2 && quads2, "vk_zoom_merge: null second-pass buffer with %d windows", n);
    VK_CHECK_ARG(max_components2 >= 1 && max_components2 <= 4096, "vk_zoom_merge: max_components2 = %d outside 1..4096", max_components2);
    if (int rc = zoom_check_records("vk_zoom_merge", record_stride2, box_offset2, valid_offset2)) return rc;
    VK_CHECK_ARG((((uintptr_t)records2 | (uintptr_t)counts2) & 3) == 0 && (((uintptr_t)windows | (uintptr_t)quads2) & 7) == 0,
                 "vk_zoom_merge: misaligned second-pass buffer");
  }
  hipStream_t st = (hipStream_t)stream;
  const long long total = (long long)batch * max_components;
  vkh::ProfScope ps_("zoom_merge", st, 0.0, (double)total * (2.0 * sizeof(vk_subpix_quad) + 12.0));
  hipLaunchKernelGGL(k_zoom_merge, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, S, agree, n, windows, (const char*)records2,
                     record_stride2, box_offset2, valid_offset2, counts2, max_components2, quads2, batch, max_components, counts, coarse, out,
                     status, scale);
  VK_CHECK_HIP(hipGetLastError());
  return VK_OK;
}
