// Validation panels and detection overlays on the device: vk_render_val_panels, vk_render_primitives,
// vk_render_draw, vk_render_reduce, vk_render_glyph.
//
//   k_render_panels : one thread per pixel of one validation image: the de-normalised input (float64), the two maps as bytes, the
//        float32 blend; twelve bytes into the four panels of the pixel's row.
//   k_render_prims  : one workgroup per map.  Pass 1 leaves the state (not drawn / drawn / skipped) and the area of every slot in LDS;
//        pass 2 ranks every drawn slot by counting over LDS (no sort, no atomics) and writes its record at [rank]: corners, the two
//        diagonals (int64 squared distances), colour, label (the digits of "%.1f" through an exact two-term product), anchor, box.
//   k_render_draw   : the hot path.  One workgroup per 32 x 8 tile of one map.  Binned (the default): the workgroup tests the records'
//        boxes against the tile, 256 at a time, and compacts the hits into LDS in list order (ballot + prefix count); a pixel then
//        walks that short list from its end and stops at the first record that covers it, which is the last one painted.  Direct
//        (VK_RENDER_DIRECT): every pixel walks the whole list the same way.  Coverage is integer arithmetic (int64; see the header for
//        why every product fits).
//   k_render_reduce : one thread per output pixel: the rounded mean of its k x k block, partial at the edges.
// The rules are spelt out in include/vk_unet.h and mirrored by tests/render_ref.py.  Every read and write is checked against the sizes
// it was given, every byte offset is 64-bit, nothing depends on the launch shape.
#include "vk_common.h"

#include <math.h>

#pragma clang fp contract(off)

#define VK_GLYPH_ROWS                                                                              \
  {{0b01110, 0b10001, 0b10011, 0b10101, 0b11001, 0b10001, 0b01110},  /* 0 */                     \
   {0b00100, 0b01100, 0b00100, 0b00100, 0b00100, 0b00100, 0b01110},  /* 1 */                     \
   {0b01110, 0b10001, 0b00001, 0b00010, 0b00100, 0b01000, 0b11111},  /* 2 */                     \
   {0b11111, 0b00010, 0b00100, 0b00010, 0b00001, 0b10001, 0b01110},  /* 3 */                     \
   {0b00010, 0b00110, 0b01010, 0b10010, 0b11111, 0b00010, 0b00010},  /* 4 */                     \
   {0b11111, 0b10000, 0b11110, 0b00001, 0b00001, 0b10001, 0b01110},  /* 5 */                     \
   {0b00110, 0b01000, 0b10000, 0b11110, 0b10001, 0b10001, 0b01110},  /* 6 */                     \
   {0b11111, 0b00001, 0b00010, 0b00100, 0b01000, 0b01000, 0b01000},  /* 7 */                     \
   {0b01110, 0b10001, 0b10001, 0b01110, 0b10001, 0b10001, 0b01110},  /* 8 */                     \
   {0b01110, 0b10001, 0b10001, 0b01111, 0b00001, 0b00010, 0b01100},  /* 9 */                     \
   {0b01010, 0b01010, 0b11111, 0b01010, 0b11111, 0b01010, 0b01010},  /* # */                     \
   {0b00000, 0b00000, 0b00000, 0b00000, 0b00000, 0b00000, 0b00000},  /* space */                 \
   {0b00000, 0b00000, 0b11010, 0b10101, 0b10101, 0b10001, 0b10001},  /* m */                     \
   {0b00000, 0b00000, 0b01110, 0b10001, 0b11111, 0b10000, 0b01110},  /* e */                     \
   {0b00000, 0b00000, 0b01110, 0b00001, 0b01111, 0b10001, 0b01111},  /* a */                     \
   {0b00000, 0b00000, 0b10110, 0b11001, 0b10001, 0b10001, 0b10001},  /* n */                     \
   {0b00000, 0b00000, 0b11111, 0b00000, 0b11111, 0b00000, 0b00000},  /* = */                     \
   {0b00000, 0b00000, 0b00000, 0b00000, 0b00000, 0b01100, 0b01100},  /* . */                     \
   {0b00000, 0b00000, 0b11110, 0b10001, 0b11110, 0b10000, 0b10000},  /* p */                     \
   {0b00000, 0b00000, 0b10001, 0b01010, 0b00100, 0b01010, 0b10001},  /* x */                     \
   {0b01110, 0b10001, 0b00001, 0b00010, 0b00100, 0b00000, 0b00100}}  /* ? */

namespace vk {

static_assert(sizeof(vk_render_blend) == 16 && sizeof(vk_render_style) == 36 && sizeof(vk_render_prim) == 104 && sizeof(vk_render_view) == 88,
              "vk_render_* layouts");

constexpr int RN_GLYPHS = 21;
static const uint8_t h_glyph[RN_GLYPHS][7] = VK_GLYPH_ROWS;
__constant__ uint8_t d_glyph[RN_GLYPHS][7] = VK_GLYPH_ROWS;

__host__ __device__ inline int glyph_index(int ch) {
  if (ch >= '0' && ch <= '9') return ch - '0';
  switch (ch) {
    case '#': return 10;
    case ' ': return 11;
    case 'm': return 12;
    case 'e': return 13;
    case 'a': return 14;
    case 'n': return 15;
    case '=': return 16;
    case '.': return 17;
    case 'p': return 18;
    case 'x': return 19;
    case '?': return 20;
  }
  return -1;
}

constexpr int RT_W = 32, RT_H = 8;
constexpr int RN_MAX_M = 4096;

// ------------------------------------------------------------------------------------------------ bytes
__device__ __forceinline__ uint8_t f64_to_u8(double v) {                    // np.clip(v, 0, 255).astype(np.uint8), NaN -> 0
  if (!(v > 0.0)) return 0;
  return v >= 255.0 ? (uint8_t)255 : (uint8_t)(int)v;
}

__device__ __forceinline__ uint8_t unit_to_u8(float p) {                    // (uint8)(p * 255.f), clamped, NaN -> 0
#pragma clang fp contract(off)
  const float v = p * 255.f;
  if (!(v > 0.f)) return 0;
  return v >= 255.f ? (uint8_t)255 : (uint8_t)(int)v;
}

__device__ __forceinline__ uint8_t blend_u8(uint8_t a, uint8_t c, float alpha, float beta, float gamma) {
#pragma clang fp contract(off)
  const float p = (float)a * alpha;
  const float q = (float)c * beta;
  const float r = rintf((p + q) + gamma);                                  // round to nearest, ties to even
  if (!(r > 0.f)) return 0;
  return r >= 255.f ? (uint8_t)255 : (uint8_t)(int)r;
}

// ------------------------------------------------------------------------------------------------ panels
struct PanelArgs {
  double mean[3], stdv[3];
  vk_render_blend bl;
};

__global__ __launch_bounds__(256) void k_render_panels(int H, int W, const float* __restrict__ x, const float* __restrict__ y,
                                                       const float* __restrict__ pr, const PanelArgs A, int rgb, uint8_t* __restrict__ out,
                                                       long long row_stride) {
#pragma clang fp contract(off)
  const int px = blockIdx.x * RT_W + (threadIdx.x & (RT_W - 1)), py = blockIdx.y * RT_H + threadIdx.x / RT_W, n = blockIdx.z;
  if (px >= W || py >= H) return;
  const size_t plane = (size_t)H * W, pix = (size_t)py * W + px;
  const float* xn = x + (size_t)n * 3 * plane + pix;
  uint8_t base[3];                                                         // BGR
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double v = (((double)xn[k * plane] * A.stdv[k]) + A.mean[k]) * 255.0;
    base[2 - k] = f64_to_u8(v);
  }
  const uint8_t gt = unit_to_u8(y[(size_t)n * plane + pix]);
  const uint8_t pd = unit_to_u8(pr[(size_t)n * plane + pix]);
  uint8_t* row = out + ((size_t)n * H + py) * (size_t)row_stride;
  uint8_t* p0 = row + 3 * (size_t)px;
  uint8_t* p1 = row + 3 * ((size_t)W + px);
  uint8_t* p2 = row + 3 * (2 * (size_t)W + px);
  uint8_t* p3 = row + 3 * (3 * (size_t)W + px);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int o = rgb ? 2 - c : c;
    p0[o] = base[c];
    p1[o] = gt;
    p2[o] = pd;
    p3[o] = blend_u8(base[c], pd > 127 ? A.bl.color[c] : (uint8_t)0, A.bl.alpha, A.bl.beta, A.bl.gamma);
  }
}

// ------------------------------------------------------------------------------------------------ primitives
struct PrimArgs {
  size_t stride, box_off;
  int valid_off, diag_off, center_off, mode, M;
  vk_render_style style;
};

// state of a slot: 0 not drawn, 1 drawn, 2 skipped (a coordinate outside the range).  X: the eight corner coordinates, A: the anchor.
__device__ int prim_geometry(const PrimArgs& P, const char* rec, int t, int used, const double* aff, int* X, int* A) {
#pragma clang fp contract(off)
  if (t >= used) return 0;
  if (P.valid_off >= 0 && *reinterpret_cast<const int*>(rec + P.valid_off) == 0) return 0;
  double ox = 0.0, oy = 0.0, inv = 1.0;
  if (aff && P.mode != VK_RENDER_COORD_VS) { ox = aff[0]; oy = aff[1]; inv = aff[2]; }
  double m[8];
  if (P.mode == VK_RENDER_COORD_BOX) {
    const int* box = reinterpret_cast<const int*>(rec + P.box_off);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      m[2 * q] = ((double)box[2 * q] - ox) * inv;
      m[2 * q + 1] = ((double)box[2 * q + 1] - oy) * inv;
    }
  } else {
    const double* v = reinterpret_cast<const double*>(rec + P.box_off);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      m[2 * q] = (v[2 * q] - ox) * inv;
      m[2 * q + 1] = (v[2 * q + 1] - oy) * inv;
    }
  }
  double cx, cy;
  if (P.mode == VK_RENDER_COORD_BOX) {
    const float* c = reinterpret_cast<const float*>(rec + P.center_off);
    cx = ((double)c[0] - ox) * inv;
    cy = ((double)c[1] - oy) * inv;
  } else {
    cx = (((m[0] + m[2]) + m[4]) + m[6]) * 0.25;
    cy = (((m[1] + m[3]) + m[5]) + m[7]) * 0.25;
  }
  const double R = (double)VK_RENDER_MAX_COORD;
  bool ok = fabs(cx) <= R && fabs(cy) <= R;                                 // a NaN fails
#pragma unroll
  for (int q = 0; q < 8; ++q) ok = ok && fabs(m[q]) <= R;
  if (!ok) return 2;
#pragma unroll
  for (int q = 0; q < 8; ++q) X[q] = (int)rint(m[q]);
  A[0] = (int)cx + 6;
  A[1] = (int)cy - 6;
  return 1;
}

// the label goes straight to the record in global memory: a private character array indexed at run time would live in scratch
__device__ int put_uint(char* __restrict__ s, int at, long long v) {
  long long p = 1;
  while (v / p >= 10) p *= 10;
  for (; p > 0; p /= 10) s[at++] = (char)('0' + (int)((v / p) % 10));
  return at;
}

__device__ int make_label(char* __restrict__ s, int idx, double d) {
#pragma clang fp contract(off)
  for (int i = 0; i < VK_RENDER_LABEL_MAX; ++i) s[i] = 0;
  int at = 0;
  s[at++] = '#';
  at = put_uint(s, at, idx);
  s[at++] = ' '; s[at++] = 'm'; s[at++] = 'e'; s[at++] = 'a'; s[at++] = 'n'; s[at++] = '=';
  if (d >= 0.0 && d < 1.0e6) {                                             // finite; a NaN fails
    const double hi = d * 10.0, lo = fma(d, 10.0, -hi), f = floor(hi);
    const double r = ((hi - f) - 0.5) + lo;                                // the sign of 10 d - (f + 0.5), exactly
    long long n = (long long)f;
    if (r > 0.0 || (r == 0.0 && (n & 1))) n += 1;
    at = put_uint(s, at, n / 10);
    s[at++] = '.';
    s[at++] = (char)('0' + (int)(n % 10));
  } else {
    s[at++] = '?';
  }
  s[at++] = 'p';
  s[at++] = 'x';
  return at;
}

// the six corner pairs in the order (0,1) (0,2) (0,3) (1,2) (1,3) (2,3); the pair of the other two corners is number 5 - p
__device__ __forceinline__ int pair_i(int p) { return p < 3 ? 0 : (p < 5 ? 1 : 2); }
__device__ __forceinline__ int pair_j(int p) { return p < 3 ? p + 1 : (p < 5 ? p - 1 : 3); }

__global__ __launch_bounds__(256) void k_render_prims(const PrimArgs P, const char* __restrict__ recs, const int32_t* __restrict__ counts,
                                                      const double* __restrict__ affine, vk_render_prim* __restrict__ prims,
                                                      int32_t* __restrict__ drawn, int32_t* __restrict__ skipped) {
#pragma clang fp contract(off)
  __shared__ int s_area[RN_MAX_M];
  __shared__ uint8_t s_state[RN_MAX_M];
  __shared__ int s_cnt[4][2];
  const int b = blockIdx.x, tid = threadIdx.x, M = P.M;
  const int cnt = counts[b];
  const int used = cnt < 0 ? 0 : (cnt > M ? M : cnt);
  const double* aff = affine ? affine + 3 * (size_t)b : nullptr;
  const char* base = recs + (size_t)b * M * P.stride;
  int n_drawn = 0, n_skipped = 0;
  for (int t = tid; t < used; t += 256) {
    const char* rec = base + (size_t)t * P.stride;
    int X[8], A[2];
    const int st = prim_geometry(P, rec, t, used, aff, X, A);
    s_state[t] = (uint8_t)st;
    s_area[t] = reinterpret_cast<const int*>(rec)[1];
    n_drawn += st == 1;
    n_skipped += st == 2;
  }
  // the two counts of the map: wave sums, then four wave totals in LDS
  for (int o = 32; o > 0; o >>= 1) {
    n_drawn += __shfl_xor(n_drawn, o, 64);
    n_skipped += __shfl_xor(n_skipped, o, 64);
  }
  if ((tid & 63) == 0) { s_cnt[tid >> 6][0] = n_drawn; s_cnt[tid >> 6][1] = n_skipped; }
  __syncthreads();
  if (tid == 0) {
    drawn[b] = (s_cnt[0][0] + s_cnt[1][0]) + (s_cnt[2][0] + s_cnt[3][0]);
    skipped[b] = (s_cnt[0][1] + s_cnt[1][1]) + (s_cnt[2][1] + s_cnt[3][1]);
  }
  for (int t = tid; t < used; t += 256) {
    if (s_state[t] != 1) continue;
    const int area = s_area[t];
    int rank = 0;
    for (int u = 0; u < used; ++u)
      rank += (s_state[u] == 1) && (s_area[u] > area || (s_area[u] == area && u < t));
    const char* rec = base + (size_t)t * P.stride;
    int X[8], A[2];
    prim_geometry(P, rec, t, used, aff, X, A);
    vk_render_prim* __restrict__ r = prims + ((size_t)b * M + rank);
    r->rank = rank;
    r->slot = t;
#pragma unroll
    for (int q = 0; q < 8; ++q) r->corner[q] = X[q];
    r->anchor[0] = A[0];
    r->anchor[1] = A[1];
    // the first diagonal: the first pair of largest squared distance
    long long best = -1;
    int bp = 0;
#pragma unroll
    for (int p = 0; p < 6; ++p) {
      const int i = pair_i(p), j = pair_j(p);
      const long long dx = (long long)X[2 * i] - X[2 * j], dy = (long long)X[2 * i + 1] - X[2 * j + 1];
      const long long d2 = dx * dx + dy * dy;
      if (d2 > best) { best = d2; bp = p; }
    }
    r->diag[0] = (uint8_t)pair_i(bp); r->diag[1] = (uint8_t)pair_j(bp); r->diag[2] = (uint8_t)pair_i(5 - bp); r->diag[3] = (uint8_t)pair_j(5 - bp);
    const int pal = rank & 7;
#pragma unroll
    for (int c = 0; c < 3; ++c) { r->color[c] = P.style.palette[pal][c]; r->diag_color[c] = P.style.diag[c]; }
    r->thickness = (uint8_t)P.style.thickness;
    r->text_scale = (uint8_t)P.style.text_scale;
    r->pad[0] = r->pad[1] = r->pad[2] = 0;
    const double d = *reinterpret_cast<const double*>(rec + P.diag_off);
    const int len = make_label(r->label, rank + 1, d);
    r->label_len = (uint8_t)len;
    const int pad = (P.style.thickness + 1) / 2, ts = P.style.text_scale;
    int x0 = X[0], x1 = X[0], y0 = X[1], y1 = X[1];
#pragma unroll
    for (int q = 1; q < 4; ++q) {
      x0 = min(x0, X[2 * q]); x1 = max(x1, X[2 * q]);
      y0 = min(y0, X[2 * q + 1]); y1 = max(y1, X[2 * q + 1]);
    }
    r->bbox[0] = min(x0 - pad, A[0]);
    r->bbox[1] = min(y0 - pad, A[1] - 7 * ts + 1);
    r->bbox[2] = max(x1 + pad, A[0] + 6 * ts * len - 1);
    r->bbox[3] = max(y1 + pad, A[1]);
  }
}

// ------------------------------------------------------------------------------------------------ draw
__device__ __forceinline__ bool seg_covers(long long px, long long py, long long ax, long long ay, long long bx, long long by, long long tt) {
  const long long dx = bx - ax, dy = by - ay, ex = px - ax, ey = py - ay;
  const long long L = dx * dx + dy * dy, u = ex * dx + ey * dy;
  if (L == 0 || u <= 0) return 4 * (ex * ex + ey * ey) <= tt;
  if (u >= L) {
    const long long fx = px - bx, fy = py - by;
    return 4 * (fx * fx + fy * fy) <= tt;
  }
  long long cr = dx * ey - dy * ex;
  cr = cr < 0 ? -cr : cr;
  if (cr >= (1ll << 26)) return false;                                     // 4 cr^2 >= 2^54 > 64 * 2^43 >= tt * L
  return 4 * cr * cr <= tt * L;
}

__device__ __forceinline__ bool prim_ok(const vk_render_prim& p) {
  bool ok = p.thickness >= 1 && p.thickness <= 8 && p.text_scale >= 1 && p.text_scale <= 8 && p.label_len <= VK_RENDER_LABEL_MAX;
#pragma unroll
  for (int q = 0; q < 4; ++q) ok = ok && p.diag[q] < 4;
#pragma unroll
  for (int q = 0; q < 8; ++q) ok = ok && p.corner[q] >= -VK_RENDER_MAX_COORD && p.corner[q] <= VK_RENDER_MAX_COORD;
  ok = ok && p.anchor[0] >= -2 * VK_RENDER_MAX_COORD && p.anchor[0] <= 2 * VK_RENDER_MAX_COORD;
  ok = ok && p.anchor[1] >= -2 * VK_RENDER_MAX_COORD && p.anchor[1] <= 2 * VK_RENDER_MAX_COORD;
  return ok;
}

// whether record p paints pixel (X, Y), and with which colour: the text over the diagonals over the sides
__device__ bool prim_paints(const vk_render_prim* __restrict__ p, int X, int Y, uint8_t* col) {
  if (X < p->bbox[0] || X > p->bbox[2] || Y < p->bbox[1] || Y > p->bbox[3]) return false;
  const int ts = p->text_scale, len = p->label_len;
  const int u = X - p->anchor[0], v = Y - (p->anchor[1] - 7 * ts + 1);
  if (u >= 0 && v >= 0 && v < 7 * ts && u < 6 * ts * len) {
    const int cell = u / ts, row = v / ts, k = cell / 6, c = cell - 6 * k;
    const int g = glyph_index(p->label[k]);
    if (c < 5 && g >= 0 && ((d_glyph[g][row] >> (4 - c)) & 1)) {
      col[0] = p->color[0]; col[1] = p->color[1]; col[2] = p->color[2];
      return true;
    }
  }
  const long long tt = (long long)p->thickness * p->thickness;
  const int* C = p->corner;
  const int a = p->diag[0], b = p->diag[1], c = p->diag[2], d = p->diag[3];
  if (seg_covers(X, Y, C[2 * a], C[2 * a + 1], C[2 * b], C[2 * b + 1], tt) || seg_covers(X, Y, C[2 * c], C[2 * c + 1], C[2 * d], C[2 * d + 1], tt)) {
    col[0] = p->diag_color[0]; col[1] = p->diag_color[1]; col[2] = p->diag_color[2];
    return true;
  }
  for (int q = 0; q < 4; ++q) {
    const int q1 = (q + 1) & 3;
    if (seg_covers(X, Y, C[2 * q], C[2 * q + 1], C[2 * q1], C[2 * q1 + 1], tt)) {
      col[0] = p->color[0]; col[1] = p->color[1]; col[2] = p->color[2];
      return true;
    }
  }
  return false;
}

struct DrawArgs {
  int mask_kind, M;
  float thresh;
  vk_render_blend bl;
};

template <bool BINNED>
__global__ __launch_bounds__(256) void k_render_draw(const vk_render_view* __restrict__ views, const DrawArgs A,
                                                     const vk_render_prim* __restrict__ prims, const int32_t* __restrict__ drawn) {
#pragma clang fp contract(off)
  __shared__ uint16_t s_list[BINNED ? RN_MAX_M : 1];
  __shared__ int s_wave[4];
  const int b = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const vk_render_view V = views[b];
  const int xs = blockIdx.x * RT_W, ys = blockIdx.y * RT_H;
  if (xs >= V.w || ys >= V.h) return;                                       // uniform over the workgroup
  int n = 0;
  if (prims) {
    n = drawn[b];
    n = n < 0 ? 0 : (n > A.M ? A.M : n);
  }
  const vk_render_prim* P = prims + (size_t)b * A.M;
  int listed = 0;
  if constexpr (BINNED) {
    for (int c0 = 0; c0 < n; c0 += 256) {
      const int i = c0 + tid;
      bool have = false;
      if (i < n) {
        const vk_render_prim p = P[i];
        have = prim_ok(p) && p.bbox[0] <= xs + RT_W - 1 && p.bbox[2] >= xs && p.bbox[1] <= ys + RT_H - 1 && p.bbox[3] >= ys;
      }
      const unsigned long long m = __ballot(have);
      if (lane == 0) s_wave[wave] = __popcll(m);
      __syncthreads();
      int before = listed, chunk = 0;
      for (int k = 0; k < 4; ++k) {
        if (k < wave) before += s_wave[k];
        chunk += s_wave[k];
      }
      if (have) s_list[before + __popcll(m & ((1ull << lane) - 1ull))] = (uint16_t)i;
      listed += chunk;
      __syncthreads();                                                     // s_wave is written again by the next chunk
    }
  }
  const int X = xs + (tid & (RT_W - 1)), Y = ys + tid / RT_W;
  if (X >= V.w || Y >= V.h) return;
  uint8_t col[3] = {0, 0, 0};
  bool hit = false;
  if constexpr (BINNED) {
    for (int k = listed - 1; k >= 0 && !hit; --k) hit = prim_paints(P + s_list[k], X, Y, col);
  } else {
    for (int k = n - 1; k >= 0 && !hit; --k) hit = prim_ok(P[k]) && prim_paints(P + k, X, Y, col);
  }
  const uint8_t* sp = reinterpret_cast<const uint8_t*>(V.src) + (size_t)Y * (size_t)V.src_stride + 3 * (size_t)X;
  const uint8_t s0 = sp[0], s1 = sp[1], s2 = sp[2];
  bool fg;
  if (A.mask_kind == VK_RENDER_MASK_U8) {
    fg = reinterpret_cast<const uint8_t*>(V.mask)[(size_t)Y * (size_t)V.mask_stride + X] != 0;
  } else {
    const float pv = *reinterpret_cast<const float*>(reinterpret_cast<const uint8_t*>(V.mask) + (size_t)Y * (size_t)V.mask_stride + 4 * (size_t)X);
    fg = pv > A.thresh;
  }
  if (V.out[0]) {
    uint8_t* o = reinterpret_cast<uint8_t*>(V.out[0]) + (size_t)Y * (size_t)V.out_stride[0] + 3 * (size_t)X;
    o[0] = hit ? col[0] : s0; o[1] = hit ? col[1] : s1; o[2] = hit ? col[2] : s2;
  }
  if (V.out[1]) {
    uint8_t* o = reinterpret_cast<uint8_t*>(V.out[1]) + (size_t)Y * (size_t)V.out_stride[1] + 3 * (size_t)X;
    const uint8_t m = fg ? 255 : 0;
    o[0] = hit ? col[0] : m; o[1] = hit ? col[1] : m; o[2] = hit ? col[2] : m;
  }
  if (V.out[2]) {
    uint8_t* o = reinterpret_cast<uint8_t*>(V.out[2]) + (size_t)Y * (size_t)V.out_stride[2] + 3 * (size_t)X;
    if (hit) {
      o[0] = col[0]; o[1] = col[1]; o[2] = col[2];
    } else {
      o[0] = blend_u8(s0, fg ? A.bl.color[0] : (uint8_t)0, A.bl.alpha, A.bl.beta, A.bl.gamma);
      o[1] = blend_u8(s1, fg ? A.bl.color[1] : (uint8_t)0, A.bl.alpha, A.bl.beta, A.bl.gamma);
      o[2] = blend_u8(s2, fg ? A.bl.color[2] : (uint8_t)0, A.bl.alpha, A.bl.beta, A.bl.gamma);
    }
  }
}

// ------------------------------------------------------------------------------------------------ reduce
__global__ __launch_bounds__(256) void k_render_reduce(int h, int w, int k, const uint8_t* __restrict__ src, long long sstride,
                                                       uint8_t* __restrict__ dst, long long dstride) {
  const int oh = (h + k - 1) / k, ow = (w + k - 1) / k;
  const int X = blockIdx.x * RT_W + (threadIdx.x & (RT_W - 1)), Y = blockIdx.y * RT_H + threadIdx.x / RT_W;
  if (X >= ow || Y >= oh) return;
  const int y0 = Y * k, x0 = X * k, y1 = min(y0 + k, h), x1 = min(x0 + k, w);
  int s[3] = {0, 0, 0};
  for (int y = y0; y < y1; ++y) {
    const uint8_t* row = src + (size_t)y * (size_t)sstride;
    for (int x = x0; x < x1; ++x) {
      const uint8_t* p = row + 3 * (size_t)x;
      s[0] += p[0]; s[1] += p[1]; s[2] += p[2];
    }
  }
  const int n = (y1 - y0) * (x1 - x0);
  uint8_t* o = dst + (size_t)Y * (size_t)dstride + 3 * (size_t)X;
  o[0] = (uint8_t)((s[0] + n / 2) / n);
  o[1] = (uint8_t)((s[1] + n / 2) / n);
  o[2] = (uint8_t)((s[2] + n / 2) / n);
}

}  // namespace vk

using namespace vk;

static bool finite_weight(float v) { return v >= -1.0e6f && v <= 1.0e6f; }

static int render_check_blend(const char* who, const vk_render_blend* bl) {
  VK_CHECK_ARG(bl, "%s: null blend", who);
  VK_CHECK_ARG(finite_weight(bl->alpha) && finite_weight(bl->beta) && finite_weight(bl->gamma),
               "%s: blend weights alpha = %g, beta = %g, gamma = %g outside [-1e6, 1e6]", who, (double)bl->alpha, (double)bl->beta, (double)bl->gamma);
  return VK_OK;
}

extern "C" int vk_render_glyph(int ch, uint8_t rows[7]) {
  VK_CHECK_ARG(rows, "vk_render_glyph: null rows");
  const int g = glyph_index(ch);
  VK_CHECK_ARG(g >= 0, "vk_render_glyph: no glyph for character %d", ch);
  for (int r = 0; r < 7; ++r) rows[r] = h_glyph[g][r];
  return VK_OK;
}

extern "C" int vk_render_val_panels(int N, int H, int W, const float* x, const float* y, const float* prob, const double* mean, const double* stdv,
                                    const vk_render_blend* blend, int flags, uint8_t* out, int64_t row_stride, void* stream) {
  VK_CHECK_ARG(N >= 1 && N <= 65535, "vk_render_val_panels: N = %d outside 1..65535", N);
  VK_CHECK_ARG(H >= 1 && H <= 16384 && W >= 1 && W <= 16384, "vk_render_val_panels: size %dx%d outside 1..16384", H, W);
  VK_CHECK_ARG(x && y && prob && mean && stdv && out, "vk_render_val_panels: null buffer");
  VK_CHECK_ARG((((uintptr_t)x | (uintptr_t)y | (uintptr_t)prob) & 3) == 0, "vk_render_val_panels: misaligned buffer");
  if (int rc = render_check_blend("vk_render_val_panels", blend)) return rc;
  VK_CHECK_ARG((flags & ~VK_RENDER_RGB) == 0, "vk_render_val_panels: unknown flags 0x%x", flags);
  VK_CHECK_ARG(row_stride >= 12 * (int64_t)W && row_stride <= ((int64_t)1 << 31), "vk_render_val_panels: row stride %lld below 12 * W",
               (long long)row_stride);
  PanelArgs A;
  for (int k = 0; k < 3; ++k) {
    VK_CHECK_ARG(fabs(mean[k]) <= 1.0e6 && fabs(stdv[k]) <= 1.0e6, "vk_render_val_panels: mean / std of channel %d is not finite", k);
    A.mean[k] = mean[k];
    A.stdv[k] = stdv[k];
  }
  A.bl = *blend;
  hipStream_t st = (hipStream_t)stream;
  vkh::ProfScope ps_("render_panels", st, 0.0, (double)N * H * W * (20.0 + 12.0));
  const dim3 grid((W + RT_W - 1) / RT_W, (H + RT_H - 1) / RT_H, N);
  hipLaunchKernelGGL(k_render_panels, grid, dim3(256), 0, st, H, W, x, y, prob, A, flags & VK_RENDER_RGB, out, (long long)row_stride);
  VK_CHECK_HIP(hipGetLastError());
  return VK_OK;
}

extern "C" int vk_render_primitives(int batch, const void* records, size_t record_stride, size_t box_offset, int valid_offset, int diag_offset,
                                    int center_offset, int coord_mode, const int32_t* counts, int max_components, const double* affine,
                                    const vk_render_style* style, vk_render_prim* prims, int32_t* drawn, int32_t* skipped, void* stream) {
  VK_CHECK_ARG(batch >= 1 && batch <= 65535, "vk_render_primitives: batch %d outside 1..65535", batch);
  VK_CHECK_ARG(max_components >= 1 && max_components <= RN_MAX_M, "vk_render_primitives: max_components = %d outside 1..4096", max_components);
  VK_CHECK_ARG(coord_mode == VK_RENDER_COORD_BOX || coord_mode == VK_RENDER_COORD_V || coord_mode == VK_RENDER_COORD_VS,
               "vk_render_primitives: unknown coordinate mode %d", coord_mode);
  VK_CHECK_ARG(records && counts && style && prims && drawn && skipped, "vk_render_primitives: null buffer");
  const size_t box_bytes = coord_mode == VK_RENDER_COORD_BOX ? 32 : 64, box_align = coord_mode == VK_RENDER_COORD_BOX ? 4 : 8;
  VK_CHECK_ARG(record_stride % 8 == 0 && box_offset % box_align == 0 && box_offset >= 8 && box_offset + box_bytes <= record_stride,
               "vk_render_primitives: record stride %zu / box offset %zu: a stride that is a multiple of 8 with label, area and the corners inside "
               "the record", record_stride, box_offset);
  VK_CHECK_ARG(valid_offset == -1 || (valid_offset >= 8 && valid_offset % 4 == 0 && (size_t)valid_offset + 4 <= record_stride),
               "vk_render_primitives: valid offset %d is neither -1 nor an int inside the record", valid_offset);
  VK_CHECK_ARG(diag_offset >= 8 && diag_offset % 8 == 0 && (size_t)diag_offset + 8 <= record_stride,
               "vk_render_primitives: diag offset %d is not a double inside the record", diag_offset);
  if (coord_mode == VK_RENDER_COORD_BOX)
    VK_CHECK_ARG(center_offset >= 8 && center_offset % 4 == 0 && (size_t)center_offset + 8 <= record_stride,
                 "vk_render_primitives: center offset %d is not two floats inside the record", center_offset);
  VK_CHECK_ARG(style->thickness >= 1 && style->thickness <= 8, "vk_render_primitives: thickness = %d outside 1..8", style->thickness);
  VK_CHECK_ARG(style->text_scale >= 1 && style->text_scale <= 8, "vk_render_primitives: text_scale = %d outside 1..8", style->text_scale);
  VK_CHECK_ARG((((uintptr_t)counts | (uintptr_t)drawn | (uintptr_t)skipped) & 3) == 0 &&
                   (((uintptr_t)records | (uintptr_t)prims | (uintptr_t)affine) & 7) == 0,
               "vk_render_primitives: misaligned buffer");
  PrimArgs P;
  P.stride = record_stride; P.box_off = box_offset; P.valid_off = valid_offset; P.diag_off = diag_offset; P.center_off = center_offset;
  P.mode = coord_mode; P.M = max_components; P.style = *style;
  hipStream_t st = (hipStream_t)stream;
  vkh::ProfScope ps_("render_prims", st, 0.0, (double)batch * (double)max_components * (double)(record_stride + sizeof(vk_render_prim)));
  hipLaunchKernelGGL(k_render_prims, dim3(batch), dim3(256), 0, st, P, (const char*)records, counts, affine, prims, drawn, skipped);
  VK_CHECK_HIP(hipGetLastError());
  return VK_OK;
}

extern "C" int vk_render_draw(int batch, const vk_render_view* views_host, void* views_dev, int mask_kind, float thresh,
                              const vk_render_blend* blend, const vk_render_prim* prims, const int32_t* drawn, int max_components, int flags,
                              void* stream) {
  VK_CHECK_ARG(batch >= 1 && batch <= 65535, "vk_render_draw: batch %d outside 1..65535", batch);
  VK_CHECK_ARG(views_host && views_dev, "vk_render_draw: null buffer");
  VK_CHECK_ARG(((uintptr_t)views_dev & 7) == 0, "vk_render_draw: misaligned buffer");
  VK_CHECK_ARG(mask_kind == VK_RENDER_MASK_U8 || mask_kind == VK_RENDER_MASK_F32, "vk_render_draw: unknown mask kind %d", mask_kind);
  VK_CHECK_ARG(mask_kind == VK_RENDER_MASK_U8 || thresh == thresh, "vk_render_draw: thresh is not a number");
  if (int rc = render_check_blend("vk_render_draw", blend)) return rc;
  VK_CHECK_ARG((flags & ~VK_RENDER_DIRECT) == 0, "vk_render_draw: unknown flags 0x%x", flags);
  if (prims) {
    VK_CHECK_ARG(drawn, "vk_render_draw: null buffer: a primitive list without its counts");
    VK_CHECK_ARG(max_components >= 1 && max_components <= RN_MAX_M, "vk_render_draw: max_components = %d outside 1..4096", max_components);
    VK_CHECK_ARG(((uintptr_t)prims & 7) == 0 && ((uintptr_t)drawn & 3) == 0, "vk_render_draw: misaligned buffer");
  }
  int max_h = 0, max_w = 0;
  double bytes = 0.0;
  for (int i = 0; i < batch; ++i) {
    const vk_render_view& v = views_host[i];
    VK_CHECK_ARG(v.h >= 1 && v.h <= 16384 && v.w >= 1 && v.w <= 16384, "vk_render_draw: map %d: size %dx%d outside 1..16384", i, v.h, v.w);
    VK_CHECK_ARG(v.src != 0 && v.mask != 0, "vk_render_draw: map %d: null address", i);
    VK_CHECK_ARG(v.src_stride >= 3 * (int64_t)v.w && v.src_stride <= ((int64_t)1 << 31), "vk_render_draw: map %d: row stride %lld below 3 * w", i,
                 (long long)v.src_stride);
    const int64_t mb = mask_kind == VK_RENDER_MASK_U8 ? 1 : 4;
    VK_CHECK_ARG(v.mask_stride >= mb * v.w && v.mask_stride <= ((int64_t)1 << 31) && v.mask_stride % mb == 0 && v.mask % (uint64_t)mb == 0,
                 "vk_render_draw: map %d: mask row stride %lld below the row or misaligned", i, (long long)v.mask_stride);
    int wanted = 0;
    for (int o = 0; o < 3; ++o) {
      if (!v.out[o]) continue;
      ++wanted;
      VK_CHECK_ARG(v.out_stride[o] >= 3 * (int64_t)v.w && v.out_stride[o] <= ((int64_t)1 << 31),
                   "vk_render_draw: map %d: output %d: row stride %lld below 3 * w", i, o, (long long)v.out_stride[o]);
    }
    VK_CHECK_ARG(wanted > 0, "vk_render_draw: map %d: no output wanted", i);
    max_h = v.h > max_h ? v.h : max_h;
    max_w = v.w > max_w ? v.w : max_w;
    bytes += (double)v.h * v.w * (3.0 + (double)mb + 3.0 * wanted);
  }
  hipStream_t st = (hipStream_t)stream;
  VK_CHECK_HIP(hipMemcpyAsync(views_dev, views_host, (size_t)batch * sizeof(vk_render_view), hipMemcpyHostToDevice, st));
  DrawArgs A;
  A.mask_kind = mask_kind; A.M = prims ? max_components : 0; A.thresh = thresh; A.bl = *blend;
  vkh::ProfScope ps_((flags & VK_RENDER_DIRECT) ? "render_draw_direct" : "render_draw", st, 0.0, bytes);
  const dim3 grid((max_w + RT_W - 1) / RT_W, (max_h + RT_H - 1) / RT_H, batch);
  if (flags & VK_RENDER_DIRECT)
    hipLaunchKernelGGL(k_render_draw<false>, grid, dim3(256), 0, st, (const vk_render_view*)views_dev, A, prims, drawn);
  else
    hipLaunchKernelGGL(k_render_draw<true>, grid, dim3(256), 0, st, (const vk_render_view*)views_dev, A, prims, drawn);
  VK_CHECK_HIP(hipGetLastError());
  return VK_OK;
}

extern "C" int vk_render_reduce(int h, int w, int k, const uint8_t* src, int64_t src_stride, uint8_t* dst, int64_t dst_stride, void* stream) {
  VK_CHECK_ARG(h >= 1 && h <= 16384 && w >= 1 && w <= 16384, "vk_render_reduce: size %dx%d outside 1..16384", h, w);
  VK_CHECK_ARG(k >= 1 && k <= 16, "vk_render_reduce: k = %d outside 1..16", k);
  VK_CHECK_ARG(src && dst, "vk_render_reduce: null buffer");
  const int ow = (w + k - 1) / k;
  VK_CHECK_ARG(src_stride >= 3 * (int64_t)w && src_stride <= ((int64_t)1 << 31), "vk_render_reduce: source row stride %lld below 3 * w",
               (long long)src_stride);
  VK_CHECK_ARG(dst_stride >= 3 * (int64_t)ow && dst_stride <= ((int64_t)1 << 31), "vk_render_reduce: output row stride %lld below 3 * ceil(w / k)",
               (long long)dst_stride);
  const int oh = (h + k - 1) / k;
  hipStream_t st = (hipStream_t)stream;
  vkh::ProfScope ps_("render_reduce", st, 0.0, 3.0 * ((double)h * w + (double)oh * ow));
  const dim3 grid((ow + RT_W - 1) / RT_W, (oh + RT_H - 1) / RT_H, 1);
  hipLaunchKernelGGL(k_render_reduce, grid, dim3(256), 0, st, h, w, k, src, (long long)src_stride, dst, (long long)dst_stride);
  VK_CHECK_HIP(hipGetLastError());
  return VK_OK;
}
