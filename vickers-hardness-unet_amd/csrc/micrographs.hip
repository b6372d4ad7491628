// Synthetic micrographs on the device: vk_mg_render fills the uint8 pixel and mask buffers vk_augment_batch reads from
// fixed-layout scene records, so a training step can be fed without a dataset and every mask and diagonal is known exactly.
//
//   k_mg_render : one launch; a workgroup (256 lanes) owns a 64 x 16 tile of one image.
//        1. the image's vk_mg_scene (3,200 bytes) goes into LDS once, and wave 0 lists the scratches that can touch the tile at all (one
//           per lane, compacted with a ballot): a scratch crosses about one tile in six;
//        2. the ideal (unblurred) image is evaluated over the tile and its 3-pixel apron, 70 x 22 pixels, as 25 pieces: 22 row pieces of
//           64 pixels and 3 pieces of the 6 x 22 strip on the right; a wave takes every fourth piece.  A piece is a rectangle that is the
//           same in every lane, so "this record cannot touch my pixels" is decided on values read through readfirstlane: a scratch by the
//           sign and size of its (affine) cross product at the rectangle's corners, a blob or an indentation by its box.  A record that
//           misses costs a few scalar instructions; the int64 products run only where a record can hit;
//        3. the binomial rows, then columns, out of LDS (as k_cp_alpha of copypaste.hip); seven taps with zero weights below radius 3;
//        4. noise, rects, stores: 4 pixels per lane with three 4-byte stores of pixels and one of mask where S % 4 == 0, bytes otherwise.
//        Every output byte is written exactly once; no atomics, no workspace but the record scratch.
//   LDS per workgroup: scene 3,200 + ideal 3 x 22 x 72 = 4,752 + mask 16 x 64 = 1,024 + row sums 3 x 22 x 64 x 2 = 8,448 + scratch list 68 = 17,492 bytes:
//        nine workgroups fit the 160 KiB of a compute unit, more than its 32 wave slots hold (eight), so LDS does not bound occupancy.
// All arithmetic is integer and follows tests/micrographs_ref.py: the outputs are the same bytes.
#include "vk_common.h"

namespace vk {

static_assert(sizeof(vk_mg_scene) == 3200 && sizeof(vk_mg_indent) == 96 && sizeof(vk_mg_scratch) == 32, "vk_mg_scene layout");
constexpr int MG_SCENE_INTS = sizeof(vk_mg_scene) / 4;
constexpr int MG_W = 64, MG_H = 16, MG_R = 3;
constexpr int MG_TW = MG_W + 2 * MG_R, MG_TH = MG_H + 2 * MG_R;          // 70 x 22 with the apron
constexpr int MG_PITCH = 72;
constexpr int MG_ROW_PIECES = MG_TH;                                     // 64 pixels of one row each
constexpr int MG_SIDE_PER = 64 / (2 * MG_R);                             // rows of the 6-pixel strip one piece holds: 10
constexpr int MG_SIDE_PIECES = (MG_TH + MG_SIDE_PER - 1) / MG_SIDE_PER;  // 3

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int64_t cr64(int ax, int ay, int bx, int by) { return (int64_t)ax * by - (int64_t)ay * bx; }
__device__ __forceinline__ int64_t sq64(int a) { return (int64_t)a * a; }
__device__ __forceinline__ uint32_t mg_mix(uint32_t h) {
  h ^= h >> 16; h *= 0x7feb352du; h ^= h >> 15; h *= 0x846ca68bu; h ^= h >> 16;
  return h;
}
__device__ __forceinline__ int mg_lattice(int i, int j, uint32_t seed) {
  return (int)(mg_mix((uint32_t)i * 0x9E3779B1u + (uint32_t)j * 0x85EBCA77u + seed) & 255u);
}
// min(256, (R^2 - d2) / (R^2 >> 8)) for 0 <= d2 < R^2 <= 2^30
__device__ __forceinline__ int mg_falloff(int R2, int64_t d2) { return (int)min(256u, (uint32_t)(R2 - (int)d2) / (uint32_t)(R2 >> 8)); }

// Can the scratch touch a pixel centre of the rectangle (1/16 pixel, inclusive)?  c and t are affine in the pixel, so over the rectangle
// they take their extremes at its corners: all corners on one side of the line and further than hw, or all outside the extent: no.
__device__ __forceinline__ bool mg_scratch_may_hit(int sx, int sy, int dx, int dy, int64_t lim, int t0, int t1, int RX0, int RY0, int RX1, int RY1) {
  const int64_t c00 = cr64(RX0 - sx, RY0 - sy, dx, dy), c10 = cr64(RX1 - sx, RY0 - sy, dx, dy), c01 = cr64(RX0 - sx, RY1 - sy, dx, dy),
                c11 = cr64(RX1 - sx, RY1 - sy, dx, dy);
  const int64_t cmin = min(min(c00, c10), min(c01, c11)), cmax = max(max(c00, c10), max(c01, c11));
  if (cmin > 0 && cmin * cmin > lim) return false;
  if (cmax < 0 && cmax * cmax > lim) return false;
  const int64_t a00 = (int64_t)(RX0 - sx) * dx + (int64_t)(RY0 - sy) * dy, a10 = (int64_t)(RX1 - sx) * dx + (int64_t)(RY0 - sy) * dy,
                a01 = (int64_t)(RX0 - sx) * dx + (int64_t)(RY1 - sy) * dy, a11 = (int64_t)(RX1 - sx) * dx + (int64_t)(RY1 - sy) * dy;
  return !(max(max(a00, a10), max(a01, a11)) < t0 || min(min(a00, a10), min(a01, a11)) > t1);
}

// The ideal level of pixel (x, y) and its mask bit.  (bx0, by0) .. (bx1, by1): the piece's rectangle in pixels, the same in every lane;
// slist[0 .. scount): the scratches that can touch the workgroup's tile at all, ascending.
__device__ __forceinline__ void mg_ideal(const vk_mg_scene& sc, const uint8_t* slist, int scount, int x, int y, int bx0, int by0, int bx1, int by1,
                                         int& L_out, int& m_out) {
  const int X = 16 * x, Y = 16 * y;
  const int RX0 = 16 * bx0, RY0 = 16 * by0, RX1 = 16 * bx1, RY1 = 16 * by1;
  int T = 0;
  const int amp = uni(sc.tex_amp);
  if (amp != 0) {
    const int c = uni(sc.tex_cos), sn = uni(sc.tex_sin), lu = uni(sc.tex_lu), lv = uni(sc.tex_lv);
    const uint32_t seed = (uint32_t)uni((int)sc.tex_seed);
    const int u = x * c + y * sn, v = y * c - x * sn;
    const int iu = u >> (14 + lu), fu = (u >> (6 + lu)) & 255, iv = v >> (14 + lv), fv = (v >> (6 + lv)) & 255;
    const int top = mg_lattice(iu, iv, seed) * (256 - fu) + mg_lattice(iu + 1, iv, seed) * fu;
    const int bot = mg_lattice(iu, iv + 1, seed) * (256 - fu) + mg_lattice(iu + 1, iv + 1, seed) * fu;
    const int val = (top * (256 - fv) + bot * fv + 32768) >> 16;
    T = ((val - 128) * amp) >> 8;
  }
  const int vdx = x - uni(sc.vig_cx), vdy = y - uni(sc.vig_cy);
  int L = uni(sc.base) + ((uni(sc.grad_x) * (x - uni(sc.grad_cx)) + uni(sc.grad_y) * (y - uni(sc.grad_cy))) >> 8) -
          ((uni(sc.vig) * (vdx * vdx + vdy * vdy)) >> 16) + T;

  for (int j = 0; j < scount; ++j) {
    const vk_mg_scratch& r = sc.scratches[uni(slist[j])];
    const int sx = uni(r.x), sy = uni(r.y), dx = uni(r.dx), dy = uni(r.dy), hw = uni(r.hw), t0 = uni(r.t0), t1 = uni(r.t1);
    const int64_t lim = sq64(hw) * (sq64(dx) + sq64(dy));
    if (!mg_scratch_may_hit(sx, sy, dx, dy, lim, t0, t1, RX0, RY0, RX1, RY1)) continue;
    const int qx = X - sx, qy = Y - sy;
    const int64_t c = cr64(qx, qy, dx, dy), t = (int64_t)qx * dx + (int64_t)qy * dy;
    if (c * c <= lim && t >= t0 && t <= t1) L += uni(r.depth);
  }

  const int nb = uni(sc.n_blobs);
  for (int k = 0; k < nb; ++k) {
    const vk_mg_blob& b = sc.blobs[k];
    const int cx = uni(b.x), cy = uni(b.y), R = uni(b.r);
    if (cx + R < RX0 || cx - R > RX1 || cy + R < RY0 || cy - R > RY1) continue;
    const int64_t d2 = sq64(X - cx) + sq64(Y - cy);
    if (d2 < sq64(R)) L -= (uni(b.dark) * mg_falloff(R * R, d2)) >> 8;
  }

  int m = 0;
  const int ni = uni(sc.n_indents);
  for (int k = 0; k < ni; ++k) {
    const vk_mg_indent& q = sc.indents[k];
    int vx[4], vy[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { vx[i] = uni(q.vx[i]); vy[i] = uni(q.vy[i]); }
    const int R = uni(q.halo_r);
    if (max(max(vx[0], vx[1]), max(vx[2], vx[3])) + R < RX0 || min(min(vx[0], vx[1]), min(vx[2], vx[3])) - R > RX1 ||
        max(max(vy[0], vy[1]), max(vy[2], vy[3])) + R < RY0 || min(min(vy[0], vy[1]), min(vy[2], vy[3])) - R > RY1)
      continue;
    const int ax = uni(q.ax), ay = uni(q.ay);
    int64_t ce[4];
    bool in = true;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = (i + 1) & 3;
      ce[i] = cr64(vx[j] - vx[i], vy[j] - vy[i], X - vx[i], Y - vy[i]);
      in = in && ce[i] >= 0;
    }
    if (in) {
      m = 1;
      const int px = X - ax, py = Y - ay;
      int64_t ca[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) ca[i] = cr64(vx[i] - ax, vy[i] - ay, px, py);
      int f = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (ca[i] >= 0 && ca[(i + 1) & 3] < 0) f = i;
      int64_t cef = ce[0];
      int fx0 = vx[0], fy0 = vy[0], fx1 = vx[1], fy1 = vy[1], shade = uni(q.shade[0]), slope = uni(q.slope[0]);
#pragma unroll
      for (int i = 1; i < 4; ++i)
        if (f == i) {
          cef = ce[i]; fx0 = vx[i]; fy0 = vy[i]; fx1 = vx[(i + 1) & 3]; fy1 = vy[(i + 1) & 3];
          shade = uni(q.shade[i]); slope = uni(q.slope[i]);
        }
      const int64_t den = cr64(fx1 - fx0, fy1 - fy0, ax - fx0, ay - fy0);          // > 0: the apex is strictly inside
      const int kk = (int)((256 * cef) / den);
      L = shade + ((slope * kk) >> 8) + (T >> 1);
      const int64_t hw2 = sq64(uni(q.ridge_hw));
      bool ridge = false;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int wx = vx[i] - ax, wy = vy[i] - ay;
        const int64_t w2 = sq64(wx) + sq64(wy), dot = (int64_t)px * wx + (int64_t)py * wy;
        ridge = ridge || (dot >= 0 && dot <= w2 && ca[i] * ca[i] <= hw2 * w2);
      }
      if (ridge) L += uni(q.ridge);
    } else if (R > 0) {
      int64_t d2 = INT64_MAX;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int j = (i + 1) & 3;
        const int ex = vx[j] - vx[i], ey = vy[j] - vy[i], px = X - vx[i], py = Y - vy[i];
        const int64_t e2 = sq64(ex) + sq64(ey), dot = (int64_t)px * ex + (int64_t)py * ey;
        int64_t d;
        if (dot <= 0) d = sq64(px) + sq64(py);
        else if (dot >= e2) d = sq64(X - vx[j]) + sq64(Y - vy[j]);
        else if (ce[i] * ce[i] >= sq64(R) * e2) d = INT64_MAX;                 // at least R from the line: no division
        else d = (ce[i] * ce[i]) / e2;
        d2 = min(d2, d);
      }
      if (d2 < sq64(R)) L -= (uni(q.halo_depth) * mg_falloff(R * R, d2)) >> 8;
    }
  }
  L_out = L;
  m_out = m;
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_mg_render(int S, const int* __restrict__ scenes, uint8_t* __restrict__ rgb, uint8_t* __restrict__ mask) {
  __shared__ int sc_raw[MG_SCENE_INTS];
  __shared__ uint8_t idl[3][MG_TH][MG_PITCH];       // the ideal image with the apron
  __shared__ uint8_t mk[MG_H][MG_W];                // the mask of the tile
  __shared__ uint16_t hs[3][MG_TH][MG_W];           // row sums: at most 255 * 64
  __shared__ uint8_t slist[VK_MG_MAX_SCRATCHES];    // the scratches that can touch this tile
  __shared__ int scount_s;
  const int n = blockIdx.z, t = threadIdx.x, lane = t & 63;
  const int wave = uni(t >> 6);
  for (int e = t; e < MG_SCENE_INTS; e += 256) sc_raw[e] = scenes[(size_t)n * MG_SCENE_INTS + e];
  __syncthreads();
  const vk_mg_scene& sc = *reinterpret_cast<const vk_mg_scene*>(sc_raw);
  const int xs = blockIdx.x * MG_W, ys = blockIdx.y * MG_H;
  // a scratch crosses a few of the tiles of an image: wave 0 tests one per lane against the tile with its apron and compacts the hits
  if (wave == 0) {
    bool hit = false;
    if (lane < sc.n_scratches) {
      const vk_mg_scratch& r = sc.scratches[lane];
      hit = mg_scratch_may_hit(r.x, r.y, r.dx, r.dy, sq64(r.hw) * (sq64(r.dx) + sq64(r.dy)), r.t0, r.t1, 16 * (xs - MG_R), 16 * (ys - MG_R),
                               16 * (xs + MG_W + MG_R - 1), 16 * (ys + MG_H + MG_R - 1));
    }
    const unsigned long long bm = __ballot(hit);
    if (hit) slist[__popcll(bm & ((1ull << lane) - 1ull))] = (uint8_t)lane;
    if (lane == 0) scount_s = __popcll(bm);
  }
  __syncthreads();
  const int scount = uni(scount_s);

  const int tint0 = uni(sc.tint[0]), tint1 = uni(sc.tint[1]), tint2 = uni(sc.tint[2]);
  for (int p = wave; p < MG_ROW_PIECES + MG_SIDE_PIECES; p += 4) {
    int rx, ry, bx0, by0, bx1, by1;
    bool active = true;
    if (p < MG_ROW_PIECES) {
      rx = lane; ry = p;
      bx0 = 0; bx1 = 63; by0 = by1 = p;
    } else {
      const int first = (p - MG_ROW_PIECES) * MG_SIDE_PER;
      ry = first + lane / (2 * MG_R); rx = MG_W + lane % (2 * MG_R);
      active = lane < MG_SIDE_PER * 2 * MG_R && ry < MG_TH;
      bx0 = MG_W; bx1 = MG_TW - 1; by0 = first; by1 = min(first + MG_SIDE_PER, MG_TH) - 1;
      if (!active) { rx = MG_W; ry = first; }
    }
    int L, m;
    mg_ideal(sc, slist, scount, xs + rx - MG_R, ys + ry - MG_R, xs + bx0 - MG_R, ys + by0 - MG_R, xs + bx1 - MG_R, ys + by1 - MG_R, L, m);
    if (active) {
      idl[0][ry][rx] = (uint8_t)min(max((L * tint0 + 128) >> 8, 0), 255);
      idl[1][ry][rx] = (uint8_t)min(max((L * tint1 + 128) >> 8, 0), 255);
      idl[2][ry][rx] = (uint8_t)min(max((L * tint2 + 128) >> 8, 0), 255);
      if (ry >= MG_R && ry < MG_R + MG_H && rx >= MG_R && rx < MG_R + MG_W) mk[ry - MG_R][rx - MG_R] = (uint8_t)m;
    }
  }
  __syncthreads();

  const int br = uni(sc.blur_r);
  int w[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) w[k] = 0;
  if (br == 0) { w[3] = 1; }
  else if (br == 1) { w[2] = 1; w[3] = 2; w[4] = 1; }
  else if (br == 2) { w[1] = 1; w[2] = 4; w[3] = 6; w[4] = 4; w[5] = 1; }
  else { w[0] = 1; w[1] = 6; w[2] = 15; w[3] = 20; w[4] = 15; w[5] = 6; w[6] = 1; }
  for (int e = t; e < 3 * MG_TH * MG_W; e += 256) {
    const int c = e / (MG_TH * MG_W), rem = e - c * (MG_TH * MG_W), ry = rem >> 6, cx = rem & 63;
    const uint8_t* r = &idl[c][ry][cx];
    int acc = 0;
#pragma unroll
    for (int k = 0; k < 7; ++k)
      if (k >= MG_R - br && k <= MG_R + br) acc += w[k] * r[k];
    hs[c][ry][cx] = (uint16_t)acc;
  }
  __syncthreads();

  const int ly = t >> 4, lx = (t & 15) * 4;
  const int gy = ys + ly, gx = xs + lx;
  if (gy >= S || gx >= S) return;
  const int npx = VEC ? 4 : min(4, S - gx);
  const int shift = 4 * br, half = (1 << shift) >> 1;
  const int namp = uni(sc.noise_amp), nr = uni(sc.n_rects);
  const uint32_t nseed = (uint32_t)uni((int)sc.noise_seed);
  uint32_t b[12], mb[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int x = gx + q;
    int v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      int acc = 0;
#pragma unroll
      for (int k = 0; k < 7; ++k)
        if (k >= MG_R - br && k <= MG_R + br) acc += w[k] * hs[c][ly + k][lx + q];
      v[c] = (acc + half) >> shift;
      if (namp != 0) {
        const uint32_t h = mg_mix((uint32_t)(((uint32_t)gy * (uint32_t)S + (uint32_t)x) * 3u + (uint32_t)c) * 0x9E3779B1u + nseed);
        const int tt = (int)((h & 255u) + ((h >> 8) & 255u) + ((h >> 16) & 255u) + (h >> 24)) - 510;
        v[c] = min(max(v[c] + ((tt * namp + 128) >> 8), 0), 255);
      }
    }
    for (int k = 0; k < nr; ++k) {
      const vk_mg_rect& r = sc.rects[k];
      const int x0 = uni(r.x0), y0 = uni(r.y0), x1 = uni(r.x1), y1 = uni(r.y1), th = uni(r.thickness);
      if (gy < y0 || gy > y1 || x < x0 || x > x1) continue;
      if (th > 0 && x >= x0 + th && x <= x1 - th && gy >= y0 + th && gy <= y1 - th) continue;
      v[0] = uni(r.color[0]); v[1] = uni(r.color[1]); v[2] = uni(r.color[2]);
    }
    b[3 * q] = (uint32_t)v[0] & 255u; b[3 * q + 1] = (uint32_t)v[1] & 255u; b[3 * q + 2] = (uint32_t)v[2] & 255u;
    mb[q] = mk[ly][lx + q];
  }
  const size_t dst = ((size_t)n * S + gy) * S + gx;
  if (VEC) {
    uint32_t* o = (uint32_t*)(rgb + dst * 3);
    o[0] = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
    o[1] = b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24);
    o[2] = b[8] | (b[9] << 8) | (b[10] << 16) | (b[11] << 24);
    *(uint32_t*)(mask + dst) = mb[0] | (mb[1] << 8) | (mb[2] << 16) | (mb[3] << 24);
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (q < npx) {
        uint8_t* o = rgb + (dst + q) * 3;
        o[0] = (uint8_t)b[3 * q]; o[1] = (uint8_t)b[3 * q + 1]; o[2] = (uint8_t)b[3 * q + 2];
        mask[dst + q] = (uint8_t)mb[q];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ host checks
static bool mg_in(int64_t v, int64_t lo, int64_t hi) { return v >= lo && v <= hi; }
static int64_t mg_cr(int64_t ax, int64_t ay, int64_t bx, int64_t by) { return ax * by - ay * bx; }

static int mg_check_scene(int k, int S, const vk_mg_scene& s) {
  const int64_t lo = -VK_MG_COORD_MARGIN, hi = 16 * (int64_t)S + VK_MG_COORD_MARGIN;
  VK_CHECK_ARG(s.n_indents >= 0 && s.n_indents <= VK_MG_MAX_INDENTS, "vk_mg_render: scene %d: %d indentations, limit %d", k, s.n_indents,
               VK_MG_MAX_INDENTS);
  VK_CHECK_ARG(s.n_scratches >= 0 && s.n_scratches <= VK_MG_MAX_SCRATCHES, "vk_mg_render: scene %d: %d scratches, limit %d", k, s.n_scratches,
               VK_MG_MAX_SCRATCHES);
  VK_CHECK_ARG(s.n_blobs >= 0 && s.n_blobs <= VK_MG_MAX_BLOBS, "vk_mg_render: scene %d: %d blobs, limit %d", k, s.n_blobs, VK_MG_MAX_BLOBS);
  VK_CHECK_ARG(s.n_rects >= 0 && s.n_rects <= VK_MG_MAX_RECTS, "vk_mg_render: scene %d: %d rects, limit %d", k, s.n_rects, VK_MG_MAX_RECTS);
  VK_CHECK_ARG(s.blur_r >= 0 && s.blur_r <= 3, "vk_mg_render: scene %d: blur radius %d outside 0..3", k, s.blur_r);
  VK_CHECK_ARG(mg_in(s.base, -1024, 1024) && mg_in(s.tint[0], 0, 1024) && mg_in(s.tint[1], 0, 1024) && mg_in(s.tint[2], 0, 1024),
               "vk_mg_render: scene %d: background level or tint out of range", k);
  VK_CHECK_ARG(mg_in(s.grad_x, -1024, 1024) && mg_in(s.grad_y, -1024, 1024) && mg_in(s.grad_cx, -512, S + 512) && mg_in(s.grad_cy, -512, S + 512),
               "vk_mg_render: scene %d: gradient out of range", k);
  VK_CHECK_ARG(mg_in(s.vig, 0, 255) && mg_in(s.vig_cx, -512, S + 512) && mg_in(s.vig_cy, -512, S + 512), "vk_mg_render: scene %d: vignette out of range", k);
  VK_CHECK_ARG(mg_in(s.tex_amp, -1024, 1024) && mg_in(s.tex_cos, -16384, 16384) && mg_in(s.tex_sin, -16384, 16384) && mg_in(s.tex_lu, 0, 8) &&
                   mg_in(s.tex_lv, 0, 8),
               "vk_mg_render: scene %d: texture out of range", k);
  VK_CHECK_ARG(mg_in(s.noise_amp, 0, 255), "vk_mg_render: scene %d: noise amplitude %d outside 0..255", k, s.noise_amp);
  for (int i = 0; i < s.n_indents; ++i) {
    const vk_mg_indent& q = s.indents[i];
    for (int j = 0; j < 4; ++j)
      VK_CHECK_ARG(mg_in(q.vx[j], lo, hi) && mg_in(q.vy[j], lo, hi), "vk_mg_render: scene %d indentation %d: vertex %d (%d, %d) outside [%d, %d]", k, i,
                   j, q.vx[j], q.vy[j], (int)lo, (int)hi);
    for (int j = 0; j < 4; ++j) {
      const int a = (j + 1) & 3, b = (j + 2) & 3;
      VK_CHECK_ARG(mg_cr(q.vx[a] - (int64_t)q.vx[j], q.vy[a] - (int64_t)q.vy[j], q.vx[b] - (int64_t)q.vx[a], q.vy[b] - (int64_t)q.vy[a]) > 0,
                   "vk_mg_render: scene %d indentation %d: not convex and clockwise at vertex %d", k, i, a);
    }
    for (int j = 0; j < 4; ++j) {
      const int a = (j + 1) & 3;
      VK_CHECK_ARG(mg_cr(q.vx[a] - (int64_t)q.vx[j], q.vy[a] - (int64_t)q.vy[j], q.ax - (int64_t)q.vx[j], q.ay - (int64_t)q.vy[j]) > 0,
                   "vk_mg_render: scene %d indentation %d: apex (%d, %d) not strictly inside", k, i, q.ax, q.ay);
    }
    for (int j = 0; j < 4; ++j)
      VK_CHECK_ARG(mg_in(q.shade[j], -1024, 1024) && mg_in(q.slope[j], -1024, 1024), "vk_mg_render: scene %d indentation %d: facet %d level out of range",
                   k, i, j);
    VK_CHECK_ARG(mg_in(q.ridge, -1024, 1024) && mg_in(q.ridge_hw, 0, 32767), "vk_mg_render: scene %d indentation %d: ridge out of range", k, i);
    VK_CHECK_ARG((q.halo_r == 0 || mg_in(q.halo_r, 16, 32767)) && mg_in(q.halo_depth, -1024, 1024),
                 "vk_mg_render: scene %d indentation %d: halo out of range", k, i);
  }
  for (int i = 0; i < s.n_scratches; ++i) {
    const vk_mg_scratch& r = s.scratches[i];
    VK_CHECK_ARG(mg_in(r.x, lo, hi) && mg_in(r.y, lo, hi), "vk_mg_render: scene %d scratch %d: point (%d, %d) outside [%d, %d]", k, i, r.x, r.y, (int)lo,
                 (int)hi);
    VK_CHECK_ARG(mg_in(r.dx, -16384, 16384) && mg_in(r.dy, -16384, 16384) && (r.dx != 0 || r.dy != 0), "vk_mg_render: scene %d scratch %d: direction (%d, %d)",
                 k, i, r.dx, r.dy);
    VK_CHECK_ARG(mg_in(r.hw, 0, 32767) && mg_in(r.depth, -255, 255), "vk_mg_render: scene %d scratch %d: half width or depth out of range", k, i);
  }
  for (int i = 0; i < s.n_blobs; ++i) {
    const vk_mg_blob& b = s.blobs[i];
    VK_CHECK_ARG(mg_in(b.x, lo, hi) && mg_in(b.y, lo, hi), "vk_mg_render: scene %d blob %d: centre (%d, %d) outside [%d, %d]", k, i, b.x, b.y, (int)lo,
                 (int)hi);
    VK_CHECK_ARG(mg_in(b.r, 16, 32767) && mg_in(b.dark, -1024, 1024), "vk_mg_render: scene %d blob %d: radius or darkness out of range", k, i);
  }
  for (int i = 0; i < s.n_rects; ++i) {
    const vk_mg_rect& r = s.rects[i];
    VK_CHECK_ARG(mg_in(r.x0, -4096, 4096) && mg_in(r.y0, -4096, 4096) && mg_in(r.x1, -4096, 4096) && mg_in(r.y1, -4096, 4096) && mg_in(r.thickness, 0, 4096),
                 "vk_mg_render: scene %d rect %d: box or thickness out of range", k, i);
    VK_CHECK_ARG(mg_in(r.color[0], 0, 255) && mg_in(r.color[1], 0, 255) && mg_in(r.color[2], 0, 255), "vk_mg_render: scene %d rect %d: colour out of range", k,
                 i);
  }
  return VK_OK;
}

}  // namespace vk

using namespace vk;

extern "C" size_t vk_mg_scenes_dev_bytes(int n) { return n < 1 ? 0 : VK_MG_SCENES_DEV_BYTES(n); }

extern "C" int vk_mg_render(int n, int S, const vk_mg_scene* scenes_host, void* scenes_dev, size_t scenes_dev_bytes, uint8_t* rgb, uint8_t* mask,
                            void* stream) {
  VK_CHECK_ARG(scenes_host && scenes_dev && rgb && mask, "vk_mg_render: null buffer");
  VK_CHECK_ARG(n >= 1 && n <= 65535, "vk_mg_render: batch %d outside 1..65535", n);
  VK_CHECK_ARG(S >= VK_MG_MIN_SIDE && S <= VK_MG_MAX_SIDE, "vk_mg_render: S = %d outside %d..%d", S, VK_MG_MIN_SIDE, VK_MG_MAX_SIDE);
  VK_CHECK_ARG(scenes_dev_bytes >= VK_MG_SCENES_DEV_BYTES(n), "vk_mg_render: scene scratch of %zu bytes, %zu needed", scenes_dev_bytes,
               VK_MG_SCENES_DEV_BYTES(n));
  VK_CHECK_ARG(((uintptr_t)scenes_host & 3) == 0 && ((uintptr_t)scenes_dev & 3) == 0 && ((uintptr_t)rgb & 3) == 0 && ((uintptr_t)mask & 3) == 0,
               "vk_mg_render: misaligned buffer");
  for (int k = 0; k < n; ++k) {
    const int rc = mg_check_scene(k, S, scenes_host[k]);
    if (rc != VK_OK) return rc;
  }
  hipStream_t st = (hipStream_t)stream;
  VK_CHECK_HIP(hipMemcpyAsync(scenes_dev, scenes_host, VK_MG_SCENES_DEV_BYTES(n), hipMemcpyHostToDevice, st));
  vkh::ProfScope ps("mg_render", st, 0.0, (double)n * S * S * 4.0);              // 4 bytes written per pixel; nothing read but the records
  const dim3 grid((S + MG_W - 1) / MG_W, (S + MG_H - 1) / MG_H, n);
  if (S % 4 == 0)
    hipLaunchKernelGGL(k_mg_render<true>, grid, dim3(256), 0, st, S, (const int*)scenes_dev, rgb, mask);
  else
    hipLaunchKernelGGL(k_mg_render<false>, grid, dim3(256), 0, st, S, (const int*)scenes_dev, rgb, mask);
  VK_CHECK_HIP(hipGetLastError());
  return VK_OK;
}
