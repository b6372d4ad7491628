// Sub-pixel vertex refinement of the indentation fit: vk_subpix_refine, k_subpix.
//
// The geometry records carry int32 corners; the probability map they were fitted to holds the edge to a fraction of a pixel.  One
// 256-thread workgroup per (image, slot), wave k refines vertex k with one of two estimators (a wave-uniform branch):
//   corner: the gradient-orthogonality iteration.  Per iteration all 64 lanes sample the (2 win + 3)^2 patch into the wave's LDS,
//           lane j sums row j of the five accumulators left to right, and the row sums are added top to bottom;
//   lines:  per side all 64 lanes sample the n_stations x (2 R + 1) profiles into the same LDS, lane k finds station k's crossing,
//           and the two total-least-squares lines are intersected.
// The samples are independent, so sampling in parallel changes no bit; every ordered sum is one lane's sequential loop, and the short
// tails (row totals, the line fit, the 2 x 2 solve) are done by all lanes of the wave on broadcast LDS reads, which keeps q identical
// in every lane and the loop wave-uniform without a shuffle.  A wave shares LDS only with itself until the one barrier before the
// record is written, so the waves may run different numbers of iterations.
//
// IEEE float64 with contraction off; only + - * / sqrt floor fabs and compares.  The arithmetic is spelt out in include/vk_unet.h
// and mirrored line for line by tests/subpix_ref.py.  Every index is formed from a clamped coordinate: nothing read from the map or
// from a record can address memory outside the map.
#include "vk_common.h"
#include "subpix_tail.h"

#include <float.h>
#include <math.h>

#pragma clang fp contract(off)

namespace vk {

constexpr int kSpMaxWin = VK_SUBPIX_MAX_WIN;
constexpr int kSpMaxSide = 2 * kSpMaxWin + 3;                 // 33
constexpr int kSpPatch = kSpMaxSide * kSpMaxSide;             // 1089 doubles per wave; the lines method needs 32 * 31 = 992
constexpr int kSpMaxStations = VK_SUBPIX_MAX_STATIONS;
static_assert(kSpMaxStations * (2 * VK_SUBPIX_MAX_REACH + 1) <= kSpPatch, "the profiles of one side fit the wave's patch");
static_assert(sizeof(vk_subpix_quad) == 200 && sizeof(vk_subpix_quad) % 8 == 0, "vk_subpix_quad layout");

// LDS written by some lanes of a wave and read by others of the same wave
__device__ __forceinline__ void sp_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ bool sp_uniform(bool c) { return __builtin_amdgcn_readfirstlane(c ? 1 : 0) != 0; }

__device__ __forceinline__ double sp_sample(const float* __restrict__ p, int h, int w, double x, double y) {
#pragma clang fp contract(off)
  const double xm = (double)(w - 1), ym = (double)(h - 1);
  x = x > 0.0 ? x : 0.0;
  x = x < xm ? x : xm;
  y = y > 0.0 ? y : 0.0;
  y = y < ym ? y : ym;
  int x0 = 0, x1 = 0, y0 = 0, y1 = 0;
  if (w > 1) { x0 = (int)floor(x); x0 = x0 < w - 2 ? x0 : w - 2; x1 = x0 + 1; }
  if (h > 1) { y0 = (int)floor(y); y0 = y0 < h - 2 ? y0 : h - 2; y1 = y0 + 1; }
  const double fx = x - (double)x0, fy = y - (double)y0;
  const double p00 = (double)p[(size_t)y0 * w + x0], p01 = (double)p[(size_t)y0 * w + x1];
  const double p10 = (double)p[(size_t)y1 * w + x0], p11 = (double)p[(size_t)y1 * w + x1];
  const double top = p00 * (1.0 - fx) + p01 * fx;
  const double bot = p10 * (1.0 - fx) + p11 * fx;
  return top * (1.0 - fy) + bot * fy;
}

struct SpVertex {
  double x, y;
  int flags, iters;
};

// ------------------------------------------------------------------------------------------------ corner
__device__ SpVertex sp_corner(const vk_subpix_params& P, const float* __restrict__ map, int h, int w, double sx, double sy, int lane,
                              double* __restrict__ patch, double* __restrict__ rows) {
#pragma clang fp contract(off)
  const int win = P.win, zz = P.zero_zone, n = 2 * win + 3, nw = 2 * win + 1;
  const double eps2 = P.eps * P.eps;
  double qx = sx, qy = sy;
  int flags = 0, iters = 0;
  for (;;) {
    for (int e = lane; e < n * n; e += 64) {
      const int j = e / n, i = e - j * n;
      patch[e] = sp_sample(map, h, w, qx + (double)(i - win - 1), qy + (double)(j - win - 1));
    }
    sp_wave_sync();
    if (lane < nw) {
      const int j = lane;
      const double py = (double)(j - win);
      double ra = 0.0, rb = 0.0, rc = 0.0, r1 = 0.0, r2 = 0.0;
      for (int i = 0; i < nw; ++i) {
        const double px = (double)(i - win);
        double mk = P.wt[j] * P.wt[i];
        const int ai = i - win < 0 ? win - i : i - win, aj = j - win < 0 ? win - j : j - win;
        if (zz >= 0 && ai <= zz && aj <= zz) mk = 0.0;
        const double gx = patch[(j + 1) * n + i + 2] - patch[(j + 1) * n + i];
        const double gy = patch[(j + 2) * n + i + 1] - patch[j * n + i + 1];
        const double gxx = gx * gx, gxy = gx * gy, gyy = gy * gy;
        ra = ra + mk * gxx;
        rb = rb + mk * gxy;
        rc = rc + mk * gyy;
        r1 = r1 + mk * (gxx * px + gxy * py);
        r2 = r2 + mk * (gxy * px + gyy * py);
      }
      rows[0 * 32 + j] = ra;
      rows[1 * 32 + j] = rb;
      rows[2 * 32 + j] = rc;
      rows[3 * 32 + j] = r1;
      rows[4 * 32 + j] = r2;
    }
    sp_wave_sync();
    double a = 0.0, b = 0.0, c = 0.0, bb1 = 0.0, bb2 = 0.0;
    for (int j = 0; j < nw; ++j) {
      a = a + rows[0 * 32 + j];
      b = b + rows[1 * 32 + j];
      c = c + rows[2 * 32 + j];
      bb1 = bb1 + rows[3 * 32 + j];
      bb2 = bb2 + rows[4 * 32 + j];
    }
    sp_wave_sync();                                            // the next iteration writes patch and rows again
    const double det = a * c - b * b;
    if (sp_uniform(!(fabs(det) > DBL_EPSILON * DBL_EPSILON) || !(fabs(det) <= DBL_MAX))) {
      flags |= VK_SUBPIX_SINGULAR;
      break;
    }
    const double stx = (c * bb1 - b * bb2) / det;
    const double sty = (a * bb2 - b * bb1) / det;
    qx = qx + stx;
    qy = qy + sty;
    ++iters;
    if (sp_uniform(stx * stx + sty * sty <= eps2)) break;
    if (sp_uniform(!(qx >= 0.0 && qx < (double)w && qy >= 0.0 && qy < (double)h))) {
      flags |= VK_SUBPIX_LEFT_MAP;
      break;
    }
    if (iters >= P.max_iter) {
      flags |= VK_SUBPIX_NOT_CONVERGED;
      break;
    }
  }
  if (!(fabs(qx - sx) <= (double)win && fabs(qy - sy) <= (double)win)) {
    qx = sx;
    qy = sy;
    flags |= VK_SUBPIX_RESTORED;
  }
  return SpVertex{qx, qy, flags, iters};
}

// ------------------------------------------------------------------------------------------------ lines
struct SpLine {
  double cx, cy, vx, vy;
  int flags, n;
};

// The side from start vertex i towards start vertex j.  ptx, pty, ok: 32 entries each of the wave's LDS.
__device__ SpLine sp_side(const vk_subpix_params& P, const float* __restrict__ map, int h, int w, const int* box, int i, int j, double ccx,
                          double ccy, int lane, double* __restrict__ patch, double* __restrict__ ptx, double* __restrict__ pty,
                          int* __restrict__ ok) {
#pragma clang fp contract(off)
  SpLine o{0.0, 0.0, 0.0, 0.0, 0, 0};
  const double vx = (double)box[2 * i], vy = (double)box[2 * i + 1];
  const double dx = (double)box[2 * j] - vx, dy = (double)box[2 * j + 1] - vy;
  const double L = sqrt(dx * dx + dy * dy);
  if (L < 8.0) {                                               // uniform: the box is the same in every lane
    o.flags = VK_SUBPIX_SHORT_SIDE;
    return o;
  }
  double nx = dy / L, ny = -dx / L;
  if (nx * (vx - ccx) + ny * (vy - ccy) < 0.0) { nx = -nx; ny = -ny; }
  const int ns = P.n_stations, R = P.reach, T = 2 * R + 1;
  const double span = P.hi - P.lo;
  for (int e = lane; e < ns * T; e += 64) {
    const int k = e / T, t = e - k * T - R;
    const double f = P.lo + (span * (double)k) / (double)(ns - 1);
    const double stx = vx + dx * f, sty = vy + dy * f;
    patch[e] = sp_sample(map, h, w, stx + (double)t * nx, sty + (double)t * ny);
  }
  sp_wave_sync();
  if (lane < ns) {
    const int k = lane;
    const double* g = patch + k * T;
    double best = 0.0, best_abs = INFINITY;
    for (int t = -R; t < R; ++t) {
      const double g0 = g[t + R], g1 = g[t + R + 1];
      if (g0 >= P.level && P.level > g1) {
        const double pos = (double)t + (g0 - P.level) / (g0 - g1);
        if (fabs(pos) < best_abs) { best = pos; best_abs = fabs(pos); }
      }
    }
    const double f = P.lo + (span * (double)k) / (double)(ns - 1);
    const double stx = vx + dx * f, sty = vy + dy * f;
    ok[k] = best_abs < INFINITY ? 1 : 0;
    ptx[k] = stx + best * nx;
    pty[k] = sty + best * ny;
  }
  sp_wave_sync();
  int cnt = 0;
  double sx = 0.0, sy = 0.0;
  for (int k = 0; k < ns; ++k)
    if (ok[k]) { ++cnt; sx = sx + ptx[k]; sy = sy + pty[k]; }
  o.n = cnt;
  if (sp_uniform(cnt < 3)) {
    o.flags = VK_SUBPIX_NO_EDGE;
  } else {
    const double cx = sx / (double)cnt, cy = sy / (double)cnt;
    double sxx = 0.0, syy = 0.0, sxy = 0.0;
    for (int k = 0; k < ns; ++k)
      if (ok[k]) {
        const double ex = ptx[k] - cx, ey = pty[k] - cy;
        sxx = sxx + ex * ex;
        syy = syy + ey * ey;
        sxy = sxy + ex * ey;
      }
    const double hs = (sxx + syy) * 0.5, hd = (sxx - syy) * 0.5;
    const double lam = hs + sqrt(hd * hd + sxy * sxy);
    o.cx = cx;
    o.cy = cy;
    if (fabs(lam - sxx) > fabs(lam - syy)) { o.vx = sxy; o.vy = lam - sxx; }
    else { o.vx = lam - syy; o.vy = sxy; }
  }
  sp_wave_sync();                                              // the next side writes patch and the points again
  return o;
}

__device__ SpVertex sp_lines(const vk_subpix_params& P, const float* __restrict__ map, int h, int w, const int* box, int i, int lane,
                             double* __restrict__ patch, double* __restrict__ ptx, double* __restrict__ pty, int* __restrict__ ok) {
#pragma clang fp contract(off)
  const double sx = (double)box[2 * i], sy = (double)box[2 * i + 1];
  const double ccx = ((((double)box[0] + (double)box[2]) + (double)box[4]) + (double)box[6]) * 0.25;
  const double ccy = ((((double)box[1] + (double)box[3]) + (double)box[5]) + (double)box[7]) * 0.25;
  const SpLine l1 = sp_side(P, map, h, w, box, i, (i + 1) & 3, ccx, ccy, lane, patch, ptx, pty, ok);
  const SpLine l2 = sp_side(P, map, h, w, box, i, (i + 3) & 3, ccx, ccy, lane, patch, ptx, pty, ok);
  SpVertex o{sx, sy, l1.flags | l2.flags, l1.n + l2.n};
  if (o.flags) return o;
  const double den = l1.vx * l2.vy - l1.vy * l2.vx;
  if (!(den * den > 1e-6 * ((l1.vx * l1.vx + l1.vy * l1.vy) * (l2.vx * l2.vx + l2.vy * l2.vy)))) {
    o.flags = VK_SUBPIX_PARALLEL;
    return o;
  }
  const double ex = l2.cx - l1.cx, ey = l2.cy - l1.cy;
  const double u = (ex * l2.vy - ey * l2.vx) / den;
  const double qx = l1.cx + u * l1.vx, qy = l1.cy + u * l1.vy;
  if (!(fabs(qx - sx) <= P.max_shift && fabs(qy - sy) <= P.max_shift)) {
    o.flags = VK_SUBPIX_RESTORED;
    return o;
  }
  o.x = qx;
  o.y = qy;
  return o;
}

// ------------------------------------------------------------------------------------------------ the kernel
__global__ __launch_bounds__(256) void k_subpix(const vk_subpix_params P, int h, int w, const float* __restrict__ prob,
                                                const char* __restrict__ recs, size_t stride, size_t box_off, int valid_off,
                                                const int32_t* __restrict__ counts, int M, const double* __restrict__ affine,
                                                vk_subpix_quad* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double s_patch[4][kSpPatch];
  __shared__ double s_rows[4][5 * 32];
  __shared__ double s_ptx[4][kSpMaxStations], s_pty[4][kSpMaxStations];
  __shared__ int s_ok[4][kSpMaxStations];
  __shared__ double s_vx[4], s_vy[4];
  __shared__ int s_fl[4], s_it[4];
  const int slot = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cnt = counts[b];
  const int used = cnt < 0 ? 0 : (cnt > M ? M : cnt);
  if (slot >= used) return;                                    // the whole workgroup, before any barrier
  const char* rec = recs + ((size_t)b * M + slot) * stride;
  const int* box = reinterpret_cast<const int*>(rec + box_off);      // read where it is: a private copy indexed by the wave would spill
  const int valid = valid_off >= 0 ? (*reinterpret_cast<const int*>(rec + valid_off) != 0 ? 1 : 0) : 1;
  vk_subpix_quad* dst = out + (size_t)b * M + slot;
  if (!valid) {                                                // the whole workgroup again
    if (tid == 0) sp_write_invalid(dst, rec);
    return;
  }
  const float* map = prob + (size_t)b * ((size_t)h * w);
  SpVertex r;
  if (P.method == VK_SUBPIX_CORNER)
    r = sp_corner(P, map, h, w, (double)box[2 * wave], (double)box[2 * wave + 1], lane, s_patch[wave], s_rows[wave]);
  else
    r = sp_lines(P, map, h, w, box, wave, lane, s_patch[wave], s_ptx[wave], s_pty[wave], s_ok[wave]);
  if (lane == 0) { s_vx[wave] = r.x; s_vy[wave] = r.y; s_fl[wave] = r.flags; s_it[wave] = r.iters; }
  __syncthreads();
  if (tid != 0) return;
  sp_write_record(dst, rec, affine, b, s_vx, s_vy, s_fl, s_it);             // subpix_tail.h: shared with vk_kp_refine
}

}  // namespace vk

using namespace vk;

extern "C" int vk_subpix_refine(const vk_subpix_params* params, int batch, int h, int w, const float* prob, const void* records,
                                size_t record_stride, size_t box_offset, int valid_offset, const int32_t* counts, int max_components,
                                const double* affine, vk_subpix_quad* out, void* stream) {
  VK_CHECK_ARG(params, "vk_subpix_refine: null parameters");
  const vk_subpix_params& p = *params;
  VK_CHECK_ARG(p.method == VK_SUBPIX_CORNER || p.method == VK_SUBPIX_LINES, "vk_subpix_refine: method %d is neither corner nor lines", p.method);
  if (p.method == VK_SUBPIX_CORNER) {
    VK_CHECK_ARG(p.win >= 2 && p.win <= VK_SUBPIX_MAX_WIN, "vk_subpix_refine: win = %d outside 2..%d", p.win, VK_SUBPIX_MAX_WIN);
    VK_CHECK_ARG(p.zero_zone >= -1 && p.zero_zone < p.win, "vk_subpix_refine: zero_zone = %d outside -1..win - 1", p.zero_zone);
    VK_CHECK_ARG(p.max_iter >= 1 && p.max_iter <= 100, "vk_subpix_refine: max_iter = %d outside 1..100", p.max_iter);
    VK_CHECK_ARG(isfinite(p.eps) && p.eps > 0.0, "vk_subpix_refine: eps = %g is not a positive finite number", p.eps);
    for (int k = 0; k < 2 * p.win + 1; ++k) VK_CHECK_ARG(isfinite(p.wt[k]), "vk_subpix_refine: weight %d is not finite", k);
  } else {
    VK_CHECK_ARG(p.n_stations >= 3 && p.n_stations <= VK_SUBPIX_MAX_STATIONS, "vk_subpix_refine: n_stations = %d outside 3..%d", p.n_stations,
                 VK_SUBPIX_MAX_STATIONS);
    VK_CHECK_ARG(p.reach >= 1 && p.reach <= VK_SUBPIX_MAX_REACH, "vk_subpix_refine: reach = %d outside 1..%d", p.reach, VK_SUBPIX_MAX_REACH);
    VK_CHECK_ARG(p.lo >= 0.0 && p.lo < p.hi && p.hi <= 1.0, "vk_subpix_refine: lo = %g, hi = %g: need 0 <= lo < hi <= 1", p.lo, p.hi);
    VK_CHECK_ARG(isfinite(p.level), "vk_subpix_refine: level is not finite");
    VK_CHECK_ARG(isfinite(p.max_shift) && p.max_shift > 0.0, "vk_subpix_refine: max_shift = %g is not a positive finite number", p.max_shift);
  }
  VK_CHECK_ARG(batch >= 1 && batch <= 65535, "vk_subpix_refine: batch %d outside 1..65535", batch);
  VK_CHECK_ARG(h >= 1 && w >= 1, "vk_subpix_refine: map size %dx%d", h, w);
  VK_CHECK_ARG((size_t)h * (size_t)w < ((size_t)1 << 30), "vk_subpix_refine: more than 2^30 pixels per map");
  VK_CHECK_ARG(max_components >= 1 && max_components <= 4096, "vk_subpix_refine: max_components = %d outside 1..4096", max_components);
  VK_CHECK_ARG(prob && records && counts && out, "vk_subpix_refine: null buffer");
  VK_CHECK_ARG(record_stride % 4 == 0 && box_offset % 4 == 0 && box_offset >= 8 && box_offset + 32 <= record_stride,
               "vk_subpix_refine: record stride %zu / box offset %zu: multiples of 4 with label, area and box[8] inside the record",
               record_stride, box_offset);
  VK_CHECK_ARG(valid_offset == -1 || (valid_offset >= 8 && valid_offset % 4 == 0 && (size_t)valid_offset + 4 <= record_stride),
               "vk_subpix_refine: valid offset %d is neither -1 nor an int inside the record", valid_offset);
  VK_CHECK_ARG((((uintptr_t)prob | (uintptr_t)records | (uintptr_t)counts) & 3) == 0 && (((uintptr_t)out | (uintptr_t)affine) & 7) == 0,
               "vk_subpix_refine: misaligned buffer");
  hipStream_t st = (hipStream_t)stream;
  vkh::ProfScope ps_("subpix_refine", st, 0.0, (double)batch * (double)max_components * (double)sizeof(vk_subpix_quad));
  hipLaunchKernelGGL(k_subpix, dim3((unsigned)max_components, (unsigned)batch), dim3(256), 0, st, p, h, w, prob, (const char*)records,
                     record_stride, box_offset, valid_offset, counts, max_components, affine, out);
  VK_CHECK_HIP(hipGetLastError());
  return VK_OK;
}
