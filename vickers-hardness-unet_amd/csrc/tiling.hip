// Sliding-window inference at the image's own resolution, with D4 test-time augmentation: the two passes either side
// of the forward pass, one kernel each.
//
//   k_tile_pre   : uint8 BGR [h][w][3] -> every (tile, view) of the grid as float32 [ntiles*nviews][3][T][T]: the view map, the source
//                  pixel (or pad_value outside the image), BGR->RGB, /255, (x - mean) / std — the expressions of k_letterbox_pre
//   k_tile_blend : logits [ntiles*nviews][C][T][T] -> one map [C][h][w] (+ uint8 masks): per pixel the views of every covering tile
//                  are mapped back and averaged, the tiles blended with a separable ramp window.  A gather: no atomics, every logit
//                  read once, the summation order fixed (tiles ascending, views ascending).
//
// View v = 4*tr + 2*fy + fx of a tile A:  A_v[i][j] = A[i0][j0],  (a, b) = tr ? (j, i) : (i, j),  i0 = fy ? T-1-a : a,
// j0 = fx ? T-1-b : b.  Its inverse, used by the blend: tile pixel (ty, tx) sits at (i, j) = tr ? (b, a) : (a, b) with
// a = fy ? T-1-ty : ty, b = fx ? T-1-tx : tx.
//
// Both kernels are byte-bound.  Lanes run along x of the output.  A transposing view turns that into a walk down a column of the
// other side: k_tile_pre stages the 32 x 32 source patch of its output patch in LDS (rows of 100 bytes = 25 dwords, odd, so the 32
// lanes of a column read hit 32 banks); k_tile_blend works on 16 x 16 pixel blocks, so that what the block reads of a transposed
// logit plane is 16 rows of 16 floats — whole 64-byte segments, each fetched once and shared by the block's four waves.
// Floating-point contraction is off: products and sums round as the scalar restatement in tests/tiling_ref.py does.
#include "letterbox.h"

#pragma clang fp contract(off)

namespace vk {

constexpr int TP = 32, TP_PITCH = 100;      // k_tile_pre: output patch side, bytes per LDS row (96 used)
constexpr int TB = 16;                      // k_tile_blend: output block side

// origin i of an axis of length L (the host has checked that the descriptor's arrays hold exactly these)
__device__ __forceinline__ int origin(int i, int s, int L, int T) { return min(i * s, max(L - T, 0)); }

__global__ __launch_bounds__(256) void k_tile_pre(const vk_tile_desc d, int nv, const uint8_t* __restrict__ src, float* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ uint8_t patch[TP][TP_PITCH];
  const int T = d.T;
  const int tv = blockIdx.z, t = tv / nv, v = tv - t * nv;
  const int y0 = origin(t / d.nx, T - d.overlap, d.h, T), x0 = origin(t % d.nx, T - d.overlap, d.w, T);
  const bool tr = v & 4, fy = v & 2, fx = v & 1;
  const int ab = tr ? blockIdx.x : blockIdx.y, bb = tr ? blockIdx.y : blockIdx.x;     // patch index along a (source rows), b (columns)
  const int r0 = fy ? T - 1 - (ab * TP + TP - 1) : ab * TP;                           // first source row / column of the patch, in tile
  const int c0 = fx ? T - 1 - (bb * TP + TP - 1) : bb * TP;                           // coordinates (negative where T % 32 != 0)
  for (int idx = threadIdx.x; idx < TP * TP * 3; idx += 256) {
    const int lr = idx / (TP * 3), lb = idx - lr * (TP * 3), lc = lb / 3;
    const int ty = r0 + lr, tx = c0 + lc;
    int val = d.pad_value;
    if ((unsigned)ty < (unsigned)T && (unsigned)tx < (unsigned)T && y0 + ty < d.h && x0 + tx < d.w)
      val = src[(size_t)(y0 + ty) * d.src_stride + (size_t)(x0 + tx) * 3 + (lb - lc * 3)];
    patch[lr][lb] = (uint8_t)val;
  }
  __syncthreads();
  const int lj = threadIdx.x & 31, j = blockIdx.x * TP + lj;
  if (j >= T) return;
  const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
  const size_t plane = (size_t)T * T;
  float* o = out + (size_t)tv * 3 * plane;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int li = (threadIdx.x >> 5) + u * 8, i = blockIdx.y * TP + li;
    if (i >= T) break;
    const int la = tr ? lj : li, lb = tr ? li : lj;
    const uint8_t* px = &patch[fy ? TP - 1 - la : la][(fx ? TP - 1 - lb : lb) * 3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float f = (float)px[2 - k] / 255.f;      // RGB plane k = BGR channel 2-k
      o[k * plane + (size_t)i * T + j] = (f - mean[k]) / stdv[k];
    }
  }
}

// origins covering coordinate p along one axis: they are consecutive, first index lo, count n (at most 3: two regular tiles, and the
// last one, pulled back flush with the edge)
__device__ __forceinline__ void covering(int n_org, int L, int T, int s, int p, int& lo, int& n) {
  lo = p >= T ? (p - T) / s + 1 : 0;
  n = 0;
#pragma unroll
  for (int u = 0; u < 3; ++u)
    if (lo + u < n_org && origin(lo + u, s, L, T) <= p) n = u + 1;
}

__device__ __forceinline__ float ramp(int t, int T, int R) {
#pragma clang fp contract(off)
  return (float)min(min(t + 1, T - t), R) / (float)R;
}

template <int NV, bool PROB>
__global__ __launch_bounds__(256) void k_tile_blend(const vk_tile_desc d, const float* __restrict__ logits, float thresh,
                                                    float* __restrict__ out, uint8_t* __restrict__ mask) {
#pragma clang fp contract(off)
  const int x = blockIdx.x * TB + (threadIdx.x & (TB - 1));
  const int y = blockIdx.y * TB + (threadIdx.x >> 4);
  if (x >= d.w || y >= d.h) return;
  const int T = d.T, s = T - d.overlap, R = d.overlap > 0 ? d.overlap : 1;
  int ylo, nyc, xlo, nxc;
  covering(d.ny, d.h, T, s, y, ylo, nyc);
  covering(d.nx, d.w, T, s, x, xlo, nxc);
  int ty[3], tx[3];
  float wy[3], wx[3];
#pragma unroll
  for (int u = 0; u < 3; ++u) {
    ty[u] = u < nyc ? y - origin(ylo + u, s, d.h, T) : 0;
    tx[u] = u < nxc ? x - origin(xlo + u, s, d.w, T) : 0;
    wy[u] = ramp(ty[u], T, R);
    wx[u] = ramp(tx[u], T, R);
  }
  const size_t plane = (size_t)T * T, view = plane * d.C;
  const bool single = nyc * nxc == 1;
  for (int c = 0; c < d.C; ++c) {
    // every covering (tile, view) logit of this pixel and plane is requested before the first expf
    float l[3][3][NV];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        if (a >= nyc || b >= nxc) continue;
        const float* base = logits + ((size_t)((ylo + a) * d.nx + xlo + b) * NV) * view + c * plane;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
          const int ia = (v & 2) ? T - 1 - ty[a] : ty[a], ib = (v & 1) ? T - 1 - tx[b] : tx[b];
          l[a][b][v] = base[v * view + (size_t)((v & 4) ? ib : ia) * T + ((v & 4) ? ia : ib)];
        }
      }
    float acc = 0.f, wsum = 0.f, q1 = 0.f;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        if (a >= nyc || b >= nxc) continue;
        float sum = PROB ? sigmoidf(l[a][b][0]) : l[a][b][0];
#pragma unroll
        for (int v = 1; v < NV; ++v) sum = sum + (PROB ? sigmoidf(l[a][b][v]) : l[a][b][v]);
        const float q = sum * (1.f / NV);
        const float w = wy[a] * wx[b];
        acc = acc + w * q;
        wsum = wsum + w;
        q1 = q;
      }
    float val = single ? q1 : acc / wsum;
    if (PROB) val = fminf(fmaxf(val, 0.f), 1.f);
    const size_t o = ((size_t)c * d.h + y) * d.w + x;
    if (out) out[o] = val;
    if (mask) mask[o] = (PROB ? val : sigmoidf(val)) >= thresh ? 255 : 0;
  }
}

static int view_count(int mask) { return mask == 0x01 ? 1 : mask == 0x03 ? 2 : mask == 0x0F ? 4 : mask == 0xFF ? 8 : 0; }

// the origins of one axis must be exactly those of the grid rule: every bound of the kernels rests on it
static bool axis_ok(int L, int T, int overlap, int n, const int* org) {
  const int s = T - overlap;
  const long want = L <= T ? 1 : ((long)L - T + s - 1) / s + 1;
  if (n != want) return false;
  const int last = L > T ? L - T : 0;
  for (int i = 0; i < n; ++i)
    if (org[i] != ((long)i * s < last ? i * s : last)) return false;
  return true;
}

static int check_desc(const vk_tile_desc* d, const char* who) {
  VK_CHECK_ARG(d != nullptr, "%s: null descriptor", who);
  VK_CHECK_ARG(d->h > 0 && d->w > 0, "%s: non-positive image size %dx%d", who, d->h, d->w);
  VK_CHECK_ARG(d->T >= 1 && d->T <= VK_TILE_MAX_SIDE, "%s: tile side %d outside 1..%d", who, d->T, VK_TILE_MAX_SIDE);
  VK_CHECK_ARG(d->overlap >= 0 && 2 * d->overlap <= d->T, "%s: overlap %d outside 0..tile/2 (tile %d)", who, d->overlap, d->T);
  VK_CHECK_ARG(d->ny >= 1 && d->ny <= VK_TILE_MAX_ORIGINS && d->nx >= 1 && d->nx <= VK_TILE_MAX_ORIGINS,
               "%s: %d x %d tile origins, at most %d per axis", who, d->ny, d->nx, VK_TILE_MAX_ORIGINS);
  VK_CHECK_ARG(axis_ok(d->h, d->T, d->overlap, d->ny, d->ys) && axis_ok(d->w, d->T, d->overlap, d->nx, d->xs),
               "%s: the origins are not those of tile %d, overlap %d on a %dx%d image", who, d->T, d->overlap, d->h, d->w);
  VK_CHECK_ARG(view_count(d->view_mask) != 0, "%s: view mask 0x%x is none of 0x01, 0x03, 0x0f, 0xff", who, d->view_mask);
  return VK_OK;
}

template <bool PROB>
static void launch_blend(int nv, dim3 grid, hipStream_t st, const vk_tile_desc& d, const float* logits, float thresh, float* out,
                         uint8_t* mask) {
  switch (nv) {
    case 1: hipLaunchKernelGGL((k_tile_blend<1, PROB>), grid, dim3(256), 0, st, d, logits, thresh, out, mask); break;
    case 2: hipLaunchKernelGGL((k_tile_blend<2, PROB>), grid, dim3(256), 0, st, d, logits, thresh, out, mask); break;
    case 4: hipLaunchKernelGGL((k_tile_blend<4, PROB>), grid, dim3(256), 0, st, d, logits, thresh, out, mask); break;
    default: hipLaunchKernelGGL((k_tile_blend<8, PROB>), grid, dim3(256), 0, st, d, logits, thresh, out, mask); break;
  }
}

}  // namespace vk

using namespace vk;

extern "C" int vk_tile_preprocess(const vk_tile_desc* d, const uint8_t* bgr, float* x, void* stream) {
  int rc = check_desc(d, "vk_tile_preprocess");
  if (rc != VK_OK) return rc;
  VK_CHECK_ARG(bgr && x, "vk_tile_preprocess: null buffer");
  VK_CHECK_ARG(d->src_stride >= 3 * d->w, "vk_tile_preprocess: src_stride %d below 3*w", d->src_stride);
  VK_CHECK_ARG(d->pad_value >= 0 && d->pad_value <= 255, "vk_tile_preprocess: pad_value outside 0..255");
  const int nv = view_count(d->view_mask), nt = d->ny * d->nx, nb = (d->T + TP - 1) / TP;
  vkh::ProfScope ps("tile_pre", (hipStream_t)stream, 0.0, 3.0 * d->h * d->w + 12.0 * d->T * d->T * nt * nv);
  hipLaunchKernelGGL(k_tile_pre, dim3(nb, nb, nt * nv), dim3(256), 0, (hipStream_t)stream, *d, nv, bgr, x);
  VK_CHECK_HIP(hipGetLastError());
  return VK_OK;
}

extern "C" int vk_tile_blend(const vk_tile_desc* d, int mode, const float* logits, float thresh, float* out_chw, uint8_t* mask_chw,
                             void* stream) {
  int rc = check_desc(d, "vk_tile_blend");
  if (rc != VK_OK) return rc;
  VK_CHECK_ARG(d->C >= 1 && d->C <= 16, "vk_tile_blend: C = %d outside 1..16", d->C);
  VK_CHECK_ARG(mode == VK_BLEND_PROB || mode == VK_BLEND_LOGIT, "vk_tile_blend: unknown mode %d", mode);
  VK_CHECK_ARG(logits != nullptr, "vk_tile_blend: null logits");
  VK_CHECK_ARG(out_chw || mask_chw, "vk_tile_blend: both outputs are null");
  const int nv = view_count(d->view_mask), nt = d->ny * d->nx;
  vkh::ProfScope ps("tile_blend", (hipStream_t)stream, 0.0, 4.0 * d->C * d->T * d->T * nt * nv + 4.0 * d->C * d->h * d->w);
  const dim3 grid((d->w + TB - 1) / TB, (d->h + TB - 1) / TB);
  if (mode == VK_BLEND_PROB)
    launch_blend<true>(nv, grid, (hipStream_t)stream, *d, logits, thresh, out_chw, mask_chw);
  else
    launch_blend<false>(nv, grid, (hipStream_t)stream, *d, logits, thresh, out_chw, mask_chw);
  VK_CHECK_HIP(hipGetLastError());
  return VK_OK;
}
