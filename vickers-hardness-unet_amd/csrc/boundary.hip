// Distance maps of masks on the device: the exact squared Euclidean distance transform, the signed map of the boundary
// loss, surface-distance statistics of a prediction against its label, and the boundary loss itself.
//
//   k_edt_cols : a lane owns one column (neighbouring columns in neighbouring lanes: every load and store of a wave is one row piece),
//        a wave one of 16 runs of rows of its 64 columns.  Down the run: the distance to the nearest site above inside it; the first
//        and last site of every run go through LDS, so each run knows its nearest site beyond either end; up the run: the minimum
//        of both directions, squared; 2^30 where the column holds no site.  The site test (foreground, background, inner boundary)
//        is made here from the source map: no site map is stored.
//   k_edt_rows : a wave owns one row, staged in LDS (8 bytes per pixel, sized by the launch), and takes one of two exact forms.
//        Search: every pixel walks outwards from its own column and stops at dx^2 >= best; lanes read consecutive LDS words; the
//        cost grows with the distance found.  Envelope: the lower envelope of the parabolas (Felzenszwalb & Huttenlocher) built in
//        LDS with integer ceil-divisions, then a binary search per pixel; the cost grows with the number of columns that hold a
//        site.  Per row: the search where its steps, bounded from the column distances, number at most 128 per column with a site
//        (measured: the chip does about 195 search steps in the time of one stack step), else the envelope.  VK_EDT_ROWS_SEARCH / _ENVELOPE in `sites` force one form; profiles/boundary/README.md has the times.
//   k_boundary_phi : elementwise, fp64 square root (correctly rounded) and one conversion to fp32.
//   k_bs_main / k_bs_hist / k_bs_pick / k_bs_final : the statistics.  Counts and maxima by integer atomics (LDS, then global); the two
//        fp64 sums as per-workgroup partials added in a fixed order; the nearest-rank percentile by a 9 + 8 + 8 bit radix select over
//        the int32 keys (every true d^2 is below 2^25).
//   k_bl_main / k_bl_final : sum of sigmoid(x) phi in fp64 partials, the gradient in the same pass.
// All distance arithmetic is integer and follows tests/boundary_ref.py.
#include <math.h>

#include "vk_common.h"

namespace vk {

static_assert(sizeof(vk_boundary_rec) == 216, "vk_boundary_rec layout");
constexpr int EDT_INF = 1 << 30;            // "no site in this column": adding any dx^2 <= 4095^2 cannot overflow
constexpr int EDT_FAR = 1 << 14;            // a column distance no map of 4096 rows reaches
constexpr int EDT_SEARCH_STEPS = 128;       // search steps that cost what one stack step of the envelope costs, rounded down (see k_edt_rows)

template <bool F32>
__device__ __forceinline__ bool edt_fg(const void* src, float thr, size_t i) {
  if (F32) return ((const float*)src)[i] > thr;
  return ((const uint8_t*)src)[i] != 0;
}

// ------------------------------------------------------------------------------------------------ columns
constexpr int EC_SEGS = 16;                 // waves of a workgroup: each owns one run of rows of the same 64 columns

template <bool F32>
__global__ __launch_bounds__(64 * EC_SEGS) void k_edt_cols(int h, int w, int seg_rows, const void* __restrict__ src, float thr, int sites,
                                                           int* __restrict__ g) {
  __shared__ short first_site[EC_SEGS][64], last_site[EC_SEGS][64];        // row of the first / last site of the run, -1: none
  const int lane = threadIdx.x & 63, seg = threadIdx.x >> 6;
  const int x = blockIdx.x * 64 + lane;
  const int y0 = seg * seg_rows, y1 = min(y0 + seg_rows, h);
  const bool live = x < w && y0 < h;
  const size_t plane = (size_t)blockIdx.y * h * w;
  int fs = -1, ls = -1;
  if (live) {
    // down the run: the distance to the nearest site above INSIDE the run
    bool up = y0 > 0 ? edt_fg<F32>(src, thr, plane + (size_t)(y0 - 1) * w + x) : true;      // beyond the border counts as foreground
    bool cur = edt_fg<F32>(src, thr, plane + (size_t)y0 * w + x);
    int dist = EDT_FAR;
#pragma unroll 4
    for (int y = y0; y < y1; ++y) {
      const size_t o = plane + (size_t)y * w + x;
      const bool next = y + 1 < h ? edt_fg<F32>(src, thr, o + w) : true;
      bool site;
      if (sites == VK_EDT_FG) site = cur;
      else if (sites == VK_EDT_BG) site = !cur;
      else {
        const bool left = x > 0 ? edt_fg<F32>(src, thr, o - 1) : true;
        const bool right = x + 1 < w ? edt_fg<F32>(src, thr, o + 1) : true;
        site = cur && !(up && next && left && right);
      }
      if (site) {
        if (fs < 0) fs = y;
        ls = y;
      }
      dist = site ? 0 : min(dist + 1, EDT_FAR);
      g[o] = dist;
      up = cur;
      cur = next;
    }
  }
  first_site[seg][lane] = (short)fs;
  last_site[seg][lane] = (short)ls;
  __syncthreads();
  if (!live) return;
  int above = EDT_FAR;                      // from row y0 to the nearest site of the runs above
  for (int s = seg - 1; s >= 0; --s) {
    const int l = last_site[s][lane];
    if (l >= 0) { above = y0 - l; break; }
  }
  int below = EDT_FAR;                      // from row y1 to the nearest site of the runs below
  for (int s = seg + 1; s < EC_SEGS; ++s) {
    const int f = first_site[s][lane];
    if (f >= 0) { below = f - y1; break; }
  }
  // up the run: the minimum of both directions, squared
  for (int y = y1 - 1; y >= y0; --y) {
    const size_t o = plane + (size_t)y * w + x;
    const int gd = g[o];
    below = gd == 0 ? 0 : min(below + 1, EDT_FAR);
    const int m = min(min(gd, above + (y - y0)), below);
    g[o] = m >= EDT_FAR ? EDT_INF : m * m;
  }
}

// ------------------------------------------------------------------------------------------------ rows
// ceil(a / b), b > 0
__device__ __forceinline__ int ceil_div(int a, int b) { return a >= 0 ? (a + b - 1) / b : -((-a) / b); }

__global__ __launch_bounds__(64) void k_edt_rows(int h, int w, int form, const int* __restrict__ g, int* __restrict__ d2) {
  extern __shared__ int env_lds[];          // 8 w bytes: a narrow map leaves room for many rows per compute unit
  int* row = env_lds;                                      // g^2 of the row
  uint16_t* vs = (uint16_t*)(env_lds + w);                 // column of the k-th parabola of the envelope
  uint16_t* zs = vs + w;                                   // first pixel at which it is the lowest
  const int lane = threadIdx.x;
  const size_t off = ((size_t)blockIdx.y * h + blockIdx.x) * w;
  // what each form would cost: the search at most min(g, reach) steps per pixel, the envelope one stack step per column with a site
  int steps = 0, sited = 0;
  for (int x = lane; x < w; x += 64) {
    const int v = g[off + x];
    row[x] = v;
    const int reach = max(x, w - 1 - x);
    steps += v < EDT_INF ? min((int)sqrtf((float)v), reach) : reach;
    sited += v < EDT_INF;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    steps += __shfl_xor(steps, o, 64);
    sited += __shfl_xor(sited, o, 64);
  }
  __syncthreads();
  if (form == VK_EDT_ROWS_SEARCH || (form == 0 && steps <= EDT_SEARCH_STEPS * sited)) {
    for (int x = lane; x < w; x += 64) {
      int best = row[x];
      const int reach = max(x, w - 1 - x);                                 // beyond it both sides are outside the row
      for (int d = 1; d <= reach && d * d < best; ++d) {
        const int dd = d * d;
        if (x - d >= 0) best = min(best, row[x - d] + dd);
        if (x + d < w) best = min(best, row[x + d] + dd);
      }
      d2[off + x] = best >= EDT_INF ? VK_EDT_NONE : best;
    }
    return;
  }
  // every lane walks the same stack and writes the same words: a lane reads back what it wrote itself
  int k = -1, topv = 0, topc = 0, topz = 0;
  int fnext = row[0];
  for (int q = 0; q < w; ++q) {
    const int fq = fnext;
    fnext = row[min(q + 1, w - 1)];                                        // one step ahead of the stack work
    if (fq >= EDT_INF) continue;
    const int cq = fq + q * q;
    int s = 0;
    while (k >= 0) {
      s = ceil_div(cq - topc, 2 * (q - topv));                            // q is the lower one from pixel s on
      if (s > topz) break;
      --k;
      if (k >= 0) {
        topv = vs[k];
        topz = zs[k];
        topc = row[topv] + topv * topv;
      }
    }
    if (k < 0) s = 0;
    if (s >= w) continue;                                                  // never the lowest inside the row
    ++k;
    topv = q; topz = s; topc = cq;
    vs[k] = (uint16_t)q;
    zs[k] = (uint16_t)s;
  }
  __syncthreads();
  for (int x = lane; x < w; x += 64) {
    int out = VK_EDT_NONE;
    if (k >= 0) {
      int lo = 0, hi = k;                                                  // the last parabola with zs <= x; zs[0] = 0
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((int)zs[mid] <= x) lo = mid; else hi = mid - 1;
      }
      const int v = vs[lo];
      out = (x - v) * (x - v) + row[v];
    }
    d2[off + x] = out;
  }
}

// ------------------------------------------------------------------------------------------------ phi
__global__ __launch_bounds__(256) void k_boundary_phi(size_t total, const int* __restrict__ d2_fg, const int* __restrict__ d2_bg,
                                                      float* __restrict__ phi) {
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    const int a = d2_fg[i], b = d2_bg[i];
    float v = 0.f;
    if (a > 0) {                                                           // a background pixel
      if (a != VK_EDT_NONE) v = (float)sqrt((double)a);
    } else if (b != VK_EDT_NONE) {
      v = (float)(1.0 - sqrt((double)b));
    }
    phi[i] = v;
  }
}

// ------------------------------------------------------------------------------------------------ statistics
constexpr int BS_MAX_BLOCKS = 64;           // workgroups (fp64 partials) per image
constexpr int BS_BINS = 512;                // 2^25 >> 16
constexpr int BS_ACC = 24;                  // 64-bit accumulators per image
enum { BA_NP = 0, BA_NG, BA_AP, BA_AG, BA_BI, BA_BU, BA_WPG = 6, BA_WGP = 14, BA_MPG = 22, BA_MGP = 23 };

struct BsTol {
  int n, band2;
  int tol2[8];
};

__device__ __forceinline__ double block_sum_d(double v, double* sh) {       // fixed order: the butterfly of a wave, then wave 0..3
  v = wave_sum_d(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  const double r = ((sh[0] + sh[1]) + sh[2]) + sh[3];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(256) void k_bs_main(int hw, BsTol tol, const int* __restrict__ ep, const int* __restrict__ eg,
                                                 const int* __restrict__ bp, const int* __restrict__ bg,
                                                 unsigned long long* __restrict__ acc, int* __restrict__ hist, double* __restrict__ part) {
  __shared__ unsigned int tab[BS_ACC];
  __shared__ double sh[4];
  const int t = threadIdx.x, img = blockIdx.y;
  if (t < BS_ACC) tab[t] = 0;
  __syncthreads();
  const size_t plane = (size_t)img * hw;
  int* h_pg = hist + ((size_t)img * 2 + 0) * BS_BINS;
  int* h_gp = hist + ((size_t)img * 2 + 1) * BS_BINS;
  unsigned int c[BS_ACC];
#pragma unroll
  for (int k = 0; k < BS_ACC; ++k) c[k] = 0;
  double s_pg = 0.0, s_gp = 0.0;
  for (int i = blockIdx.x * 256 + t; i < hw; i += gridDim.x * 256) {
    const int vep = ep[plane + i], veg = eg[plane + i], vbp = bp[plane + i], vbg = bg[plane + i];
    const bool pf = vbp > 0, gf = vbg > 0;
    c[BA_AP] += pf;
    c[BA_AG] += gf;
    const bool pb = pf && vbp <= tol.band2, gb = gf && vbg <= tol.band2;
    c[BA_BI] += pb && gb;
    c[BA_BU] += pb || gb;
    if (vep == 0) {
      c[BA_NP] += 1;
      if (veg != VK_EDT_NONE) {
        c[BA_MPG] = max(c[BA_MPG], (unsigned int)veg);
        s_pg += sqrt((double)veg);
#pragma unroll
        for (int k = 0; k < 8; ++k) c[BA_WPG + k] += k < tol.n && veg <= tol.tol2[k];
        atomicAdd(&h_pg[veg >> 16], 1);
      }
    }
    if (veg == 0) {
      c[BA_NG] += 1;
      if (vep != VK_EDT_NONE) {
        c[BA_MGP] = max(c[BA_MGP], (unsigned int)vep);
        s_gp += sqrt((double)vep);
#pragma unroll
        for (int k = 0; k < 8; ++k) c[BA_WGP + k] += k < tol.n && vep <= tol.tol2[k];
        atomicAdd(&h_gp[vep >> 16], 1);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < BS_ACC; ++k) {
    if (c[k]) {
      if (k >= BA_MPG) atomicMax(&tab[k], c[k]); else atomicAdd(&tab[k], c[k]);
    }
  }
  const double b_pg = block_sum_d(s_pg, sh), b_gp = block_sum_d(s_gp, sh);      // the barriers inside publish tab as well
  if (t < BS_ACC && tab[t]) {
    unsigned long long* a = acc + (size_t)img * BS_ACC + t;
    if (t >= BA_MPG) atomicMax(a, (unsigned long long)tab[t]); else atomicAdd(a, (unsigned long long)tab[t]);
  }
  if (t == 0) {
    double* p = part + ((size_t)img * BS_MAX_BLOCKS + blockIdx.x) * 2;
    p[0] = b_pg;
    p[1] = b_gp;
  }
}

// state[img][dir] = {rank left inside the chosen bin (0: undefined), key prefix}
__global__ __launch_bounds__(256) void k_bs_hist(int hw, int shift, const int* __restrict__ ep, const int* __restrict__ eg,
                                                 const int* __restrict__ state, int* __restrict__ hist) {
  const int img = blockIdx.y;
  const int* st = state + (size_t)img * 4;
  const int k_pg = st[0], pre_pg = st[1], k_gp = st[2], pre_gp = st[3];
  if (k_pg == 0 && k_gp == 0) return;
  const size_t plane = (size_t)img * hw;
  int* h_pg = hist + ((size_t)img * 2 + 0) * BS_BINS;
  int* h_gp = hist + ((size_t)img * 2 + 1) * BS_BINS;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < hw; i += gridDim.x * 256) {
    const int vep = ep[plane + i], veg = eg[plane + i];
    if (k_pg && vep == 0 && veg != VK_EDT_NONE && (veg >> (shift + 8)) == pre_pg) atomicAdd(&h_pg[(veg >> shift) & 255], 1);
    if (k_gp && veg == 0 && vep != VK_EDT_NONE && (vep >> (shift + 8)) == pre_gp) atomicAdd(&h_gp[(vep >> shift) & 255], 1);
  }
}

// one wave per (direction, image): the bin that holds the wanted rank
__global__ __launch_bounds__(64) void k_bs_pick(int first, const unsigned long long* __restrict__ acc, const int* __restrict__ hist,
                                                int* __restrict__ state) {
  const int dir = blockIdx.x, img = blockIdx.y, lane = threadIdx.x;
  int* st = state + (size_t)img * 4 + dir * 2;
  int want, prefix = 0;
  if (first) {
    const unsigned long long n_own = acc[(size_t)img * BS_ACC + (dir ? BA_NG : BA_NP)], n_other = acc[(size_t)img * BS_ACC + (dir ? BA_NP : BA_NG)];
    want = (n_own && n_other) ? (int)((95ull * n_own + 99ull) / 100ull) : 0;
  } else {
    want = st[0];
    prefix = st[1];
  }
  if (want == 0) {
    if (lane == 0) { st[0] = 0; st[1] = 0; }
    return;
  }
  const int* hb = hist + ((size_t)img * 2 + dir) * BS_BINS + lane * 8;
  int own[8], tot = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) { own[j] = hb[j]; tot += own[j]; }
  int cum = tot;                                                            // inclusive scan over the lanes
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(cum, o, 64);
    if (lane >= o) cum += u;
  }
  const unsigned long long reach = __ballot(cum >= want);
  const int owner = reach ? __ffsll((long long)reach) - 1 : 63;
  if (lane == owner) {
    int before = cum - tot, bin = 7;
    for (int j = 0; j < 8; ++j) {
      if (before + own[j] >= want) { bin = j; break; }
      before += own[j];
    }
    st[0] = want - before;
    st[1] = first ? lane * 8 + bin : ((prefix << 8) | (lane * 8 + bin));
  }
}

__global__ __launch_bounds__(64) void k_bs_final(int nb, int n_tol, const unsigned long long* __restrict__ acc, const int* __restrict__ state,
                                                 const double* __restrict__ part, vk_boundary_rec* __restrict__ out) {
  const int img = blockIdx.x, lane = threadIdx.x;
  const double* p = part + (size_t)img * BS_MAX_BLOCKS * 2;
  const double s_pg = wave_sum_d(lane < nb ? p[lane * 2] : 0.0), s_gp = wave_sum_d(lane < nb ? p[lane * 2 + 1] : 0.0);
  if (lane != 0) return;
  const unsigned long long* a = acc + (size_t)img * BS_ACC;
  const int* st = state + (size_t)img * 4;
  vk_boundary_rec r;
  r.n_pred = (int64_t)a[BA_NP]; r.n_gt = (int64_t)a[BA_NG];
  r.area_pred = (int64_t)a[BA_AP]; r.area_gt = (int64_t)a[BA_AG];
  const bool defined = a[BA_NP] && a[BA_NG];
  r.max2_pg = defined ? (int32_t)a[BA_MPG] : -1;
  r.max2_gp = defined ? (int32_t)a[BA_MGP] : -1;
  r.q95_2_pg = defined && st[0] ? st[1] : -1;
  r.q95_2_gp = defined && st[2] ? st[3] : -1;
  r.sum_pg = defined ? s_pg : 0.0;
  r.sum_gp = defined ? s_gp : 0.0;
  for (int k = 0; k < 8; ++k) {
    r.within_pg[k] = k < n_tol ? (int64_t)a[BA_WPG + k] : 0;
    r.within_gp[k] = k < n_tol ? (int64_t)a[BA_WGP + k] : 0;
  }
  r.band_inter = (int64_t)a[BA_BI]; r.band_union = (int64_t)a[BA_BU];
  r.flags = (a[BA_AP] == 0 ? 1 : 0) | (a[BA_AG] == 0 ? 2 : 0);
  r.reserved = 0;
  out[img] = r;
}

// ------------------------------------------------------------------------------------------------ loss
constexpr int BL_MAX_BLOCKS = VK_BOUNDARY_LOSS_WS_BYTES / 8;

// p = sigmoid(x) and 1 - p: the expression of sl_sigmoid in seg_loss.hip, kept identical (tests/tail_cases.py K_FUNC measures it)
__device__ __forceinline__ void bl_sigmoid(float x, float* p, float* omp) {
  const float e = expf(-fabsf(x));
  const float r = 1.f / (1.f + e);
  *p = x >= 0.f ? r : e * r;
  *omp = x >= 0.f ? e * r : r;
}

// one element: p phi for the sum (exact in fp64), and ((phi p (1 - p)) grad_scale) / count rounded once to fp32
template <bool GRAD>
__device__ __forceinline__ double bl_elem(float x, float f, double grad_scale, double cnt, float* g) {
  float p, omp;
  bl_sigmoid(x, &p, &omp);
  if (GRAD) *g = (float)((((double)f * (double)(p * omp)) * grad_scale) / cnt);
  return (double)p * (double)f;
}

template <bool GRAD>
__global__ __launch_bounds__(256) void k_bl_main(size_t count, size_t n4, const float* __restrict__ x, const float* __restrict__ phi,
                                                 double grad_scale, float* __restrict__ dlogits, double* __restrict__ part) {
  __shared__ double sh[4];
  const size_t stride = (size_t)gridDim.x * 256, t0 = (size_t)blockIdx.x * 256 + threadIdx.x;
  const double cnt = (double)count;
  double s = 0.0;
  for (size_t i = t0; i < n4; i += stride) {
    const f32x4_t xv = ((const f32x4_t*)x)[i], fv = ((const f32x4_t*)phi)[i];
    float g[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) s += bl_elem<GRAD>(xv[j], fv[j], grad_scale, cnt, &g[j]);
    if (GRAD) ((f32x4_t*)dlogits)[i] = f32x4_t{g[0], g[1], g[2], g[3]};
  }
  for (size_t i = n4 * 4 + t0; i < count; i += stride) {
    float g = 0.f;
    s += bl_elem<GRAD>(x[i], phi[i], grad_scale, cnt, &g);
    if (GRAD) dlogits[i] = g;
  }
  const double b = block_sum_d(s, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = b;
}

__global__ __launch_bounds__(256) void k_bl_final(int nb, size_t count, const double* __restrict__ part, float* __restrict__ loss_out) {
  __shared__ double sh[4];
  double s = 0.0;
  for (int i = threadIdx.x; i < nb; i += 256) s += part[i];
  const double tot = block_sum_d(s, sh);
  if (threadIdx.x == 0) loss_out[0] = (float)(tot / (double)count);
}

// ------------------------------------------------------------------------------------------------ host
static bool aligned_to(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

static int check_maps(const char* who, int batch, int h, int w) {
  VK_CHECK_ARG(batch >= 1 && batch <= 65535, "%s: batch %d outside 1..65535", who, batch);
  VK_CHECK_ARG(h >= 1 && h <= VK_EDT_MAX_SIDE && w >= 1 && w <= VK_EDT_MAX_SIDE, "%s: map size %d x %d outside 1..%d", who, h, w, VK_EDT_MAX_SIDE);
  return VK_OK;
}

static int check_src(const char* who, const char* name, const void* src, int kind, float thresh) {
  VK_CHECK_ARG(kind == VK_EDT_SRC_U8 || kind == VK_EDT_SRC_F32, "%s: %s kind %d is neither VK_EDT_SRC_U8 nor VK_EDT_SRC_F32", who, name, kind);
  VK_CHECK_ARG(src, "%s: null buffer (%s)", who, name);
  VK_CHECK_ARG(kind == VK_EDT_SRC_U8 || aligned_to(src, 4), "%s: misaligned buffer (%s)", who, name);
  VK_CHECK_ARG(kind == VK_EDT_SRC_U8 || thresh == thresh, "%s: %s threshold is NaN", who, name);
  return VK_OK;
}

// both passes; every argument is checked by the caller
static void edt_launch(int batch, int h, int w, const void* src, int kind, float thresh, int sites, int* d2, int* g, hipStream_t st) {
  const int form = sites & VK_EDT_ROWS_MASK, s = sites & ~VK_EDT_ROWS_MASK;
  const dim3 cgrid((w + 63) / 64, batch);
  const int seg_rows = (h + EC_SEGS - 1) / EC_SEGS;
  if (kind == VK_EDT_SRC_F32)
    hipLaunchKernelGGL(k_edt_cols<true>, cgrid, dim3(64 * EC_SEGS), 0, st, h, w, seg_rows, src, thresh, s, g);
  else
    hipLaunchKernelGGL(k_edt_cols<false>, cgrid, dim3(64 * EC_SEGS), 0, st, h, w, seg_rows, src, thresh, s, g);
  hipLaunchKernelGGL(k_edt_rows, dim3(h, batch), dim3(64), (size_t)w * 8, st, h, w, form, g, d2);
}

static size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct BsLayout {
  size_t g, map[4], hist, state, acc, part, zero_from, zero_bytes, total;
};
static BsLayout bs_layout(int batch, int h, int w) {
  BsLayout l;
  const size_t m = round_up((size_t)batch * h * w * 4, 256);
  size_t o = 0;
  l.g = o; o += m;
  for (int i = 0; i < 4; ++i) { l.map[i] = o; o += m; }
  l.zero_from = o;
  l.hist = o; o += round_up((size_t)3 * batch * 2 * BS_BINS * 4, 256);
  l.acc = o; o += round_up((size_t)batch * BS_ACC * 8, 256);
  l.zero_bytes = o - l.zero_from;
  l.state = o; o += round_up((size_t)batch * 4 * 4, 256);
  l.part = o; o += round_up((size_t)batch * BS_MAX_BLOCKS * 2 * 8, 256);
  l.total = o;
  return l;
}

}  // namespace vk

using namespace vk;

extern "C" size_t vk_edt_workspace_bytes(int batch, int h, int w) {
  if (batch < 1 || batch > 65535 || h < 1 || h > VK_EDT_MAX_SIDE || w < 1 || w > VK_EDT_MAX_SIDE) return 0;
  return (size_t)batch * h * w * 4;
}

extern "C" int vk_edt_sq(int batch, int h, int w, const void* src, int src_kind, float thresh, int sites, int32_t* d2, void* workspace,
                         size_t workspace_bytes, void* stream) {
  int rc = check_maps("vk_edt_sq", batch, h, w);
  if (rc != VK_OK) return rc;
  rc = check_src("vk_edt_sq", "src", src, src_kind, thresh);
  if (rc != VK_OK) return rc;
  const int s = sites & ~VK_EDT_ROWS_MASK;
  VK_CHECK_ARG(sites >= 0 && (s == VK_EDT_FG || s == VK_EDT_BG || s == VK_EDT_EDGE) && (sites & VK_EDT_ROWS_MASK) != VK_EDT_ROWS_MASK,
               "vk_edt_sq: sites %d is not VK_EDT_FG, VK_EDT_BG or VK_EDT_EDGE with at most one VK_EDT_ROWS_* bit", sites);
  VK_CHECK_ARG(d2 && workspace, "vk_edt_sq: null buffer");
  VK_CHECK_ARG(aligned_to(d2, 4) && aligned_to(workspace, 4), "vk_edt_sq: misaligned buffer");
  const size_t need = vk_edt_workspace_bytes(batch, h, w);
  VK_CHECK_ARG(workspace_bytes >= need, "vk_edt_sq: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  const double px = (double)batch * h * w;
  vkh::ProfScope ps("edt_sq", st, 0.0, px * ((src_kind == VK_EDT_SRC_F32 ? 4.0 : 1.0) + 4.0 * 5.0));      // g written, read, written, read; d2 written
  edt_launch(batch, h, w, src, src_kind, thresh, sites, d2, (int*)workspace, st);
  VK_CHECK_HIP(hipGetLastError());
  return VK_OK;
}

extern "C" int vk_boundary_phi(int batch, int h, int w, const int32_t* d2_fg, const int32_t* d2_bg, float* phi, void* stream) {
  int rc = check_maps("vk_boundary_phi", batch, h, w);
  if (rc != VK_OK) return rc;
  VK_CHECK_ARG(d2_fg && d2_bg && phi, "vk_boundary_phi: null buffer");
  VK_CHECK_ARG(aligned_to(d2_fg, 4) && aligned_to(d2_bg, 4) && aligned_to(phi, 4), "vk_boundary_phi: misaligned buffer");
  hipStream_t st = (hipStream_t)stream;
  const size_t total = (size_t)batch * h * w;
  vkh::ProfScope ps("boundary_phi", st, 0.0, (double)total * 12.0);
  hipLaunchKernelGGL(k_boundary_phi, dim3(grid_for(total)), dim3(256), 0, st, total, d2_fg, d2_bg, phi);
  VK_CHECK_HIP(hipGetLastError());
  return VK_OK;
}

extern "C" size_t vk_boundary_stats_workspace_bytes(int batch, int h, int w) {
  if (batch < 1 || batch > 65535 || h < 1 || h > VK_EDT_MAX_SIDE || w < 1 || w > VK_EDT_MAX_SIDE) return 0;
  return bs_layout(batch, h, w).total;
}

extern "C" int vk_boundary_stats(int batch, int h, int w, const void* pred, int pred_kind, float pred_thresh, const void* gt, int gt_kind,
                                 float gt_thresh, int n_tol, const int32_t* tol2, int32_t band2, vk_boundary_rec* out, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  int rc = check_maps("vk_boundary_stats", batch, h, w);
  if (rc != VK_OK) return rc;
  rc = check_src("vk_boundary_stats", "pred", pred, pred_kind, pred_thresh);
  if (rc != VK_OK) return rc;
  rc = check_src("vk_boundary_stats", "gt", gt, gt_kind, gt_thresh);
  if (rc != VK_OK) return rc;
  VK_CHECK_ARG(n_tol >= 0 && n_tol <= 8, "vk_boundary_stats: %d tolerances, at most 8", n_tol);
  VK_CHECK_ARG(n_tol == 0 || tol2, "vk_boundary_stats: null buffer (tol2)");
  BsTol tol;
  tol.n = n_tol;
  tol.band2 = band2;
  for (int k = 0; k < 8; ++k) tol.tol2[k] = 0;
  for (int k = 0; k < n_tol; ++k) {
    VK_CHECK_ARG(tol2[k] >= 0, "vk_boundary_stats: tol2[%d] = %d is negative", k, tol2[k]);
    tol.tol2[k] = tol2[k];
  }
  VK_CHECK_ARG(band2 >= 0, "vk_boundary_stats: band2 = %d is negative", band2);
  VK_CHECK_ARG(out && workspace, "vk_boundary_stats: null buffer");
  VK_CHECK_ARG(aligned_to(out, 8) && aligned_to(workspace, 8), "vk_boundary_stats: misaligned buffer");
  const BsLayout l = bs_layout(batch, h, w);
  VK_CHECK_ARG(workspace_bytes >= l.total, "vk_boundary_stats: workspace of %zu bytes, %zu needed", workspace_bytes, l.total);
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  int* g = (int*)(ws + l.g);
  int *ep = (int*)(ws + l.map[0]), *eg = (int*)(ws + l.map[1]), *bp = (int*)(ws + l.map[2]), *bg = (int*)(ws + l.map[3]);
  int* hist = (int*)(ws + l.hist);
  int* state = (int*)(ws + l.state);
  unsigned long long* acc = (unsigned long long*)(ws + l.acc);
  double* part = (double*)(ws + l.part);
  const int hw = h * w;
  const double px = (double)batch * hw;
  vkh::ProfScope ps("boundary_stats", st, 0.0, px * (4.0 * 21.0 + 16.0 + 3.0 * 8.0));
  VK_CHECK_HIP(hipMemsetAsync(ws + l.zero_from, 0, l.zero_bytes, st));
  edt_launch(batch, h, w, pred, pred_kind, pred_thresh, VK_EDT_EDGE, ep, g, st);
  edt_launch(batch, h, w, gt, gt_kind, gt_thresh, VK_EDT_EDGE, eg, g, st);
  edt_launch(batch, h, w, pred, pred_kind, pred_thresh, VK_EDT_BG, bp, g, st);
  edt_launch(batch, h, w, gt, gt_kind, gt_thresh, VK_EDT_BG, bg, g, st);
  const int nb = min(max((hw + 1023) / 1024, 1), BS_MAX_BLOCKS);
  const size_t hstep = (size_t)batch * 2 * BS_BINS;
  hipLaunchKernelGGL(k_bs_main, dim3(nb, batch), dim3(256), 0, st, hw, tol, ep, eg, bp, bg, acc, hist, part);
  hipLaunchKernelGGL(k_bs_pick, dim3(2, batch), dim3(64), 0, st, 1, acc, hist, state);
  hipLaunchKernelGGL(k_bs_hist, dim3(nb, batch), dim3(256), 0, st, hw, 8, ep, eg, state, hist + hstep);
  hipLaunchKernelGGL(k_bs_pick, dim3(2, batch), dim3(64), 0, st, 0, acc, hist + hstep, state);
  hipLaunchKernelGGL(k_bs_hist, dim3(nb, batch), dim3(256), 0, st, hw, 0, ep, eg, state, hist + 2 * hstep);
  hipLaunchKernelGGL(k_bs_pick, dim3(2, batch), dim3(64), 0, st, 0, acc, hist + 2 * hstep, state);
  hipLaunchKernelGGL(k_bs_final, dim3(batch), dim3(64), 0, st, nb, n_tol, acc, state, part, out);
  VK_CHECK_HIP(hipGetLastError());
  return VK_OK;
}

extern "C" int vk_boundary_loss(int n, int c, int hw, const float* logits, const float* phi, float grad_scale, float* dlogits,
                                float* loss_out, void* workspace, size_t workspace_bytes, void* stream) {
  VK_CHECK_ARG(n >= 1, "vk_boundary_loss: batch %d below 1", n);
  VK_CHECK_ARG(c >= 1 && c <= 16, "vk_boundary_loss: %d classes outside 1..16", c);
  VK_CHECK_ARG(hw >= 1, "vk_boundary_loss: plane of %d pixels", hw);
  VK_CHECK_ARG(logits && phi && loss_out && workspace, "vk_boundary_loss: null buffer");
  VK_CHECK_ARG(aligned_to(logits, 4) && aligned_to(phi, 4) && aligned_to(loss_out, 4) && aligned_to(workspace, 8) &&
                   (!dlogits || aligned_to(dlogits, 4)),
               "vk_boundary_loss: misaligned buffer");
  VK_CHECK_ARG(workspace_bytes >= VK_BOUNDARY_LOSS_WS_BYTES, "vk_boundary_loss: workspace of %zu bytes, %d needed", workspace_bytes,
               VK_BOUNDARY_LOSS_WS_BYTES);
  hipStream_t st = (hipStream_t)stream;
  const size_t count = (size_t)n * c * hw;
  const bool vec = aligned_to(logits, 16) && aligned_to(phi, 16) && (!dlogits || aligned_to(dlogits, 16));
  const size_t n4 = vec ? count / 4 : 0;
  const int nb = grid_for(vec ? (count + 3) / 4 : count, 256, BL_MAX_BLOCKS);
  vkh::ProfScope ps("boundary_loss", st, 0.0, (double)count * (dlogits ? 12.0 : 8.0));
  double* part = (double*)workspace;
  if (dlogits)
    hipLaunchKernelGGL(k_bl_main<true>, dim3(nb), dim3(256), 0, st, count, n4, logits, phi, (double)grad_scale, dlogits, part);
  else
    hipLaunchKernelGGL(k_bl_main<false>, dim3(nb), dim3(256), 0, st, count, n4, logits, phi, 0.0, (float*)nullptr, part);
  hipLaunchKernelGGL(k_bl_final, dim3(1), dim3(256), 0, st, nb, count, part, loss_out);
  VK_CHECK_HIP(hipGetLastError());
  return VK_OK;
}
