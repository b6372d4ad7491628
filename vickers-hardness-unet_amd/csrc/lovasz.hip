// Lovasz losses (vk_lovasz_flat, vk_lovasz_loss): the only loss of the family that is not a function of the I, P, T sums of seg_loss.hip.
// It needs the errors in descending order, a prefix count of the foreground labels over that order and a scatter back:
//   sort      stable least-significant-digit radix sort of (32-bit key, 32-bit payload) pairs over S equal-length segments: four passes of
//             8 bits, each {histogram per tile, scan per (segment, digit) row, scatter}.  key = the fp32 error mapped so that unsigned
//             ascending order is error descending (0xFFFFFFFF: an ignored entry, behind everything); payload = index inside the segment
//             | label bit << 31.  The first pass makes its keys from the caller's tensors while it reads them (no pass of its own).
//   count     foreground labels per tile of the sorted order
//   apply     c_k by ballots over the sorted order, the Jaccard increment in closed form (an integer prefix count, no float cumsum),
//             relu(e) dJ into one fp64 partial per workgroup, the gradient scattered to the entry's index
//   finalize  one workgroup adds the partials in a fixed order
// Multiclass (softmax) sorts class by class, leaves G_c(i) in a [N][C][HW] buffer and ends with an elementwise softmax backward.
// Ranks inside a tile come from ballots over lanes in index order (wave64); the only atomics are integer counters whose final value
// does not depend on the order of the additions.  The same inputs give the same bits.
// A tile is 4096 entries: wave w of 4 owns the 1024 consecutive entries [1024 w, 1024 (w + 1)) in 16 rounds of 64 lanes, so that
// (wave, round, lane) is index order.  Per-thread arrays are indexed by unrolled loops only (registers, no scratch).
#include <math.h>

#include "vk_common.h"

namespace vk {

constexpr int kLvRounds = 16;
constexpr uint32_t kLvTile = 256u * kLvRounds;
constexpr uint32_t kLvIgnKey = 0xFFFFFFFFu;
enum { LV_BUF = 0, LV_FLAT = 1, LV_HINGE = 2, LV_SOFTMAX = 3 };

// where the pairs of a pass come from: a buffer of sorted-so-far pairs, or the caller's tensors (first pass)
struct LvSrc {
  const u32x2_t* buf;
  const float* a;          // errors (flat) or logits
  const void* b;           // flags uint8 (flat), target fp32 (hinge), labels int64 (softmax)
  int has_ignore, ignore;
  int C, c, HW;
  FastDiv dHW;
};

// where the apply pass writes
struct LvOut {
  float* out;              // flat: derr [S][L]; hinge: dlogits; softmax: G [N][C][HW]   (may be null)
  uint32_t* rank;          // flat only (may be null)
  float scale;
  int accumulate;
  int C, c, HW;
  FastDiv dHW;
  double* part;            // [slot][S][T]
  uint32_t* gcnt;          // [slot][S]: foreground count of the segment
  int slot;
};

// fp32 -> key: unsigned ascending = value descending, in the usual radix order of the bit patterns (-NaN .. -0 +0 .. +NaN ascending);
// 0xFFFFFFFF is kept for ignored entries
__device__ __forceinline__ uint32_t lv_key(float e) {
  const uint32_t u = as_u32(e);
  const uint32_t asc = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  const uint32_t k = ~asc;
  return k < 0xFFFFFFFEu ? k : 0xFFFFFFFEu;
}
__device__ __forceinline__ float lv_unkey(uint32_t k) {
  const uint32_t asc = ~k;
  return as_f32((asc & 0x80000000u) ? (asc ^ 0x80000000u) : ~asc);
}

// softmax pieces of pixel i of image xn [C][HW]: the maximum and 1 / sum exp, in fp64, so that p_c rounded to fp32 is (but for rare
// double roundings) the correctly rounded probability: two probabilities that differ compare as they do in exact arithmetic, and the
// order of near-equal errors does not depend on the last bits of an fp32 exp.  Every kernel that needs p_c goes through this and
// lv_prob, so the key a probability was sorted by and the probability of the backward pass are the same bits.
__device__ __forceinline__ void lv_softmax_stats(const float* __restrict__ xn, int C, int HW, uint32_t i, float* m, double* inv) {
  float mx = xn[i];
  for (int k = 1; k < C; ++k) mx = fmaxf(mx, xn[(size_t)k * HW + i]);
  double s = 0.0;
  for (int k = 0; k < C; ++k) s += exp((double)xn[(size_t)k * HW + i] - (double)mx);
  *m = mx;
  *inv = 1.0 / s;
}
__device__ __forceinline__ float lv_prob(const float* __restrict__ xn, int HW, uint32_t i, int k, float m, double inv) {
  return (float)(exp((double)xn[(size_t)k * HW + i] - (double)m) * inv);
}

template <int SRC>
__device__ __forceinline__ void lv_gen(const LvSrc& s, uint32_t seg, uint32_t L, uint32_t j, uint32_t* key, uint32_t* pay) {
  const size_t q = (size_t)seg * L + j;
  if constexpr (SRC == LV_BUF) {
    const u32x2_t v = s.buf[q];
    *key = v.x;
    *pay = v.y;
  } else {
    float e;
    bool fg, ign;
    if constexpr (SRC == LV_FLAT) {
      e = s.a[q];
      const unsigned f = ((const uint8_t*)s.b)[q];
      fg = f == 1u;
      ign = f >= 2u;
    } else if constexpr (SRC == LV_HINGE) {
      const float x = s.a[q], y = ((const float*)s.b)[q];
      ign = s.has_ignore && y == (float)s.ignore;
      e = 1.f - x * (2.f * y - 1.f);          // x * (+-1) is exact: one rounding with or without contraction
      fg = y > 0.5f;
    } else {
      const uint32_t n = fdiv((uint32_t)q, s.dHW), i = (uint32_t)q - n * (uint32_t)s.HW;
      const int64_t t = ((const int64_t*)s.b)[q];
      ign = !(t >= 0 && t < s.C) || (s.has_ignore && t == (int64_t)s.ignore);      // a bad label is never used as an index
      const float* xn = s.a + (size_t)n * s.C * s.HW;
      float m;
      double inv;
      lv_softmax_stats(xn, s.C, s.HW, i, &m, &inv);
      fg = t == (int64_t)s.c;
      e = fabsf((fg ? 1.f : 0.f) - lv_prob(xn, s.HW, i, s.c, m, inv));
    }
    *key = ign ? kLvIgnKey : lv_key(e);
    *pay = j | ((fg && !ign) ? 0x80000000u : 0u);
  }
}

__device__ __forceinline__ uint32_t lv_wave_incl_scan(uint32_t v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

// ---------------------------------------------------------------------------------------------- sort
// grid (T, S): digit counts of one tile -> hist[seg][digit][tile]
template <int SRC>
__global__ __launch_bounds__(256) void k_lv_hist(LvSrc s, uint32_t L, uint32_t T, int shift, uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[256];
  const uint32_t tile = blockIdx.x, seg = blockIdx.y;
  h[threadIdx.x] = 0u;
  __syncthreads();
  const uint32_t base = tile * kLvTile;
#pragma unroll 4
  for (int r = 0; r < kLvRounds; ++r) {
    const uint32_t j = base + r * 256u + threadIdx.x;
    if (j < L) {
      uint32_t key, pay;
      lv_gen<SRC>(s, seg, L, j, &key, &pay);
      atomicAdd(&h[(key >> shift) & 255u], 1u);
    }
  }
  __syncthreads();
  hist[((size_t)seg * 256u + threadIdx.x) * T + tile] = h[threadIdx.x];
}

// grid (256 digits, S): exclusive scan of one (segment, digit) row over the tiles, in place; the row's total -> tot[seg][digit]
__global__ __launch_bounds__(256) void k_lv_scan(uint32_t T, uint32_t* __restrict__ hist, uint32_t* __restrict__ tot) {
  __shared__ uint32_t wsum[4];
  uint32_t* row = hist + ((size_t)blockIdx.y * 256u + blockIdx.x) * T;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t carry = 0u;
  for (uint32_t t0 = 0; t0 < T; t0 += 256u) {
    const uint32_t t = t0 + threadIdx.x;
    const uint32_t v = t < T ? row[t] : 0u;
    const uint32_t incl = lv_wave_incl_scan(v, lane);
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t wb = 0u;
#pragma unroll
    for (int w = 0; w < 4; ++w) wb += w < wave ? wsum[w] : 0u;
    const uint32_t total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    if (t < T) row[t] = carry + wb + incl - v;
    carry += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) tot[blockIdx.y * 256u + blockIdx.x] = carry;
}

// grid (T, S): every pair of the tile to its place in the order by this digit.  Place = entries of the segment with a smaller digit
// + entries with this digit in earlier tiles (hist, scanned) + in earlier waves of the tile + earlier in this wave (ballots).
template <int SRC>
__global__ __launch_bounds__(256) void k_lv_scatter(LvSrc s, uint32_t L, uint32_t T, int shift, const uint32_t* __restrict__ hist,
                                                    const uint32_t* __restrict__ tot, u32x2_t* __restrict__ out) {
  __shared__ uint32_t cnt[4][256];
  __shared__ uint32_t wsum[4];
  const uint32_t tile = blockIdx.x, seg = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int w = 0; w < 4; ++w) cnt[w][tid] = 0u;
  __syncthreads();
  uint32_t key[kLvRounds], pay[kLvRounds], off[kLvRounds];
  const uint32_t wbase = tile * kLvTile + (uint32_t)wave * (64u * kLvRounds);
#pragma unroll
  for (int r = 0; r < kLvRounds; ++r) {
    const uint32_t j = wbase + r * 64u + lane;
    key[r] = kLvIgnKey;
    pay[r] = 0u;
    if (j < L) lv_gen<SRC>(s, seg, L, j, &key[r], &pay[r]);
  }
  volatile uint32_t* mycnt = cnt[wave];
  const uint64_t lt = (1ull << lane) - 1ull;
#pragma unroll
  for (int r = 0; r < kLvRounds; ++r) {
    const bool valid = wbase + r * 64u + lane < L;
    const uint32_t d = (key[r] >> shift) & 255u;
    uint64_t peers = __ballot(valid);              // the valid lanes of this round that hold the same digit
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1u;
      const uint64_t bal = __ballot(bit);
      peers &= bit ? bal : ~bal;
    }
    const uint32_t old = mycnt[d];
    __builtin_amdgcn_wave_barrier();
    if (valid && (peers >> lane) == 1ull) mycnt[d] = old + (uint32_t)__popcll(peers);       // the highest lane of the group
    __builtin_amdgcn_wave_barrier();
    off[r] = old + (uint32_t)__popcll(peers & lt);
  }
  __syncthreads();
  {
    const uint32_t c0 = cnt[0][tid], c1 = cnt[1][tid], c2 = cnt[2][tid];
    const uint32_t dt = tot[seg * 256u + tid];
    const uint32_t incl = lv_wave_incl_scan(dt, lane);
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t base = incl - dt + hist[((size_t)seg * 256u + tid) * T + tile];
#pragma unroll
    for (int w = 0; w < 4; ++w) base += w < wave ? wsum[w] : 0u;
    cnt[0][tid] = base;
    cnt[1][tid] = base + c0;
    cnt[2][tid] = base + c0 + c1;
    cnt[3][tid] = base + c0 + c1 + c2;
  }
  __syncthreads();
  u32x2_t* oseg = out + (size_t)seg * L;
#pragma unroll
  for (int r = 0; r < kLvRounds; ++r) {
    const bool valid = wbase + r * 64u + lane < L;
    const uint32_t pos = cnt[wave][(key[r] >> shift) & 255u] + off[r];
    if (valid && pos < L) oseg[pos] = u32x2_t{key[r], pay[r]};      // pos < L holds by construction; the test keeps any bits in bounds
  }
}

// grid (T, S): foreground labels per tile of the sorted order
__global__ __launch_bounds__(256) void k_lv_count(const u32x2_t* __restrict__ sorted, uint32_t L, uint32_t T, uint32_t* __restrict__ tilecnt) {
  __shared__ uint32_t n;
  const uint32_t tile = blockIdx.x, seg = blockIdx.y;
  if (threadIdx.x == 0) n = 0u;
  __syncthreads();
  uint32_t c = 0u;
#pragma unroll 4
  for (int r = 0; r < kLvRounds; ++r) {
    const uint32_t j = tile * kLvTile + r * 256u + threadIdx.x;
    if (j < L) c += sorted[(size_t)seg * L + j].y >> 31;
  }
  atomicAdd(&n, c);
  __syncthreads();
  if (threadIdx.x == 0) tilecnt[(size_t)seg * T + tile] = n;
}

// ---------------------------------------------------------------------------------------------- apply
// grid (T, S).  Position k of the sorted order: c_k = foreground labels in [0, k], G = all of them, U = G + (k + 1) - c_k, I = G - c_k;
// dJ = 1 / U at a foreground entry, I / (U (U - 1)) at a background one (U >= 2 there when G > 0); G = 0: dJ_0 = 1, else 0.
template <int MODE>
__global__ __launch_bounds__(256) void k_lv_apply(const u32x2_t* __restrict__ sorted, uint32_t L, uint32_t T,
                                                  const uint32_t* __restrict__ tilecnt, LvOut o) {
  __shared__ uint32_t red[2];
  __shared__ uint32_t wc[4];
  __shared__ double dred[4];
  const uint32_t tile = blockIdx.x, seg = blockIdx.y, S = gridDim.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid < 2) red[tid] = 0u;
  __syncthreads();
  {
    uint32_t below = 0u, all = 0u;
    for (uint32_t t = tid; t < T; t += 256u) {
      const uint32_t v = tilecnt[(size_t)seg * T + t];
      all += v;
      below += t < tile ? v : 0u;
    }
    atomicAdd(&red[0], below);
    atomicAdd(&red[1], all);
  }
  uint32_t key[kLvRounds], pay[kLvRounds];
  const uint32_t wbase = tile * kLvTile + (uint32_t)wave * (64u * kLvRounds);
  uint32_t mine = 0u;
#pragma unroll
  for (int r = 0; r < kLvRounds; ++r) {
    const uint32_t j = wbase + r * 64u + lane;
    key[r] = kLvIgnKey;
    pay[r] = 0u;
    if (j < L) {
      const u32x2_t v = sorted[(size_t)seg * L + j];
      key[r] = v.x;
      pay[r] = v.y;
    }
    mine += (uint32_t)__popcll(__ballot((pay[r] >> 31) != 0u));
  }
  if (lane == 0) wc[wave] = mine;
  __syncthreads();
  const uint32_t G = red[1];
  uint32_t running = red[0];
#pragma unroll
  for (int w = 0; w < 4; ++w) running += w < wave ? wc[w] : 0u;
  const uint64_t le = lane == 63 ? ~0ull : ((2ull << lane) - 1ull);
  const bool absent = MODE == LV_SOFTMAX && G == 0u;          // a class without a valid pixel in the segment has no term
  double acc = 0.0;
#pragma unroll
  for (int r = 0; r < kLvRounds; ++r) {
    const uint32_t k = wbase + r * 64u + lane;
    const bool fg = (pay[r] >> 31) != 0u;
    const uint64_t bal = __ballot(fg);
    const uint32_t ck = running + (uint32_t)__popcll(bal & le);
    running += (uint32_t)__popcll(bal);
    if (k >= L) continue;
    const bool ign = key[r] == kLvIgnKey;
    const uint32_t idx = pay[r] & 0x7FFFFFFFu;
    const float e = lv_unkey(key[r]);
    const uint32_t U = G + (k + 1u) - ck, I = G - ck;
    float dJ;
    if (G == 0u) dJ = k == 0u ? 1.f : 0.f;
    else dJ = fg ? 1.f / (float)U : (float)I / ((float)U * (float)(U - 1u));
    if (ign || absent) dJ = 0.f;
    const bool pos = e > 0.f;
    const float re = pos ? e : (e == e ? 0.f : e);          // relu that lets a NaN through
    if (!ign && !absent) acc += (double)(re * dJ);
    if (idx >= L) continue;                                  // cannot happen (the payload is an index < L); keeps any bits in bounds
    const size_t q = (size_t)seg * L + idx;
    if constexpr (MODE == LV_FLAT) {
      if (o.out) o.out[q] = pos ? dJ : 0.f;
      if (o.rank) o.rank[q] = ign ? 0xFFFFFFFFu : k;
    } else if constexpr (MODE == LV_HINGE) {
      if (o.out) {
        const float v = pos ? (fg ? -dJ : dJ) * o.scale : 0.f;
        if (!o.accumulate) o.out[q] = v;
        else if (!ign) o.out[q] += v;
      }
    } else {
      const uint32_t n = fdiv((uint32_t)q, o.dHW), i = (uint32_t)q - n * (uint32_t)o.HW;
      o.out[((size_t)n * o.C + o.c) * o.HW + i] = pos ? (fg ? -dJ : dJ) : 0.f;
    }
  }
  acc = wave_sum_d(acc);
  if (lane == 0) dred[wave] = acc;
  __syncthreads();
  if (tid == 0) {
    o.part[((size_t)o.slot * S + seg) * T + tile] = ((dred[0] + dred[1]) + dred[2]) + dred[3];
    if (tile == 0u) o.gcnt[(size_t)o.slot * S + seg] = G;
  }
}

// one workgroup: wave w adds the partials of the (slot, segment) pairs w, w + 4, ... in a fixed order; thread 0 forms the value.
// mode LV_FLAT: loss_out[seg]; LV_HINGE: {mean over the segments, 0, 0, 0}; LV_SOFTMAX: {mean over the segments of the mean over the
// present classes, bad labels, 0, 0} and scale[seg] = 1 / (present classes * S) for the backward.
__global__ __launch_bounds__(256) void k_lv_finalize(int mode, int slots, uint32_t S, uint32_t T, const double* __restrict__ part,
                                                     const uint32_t* __restrict__ gcnt, const uint32_t* __restrict__ bad,
                                                     double* __restrict__ segsum, float* __restrict__ scale,
                                                     float* __restrict__ loss_out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t pairs = (size_t)slots * S;
  for (size_t p = wave; p < pairs; p += 4) {
    double v = 0.0;
    for (uint32_t t = lane; t < T; t += 64u) v += part[p * T + t];
    v = wave_sum_d(v);
    if (lane == 0) segsum[p] = v;
  }
  __threadfence_block();
  __syncthreads();
  if (threadIdx.x != 0) return;
  if (mode == LV_FLAT) {
    for (uint32_t sg = 0; sg < S; ++sg) loss_out[sg] = (float)segsum[sg];
    return;
  }
  double total = 0.0;
  if (mode == LV_HINGE) {
    for (uint32_t sg = 0; sg < S; ++sg) total += segsum[sg];
  } else {
    for (uint32_t sg = 0; sg < S; ++sg) {
      int present = 0;
      double sum = 0.0;
      for (int c = 0; c < slots; ++c) {
        if (gcnt[(size_t)c * S + sg] > 0u) {
          ++present;
          sum += segsum[(size_t)c * S + sg];
        }
      }
      scale[sg] = present ? (float)(1.0 / ((double)present * (double)S)) : 0.f;
      total += present ? sum / present : 0.0;
    }
  }
  total /= (double)S;
  const uint32_t nbad = mode == LV_SOFTMAX ? *bad : 0u;
  loss_out[0] = nbad ? __builtin_nanf("") : (float)total;
  loss_out[1] = (float)nbad;
  loss_out[2] = 0.f;
  loss_out[3] = 0.f;
}

// labels that are neither a class nor ignore_index (an integer counter: the count does not depend on the order)
__global__ __launch_bounds__(256) void k_lv_bad(const int64_t* __restrict__ t, uint32_t n, int C, int has_ignore, int ignore,
                                                uint32_t* __restrict__ bad) {
  uint32_t c = 0u;
  for (uint32_t q = blockIdx.x * 256u + threadIdx.x; q < n; q += gridDim.x * 256u) {
    const int64_t l = t[q];
    c += (!(l >= 0 && l < C) && !(has_ignore && l == (int64_t)ignore)) ? 1u : 0u;
  }
  const uint64_t any = __ballot(c != 0u);
  if (any) atomicAdd(bad, c);
}

// dx_k = grad_scale * scale[seg] * p_k (G_k - sum_c G_c p_c); an ignored (or bad) pixel gets exactly 0 (left alone when accumulating)
__global__ __launch_bounds__(256) void k_lv_softmax_bwd(const float* __restrict__ x, const int64_t* __restrict__ t,
                                                        const float* __restrict__ G, const float* __restrict__ scale, int has_ignore,
                                                        int ignore, uint32_t NHW, int C, int HW, FastDiv dHW, int per_image,
                                                        float grad_scale, int accumulate, float* __restrict__ dl) {
  for (uint32_t q = blockIdx.x * 256u + threadIdx.x; q < NHW; q += gridDim.x * 256u) {
    const uint32_t n = fdiv(q, dHW), i = q - n * (uint32_t)HW;
    const int64_t l = t[q];
    const bool ok = l >= 0 && l < C && !(has_ignore && l == (int64_t)ignore);
    const size_t base = (size_t)n * C * HW;
    if (!ok) {
      if (!accumulate)
        for (int k = 0; k < C; ++k) dl[base + (size_t)k * HW + i] = 0.f;
      continue;
    }
    const float* xn = x + base;
    const float* gn = G + base;
    float m;
    double inv;
    lv_softmax_stats(xn, C, HW, i, &m, &inv);
    float dot = 0.f;
    for (int k = 0; k < C; ++k) dot = fmaf(gn[(size_t)k * HW + i], lv_prob(xn, HW, i, k, m, inv), dot);
    const float sc = scale[per_image ? n : 0u] * grad_scale;
    for (int k = 0; k < C; ++k) {
      const float v = lv_prob(xn, HW, i, k, m, inv) * (gn[(size_t)k * HW + i] - dot) * sc;
      float* d = dl + base + (size_t)k * HW + i;
      *d = accumulate ? *d + v : v;
    }
  }
}

__global__ void k_lv_combine(float* loss_out, float w) {
  if (threadIdx.x == 0) {
    loss_out[0] += w * loss_out[8];
    loss_out[6] += loss_out[9];
  }
}

}  // namespace vk

// =================================================================================================
// C ABI
// =================================================================================================
using namespace vk;

namespace {
constexpr int64_t kLvMaxEntries = 2147483647ll;

size_t lv_up(size_t b) { return (b + 255) & ~(size_t)255; }

struct LvWs {
  size_t bufA, bufB, hist, tot, tilecnt, part, gcnt, segsum, scale, bad, gbuf, total;
};
LvWs lv_layout(uint64_t S, uint64_t L, uint64_t slots, uint64_t gbuf_elems) {
  const uint64_t T = (L + kLvTile - 1) / kLvTile;
  LvWs w;
  size_t o = 0;
  w.bufA = o; o += lv_up(S * L * 8);
  w.bufB = o; o += lv_up(S * L * 8);
  w.hist = o; o += lv_up(S * 256 * T * 4);
  w.tot = o; o += lv_up(S * 256 * 4);
  w.tilecnt = o; o += lv_up(S * T * 4);
  w.part = o; o += lv_up(slots * S * T * 8);
  w.gcnt = o; o += lv_up(slots * S * 4);
  w.segsum = o; o += lv_up(slots * S * 8);
  w.scale = o; o += lv_up(S * 4);
  w.bad = o; o += 256;
  w.gbuf = o; o += lv_up(gbuf_elems * 4);
  w.total = o;
  return w;
}

// the four sort passes (first from `first`), the label count and the apply pass of one set of S segments; the sorted pairs end in bufB
template <int SRC, int MODE>
void lv_sort_apply(LvSrc first, uint32_t S, uint32_t L, char* ws, const LvWs& w, LvOut o, hipStream_t st) {
  const uint32_t T = (L + kLvTile - 1) / kLvTile;
  u32x2_t* A = (u32x2_t*)(ws + w.bufA);
  u32x2_t* B = (u32x2_t*)(ws + w.bufB);
  uint32_t* hist = (uint32_t*)(ws + w.hist);
  uint32_t* tot = (uint32_t*)(ws + w.tot);
  uint32_t* tilecnt = (uint32_t*)(ws + w.tilecnt);
  const dim3 grid(T, S);
  LvSrc s = first;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 8 * pass;
    u32x2_t* dst = (pass & 1) ? B : A;
    if (pass == 0) hipLaunchKernelGGL((k_lv_hist<SRC>), grid, dim3(256), 0, st, s, L, T, shift, hist);
    else hipLaunchKernelGGL((k_lv_hist<LV_BUF>), grid, dim3(256), 0, st, s, L, T, shift, hist);
    hipLaunchKernelGGL(k_lv_scan, dim3(256, S), dim3(256), 0, st, T, hist, tot);
    if (pass == 0) hipLaunchKernelGGL((k_lv_scatter<SRC>), grid, dim3(256), 0, st, s, L, T, shift, (const uint32_t*)hist, (const uint32_t*)tot, dst);
    else hipLaunchKernelGGL((k_lv_scatter<LV_BUF>), grid, dim3(256), 0, st, s, L, T, shift, (const uint32_t*)hist, (const uint32_t*)tot, dst);
    s.buf = dst;
  }
  hipLaunchKernelGGL(k_lv_count, grid, dim3(256), 0, st, (const u32x2_t*)B, L, T, tilecnt);
  o.part = (double*)(ws + w.part);
  o.gcnt = (uint32_t*)(ws + w.gcnt);
  hipLaunchKernelGGL((k_lv_apply<MODE>), grid, dim3(256), 0, st, (const u32x2_t*)B, L, T, (const uint32_t*)tilecnt, o);
}

void lv_finalize(int mode, int slots, uint32_t S, uint32_t L, char* ws, const LvWs& w, float* loss_out, hipStream_t st) {
  const uint32_t T = (L + kLvTile - 1) / kLvTile;
  hipLaunchKernelGGL(k_lv_finalize, dim3(1), dim3(256), 0, st, mode, slots, S, T, (const double*)(ws + w.part),
                     (const uint32_t*)(ws + w.gcnt), (const uint32_t*)(ws + w.bad), (double*)(ws + w.segsum), (float*)(ws + w.scale),
                     loss_out);
}

bool lv_finite(float v) { return v == v && v - v == 0.f; }

// configuration and shape; the text goes to vk_last_error_string when `who` is given
bool lv_check(const vk_lovasz_cfg* c, int N, int C, int HW, const char* who) {
#define LV_REQ(cond, ...)                      \
  do {                                         \
    if (!(cond)) {                             \
      if (who) vkh::set_error(__VA_ARGS__);    \
      return false;                            \
    }                                          \
  } while (0)
  const char* w = who ? who : "";
  LV_REQ(c, "%s: null configuration", w);
  LV_REQ(c->struct_size == sizeof(vk_lovasz_cfg), "%s: struct_size %u, this library expects %zu", w, c->struct_size, sizeof(vk_lovasz_cfg));
  LV_REQ(c->mode == VK_LOSS_BINARY || c->mode == VK_LOSS_MULTILABEL || c->mode == VK_LOSS_MULTICLASS, "%s: bad mode %d", w, c->mode);
  LV_REQ(C >= 1 && C <= 16, "%s: classes must be 1..16 (got %d)", w, C);
  LV_REQ(c->mode != VK_LOSS_BINARY || C == 1, "%s: mode binary needs C == 1 (got %d)", w, C);
  LV_REQ(c->mode != VK_LOSS_MULTICLASS || C >= 2, "%s: mode multiclass needs C >= 2 (got %d)", w, C);
  LV_REQ((c->per_image == 0 || c->per_image == 1) && (c->has_ignore == 0 || c->has_ignore == 1), "%s: per_image and has_ignore must be 0 or 1", w);
  LV_REQ(N >= 1 && HW >= 1 && N <= 65535, "%s: bad shape N=%d C=%d HW=%d", w, N, C, HW);
  LV_REQ((int64_t)N * C * HW <= kLvMaxEntries, "%s: N C HW = %lld entries, at most 2^31 - 1 in one call", w, (long long)N * C * HW);
  return true;
#undef LV_REQ
}

LvWs lv_loss_layout(const vk_lovasz_cfg* c, int N, int C, int HW) {
  const uint64_t S = c->per_image ? N : 1;
  if (c->mode == VK_LOSS_MULTICLASS) return lv_layout(S, (uint64_t)N * HW / S, C, (uint64_t)N * C * HW);
  return lv_layout(S, (uint64_t)N * C * HW / S, 1, 0);
}
}  // namespace

extern "C" size_t vk_lovasz_cfg_size(void) { return sizeof(vk_lovasz_cfg); }

extern "C" size_t vk_lovasz_workspace_bytes(const vk_lovasz_cfg* cfg, int N, int C, int HW) {
  if (!lv_check(cfg, N, C, HW, nullptr)) return 0;
  return lv_loss_layout(cfg, N, C, HW).total;
}

extern "C" size_t vk_lovasz_flat_workspace_bytes(int S, int64_t L) {
  if (S < 1 || S > 65535 || L < 1 || (int64_t)S * L > kLvMaxEntries) return 0;
  return lv_layout(S, L, 1, 0).total;
}

extern "C" int vk_lovasz_flat(const float* errors, const uint8_t* flag, int S, int64_t L, void* workspace, size_t workspace_bytes,
                              float* loss_out, float* derr_out, uint32_t* rank_out, void* stream) {
  VK_CHECK_ARG(S >= 1 && S <= 65535 && L >= 1 && (int64_t)S * L <= kLvMaxEntries, "vk_lovasz_flat: bad shape S=%d L=%lld", S, (long long)L);
  VK_CHECK_ARG(errors && flag && workspace && loss_out, "vk_lovasz_flat: null argument");
  const LvWs w = lv_layout(S, L, 1, 0);
  VK_CHECK_ARG(((uintptr_t)workspace & 7) == 0 && workspace_bytes >= w.total,
               "vk_lovasz_flat: workspace too small or misaligned (%zu bytes, needs %zu)", workspace_bytes, w.total);
  hipStream_t st = (hipStream_t)stream;
  vkh::ProfScope ps_("lovasz", st, 0.0, (double)S * L * (5.0 + 4.0 * 36.0 + 24.0));
  LvSrc s = {};
  s.a = errors;
  s.b = flag;
  LvOut o = {};
  o.out = derr_out;
  o.rank = rank_out;
  lv_sort_apply<LV_FLAT, LV_FLAT>(s, (uint32_t)S, (uint32_t)L, (char*)workspace, w, o, st);
  lv_finalize(LV_FLAT, 1, (uint32_t)S, (uint32_t)L, (char*)workspace, w, loss_out, st);
  VK_CHECK_HIP(hipGetLastError());
  return VK_OK;
}

extern "C" int vk_lovasz_loss(const vk_lovasz_cfg* cfg, int N, int C, int HW, const float* logits, const void* target, void* workspace,
                              size_t workspace_bytes, float* loss_out, float* dlogits, float grad_scale, int accumulate, void* stream) {
  if (!lv_check(cfg, N, C, HW, "vk_lovasz_loss")) return VK_ERR_ARG;
  VK_CHECK_ARG(lv_finite(grad_scale), "vk_lovasz_loss: grad_scale is not finite");
  VK_CHECK_ARG(accumulate == 0 || accumulate == 1, "vk_lovasz_loss: accumulate must be 0 or 1");
  VK_CHECK_ARG(logits && target && workspace && loss_out, "vk_lovasz_loss: null argument");
  const LvWs w = lv_loss_layout(cfg, N, C, HW);
  VK_CHECK_ARG(((uintptr_t)workspace & 7) == 0 && workspace_bytes >= w.total,
               "vk_lovasz_loss: workspace too small or misaligned (%zu bytes, needs %zu)", workspace_bytes, w.total);
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  const uint32_t S = cfg->per_image ? (uint32_t)N : 1u;
  const bool mc = cfg->mode == VK_LOSS_MULTICLASS;
  const double entries = (double)N * C * HW;
  vkh::ProfScope ps_("lovasz", st, 0.0, entries * (8.0 + 4.0 * 36.0 + 24.0));
  LvSrc s = {};
  s.a = logits;
  s.b = target;
  s.has_ignore = cfg->has_ignore;
  s.ignore = cfg->ignore_index;
  s.C = C;
  s.HW = HW;
  s.dHW = vkh::make_fastdiv((uint32_t)HW);
  LvOut o = {};
  o.accumulate = accumulate;
  o.C = C;
  o.HW = HW;
  o.dHW = s.dHW;
  if (!mc) {
    const uint32_t L = (uint32_t)((uint64_t)N * C * HW / S);
    o.out = dlogits;
    o.scale = grad_scale / (float)S;
    lv_sort_apply<LV_HINGE, LV_HINGE>(s, S, L, ws, w, o, st);
    lv_finalize(LV_HINGE, 1, S, L, ws, w, loss_out, st);
  } else {
    const uint32_t NHW = (uint32_t)((uint64_t)N * HW), L = NHW / S;
    uint32_t* bad = (uint32_t*)(ws + w.bad);
    float* gbuf = (float*)(ws + w.gbuf);
    VK_CHECK_HIP(hipMemsetAsync(bad, 0, sizeof(uint32_t), st));
    const unsigned nb = (NHW + 255u) / 256u;
    hipLaunchKernelGGL(k_lv_bad, dim3(nb < 1024u ? nb : 1024u), dim3(256), 0, st, (const int64_t*)target, NHW, C, cfg->has_ignore,
                       cfg->ignore_index, bad);
    o.out = gbuf;
    for (int c = 0; c < C; ++c) {
      s.c = c;
      o.c = c;
      o.slot = c;
      lv_sort_apply<LV_SOFTMAX, LV_SOFTMAX>(s, S, L, ws, w, o, st);
    }
    lv_finalize(LV_SOFTMAX, C, S, L, ws, w, loss_out, st);
    if (dlogits)
      hipLaunchKernelGGL(k_lv_softmax_bwd, dim3(nb < 8192u ? nb : 8192u), dim3(256), 0, st, logits, (const int64_t*)target,
                         (const float*)gbuf, (const float*)(ws + w.scale), cfg->has_ignore, cfg->ignore_index, NHW, C, HW, s.dHW,
                         cfg->per_image, grad_scale, accumulate, dlogits);
  }
  VK_CHECK_HIP(hipGetLastError());
  return VK_OK;
}

namespace vk {
// loss_out float[16]: [0, 8) as vk_seg_loss leaves them (zeros without a seg part), [8, 12) as vk_lovasz_loss leaves them;
// total += w * lovasz, bad labels += lovasz's count
int lovasz_combine(float* loss_out, float w, hipStream_t st) {
  hipLaunchKernelGGL(k_lv_combine, dim3(1), dim3(64), 0, st, loss_out, w);
  VK_CHECK_HIP(hipGetLastError());
  return VK_OK;
}
}  // namespace vk
