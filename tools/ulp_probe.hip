// ulp_probe: the error, in units in the last place of the fp32 result, of the three device expressions the BCE+Dice kernels
// (csrc/elementwise.hip: k_loss_reduce, k_loss_bwd) are built from, against the host's float64:
//     e(x) = expf(-|x|)      s(x) = log1pf(expf(-|x|))      p(x) = 1 / (1 + expf(-x))
// Stand-alone: it does not link libvkunet.so.  Build and run (same flags as csrc/Makefile, so the same expf / log1pf / division):
//     hipcc -O3 -std=c++17 --offload-arch=gfx950 tools/ulp_probe.hip -o ulp_probe && ./ulp_probe
// p(x) is judged in ulps where expf(-x) is finite (x >= -88.72); below that the expression gives 0 for a value under 2^-127, and the
// largest such absolute difference is printed instead.
// Arguments: 2^24 points evenly spaced over [-104, 104] (the range in which expf(-|x|) is not yet zero) and 2^24 points whose bit
// patterns are evenly spaced over the positive floats up to 104, with alternating sign (every binade down to the subnormals gets the
// same share).  Not exhaustive: tests/tail_cases.py uses twice the largest figure printed here (profiles/tailsweep/README.md).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#define CHECK(x)                                                                    \
  do {                                                                              \
    hipError_t e_ = (x);                                                            \
    if (e_ != hipSuccess) {                                                         \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, hipGetErrorString(e_));    \
      return 1;                                                                     \
    }                                                                               \
  } while (0)

__global__ void k_probe(size_t n, const float* __restrict__ x, float* __restrict__ e, float* __restrict__ s, float* __restrict__ p) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float xv = x[i];
    e[i] = expf(-fabsf(xv));
    s[i] = log1pf(expf(-fabsf(xv)));
    p[i] = 1.f / (1.f + expf(-xv));
  }
}

// distance in ulps of the float nearest `want`: spacing of the binade of |want|, 2^-149 in the subnormal range
static double ulps(float got, double want) {
  int ex;
  frexp(fabs(want), &ex);                       // |want| in [2^(ex-1), 2^ex)
  int q = ex - 24;
  if (q < -149) q = -149;
  return fabs((double)got - want) / ldexp(1.0, q);
}

int main() {
  const size_t half = (size_t)1 << 24, n = 2 * half;
  std::vector<float> x(n), e(n), s(n), p(n);
  for (size_t i = 0; i < half; ++i) x[i] = (float)(-104.0 + 208.0 * (double)i / (double)(half - 1));
  uint32_t top;
  {
    const float lim = 104.f;
    memcpy(&top, &lim, 4);
  }
  for (size_t i = 0; i < half; ++i) {
    const uint32_t bits = (uint32_t)((double)top * (double)i / (double)(half - 1));
    float v;
    memcpy(&v, &bits, 4);
    x[half + i] = (i & 1) ? -v : v;
  }
  float *dx, *de, *ds, *dp;
  CHECK(hipMalloc(&dx, n * 4));
  CHECK(hipMalloc(&de, n * 4));
  CHECK(hipMalloc(&ds, n * 4));
  CHECK(hipMalloc(&dp, n * 4));
  CHECK(hipMemcpy(dx, x.data(), n * 4, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_probe, dim3(4096), dim3(256), 0, 0, n, dx, de, ds, dp);
  CHECK(hipGetLastError());
  CHECK(hipDeviceSynchronize());
  CHECK(hipMemcpy(e.data(), de, n * 4, hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(s.data(), ds, n * 4, hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(p.data(), dp, n * 4, hipMemcpyDeviceToHost));
  double me = 0, ms = 0, mp = 0, mo = 0;
  float ae = 0, as = 0, ap = 0;
  for (size_t i = 0; i < n; ++i) {
    const double xd = x[i];
    const double we = exp(-fabs(xd)), wsp = log1p(exp(-fabs(xd))), wp = 1.0 / (1.0 + exp(-xd));
    const double ue = ulps(e[i], we), us = ulps(s[i], wsp), up = ulps(p[i], wp);
    if (ue > me) { me = ue; ae = x[i]; }
    if (us > ms) { ms = us; as = x[i]; }
    if (exp(-xd) > 3.4028234663852886e38) {       // expf(-x) overflows to inf: p is 0 in place of a value below 2^-127
      if (fabs((double)p[i] - wp) > mo) mo = fabs((double)p[i] - wp);
    } else if (up > mp) { mp = up; ap = x[i]; }
  }
  printf("{\"points\": %zu, \"expf_ulp\": %.4f, \"expf_at\": %.9g, \"softplus_ulp\": %.4f, \"softplus_at\": %.9g, "
         "\"sigmoid_ulp\": %.4f, \"sigmoid_at\": %.9g, \"sigmoid_abs_where_expf_overflows\": %.4g}\n", n, me, (double)ae, ms, (double)as,
         mp, (double)ap, mo);
  (void)hipFree(dx); (void)hipFree(de); (void)hipFree(ds); (void)hipFree(dp);
  return 0;
}
