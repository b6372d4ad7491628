// Stand-alone driver for the host-side argument checks of csrc/keypoints.hip, meant for a sanitizer build of the HOST code (no GPU runs):
//
//   hipcc -std=c++17 --offload-arch=gfx950 -g -Xarch_host -fsanitize=address,undefined \
//         vickers-hardness-unet_amd/csrc/keypoints.hip tests/diag/keypoints_host_checks.hip -o keypoints_host_checks && ./keypoints_host_checks
//
// Every call below must come back with VK_ERR_ARG before anything touches a stream, and must leave its buffers as they were.  The
// two helpers of engine.hip that keypoints.hip links against are replaced by the smallest stand-ins.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../vickers-hardness-unet_amd/csrc/vk_common.h"

static char g_err[512];
namespace vkh {
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
}
ProfScope::ProfScope(const char*, hipStream_t stream, double, double) : idx(-1), st(stream), ev_end(nullptr) {
  fprintf(stderr, "a launch was reached: an argument check is missing\n");
  abort();
}
ProfScope::~ProfScope() {}
}  // namespace vkh

static int g_fail = 0, g_calls = 0;
static void expect(int rc, const char* word, const char* what) {
  ++g_calls;
  if (rc != VK_ERR_ARG || !strstr(g_err, word)) {
    printf("FAIL %s: rc = %d, message '%s' (expected '%s')\n", what, rc, g_err, word);
    ++g_fail;
  }
  g_err[0] = 0;
}

struct TArgs {
  int batch = 1, h = 8, w = 8;
  size_t stride = 96, voff = 8;
  int vtype = VK_KP_VERT_I32, valid_off = -1, cap = 2, table_len = 65;
  size_t istride = 64;
  int flags = 0;
};
struct PArgs {
  int batch = 1, h = 8, w = 8;
  size_t istride = 64;
  double min_peak = 0.3;
  int r = 2, max_peaks = 4;
  size_t ws_bytes = 260;
};
struct RArgs {
  vk_kp_params p{VK_KP_PARABOLA, 6, 3, 0.3, 0.25};
  int batch = 1, h = 8, w = 8;
  size_t istride = 64, stride = 96, box_off = 8;
  int valid_off = -1, cap = 2;
};

int main() {
  std::vector<int64_t> records(96, 7);
  std::vector<int32_t> counts(4, 7), ws(2048, 7);
  std::vector<float> table(80, 7.f), heat(128, 7.f);
  std::vector<double> out(256, 7.0), affine(8, 7.0);
  char* rec = (char*)records.data();

  auto T = [&](const TArgs& a, const void* r, const int32_t* c, const float* t, float* o) {
    return vk_kp_targets(a.batch, a.h, a.w, r, a.stride, a.voff, a.vtype, a.valid_off, c, a.cap, t, a.table_len, o, a.istride, a.flags, nullptr);
  };
  auto Tn = [&](const TArgs& a) { return T(a, rec, counts.data(), table.data(), (float*)out.data()); };
  auto P = [&](const PArgs& a, const float* m, vk_kp_peak* o, int32_t* c, void* w) {
    return vk_kp_peaks(a.batch, a.h, a.w, m, a.istride, a.min_peak, a.r, a.max_peaks, o, c, w, a.ws_bytes, nullptr);
  };
  auto Pn = [&](const PArgs& a) { return P(a, heat.data(), (vk_kp_peak*)out.data(), counts.data(), ws.data()); };
  auto Rf = [&](const RArgs& a, const vk_kp_params* p, const float* m, const void* r, const int32_t* c, const double* af, vk_subpix_quad* o) {
    return vk_kp_refine(p, a.batch, a.h, a.w, m, a.istride, r, a.stride, a.box_off, a.valid_off, c, a.cap, af, o, nullptr);
  };
  auto Rn = [&](const RArgs& a) { return Rf(a, &a.p, heat.data(), rec, counts.data(), affine.data(), (vk_subpix_quad*)out.data()); };

  // ---- the map arguments, shared by the three calls
  {
    TArgs a; a.batch = 0; expect(Tn(a), "batch 0", "targets batch 0");
    a = TArgs(); a.batch = 65536; expect(Tn(a), "batch 65536", "targets batch 65536");
    a = TArgs(); a.h = 0; expect(Tn(a), "map size", "targets h 0");
    a = TArgs(); a.w = -1; expect(Tn(a), "map size", "targets w -1");
    a = TArgs(); a.h = 1 << 15; a.w = (1 << 15) + 1; a.istride = (size_t)1 << 31; expect(Tn(a), "2^30", "targets 2^30");
    a = TArgs(); a.istride = 63; expect(Tn(a), "image stride", "targets stride below h w");
    a = TArgs(); a.istride = (size_t)1 << 41; expect(Tn(a), "image stride", "targets stride above 2^40");
    PArgs p; p.batch = 0; expect(Pn(p), "batch 0", "peaks batch 0");
    p = PArgs(); p.h = -3; expect(Pn(p), "map size", "peaks h -3");
    p = PArgs(); p.istride = 0; expect(Pn(p), "image stride", "peaks stride 0");
    p = PArgs(); p.h = 1 << 16; p.w = 1 << 16; p.istride = (size_t)1 << 32; expect(Pn(p), "2^30", "peaks 2^32 pixels");
    RArgs r; r.batch = 65536; expect(Rn(r), "batch 65536", "refine batch 65536");
    r = RArgs(); r.w = 0; expect(Rn(r), "map size", "refine w 0");
    r = RArgs(); r.istride = 63; expect(Rn(r), "image stride", "refine stride below h w");
  }
  // ---- vk_kp_targets
  {
    TArgs a;
    a.cap = 0; expect(Tn(a), "max_components = 0", "cap 0");
    a = TArgs(); a.cap = 4097; expect(Tn(a), "max_components = 4097", "cap 4097");
    a = TArgs(); a.vtype = 2; expect(Tn(a), "vertex type 2", "vertex type 2");
    a = TArgs(); a.vtype = -1; expect(Tn(a), "vertex type -1", "vertex type -1");
    a = TArgs(); a.stride = 38; expect(Tn(a), "record stride", "stride 38");
    a = TArgs(); a.stride = 36; expect(Tn(a), "record stride", "stride 36: the box ends outside");
    a = TArgs(); a.voff = 6; expect(Tn(a), "record stride", "offset 6");
    a = TArgs(); a.voff = 68; expect(Tn(a), "record stride", "offset 68");
    a = TArgs(); a.voff = (size_t)-32; expect(Tn(a), "record stride", "an offset that wraps");
    a = TArgs(); a.stride = (size_t)1 << 21; expect(Tn(a), "record stride", "stride 2^21");
    a = TArgs(); a.vtype = VK_KP_VERT_F64; a.stride = 100; expect(Tn(a), "record stride", "float64 stride 100");
    a = TArgs(); a.vtype = VK_KP_VERT_F64; a.voff = 12; expect(Tn(a), "record stride", "float64 offset 12");
    a = TArgs(); a.vtype = VK_KP_VERT_F64; a.voff = 40; expect(Tn(a), "record stride", "float64 offset 40: 64 bytes do not fit");
    a = TArgs(); a.valid_off = -2; expect(Tn(a), "valid offset", "valid -2");
    a = TArgs(); a.valid_off = 94; expect(Tn(a), "valid offset", "valid 94");
    a = TArgs(); a.valid_off = 96; expect(Tn(a), "valid offset", "valid 96");
    a = TArgs(); a.valid_off = INT32_MAX; expect(Tn(a), "valid offset", "valid INT_MAX");
    for (int len : {0, 1, 64, 66, -5, 193 * 193 + 1, INT32_MAX, INT32_MIN}) {
      a = TArgs(); a.table_len = len; expect(Tn(a), "table_len", "table_len");
    }
    a = TArgs(); a.flags = 3; expect(Tn(a), "flags = 3", "flags 3");
    a = TArgs(); a.flags = -1; expect(Tn(a), "flags = -1", "flags -1");
    a = TArgs(); a.flags = VK_KP_TABLE_LDS; a.table_len = 124 * 124 + 1; expect(Tn(a), "LDS path", "a table too large for LDS");
    a = TArgs();
    expect(T(a, nullptr, counts.data(), table.data(), (float*)out.data()), "null buffer", "null records");
    expect(T(a, rec, nullptr, table.data(), (float*)out.data()), "null buffer", "null counts");
    expect(T(a, rec, counts.data(), nullptr, (float*)out.data()), "null buffer", "null table");
    expect(T(a, rec, counts.data(), table.data(), nullptr), "null buffer", "null out");
    expect(T(a, rec + 2, counts.data(), table.data(), (float*)out.data()), "misaligned", "records + 2");
    expect(T(a, rec, (int32_t*)((char*)counts.data() + 1), table.data(), (float*)out.data()), "misaligned", "counts + 1");
    expect(T(a, rec, counts.data(), (float*)((char*)table.data() + 2), (float*)out.data()), "misaligned", "table + 2");
    expect(T(a, rec, counts.data(), table.data(), (float*)((char*)out.data() + 2)), "misaligned", "out + 2");
    a.vtype = VK_KP_VERT_F64;
    expect(T(a, rec + 4, counts.data(), table.data(), (float*)out.data()), "misaligned", "float64 records + 4");
  }
  // ---- vk_kp_peaks and its workspace size
  {
    if (vk_kp_peaks_workspace_bytes(1, 1, 1) != 260 || vk_kp_peaks_workspace_bytes(3, 40, 70) != 3 * 3 * 260 ||
        vk_kp_peaks_workspace_bytes(2, 1 << 15, 1 << 15) != (size_t)2 * (1 << 20) * 260 || vk_kp_peaks_workspace_bytes(0, 8, 8) != 0 ||
        vk_kp_peaks_workspace_bytes(65536, 8, 8) != 0 || vk_kp_peaks_workspace_bytes(1, 0, 8) != 0 || vk_kp_peaks_workspace_bytes(1, 8, -1) != 0 ||
        vk_kp_peaks_workspace_bytes(1, 1 << 15, (1 << 15) + 1) != 0 || vk_kp_peaks_workspace_bytes(1, INT32_MAX, INT32_MAX) != 0) {
      printf("FAIL: vk_kp_peaks_workspace_bytes\n");
      ++g_fail;
    }
    PArgs a;
    a.min_peak = NAN; expect(Pn(a), "min_peak", "min_peak NaN");
    a = PArgs(); a.min_peak = INFINITY; expect(Pn(a), "min_peak", "min_peak inf");
    a = PArgs(); a.r = 0; expect(Pn(a), "nms_radius = 0", "radius 0");
    a = PArgs(); a.r = 9; expect(Pn(a), "nms_radius = 9", "radius 9");
    a = PArgs(); a.r = INT32_MIN; expect(Pn(a), "nms_radius", "radius INT_MIN");
    a = PArgs(); a.max_peaks = 0; expect(Pn(a), "max_peaks = 0", "max_peaks 0");
    a = PArgs(); a.max_peaks = 4097; expect(Pn(a), "max_peaks = 4097", "max_peaks 4097");
    a = PArgs(); a.ws_bytes = 259; expect(Pn(a), "workspace", "workspace one byte short");
    a = PArgs(); a.ws_bytes = 0; expect(Pn(a), "workspace", "workspace of no bytes");
    a = PArgs(); a.batch = 2; expect(Pn(a), "workspace", "workspace for one map of two");
    a = PArgs();
    expect(P(a, nullptr, (vk_kp_peak*)out.data(), counts.data(), ws.data()), "null buffer", "null heat");
    expect(P(a, heat.data(), nullptr, counts.data(), ws.data()), "null buffer", "null out");
    expect(P(a, heat.data(), (vk_kp_peak*)out.data(), nullptr, ws.data()), "null buffer", "null counts");
    expect(P(a, heat.data(), (vk_kp_peak*)out.data(), counts.data(), nullptr), "null buffer", "null workspace");
    expect(P(a, (float*)((char*)heat.data() + 2), (vk_kp_peak*)out.data(), counts.data(), ws.data()), "misaligned", "heat + 2");
    expect(P(a, heat.data(), (vk_kp_peak*)((char*)out.data() + 2), counts.data(), ws.data()), "misaligned", "out + 2");
    expect(P(a, heat.data(), (vk_kp_peak*)out.data(), (int32_t*)((char*)counts.data() + 1), ws.data()), "misaligned", "counts + 1");
    expect(P(a, heat.data(), (vk_kp_peak*)out.data(), counts.data(), (char*)ws.data() + 3), "misaligned", "workspace + 3");
  }
  // ---- vk_kp_refine
  {
    RArgs a;
    a.p.method = 2; expect(Rn(a), "method 2", "method 2");
    a = RArgs(); a.p.method = -1; expect(Rn(a), "method -1", "method -1");
    a = RArgs(); a.p.search = 0; expect(Rn(a), "search = 0", "search 0");
    a = RArgs(); a.p.search = 32; expect(Rn(a), "search = 32", "search 32");
    a = RArgs(); a.p.search = INT32_MAX; expect(Rn(a), "search", "search INT_MAX");
    a = RArgs(); a.p.cwin = 0; expect(Rn(a), "cwin = 0", "cwin 0");
    a = RArgs(); a.p.cwin = 8; expect(Rn(a), "cwin = 8", "cwin 8");
    a = RArgs(); a.p.min_peak = NAN; expect(Rn(a), "min_peak", "min_peak NaN");
    a = RArgs(); a.p.min_peak = -INFINITY; expect(Rn(a), "min_peak", "min_peak -inf");
    a = RArgs(); a.p.floor_frac = 1.0; expect(Rn(a), "floor_frac", "floor_frac 1");
    a = RArgs(); a.p.floor_frac = -0.1; expect(Rn(a), "floor_frac", "floor_frac -0.1");
    a = RArgs(); a.p.floor_frac = NAN; expect(Rn(a), "floor_frac", "floor_frac NaN");
    a = RArgs(); a.cap = 0; expect(Rn(a), "max_components = 0", "cap 0");
    a = RArgs(); a.cap = 4097; expect(Rn(a), "max_components = 4097", "cap 4097");
    a = RArgs(); a.stride = 38; expect(Rn(a), "record stride", "stride 38");
    a = RArgs(); a.stride = 36; expect(Rn(a), "record stride", "stride 36");
    a = RArgs(); a.box_off = 6; expect(Rn(a), "record stride", "box offset 6");
    a = RArgs(); a.box_off = 4; expect(Rn(a), "record stride", "box offset 4");
    a = RArgs(); a.box_off = 68; expect(Rn(a), "record stride", "box offset 68");
    a = RArgs(); a.box_off = (size_t)-32; expect(Rn(a), "record stride", "a box offset that wraps");
    a = RArgs(); a.valid_off = -2; expect(Rn(a), "valid offset", "valid -2");
    a = RArgs(); a.valid_off = 94; expect(Rn(a), "valid offset", "valid 94");
    a = RArgs(); a.valid_off = 96; expect(Rn(a), "valid offset", "valid 96");
    a = RArgs(); a.valid_off = 4; expect(Rn(a), "valid offset", "valid 4");
    a = RArgs();
    expect(Rf(a, nullptr, heat.data(), rec, counts.data(), affine.data(), (vk_subpix_quad*)out.data()), "null parameters", "null parameters");
    expect(Rf(a, &a.p, nullptr, rec, counts.data(), affine.data(), (vk_subpix_quad*)out.data()), "null buffer", "null heat");
    expect(Rf(a, &a.p, heat.data(), nullptr, counts.data(), affine.data(), (vk_subpix_quad*)out.data()), "null buffer", "null records");
    expect(Rf(a, &a.p, heat.data(), rec, nullptr, affine.data(), (vk_subpix_quad*)out.data()), "null buffer", "null counts");
    expect(Rf(a, &a.p, heat.data(), rec, counts.data(), affine.data(), nullptr), "null buffer", "null out");
    expect(Rf(a, &a.p, (float*)((char*)heat.data() + 2), rec, counts.data(), affine.data(), (vk_subpix_quad*)out.data()), "misaligned", "heat + 2");
    expect(Rf(a, &a.p, heat.data(), rec + 2, counts.data(), affine.data(), (vk_subpix_quad*)out.data()), "misaligned", "records + 2");
    expect(Rf(a, &a.p, heat.data(), rec, (int32_t*)((char*)counts.data() + 1), affine.data(), (vk_subpix_quad*)out.data()), "misaligned", "counts + 1");
    expect(Rf(a, &a.p, heat.data(), rec, counts.data(), (double*)((char*)affine.data() + 4), (vk_subpix_quad*)out.data()), "misaligned", "affine + 4");
    expect(Rf(a, &a.p, heat.data(), rec, counts.data(), affine.data(), (vk_subpix_quad*)((char*)out.data() + 4)), "misaligned", "out + 4");
  }

  bool touched = false;
  for (auto v : records) touched |= v != 7;
  for (auto v : counts) touched |= v != 7;
  for (auto v : ws) touched |= v != 7;
  for (auto v : table) touched |= v != 7.f;
  for (auto v : heat) touched |= v != 7.f;
  for (auto v : out) touched |= v != 7.0;
  for (auto v : affine) touched |= v != 7.0;
  if (touched) { printf("FAIL: a buffer was written\n"); ++g_fail; }
  printf("%d calls, %d failures\n", g_calls, g_fail);
  return g_fail ? 1 : 0;
}
