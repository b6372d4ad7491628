// Stand-alone driver for the host-side argument checks of csrc/boundary.hip, meant for a sanitizer build of the HOST code (no GPU runs):
//
//   hipcc -std=c++17 --offload-arch=gfx950 -g -Xarch_host -fsanitize=address,undefined \
//         vickers-hardness-unet_amd/csrc/boundary.hip tests/diag/boundary_host_checks.hip -o boundary_host_checks && ./boundary_host_checks
//
// Every call below must come back with VK_ERR_ARG before anything touches a stream, and must leave its buffers as they were.  The
// two helpers of engine.hip that boundary.hip links against are replaced by the smallest stand-ins.
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

int main() {
  std::vector<float> src(256, 7.f), gt(256, 7.f), phi(256, 7.f), logits(256, 7.f), grad(256, 7.f), loss(4, 7.f);
  std::vector<int32_t> d2(256, 7), d2b(256, 7);
  std::vector<int64_t> ws(65536, 7), out(64, 7);
  const size_t W = ws.size() * 8;
  const float nanv = nanf("");
  auto off = [](void* p, int n) { return (void*)((char*)p + n); };

  if (vk_edt_workspace_bytes(3, 7, 5) != 420 || vk_edt_workspace_bytes(1, 4097, 1) != 0 || vk_edt_workspace_bytes(0, 1, 1) != 0 ||
      vk_boundary_stats_workspace_bytes(1, 0, 1) != 0 || vk_boundary_stats_workspace_bytes(1, 4, 4) > W) {
    printf("FAIL: workspace sizes\n");
    ++g_fail;
  }
  auto edt = [&](int b = 1, int h = 4, int w = 4, const void* s = nullptr, int kind = 1, float thr = 0.5f, int sites = 0, int32_t* o = nullptr,
                 void* wsp = nullptr, size_t wb = 64) {
    return vk_edt_sq(b, h, w, s ? s : src.data(), kind, thr, sites, o ? o : d2.data(), wsp ? wsp : ws.data(), wb, nullptr);
  };
  expect(edt(0), "batch", "edt: batch 0");
  expect(edt(65536), "batch", "edt: batch 65536");
  expect(edt(1, 0), "map size", "edt: h 0");
  expect(edt(1, 4, 4097), "map size", "edt: w 4097");
  expect(edt(1, 2147483647, 2147483647), "map size", "edt: INT_MAX sides");
  expect(edt(1, 4, 4, nullptr, 2), "kind 2", "edt: kind 2");
  expect(edt(1, 4, 4, nullptr, 1, nanv), "NaN", "edt: NaN threshold");
  expect(edt(1, 4, 4, nullptr, 1, 0.5f, 3), "sites 3", "edt: sites 3");
  expect(edt(1, 4, 4, nullptr, 1, 0.5f, -1), "sites -1", "edt: sites -1");
  expect(edt(1, 4, 4, nullptr, 1, 0.5f, 0x300), "sites", "edt: both row forms");
  expect(edt(1, 4, 4, nullptr, 1, 0.5f, 0x400), "sites", "edt: unknown bit");
  expect(edt(1, 4, 4, off(src.data(), 2)), "misaligned", "edt: misaligned fp32 source");
  expect(edt(1, 4, 4, nullptr, 1, 0.5f, 0, (int32_t*)off(d2.data(), 1)), "misaligned", "edt: misaligned d2");
  expect(edt(1, 4, 4, nullptr, 1, 0.5f, 0, nullptr, off(ws.data(), 2)), "misaligned", "edt: misaligned workspace");
  expect(edt(1, 4, 4, nullptr, 1, 0.5f, 0, nullptr, nullptr, 63), "workspace", "edt: short workspace");
  expect(vk_edt_sq(1, 4, 4, nullptr, 0, 0.5f, 0, d2.data(), ws.data(), 64, nullptr), "null buffer", "edt: null source");
  expect(vk_edt_sq(1, 4, 4, src.data(), 0, 0.5f, 0, nullptr, ws.data(), 64, nullptr), "null buffer", "edt: null d2");
  expect(vk_edt_sq(1, 4, 4, src.data(), 0, 0.5f, 0, d2.data(), nullptr, 64, nullptr), "null buffer", "edt: null workspace");

  expect(vk_boundary_phi(0, 4, 4, d2.data(), d2b.data(), phi.data(), nullptr), "batch", "phi: batch 0");
  expect(vk_boundary_phi(1, 4097, 4, d2.data(), d2b.data(), phi.data(), nullptr), "map size", "phi: h 4097");
  expect(vk_boundary_phi(1, 4, 4, nullptr, d2b.data(), phi.data(), nullptr), "null buffer", "phi: null d2_fg");
  expect(vk_boundary_phi(1, 4, 4, d2.data(), nullptr, phi.data(), nullptr), "null buffer", "phi: null d2_bg");
  expect(vk_boundary_phi(1, 4, 4, d2.data(), d2b.data(), nullptr, nullptr), "null buffer", "phi: null phi");
  expect(vk_boundary_phi(1, 4, 4, (int32_t*)off(d2.data(), 2), d2b.data(), phi.data(), nullptr), "misaligned", "phi: misaligned d2_fg");
  expect(vk_boundary_phi(1, 4, 4, d2.data(), d2b.data(), (float*)off(phi.data(), 3), nullptr), "misaligned", "phi: misaligned phi");

  int32_t tol[8] = {1, 4, 9, 0, 0, 0, 0, 0};
  auto stats = [&](int b = 1, int h = 4, int w = 4, int pk = 1, float pt = 0.5f, int gk = 1, float gtt = 0.5f, int nt = 3, const int32_t* t = nullptr,
                   int band2 = 4, void* o = nullptr, void* wsp = nullptr, size_t wb = 0) {
    return vk_boundary_stats(b, h, w, src.data(), pk, pt, gt.data(), gk, gtt, nt, t ? t : tol, band2, (vk_boundary_rec*)(o ? o : out.data()),
                             wsp ? wsp : ws.data(), wb ? wb : W, nullptr);
  };
  expect(stats(0), "batch", "stats: batch 0");
  expect(stats(1, 4, 0), "map size", "stats: w 0");
  expect(stats(1, 4, 4, 2), "pred kind 2", "stats: pred kind");
  expect(stats(1, 4, 4, 1, 0.5f, -3), "gt kind -3", "stats: gt kind");
  expect(stats(1, 4, 4, 1, nanv), "pred threshold", "stats: NaN pred threshold");
  expect(stats(1, 4, 4, 1, 0.5f, 1, nanv), "gt threshold", "stats: NaN gt threshold");
  expect(stats(1, 4, 4, 1, 0.5f, 1, 0.5f, -1), "tolerances", "stats: n_tol -1");
  expect(stats(1, 4, 4, 1, 0.5f, 1, 0.5f, 9), "tolerances", "stats: n_tol 9");
  { int32_t t[8] = {1, -4, 9, 0, 0, 0, 0, 0}; expect(stats(1, 4, 4, 1, 0.5f, 1, 0.5f, 3, t), "tol2[1]", "stats: negative tolerance"); }
  expect(stats(1, 4, 4, 1, 0.5f, 1, 0.5f, 3, nullptr, -1), "band2", "stats: negative band");
  expect(stats(1, 4, 4, 1, 0.5f, 1, 0.5f, 3, nullptr, 4, off(out.data(), 4)), "misaligned", "stats: misaligned records");
  expect(stats(1, 4, 4, 1, 0.5f, 1, 0.5f, 3, nullptr, 4, nullptr, off(ws.data(), 4)), "misaligned", "stats: misaligned workspace");
  expect(stats(1, 4, 4, 1, 0.5f, 1, 0.5f, 3, nullptr, 4, nullptr, nullptr, vk_boundary_stats_workspace_bytes(1, 4, 4) - 1), "workspace",
         "stats: short workspace");
  expect(vk_boundary_stats(1, 4, 4, nullptr, 1, 0.5f, gt.data(), 1, 0.5f, 3, tol, 4, (vk_boundary_rec*)out.data(), ws.data(), W, nullptr), "null buffer",
         "stats: null pred");
  expect(vk_boundary_stats(1, 4, 4, src.data(), 1, 0.5f, nullptr, 1, 0.5f, 3, tol, 4, (vk_boundary_rec*)out.data(), ws.data(), W, nullptr), "null buffer",
         "stats: null gt");
  expect(vk_boundary_stats(1, 4, 4, src.data(), 1, 0.5f, gt.data(), 1, 0.5f, 3, nullptr, 4, (vk_boundary_rec*)out.data(), ws.data(), W, nullptr), "tol2",
         "stats: null tolerances");
  expect(vk_boundary_stats(1, 4, 4, src.data(), 1, 0.5f, gt.data(), 1, 0.5f, 3, tol, 4, nullptr, ws.data(), W, nullptr), "null buffer", "stats: null records");
  expect(vk_boundary_stats(1, 4, 4, src.data(), 1, 0.5f, gt.data(), 1, 0.5f, 3, tol, 4, (vk_boundary_rec*)out.data(), nullptr, W, nullptr), "null buffer",
         "stats: null workspace");

  auto bl = [&](int n = 1, int c = 1, int hw = 16, const float* x = nullptr, const float* f = nullptr, float* g = nullptr, float* lo = nullptr,
                void* wsp = nullptr, size_t wb = VK_BOUNDARY_LOSS_WS_BYTES) {
    return vk_boundary_loss(n, c, hw, x ? x : logits.data(), f ? f : phi.data(), 1.f, g ? g : grad.data(), lo ? lo : loss.data(), wsp ? wsp : ws.data(), wb,
                            nullptr);
  };
  expect(bl(0), "batch", "loss: n 0");
  expect(bl(-2147483647 - 1), "batch", "loss: n INT_MIN");
  expect(bl(1, 0), "classes", "loss: c 0");
  expect(bl(1, 17), "classes", "loss: c 17");
  expect(bl(1, 1, 0), "plane", "loss: hw 0");
  expect(bl(1, 1, 16, (float*)off(logits.data(), 2)), "misaligned", "loss: misaligned logits");
  expect(bl(1, 1, 16, nullptr, (float*)off(phi.data(), 1)), "misaligned", "loss: misaligned phi");
  expect(bl(1, 1, 16, nullptr, nullptr, (float*)off(grad.data(), 2)), "misaligned", "loss: misaligned gradient");
  expect(bl(1, 1, 16, nullptr, nullptr, nullptr, (float*)off(loss.data(), 2)), "misaligned", "loss: misaligned output");
  expect(bl(1, 1, 16, nullptr, nullptr, nullptr, nullptr, off(ws.data(), 4)), "misaligned", "loss: misaligned workspace");
  expect(bl(1, 1, 16, nullptr, nullptr, nullptr, nullptr, nullptr, VK_BOUNDARY_LOSS_WS_BYTES - 1), "workspace", "loss: short workspace");
  expect(vk_boundary_loss(1, 1, 16, nullptr, phi.data(), 1.f, grad.data(), loss.data(), ws.data(), W, nullptr), "null buffer", "loss: null logits");
  expect(vk_boundary_loss(1, 1, 16, logits.data(), nullptr, 1.f, grad.data(), loss.data(), ws.data(), W, nullptr), "null buffer", "loss: null phi");
  expect(vk_boundary_loss(1, 1, 16, logits.data(), phi.data(), 1.f, grad.data(), nullptr, ws.data(), W, nullptr), "null buffer", "loss: null output");
  expect(vk_boundary_loss(1, 1, 16, logits.data(), phi.data(), 1.f, grad.data(), loss.data(), nullptr, W, nullptr), "null buffer", "loss: null workspace");

  bool touched = false;
  for (auto v : src) touched |= v != 7.f;
  for (auto v : gt) touched |= v != 7.f;
  for (auto v : phi) touched |= v != 7.f;
  for (auto v : logits) touched |= v != 7.f;
  for (auto v : grad) touched |= v != 7.f;
  for (auto v : loss) touched |= v != 7.f;
  for (auto v : d2) touched |= v != 7;
  for (auto v : d2b) touched |= v != 7;
  for (auto v : ws) touched |= v != 7;
  for (auto v : out) touched |= v != 7;
  if (touched) { printf("FAIL: a buffer was written\n"); ++g_fail; }
  printf("%d calls, %d failures\n", g_calls, g_fail);
  return g_fail ? 1 : 0;
}
