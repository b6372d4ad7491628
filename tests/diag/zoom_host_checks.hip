// Stand-alone driver for the host-side argument checks of csrc/zoom.hip, meant for a sanitizer build of the HOST code (no GPU runs):
//
//   hipcc -std=c++17 --offload-arch=gfx950 -g -Xarch_host -fsanitize=address,undefined \
//         vickers-hardness-unet_amd/csrc/zoom.hip tests/diag/zoom_host_checks.hip -o zoom_host_checks && ./zoom_host_checks
//
// Every call below must come back with VK_ERR_ARG before anything touches a stream, and must leave its buffers as they were.  The
// two helpers of engine.hip that zoom.hip links against are replaced by the smallest stand-ins.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <cmath>
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
  std::vector<int64_t> recs(3 * 4 * 96 / 8, 7), win(64 * 5, 7), quads(3 * 4 * 25, 7), coarse(3 * 4 * 25, 7), outq(3 * 4 * 25, 7), tabdev(16, 7);
  std::vector<int32_t> counts(4, 7), sizes(8, 7), nwin(2, 7), status(16, 7);
  std::vector<double> aff(16, 7.0), scale(16, 7.0);
  std::vector<float> out(4096, 7.f);
  vk_zoom_window* W = (vk_zoom_window*)win.data();
  vk_subpix_quad* Q = (vk_subpix_quad*)quads.data();
  vk_subpix_quad* Cq = (vk_subpix_quad*)coarse.data();
  vk_subpix_quad* O = (vk_subpix_quad*)outq.data();
  const vk_zoom_params good{64, 8, 1.5, 1.0, 32.0};

  auto windows = [&](vk_zoom_params p, int batch = 3, size_t stride = 96, size_t box = 8, int valid = -1, int M = 4, const void* r = nullptr,
                     const int32_t* c = nullptr, bool null_sizes = false) {
    return vk_zoom_windows(&p, batch, r ? r : recs.data(), stride, box, valid, c ? c : counts.data(), M, aff.data(),
                           null_sizes ? nullptr : sizes.data(), W, nwin.data(), nullptr);
  };
  expect(vk_zoom_windows(nullptr, 3, recs.data(), 96, 8, -1, counts.data(), 4, nullptr, sizes.data(), W, nwin.data(), nullptr), "null parameters",
         "windows: null parameters");
  { vk_zoom_params p = good; p.S = 0; expect(windows(p), "S = 0", "windows: S = 0"); }
  { vk_zoom_params p = good; p.S = 16385; expect(windows(p), "S = 16385", "windows: S too large"); }
  { vk_zoom_params p = good; p.s_min = 0.2; expect(windows(p), "s_min", "windows: s_min"); }
  { vk_zoom_params p = good; p.s_min = 2.0; p.s_max = 1.5; expect(windows(p), "s_min", "windows: s_min > s_max"); }
  { vk_zoom_params p = good; p.s_max = 64.5; expect(windows(p), "s_max", "windows: s_max"); }
  { vk_zoom_params p = good; p.s_min = NAN; expect(windows(p), "s_min", "windows: NaN s_min"); }
  { vk_zoom_params p = good; p.margin = 0.5; expect(windows(p), "margin", "windows: margin"); }
  { vk_zoom_params p = good; p.margin = NAN; expect(windows(p), "margin", "windows: NaN margin"); }
  { vk_zoom_params p = good; p.max_windows = 0; expect(windows(p), "max_windows", "windows: max_windows 0"); }
  { vk_zoom_params p = good; p.max_windows = 65536; expect(windows(p), "max_windows", "windows: max_windows 65536"); }
  expect(windows(good, 0), "batch", "windows: batch 0");
  expect(windows(good, 65536), "batch", "windows: batch 65536");
  expect(windows(good, 3, 94), "record stride", "windows: stride");
  expect(windows(good, 3, 96, 72), "record stride", "windows: box offset");
  expect(windows(good, 3, 96, 8, 96), "valid offset", "windows: valid offset");
  expect(windows(good, 3, 96, 8, -1, 0), "max_components", "windows: max_components 0");
  expect(windows(good, 3, 96, 8, -1, 4097), "max_components", "windows: max_components 4097");
  expect(windows(good, 3, 96, 8, -1, 4, (const char*)recs.data() + 1), "misaligned", "windows: misaligned records");
  expect(windows(good, 3, 96, 8, -1, 4, nullptr, (const int32_t*)((const char*)counts.data() + 2)), "misaligned", "windows: misaligned counts");
  expect(windows(good, 3, 96, 8, -1, 4, nullptr, nullptr, true), "null buffer", "windows: null sizes");

  vk_zoom_image tab[2] = {{4096, 5, 7, 21}, {8192, 1, 1, 8}};
  auto gather = [&](int n = 2, int S = 8, int n_images = 2, int pad = 0, int flags = 0, const vk_zoom_image* t = nullptr, float* o = nullptr) {
    return vk_zoom_gather(n, S, W, n_images, t ? t : tab, tabdev.data(), pad, flags, o ? o : out.data(), nullptr);
  };
  expect(gather(0), "windows", "gather: n 0");
  expect(gather(65536), "windows", "gather: n 65536");
  expect(gather(2, 0), "S = 0", "gather: S 0");
  expect(gather(2, 16385), "S = 16385", "gather: S too large");
  expect(gather(2, 8, 0), "images", "gather: no images");
  expect(gather(2, 8, 2, -1), "pad_value", "gather: pad -1");
  expect(gather(2, 8, 2, 256), "pad_value", "gather: pad 256");
  expect(gather(2, 8, 2, 0, 2), "unknown flags", "gather: flags");
  expect(vk_zoom_gather(2, 8, nullptr, 2, tab, tabdev.data(), 0, 0, out.data(), nullptr), "null buffer", "gather: null windows");
  expect(vk_zoom_gather(2, 8, W, 2, nullptr, tabdev.data(), 0, 0, out.data(), nullptr), "null buffer", "gather: null table");
  expect(vk_zoom_gather(2, 8, W, 2, tab, nullptr, 0, 0, out.data(), nullptr), "null buffer", "gather: null device table");
  expect(vk_zoom_gather(2, 8, W, 2, tab, tabdev.data(), 0, 0, nullptr, nullptr), "null buffer", "gather: null output");
  expect(gather(2, 8, 2, 0, 0, nullptr, (float*)((char*)out.data() + 2)), "misaligned", "gather: misaligned output");
  { vk_zoom_image t[2] = {tab[0], {0, 4, 4, 12}}; expect(gather(2, 8, 2, 0, 0, t), "null address", "gather: null image"); }
  { vk_zoom_image t[2] = {tab[0], {64, 0, 4, 12}}; expect(gather(2, 8, 2, 0, 0, t), "size", "gather: h 0"); }
  { vk_zoom_image t[2] = {tab[0], {64, 4, 16385, 3 * 16385}}; expect(gather(2, 8, 2, 0, 0, t), "size", "gather: w too large"); }
  { vk_zoom_image t[2] = {tab[0], {64, 4, 4, 11}}; expect(gather(2, 8, 2, 0, 0, t), "row stride", "gather: stride"); }

  auto merge = [&](int S = 64, double agree = 0.25, int n = 2, size_t stride = 96, int valid = -1, int M2 = 4, int batch = 3, int M = 4,
                   const vk_zoom_window* w = nullptr, bool null_w = false, int32_t* st = nullptr) {
    return vk_zoom_merge(S, agree, n, null_w ? nullptr : (w ? w : W), recs.data(), stride, 8, valid, counts.data(), M2, Q, batch, M, sizes.data(), Cq, O,
                         st ? st : status.data(), scale.data(), nullptr);
  };
  expect(merge(0), "S = 0", "merge: S 0");
  expect(merge(64, -0.1), "agree", "merge: agree < 0");
  expect(merge(64, NAN), "agree", "merge: NaN agree");
  expect(merge(64, INFINITY), "agree", "merge: infinite agree");
  expect(merge(64, 0.25, -1), "windows", "merge: n -1");
  expect(merge(64, 0.25, 65536), "windows", "merge: n 65536");
  expect(merge(64, 0.25, 2, 90), "record stride", "merge: stride");
  expect(merge(64, 0.25, 2, 96, 2), "valid offset", "merge: valid offset");
  expect(merge(64, 0.25, 2, 96, -1, 0), "max_components2", "merge: max_components2");
  expect(merge(64, 0.25, 2, 96, -1, 4, 0), "batch", "merge: batch 0");
  expect(merge(64, 0.25, 2, 96, -1, 4, 3, 0), "max_components", "merge: max_components 0");
  expect(merge(64, 0.25, 2, 96, -1, 4, 3, 4, nullptr, true), "null second-pass", "merge: null windows");
  expect(merge(64, 0.25, 2, 96, -1, 4, 3, 4, (const vk_zoom_window*)((const char*)W + 4)), "misaligned second-pass", "merge: misaligned windows");
  expect(merge(64, 0.25, 2, 96, -1, 4, 3, 4, nullptr, false, (int32_t*)((char*)status.data() + 2)), "misaligned", "merge: misaligned status");
  expect(vk_zoom_merge(64, 0.25, 0, nullptr, nullptr, 0, 0, -1, nullptr, 0, nullptr, 3, 4, sizes.data(), nullptr, O, status.data(), scale.data(), nullptr),
         "null buffer", "merge: null coarse");

  bool touched = false;
  for (auto v : recs) touched |= v != 7;
  for (auto v : win) touched |= v != 7;
  for (auto v : quads) touched |= v != 7;
  for (auto v : coarse) touched |= v != 7;
  for (auto v : outq) touched |= v != 7;
  for (auto v : tabdev) touched |= v != 7;
  for (auto v : counts) touched |= v != 7;
  for (auto v : sizes) touched |= v != 7;
  for (auto v : nwin) touched |= v != 7;
  for (auto v : status) touched |= v != 7;
  for (auto v : aff) touched |= v != 7.0;
  for (auto v : scale) touched |= v != 7.0;
  for (auto v : out) touched |= v != 7.f;
  if (touched) { printf("FAIL: a buffer was written\n"); ++g_fail; }
  printf("%d calls, %d failures\n", g_calls, g_fail);
  return g_fail ? 1 : 0;
}
