// Stand-alone driver for the host-side argument checks of csrc/render.hip, meant for a sanitizer build of the HOST code (no GPU runs):
//
//   hipcc -std=c++17 --offload-arch=gfx950 -g -Xarch_host -fsanitize=address,undefined \
//         vickers-hardness-unet_amd/csrc/render.hip tests/diag/render_host_checks.hip -o render_host_checks && ./render_host_checks
//
// Every call below must come back with VK_ERR_ARG before anything touches a stream, and must leave its buffers as they were; the glyph
// table is read through vk_render_glyph for every character and past both of its ends.  The two helpers of engine.hip that render.hip
// links against are replaced by the smallest stand-ins.
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
  std::vector<float> x(4096, 7.f), y(4096, 7.f), pr(4096, 7.f);
  std::vector<uint8_t> out(8192, 7), src(4096, 7), dst(4096, 7);
  std::vector<int64_t> recs(3 * 4 * 104 / 8, 7), prims(3 * 4 * 13, 7), views(64, 7);
  std::vector<int32_t> counts(4, 7), drawn(4, 7), skipped(4, 7);
  std::vector<double> aff(16, 7.0);
  const double mean[3] = {0.5, 0.5, 0.5}, stdv[3] = {0.25, 0.25, 0.25};
  const vk_render_blend good_bl{{0, 140, 255}, 0, 1.f, 0.35f, 0.f};
  vk_render_style good_st;
  memset(&good_st, 0, sizeof good_st);
  good_st.thickness = 2;
  good_st.text_scale = 2;

  // ---- glyphs
  uint8_t rows[7];
  int known = 0;
  for (int ch = -300; ch < 600; ++ch) {
    const int rc = vk_render_glyph(ch, rows);
    if (rc == VK_OK) ++known; else if (rc != VK_ERR_ARG) { printf("FAIL glyph %d: rc = %d\n", ch, rc); ++g_fail; }
  }
  if (known != 21) { printf("FAIL: %d glyphs, expected 21\n", known); ++g_fail; }
  expect(vk_render_glyph('0', nullptr), "null rows", "glyph: null rows");
  g_err[0] = 0;

  // ---- panels
  auto panels = [&](int N = 2, int H = 5, int W = 7, int64_t stride = 84, int flags = 0, const vk_render_blend* bl = nullptr, const float* xx = nullptr,
                    const double* mm = nullptr, uint8_t* oo = nullptr, bool null_out = false) {
    return vk_render_val_panels(N, H, W, xx ? xx : x.data(), y.data(), pr.data(), mm ? mm : mean, stdv, bl ? bl : &good_bl, flags,
                                null_out ? nullptr : (oo ? oo : out.data()), stride, nullptr);
  };
  expect(panels(0), "N = 0", "panels: N 0");
  expect(panels(65536), "N = 65536", "panels: N 65536");
  expect(panels(2, 0), "size", "panels: H 0");
  expect(panels(2, 5, 16385), "size", "panels: W too large");
  expect(panels(2, 5, 7, 83), "row stride", "panels: stride");
  expect(panels(2, 5, 7, ((int64_t)1 << 31) + 1), "row stride", "panels: stride too large");
  expect(panels(2, 5, 7, 84, 2), "unknown flags", "panels: flags");
  { vk_render_blend b = good_bl; b.alpha = NAN; expect(panels(2, 5, 7, 84, 0, &b), "blend weights", "panels: NaN alpha"); }
  { vk_render_blend b = good_bl; b.gamma = INFINITY; expect(panels(2, 5, 7, 84, 0, &b), "blend weights", "panels: infinite gamma"); }
  expect(vk_render_val_panels(2, 5, 7, x.data(), y.data(), pr.data(), mean, stdv, nullptr, 0, out.data(), 84, nullptr), "null blend", "panels: null blend");
  expect(panels(2, 5, 7, 84, 0, nullptr, (const float*)((const char*)x.data() + 2)), "misaligned", "panels: misaligned x");
  { const double m[3] = {0.5, NAN, 0.5}; expect(panels(2, 5, 7, 84, 0, nullptr, nullptr, m), "not finite", "panels: NaN mean"); }
  expect(panels(2, 5, 7, 84, 0, nullptr, nullptr, nullptr, nullptr, true), "null buffer", "panels: null output");
  expect(vk_render_val_panels(2, 5, 7, x.data(), nullptr, pr.data(), mean, stdv, &good_bl, 0, out.data(), 84, nullptr), "null buffer", "panels: null y");
  expect(vk_render_val_panels(2, 5, 7, x.data(), y.data(), pr.data(), nullptr, stdv, &good_bl, 0, out.data(), 84, nullptr), "null buffer", "panels: null mean");

  // ---- primitives
  auto prim = [&](int batch = 3, size_t stride = 104, size_t box = 8, int valid = 48, int diag = 96, int center = 40, int mode = 0, int M = 4,
                  const vk_render_style* st = nullptr, const void* r = nullptr, const int32_t* c = nullptr, vk_render_prim* p = nullptr) {
    return vk_render_primitives(batch, r ? r : recs.data(), stride, box, valid, diag, center, mode, c ? c : counts.data(), M, aff.data(),
                                st ? st : &good_st, p ? p : (vk_render_prim*)prims.data(), drawn.data(), skipped.data(), nullptr);
  };
  expect(prim(0), "batch", "primitives: batch 0");
  expect(prim(65536), "batch", "primitives: batch 65536");
  expect(prim(3, 100), "record stride", "primitives: stride");
  expect(prim(3, 104, 4), "record stride", "primitives: box offset 4");
  expect(prim(3, 104, 80), "record stride", "primitives: box offset 80");
  expect(prim(3, 104, 44, 8, 96, 40, 1), "record stride", "primitives: v offset");
  expect(prim(3, 104, 8, 4), "valid offset", "primitives: valid offset 4");
  expect(prim(3, 104, 8, 104), "valid offset", "primitives: valid offset 104");
  expect(prim(3, 104, 8, 48, 100), "diag offset", "primitives: diag offset 100");
  expect(prim(3, 104, 8, 48, 104), "diag offset", "primitives: diag offset 104");
  expect(prim(3, 104, 8, 48, 96, -1), "center offset", "primitives: center offset -1");
  expect(prim(3, 104, 8, 48, 96, 100), "center offset", "primitives: center offset 100");
  expect(prim(3, 104, 8, 48, 96, 40, 3), "coordinate mode", "primitives: mode 3");
  expect(prim(3, 104, 8, 48, 96, 40, 0, 0), "max_components", "primitives: max_components 0");
  expect(prim(3, 104, 8, 48, 96, 40, 0, 4097), "max_components", "primitives: max_components 4097");
  { vk_render_style s = good_st; s.thickness = 0; expect(prim(3, 104, 8, 48, 96, 40, 0, 4, &s), "thickness", "primitives: thickness 0"); }
  { vk_render_style s = good_st; s.thickness = 9; expect(prim(3, 104, 8, 48, 96, 40, 0, 4, &s), "thickness", "primitives: thickness 9"); }
  { vk_render_style s = good_st; s.text_scale = 0; expect(prim(3, 104, 8, 48, 96, 40, 0, 4, &s), "text_scale", "primitives: text_scale 0"); }
  { vk_render_style s = good_st; s.text_scale = 9; expect(prim(3, 104, 8, 48, 96, 40, 0, 4, &s), "text_scale", "primitives: text_scale 9"); }
  expect(prim(3, 104, 8, 48, 96, 40, 0, 4, nullptr, (const char*)recs.data() + 4), "misaligned", "primitives: misaligned records");
  expect(prim(3, 104, 8, 48, 96, 40, 0, 4, nullptr, nullptr, (const int32_t*)((const char*)counts.data() + 2)), "misaligned", "primitives: misaligned counts");
  expect(prim(3, 104, 8, 48, 96, 40, 0, 4, nullptr, nullptr, nullptr, (vk_render_prim*)((char*)prims.data() + 4)), "misaligned", "primitives: misaligned output");
  expect(vk_render_primitives(3, nullptr, 104, 8, 48, 96, 40, 0, counts.data(), 4, nullptr, &good_st, (vk_render_prim*)prims.data(), drawn.data(),
                              skipped.data(), nullptr), "null buffer", "primitives: null records");
  expect(vk_render_primitives(3, recs.data(), 104, 8, 48, 96, 40, 0, counts.data(), 4, nullptr, nullptr, (vk_render_prim*)prims.data(), drawn.data(),
                              skipped.data(), nullptr), "null buffer", "primitives: null style");
  expect(vk_render_primitives(3, recs.data(), 104, 8, 48, 96, 40, 0, counts.data(), 4, nullptr, &good_st, (vk_render_prim*)prims.data(), drawn.data(),
                              nullptr, nullptr), "null buffer", "primitives: null skipped");

  // ---- draw
  const vk_render_view good_v{4096, 21, 8192, 7, {256, 512, 1024}, {21, 21, 21}, 5, 7};
  auto draw = [&](vk_render_view v, int batch = 1, int kind = 0, float thresh = 0.5f, int flags = 0, int M = 4, const vk_render_blend* bl = nullptr,
                  const vk_render_prim* p = nullptr, const int32_t* d = nullptr, bool null_drawn = false, void* vd = nullptr) {
    return vk_render_draw(batch, &v, vd ? vd : views.data(), kind, thresh, bl ? bl : &good_bl, p ? p : (const vk_render_prim*)prims.data(),
                          null_drawn ? nullptr : (d ? d : drawn.data()), M, flags, nullptr);
  };
  expect(draw(good_v, 0), "batch", "draw: batch 0");
  expect(draw(good_v, 1, 2), "mask kind", "draw: mask kind");
  expect(draw(good_v, 1, 1, NAN), "thresh", "draw: NaN thresh");
  expect(draw(good_v, 1, 0, 0.5f, 2), "unknown flags", "draw: flags");
  expect(draw(good_v, 1, 0, 0.5f, 0, 0), "max_components", "draw: max_components 0");
  expect(draw(good_v, 1, 0, 0.5f, 0, 4097), "max_components", "draw: max_components 4097");
  { vk_render_blend b = good_bl; b.beta = NAN; expect(draw(good_v, 1, 0, 0.5f, 0, 4, &b), "blend weights", "draw: NaN beta"); }
  expect(draw(good_v, 1, 0, 0.5f, 0, 4, nullptr, (const vk_render_prim*)((const char*)prims.data() + 4)), "misaligned", "draw: misaligned list");
  expect(draw(good_v, 1, 0, 0.5f, 0, 4, nullptr, nullptr, (const int32_t*)((const char*)drawn.data() + 2)), "misaligned", "draw: misaligned counts");
  expect(draw(good_v, 1, 0, 0.5f, 0, 4, nullptr, nullptr, nullptr, true), "null buffer", "draw: list without counts");
  expect(draw(good_v, 1, 0, 0.5f, 0, 4, nullptr, nullptr, nullptr, false, (char*)views.data() + 4), "misaligned", "draw: misaligned table");
  expect(vk_render_draw(1, nullptr, views.data(), 0, 0.5f, &good_bl, nullptr, nullptr, 0, 0, nullptr), "null buffer", "draw: null table");
  expect(vk_render_draw(1, &good_v, nullptr, 0, 0.5f, &good_bl, nullptr, nullptr, 0, 0, nullptr), "null buffer", "draw: null device table");
  expect(vk_render_draw(1, &good_v, views.data(), 0, 0.5f, nullptr, nullptr, nullptr, 0, 0, nullptr), "null blend", "draw: null blend");
  { vk_render_view v = good_v; v.h = 0; expect(draw(v), "size", "draw: h 0"); }
  { vk_render_view v = good_v; v.w = 16385; v.src_stride = 3 * 16385; expect(draw(v), "size", "draw: w too large"); }
  { vk_render_view v = good_v; v.src = 0; expect(draw(v), "null address", "draw: null source"); }
  { vk_render_view v = good_v; v.mask = 0; expect(draw(v), "null address", "draw: null mask"); }
  { vk_render_view v = good_v; v.src_stride = 20; expect(draw(v), "row stride", "draw: source stride"); }
  { vk_render_view v = good_v; v.mask_stride = 6; expect(draw(v), "mask row stride", "draw: mask stride"); }
  { vk_render_view v = good_v; v.mask_stride = 27; expect(draw(v, 1, 1), "mask row stride", "draw: float mask stride"); }
  { vk_render_view v = good_v; v.mask_stride = 28; v.mask = 8194; expect(draw(v, 1, 1), "mask row stride", "draw: misaligned float mask"); }
  { vk_render_view v = good_v; v.out_stride[2] = 20; expect(draw(v), "output 2", "draw: output stride"); }
  { vk_render_view v = good_v; v.out[0] = v.out[1] = v.out[2] = 0; expect(draw(v), "no output", "draw: no output"); }
  { vk_render_view v[2] = {good_v, good_v}; v[1].h = -1;
    expect(vk_render_draw(2, v, views.data(), 0, 0.5f, &good_bl, nullptr, nullptr, 0, 0, nullptr), "map 1", "draw: the second map"); }

  // ---- reduce
  auto reduce = [&](int h = 5, int w = 7, int k = 2, int64_t ss = 21, int64_t ds = 12, bool null_src = false, bool null_dst = false) {
    return vk_render_reduce(h, w, k, null_src ? nullptr : src.data(), ss, null_dst ? nullptr : dst.data(), ds, nullptr);
  };
  expect(reduce(0), "size", "reduce: h 0");
  expect(reduce(5, 16385), "size", "reduce: w too large");
  expect(reduce(5, 7, 0), "k = 0", "reduce: k 0");
  expect(reduce(5, 7, 17), "k = 17", "reduce: k 17");
  expect(reduce(5, 7, 2, 20), "source row stride", "reduce: source stride");
  expect(reduce(5, 7, 2, 21, 11), "output row stride", "reduce: output stride");
  expect(reduce(5, 7, 2, 21, 12, true), "null buffer", "reduce: null source");
  expect(reduce(5, 7, 2, 21, 12, false, true), "null buffer", "reduce: null output");

  bool touched = false;
  for (auto v : x) touched |= v != 7.f;
  for (auto v : y) touched |= v != 7.f;
  for (auto v : pr) touched |= v != 7.f;
  for (auto v : out) touched |= v != 7;
  for (auto v : src) touched |= v != 7;
  for (auto v : dst) touched |= v != 7;
  for (auto v : recs) touched |= v != 7;
  for (auto v : prims) touched |= v != 7;
  for (auto v : views) touched |= v != 7;
  for (auto v : counts) touched |= v != 7;
  for (auto v : drawn) touched |= v != 7;
  for (auto v : skipped) touched |= v != 7;
  for (auto v : aff) touched |= v != 7.0;
  if (touched) { printf("FAIL: a buffer was written\n"); ++g_fail; }
  printf("%d calls, %d failures\n", g_calls, g_fail);
  return g_fail ? 1 : 0;
}
