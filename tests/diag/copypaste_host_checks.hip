// Stand-alone driver for the host-side argument checks of csrc/copypaste.hip, meant for a sanitizer build of the HOST code (no GPU runs):
//
//   hipcc -std=c++17 --offload-arch=gfx950 -g -Xarch_host -fsanitize=address,undefined \
//         vickers-hardness-unet_amd/csrc/copypaste.hip tests/diag/copypaste_host_checks.hip -o copypaste_host_checks && ./copypaste_host_checks
//
// Every call below must come back with VK_ERR_ARG before anything touches a stream, and must leave its buffers as they were.  The
// two helpers of engine.hip that copypaste.hip links against are replaced by the smallest stand-ins.
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
  std::vector<int32_t> slots(64, 7), boxes(64, 7), base(8, 7), recs_dev(256, 7);
  std::vector<uint8_t> kept(64, 7), alpha(64, 7), images(256, 7), masks(64, 7), out_rgb(256, 7), out_mask(64, 7);
  char* odd = (char*)slots.data() + 2;

  expect(vk_cp_boxes(0, 4, 4, slots.data(), 2, boxes.data(), nullptr), "batch", "boxes: batch 0");
  expect(vk_cp_boxes(65536, 4, 4, slots.data(), 2, boxes.data(), nullptr), "batch", "boxes: batch 65536");
  expect(vk_cp_boxes(1, 0, 4, slots.data(), 2, boxes.data(), nullptr), "map size", "boxes: h 0");
  expect(vk_cp_boxes(1, 4, 16385, slots.data(), 2, boxes.data(), nullptr), "map size", "boxes: w too large");
  expect(vk_cp_boxes(1, 4, 4, slots.data(), 0, boxes.data(), nullptr), "max_slots", "boxes: max_slots 0");
  expect(vk_cp_boxes(1, 4, 4, slots.data(), 257, boxes.data(), nullptr), "max_slots", "boxes: max_slots 257");
  expect(vk_cp_boxes(1, 4, 4, nullptr, 2, boxes.data(), nullptr), "null buffer", "boxes: null slots");
  expect(vk_cp_boxes(1, 4, 4, slots.data(), 2, nullptr, nullptr), "null buffer", "boxes: null boxes");
  expect(vk_cp_boxes(1, 4, 4, (const int32_t*)odd, 2, boxes.data(), nullptr), "misaligned", "boxes: misaligned slots");
  expect(vk_cp_boxes(1, 4, 4, slots.data(), 2, (int32_t*)((char*)boxes.data() + 1), nullptr), "misaligned", "boxes: misaligned boxes");

  expect(vk_cp_alpha(0, 4, 4, slots.data(), kept.data(), alpha.data(), nullptr), "batch", "alpha: batch 0");
  expect(vk_cp_alpha(1, 16385, 4, slots.data(), kept.data(), alpha.data(), nullptr), "map size", "alpha: h too large");
  expect(vk_cp_alpha(1, 4, 0, slots.data(), kept.data(), alpha.data(), nullptr), "map size", "alpha: w 0");
  expect(vk_cp_alpha(1, 4, 4, nullptr, kept.data(), alpha.data(), nullptr), "null buffer", "alpha: null slots");
  expect(vk_cp_alpha(1, 4, 4, slots.data(), nullptr, alpha.data(), nullptr), "null buffer", "alpha: null kept");
  expect(vk_cp_alpha(1, 4, 4, slots.data(), kept.data(), nullptr, nullptr), "null buffer", "alpha: null alpha");
  expect(vk_cp_alpha(1, 4, 4, (const int32_t*)odd, kept.data(), alpha.data(), nullptr), "misaligned", "alpha: misaligned slots");

  const vk_cp_rec good{1, 1, 2, 3, 4, 5, -3, 6, 7, 16};          // S = 8
  std::vector<vk_cp_rec> recs(16, good);
  int32_t counts[2] = {1, 2};
  auto paste = [&](int n = 2, int S = 8, int n_items = 2, const uint8_t* im = nullptr, uint8_t* o = nullptr, const int32_t* c = nullptr) {
    return vk_cp_paste(n, S, n_items, im ? im : images.data(), masks.data(), kept.data(), alpha.data(), base.data(), c ? c : counts, recs.data(),
                       recs_dev.data(), o ? o : out_rgb.data(), out_mask.data(), nullptr);
  };
  expect(paste(0), "batch", "paste: n 0");
  expect(paste(65536), "batch", "paste: n 65536");
  expect(paste(2, 0), "S = 0", "paste: S 0");
  expect(paste(2, 4097), "S = 4097", "paste: S too large");
  expect(paste(2, 8, 0), "no items", "paste: no items");
  expect(paste(2, 8, 2, images.data() + 2), "misaligned", "paste: misaligned images");
  expect(paste(2, 8, 2, nullptr, out_rgb.data() + 1), "misaligned", "paste: misaligned output");
  expect(vk_cp_paste(2, 8, 2, nullptr, masks.data(), kept.data(), alpha.data(), base.data(), counts, recs.data(), recs_dev.data(), out_rgb.data(),
                     out_mask.data(), nullptr), "null buffer", "paste: null images");
  expect(vk_cp_paste(2, 8, 2, images.data(), masks.data(), kept.data(), alpha.data(), nullptr, counts, recs.data(), recs_dev.data(), out_rgb.data(),
                     out_mask.data(), nullptr), "null buffer", "paste: null base index");
  expect(vk_cp_paste(2, 8, 2, images.data(), masks.data(), kept.data(), alpha.data(), base.data(), nullptr, recs.data(), recs_dev.data(),
                     out_rgb.data(), out_mask.data(), nullptr), "null buffer", "paste: null counts");
  expect(vk_cp_paste(2, 8, 2, images.data(), masks.data(), kept.data(), alpha.data(), base.data(), counts, nullptr, recs_dev.data(), out_rgb.data(),
                     out_mask.data(), nullptr), "null buffer", "paste: null records");
  expect(vk_cp_paste(2, 8, 2, images.data(), masks.data(), kept.data(), alpha.data(), base.data(), counts, recs.data(), nullptr, out_rgb.data(),
                     out_mask.data(), nullptr), "null buffer", "paste: null record scratch");
  expect(vk_cp_paste(2, 8, 2, images.data(), masks.data(), kept.data(), alpha.data(), base.data(), counts, recs.data(), recs_dev.data(), out_rgb.data(),
                     nullptr, nullptr), "null buffer", "paste: null mask output");
  { int32_t c[2] = {1, 9}; expect(paste(2, 8, 2, nullptr, nullptr, c), "count 9", "paste: count 9"); }
  { int32_t c[2] = {-1, 0}; expect(paste(2, 8, 2, nullptr, nullptr, c), "count -1", "paste: count -1"); }
  auto bad = [&](int field, int32_t value, const char* word, const char* what) {
    int32_t* f = (int32_t*)&recs[8 + 1];                          // sample 1, record 1
    const int32_t keep = f[field];
    f[field] = value;
    expect(paste(), word, what);
    f[field] = keep;
  };
  bad(0, 2, "donor 2", "paste: donor 2");
  bad(0, -1, "donor -1", "paste: donor -1");
  bad(3, 0, "donor box", "paste: sw 0");
  bad(4, 0, "donor box", "paste: sh 0");
  bad(1, -1, "donor box", "paste: sx0 -1");
  bad(2, -1, "donor box", "paste: sy0 -1");
  bad(1, 6, "donor box", "paste: donor box over the right edge");
  bad(2, 5, "donor box", "paste: donor box over the bottom edge");
  bad(3, 2147483647, "donor box", "paste: sw INT_MAX");
  bad(1, 2147483647, "donor box", "paste: sx0 INT_MAX");
  bad(5, 8, "d4 8", "paste: d4 8");
  bad(5, -1, "d4 -1", "paste: d4 -1");
  bad(8, 0, "destination size", "paste: dw 0");
  bad(9, 17, "destination size", "paste: dh 17");
  bad(8, 2147483647, "destination size", "paste: dw INT_MAX");
  bad(6, -17, "destination origin", "paste: dx0 -17");
  bad(7, 17, "destination origin", "paste: dy0 17");
  bad(7, -2147483647 - 1, "destination origin", "paste: dy0 INT_MIN");

  bool touched = false;
  for (auto v : slots) touched |= v != 7;
  for (auto v : boxes) touched |= v != 7;
  for (auto v : base) touched |= v != 7;
  for (auto v : recs_dev) touched |= v != 7;
  for (auto v : kept) touched |= v != 7;
  for (auto v : alpha) touched |= v != 7;
  for (auto v : images) touched |= v != 7;
  for (auto v : masks) touched |= v != 7;
  for (auto v : out_rgb) touched |= v != 7;
  for (auto v : out_mask) touched |= v != 7;
  if (touched) { printf("FAIL: a buffer was written\n"); ++g_fail; }
  printf("%d calls, %d failures\n", g_calls, g_fail);
  return g_fail ? 1 : 0;
}
