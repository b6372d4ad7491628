// Stand-alone driver for the host-side argument checks of the entry points of vk.inputs (csrc/elementwise.hip: vk_input_transform_c,
// vk_input_mix; csrc/conv_wgrad.hip: vk_stem_wgrad_c, vk_stem_wgrad_bn_c, vk_stem_dgrad_c), meant for a sanitizer build of the HOST code
// (no GPU runs):
//
//   hipcc -std=c++17 --offload-arch=gfx950 -g -Xarch_host -fsanitize=address,undefined -Ivickers-hardness-unet_amd/csrc \
//         vickers-hardness-unet_amd/csrc/elementwise.hip vickers-hardness-unet_amd/csrc/conv_wgrad.hip \
//         vickers-hardness-unet_amd/csrc/wgrad_halo.hip tests/diag/inputs_host_checks.hip -o inputs_host_checks && ./inputs_host_checks
//
// Every call below must come back with VK_ERR_ARG before anything touches a stream, and must leave its buffers as they were.  The
// helpers of engine.hip that the three sources link against are replaced by the smallest stand-ins; a ProfScope (every launch builds one)
// aborts.  (A vk_dtype outside the enumeration is left to tests/test_inputs_cpu.py: forming one in C++ is itself undefined.)
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
int reserved_cus() { return 0; }
const char* prof_tag(char*, size_t, const char* tag, const ProfDetail&) { return tag; }
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
  std::vector<float> x(4096, 7.f), x4(4096, 7.f), dz(4096, 7.f), z(4096, 7.f), coef(4096, 7.f), w(4096, 7.f), dw(4096, 7.f), dx(4096, 7.f),
      ws(4096, 7.f), out(4096, 7.f), M(12, 7.f), b(4, 7.f);
  const vk_dtype types[2] = {VK_F32, VK_BF16};
  const int bad_cin[4] = {0, 5, -3, 1 << 20};
  for (vk_dtype dt : types)
    for (int cin : bad_cin) {
      expect(vk_input_transform_c(dt, 1, cin, 8, 32, x.data(), x4.data(), nullptr), "cin", "transform: cin");
      expect(vk_stem_wgrad_c(dt, 1, 8, 32, cin, x4.data(), dz.data(), dw.data(), ws.data(), 4096, nullptr), "cin", "wgrad: cin");
      expect(vk_stem_wgrad_bn_c(dt, 1, 8, 32, cin, x4.data(), dz.data(), z.data(), coef.data(), dw.data(), nullptr, 0, nullptr), "cin", "wgrad_bn: cin");
      expect(vk_stem_dgrad_c(dt, 1, 8, 32, cin, dz.data(), nullptr, nullptr, w.data(), dx.data(), nullptr), "cin", "dgrad: cin");
    }
  for (int cout : bad_cin) expect(vk_input_mix(1, cout, 16, x.data(), M.data(), nullptr, out.data(), nullptr), "cout", "mix: cout");
  expect(vk_input_transform_c(VK_F32, 1, 1, 8, 32, nullptr, x4.data(), nullptr), "bad argument", "transform: null x");
  expect(vk_input_transform_c(VK_F32, 1, 1, 8, 32, x.data(), nullptr, nullptr), "bad argument", "transform: null x4");
  expect(vk_input_transform_c(VK_F32, 0, 1, 8, 32, x.data(), x4.data(), nullptr), "bad argument", "transform: N 0");
  expect(vk_input_transform_c(VK_F32, 1, 1, 0, 32, x.data(), x4.data(), nullptr), "bad argument", "transform: H 0");
  expect(vk_input_transform_c(VK_F32, 65536, 1, 8, 32, x.data(), x4.data(), nullptr), "too large", "transform: N 65536");
  expect(vk_stem_wgrad_c(VK_F32, 1, 8, 32, 1, nullptr, dz.data(), dw.data(), nullptr, 0, nullptr), "null", "wgrad: null x4");
  expect(vk_stem_wgrad_c(VK_F32, 1, 8, 32, 1, x4.data(), nullptr, dw.data(), nullptr, 0, nullptr), "null", "wgrad: null dz");
  expect(vk_stem_wgrad_c(VK_F32, 1, 8, 32, 1, x4.data(), dz.data(), nullptr, nullptr, 0, nullptr), "null", "wgrad: null dw");
  expect(vk_stem_wgrad_bn_c(VK_BF16, 1, 8, 32, 1, x4.data(), dz.data(), nullptr, coef.data(), dw.data(), nullptr, 0, nullptr), "null", "wgrad_bn: null z");
  expect(vk_stem_wgrad_bn_c(VK_BF16, 1, 8, 32, 1, x4.data(), dz.data(), z.data(), nullptr, dw.data(), nullptr, 0, nullptr), "null", "wgrad_bn: null coef");
  expect(vk_stem_dgrad_c(VK_F32, 1, 8, 32, 1, nullptr, nullptr, nullptr, w.data(), dx.data(), nullptr), "null", "dgrad: null g");
  expect(vk_stem_dgrad_c(VK_F32, 1, 8, 32, 1, dz.data(), nullptr, nullptr, nullptr, dx.data(), nullptr), "null", "dgrad: null w");
  expect(vk_stem_dgrad_c(VK_F32, 1, 8, 32, 1, dz.data(), nullptr, nullptr, w.data(), nullptr, nullptr), "null", "dgrad: null dx");
  expect(vk_stem_dgrad_c(VK_F32, 1, 8, 32, 1, dz.data(), nullptr, coef.data(), w.data(), dx.data(), nullptr), "null", "dgrad: coef without z");
  expect(vk_stem_dgrad_c(VK_F32, 1, 8, 48, 1, dz.data(), nullptr, nullptr, w.data(), dx.data(), nullptr), "W=48", "dgrad: W 48");
  expect(vk_stem_dgrad_c(VK_F32, 1, 12, 32, 1, dz.data(), nullptr, nullptr, w.data(), dx.data(), nullptr), "H=12", "dgrad: H 12");
  expect(vk_stem_dgrad_c(VK_F32, 0, 8, 32, 1, dz.data(), nullptr, nullptr, w.data(), dx.data(), nullptr), "H=8", "dgrad: N 0");
  expect(vk_input_mix(1, 1, 16, nullptr, M.data(), nullptr, out.data(), nullptr), "null", "mix: null x3");
  expect(vk_input_mix(1, 1, 16, x.data(), nullptr, nullptr, out.data(), nullptr), "null", "mix: null M");
  expect(vk_input_mix(1, 1, 16, x.data(), M.data(), b.data(), nullptr, nullptr), "null", "mix: null out");
  expect(vk_input_mix(0, 1, 16, x.data(), M.data(), nullptr, out.data(), nullptr), "N=0", "mix: N 0");
  expect(vk_input_mix(65536, 1, 16, x.data(), M.data(), nullptr, out.data(), nullptr), "N=65536", "mix: N 65536");
  expect(vk_input_mix(1, 1, 0, x.data(), M.data(), nullptr, out.data(), nullptr), "hw=0", "mix: hw 0");
  expect(vk_input_mix(1, 1, 16, (const float*)((const char*)x.data() + 2), M.data(), nullptr, out.data(), nullptr), "unaligned", "mix: x3 + 2 bytes");
  expect(vk_input_mix(1, 1, 16, x.data(), M.data(), nullptr, (float*)((char*)out.data() + 1), nullptr), "unaligned", "mix: out + 1 byte");
  for (const std::vector<float>* v : {&x, &x4, &dz, &z, &coef, &w, &dw, &dx, &ws, &out, &M, &b})
    for (float f : *v)
      if (f != 7.f) {
        printf("FAIL: a refused call wrote a buffer\n");
        ++g_fail;
        break;
      }
  printf("%d calls, %d failures\n", g_calls, g_fail);
  return g_fail ? 1 : 0;
}
