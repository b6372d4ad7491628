// Stand-alone driver for the host-side argument checks of csrc/kp_loss.hip, meant for a sanitizer build of the HOST code (no GPU runs):
//
//   hipcc -std=c++17 --offload-arch=gfx950 -g -Xarch_host -fsanitize=address,undefined \
//         vickers-hardness-unet_amd/csrc/kp_loss.hip tests/diag/kp_loss_host_checks.hip -o kp_loss_host_checks && ./kp_loss_host_checks
//
// Every call below must come back with VK_ERR_ARG before anything touches a stream, and must leave its buffers as they were.  The
// two helpers of engine.hip that kp_loss.hip links against are replaced by the smallest stand-ins.  vk_unet_loss_kp needs a plan and
// lives in engine.hip; its checks of the configuration are vk::kp_check and vk::kp_check_workspace, which are driven here directly.
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

static vk_kp_loss_cfg good() {
  vk_kp_loss_cfg c;
  memset(&c, 0, sizeof c);
  c.struct_size = sizeof c;
  c.heat_planes = 2;
  c.bce_planes = 1;
  c.w_heat = c.w_bce = 1.f;
  c.alpha = 2;
  c.beta = 4;
  c.pos_threshold = 1.f;
  for (float& v : c.pos_weight) v = 1.f;
  return c;
}

struct Args {
  int N = 2, C = 2, HW = 32;
  size_t ws_bytes = (size_t)1 << 40;
  float grad_scale = 1.f;
  int accumulate = 0;
};

int main() {
  std::vector<float> x(256, 7.f), y(256, 7.f), dl(256, 7.f), out(8, 7.f);
  std::vector<int64_t> pos(16, 7);
  std::vector<double> ws(64, 7.0);

  auto K = [&](const vk_kp_loss_cfg* c, const Args& a, const float* xp, const float* yp, void* w, float* o) {
    return vk_kp_loss(c, a.N, a.C, a.HW, xp, yp, w, a.ws_bytes, o, pos.data(), dl.data(), a.grad_scale, a.accumulate, nullptr);
  };
  auto Kn = [&](const vk_kp_loss_cfg& c, const Args& a) { return K(&c, a, x.data(), y.data(), ws.data(), out.data()); };

  if (vk_kp_loss_cfg_size() != sizeof(vk_kp_loss_cfg) || sizeof(vk_kp_loss_cfg) != 100) { printf("FAIL: structure size\n"); ++g_fail; }
  // ---- the configuration
  {
    Args a;
    vk_kp_loss_cfg c = good();
    expect(K(nullptr, a, x.data(), y.data(), ws.data(), out.data()), "null configuration", "null configuration");
    c.struct_size = 96; expect(Kn(c, a), "struct_size", "struct_size 96");
    c = good(); c.struct_size = 0; expect(Kn(c, a), "struct_size", "struct_size 0");
    c = good(); c.heat_planes = c.bce_planes = 0; expect(Kn(c, a), "empty", "both masks empty");
    c = good(); c.heat_planes = 3; expect(Kn(c, a), "overlap", "masks overlap");
    c = good(); c.heat_planes = 4; expect(Kn(c, a), "plane >= C", "heat bit 2 at C = 2");
    c = good(); c.bce_planes = 1u << 31; expect(Kn(c, a), "plane >= C", "bce bit 31");
    c = good(); c.bce_planes = 1u << 16; a.C = 16; expect(Kn(c, a), "plane >= C", "bce bit 16 at C = 16"); a = Args();
    c = good(); c.w_heat = NAN; expect(Kn(c, a), "weight", "w_heat NaN");
    c = good(); c.w_bce = INFINITY; expect(Kn(c, a), "weight", "w_bce inf");
    c = good(); c.w_bce = -INFINITY; expect(Kn(c, a), "weight", "w_bce -inf");
    for (int e : {-1, 9, INT32_MAX, INT32_MIN}) {
      c = good(); c.alpha = e; expect(Kn(c, a), "exponents", "alpha");
      c = good(); c.beta = e; expect(Kn(c, a), "exponents", "beta");
    }
    for (float t : {0.f, -0.f, -1.f, 1.0000001f, 2.f, (float)NAN, (float)INFINITY, -(float)INFINITY}) {
      c = good(); c.pos_threshold = t; expect(Kn(c, a), "pos_threshold", "pos_threshold");
    }
    c = good(); c.has_pos_weight = 2; expect(Kn(c, a), "has_pos_weight", "has_pos_weight 2");
    c = good(); c.has_pos_weight = -1; expect(Kn(c, a), "has_pos_weight", "has_pos_weight -1");
    for (float w : {0.f, -1.f, (float)NAN, (float)INFINITY}) {
      c = good(); c.has_pos_weight = 1; c.pos_weight[1] = w; expect(Kn(c, a), "pos_weight[1]", "pos_weight[1]");
    }
  }
  // ---- the shape
  {
    vk_kp_loss_cfg c = good();
    Args a;
    a.C = 0; expect(Kn(c, a), "1..16", "C 0");
    a = Args(); a.C = 17; expect(Kn(c, a), "1..16", "C 17");
    a = Args(); a.C = -3; expect(Kn(c, a), "1..16", "C -3");
    a = Args(); a.N = 0; expect(Kn(c, a), "shape", "N 0");
    a = Args(); a.N = -2; expect(Kn(c, a), "shape", "N -2");
    a = Args(); a.N = INT32_MAX; expect(Kn(c, a), "shape", "N INT_MAX");
    a = Args(); a.N = 32768; expect(Kn(c, a), "shape", "N C = 65536");
    a = Args(); a.HW = 0; expect(Kn(c, a), "shape", "HW 0");
    a = Args(); a.HW = -32; expect(Kn(c, a), "shape", "HW -32");
    a = Args(); a.HW = (1 << 28) + 1; expect(Kn(c, a), "shape", "HW above 2^28");
    a = Args(); a.HW = INT32_MAX; expect(Kn(c, a), "shape", "HW INT_MAX");
    a = Args(); a.N = 4; a.HW = 1 << 28; expect(Kn(c, a), "2^31", "N C HW = 2^31");
    a = Args(); a.N = 30000; a.HW = 1 << 20; expect(Kn(c, a), "2^31", "N C HW far above 2^31");
    if (vk_kp_loss_workspace_bytes(1, 1, 1) != 16 * 8 + 16 || vk_kp_loss_workspace_bytes(2, 2, 4096) != 16 * 8 + 8 * 16 ||
        vk_kp_loss_workspace_bytes(0, 1, 8) != 0 || vk_kp_loss_workspace_bytes(1, 17, 8) != 0 || vk_kp_loss_workspace_bytes(1, 1, 0) != 0 ||
        vk_kp_loss_workspace_bytes(4, 2, 1 << 28) != 0 || vk_kp_loss_workspace_bytes(32768, 2, 8) != 0 ||
        vk_kp_loss_workspace_bytes(INT32_MAX, 16, INT32_MAX) != 0 || vk_kp_loss_workspace_bytes(-1, -1, -1) != 0 ||
        vk_kp_loss_workspace_bytes(7, 1, 1 << 28) == 0) {
      printf("FAIL: vk_kp_loss_workspace_bytes\n");
      ++g_fail;
    }
  }
  // ---- the scalars, the pointers and the workspace
  {
    vk_kp_loss_cfg c = good();
    Args a;
    a.grad_scale = NAN; expect(Kn(c, a), "grad_scale", "grad_scale NaN");
    a = Args(); a.grad_scale = INFINITY; expect(Kn(c, a), "grad_scale", "grad_scale inf");
    a = Args(); a.accumulate = 2; expect(Kn(c, a), "accumulate", "accumulate 2");
    a = Args(); a.accumulate = -1; expect(Kn(c, a), "accumulate", "accumulate -1");
    a = Args();
    expect(K(&c, a, nullptr, y.data(), ws.data(), out.data()), "null argument", "null logits");
    expect(K(&c, a, x.data(), nullptr, ws.data(), out.data()), "null argument", "null target");
    expect(K(&c, a, x.data(), y.data(), nullptr, out.data()), "null argument", "null workspace");
    expect(K(&c, a, x.data(), y.data(), ws.data(), nullptr), "null argument", "null loss_out");
    expect(K(&c, a, x.data(), y.data(), (char*)ws.data() + 4, out.data()), "workspace", "workspace + 4");
    a.ws_bytes = 16 * 8 + 4 * 16 - 1; expect(Kn(c, a), "workspace", "workspace one byte short");
    a.ws_bytes = 0; expect(Kn(c, a), "workspace", "workspace of no bytes");
    a = Args(); a.N = 3; a.ws_bytes = 16 * 8 + 4 * 16; expect(Kn(c, a), "workspace", "workspace for two images of three");
  }
  // ---- what vk_unet_loss_kp runs before its first launch
  {
    vk_kp_loss_cfg c = good();
    ++g_calls;
    if (!vk::kp_check(&c, 2, 2, 32, "vk_unet_loss_kp") || !vk::kp_check_workspace(2, 2, 32, ws.data(), 16 * 8 + 4 * 16, "vk_unet_loss_kp")) {
      printf("FAIL: a good configuration is refused: '%s'\n", g_err);
      ++g_fail;
    }
    c.heat_planes = 5;
    expect(vk::kp_check(&c, 2, 2, 32, "vk_unet_loss_kp") ? VK_OK : VK_ERR_ARG, "vk_unet_loss_kp", "kp_check names its caller");
    expect(vk::kp_check(nullptr, 2, 2, 32, "vk_unet_loss_kp") ? VK_OK : VK_ERR_ARG, "null configuration", "kp_check null");
    expect(vk::kp_check_workspace(2, 2, 32, nullptr, 1 << 20, "vk_unet_loss_kp") ? VK_OK : VK_ERR_ARG, "null argument", "workspace null");
    expect(vk::kp_check_workspace(2, 2, 32, ws.data(), 8, "vk_unet_loss_kp") ? VK_OK : VK_ERR_ARG, "workspace", "workspace of 8 bytes");
  }

  bool touched = false;
  for (auto v : x) touched |= v != 7.f;
  for (auto v : y) touched |= v != 7.f;
  for (auto v : dl) touched |= v != 7.f;
  for (auto v : out) touched |= v != 7.f;
  for (auto v : pos) touched |= v != 7;
  for (auto v : ws) touched |= v != 7.0;
  if (touched) { printf("FAIL: a buffer was written\n"); ++g_fail; }
  printf("%d calls, %d failures\n", g_calls, g_fail);
  return g_fail ? 1 : 0;
}
