// Host layer shared by the convolution files (conv_igemm, conv1x1, conv_halo, conv_bwd_onepass, conv_wgrad, wgrad_halo): the source
// operand as the kernels see it, the one kernel launch, the element-type dispatch and the rules that several launchers must agree on.
// Host-only except for `Src`, which is a member of every kernel parameter block.
#pragma once
#include <stddef.h>

#include "vk_common.h"

namespace vk {

// ---------------------------------------------------------------- a source operand (vk_src) as the kernels see it
struct Src {
  const void* ptr;
  const float* scale;
  const float* shift;
  int C, up, relu;
  uint32_t bytes;      // extent for the buffer descriptor (bounds check); 0 without a source
};
static_assert(sizeof(Src) == 40 && offsetof(Src, bytes) == 36, "Src is laid out inside ConvParams, WgradParams, HaloParams and WhParams");

inline Src no_src() { return Src{nullptr, nullptr, nullptr, 0, 0, 0, 0u}; }
// N x H x W: the layer's input extent (a source with up = 1 is stored at half of it)
inline Src make_src(const vk_src& s, int N, int H, int W, int elem_bytes) {
  return Src{s.ptr, s.scale, s.shift, s.C, s.up, s.relu, s.ptr ? (uint32_t)((size_t)N * (H >> s.up) * (W >> s.up) * s.C * elem_bytes) : 0u};
}
// a materialised [N][H][W][C] tensor read as it is (the stem's 4-channel input)
inline Src plain_src(const void* ptr, int C, int N, int H, int W, int elem_bytes) {
  return Src{ptr, nullptr, nullptr, C, 0, 0, (uint32_t)((size_t)N * H * W * C * elem_bytes)};
}
// the second (concat) source of a descriptor: every field zero when there is none
inline Src make_src1(const vk_conv_desc* d, int elem_bytes) { return d->src1.ptr ? make_src(d->src1, d->N, d->H, d->W, elem_bytes) : no_src(); }

// ---------------------------------------------------------------- element-type dispatch
// f(T()) with T = float / bf16_t / f16_t.  An unknown dtype returns VK_ERR_ARG, with the "bad dtype" message when `report` is set.
template <typename F>
int dispatch_dtype(vk_dtype dt, F&& f, bool report = false) {
  switch (dt) {
    case VK_F32: return f(float());
    case VK_BF16: return f(bf16_t());
    case VK_F16: return f(f16_t());
  }
  if (report) vkh::set_error("bad dtype %d", (int)dt);
  return VK_ERR_ARG;
}

// ---------------------------------------------------------------- strip height of the streaming 3x3 kernels
// Output rows per strip of conv3x3_stream_kernel: as tall as leaves >= 4096 strips (two rounds of the 2048 resident waves), 32 .. 256.
// INVARIANT: the one-pass backward kernels add their BatchNorm-backward fp32 partial sums over exactly these rows
// (RSsum), so that the sums — and through them conv1's coefficients — are the ones the streaming data gradient adds up; a build with
// other strips moved the step's gradients by 0.4 %.  launch_stream and both one-pass launchers call this; VK_STREAM_RS is handled by
// each caller (a forced strip height also forces RSsum).
constexpr int kStreamStripMin = 32;
inline int stream_strip_rows(int N, int H, int W) {
  const long per_row_block = (long)N * ((W + 15) / 16);
  int rows = kStreamStripMin;
  while (rows * 2 <= 256 && per_row_block * ((H + 2 * rows - 1) / (2 * rows)) >= 4096) rows *= 2;
  return rows;
}

// ---------------------------------------------------------------- which 3x3 tile kernel a descriptor belongs to (conv_halo.hip)
// Every condition that depends on the descriptor alone (shape, channel multiples, 2^31 / 2^32 extents, VK_NO_S2_TILE).  conv3x3_halo_try
// adds what depends on the call; vk_conv_uses_halo_pack adds VK_NO_HALO.  All classes but C16 take halo-pack weights (vk_halo_pack).
enum class HaloClass { NONE, C16, S1, S2, S2D };
HaloClass halo_class(const vk_conv_desc* d);

}  // namespace vk

namespace vkh {

template <auto Kernel>
int lds_attr_once(size_t lds_bytes) {      // Kernel is a template argument: one flag per kernel
  static bool attr_done = false;
  if (!attr_done) {
    VK_CHECK_HIP(hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    attr_done = true;
  }
  return VK_OK;
}

template <auto Kernel, typename... Args>
int launch(dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st, const char* tag, const ProfDetail& detail, double flops, double bytes,
           const Args&... args) {
  if (lds_bytes > 64 * 1024) {
    const int rc = lds_attr_once<Kernel>(lds_bytes);
    if (rc != VK_OK) return rc;
  }
  {
    char buf[160];
    ProfScope ps(prof_tag(buf, sizeof(buf), tag, detail), st, flops, bytes);
    hipLaunchKernelGGL(Kernel, grid, block, lds_bytes, st, args...);
  }
  VK_CHECK_HIP(hipGetLastError());
  return VK_OK;
}

}  // namespace vkh
