"""Argument checks of the per-channel BatchNorm entry points that return before any device call, so they need no GPU: channel counts
outside the documented set (a multiple of 8 up to 512, or 1024 / 2048) are refused by all four flat kernels, and vk_bn_finalize takes
its two running statistics together or not at all."""
import ctypes as C

import pytest

REFUSED_C = [0, -8, 12, 20, 520, 1536, 4096]


@pytest.mark.parametrize("Cc", REFUSED_C)
def test_flat_bn_kernels_refuse_undocumented_channel_counts(vk, Cc):
    L = vk.lib()
    p = C.c_void_p(256)                        # never dereferenced: every call below is refused on the host, and pixels = 0
    want = -1 if Cc <= 0 or Cc % 8 else -3     # VK_ERR_ARG for a malformed count, VK_ERR_UNSUPPORTED for one the kernels cannot do
    for dt in (vk._lib.VK_F32, vk._lib.VK_BF16, vk._lib.VK_F16):
        assert L.vk_bn_add_relu(dt, 0, Cc, p, p, p, p, p, p, p, None) == want
        assert L.vk_bn_bwd_reduce(dt, 0, Cc, p, p, 1, p, p, None, p, None) == want
        assert L.vk_bn_bwd_apply(dt, 0, Cc, p, p, 1, p, p, None, p, p, p, 0, None) == want
        assert L.vk_bn_bwd_apply_fused(dt, 0, Cc, p, p, 1, p, p, None, p, 1.0, p, p, p, p, p, p, p, 0, None) == want
        if Cc > 512:
            assert (b"C=%d unsupported" % Cc) in L.vk_last_error_string()


def test_bn_finalize_running_statistics_come_in_pairs(vk):
    L = vk.lib()
    p = C.c_void_p(256)
    assert L.vk_bn_finalize(64, 1, p, 10.0, p, p, p, None, 1e-5, 0.1, p, p, p, p, None) == -1
    assert L.vk_bn_finalize(64, 1, p, 10.0, p, p, None, p, 1e-5, 0.1, p, p, p, p, None) == -1
    assert L.vk_bn_finalize(64, 0, None, 0.0, p, p, p, None, 1e-5, 0.1, p, p, None, None, None) == -1
    assert L.vk_bn_finalize(0, 1, p, 10.0, p, p, None, None, 1e-5, 0.1, p, p, p, p, None) == -1
