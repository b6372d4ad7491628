"""Frozen BatchNorm statistics and the input gradient, the parts that need no GPU: the two new engine entry points on a host-only handle,
the 46 per-layer flags the nn.Module derives from its holders' modes, and the new symbols in header, exports and ctypes table."""
import ctypes as C
import re
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
NEW = ("vk_unet_set_bn_frozen", "vk_unet_set_input_grad", "vk_stem_dgrad", "vk_bn_bwd_coeffs_frozen")


def _handle(vk, training=1):
    L = vk.lib()
    cfg = vk._lib.vk_unet_config(2, 64, vk._lib.VK_BF16, training)
    h = C.c_void_p()
    vk._lib.check(L.vk_unet_create(C.byref(cfg), C.byref(h)))
    return L, h


def test_set_bn_frozen_takes_one_flag_per_batchnorm_layer(vk):
    L, h = _handle(vk)
    try:
        for flags in ([1] * 46, [0] * 46, [i % 2 for i in range(46)]):
            assert L.vk_unet_set_bn_frozen(h, (C.c_uint8 * 46)(*flags), 46) == 0
        for bad in (45, 47, 0, 140):
            assert L.vk_unet_set_bn_frozen(h, (C.c_uint8 * max(bad, 1))(), bad) == -1          # VK_ERR_ARG
            assert b"BatchNorm layers" in L.vk_last_error_string()
        assert L.vk_unet_set_bn_frozen(h, None, 46) == -1
        assert L.vk_unet_set_bn_frozen(None, (C.c_uint8 * 46)(), 46) == -1
    finally:
        L.vk_unet_destroy(h)


def test_set_input_grad_arguments(vk):
    L, h = _handle(vk)
    try:
        buf = (C.c_float * 4)()
        assert L.vk_unet_set_input_grad(h, C.cast(buf, C.c_void_p)) == 0
        assert L.vk_unet_set_input_grad(h, None) == 0
        assert L.vk_unet_set_input_grad(None, None) == -1
    finally:
        L.vk_unet_destroy(h)
    L, h = _handle(vk, training=0)            # an inference plan has no backward to write it
    try:
        assert L.vk_unet_set_input_grad(h, C.cast((C.c_float * 4)(), C.c_void_p)) == -1
        assert L.vk_unet_set_input_grad(h, None) == 0
    finally:
        L.vk_unet_destroy(h)


def test_stem_dgrad_argument_checks(vk):
    L = vk.lib()
    p = C.c_void_p(256)                        # never dereferenced: every call below is refused on the host
    assert L.vk_stem_dgrad(vk._lib.VK_BF16, 1, 64, 64, None, None, None, p, p, None) == -1
    assert L.vk_stem_dgrad(vk._lib.VK_BF16, 1, 64, 64, p, None, p, p, p, None) == -1       # coefficients without z
    assert L.vk_stem_dgrad(vk._lib.VK_BF16, 1, 64, 48, p, None, None, p, p, None) == -1    # W % 32
    assert L.vk_stem_dgrad(vk._lib.VK_BF16, 1, 36, 64, p, None, None, p, p, None) == -1    # H % 8
    assert L.vk_stem_dgrad(vk._lib.VK_BF16, 0, 64, 64, p, None, None, p, p, None) == -1
    assert L.vk_bn_bwd_coeffs_frozen(64, None, p, p, p, p, p, p, None) == -1


def _bn_prefixes(m):
    return [n[:-len(".num_batches_tracked")] for n, _ in m.named_buffers() if n.endswith("num_batches_tracked")]


def test_bn_flags_follow_module_modes(vk):
    m = vk.Unet(encoder_name="resnet34", encoder_weights=None, in_channels=3, classes=1, activation=None)
    names = _bn_prefixes(m)
    assert len(names) == 46
    # the engine's BatchNorm order is the order of the num_batches_tracked entries of its tensor table
    table = [t[0][:-len(".num_batches_tracked")] for t in m._table if t[1] == 3]
    assert names == table
    assert m._bn_frozen_flags() == (False,) * 46
    m.eval()
    assert m._bn_frozen_flags() == (True,) * 46
    m.train()
    m.encoder.eval()
    assert m._bn_frozen_flags() == tuple(n.startswith("encoder.") for n in names)
    m.train()
    m.get_submodule("decoder.blocks.3.conv1.1").eval()
    assert m._bn_frozen_flags() == tuple(n == "decoder.blocks.3.conv1.1" for n in names)
    m.train()
    m.get_submodule("encoder.layer2.0.downsample").eval()     # a parent holder flips its children, as nn.Module.eval() does
    assert m._bn_frozen_flags() == tuple(n == "encoder.layer2.0.downsample.1" for n in names)
    m.eval()
    m.training = True                                         # the root's own flag does not decide a layer's mode
    assert m._bn_frozen_flags() == (True,) * 46


def test_new_symbols_in_header_exports_and_table(vk):
    hdr = (ROOT / "include" / "vk_unet.h").read_text()
    L = vk.lib()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in vk._lib.SIGNATURES, name
        assert hasattr(L, name), name
