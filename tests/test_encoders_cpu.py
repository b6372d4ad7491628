"""vk.encoders (resnet18 / resnet34 / resnet50 encoders), the parts that need no GPU: the state-dict contract against the CPU restatement
of smp.Unet (tests/encoders_ref.py), default initialisation under a seed, save / load round trips, the engine's tensor table and
gradient buckets on host-only handles, and the refusals."""
import ctypes as C
import io

import pytest
import torch

import encoders_ref as R

ENCODERS = ("resnet18", "resnet34", "resnet50")
CODES = {"resnet18": 18, "resnet34": 34, "resnet50": 50}


def _handle(vk, encoder, classes=1, training=1, size=64, width=0):
    L = vk.lib()
    cfg = vk._lib.vk_unet_config(2, size, vk._lib.VK_BF16, training, width)
    h = C.c_void_p()
    vk._lib.check(L.vk_unet_create_enc(C.byref(cfg), classes, CODES[encoder], C.byref(h)), "vk_unet_create_enc")
    return L, h


def _table(vk, L, h):
    out = []
    for i in range(L.vk_unet_num_tensors(h)):
        ti = vk._lib.vk_tensor_info()
        vk._lib.check(L.vk_unet_tensor_info(h, i, C.byref(ti)))
        out.append((ti.name.decode(), ti.kind, [ti.dims[j] for j in range(ti.ndim)], ti.offset, ti.numel))
    return out


def _buckets(vk, L, h):
    out = []
    for b in range(L.vk_unet_num_buckets(h)):
        b0, b1 = C.c_int64(), C.c_int64()
        vk._lib.check(L.vk_unet_bucket_range(h, b, C.byref(b0), C.byref(b1)))
        out.append((b0.value, b1.value))
    return out


@pytest.mark.parametrize("encoder", ENCODERS)
def test_state_dict_keys_shapes_counts(vk, encoder):
    model = vk.encoders.Unet(encoder_name=encoder, encoder_weights=None)
    ref = R.build(encoder)
    sd, rsd = model.state_dict(), ref.state_dict()
    assert list(sd.keys()) == list(rsd.keys())
    assert [tuple(v.shape) for v in sd.values()] == [tuple(v.shape) for v in rsd.values()]
    n_params = sum(p.numel() for p in model.parameters())
    assert (n_params, len(sd)) == R.EXPECTED[encoder]
    assert sum(p.numel() for p in ref.parameters()) == n_params
    assert model.encoder_name == encoder


@pytest.mark.parametrize("encoder", ENCODERS)
@pytest.mark.parametrize("classes", [1, 4])
def test_default_init_matches_restatement(vk, oracle, encoder, classes):
    oracle.set_seed(7)
    model = vk.encoders.Unet(encoder_name=encoder, encoder_weights=None, classes=classes)
    ref = R.build(encoder, classes, seed=7)
    sd, rsd = model.state_dict(), ref.state_dict()
    for k, v in rsd.items():
        assert torch.equal(sd[k], v), k


@pytest.mark.parametrize("encoder", ENCODERS)
def test_save_load_round_trip(vk, encoder):
    ref = R.build(encoder, seed=3)
    model = vk.encoders.Unet(encoder_name=encoder, encoder_weights=None)
    model.load_state_dict(ref.state_dict(), strict=True)
    buf = io.BytesIO()
    torch.save(model.state_dict(), buf)
    buf.seek(0)
    ref2 = R.EncoderUnet(encoder)
    ref2.load_state_dict(torch.load(buf), strict=True)
    for k, v in ref.state_dict().items():
        assert torch.equal(ref2.state_dict()[k], v), k
    model2 = vk.encoders.Unet(encoder_name=encoder, encoder_weights=None)
    model2.load_state_dict(ref2.state_dict(), strict=True)
    for k, v in model2.state_dict().items():
        assert torch.equal(v, ref.state_dict()[k]), k


@pytest.mark.parametrize("encoder", ENCODERS)
@pytest.mark.parametrize("size,width", [(64, 0), (64, 96)])
def test_buckets_whole_tensor_contiguous(vk, encoder, size, width):
    L, h = _handle(vk, encoder, size=size, width=width)
    try:
        assert L.vk_unet_encoder(h) == CODES[encoder]
        table = _table(vk, L, h)
        buckets = _buckets(vk, L, h)
        P = L.vk_unet_param_numel(h)
        assert len(buckets) == {"resnet18": 8, "resnet34": 10, "resnet50": 10}[encoder]
        # backward completion order: each bucket ends where the previous one begins; together they cover [0, P)
        assert buckets[0][1] == P and buckets[-1][0] == 0
        for (a0, _), (_, b1) in zip(buckets, buckets[1:]):
            assert b1 == a0
        assert all(b0 < b1 for b0, b1 in buckets)
        # whole tensors: no parameter tensor straddles a bucket boundary
        cuts = {b0 for b0, _ in buckets}
        for name, kind, dims, off, numel in table:
            if kind in (0, 1):
                assert not any(off < c < off + numel for c in cuts), name
        # encoder buckets end at the head of a stage's first block
        names_at = {off: name for name, kind, dims, off, numel in table if kind in (0, 1)}
        for b0, _ in buckets[3:-1]:
            assert names_at[b0].startswith("encoder.layer") and names_at[b0].endswith(".conv1.weight"), names_at[b0]
        n_bn = sum(1 for t in table if t[1] == 3)
        assert n_bn == {"resnet18": 30, "resnet34": 46, "resnet50": 63}[encoder]
    finally:
        L.vk_unet_destroy(h)


@pytest.mark.parametrize("classes", [1, 3])
@pytest.mark.parametrize("training", [0, 1])
def test_resnet34_plan_identical(vk, classes, training):
    """vk.encoders' resnet34 is vk.Unet's plan: the same tensor table, buckets and buffer / workspace sizes."""
    L = vk.lib()
    for size, width in [(64, 0), (96, 64)]:
        cfg = vk._lib.vk_unet_config(2, size, vk._lib.VK_BF16, training, width)
        ha, hb = C.c_void_p(), C.c_void_p()
        vk._lib.check(L.vk_unet_create_ex(C.byref(cfg), classes, C.byref(ha)))
        vk._lib.check(L.vk_unet_create_enc(C.byref(cfg), classes, 34, C.byref(hb)))
        try:
            assert _table(vk, L, ha) == _table(vk, L, hb)
            assert _buckets(vk, L, ha) == _buckets(vk, L, hb)
            for fn in ("vk_unet_param_numel", "vk_unet_buffer_numel", "vk_unet_workspace_bytes"):
                assert getattr(L, fn)(ha) == getattr(L, fn)(hb), fn
            assert L.vk_unet_encoder(ha) == 34
        finally:
            L.vk_unet_destroy(ha)
            L.vk_unet_destroy(hb)
    a = vk.Unet(encoder_weights=None) if classes == 1 else vk.multiclass.Unet(encoder_weights=None, classes=classes)
    b = vk.encoders.Unet(encoder_name="resnet34", encoder_weights=None, classes=classes)
    assert a._table == b._table


@pytest.mark.parametrize("encoder", ["resnet18", "resnet50"])
def test_bn_and_trainable_flag_counts(vk, encoder):
    L, h = _handle(vk, encoder)
    try:
        table = _table(vk, L, h)
        n_p = sum(1 for t in table if t[1] in (0, 1))
        n_bn = sum(1 for t in table if t[1] == 3)
        ok = (C.c_uint8 * n_p)(*([1] * n_p))
        assert L.vk_unet_set_trainable(h, ok, n_p) == 0
        assert L.vk_unet_set_trainable(h, ok, n_p - 1) != 0
        fl = (C.c_uint8 * n_bn)(*([0] * n_bn))
        assert L.vk_unet_set_bn_frozen(h, fl, n_bn) == 0
        assert L.vk_unet_set_bn_frozen(h, fl, 46 if n_bn != 46 else 45) != 0
    finally:
        L.vk_unet_destroy(h)


def test_refusals(vk):
    for name in ("efficientnet-b0", "resnet101", "resnet152"):
        with pytest.raises(NotImplementedError):
            vk.encoders.Unet(encoder_name=name, encoder_weights=None)
    with pytest.raises(vk.VkError):
        vk.encoders.Unet(encoder_name="resnet18", encoder_weights="imagenet")
    with pytest.raises(vk.VkError):
        vk.encoders.build_model("resnet18", weights="imagenet")
    # the reference's drop-ins keep refusing the other encoders
    for cls in (vk.Unet, vk.multiclass.Unet):
        for name in ("resnet18", "resnet50"):
            with pytest.raises(NotImplementedError):
                cls(encoder_name=name, encoder_weights=None)
    with pytest.raises(NotImplementedError):
        vk.build_model("resnet50", weights=None)
    L = vk.lib()
    cfg = vk._lib.vk_unet_config(2, 64, vk._lib.VK_BF16, 1, 0)
    h = C.c_void_p()
    assert L.vk_unet_create_enc(C.byref(cfg), 1, 101, C.byref(h)) == -1
    assert L.vk_unet_create_enc(C.byref(cfg), 17, 18, C.byref(h)) != 0


def test_resnet50_engine_table_matches_restatement(vk):
    """The engine's own resnet50 tensor table (not the Python tree built from it): smp's names, shapes and order, with offsets that
    tile the flat buffers."""
    L, h = _handle(vk, "resnet50")
    try:
        table = _table(vk, L, h)
        ref = R.build("resnet50")
        assert [(t[0], tuple(t[2])) for t in table] == [(k, tuple(v.shape)) for k, v in ref.state_dict().items()]
        assert sum(t[4] for t in table if t[1] in (0, 1)) == R.EXPECTED["resnet50"][0]
        assert len(table) == R.EXPECTED["resnet50"][1]
        P = L.vk_unet_param_numel(h)
        spans = sorted((t[3], t[3] + t[4]) for t in table if t[1] in (0, 1))
        assert all(a1 <= b0 for (_, a1), (b0, _) in zip(spans, spans[1:])) and spans[-1][1] <= P
        assert "decoder.blocks.0.conv1.0.weight" in {t[0] for t in table}
        d0 = [t for t in table if t[0] == "decoder.blocks.0.conv1.0.weight"][0]
        assert d0[2] == [256, 3072, 3, 3]
    finally:
        L.vk_unet_destroy(h)


@pytest.mark.parametrize("encoder", ENCODERS)
def test_build_model(vk, encoder):
    m = vk.encoders.build_model(encoder)
    assert isinstance(m, vk.encoders.Unet) and isinstance(m, vk.multiclass.Unet)
    assert m.classes == 1 and m.encoder_name == encoder
    assert sum(p.numel() for p in m.parameters()) == R.EXPECTED[encoder][0]


def test_conv1x1_refuses_other_descriptors(vk):
    """Host-side checks of the pointwise entry points: anything but R = S = 1, pad 0, stride 1 / 2 is VK_ERR_UNSUPPORTED (-3), before
    any device work."""
    L = vk.lib()
    src = vk._lib.vk_src(1 << 20, 64, 0, None, None, 0)
    null = vk._lib.vk_src(None, 0, 0, None, None, 0)
    base = dict(dtype=vk._lib.VK_BF16, N=1, H=8, W=8, Ho=8, Wo=8, K=64, R=1, S=1, stride=1, pad=0, transposed=0)
    for bad in (dict(R=3, S=3, pad=1), dict(pad=1), dict(stride=3), dict(S=3)):
        d = vk._lib.vk_conv_desc(**{**base, **bad}, src0=src, src1=null)
        assert L.vk_conv1x1_fwd(C.byref(d), 1 << 20, 1 << 20, 0, None, None) == -3
        assert L.vk_conv1x1_wgrad(C.byref(d), 1 << 20, 1 << 20, None, 0, None) == -3
    up = vk._lib.vk_src(1 << 20, 64, 1, None, None, 0)
    d = vk._lib.vk_conv_desc(**base, src0=up, src1=null)
    assert L.vk_conv1x1_fwd(C.byref(d), 1 << 20, 1 << 20, 0, None, None) == -3
    d = vk._lib.vk_conv_desc(**base, src0=src, src1=src)
    assert L.vk_conv1x1_fwd(C.byref(d), 1 << 20, 1 << 20, 0, None, None) == -3
    # argument errors: channels not a multiple of the vector width, output grid not matching the stride
    d = vk._lib.vk_conv_desc(**{**base, "K": 12}, src0=src, src1=null)
    assert L.vk_conv1x1_fwd(C.byref(d), 1 << 20, 1 << 20, 0, None, None) == -1
    d = vk._lib.vk_conv_desc(**{**base, "stride": 2}, src0=src, src1=null)
    assert L.vk_conv1x1_fwd(C.byref(d), 1 << 20, 1 << 20, 0, None, None) == -1
