"""vk.inputs without a GPU: the exactness conditions of the stem sweep for 1, 2 and 4 input channels proved on the reference alone, the
mix restatement and its bounds, adapt_first_conv against hand values, the initial weights against the restatement of smp
(tests/inputs_ref.py), parameter counts / key order / shapes, the classes that must go on refusing in_channels != 3, and every argument
error of the new entry points, which the library finds before it touches a stream."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_lattice as CL
import encoders_ref as ER
import inputs_cases as IC
import inputs_ref as IR
from averaging_ref import fma32_exact


# ------------------------------------------------------------------------------------------------ 1. the lattice conditions
@pytest.mark.parametrize("shape", IC.STEM_MAPS, ids=lambda s: "n%d_%dx%d" % s)
@pytest.mark.parametrize("cin", IC.CINS)
def test_stem_fwd_and_wgrad_lattice_conditions(cin, shape):
    N, H, W = shape
    x, w, _ = IC.stem_operands(N, H, W, cin, 700 + H)
    assert x.shape[1] == cin and float(x.abs().max()) <= 2 and set(w.unique().tolist()) <= {-1.0, 0.0, 1.0}
    y = F.conv2d(x, w, stride=2, padding=3)
    ymax = float(y.abs().max())
    assert ymax <= 2 * 49 * cin                                          # 49 cin ternary taps of |x| <= 2
    for dtn in IC.DTYPES:
        assert CL.exact_in(y, dtn)
    assert CL.TILE_PIX * 2 * ymax ** 2 < CL.TWO24                        # the fp32 statistics partial of one tile is exact
    x, _, dz = IC.stem_operands(N, H, W, cin, 720 + H)
    z, a, bb, cc, dz_bn = IC.bn_fold(dz, 730 + H)
    for dzv in (dz, dz_bn):
        for dtn in IC.DTYPES:
            assert CL.exact_in(dzv, dtn)
        wa = torch.zeros(64, cin, 7, 7, dtype=torch.float64, requires_grad=True)
        F.conv2d(x.abs(), wa, stride=2, padding=3).backward(dzv.abs())
        assert float(wa.grad.max()) + IC.DW0 < CL.TWO24                  # every partial sum of the weight gradient is an exact fp32
        print("cin %d %s: max |y| = %d, absolute weight-gradient sum <= %d" % (cin, shape, int(ymax), int(wa.grad.max())))


@pytest.mark.parametrize("shape", IC.DGRAD_MAPS, ids=lambda s: "n%d_%dx%d" % s)
@pytest.mark.parametrize("cin", IC.CINS)
def test_stem_dgrad_lattice_conditions(cin, shape):
    N, H, W = shape
    assert H % 8 == 0 and W % 32 == 0
    x, w, dz = IC.stem_operands(N, H, W, cin, 740 + H)
    z, a, bb, cc, dz_bn = IC.bn_fold(dz, 750 + H)
    for dzv in (dz, dz_bn):
        for dtn in IC.DTYPES:
            assert CL.exact_in(dzv, dtn)
        xin = torch.zeros(N, cin, H, W, dtype=torch.float64, requires_grad=True)
        F.conv2d(xin, w.abs(), stride=2, padding=3).backward(dzv.abs())
        assert float(xin.grad.max()) < CL.TWO24
        print("cin %d %s: absolute data-gradient sum <= %d" % (cin, shape, int(xin.grad.max())))


# ------------------------------------------------------------------------------------------------ 2. the mix
def test_mix_ref_is_the_fma_chain():
    rng = np.random.default_rng(5)
    x3 = rng.standard_normal((2, 3, 7)).astype(np.float32)
    M = rng.standard_normal((4, 3)).astype(np.float32)
    b = rng.standard_normal(4).astype(np.float32)
    out = IC.mix_ref(x3, M, b)
    assert out.shape == (2, 4, 7) and out.dtype == np.float32
    for n in range(2):
        for o in range(4):
            for p in range(7):
                acc = b[o]
                for j in range(3):
                    acc = fma32_exact(x3[n, j, p], M[o, j], acc)
                assert out[n, o, p].tobytes() == np.float32(acc).tobytes(), (n, o, p)
    # cout = 1 uses row 0 only; b = 0 and the identity rows give the planes back
    eye = IC.mix_ref(x3, np.eye(3, dtype=np.float32), np.zeros(3, np.float32))
    assert eye.tobytes() == x3.tobytes()


def test_luma_row_and_closed_form(vk):
    M, b = vk.inputs.luma_matrix()
    assert b == [0.0] and len(M) == 1 and M[0] == IC.luma_row()
    assert (vk.inputs.IMAGENET_MEAN, vk.inputs.IMAGENET_STD, vk.inputs.LUMA_WEIGHTS) == (IC.IMAGENET_MEAN, IC.IMAGENET_STD, IC.LUMA_WEIGHTS)
    row32 = np.asarray(M[0], dtype=np.float32)
    assert abs(float(row32.astype(np.float64).sum()) - 1.0) <= 2.0 ** -23          # one ulp of 1
    v = np.arange(256)
    want, t, S = IC.luma_closed_form(v)
    x3 = np.stack([np.asarray(tj, dtype=np.float32) for tj in t])[None]            # the replicated, normalised gray image [1][3][256]
    got = IC.mix_ref(x3, row32[None], np.zeros(1, np.float32))[0, 0].astype(np.float64)
    err = np.abs(got - want)
    print("luma: max |err| / bound = %.3f" % float((err / IC.luma_bound(S)).max()))
    assert (err <= IC.luma_bound(S)).all()
    ad = vk.inputs.ChannelAdapter(torch.nn.Identity(), mode="luma")
    assert ad.cout == 1 and ad.matrix.numpy().tobytes() == row32.tobytes() and float(ad.bias[0]) == 0.0


def test_channel_adapter_refuses_wrong_arguments(vk):
    A = vk.inputs.ChannelAdapter
    ident = torch.nn.Identity()
    for kw in (dict(), dict(mode="luma", matrix=[[1, 0, 0]]), dict(mode="chroma"), dict(mode="luma", bias=[0.0]), dict(matrix=[[1, 0]]),
               dict(matrix=[[1, 0, 0]] * 5), dict(matrix=[[1, 0, 0]], bias=[0.0, 1.0]), dict(matrix=[[float("nan"), 0, 0]])):
        with pytest.raises(ValueError):
            A(ident, **kw)
    m = vk.inputs.Unet(encoder_name="resnet18", encoder_weights=None, in_channels=2)
    with pytest.raises(ValueError, match="in_channels=2"):
        A(m, mode="luma")
    ad = A(m, matrix=[[1, 0, 0], [0, 0.5, 0.5]])
    with pytest.raises(ValueError):
        ad.mix(torch.zeros(1, 2, 32, 32))
    with pytest.raises(vk.VkError):
        ad.mix(torch.zeros(1, 3, 32, 32))            # a CPU tensor: no fallback


# ------------------------------------------------------------------------------------------------ 3. adapt_first_conv
def test_adapt_first_conv_hand_values(vk):
    w = torch.tensor([[[[1.0, 2.0]], [[10.0, 20.0]], [[100.0, 200.0]]],
                      [[[-1.0, 0.5]], [[0.25, 4.0]], [[8.0, -16.0]]]])            # [2][3][1][2]
    a = vk.inputs.adapt_first_conv
    assert a(w, 1).tolist() == [[[[111.0, 222.0]]], [[[7.25, -11.5]]]]
    assert torch.equal(a(w, 3), w) and a(w, 3) is not w
    w2 = a(w, 2)
    assert w2.shape == (2, 2, 1, 2) and torch.equal(w2, w[:, :2] * 1.5)
    w4 = a(w, 4)
    assert w4.shape == (2, 4, 1, 2) and torch.equal(w4, torch.cat([w, w[:, :1]], 1) * 0.75)
    assert w4[1, 3].tolist() == [[-0.75, 0.375]]
    for c in (1, 2, 4):
        assert torch.equal(a(w, c), IR.adapt_first_conv(w, c))
    sd = {"encoder.conv1.weight": w, "other": torch.ones(2)}
    out = a(sd, 1)
    assert out is not sd and out["other"] is sd["other"] and torch.equal(out["encoder.conv1.weight"], a(w, 1)) and sd["encoder.conv1.weight"] is w
    with pytest.raises(ValueError):
        a(torch.zeros(2, 4, 1, 1), 1)
    with pytest.raises(ValueError):
        a(w, 0)
    with pytest.raises(KeyError):
        a({"x": w}, 1)


# ------------------------------------------------------------------------------------------------ 4.-6. the model's tensors
@pytest.mark.parametrize("encoder,cin", [("resnet34", 1), ("resnet18", 4), ("resnet34", 2)])
def test_initial_weights_equal_the_restatement(vk, oracle, encoder, cin):
    ref = IR.build(encoder, cin, seed=11)
    oracle.set_seed(11)
    m = vk.inputs.Unet(encoder_name=encoder, encoder_weights=None, in_channels=cin, classes=1, activation=None)
    sd, rd = m.state_dict(), ref.state_dict()
    assert list(sd.keys()) == list(rd.keys())
    for k in rd:
        assert sd[k].shape == rd[k].shape and torch.equal(sd[k], rd[k]), k
    assert sd["encoder.conv1.weight"].shape == (64, cin, 7, 7)
    bound = 1 / math.sqrt(49 * cin)                      # kaiming_uniform_(a = sqrt(5)): U(-1 / sqrt(fan_in), 1 / sqrt(fan_in))
    assert float(sd["encoder.conv1.weight"].abs().max()) <= bound


def test_three_channels_is_the_encoders_model(vk, oracle):
    oracle.set_seed(7)
    a = vk.encoders.Unet(encoder_name="resnet18", encoder_weights=None, classes=2)
    oracle.set_seed(7)
    b = vk.inputs.Unet(encoder_name="resnet18", encoder_weights=None, in_channels=3, classes=2)
    after_a = torch.rand(1)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa.keys()) == list(sb.keys()) and all(torch.equal(sa[k], sb[k]) for k in sa)
    oracle.set_seed(7)
    vk.inputs.Unet(encoder_name="resnet18", encoder_weights=None, in_channels=3, classes=2)
    assert torch.equal(torch.rand(1), after_a)           # and nothing more was drawn
    assert isinstance(b, vk.encoders.Unet) and b.in_channels == 3 and a.in_channels == 3


@pytest.mark.parametrize("cin", [1, 2, 3, 4])
def test_parameter_counts_keys_and_shapes(vk, cin):
    m = vk.inputs.Unet(encoder_name="resnet34", encoder_weights=None, in_channels=cin)
    assert sum(p.numel() for p in m.parameters()) == 24_436_369 - 64 * 49 * (3 - cin)
    ref3 = ER.build("resnet34").state_dict()
    sd = m.state_dict()
    assert list(sd.keys()) == list(ref3.keys()) and len(sd) == 278
    for k, v in ref3.items():
        want = (64, cin, 7, 7) if k == "encoder.conv1.weight" else tuple(v.shape)
        assert tuple(sd[k].shape) == want, k
    assert sd["encoder.conv1.weight"].permute(0, 2, 3, 1).is_contiguous()          # KRSC in memory
    h = C.c_void_p()
    cfg = vk._lib.vk_unet_config(1, 32, vk._lib.VK_F32, 0)
    vk._lib.check(vk.lib().vk_unet_create_in(C.byref(cfg), 1, vk._lib.VK_ENC_RESNET34, cin, C.byref(h)))
    try:
        assert vk.lib().vk_unet_in_channels(h) == cin and vk.lib().vk_unet_encoder(h) == 34
    finally:
        vk.lib().vk_unet_destroy(h)


def test_load_pretrained_on_the_host(vk, oracle):
    oracle.set_seed(3)
    colour = vk.Unet(encoder_name="resnet34", encoder_weights=None, in_channels=3, classes=1, activation=None)
    ck = {k: v.clone() for k, v in colour.state_dict().items()}
    for cin in (1, 4):
        m = vk.inputs.Unet(encoder_name="resnet34", encoder_weights=None, in_channels=cin)
        res = vk.inputs.load_pretrained(m, ck)
        assert not res.missing_keys and not res.unexpected_keys
        sd = m.state_dict()
        for k in ck:
            want = IR.adapt_first_conv(ck[k], cin) if k == "encoder.conv1.weight" else ck[k]
            assert torch.equal(sd[k], want), k
    with pytest.raises(RuntimeError):
        m.load_state_dict(ck)                            # the plain route refuses the 3-channel conv1


@pytest.mark.parametrize("seed,scale", [(1, 1.0), (2, 30.0), (3, 1e-3)])
def test_gray_stem_bound_holds_for_fp32_stems(vk, seed, scale):
    """The bar tests/test_vk_inputs_gpu.py holds load_pretrained to, proved on fp32 convolutions of the host: each side against its own
    term of the derivation (float64 on the exactly summed weights is the exact value E), and the two terms under the 200 u A bound."""
    g = torch.Generator().manual_seed(seed)
    gray = torch.randn(2, 1, 40, 72, generator=g) * scale
    w3 = torch.randn(64, 3, 7, 7, generator=g) * 0.1
    w3[:, 1] = -w3[:, 0] + 1e-3 * torch.randn(64, 7, 7, generator=g)     # cancelling channels: the summed weight is far below sum |w_j|
    w1 = vk.inputs.adapt_first_conv(w3, 1)
    assert w1.dtype == torch.float32 and w1.shape == (64, 1, 7, 7)
    exact = F.conv2d(gray.double(), w3.double().sum(1, keepdim=True), stride=2, padding=3)
    colour = F.conv2d(gray.expand(-1, 3, -1, -1).contiguous(), w3, stride=2, padding=3).double()
    gray_out = F.conv2d(gray, w1, stride=2, padding=3).double()
    A = IC.gray_stem_A(gray, w3)
    e_c, e_g = (colour - exact).abs(), (gray_out - exact).abs()
    print("colour / its term %.3f, gray / its term %.3f, difference / bound %.3f" % (
        float((e_c / IC.colour_term(A)).max()), float((e_g / IC.gray_term(A)).max()),
        float(((colour - gray_out).abs() / IC.gray_stem_bound(gray, w3)).max())))
    assert bool((e_c <= IC.colour_term(A)).all()) and bool((e_g <= IC.gray_term(A)).all())
    assert bool((IC.colour_term(A) + IC.gray_term(A) <= IC.gray_stem_bound(gray, w3)).all())
    assert bool(((colour - gray_out).abs() <= IC.gray_stem_bound(gray, w3)).all())
    assert IC.gamma(147) + IC.gamma(2) + IC.gamma(49) * (1 + IC.gamma(2)) < 200 * IC.U32


# ------------------------------------------------------------------------------------------------ 7. what stays refused
def test_the_reference_classes_still_refuse(vk):
    for cls in (vk.Unet, vk.multiclass.Unet, vk.encoders.Unet):
        assert cls.in_channels_allowed == (3,)
        for cin in (1, 2, 4):
            with pytest.raises(NotImplementedError):
                cls(encoder_weights=None, in_channels=cin)
    assert vk.inputs.Unet.in_channels_allowed == (1, 2, 3, 4)
    for cin in (0, 5, -1, 2.5, None, "1"):
        with pytest.raises(NotImplementedError):
            vk.inputs.Unet(encoder_weights=None, in_channels=cin)
    m = vk.inputs.Unet(encoder_name="resnet18", encoder_weights=None, in_channels=1)
    with pytest.raises(ValueError, match=r"\[N,1,H,W\]"):
        m(torch.zeros(1, 3, 32, 32))


# ------------------------------------------------------------------------------------------------ 8. argument errors, before any stream
def _bufs():
    return {k: np.full(4096, 7, np.float32) for k in ("x", "x4", "dz", "z", "coef", "w", "dw", "dx", "ws", "out", "M", "b")}


def _refused(vk, who, word, call):
    b = _bufs()
    rc = call({k: v.ctypes.data for k, v in b.items()})
    err = vk.lib().vk_last_error_string().decode()
    assert rc == -1 and word in err and who in err, (who, word, rc, err)
    assert all((v == 7).all() for v in b.values()), (who, word)


@pytest.mark.parametrize("cin", [0, 5, -3, 1 << 20])
def test_entry_points_refuse_a_channel_count_outside_1_to_4(vk, cin):
    Lb, F32, BF16 = vk.lib(), vk._lib.VK_F32, vk._lib.VK_BF16
    for dt in (F32, BF16):
        _refused(vk, "vk_input_transform_c", "cin", lambda p: Lb.vk_input_transform_c(dt, 1, cin, 8, 32, p["x"], p["x4"], None))
        _refused(vk, "vk_stem_wgrad_c", "cin", lambda p: Lb.vk_stem_wgrad_c(dt, 1, 8, 32, cin, p["x4"], p["dz"], p["dw"], p["ws"], 4096, None))
        _refused(vk, "vk_stem_wgrad_c", "cin", lambda p: Lb.vk_stem_wgrad_bn_c(dt, 1, 8, 32, cin, p["x4"], p["dz"], p["z"], p["coef"], p["dw"], None, 0, None))
        _refused(vk, "vk_stem_dgrad_c", "cin", lambda p: Lb.vk_stem_dgrad_c(dt, 1, 8, 32, cin, p["dz"], None, None, p["w"], p["dx"], None))
    _refused(vk, "vk_input_mix", "cout", lambda p: Lb.vk_input_mix(1, cin, 16, p["x"], C.cast(p["M"], C.POINTER(C.c_float)), None, p["out"], None))
    h = C.c_void_p()
    cfg = vk._lib.vk_unet_config(1, 32, F32, 0)
    rc = Lb.vk_unet_create_in(C.byref(cfg), 1, vk._lib.VK_ENC_RESNET34, cin, C.byref(h))
    assert rc == -1 and h.value is None and "in_channels" in Lb.vk_last_error_string().decode()


def test_entry_points_refuse_other_bad_arguments(vk):
    Lb, F32 = vk.lib(), vk._lib.VK_F32
    fp = lambda a: C.cast(a, C.POINTER(C.c_float))      # noqa: E731
    T = "vk_input_transform"
    _refused(vk, T, "bad argument", lambda p: Lb.vk_input_transform_c(F32, 1, 1, 8, 32, None, p["x4"], None))
    _refused(vk, T, "bad argument", lambda p: Lb.vk_input_transform_c(F32, 1, 1, 8, 32, p["x"], None, None))
    _refused(vk, T, "bad argument", lambda p: Lb.vk_input_transform_c(F32, 0, 1, 8, 32, p["x"], p["x4"], None))
    _refused(vk, T, "bad argument", lambda p: Lb.vk_input_transform_c(F32, 1, 1, 0, 32, p["x"], p["x4"], None))
    _refused(vk, T, "bad dtype", lambda p: Lb.vk_input_transform_c(7, 1, 1, 8, 32, p["x"], p["x4"], None))
    _refused(vk, T, "too large", lambda p: Lb.vk_input_transform_c(F32, 65536, 1, 8, 32, p["x"], p["x4"], None))
    _refused(vk, "vk_stem_wgrad", "null", lambda p: Lb.vk_stem_wgrad_c(F32, 1, 8, 32, 1, None, p["dz"], p["dw"], None, 0, None))
    _refused(vk, "vk_stem_wgrad", "null", lambda p: Lb.vk_stem_wgrad_c(F32, 1, 8, 32, 1, p["x4"], p["dz"], None, None, 0, None))
    _refused(vk, "vk_stem_wgrad_bn", "null", lambda p: Lb.vk_stem_wgrad_bn_c(F32, 1, 8, 32, 1, p["x4"], p["dz"], None, p["coef"], p["dw"], None, 0, None))
    _refused(vk, "vk_stem_dgrad", "null", lambda p: Lb.vk_stem_dgrad_c(F32, 1, 8, 32, 1, p["dz"], None, None, None, p["dx"], None))
    _refused(vk, "vk_stem_dgrad", "null", lambda p: Lb.vk_stem_dgrad_c(F32, 1, 8, 32, 1, p["dz"], None, p["coef"], p["w"], p["dx"], None))
    _refused(vk, "vk_stem_dgrad", "W=", lambda p: Lb.vk_stem_dgrad_c(F32, 1, 8, 48, 1, p["dz"], None, None, p["w"], p["dx"], None))
    _refused(vk, "vk_stem_dgrad", "dtype", lambda p: Lb.vk_stem_dgrad_c(9, 1, 8, 32, 1, p["dz"], None, None, p["w"], p["dx"], None))
    X = "vk_input_mix"
    _refused(vk, X, "null", lambda p: Lb.vk_input_mix(1, 1, 16, None, fp(p["M"]), None, p["out"], None))
    _refused(vk, X, "null", lambda p: Lb.vk_input_mix(1, 1, 16, p["x"], None, None, p["out"], None))
    _refused(vk, X, "null", lambda p: Lb.vk_input_mix(1, 1, 16, p["x"], fp(p["M"]), None, None, None))
    _refused(vk, X, "N=0", lambda p: Lb.vk_input_mix(0, 1, 16, p["x"], fp(p["M"]), None, p["out"], None))
    _refused(vk, X, "N=65536", lambda p: Lb.vk_input_mix(65536, 1, 16, p["x"], fp(p["M"]), None, p["out"], None))
    _refused(vk, X, "hw=0", lambda p: Lb.vk_input_mix(1, 1, 0, p["x"], fp(p["M"]), None, p["out"], None))
    _refused(vk, X, "unaligned", lambda p: Lb.vk_input_mix(1, 1, 16, p["x"] + 2, fp(p["M"]), None, p["out"], None))
    _refused(vk, X, "unaligned", lambda p: Lb.vk_input_mix(1, 1, 16, p["x"], fp(p["M"]), None, p["out"] + 1, None))
    h = C.c_void_p()
    cfg = vk._lib.vk_unet_config(1, 32, F32, 0)
    assert Lb.vk_unet_create_in(None, 1, 34, 1, C.byref(h)) == -1 and Lb.vk_unet_create_in(C.byref(cfg), 1, 35, 1, C.byref(h)) == -1
    assert Lb.vk_unet_create_in(C.byref(cfg), 17, 34, 1, C.byref(h)) == -1 and h.value is None
    assert Lb.vk_unet_in_channels(None) == 0
