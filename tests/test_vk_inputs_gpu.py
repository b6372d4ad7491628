"""vk.inputs on the GPU.

Kernel tier: vk_input_transform_c, vk_stem_fwd on a cin-channel pack, vk_stem_wgrad_c / vk_stem_wgrad_bn_c and vk_stem_dgrad_c for
cin in {1, 2, 4} x {f32, bf16, f16} by EQUALITY with float64 on the integer lattice of tests/inputs_cases.py (whose conditions
tests/test_inputs_cpu.py proves), into sentinel-filled outputs with guards; each _c entry point with cin = 3 torch.equal to the entry point
it generalises; vk_input_mix to the bytes of the fma32 restatement.

Model tier (equalities): vk.inputs.Unet(in_channels=3) is vk.encoders.Unet bit for bit; in_channels = 1, 2 equal the 3-channel model whose
conv1.weight has zero channels appended, on the input with zero planes appended; in_channels = 4 with a zero fourth weight channel and a
random fourth plane equals the 3-channel model.  Bars: fp32 logits and gradients against tests/inputs_ref.py with the float64 arbiter and
the constants of tests/test_encoders_gpu.py, taken over as they stand; the 16-bit input gradient by the yardstick rule of
tests/test_input_grad_gpu.py."""
import contextlib
import copy
import importlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_lattice as CL
import inputs_cases as IC
import inputs_ref as IR

pytestmark = pytest.mark.gpu
vk = importlib.import_module("vickers-hardness-unet_amd")
L_ = vk._lib
DT = CL.TDT
CODE = {"f32": L_.VK_F32, "bf16": L_.VK_BF16, "f16": L_.VK_F16}
REPL = 32                    # VK_STATS_REPLICAS
SENTINEL = 77.0              # exact in every type
K_ARBITER = 4.0              # tests/test_encoders_gpu.py: engine-vs-float64 error <= K_ARBITER x (fp32 restatement-vs-float64 error) ...
FLOOR = 1.5e-2               # ... or the fp32 floor the 3-channel model is held to on these very kernels
ENV_KEYS = ["VK_NO_STEM_TILE", "VK_STEM_WGRAD_TAPS", "VK_WGRAD_ATOMICS"]
shape_id = lambda s: "n%d_%dx%d" % s      # noqa: E731


def dev():
    return torch.device("cuda:0")


def st():
    return torch.cuda.current_stream().cuda_stream


def lib():
    return vk.lib()


def set_env(mp, env):
    for k in ENV_KEYS:
        mp.delenv(k, raising=False)
    for k, v in env.items():
        mp.setenv(k, v)


def nhwc(t, dt):
    return t.permute(0, 2, 3, 1).contiguous().to(dt).to(dev())


def guarded(shape, dt, guard, value=SENTINEL):
    """(whole buffer, view of `shape` that starts `guard` elements in): both guards are checked with intact()."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * guard,), value, dtype=dt, device=dev())
    return buf, buf[guard:guard + n].view(shape)


def intact(buf, guard, value=SENTINEL):
    return bool((buf[:guard] == value).all()) and bool((buf[-guard:] == value).all())


def transform(x, cin, dtn):
    """x float64 NCHW (CPU) through vk_input_transform_c -> x4 [N][H][W][4] of the type, with its guards checked."""
    N, _, H, W = x.shape
    xd = x.float().contiguous().to(dev())
    buf, x4 = guarded((N, H, W, 4), DT[dtn], 64)
    L_.check(lib().vk_input_transform_c(CODE[dtn], N, cin, H, W, xd.data_ptr(), x4.data_ptr(), st()), "vk_input_transform_c")
    torch.cuda.synchronize()
    assert intact(buf, 64)
    return x4


# ================================================================================================ kernel tier
@pytest.mark.parametrize("shape", [(2, 5, 7), (1, 40, 104), (3, 2, 2)], ids=shape_id)
@pytest.mark.parametrize("dtn", IC.DTYPES)
@pytest.mark.parametrize("cin", [1, 2, 3, 4])
def test_input_transform_c(cin, dtn, shape):
    N, H, W = shape
    x = CL.ints((N, cin, H, W), -2, 2, torch.Generator().manual_seed(690 + H + cin))
    x4 = transform(x, cin, dtn)
    got = x4.double().cpu()
    assert torch.equal(got[..., :cin], x.permute(0, 2, 3, 1))
    assert bool((got[..., cin:] == 0).all())                     # the padding channels are written, as zero
    if cin == 3:
        old = torch.full_like(x4, SENTINEL)
        L_.check(lib().vk_input_transform(CODE[dtn], N, H, W, x.float().to(dev()).data_ptr(), old.data_ptr(), st()), "vk_input_transform")
        torch.cuda.synchronize()
        assert torch.equal(old, x4)


@pytest.mark.parametrize("shape", IC.STEM_MAPS, ids=shape_id)
@pytest.mark.parametrize("dtn", IC.DTYPES)
@pytest.mark.parametrize("cin", IC.CINS)
def test_stem_fwd_on_a_cin_channel_pack(cin, dtn, shape, monkeypatch):
    """With 4 channels the fourth column of the pack carries data for the first time."""
    N, H, W = shape
    dt = DT[dtn]
    x, w, _ = IC.stem_operands(N, H, W, cin, 700 + H)
    ref = F.conv2d(x, w, stride=2, padding=3)
    x4 = transform(x, cin, dtn)
    wp = torch.zeros(64, 7, 8, 4, dtype=torch.float64)
    wp[:, :, :7, :cin] = w.permute(0, 2, 3, 1)
    wpd = wp.reshape(64, 7, 32).to(dt).to(dev())
    ref2 = torch.stack([ref.sum(dim=(0, 2, 3)), (ref * ref).sum(dim=(0, 2, 3))])
    outs = {}
    for path, env in (("tile", {}), ("tap", {"VK_NO_STEM_TILE": "1"})):
        set_env(monkeypatch, env)
        buf, y = guarded((N, H // 2, W // 2, 64), dt, 64)
        stats = torch.zeros(REPL * 128, dtype=torch.float64, device=dev())
        L_.check(lib().vk_stem_fwd(CODE[dtn], N, H, W, x4.data_ptr(), wpd.data_ptr(), y.data_ptr(), stats.data_ptr(), st()), "vk_stem_fwd")
        torch.cuda.synchronize()
        assert intact(buf, 64), path
        bad = y.double().cpu().permute(0, 3, 1, 2) != ref
        assert not bool(bad.any()), f"[{path}] {int(bad.sum())} of {bad.numel()} wrong; first at (n, k, h, w) = {tuple(int(v) for v in bad.nonzero()[0])}"
        assert torch.equal(stats.view(REPL, 2, -1).sum(0).cpu(), ref2), path
        outs[path] = y.clone()
    assert torch.equal(outs["tile"], outs["tap"])


def wgrad_reference(x, dzv, cin):
    wv = torch.zeros(64, cin, 7, 7, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, wv, stride=2, padding=3).backward(dzv)
    return (wv.grad + IC.DW0).permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("shape", IC.STEM_MAPS, ids=shape_id)
@pytest.mark.parametrize("dtn", IC.DTYPES)
@pytest.mark.parametrize("cin", IC.CINS)
def test_stem_wgrad_c(cin, dtn, shape, monkeypatch):
    N, H, W = shape
    dt = DT[dtn]
    x, _, dz = IC.stem_operands(N, H, W, cin, 720 + H)
    z, a, bb, cc, dz_bn = IC.bn_fold(dz, 730 + H)
    ref, ref_bn = wgrad_reference(x, dz, cin), wgrad_reference(x, dz_bn, cin)
    x4, dzd, zd = transform(x, cin, dtn), nhwc(dz, dt), nhwc(z, dt)
    coef = torch.cat([a, bb, cc]).float().to(dev())
    ws = torch.empty(16 << 20, dtype=torch.uint8, device=dev())
    errors, slabs = [], []

    def run(path, wsp, bn):
        buf, dw = guarded((64, 7, 7, cin), torch.float32, 64, IC.DW0)      # 64 floats: dw stays 16-byte aligned (the slab form needs it)
        buf[:64] = SENTINEL
        buf[-64:] = SENTINEL
        wp, wn = (wsp.data_ptr(), wsp.numel()) if wsp is not None else (None, 0)
        if bn:
            rc = lib().vk_stem_wgrad_bn_c(CODE[dtn], N, H, W, cin, x4.data_ptr(), dzd.data_ptr(), zd.data_ptr(), coef.data_ptr(), dw.data_ptr(), wp, wn, st())
        else:
            rc = lib().vk_stem_wgrad_c(CODE[dtn], N, H, W, cin, x4.data_ptr(), dzd.data_ptr(), dw.data_ptr(), wp, wn, st())
        torch.cuda.synchronize()
        assert intact(buf, 64), path
        if bn and dtn == "f32":
            assert rc == -3 and bool((dw == IC.DW0).all())                 # VK_ERR_UNSUPPORTED, nothing written
            return None
        L_.check(rc, path)
        bad = dw.double().cpu() != (ref_bn if bn else ref)
        if bool(bad.any()):
            errors.append(f"[{path}] {int(bad.sum())} of {bad.numel()} wrong; first at (k, r, s, c) = {tuple(int(v) for v in bad.nonzero()[0])}")
        return dw.clone()

    for path, env, wsp in (("atomics", {}, None), ("slab", {}, ws), ("slab again", {}, ws), ("taps", {"VK_STEM_WGRAD_TAPS": "1"}, ws)):
        set_env(monkeypatch, env)
        out = run(path, wsp, False)
        if path.startswith("slab"):
            slabs.append(out)
    assert torch.equal(slabs[0], slabs[1])
    set_env(monkeypatch, {})
    for path, wsp in (("bn atomics", None), ("bn slab", ws)):
        run(path, wsp, True)
    assert not errors, "\n".join(errors)


@pytest.mark.parametrize("shape", IC.DGRAD_MAPS, ids=shape_id)
@pytest.mark.parametrize("fold", [0, 1], ids=["plain", "bn"])
@pytest.mark.parametrize("dtn", IC.DTYPES)
@pytest.mark.parametrize("cin", IC.CINS)
def test_stem_dgrad_c(cin, dtn, fold, shape):
    N, H, W = shape
    dt = DT[dtn]
    x, w, dz = IC.stem_operands(N, H, W, cin, 740 + H)
    z, a, bb, cc, dz_bn = IC.bn_fold(dz, 750 + H)
    dzv = dz_bn if fold else dz
    xin = torch.zeros(N, cin, H, W, dtype=torch.float64, requires_grad=True)
    F.conv2d(xin, w, stride=2, padding=3).backward(dzv)
    ref = xin.grad
    dzd, zd = nhwc(dz, dt), nhwc(z, dt)
    coef = torch.cat([a, bb, cc]).float().to(dev())
    wd = w.permute(0, 2, 3, 1).contiguous().float().to(dev())
    buf, dx = guarded((N, cin, H, W), torch.float32, H * W)               # one guard plane either side
    L_.check(lib().vk_stem_dgrad_c(CODE[dtn], N, H, W, cin, dzd.data_ptr(), zd.data_ptr() if fold else None, coef.data_ptr() if fold else None,
                                   wd.data_ptr(), dx.data_ptr(), st()), "vk_stem_dgrad_c")
    torch.cuda.synchronize()
    assert intact(buf, H * W)
    bad = dx.double().cpu() != ref
    assert not bool(bad.any()), f"{int(bad.sum())} of {bad.numel()} wrong; first at (n, c, h, w) = {tuple(int(v) for v in bad.nonzero()[0])}"


@pytest.mark.parametrize("dtn", IC.DTYPES)
def test_three_channels_equal_the_old_entry_points(dtn, monkeypatch):
    N, H, W = 2, 40, 96
    dt = DT[dtn]
    x, w, dz = IC.stem_operands(N, H, W, 3, 760)
    z, a, bb, cc, _ = IC.bn_fold(dz, 761)
    x4, dzd, zd = transform(x, 3, dtn), nhwc(dz, dt), nhwc(z, dt)
    coef = torch.cat([a, bb, cc]).float().to(dev())
    wd = w.permute(0, 2, 3, 1).contiguous().float().to(dev())
    ws = torch.empty(16 << 20, dtype=torch.uint8, device=dev())
    L = lib()
    for env in ({}, {"VK_STEM_WGRAD_TAPS": "1"}):
        set_env(monkeypatch, env)
        for wsp in (None, ws):
            wp, wn = (wsp.data_ptr(), wsp.numel()) if wsp is not None else (None, 0)
            d_old, d_new = (torch.full((64, 7, 7, 3), IC.DW0, dtype=torch.float32, device=dev()) for _ in range(2))
            L_.check(L.vk_stem_wgrad(CODE[dtn], N, H, W, x4.data_ptr(), dzd.data_ptr(), d_old.data_ptr(), wp, wn, st()))
            L_.check(L.vk_stem_wgrad_c(CODE[dtn], N, H, W, 3, x4.data_ptr(), dzd.data_ptr(), d_new.data_ptr(), wp, wn, st()))
            torch.cuda.synchronize()
            assert torch.equal(d_old, d_new)
            if dtn != "f32" and not env:
                d_old, d_new = (torch.full((64, 7, 7, 3), IC.DW0, dtype=torch.float32, device=dev()) for _ in range(2))
                L_.check(L.vk_stem_wgrad_bn(CODE[dtn], N, H, W, x4.data_ptr(), dzd.data_ptr(), zd.data_ptr(), coef.data_ptr(), d_old.data_ptr(), wp, wn, st()))
                L_.check(L.vk_stem_wgrad_bn_c(CODE[dtn], N, H, W, 3, x4.data_ptr(), dzd.data_ptr(), zd.data_ptr(), coef.data_ptr(), d_new.data_ptr(), wp, wn, st()))
                torch.cuda.synchronize()
                assert torch.equal(d_old, d_new)
    set_env(monkeypatch, {})
    for fold in (0, 1):
        g_old, g_new = (torch.full((N, 3, H, W), SENTINEL, dtype=torch.float32, device=dev()) for _ in range(2))
        zz, cf = (zd.data_ptr(), coef.data_ptr()) if fold else (None, None)
        L_.check(L.vk_stem_dgrad(CODE[dtn], N, H, W, dzd.data_ptr(), zz, cf, wd.data_ptr(), g_old.data_ptr(), st()))
        L_.check(L.vk_stem_dgrad_c(CODE[dtn], N, H, W, 3, dzd.data_ptr(), zz, cf, wd.data_ptr(), g_new.data_ptr(), st()))
        torch.cuda.synchronize()
        assert torch.equal(g_old, g_new)


# ================================================================================================ vk_input_mix
MIX_HW = IC.MIX_HW + (8, 4096)          # and sizes that take the 16-byte path: one vector pair, and more than one workgroup


@pytest.mark.parametrize("shift", [(0, 0), (1, 0), (0, 3), (2, 1)], ids=lambda s: "x+%d_out+%d" % s)
@pytest.mark.parametrize("hw", MIX_HW)
@pytest.mark.parametrize("cout", [1, 2, 3, 4])
def test_input_mix_bytes(cout, hw, shift):
    """Plane starts off the 16-byte grid (shift of the tensor's start in floats, and hw % 4 != 0) take the element path."""
    import ctypes as C
    N = 2
    rng = np.random.default_rng(100 * cout + hw % 97)
    x3 = rng.standard_normal((N, 3, hw)).astype(np.float32)
    M = rng.standard_normal((cout, 3)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    want = IC.mix_ref(x3, M, b)
    xbuf = torch.zeros(N * 3 * hw + 8, dtype=torch.float32, device=dev())
    xs = xbuf[shift[0]:shift[0] + N * 3 * hw]
    xs.copy_(torch.from_numpy(x3).flatten())
    obuf = torch.full((N * cout * hw + 16,), SENTINEL, dtype=torch.float32, device=dev())
    o0 = 4 + shift[1]
    out = obuf[o0:o0 + N * cout * hw]
    for bias in (b, None):
        obuf.fill_(SENTINEL)
        L_.check(lib().vk_input_mix(N, cout, hw, xs.data_ptr(), (C.c_float * (3 * cout))(*M.flatten().tolist()),
                                    (C.c_float * cout)(*b.tolist()) if bias is not None else None, out.data_ptr(), st()), "vk_input_mix")
        torch.cuda.synchronize()
        assert bool((obuf[:o0] == SENTINEL).all()) and bool((obuf[o0 + N * cout * hw:] == SENTINEL).all())
        ref = want if bias is not None else IC.mix_ref(x3, M, np.zeros(cout, np.float32))
        assert out.cpu().numpy().tobytes() == ref.tobytes()
    assert xs.cpu().numpy().tobytes() == x3.tobytes()


# ================================================================================================ model tier
def _O():
    from oracle import unet_oracle as O
    return O


def _rel(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-30)).item()


def _loss(lg, y):
    return F.binary_cross_entropy_with_logits(lg, y) + vk.DiceLoss(mode="binary")(lg, y)


def _batch(N, cin, H, W, seed=1234):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, cin, H, W, generator=g), (torch.rand(N, 1, H, W, generator=g) > 0.6).float()


def _step(m, x, y, dtype):
    """One training forward + backward with x.requires_grad: (logits, parameter gradients, x.grad, buffers, the plan's x4)."""
    m.train()
    m.zero_grad(set_to_none=True)
    xd = x.to(dev()).requires_grad_(True)
    ctx = torch.autocast("cuda", dtype=dtype) if dtype != torch.float32 else contextlib.nullcontext()
    with ctx:
        lg = m(xd)
    _loss(lg.float(), y.to(dev())).backward()
    torch.cuda.synchronize()
    plan = m.plan_for(x.shape[0], x.shape[2] if x.shape[2] == x.shape[3] else (x.shape[2], x.shape[3]), dtype, True)
    return (lg.detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters()}, xd.grad.detach().clone(),
            {k: v.detach().clone() for k, v in m.named_buffers()}, plan.debug_tensor("x4"))


def _model(cin, encoder="resnet34", seed=42, cls=None):
    _O().set_seed(seed)
    cls = cls or vk.inputs.Unet
    kw = {} if cls is not vk.inputs.Unet else {"in_channels": cin}
    return cls(encoder_name=encoder, encoder_weights=None, classes=1, activation=None, **kw).to(dev())


def _widened(m_c, cin, encoder):
    """The 3-channel model with m_c's tensors: conv1.weight is m_c's with zero channels appended (or, from 4, its first three)."""
    m3 = _model(3, encoder, seed=1)
    sd = {k: v.clone() for k, v in m_c.state_dict().items()}
    w = sd["encoder.conv1.weight"]
    sd["encoder.conv1.weight"] = torch.cat([w, torch.zeros(64, 3 - cin, 7, 7, device=w.device)], 1) if cin < 3 else w[:, :3].clone()
    m3.load_state_dict(sd)
    return m3


CONFIGS = [("resnet34", (64, 64), torch.float32), ("resnet34", (64, 96), torch.float32), ("resnet34", (64, 64), torch.bfloat16),
           ("resnet34", (64, 96), torch.bfloat16), ("resnet18", (64, 96), torch.bfloat16)]
cfg_id = lambda c: "%s-%dx%d-%s" % (c[0], c[1][0], c[1][1], str(c[2]).replace("torch.", ""))      # noqa: E731


def _same(a, b, c=None):
    """Every entry of the five-tuple of _step equal bit for bit; with c: conv1.weight.grad and x.grad on their first c channels."""
    assert torch.equal(a[0], b[0]), "logits"
    assert a[3].keys() == b[3].keys() and all(torch.equal(a[3][k], b[3][k]) for k in a[3]), "buffers"
    for k in a[1]:
        ga, gb = a[1][k], b[1][k]
        if c is not None and k == "encoder.conv1.weight":
            ga, gb = ga[:, :c], gb[:, :c]
        assert torch.equal(ga, gb), k
    assert torch.equal(a[2] if c is None else a[2][:, :c], b[2] if c is None else b[2][:, :c]), "x.grad"


@pytest.mark.parametrize("cfg", CONFIGS, ids=cfg_id)
def test_three_channels_is_vk_encoders_bit_for_bit(cfg):
    encoder, (H, W), dtype = cfg
    a, b = _model(3, encoder, cls=vk.encoders.Unet), _model(3, encoder)
    x, y = _batch(2, 3, H, W)
    ra, rb = _step(a, x, y, dtype), _step(b, x, y, dtype)
    _same(ra, rb)
    assert torch.equal(ra[4], rb[4])


@pytest.mark.parametrize("cin", [1, 2])
@pytest.mark.parametrize("cfg", CONFIGS, ids=cfg_id)
def test_fewer_channels_equal_the_zero_padded_colour_model(cfg, cin):
    encoder, (H, W), dtype = cfg
    mc = _model(cin, encoder)
    m3 = _widened(mc, cin, encoder)
    x, y = _batch(2, cin, H, W)
    x3 = torch.cat([x, torch.zeros(2, 3 - cin, H, W)], 1)
    rc, r3 = _step(mc, x, y, dtype), _step(m3, x3, y, dtype)
    assert torch.equal(rc[4], r3[4])                 # the x4 the stem's kernels read is byte-identical
    _same(rc, r3, cin)
    assert rc[2].shape == (2, cin, H, W) and rc[1]["encoder.conv1.weight"].shape == (64, cin, 7, 7)


@pytest.mark.parametrize("cfg", CONFIGS, ids=cfg_id)
def test_four_channels_with_a_zero_weight_channel_equal_the_colour_model(cfg):
    encoder, (H, W), dtype = cfg
    m4 = _model(4, encoder)
    with torch.no_grad():
        m4.state_dict()["encoder.conv1.weight"][:, 3].zero_()
    m4.mark_weights_dirty()
    m3 = _widened(m4, 4, encoder)
    x, y = _batch(2, 4, H, W)                         # the fourth plane is random and finite
    r4, r3 = _step(m4, x, y, dtype), _step(m3, x[:, :3].contiguous(), y, dtype)
    assert torch.equal(r4[4][..., :3], r3[4][..., :3]) and bool((r3[4][..., 3] == 0).all())
    _same(r4, r3, 3)                                  # exact zeros added to an fp32 accumulator change nothing
    if dtype == torch.float32 and encoder == "resnet34":
        # the fourth channel's weight gradient has no 3-channel counterpart: float64 decides, with the arbiter's bar
        ref = IR.build(encoder, 4)
        ref.load_state_dict({k: v.cpu() for k, v in m4.state_dict().items()})
        ref.train()
        ref64 = copy.deepcopy(ref).double()
        _O().total_loss(ref(x), y).backward()
        _O().total_loss(ref64(x.double()), y.double()).backward()
        g64 = ref64.encoder.conv1.weight.grad[:, 3]
        e, o = _rel(r4[1]["encoder.conv1.weight"][:, 3].cpu(), g64), _rel(ref.encoder.conv1.weight.grad[:, 3], g64)
        print(f"conv1.weight.grad[:, 3] vs float64: engine {e:.2e}, fp32 restatement {o:.2e}")
        assert e <= max(K_ARBITER * o, FLOOR), (e, o)


@pytest.mark.parametrize("case", [("resnet34", 1, (64, 96)), ("resnet34", 2, (64, 64)), ("resnet34", 4, (64, 96)), ("resnet18", 1, (64, 64))],
                         ids=lambda c: "%s-c%d-%dx%d" % (c[0], c[1], c[2][0], c[2][1]))
def test_fp32_logits_and_gradients_float64_arbiter(case):
    encoder, cin, (H, W) = case
    O = _O()
    ref = IR.build(encoder, cin, seed=42)
    m = _model(cin, encoder, seed=42)
    for k, v in ref.state_dict().items():
        assert torch.equal(m.state_dict()[k].cpu(), v), k
    x, y = _batch(2, cin, H, W)
    ref.train()
    ref64 = copy.deepcopy(ref).double()
    x32, x64 = x.clone().requires_grad_(True), x.double().requires_grad_(True)
    lr = ref(x32)
    O.total_loss(lr, y).backward()
    l64 = ref64(x64)
    O.total_loss(l64, y.double()).backward()
    lg, grads, gx, bufs, _ = _step(m, x, y, torch.float32)
    e_lg, o_lg = _rel(lg.cpu(), l64.detach()), _rel(lr.detach(), l64.detach())
    print(f"{encoder} c={cin} {H}x{W}: logits vs float64: engine {e_lg:.2e}, fp32 restatement {o_lg:.2e}")
    assert e_lg <= max(K_ARBITER * o_lg, FLOOR)
    n32, n64 = dict(ref.named_parameters()), dict(ref64.named_parameters())
    assert set(n32) == set(grads)
    e64 = {k: _rel(g.cpu(), n64[k].grad) for k, g in grads.items()}
    o64 = max(_rel(n32[k].grad, n64[k].grad) for k in n32)
    worst = max(e64, key=e64.get)
    print(f"   gradients vs float64: engine worst {e64[worst]:.2e} ({worst}), fp32 restatement worst {o64:.2e}")
    assert e64[worst] <= max(K_ARBITER * o64, FLOOR), (worst, e64[worst], o64)
    e_x, o_x = _rel(gx.cpu(), x64.grad), _rel(x32.grad, x64.grad)
    print(f"   x.grad vs float64: engine {e_x:.2e}, fp32 restatement {o_x:.2e}")
    assert gx.shape == x.shape and e_x <= max(K_ARBITER * o_x, FLOOR), (e_x, o_x)
    for k, b in ref.state_dict().items():
        if k.endswith("running_mean") or k.endswith("running_var"):
            assert torch.allclose(bufs[k].cpu(), b, rtol=1e-4, atol=1e-5), k


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_gray_x_grad_16bit_vs_yardstick(dtype):
    """The rule of tests/test_input_grad_gpu.py: relative L2 against float64 <= 1.5 x the CPU-autocast restatement's + 0.02."""
    O = _O()
    ref = IR.build("resnet34", 1, seed=5).train()
    x, y = _batch(2, 1, 64, 64, seed=4322)

    def xgrad(model, xin, amp=None):
        r = copy.deepcopy(model).train()
        xr = xin.clone().requires_grad_(True)
        with (torch.autocast("cpu", dtype=amp) if amp is not None else contextlib.nullcontext()):
            lo = r(xr)
        O.total_loss(lo.to(xin.dtype), y.to(xin.dtype)).backward()
        return xr.grad.detach()

    gx64, gxy = xgrad(copy.deepcopy(ref).double(), x.double()), xgrad(ref, x, amp=dtype)
    m = _model(1, "resnet34", seed=6)
    m.load_state_dict(ref.state_dict())
    _, _, gx, _, _ = _step(m, x, y, dtype)
    assert gx.dtype == torch.float32 and torch.isfinite(gx).all()
    e, e_y = _rel(gx.cpu(), gx64), _rel(gxy, gx64)
    print(f"[gray x.grad {dtype}] engine rel L2 {e:.3e}, yardstick {e_y:.3e}")
    assert e <= 1.5 * e_y + 0.02, (e, e_y)


@pytest.mark.parametrize("cin,dtype", [(1, torch.float32), (4, torch.bfloat16), (2, torch.float16)])
def test_two_backwards_give_identical_bits(cin, dtype):
    m = _model(cin)
    x, y = _batch(2, cin, 64, 96)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    a = _step(m, x, y, dtype)
    m.load_state_dict(before)                         # the running statistics moved: put them back
    b = _step(m, x, y, dtype)
    _same(a, b)


def test_bf16_fused_adamw_trajectory_on_gray():
    O = _O()
    ref = IR.build("resnet34", 1, seed=42)
    m = _model(1, seed=42)
    x3, y = O.synthetic_batch(4, 64, seed=99)
    x = x3[:, :1].contiguous()
    ref.train(); m.train()
    opt_r = torch.optim.AdamW(ref.parameters(), lr=1e-3, weight_decay=1e-4)
    opt_g = vk.adamw_for(m, lr=1e-3, weight_decay=1e-4)
    assert isinstance(opt_g, vk.FusedAdamW)
    lr_hist = O.train_steps(ref, opt_r, [(x, y)] * 3)
    lg_hist = []
    for _ in range(3):
        opt_g.zero_grad(set_to_none=True)
        lg_hist.append(float(m.loss_and_backward(x.to(dev()), y.to(dev()), dtype=torch.bfloat16)[0]))
        opt_g.step()
    print(f"gray bf16 losses {lg_hist} fp32 restatement {lr_hist}")
    for a, b in zip(lg_hist, lr_hist):                # the bar of tests/test_encoders_gpu.py::test_bf16_adamw_trajectory
        assert abs(a - b) <= 3e-2 * abs(b), (lg_hist, lr_hist)
    assert lg_hist[-1] < lg_hist[0]


def test_load_pretrained_gray_against_colour_on_a_replicated_batch():
    """fp32 eval: the stem output of the colour model on (g, g, g) against the gray model's on g, within IC.gray_stem_bound; every other
    tensor of the gray model is the checkpoint's."""
    colour = _model(3, cls=vk.Unet, seed=8)
    ck = {k: v.clone() for k, v in colour.state_dict().items()}
    gray = _model(1, seed=9)
    vk.inputs.load_pretrained(gray, ck)
    for k, v in gray.state_dict().items():
        if k != "encoder.conv1.weight":
            assert torch.equal(v, ck[k]), k
    assert torch.equal(gray.state_dict()["encoder.conv1.weight"], ck["encoder.conv1.weight"].sum(1, keepdim=True))
    g = torch.randn(2, 1, 64, 96, generator=torch.Generator().manual_seed(3))
    colour.eval(); gray.eval()
    with torch.no_grad():
        lc = colour(g.expand(-1, 3, -1, -1).contiguous().to(dev()))
        lg = gray(g.to(dev()))
    zc = colour.plan_for(2, (64, 96), torch.float32, False).debug_tensor("z:encoder.conv1").double().cpu().permute(0, 3, 1, 2)
    zg = gray.plan_for(2, (64, 96), torch.float32, False).debug_tensor("z:encoder.conv1").double().cpu().permute(0, 3, 1, 2)
    bound = IC.gray_stem_bound(g, ck["encoder.conv1.weight"].cpu())
    ratio = float(((zc - zg).abs() / bound.clamp_min(1e-300)).max())
    print(f"stem output colour vs gray: max |difference| / bound = {ratio:.3f}; logits max |difference| = {float((lc - lg).abs().max()):.3e}")
    assert bool(((zc - zg).abs() <= bound).all())
    assert torch.isfinite(lg).all() and lg.shape == lc.shape


def test_segmenter_over_a_channel_adapter_returns_the_bytes_of_the_hand_path():
    m = _model(1, "resnet18", seed=12)
    ad = vk.inputs.ChannelAdapter(m, mode="luma")
    img = np.full((90, 120, 3), 200, np.uint8)
    img[30:62, 40:72] = 60                            # a rendered square
    seg = vk.Segmenter(ad, img_size=64, device=dev())
    got = seg.infer(img)
    x, meta = vk.prepost.preprocess(img, 64, "centered", dev())
    mixed = ad.mix(x)
    assert mixed.shape == (1, 1, 64, 64)
    with torch.no_grad():
        lg = m.eval()(mixed)
    want = vk.prepost.postprocess_prob(lg[0, 0], meta).cpu().numpy()
    assert got.shape == (90, 120) and got.tobytes() == want.tobytes()
    # the mix itself: the bytes of the restatement
    ref = IC.mix_ref(x.cpu().numpy().reshape(1, 3, -1), np.asarray(ad.matrix), np.asarray(ad.bias))
    assert mixed.cpu().numpy().tobytes() == ref.tobytes()
    # loss_and_backward goes through the same mix; no gradient flows to x3
    x3 = x.expand(2, -1, -1, -1).contiguous().requires_grad_(True)
    y = (torch.rand(2, 1, 64, 64, device=dev()) > 0.5).float()
    out = ad.loss_and_backward(x3, y)
    assert torch.isfinite(out).all() and x3.grad is None
    m.zero_grad(set_to_none=True)
    want_loss = m.loss_and_backward(ad.mix(x3), y)
    assert torch.equal(out, want_loss)


def test_ema_and_checkpoint_round_trip_of_a_four_channel_model():
    m = _model(4, seed=21)
    x, y = _batch(2, 4, 64, 64, seed=77)
    opt = vk.adamw_for(m, lr=1e-3, weight_decay=1e-4)
    ema = vk.ModelEMA(m, decay=0.9)
    for _ in range(2):
        opt.zero_grad(set_to_none=True)
        m.loss_and_backward(x.to(dev()), y.to(dev()))
        opt.step()
        ema.update()
    fresh = _model(4, seed=22)
    fresh.load_state_dict({k: v.clone() for k, v in m.state_dict().items()})
    assert all(torch.equal(v, fresh.state_dict()[k]) for k, v in m.state_dict().items())
    m.eval(); fresh.eval()
    # one image: a shape m has no training plan for, so that all three models run the eval plan (a training plan that serves an eval
    # forward takes other kernel forms; tests/test_vk_averaging_gpu.py compares on n = 1 for the same reason)
    xe = x[:1].contiguous().to(dev())
    with torch.no_grad():
        assert torch.equal(m(xe), fresh(xe))
        avg = _model(4, seed=23)
        avg.load_state_dict(ema.state_dict())
        avg.eval()
        want = avg(xe)
        assert not torch.equal(want, m(xe))
        with ema.applied():
            assert torch.equal(m(xe), want)
    assert avg.state_dict()["encoder.conv1.weight"].shape == (64, 4, 7, 7)
