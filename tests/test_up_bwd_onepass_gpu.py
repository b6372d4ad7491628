"""vk_conv_bwd_onepass with an upsampled source (-m gpu): BatchNorm-backward apply + 2x2-pooled data gradient + weight gradient of the
32 -> 16 decoder convolution behind the nearest-x2 upsample (decoder block 4 conv1) in one kernel, against the three launches it
replaces (vk_bn_bwd_apply, vk_conv_dgrad_fused with pool2 and bnr on the streaming kernel, vk_conv_wgrad with src0.up = 1), against
float64 autograd, on the integer lattice of tests/bwd_onepass_up_cases.py (equality), and through the engine (VK_NO_ONEPASS_UP=1
restores the three launches of that layer alone)."""
import ctypes as C
import importlib

import pytest
import torch
import torch.nn.functional as F

import bwd_onepass_up_cases as UC

pytestmark = pytest.mark.gpu

vk = importlib.import_module("vickers-hardness-unet_amd")
L_ = vk._lib

DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
REPL = 32       # VK_STATS_REPLICAS in include/vk_unet.h
KEEP = []       # device tensors must outlive the asynchronous launches that read them
UNSUPPORTED = -3


def dev():
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _keepalive():
    KEEP.clear()
    yield
    torch.cuda.synchronize()
    KEEP.clear()


def D(t):
    t = t.to(dev())
    KEEP.append(t)
    return t


def st():
    return torch.cuda.current_stream().cuda_stream


def nhwc(x, dt):         # NCHW cpu -> NHWC dt cuda
    return D(x.permute(0, 2, 3, 1).contiguous().to(dt))


def nchw(t):             # NHWC cuda -> NCHW float64 cpu
    return t.double().cpu().permute(0, 3, 1, 2).contiguous()


def gen(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


class Layer:
    """Device operands of the layer's backward.  g, z: [N][K][H][W]; z1: [N][Cc][H/2][W/2] (the source before the upsample);
    w_dgrad [Cc][K][3][3].  `tensors` (NHWC device tensors g, z, z1) replaces the host operands for maps too large for a host reference."""

    def __init__(self, dt, g, z, z1, coef, scale, shift, w_dgrad, up=1, tensors=None):
        self.dt, self.code, self.up = dt, L_.dtype_code(dt), up
        if tensors is None:
            self.N, self.K, self.H, self.W = g.shape
            self.Cc = z1.shape[1]
            self.g, self.z, self.z1 = nhwc(g, dt), nhwc(z, dt), nhwc(z1, dt)
        else:
            self.g, self.z, self.z1 = tensors
            self.N, self.H, self.W, self.K = self.g.shape
            self.Cc = self.z1.shape[3]
        self.Hs, self.Ws = self.z1.shape[1], self.z1.shape[2]
        self.coef, self.scale, self.shift = D(coef.float().contiguous()), D(scale.float()), D(shift.float())
        none = L_.vk_src(None, 0, 0, None, None, 0)
        self.d_fwd = L_.vk_conv_desc(self.code, self.N, self.H, self.W, self.H, self.W, self.K, 3, 3, 1, 1, 0,
                                     L_.vk_src(self.z1.data_ptr(), self.Cc, up, self.scale.data_ptr(), self.shift.data_ptr(), 1), none)
        self.dz = D(torch.empty_like(self.g))
        self.d_dg = L_.vk_conv_desc(self.code, self.N, self.H, self.W, self.H, self.W, self.Cc, 3, 3, 1, 1, 1,
                                    L_.vk_src(self.dz.data_ptr(), self.K, 0, None, None, 0), none)
        w = D(w_dgrad.permute(0, 2, 3, 1).contiguous().to(dt))                       # [Cc][3][3][K]
        self.w = D(torch.empty_like(w))
        if dt != torch.float32 and vk.lib().vk_conv_uses_halo_pack(C.byref(self.d_dg)):
            L_.check(vk.lib().vk_halo_pack(self.code, self.Cc, self.K, w.data_ptr(), self.w.data_ptr(), st()))
        else:
            self.w.copy_(w)
        self.ws = D(torch.empty(64 << 20, dtype=torch.uint8))

    def outputs(self):
        y = torch.full((self.N, self.Hs, self.Ws, self.Cc), float("nan"), device=dev(), dtype=self.dt)
        sums = torch.zeros(REPL * 2 * self.Cc, dtype=torch.float64, device=dev())
        dw = torch.zeros(self.K, 3, 3, self.Cc, dtype=torch.float32, device=dev())
        KEEP.extend([y, sums, dw])
        return y, sums, dw, L_.vk_bnr(self.z1.data_ptr(), self.scale.data_ptr(), self.shift.data_ptr(), sums.data_ptr())

    def onepass_rc(self, y, dw, bnr):
        return vk.lib().vk_conv_bwd_onepass(C.byref(self.d_fwd), self.g.data_ptr(), self.z.data_ptr(), self.coef.data_ptr(), self.w.data_ptr(),
                                            y.data_ptr(), C.byref(bnr), dw.data_ptr(), self.ws.data_ptr(), self.ws.numel(), st())

    def onepass(self):
        y, sums, dw, bnr = self.outputs()
        L_.check(self.onepass_rc(y, dw, bnr), "vk_conv_bwd_onepass")
        torch.cuda.synchronize()
        return y, sums.view(REPL, 2, self.Cc).sum(0), dw

    def three(self):
        """vk_bn_bwd_apply -> vk_conv_dgrad_fused (pool2, bnr: the streaming kernel) -> vk_conv_wgrad (src0.up = 1); leaves the stored dz."""
        lib = vk.lib()
        y, sums, dw, bnr = self.outputs()
        L_.check(lib.vk_bn_bwd_apply(self.code, self.N * self.H * self.W, self.K, self.g.data_ptr(), self.z.data_ptr(), 0, None, None, None,
                                     self.coef.data_ptr(), self.dz.data_ptr(), None, 0, st()))
        L_.check(lib.vk_conv_dgrad_fused(C.byref(self.d_dg), self.w.data_ptr(), y.data_ptr(), None, 0, 1, C.byref(bnr), st()))
        L_.check(lib.vk_conv_wgrad(C.byref(self.d_fwd), self.dz.data_ptr(), dw.data_ptr(), self.ws.data_ptr(), self.ws.numel(), st()))
        torch.cuda.synchronize()
        return y, sums.view(REPL, 2, self.Cc).sum(0), dw

    def refused(self):
        """The entry point declines before any launch: y stays NaN, dw and the sums stay zero."""
        y, sums, dw, bnr = self.outputs()
        assert self.onepass_rc(y, dw, bnr) == UNSUPPORTED
        torch.cuda.synchronize()
        assert torch.isnan(y).all() and not dw.any() and not sums.any()


def operands(Cc, K, N, H, W, zero_gz=False, hs=None, ws=None):
    g, z = gen(N, K, H, W, seed=801), gen(N, K, H, W, seed=802)
    if zero_gz:                                     # dz = c everywhere inside the map: the constant must not reach the padding
        g, z = torch.zeros_like(g), torch.zeros_like(z)
    z1 = gen(N, Cc, hs if hs is not None else H // 2, ws if ws is not None else W // 2, seed=803)
    coef = torch.stack([0.5 + torch.rand(K, generator=torch.Generator().manual_seed(804)), gen(K, seed=805, scale=0.2),
                        gen(K, seed=806, scale=0.5) + (1.0 if zero_gz else 0.0)])
    scale, shift = 0.5 + torch.rand(Cc, generator=torch.Generator().manual_seed(807)), gen(Cc, seed=808, scale=0.3)
    w_dgrad = gen(Cc, K, 3, 3, seed=809, scale=0.05)
    return g, z, z1, coef, scale, shift, w_dgrad


def random_layer(dt, N, H, W, zero_gz=False):
    return Layer(dt, *operands(32, 16, N, H, W, zero_gz))


def compare_with_three_launches(L):
    (ya, sa, wa), (yb, sb, wb) = L.three(), L.onepass()
    assert not torch.isnan(yb.float()).any()
    assert torch.equal(ya, yb), (ya.float() - yb.float()).abs().max().item()
    # equal stored values: fp32 summation order (the bound of test_stream_conv_kernels_match_tile_kernels)
    assert torch.allclose(sa, sb, rtol=1e-5, atol=1e-5 * (1.0 + sa.abs().max().item())), (sa - sb).abs().max().item()
    # the weight gradient against float64 autograd on the ROUNDED dz and the upsampled V, and against vk_conv_wgrad on that dz
    dt = L.dt
    v = torch.relu(nchw(L.z1).float() * L.scale.cpu().view(1, -1, 1, 1) + L.shift.cpu().view(1, -1, 1, 1)).to(dt).double()
    v = F.interpolate(v, scale_factor=2, mode="nearest")
    wv = torch.zeros(L.K, L.Cc, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(v, wv, padding=1).backward(nchw(L.dz))
    ref = wv.grad.float()
    scale = ref.abs().max().item() + 1e-6
    e64 = (wb.cpu().permute(0, 3, 1, 2) - ref).abs().max().item()
    e3 = (wb - wa).abs().max().item()
    print(f"dw: max|ref| {scale:.4g}  vs float64 {e64 / scale:.3g}  vs vk_conv_wgrad {e3 / scale:.3g}")
    assert e64 <= 2e-3 * scale
    assert e3 <= 1e-4 * scale
    # two runs, the same bits
    y2, s2, w2 = L.onepass()
    assert torch.equal(y2, yb) and torch.equal(w2, wb)


MAPS = [(2, 72, 40), (1, 132, 20), (3, 6, 96), (1, 2, 2), (2, 40, 22)]


@pytest.mark.parametrize("dtn", ["bf16", "f16"])
@pytest.mark.parametrize("shape", MAPS, ids=["72x40", "tall", "short", "one_pixel", "half_width_11"])
def test_onepass_up_matches_three_launches(shape, dtn, monkeypatch):
    """A ragged strip in x; a tall map with a ragged second strip and half-width 10; one shorter than a row group; one pooled pixel;
    half-width 11 (an odd source extent: the source halo is ragged)."""
    monkeypatch.delenv("VK_STREAM_RS", raising=False)
    compare_with_three_launches(random_layer(DT[dtn], *shape))


@pytest.mark.parametrize("dtn", ["bf16", "f16"])
@pytest.mark.parametrize("rs", ["8", "24"])
def test_onepass_up_at_forced_strip_heights(rs, dtn, monkeypatch):
    """VK_STREAM_RS sets the strip height of both the streaming data gradient and the one-pass kernel: 9 / 3 strips per column of a 72-row map."""
    monkeypatch.setenv("VK_STREAM_RS", rs)
    compare_with_three_launches(random_layer(DT[dtn], 2, 72, 40))


@pytest.mark.parametrize("dtn", ["bf16", "f16"])
def test_onepass_up_constant_does_not_leak_into_the_padding(dtn, monkeypatch):
    """g = z = 0 with c != 0: dz is the constant c inside the map and must be zero outside it."""
    monkeypatch.delenv("VK_STREAM_RS", raising=False)
    compare_with_three_launches(random_layer(DT[dtn], 2, 40, 24, zero_gz=True))


def test_onepass_up_sums_keep_the_streaming_kernels_partials(monkeypatch):
    """(8, 512, 512): the one-pass kernel takes a taller strip (64 rows) than the streaming data gradient (32); the fp32 partials of the
    BN-backward sums must still cover the streaming kernel's strips, so that the sums agree to the fp64 additions alone.  Bound: at most
    2^13 fp32 partials per channel added in fp64 in any order, 2^13 * 2^-53 = 1e-12 relative to the largest sum; an fp32 partial over
    another span would differ by about 1e-7.  g1 equal, on operands generated on the device (no host reference at this size)."""
    monkeypatch.delenv("VK_STREAM_RS", raising=False)
    N, H, W = 8, 512, 512
    _, _, _, coef, scale, shift, w_dgrad = operands(32, 16, 1, 2, 2)
    gd = torch.Generator(device=dev()).manual_seed(811)
    dt = torch.bfloat16
    g, z = (D(torch.randn(N, H, W, 16, device=dev(), generator=gd).to(dt)) for _ in range(2))
    z1 = D(torch.randn(N, H // 2, W // 2, 32, device=dev(), generator=gd).to(dt))
    L = Layer(dt, None, None, None, coef, scale, shift, w_dgrad, tensors=(g, z, z1))
    (ya, sa, wa), (yb, sb, wb) = L.three(), L.onepass()
    assert torch.equal(ya, yb)
    err = (sa - sb).abs().max().item()
    print(f"sums: max {sa.abs().max().item():.4g}  max difference {err:.3g}")
    assert err <= 1e-11 * (1.0 + sa.abs().max().item())
    scale_w = wa.abs().max().item()
    assert (wa - wb).abs().max().item() <= 1e-4 * scale_w


def test_onepass_up_refuses_fp32_before_any_launch():
    random_layer(torch.float32, 1, 16, 16).refused()


def test_onepass_up_refuses_an_odd_height_before_any_launch():
    """H = 15 with an 8 x 8 source: the nearest-x2 upsample has no odd extent."""
    Layer(torch.bfloat16, *operands(32, 16, 1, 15, 16, hs=8, ws=8)).refused()


def test_onepass_up_refuses_other_channel_counts_before_any_launch():
    """(C, K) = (64, 32) behind the upsample (decoder block 3 conv1's upsampled half) is not covered."""
    Layer(torch.bfloat16, *operands(64, 32, 1, 16, 16)).refused()


EXACT = UC.cases()


@pytest.mark.parametrize("dtn", ["bf16", "f16"])
@pytest.mark.parametrize("case", EXACT, ids=[UC.case_id(c) for c in EXACT])
def test_onepass_up_exact_on_the_integer_lattice(case, dtn, monkeypatch):
    """Small-integer operands, a from {0.5, 1, 2}, b from {-0.5, 0, 0.5}, integer c, ternary weights: dz (as vk_bn_bwd_apply stores it), the
    pooled and masked y, the sums and dw EQUAL the float64 reference in both types; the exactness conditions hold on the reference alone
    (UC.check)."""
    monkeypatch.delenv("VK_STREAM_RS", raising=False)
    b = UC.build(case)
    UC.check(b)
    L = Layer(DT[dtn], b.g, b.z, b.z1, b.coef, b.scale, b.shift, b.w_dgrad)
    _, _, _ = L.three()
    assert torch.equal(nchw(L.dz), b.dz)
    y, sums, dw = L.onepass()
    assert torch.equal(nchw(y), b.y), (nchw(y) - b.y).abs().max().item()
    assert torch.equal(sums.cpu(), b.sums), (sums.cpu() - b.sums).abs().max().item()
    assert torch.equal(dw.double().cpu().permute(0, 3, 1, 2), b.dw), (dw.double().cpu().permute(0, 3, 1, 2) - b.dw).abs().max().item()


TAG = "bwd_onepass_16b_c32up_k16"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("n,h,w", [(4, 128, 128), (2, 96, 160)])
def test_engine_onepass_up_matches_three_launches(monkeypatch, dtype, n, h, w):
    """One backward of the resnet34 U-Net with decoder block 4 conv1 on the one-pass kernel and one with VK_NO_ONEPASS_UP=1: the profile
    tag is there exactly when the route is on, the loss is equal, the gradients agree to summation order (the bound of
    test_fused_and_autograd_paths_agree), and the one-pass route gives the same bits run to run."""
    from oracle import unet_oracle as O
    O.set_seed(36)
    monkeypatch.delenv("VK_NO_ONEPASS", raising=False)
    monkeypatch.delenv("VK_STREAM_RS", raising=False)
    m = vk.Unet(encoder_name="resnet34", encoder_weights=None, in_channels=3, classes=1, activation=None).to(dev()).train()
    opt = vk.adamw_for(m, lr=1e-3, weight_decay=1e-4)
    g = torch.Generator().manual_seed(710)
    x = torch.randn(n, 3, h, w, generator=g).to(dev())
    y = (torch.rand(n, 1, h, w, generator=g) > 0.7).float().to(dev())
    gs = 1024.0 if dtype == torch.float16 else 1.0

    def backward(off):
        if off:
            monkeypatch.setenv("VK_NO_ONEPASS_UP", "1")
        else:
            monkeypatch.delenv("VK_NO_ONEPASS_UP", raising=False)
        opt.zero_grad(set_to_none=True)
        lib = vk.lib()
        torch.cuda.synchronize()
        lib.vk_prof_enable(1)
        try:
            loss = m.loss_and_backward(x, y, grad_scale=gs, dtype=dtype).clone()
            torch.cuda.synchronize()
        finally:
            lib.vk_prof_enable(0)
        tags = set(L_.prof_collect())
        assert (TAG in tags) == (not off), sorted(tags)
        assert "bwd_onepass_16b_c16" in tags and "bwd_onepass_16b_c32" in tags, sorted(tags)      # the other two layers keep their route
        return loss, m.flat_grads.detach().clone()

    (l1, g1), (l2, g2), (l0, g0) = backward(False), backward(False), backward(True)
    assert torch.equal(l1, l2) and torch.equal(g1, g2)
    assert torch.equal(l1, l0), (l1, l0)
    assert not torch.equal(g1, torch.zeros_like(g1))
    denom = g0.abs().max().item()
    err = (g1 - g0).abs().max().item()
    print(f"flat_grads: max|g| {denom:.4g}  one-pass vs three launches {err / denom:.3g}")
    assert err <= 1e-4 * denom
