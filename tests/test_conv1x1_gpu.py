"""The pointwise convolution kernels (csrc/conv1x1.hip) through the C ABI against float64: forward (with and without the producer's
BatchNorm scale / shift + ReLU on the operand, stride 1 / 2, accumulate, train-mode statistics), data gradient (stride-2 scatter,
accumulate) and weight gradient (fixed-order split reduction: the same bits on every run), at resnet50's layer shapes and at small
ragged ones.  fp32 is held to fp32 bars, bf16 / fp16 to bars of their own unit round-off."""
import ctypes as C
import importlib
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
vk = importlib.import_module("vickers-hardness-unet_amd")
L_ = vk._lib
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
CODE = {"f32": L_.VK_F32, "bf16": L_.VK_BF16, "f16": L_.VK_F16}
U = {"f32": 2.0 ** -24, "bf16": 2.0 ** -8, "f16": 2.0 ** -11}      # unit round-off of the stored type
REPL = 32                                                          # VK_STATS_REPLICAS
WS_BYTES = 64 << 20                                                # VK_WGRAD_WORKSPACE_BYTES

# (N, H, W, C, K, stride): resnet50 layer shapes (layer1 conv3 / downsample, layer4 conv1, layer2.0 downsample) and ragged ones
SHAPES = [(2, 128, 128, 64, 256, 1), (2, 16, 16, 2048, 512, 1), (2, 64, 64, 256, 512, 2), (1, 10, 14, 40, 24, 1),
          (1, 9, 13, 24, 40, 2), (3, 6, 5, 16, 136, 1)]
IDS = ["64to256@128", "2048to512@16", "256to512@64s2", "n1_10x14", "n1_9x13s2", "n3_6x5"]


def dev():
    return torch.device("cuda:0")


def st():
    return torch.cuda.current_stream().cuda_stream


def _src(t, Cc, scale=None, shift=None, relu=0):
    return L_.vk_src(t.data_ptr(), Cc, 0, L_.ptr(scale), L_.ptr(shift), relu)


def _null():
    return L_.vk_src(None, 0, 0, None, None, 0)


def _desc(dtn, N, H, W, Ho, Wo, K, stride, transposed, s0):
    return L_.vk_conv_desc(CODE[dtn], N, H, W, Ho, Wo, K, 1, 1, stride, 0, transposed, s0, _null())


def _operand(x, scale, shift, relu, dt):
    """V as the kernel stages it: fma in fp32, ReLU, rounded to the conv's type (then exact in float64)."""
    v = x.float()
    if scale is not None:
        v = torch.addcmul(shift.view(1, 1, 1, -1), v, scale.view(1, 1, 1, -1))
    if relu:
        v = v.clamp_min(0)
    return v.to(dt).double()


def _bound(dtn, y64, absdot, Cred, exact=False):
    """One rounding of the output to the type plus fp32 accumulation; where the operand is transformed (not exact), also one ulp of the
    type per operand element (the reference's fp32 transform may round V to the other neighbour)."""
    u = U[dtn]
    return 2 * u * y64.abs() + ((0.0 if exact else 2 * u) + 4 * math.sqrt(Cred) * 2.0 ** -24) * absdot + 1e-30


def _inputs(N, H, W, Cc, K, dt, seed, transform):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(N, H, W, Cc, generator=g).to(dt).to(dev())
    w = (torch.randn(K, Cc, generator=g) / math.sqrt(Cc)).to(dt).to(dev())
    scale = shift = None
    if transform:
        scale = (0.5 + torch.rand(Cc, generator=g)).to(dev())
        shift = (0.3 * torch.randn(Cc, generator=g)).to(dev())
    return x, w, scale, shift


@pytest.mark.parametrize("transform", [False, True], ids=["plain", "bnrelu"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
@pytest.mark.parametrize("dtn", ["f32", "bf16", "f16"])
def test_forward_stats_accumulate(dtn, shape, transform):
    N, H, W, Cc, K, s = shape
    dt = DT[dtn]
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    x, w, scale, shift = _inputs(N, H, W, Cc, K, dt, 11, transform)
    relu = 1 if transform else 0
    y = torch.empty(N, Ho, Wo, K, dtype=dt, device=dev())
    stats = torch.zeros(REPL, 2, K, dtype=torch.float64, device=dev())
    d = _desc(dtn, N, H, W, Ho, Wo, K, s, 0, _src(x, Cc, scale, shift, relu))
    L_.check(vk.lib().vk_conv1x1_fwd(C.byref(d), w.data_ptr(), y.data_ptr(), 0, stats.data_ptr(), st()), "vk_conv1x1_fwd")
    torch.cuda.synchronize()
    v = _operand(x, scale, shift, relu, dt)[:, ::s, ::s, :]
    w64 = w.double()
    y64 = torch.einsum("nhwc,kc->nhwk", v, w64)
    absdot = torch.einsum("nhwc,kc->nhwk", v.abs(), w64.abs())
    err = (y.double() - y64).abs()
    assert bool((err <= _bound(dtn, y64, absdot, Cc, not transform)).all()), err.max().item()
    # statistics: float64 sums of the STORED values, spread over the replicas
    ys = y.double().reshape(-1, K)
    st_ = stats.sum(0)
    assert torch.allclose(st_[0], ys.sum(0), rtol=0, atol=1e-5 * ys.abs().sum().item() / K + 1e-9)
    assert torch.allclose(st_[1], (ys * ys).sum(0), rtol=1e-5, atol=1e-9)
    # accumulate: y += conv (the sum rounded once to the type)
    y0 = torch.randn(N, Ho, Wo, K, generator=torch.Generator().manual_seed(5)).to(dt).to(dev())
    y2 = y0.clone()
    L_.check(vk.lib().vk_conv1x1_fwd(C.byref(d), w.data_ptr(), y2.data_ptr(), 1, None, st()), "vk_conv1x1_fwd")
    torch.cuda.synchronize()
    ya = y0.double() + y64
    err = (y2.double() - ya).abs()
    assert bool((err <= _bound(dtn, ya, absdot + y0.double().abs(), Cc, not transform)).all()), err.max().item()


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
@pytest.mark.parametrize("dtn", ["f32", "bf16", "f16"])
def test_data_gradient(dtn, shape, accumulate):
    N, H, W, Cc, K, s = shape
    dt = DT[dtn]
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    g = torch.Generator().manual_seed(21)
    dz = torch.randn(N, Ho, Wo, K, generator=g).to(dt).to(dev())
    w = (torch.randn(K, Cc, generator=g) / math.sqrt(K)).to(dt).to(dev())
    wt = w.t().contiguous()                                    # the data-gradient weights [C][K]
    dx0 = torch.randn(N, H, W, Cc, generator=g).to(dt).to(dev())
    dx = dx0.clone()
    d = _desc(dtn, N, Ho, Wo, H, W, Cc, s, 1, _src(dz, K))
    L_.check(vk.lib().vk_conv1x1_fwd(C.byref(d), wt.data_ptr(), dx.data_ptr(), accumulate, None, st()), "vk_conv1x1_fwd(transposed)")
    torch.cuda.synchronize()
    ref = dx0.double() if accumulate else torch.zeros(N, H, W, Cc, dtype=torch.float64, device=dev())
    absd = ref.abs().clone()
    ref[:, ::s, ::s, :] += torch.einsum("nhwk,kc->nhwc", dz.double(), w.double())
    absd[:, ::s, ::s, :] += torch.einsum("nhwk,kc->nhwc", dz.double().abs(), w.double().abs())
    err = (dx.double() - ref).abs()
    assert bool((err <= _bound(dtn, ref, absd, K, True)).all()), err.max().item()
    if s == 2:   # the pixels no tap reaches: zero, or untouched with accumulate
        odd = torch.ones(N, H, W, dtype=torch.bool, device=dev())
        odd[:, ::2, ::2] = False
        want = dx0[odd] if accumulate else torch.zeros_like(dx0[odd])
        assert torch.equal(dx[odd], want)


@pytest.mark.parametrize("transform", [False, True], ids=["plain", "bnrelu"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
@pytest.mark.parametrize("dtn", ["f32", "bf16", "f16"])
def test_weight_gradient_reproducible(dtn, shape, transform):
    N, H, W, Cc, K, s = shape
    dt = DT[dtn]
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    x, _, scale, shift = _inputs(N, H, W, Cc, K, dt, 31, transform)
    relu = 1 if transform else 0
    dz = torch.randn(N, Ho, Wo, K, generator=torch.Generator().manual_seed(32)).to(dt).to(dev())
    ws = torch.empty(WS_BYTES, dtype=torch.uint8, device=dev())
    d = _desc(dtn, N, H, W, Ho, Wo, K, s, 0, _src(x, Cc, scale, shift, relu))
    dw0 = torch.randn(K, Cc, generator=torch.Generator().manual_seed(33)).to(dev())
    runs = []
    for _ in range(2):
        dw = dw0.clone()
        L_.check(vk.lib().vk_conv1x1_wgrad(C.byref(d), dz.data_ptr(), dw.data_ptr(), ws.data_ptr(), WS_BYTES, st()), "vk_conv1x1_wgrad")
        torch.cuda.synchronize()
        runs.append(dw)
    assert torch.equal(runs[0], runs[1]), "weight gradient differs between two runs"
    v = _operand(x, scale, shift, relu, dt)[:, ::s, ::s, :].reshape(-1, Cc)
    z = dz.double().reshape(-1, K)
    ref = dw0.double() + z.t() @ v
    absd = dw0.double().abs() + z.abs().t() @ v.abs()
    P = z.shape[0]
    err = (runs[0].double() - ref).abs()
    # fp32 accumulation, plus one ulp of the type where the reference's fp32 transform rounds V to the other neighbour (as forward)
    bound = ((2 * U[dtn] if transform else 0.0) + 4 * math.sqrt(P) * 2.0 ** -24) * absd + 1e-30
    assert bool((err <= bound).all()), (err / absd).max().item()
    # without a workspace: one split, same result within the fp32 bar
    dw1 = dw0.clone()
    L_.check(vk.lib().vk_conv1x1_wgrad(C.byref(d), dz.data_ptr(), dw1.data_ptr(), None, 0, st()), "vk_conv1x1_wgrad")
    torch.cuda.synchronize()
    assert bool(((dw1.double() - ref).abs() <= bound).all())


def test_unsupported_descriptors_return_error():
    x = torch.zeros(1, 8, 8, 64, dtype=torch.bfloat16, device=dev())
    w = torch.zeros(64, 64, 3, 3, dtype=torch.bfloat16, device=dev())
    y = torch.zeros(1, 8, 8, 64, dtype=torch.bfloat16, device=dev())
    for R, pad, s in ((3, 1, 1), (1, 1, 1), (1, 0, 3)):
        d = L_.vk_conv_desc(L_.VK_BF16, 1, 8, 8, 8, 8, 64, R, R, s, pad, 0, _src(x, 64), _null())
        assert vk.lib().vk_conv1x1_fwd(C.byref(d), w.data_ptr(), y.data_ptr(), 0, None, st()) == -3
        assert vk.lib().vk_conv1x1_wgrad(C.byref(d), y.data_ptr(), w.data_ptr(), None, 0, st()) == -3
    torch.cuda.synchronize()
    assert torch.count_nonzero(y).item() == 0
