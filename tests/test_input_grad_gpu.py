"""The gradient of the model's input (x.grad) on the MI355X: the stem data-gradient kernel through the C ABI against the float64
conv2d input gradient, and x.grad of the nn.Module against plain torch.nn autograd in three fine-tuning set-ups and under autocast."""
import contextlib
import copy
import ctypes as C
import importlib

import pytest
import torch

pytestmark = pytest.mark.gpu
vk = importlib.import_module("vickers-hardness-unet_amd")
DT = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}


def dev():
    return torch.device("cuda:0")


def _O():
    from oracle import unet_oracle as O
    return O


def rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


# bars on relative L2 against float64: fp32 runs on the fp32 MFMA (full fp32 products, fp32 sums); 16-bit rounds dz to the storage type
# before the MFMA (bf16: 8 bits of mantissa, fp16: 11), the weights likewise, and sums in fp32
_BAR = {torch.float32: 1e-5, torch.bfloat16: 1.2e-2, torch.float16: 2e-3}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("with_coef", [False, True], ids=["dz", "bna"])
@pytest.mark.parametrize("n,h,w", [(1, 64, 64), (3, 64, 64), (1, 96, 160), (3, 96, 160), (2, 512, 512)])
def test_stem_dgrad_vs_conv2d_input_grad(dtype, with_coef, n, h, w):
    L = vk.lib()
    gen = torch.Generator().manual_seed(n * 1000 + h + w + (7 if with_coef else 0))
    ho, wo = h // 2, w // 2
    wt = torch.randn(64, 3, 7, 7, generator=gen) * 0.05
    w_krsc = wt.permute(0, 2, 3, 1).contiguous().to(dev())
    g = torch.randn(n, ho, wo, 64, generator=gen).to(dtype)                 # NHWC, as the engine stores it
    if with_coef:
        z = torch.randn(n, ho, wo, 64, generator=gen).to(dtype)
        coef = torch.randn(3, 64, generator=gen) * torch.tensor([[1.0], [0.1], [0.01]])
        dz = coef[0].double() * g.double() + coef[1].double() * z.double() + coef[2].double()
    else:
        z, coef, dz = None, None, g.double()
    ref = torch.nn.grad.conv2d_input((n, 3, h, w), wt.double(), dz.permute(0, 3, 1, 2).contiguous(), stride=2, padding=3)
    gd = g.to(dev())
    zd = z.to(dev()) if z is not None else None
    cd = coef.contiguous().to(dev()) if coef is not None else None
    dx = torch.full((n, 3, h, w), float("nan"), device=dev())               # dirty: every element must be WRITTEN
    vk._lib.check(L.vk_stem_dgrad(DT[dtype], n, h, w, gd.data_ptr(), zd.data_ptr() if zd is not None else None,
                                  cd.data_ptr() if cd is not None else None, w_krsc.data_ptr(), dx.data_ptr(),
                                  vk._lib.current_stream()), "vk_stem_dgrad")
    torch.cuda.synchronize()
    out = dx.cpu()
    assert torch.isfinite(out).all()
    e = rel(out, ref)
    assert e <= _BAR[dtype], (dtype, with_coef, n, h, w, e)


def warm_oracle(n, s, seed=5):
    O = _O()
    O.set_seed(seed)
    ref = O.build_model().train()
    with torch.no_grad():
        for k in range(3):
            ref(O.synthetic_batch(n, s, seed=700 + k)[0])
    return ref


SETUPS = {
    "saliency": lambda m: (m.eval(), m.requires_grad_(False)),
    "train_all": lambda m: m.train(),
    "train_encoder_frozen": lambda m: (m.train(), m.encoder.requires_grad_(False)),
}


def _oracle_xgrad(ref, setup, x, y, dtype, amp=None):
    O = _O()
    r = copy.deepcopy(ref).to(dtype)
    SETUPS[setup](r)
    xr = x.to(dtype).clone().requires_grad_(True)
    ctx = torch.autocast("cpu", dtype=amp) if amp is not None else contextlib.nullcontext()
    with ctx:
        lo = r(xr)
    O.total_loss(lo.to(dtype), y.to(dtype)).backward()
    return xr.grad.detach(), {k: p.grad for k, p in r.named_parameters()}


@pytest.mark.parametrize("setup", list(SETUPS))
def test_x_grad_vs_oracle(setup):
    """x.grad against the oracle's (float64 arbiter; bar max(1e-3, 3 x the fp32 oracle's own relative L2)); frozen parameters keep
    grad None; x.grad accumulates over two backwards; dtype and shape follow x (a float64 x gets a float64 x.grad)."""
    O = _O()
    n, s = 2, 64
    ref = warm_oracle(n, s)
    x, y = O.synthetic_batch(n, s, seed=4321)
    gx64, _ = _oracle_xgrad(ref, setup, x, y, torch.float64)
    gx32, gp32 = _oracle_xgrad(ref, setup, x, y, torch.float32)
    m = vk.Unet(encoder_name="resnet34", encoder_weights=None, in_channels=3, classes=1, activation=None).to(dev())
    m.load_state_dict(ref.state_dict())
    SETUPS[setup](m)
    x_dtype = torch.float64 if setup == "saliency" else torch.float32
    xd = x.to(dev(), x_dtype).requires_grad_(True)
    yd = y.to(dev())
    firsts = []
    for k in range(2):
        lg = m(xd)
        O.total_loss(lg, yd).backward()
        torch.cuda.synchronize()
        assert xd.grad is not None and xd.grad.shape == xd.shape and xd.grad.dtype == x_dtype
        firsts.append(xd.grad.clone())
    g1 = firsts[0]
    e, e_ref = rel(g1.cpu(), gx64), rel(gx32, gx64)
    print(f"\n[x.grad {setup}] engine rel L2 {e:.3e}, fp32 oracle {e_ref:.3e}")
    assert e <= max(1e-3, 3 * e_ref), (setup, e, e_ref)
    if setup != "saliency":
        # the second forward of a train-mode layer uses the batch statistics again: the same gradient, added
        assert rel(firsts[1].cpu(), 2 * g1.cpu()) <= 1e-6
    else:
        # eval mode everywhere, nothing trainable: the second backward adds the same bits
        assert torch.equal(firsts[1], 2 * g1)
    for name, p in m.named_parameters():
        if gp32[name] is None:
            assert p.grad is None, name
        else:
            assert p.grad is not None, name


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("setup", ["saliency", "train_all"])
def test_x_grad_16bit_vs_yardstick(setup, dtype):
    """Under autocast: x.grad (fp32, as x) against float64; yardstick: the oracle under CPU autocast.  Bar: relative L2 <= 1.5 x the
    yardstick's + 0.02 (floor: the engine stores every activation and gradient in 16 bits, CPU autocast keeps BatchNorm in fp32)."""
    O = _O()
    n, s = 2, 64
    ref = warm_oracle(n, s)
    x, y = O.synthetic_batch(n, s, seed=4322)
    gx64, _ = _oracle_xgrad(ref, setup, x, y, torch.float64)
    gxy, _ = _oracle_xgrad(ref, setup, x, y, torch.float32, amp=dtype)
    m = vk.Unet(encoder_name="resnet34", encoder_weights=None, in_channels=3, classes=1, activation=None).to(dev())
    m.load_state_dict(ref.state_dict())
    SETUPS[setup](m)
    xd = x.to(dev()).requires_grad_(True)
    with torch.autocast("cuda", dtype=dtype):
        lg = m(xd)
    O.total_loss(lg.float(), y.to(dev())).backward()
    torch.cuda.synchronize()
    assert xd.grad.dtype == torch.float32 and torch.isfinite(xd.grad).all()
    e, e_y = rel(xd.grad.cpu(), gx64), rel(gxy, gx64)
    print(f"\n[x.grad {setup} {dtype}] engine rel L2 {e:.3e}, yardstick {e_y:.3e}")
    assert e <= 1.5 * e_y + 0.02, (e, e_y)
