"""Unet(classes=C) on the MI355X (-m gpu): the 16 -> C head kernels and the two loss kernels through the C ABI against float64
references, the whole model against OracleUnet(classes=C), the fused step against the autograd path, determinism, fine-tuning with a
frozen encoder, the fp16 GradScaler protocol, checkpoints, and the binary model's launches staying what they were."""
import copy
import ctypes as C
import importlib

import pytest
import torch
import torch.nn.functional as F

import multiclass_ref as R

pytestmark = pytest.mark.gpu
vk = importlib.import_module("vickers-hardness-unet_amd")
L_ = vk._lib
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
REPL = 32       # VK_STATS_REPLICAS in include/vk_unet.h
K_ARBITER = 4.0  # engine-vs-float64 error <= K_ARBITER x (fp32 oracle-vs-float64 error), fixed before the first run


def dev():
    return torch.device("cuda:0")


def st():
    return torch.cuda.current_stream().cuda_stream


def _O():
    from oracle import unet_oracle as O
    return O


def _tol(dt, ref):
    return {torch.float32: 2e-5, torch.bfloat16: 1.2e-2, torch.float16: 1.5e-3}[dt] * (ref.abs().max().item() + 1e-6)


# ------------------------------------------------------------------------------------------------ head kernels
@pytest.mark.parametrize("fused", [True, False], ids=["bnr", "plain"])
@pytest.mark.parametrize("shape", [(1, 40, 33), (3, 16, 48)], ids=["ragged", "wide"])
@pytest.mark.parametrize("dtn", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("Cc", [2, 3, 4, 8, 16])
def test_head_multi_fwd_bwd(Cc, dtn, shape, fused):
    dt = DT[dtn]
    N, H, W = shape
    g = torch.Generator().manual_seed(300 + Cc)
    z = (torch.randn(N, 16, H, W, generator=g)).to(dt).float()
    sc, sh = torch.rand(16, generator=g) + 0.5, torch.randn(16, generator=g) * 0.3
    w = torch.randn(Cc, 16, 3, 3, generator=g) * 0.2
    b = torch.randn(Cc, generator=g)
    dl = torch.randn(N, Cc, H, W, generator=g)
    pre = z * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)
    a = torch.relu(pre).double().requires_grad_(True)
    wv, bv = w.double().requires_grad_(True), b.double().requires_grad_(True)
    ref = F.conv2d(a, wv, bv, padding=1)
    ref.backward(dl.double())
    zd = z.permute(0, 2, 3, 1).contiguous().to(dt).to(dev())
    scd, shd = sc.to(dev()), sh.to(dev())
    wk = w.permute(0, 2, 3, 1).contiguous().to(dev())           # KRSC [C][3][3][16]
    bd, dld = b.to(dev()), dl.to(dev())
    src = L_.vk_src(zd.data_ptr(), 16, 0, scd.data_ptr(), shd.data_ptr(), 1)
    L = vk.lib()
    logits = torch.full((N, Cc, H, W), 7.0, device=dev())
    L_.check(L.vk_head_fwd_multi(L_.dtype_code(dt), N, H, W, Cc, C.byref(src), wk.data_ptr(), bd.data_ptr(), logits.data_ptr(), st()))
    torch.cuda.synchronize()
    assert (logits.cpu() - ref.detach().float()).abs().max().item() <= 1e-4 * ref.abs().max().item()
    gy = a.grad.float()
    if fused:
        gy = gy.to(dt).float() * (pre > 0)                        # stored gradient: rounded, then masked
    ws = torch.empty(L.vk_head_multi_workspace_bytes(Cc), dtype=torch.uint8, device=dev())
    outs = []
    for rep in range(2):
        dy = torch.full((N, H, W, 16), 7.0, dtype=dt, device=dev())
        dw = torch.zeros(Cc, 3, 3, 16, device=dev())
        db = torch.zeros(Cc, device=dev())
        sums = torch.zeros(REPL * 32, dtype=torch.float64, device=dev())
        bnr = L_.vk_bnr(zd.data_ptr(), scd.data_ptr(), shd.data_ptr(), sums.data_ptr())
        L_.check(L.vk_head_bwd_multi(L_.dtype_code(dt), N, H, W, Cc, C.byref(src), wk.data_ptr(), dld.data_ptr(), dy.data_ptr(),
                                     dw.data_ptr(), db.data_ptr(), C.byref(bnr) if fused else None, ws.data_ptr(), ws.numel(), st()))
        torch.cuda.synchronize()
        got = dy.cpu().permute(0, 3, 1, 2).float()
        assert (got - gy).abs().max().item() <= _tol(dt, gy) + 1e-7
        if fused:
            ss = sums.view(REPL, 2, 16).sum(0).cpu()
            s1 = gy.double().sum(dim=(0, 2, 3))
            s2 = (gy.double() * z.double()).sum(dim=(0, 2, 3))
            k = 1.0 if dt != torch.float32 else 1e-3
            assert (ss[0] - s1).abs().max().item() <= 2e-2 * gy.abs().max().item() * (N * H * W) ** 0.5 * k
            assert (ss[1] - s2).abs().max().item() <= 2e-2 * (gy.abs().max() * z.abs().max()).item() * (N * H * W) ** 0.5 * k
        assert (dw.cpu().permute(0, 3, 1, 2) - wv.grad.float()).abs().max().item() <= 1e-3 * wv.grad.abs().max().item()
        assert (db.cpu().double() - bv.grad).abs().max().item() <= 1e-3 * bv.grad.abs().max().item() + 1e-3
        outs.append((dy, dw, db))
    assert all(torch.equal(p, q) for p, q in zip(outs[0], outs[1]))       # reproducible: the same bits twice


# ------------------------------------------------------------------------------------------------ loss kernels
def _loss_call(multiclass, x, y, grad_scale, w_pix=1.0, w_dice=1.0):
    L = vk.lib()
    N, Cc, H, W = x.shape
    ws = torch.empty(L.vk_multi_loss_workspace_bytes(N, Cc, H * W), dtype=torch.uint8, device=dev())
    out = torch.full((4,), 5.0, device=dev())
    dl = torch.empty_like(x)
    fn = L.vk_multiclass_loss if multiclass else L.vk_multilabel_loss
    L_.check(fn(N, Cc, H * W, x.data_ptr(), y.data_ptr(), ws.data_ptr(), ws.numel(), out.data_ptr(), dl.data_ptr(), grad_scale,
                w_pix, w_dice, st()))
    torch.cuda.synchronize()
    return out.cpu(), dl.cpu()


@pytest.mark.parametrize("weights", [(1.0, 1.0), (0.0, 1.0), (1.0, 0.0)])
@pytest.mark.parametrize("Cc", [1, 2, 4, 16])
def test_multilabel_loss_kernel(Cc, weights):
    g = torch.Generator().manual_seed(400 + Cc)
    x = torch.randn(3, Cc, 40, 56, generator=g) * 3
    y = (torch.rand(3, Cc, 40, 56, generator=g) > 0.7).float()
    if Cc > 1:
        y[:, 1] = 0                                              # a class absent from the batch: Dice mask 0
    tot, b, d, dl = R.multilabel(x, y, *weights)
    for gs in (1.0, 1024.0):
        out, got = _loss_call(False, x.to(dev()), y.to(dev()), gs, *weights)
        assert abs(out[0].item() - tot.item()) <= 1e-5 * abs(tot.item()) + 1e-6
        assert abs(out[1].item() - b.item()) <= 1e-5 * abs(b.item()) + 1e-6
        assert abs(out[2].item() - d.item()) <= 1e-5 * abs(d.item()) + 1e-6
        assert out[3].item() == 0.0
        assert (got.double() - gs * dl).abs().max().item() <= 1e-4 * gs * dl.abs().max().item()
    out2, got2 = _loss_call(False, x.to(dev()), y.to(dev()), 1024.0, *weights)
    assert torch.equal(out, out2) and torch.equal(got, got2)


@pytest.mark.parametrize("weights", [(1.0, 1.0), (0.0, 1.0), (1.0, 0.0)])
@pytest.mark.parametrize("Cc", [2, 3, 5, 16])
def test_multiclass_loss_kernel(Cc, weights):
    g = torch.Generator().manual_seed(500 + Cc)
    x = torch.randn(3, Cc, 40, 56, generator=g) * 3
    t = torch.randint(0, Cc, (3, 40, 56), generator=g)
    t[t == Cc - 1] = 0                                           # the last class is absent
    tot, ce, d, dl = R.multiclass(x, t, *weights)
    for gs in (1.0, 1024.0):
        out, got = _loss_call(True, x.to(dev()), t.to(dev()), gs, *weights)
        assert abs(out[0].item() - tot.item()) <= 1e-5 * abs(tot.item()) + 1e-6
        assert abs(out[1].item() - ce.item()) <= 1e-5 * abs(ce.item()) + 1e-6
        assert abs(out[2].item() - d.item()) <= 1e-5 * abs(d.item()) + 1e-6
        assert out[3].item() == 0.0
        assert (got.double() - gs * dl).abs().max().item() <= 1e-4 * gs * dl.abs().max().item()
    out2, got2 = _loss_call(True, x.to(dev()), t.to(dev()), 1024.0, *weights)
    assert torch.equal(out, out2) and torch.equal(got, got2)


def test_multiclass_bad_label_is_reported_not_faulting():
    g = torch.Generator().manual_seed(77)
    x = torch.randn(2, 3, 32, 32, generator=g)
    t = torch.randint(0, 3, (2, 32, 32), generator=g)
    t[0, 3, 4], t[1, 0, 0], t[1, 31, 31] = 3, -1, 1000
    out, dl = _loss_call(True, x.to(dev()), t.to(dev()), 1.0)
    assert out[3].item() == 3.0 and torch.isnan(out[:3]).all()
    assert dl[0, :, 3, 4].abs().max().item() == 0.0 and torch.isfinite(dl).all()
    with pytest.raises(vk.VkError, match="outside"):
        vk.multiclass.DiceLoss(mode="multiclass")(x.to(dev()).requires_grad_(True), t.to(dev()))
    torch.cuda.synchronize()                                     # the device is fine afterwards
    assert torch.isfinite(torch.ones(4, device=dev()).sum()).item()


# ------------------------------------------------------------------------------------------------ the model
def _targets(Cc, N, S, seed):
    g = torch.Generator().manual_seed(seed)
    y = (torch.rand(N, Cc, S, S, generator=g) > 0.5).float()
    y[:, :, : S // 4] = 0
    t = torch.randint(0, Cc, (N, S, S), generator=g)
    return y, t


def _torch_loss(mode, lg, y, t, dice_mod):
    if mode == "multilabel":
        return F.binary_cross_entropy_with_logits(lg, y) + dice_mod(lg, y)
    return F.cross_entropy(lg, t) + dice_mod(lg, t)


def _smp_dice(mode):
    def f(lg, target):
        Cc = lg.shape[1]
        p = torch.sigmoid(lg) if mode == "multilabel" else lg.softmax(dim=1)
        oh = target if mode == "multilabel" else F.one_hot(target, Cc).permute(0, 3, 1, 2).to(lg.dtype)
        N = lg.shape[0]
        p, oh = p.reshape(N, Cc, -1), oh.reshape(N, Cc, -1)
        inter, card = (p * oh).sum(dim=(0, 2)), (p + oh).sum(dim=(0, 2))
        return ((1 - 2 * inter / card.clamp_min(1e-7)) * (oh.sum(dim=(0, 2)) > 0).to(lg.dtype)).mean()
    return f


def _pair(Cc):
    O = _O()
    O.set_seed(42)
    ref = O.OracleUnet(classes=Cc)
    O.set_seed(42)
    m = vk.multiclass.Unet(encoder_weights=None, classes=Cc).to(dev())
    return O, ref, m


@pytest.mark.parametrize("mode", ["multilabel", "multiclass"])
@pytest.mark.parametrize("Cc", [3, 8])
def test_model_fp32_against_oracle_with_float64_arbiter(Cc, mode):
    O, ref, m = _pair(Cc)
    N, S = 8, 64                                                 # the size of the binary model's arbiter test
    x, _ = O.synthetic_batch(N, S, seed=1234)
    y, t = _targets(Cc, N, S, 99)
    ref.train(); m.train()
    ref64 = copy.deepcopy(ref).double()
    lr = ref(x)
    l32 = _torch_loss(mode, lr, y, t, _smp_dice(mode))
    l32.backward()
    lg = m(x.to(dev()))
    assert lg.shape == (N, Cc, S, S) and lg.dtype == torch.float32
    loss = _torch_loss(mode, lg, y.to(dev()), t.to(dev()), vk.multiclass.DiceLoss(mode=mode))
    loss.backward()
    torch.cuda.synchronize()
    l64 = _torch_loss(mode, ref64(x.double()), y.double(), t, _smp_dice(mode))
    l64.backward()
    assert (lg.detach().cpu() - lr.detach()).abs().max().item() <= 1e-3 * lr.abs().max().item()
    assert abs(loss.item() - l64.item()) <= 1e-4 * abs(l64.item())
    n32, n64 = dict(ref.named_parameters()), dict(ref64.named_parameters())
    e64 = max(((p.grad.cpu().double() - n64[k].grad).norm() / (n64[k].grad.norm() + 1e-30)).item() for k, p in m.named_parameters())
    o64 = max(((n32[k].grad.double() - n64[k].grad).norm() / (n64[k].grad.norm() + 1e-30)).item() for k in n32)
    print(f"C={Cc} {mode}: relative L2 gradient error against float64: engine {e64:.2e}, fp32 oracle {o64:.2e}")
    assert e64 <= K_ARBITER * o64, (e64, o64)


@pytest.mark.parametrize("mode", ["multilabel", "multiclass"])
@pytest.mark.parametrize("Cc", [3, 8])
def test_model_bf16_autocast_against_oracle(Cc, mode):
    """The bars of the binary model's bf16 test (test_bf16_training_step_tracks_reference_mixed_precision): the oracle's own CPU
    autocast run is the yardstick — logits within 1.5x of its deviation from fp32, the loss within 1 %, per-tensor gradient cosine
    against fp32 of the decoder and head no more than 0.05 below the autocast oracle's."""
    O = _O()
    N, S = 4, 64
    x, _ = O.synthetic_batch(N, S, seed=1234)
    y, t = _targets(Cc, N, S, 98)

    def run_oracle(autocast):
        O.set_seed(42)
        ref = O.OracleUnet(classes=Cc).train()
        with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
            lo = ref(x)
        loss = _torch_loss(mode, lo.float(), y, t, _smp_dice(mode))
        loss.backward()
        return lo.detach().float(), loss.item(), {k: p.grad.clone() for k, p in ref.named_parameters()}

    l32, loss32, g32 = run_oracle(False)
    l16, _, g16 = run_oracle(True)
    O.set_seed(42)
    m = vk.multiclass.Unet(encoder_weights=None, classes=Cc).to(dev()).train()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        lg = m(x.to(dev()))
    assert lg.dtype == torch.float32 and lg.shape == (N, Cc, S, S)
    loss = _torch_loss(mode, lg, y.to(dev()), t.to(dev()), vk.multiclass.DiceLoss(mode=mode))
    loss.backward()
    torch.cuda.synchronize()
    assert loss.item() == pytest.approx(loss32, rel=1e-2)
    ours, theirs = (lg.detach().cpu() - l32).abs().mean().item(), (l16 - l32).abs().mean().item()
    print(f"C={Cc} {mode} bf16: mean |logit error| {ours:.3e}, autocast oracle {theirs:.3e}")
    assert ours <= 1.5 * theirs + 1e-3, (ours, theirs)

    def cos(a, b):
        a, b = a.flatten().double(), b.flatten().double()
        return (a @ b / (a.norm() * b.norm() + 1e-30)).item()

    # the decoder and the head: what the head's gradient reaches first.  In the encoder both runs are dominated by bf16 round-off through
    # the BatchNorm chain at random init (stem: cosine 0.63 here against the autocast oracle's 0.68 in one case), not by the head
    for k, p in m.named_parameters():
        if p.numel() < 1024 or k.startswith("encoder."):
            continue
        c_ours, c_ref = cos(p.grad.cpu(), g32[k]), cos(g16[k], g32[k])
        assert c_ours >= c_ref - 0.05, f"{k}: cosine {c_ours} vs autocast oracle {c_ref}"


def _flat_grads(m):
    return m.flat_grads.detach().clone()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("mode", ["multilabel", "multiclass"])
def test_loss_and_backward_equals_autograd(mode, dtype):
    Cc = 4
    O = _O()
    O.set_seed(42)
    m = vk.multiclass.Unet(encoder_weights=None, classes=Cc).to(dev())
    x, _ = O.synthetic_batch(2, 64, seed=1234)
    x = x.to(dev())
    y, t = _targets(Cc, 2, 64, 97)
    tgt = (y if mode == "multilabel" else t).to(dev())
    fused = vk.multiclass.BCEDiceLoss(mode="multilabel") if mode == "multilabel" else vk.multiclass.CEDiceLoss()
    m.train()
    sd = copy.deepcopy(m.state_dict())
    ptrs = set()                       # where the fused steps put their results: one buffer of the plan, not one per call

    def autograd(loss_fn, scale=1.0):
        m.load_state_dict(sd)
        m.zero_grad(set_to_none=True)
        ctx = torch.autocast("cuda", dtype=dtype) if dtype != torch.float32 else torch.autocast("cuda", enabled=False)
        with ctx:
            lg = m(x)
        loss = loss_fn(lg.float(), tgt)
        (loss * scale).backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), _flat_grads(m)

    def fused_step(scale=1.0):
        m.load_state_dict(sd)
        m.zero_grad(set_to_none=True)
        out = m.loss_and_backward(x, tgt, grad_scale=scale, dtype=dtype, mode=mode)
        torch.cuda.synchronize()
        ptrs.add(out.data_ptr())
        return out.clone(), _flat_grads(m)

    l_vk, g_vk = autograd(fused)
    l_f, g_f = fused_step()
    assert torch.equal(l_f[0], l_vk) and torch.equal(g_f, g_vk)            # same kernels, same bits
    assert tuple(m.last_logits.shape) == (2, Cc, 64, 64)
    l_t, g_t = autograd(lambda lg, tg: _torch_loss(mode, lg, tg if mode == "multilabel" else None,
                                                   tg if mode == "multiclass" else None, vk.multiclass.DiceLoss(mode=mode)))
    assert abs(l_t.item() - l_f[0].item()) <= 1e-5 * abs(l_f[0].item())
    # torch's CE / BCE gradient and the kernel's differ by fp32 round-off; the head gradient sees that directly, the layers behind it
    # through 16-bit data gradients whose roundings it can flip (amplified by the train-mode BatchNorm chain)
    h0, h1 = m._param_ranges[-2][0], m._param_ranges[-1][0] + m._param_ranges[-1][1]
    assert ((g_t[h0:h1] - g_f[h0:h1]).norm() / g_f[h0:h1].norm()).item() <= 1e-5
    assert ((g_t - g_f).norm() / g_f.norm()).item() <= (1e-3 if dtype == torch.float32 else 3e-2)
    _, g_s = fused_step(scale=256.0)
    _, g_as = autograd(fused, scale=256.0)
    assert torch.equal(g_s, g_as)
    assert ((g_s - 256.0 * g_f).norm() / (256.0 * g_f).norm()).item() <= 1e-5
    assert len(ptrs) == 1
    with pytest.raises(ValueError, match="multilabel"):
        m.loss_and_backward(x, tgt, dtype=dtype)                           # classes > 1 and no mode


@pytest.mark.parametrize("mode", ["multilabel", "multiclass"])
def test_two_seeded_steps_are_bit_identical(mode):
    O = _O()
    Cc = 3
    x, _ = O.synthetic_batch(2, 64, seed=1234)
    y, t = _targets(Cc, 2, 64, 96)
    tgt = (y if mode == "multilabel" else t).to(dev())
    runs = []
    for _ in range(2):
        O.set_seed(42)
        m = vk.multiclass.Unet(encoder_weights=None, classes=Cc).to(dev()).train()
        opt = vk.adamw_for(m, lr=5e-4, weight_decay=1e-4)
        for _ in range(2):
            opt.zero_grad(set_to_none=True)
            m.loss_and_backward(x.to(dev()), tgt, dtype=torch.bfloat16, mode=mode)
            opt.step()
        torch.cuda.synchronize()
        runs.append(m.flat_params.detach().clone())
    assert torch.equal(runs[0], runs[1])


def test_frozen_encoder_multiclass_head():
    O = _O()
    Cc = 4
    x, _ = O.synthetic_batch(2, 64, seed=1234)
    _, t = _targets(Cc, 2, 64, 95)
    O.set_seed(42)
    m = vk.multiclass.Unet(encoder_weights=None, classes=Cc).to(dev()).train()
    m.encoder.eval()
    m.zero_grad(set_to_none=True)
    m.loss_and_backward(x.to(dev()), t.to(dev()), mode="multiclass")
    full = _flat_grads(m)
    for p in m.encoder.parameters():
        p.requires_grad_(False)
    m.zero_grad(set_to_none=True)
    m.loss_and_backward(x.to(dev()), t.to(dev()), mode="multiclass")
    torch.cuda.synchronize()
    part = _flat_grads(m)
    for (name, p), (off, numel) in zip(m.named_parameters(), m._param_ranges):
        if name.startswith("encoder."):
            assert p.grad is None and part[off:off + numel].abs().max().item() == 0.0, name
        else:
            ref = full[off:off + numel]
            assert (part[off:off + numel] - ref).abs().max().item() <= 1e-5 * ref.abs().max().item() + 1e-12, name


def test_fp16_gradscaler_skip_and_step():
    O = _O()
    Cc = 3
    x, _ = O.synthetic_batch(2, 64, seed=1234)
    y, _ = _targets(Cc, 2, 64, 94)
    O.set_seed(42)
    m = vk.multiclass.Unet(encoder_weights=None, classes=Cc).to(dev()).train()
    opt = vk.adamw_for(m, lr=5e-5, weight_decay=1e-4)
    scaler = vk.GradScaler("cuda", init_scale=2.0 ** 60)        # step 0: forced overflow, the fp16 gradients are inf
    loss_fn = vk.multiclass.BCEDiceLoss(mode="multilabel")
    for step in range(2):
        if step == 1:
            scaler.update(new_scale=2.0 ** 10)
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.float16):
            lg = m(x.to(dev()))
        loss = loss_fn(lg.float(), y.to(dev()))
        scaler.scale(loss).backward()
        finite = all(torch.isfinite(p.grad).all().item() for p in m.parameters())
        before = m.flat_params.detach().clone()
        scaler.step(opt)
        scaler.update()
        torch.cuda.synchronize()
        assert finite == (step == 1)
        moved = not torch.equal(before, m.flat_params)
        assert moved == (step == 1), step
    assert opt.step_count == 1


def test_checkpoint_round_trip_with_oracle():
    O = _O()
    O.set_seed(7)
    ref = O.OracleUnet(classes=3)
    m = vk.multiclass.Unet(encoder_weights=None, classes=3).to(dev())
    m.load_state_dict(ref.state_dict(), strict=True)
    sd = m.state_dict()
    for k, v in ref.state_dict().items():
        assert torch.equal(sd[k].cpu(), v), k
    ref2 = O.OracleUnet(classes=3)
    ref2.load_state_dict({k: v.cpu() for k, v in sd.items()}, strict=True)
    for k, v in ref.state_dict().items():
        assert torch.equal(ref2.state_dict()[k], v), k
    ref.eval(); m.eval()
    x, _ = O.synthetic_batch(1, 64, seed=3)
    with torch.no_grad():
        a, b = ref(x), m(x.to(dev())).cpu()
    assert (a - b).abs().max().item() <= 1e-3 * a.abs().max().item()


def test_binary_to_multiclass_transfer():
    O = _O()
    O.set_seed(1)
    binary = vk.Unet(encoder_weights=None, classes=1)
    sd = {k: v for k, v in binary.state_dict().items() if not k.startswith("segmentation_head.")}
    O.set_seed(2)
    m = vk.multiclass.Unet(encoder_weights=None, classes=4).to(dev())
    head = m.state_dict()["segmentation_head.0.weight"].clone()
    res = m.load_state_dict(sd, strict=False)
    assert sorted(res.missing_keys) == ["segmentation_head.0.bias", "segmentation_head.0.weight"] and not res.unexpected_keys
    got = m.state_dict()
    for k, v in sd.items():
        assert torch.equal(got[k].cpu(), v), k
    assert torch.equal(m.state_dict()["segmentation_head.0.weight"], head)
    x, _ = O.synthetic_batch(2, 64, seed=3)
    _, t = _targets(4, 2, 64, 93)
    out = m.train().loss_and_backward(x.to(dev()), t.to(dev()), mode="multiclass")
    assert torch.isfinite(out).all()


def _families(fn):
    L = vk.lib()
    torch.cuda.synchronize()
    vk._lib.prof_collect()
    L.vk_prof_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        L.vk_prof_enable(0)
    return vk._lib.prof_collect()


NEW_TAGS = {"head_fwd_multi", "head_bwd_multi", "multilabel_loss", "multiclass_loss"}


def test_binary_launches_unchanged_and_multi_launches_tagged():
    O = _O()
    x, y = O.synthetic_batch(2, 64, seed=1234)
    x, y = x.to(dev()), y.to(dev())
    O.set_seed(42)
    m = vk.Unet(encoder_weights=None).to(dev()).train()

    def binary_step():
        for _ in range(2):
            m.zero_grad(set_to_none=True)
            m.loss_and_backward(x, y, dtype=torch.bfloat16)
            m.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                lg = m(x)
            (F.binary_cross_entropy_with_logits(lg, y) + vk.DiceLoss(mode="binary")(lg, y)).backward()
            m.eval()
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                m(x)
            m.train()
    fam = _families(binary_step)
    assert {"head_fwd", "head_bwd_mfma", "bce_dice_loss"} <= set(fam), sorted(fam)
    assert not (NEW_TAGS & set(fam)), sorted(fam)
    O.set_seed(42)
    m3 = vk.multiclass.Unet(encoder_weights=None, classes=3).to(dev()).train()
    _, t = _targets(3, 2, 64, 92)
    fam3 = _families(lambda: m3.loss_and_backward(x, t.to(dev()), dtype=torch.bfloat16, mode="multiclass"))
    assert {"head_fwd_multi", "head_bwd_multi", "multiclass_loss"} <= set(fam3), sorted(fam3)
    assert not ({"head_fwd", "head_bwd_mfma", "head_dgrad", "head_wgrad", "bce_dice_loss"} & set(fam3)), sorted(fam3)
