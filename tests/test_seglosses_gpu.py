"""vk.seglosses on the MI355X (-m gpu): the vk_seg_loss kernels through the C ABI against the float64 closed form of
tests/seglosses_ref.py over the covering set of tests/seglosses_cases.py, the edge cases (everything ignored, empty classes, extreme
logits, bad labels), agreement with the existing losses, the autograd modules, the fused step, the launch families and seg_metrics
with ignore_index.

Bars (the project's own for the same kind of kernel, tests/test_multiclass_gpu.py): every loss_out component within
1e-5 |ref| + 1e-6, dlogits within 1e-4 grad_scale max|ref|, a second call bit-identical."""
import copy
import importlib

import numpy as np
import pytest
import torch

import multiclass_eval_ref as ER
import seglosses_cases as K
import seglosses_ref as R

pytestmark = pytest.mark.gpu
vk = importlib.import_module("vickers-hardness-unet_amd")
Ls = vk.seglosses
L_ = vk._lib


def dev():
    return torch.device("cuda:0")


def _O():
    from oracle import unet_oracle as O
    return O


def _call(cfg, x, tgt, grad_scale=1.0, grad=True):
    """vk_seg_loss on device copies of x / tgt -> (loss_out[8], dlogits) on the host"""
    L = vk.lib()
    N, Cc, H, W = x.shape
    xd = x.to(dev()).contiguous()
    td = (tgt.to(dev()).float().expand_as(xd) if cfg.mode != L_.VK_LOSS_MULTICLASS else tgt.to(dev())).contiguous()
    ws = torch.empty(L.vk_seg_loss_workspace_bytes(N, Cc, H * W), dtype=torch.uint8, device=dev())
    out = torch.full((8,), 5.0, device=dev())
    dl = torch.full_like(xd, 7.0) if grad else None
    L_.check(L.vk_seg_loss(cfg, N, Cc, H * W, xd.data_ptr(), td.data_ptr(), ws.data_ptr(), ws.numel(), out.data_ptr(), L_.ptr(dl),
                           grad_scale, torch.cuda.current_stream().cuda_stream), "vk_seg_loss")
    torch.cuda.synchronize()
    return out.cpu(), (dl.cpu() if grad else None)


def _dead(mode, x, tgt):
    d = tgt == K.IGN
    return d.unsqueeze(1).expand_as(x) if mode == "multiclass" else d.expand_as(x)


def _check(tag, cfg, spec, mode, x, tgt, scales=(1.0, 1024.0)):
    rf = R.evaluate(x, tgt, spec)
    want = R.components(rf)
    ref_g = rf["dlogits"]
    gmax = ref_g.abs().max().item()
    last = None
    for gs in scales:
        out, dl = _call(cfg, x, tgt, gs)
        verr = (out[:6].double() - want).abs()
        vbar = 1e-5 * want.abs() + 1e-6
        gerr = (dl.double() - gs * ref_g).abs().max().item()
        print("%s gs=%g: worst value error %.3g of its bar, gradient error %.3g of its bar (max|ref grad| %.3g)"
              % (tag, gs, (verr / vbar).max().item(), gerr / (1e-4 * gs * gmax) if gmax > 0 else 0.0, gmax))
        assert (verr <= vbar).all(), (out[:6].tolist(), want.tolist())
        assert out[6].item() == 0.0 and out[7].item() == 0.0
        assert gerr <= 1e-4 * gs * gmax, (gerr, gmax)
        if spec["ignore_index"] is not None:
            dead = _dead(mode, x, tgt)
            assert (dl[dead] == 0).all()                  # exactly zero, whatever grad_scale
        last = (gs, out, dl)
    gs, out, dl = last
    out2, dl2 = _call(cfg, x, tgt, gs)
    assert torch.equal(out, out2) and torch.equal(dl, dl2)
    out3, none = _call(cfg, x, tgt, gs, grad=False)       # no gradient asked for: the same values
    assert torch.equal(out, out3) and none is None


# ------------------------------------------------------------------------------------------ (1) each kind alone and the five-term sum
@pytest.mark.parametrize("si", [0, 1], ids=["vec", "scalar"])
@pytest.mark.parametrize("name", K.case_names())
@pytest.mark.parametrize("mode,Cc", K.MODE_C)
def test_kernels_against_float64(mode, Cc, name, si):
    N, H, W = K.SHAPES[si]
    ign = K.ignored(name, si)
    x, tgt = K.make_inputs(mode, Cc, N, H, W, ign)
    S = K.build(Ls, name, mode, Cc, ign)._as_sum()
    _check("%s C=%d %s %dx%d" % (mode, Cc, name, H, W), S.cfg(Cc), S.spec(Cc), mode, x, tgt)


# ------------------------------------------------------------------------------------------ (2) edge cases
@pytest.mark.parametrize("mode,Cc", [("binary", 1), ("multilabel", 4), ("multiclass", 3), ("multiclass", 16)])
def test_one_image_ignored(mode, Cc):
    for si, (N, H, W) in enumerate(K.SHAPES):
        x, tgt = K.make_inputs(mode, Cc, N, H, W, True)
        tgt[0] = K.IGN
        S = K.build(Ls, "sum5", mode, Cc, True)
        _check("%s C=%d image 0 ignored" % (mode, Cc), S.cfg(Cc), S.spec(Cc), mode, x, tgt, scales=(1.0,))


@pytest.mark.parametrize("mode,Cc", [("binary", 1), ("multilabel", 4), ("multiclass", 3), ("multiclass", 16)])
def test_whole_batch_ignored(mode, Cc):
    """every denominator is empty: every term is 0 (documented; torch and smp give NaN), every gradient 0, nothing NaN"""
    for si, (N, H, W) in enumerate(K.SHAPES):
        x, tgt = K.make_inputs(mode, Cc, N, H, W, True)
        tgt = torch.full_like(tgt, K.IGN)
        for name in K.case_names():
            S = K.build(Ls, name, mode, Cc, True)._as_sum()
            out, dl = _call(S.cfg(Cc), x, tgt, 1024.0)
            assert (out == 0).all(), (name, out.tolist())
            assert (dl == 0).all(), name


@pytest.mark.parametrize("mode,Cc", [("binary", 1), ("multilabel", 4), ("multiclass", 3)])
def test_all_background_target(mode, Cc):
    """sigmoid modes: every T_c = 0, so every region term is 0 with a zero gradient; multiclass: only class 0 is present"""
    N, H, W = K.SHAPES[0]
    x, tgt = K.make_inputs(mode, Cc, N, H, W, False)
    tgt = torch.zeros_like(tgt)
    for name in ("dice", "dice_opts", "jaccard", "tversky", "tversky_log", "sum5"):
        S = K.build(Ls, name, mode, Cc, False)._as_sum()
        _check("%s C=%d %s background" % (mode, Cc, name), S.cfg(Cc), S.spec(Cc), mode, x, tgt, scales=(1.0,))
        if mode != "multiclass" and name != "sum5":
            out, dl = _call(S.cfg(Cc), x, tgt)
            assert (out[:6] == 0).all() and (dl == 0).all()


@pytest.mark.parametrize("mode,Cc", [("binary", 1), ("multilabel", 4), ("multiclass", 3), ("multiclass", 16)])
def test_extreme_logits_stay_finite(mode, Cc):
    for si, (N, H, W) in enumerate(K.SHAPES):
        x, tgt = K.make_inputs(mode, Cc, N, H, W, True)
        flat = x.view(-1)
        for i, v in enumerate((30.0, -30.0, 88.0, -88.0)):
            flat[i::97] = v                                # planted against foreground, background and ignored entries alike
        for name in K.case_names():
            S = K.build(Ls, name, mode, Cc, True)._as_sum()
            out, dl = _call(S.cfg(Cc), x, tgt, 1024.0)
            assert torch.isfinite(out).all() and torch.isfinite(dl).all(), name
            rf = R.evaluate(x, tgt, S.spec(Cc))
            print("%s C=%d %s: total %.6g (float64 %.6g), max gradient error %.3g of max|ref| %.3g" % (
                mode, Cc, name, out[0].item(), float(rf["total"]),
                (dl.double() / 1024.0 - rf["dlogits"]).abs().max().item(), rf["dlogits"].abs().max().item()))


def test_bad_label_is_reported_not_faulting():
    """a label that is neither a class nor ignore_index, beside valid ignore labels: an argument error, counted exactly"""
    g = torch.Generator().manual_seed(77)
    x = torch.randn(2, 3, 32, 32, generator=g)
    t = torch.randint(0, 3, (2, 32, 32), generator=g)
    t[0, :4] = K.IGN
    t[0, 5, 4], t[1, 0, 0], t[1, 31, 31] = 3, -1, 1000
    S = K.build(Ls, "sum5", "multiclass", 3, True)
    out, dl = _call(S.cfg(3), x, t)
    assert out[6].item() == 3.0 and torch.isnan(out[:6]).all() and out[7].item() == 0.0
    assert torch.isfinite(dl).all()
    for n, i, j in ((0, 5, 4), (1, 0, 0), (1, 31, 31), (0, 0, 0)):
        assert dl[n, :, i, j].abs().max().item() == 0.0
    with pytest.raises(vk.VkError, match="3 label"):
        S(x.to(dev()).requires_grad_(True), t.to(dev()))
    torch.cuda.synchronize()                                     # the device is fine afterwards
    assert torch.isfinite(torch.ones(4, device=dev()).sum()).item()
    t[t > 2] = K.IGN
    t[t < 0] = K.IGN
    assert torch.isfinite(S(x.to(dev()), t.to(dev()))).item()


# ------------------------------------------------------------------------------------------ (3) agreement with what exists
@pytest.mark.parametrize("mode,Cc", [("binary", 1), ("multilabel", 4), ("multiclass", 5)])
def test_defaults_agree_with_the_existing_losses(mode, Cc):
    for si, (N, H, W) in enumerate(K.SHAPES):
        x, tgt = K.make_inputs(mode, Cc, N, H, W, False)
        if mode == "multiclass":
            pairs = [(Ls.DiceLoss(mode), vk.multiclass.DiceLoss(mode)), (Ls.CrossEntropyLoss() + Ls.DiceLoss(mode), vk.multiclass.CEDiceLoss())]
        else:
            pairs = [(Ls.DiceLoss(mode), vk.multiclass.DiceLoss(mode)),
                     (Ls.BCEWithLogitsLoss() + Ls.DiceLoss(mode), vk.multiclass.BCEDiceLoss(mode))]
        for new, old in pairs:
            xa, xb = x.to(dev()).requires_grad_(), x.to(dev()).requires_grad_()
            la, lb = new(xa, tgt.to(dev())), old(xb, tgt.to(dev()))
            la.backward(); lb.backward()
            torch.cuda.synchronize()
            assert abs(la.item() - lb.item()) <= 2e-5 * abs(lb.item()) + 2e-6, (la.item(), lb.item())
            assert (xa.grad - xb.grad).abs().max().item() <= 2e-4 * xb.grad.abs().max().item()


# ------------------------------------------------------------------------------------------ (4) autograd
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("mode,Cc", [("binary", 1), ("multilabel", 4), ("multiclass", 5)])
def test_autograd_module(mode, Cc, dtype):
    N, H, W = K.SHAPES[0]
    x, tgt = K.make_inputs(mode, Cc, N, H, W, True)
    S = 0.5 * Ls.FocalLoss(mode, ignore_index=K.IGN) + Ls.TverskyLoss(mode, alpha=0.3, beta=0.7, ignore_index=K.IGN)
    xq = x.to(dtype)                                             # the reference sees the rounded logits
    rf = R.evaluate(xq.double(), tgt, S.spec(Cc))
    xd = xq.to(dev()).requires_grad_()
    loss = S(xd, tgt.to(dev()))
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.requires_grad
    (3.0 * loss).backward()
    torch.cuda.synchronize()
    assert abs(loss.item() - float(rf["total"])) <= 1e-5 * abs(float(rf["total"])) + 1e-6
    comp = S.last_components.cpu().double()
    assert comp.shape == (6,) and ((comp - R.components(rf)).abs() <= 1e-5 * R.components(rf).abs() + 1e-6).all()
    assert comp[1] == 0 and comp[3] == 0 and comp[4] == 0
    assert xd.grad.dtype == dtype
    ref_g = 3.0 * rf["dlogits"]
    bar = 1e-4 * ref_g.abs().max().item() + (2.0 ** -8 * ref_g.abs() if dtype == torch.bfloat16 else 0.0)
    err = (xd.grad.cpu().double() - ref_g).abs()
    print("%s C=%d %s: worst gradient error %.3g of its bar" % (mode, Cc, dtype, (err / bar).max().item()))
    assert (err <= bar).all()
    assert (xd.grad.cpu()[_dead(mode, x, tgt)] == 0).all()
    with torch.no_grad():                                        # no gradient asked for: the value alone
        assert S(xd, tgt.to(dev())).item() == loss.item()


# ------------------------------------------------------------------------------------------ (5) the fused step
def _model(classes):
    O = _O()
    O.set_seed(42)
    return vk.multiclass.Unet(encoder_weights=None, classes=classes).to(dev()).train()


def _step_inputs(classes, N=2, S=64, seed=97):
    O = _O()
    x, _ = O.synthetic_batch(N, S, seed=1234)
    mode = "binary" if classes == 1 else "multiclass"
    _, tgt = K.make_inputs(mode, classes, N, S, S, True, seed=seed)
    loss = 0.5 * Ls.FocalLoss(mode, alpha=0.25, ignore_index=K.IGN) + Ls.TverskyLoss(mode, alpha=0.3, beta=0.7, ignore_index=K.IGN)
    return x, tgt, mode, loss


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("classes", [1, 3])
def test_loss_and_backward_equals_autograd(classes, dtype):
    x, tgt, mode, S = _step_inputs(classes)
    x, tgt = x.to(dev()), tgt.to(dev())
    m = _model(classes)
    sd = copy.deepcopy(m.state_dict())
    ptrs = set()                       # where the fused steps put their results: one buffer of the plan, not one per call

    def autograd(scale=1.0):
        m.load_state_dict(sd)
        m.zero_grad(set_to_none=True)
        ctx = torch.autocast("cuda", dtype=dtype) if dtype != torch.float32 else torch.autocast("cuda", enabled=False)
        with ctx:
            lg = m(x)
        loss = S(lg.float(), tgt)
        (loss * scale).backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), m.flat_grads.detach().clone()

    def fused(scale=1.0):
        m.load_state_dict(sd)
        m.zero_grad(set_to_none=True)
        out = m.loss_and_backward(x, tgt, grad_scale=scale, dtype=dtype, loss=S)
        torch.cuda.synchronize()
        ptrs.add(out.data_ptr())
        return out.clone(), m.flat_grads.detach().clone()

    l_a, g_a = autograd()
    l_f, g_f = fused()
    assert l_f.shape == (6,) and torch.isfinite(l_f).all()
    assert abs(l_f[0].item() - l_a.item()) <= 1e-5 * abs(l_a.item())
    assert ((g_f - g_a).norm() / g_a.norm()).item() <= 1e-5
    assert torch.equal(S.last_components, l_f)
    assert tuple(m.last_logits.shape) == (x.shape[0], classes) + tuple(x.shape[2:])
    assert l_f[2].item() > 0 and l_f[5].item() > 0 and l_f[1].item() == 0 and l_f[3].item() == 0 and l_f[4].item() == 0
    assert abs(l_f[0].item() - (0.5 * l_f[2].item() + l_f[5].item())) <= 1e-6 * abs(l_f[0].item())
    _, g_s = fused(scale=256.0)
    _, g_as = autograd(scale=256.0)
    assert torch.equal(g_s, g_as)
    assert ((g_s - 256.0 * g_f).norm() / (256.0 * g_f).norm()).item() <= 1e-5
    assert len(ptrs) == 1
    # the default step is what it was: its own 4-float buffer, BCE + Dice or CE + Dice
    m.load_state_dict(sd)
    m.zero_grad(set_to_none=True)
    y_def = (tgt == 1).float() if classes == 1 else tgt.clamp_max(classes - 1)
    out = m.loss_and_backward(x, y_def, dtype=dtype, mode=None if classes == 1 else "multiclass")
    assert out.shape == (3,) and torch.isfinite(out).all()


@pytest.mark.parametrize("classes", [1, 3])
def test_two_seeded_steps_are_bit_identical(classes):
    x, tgt, mode, S = _step_inputs(classes)
    runs = []
    for _ in range(2):
        m = _model(classes)
        opt = vk.adamw_for(m, lr=5e-4, weight_decay=1e-4)
        for _ in range(2):
            opt.zero_grad(set_to_none=True)
            m.loss_and_backward(x.to(dev()), tgt.to(dev()), dtype=torch.bfloat16, loss=S)
            opt.step()
        torch.cuda.synchronize()
        runs.append(m.flat_params.detach().clone())
    assert torch.equal(runs[0], runs[1])


@pytest.mark.parametrize("classes", [1, 3])
def test_frozen_encoder(classes):
    x, tgt, mode, S = _step_inputs(classes)
    m = _model(classes)
    m.encoder.eval()
    m.zero_grad(set_to_none=True)
    m.loss_and_backward(x.to(dev()), tgt.to(dev()), loss=S)
    full = m.flat_grads.detach().clone()
    for p in m.encoder.parameters():
        p.requires_grad_(False)
    m.zero_grad(set_to_none=True)
    m.loss_and_backward(x.to(dev()), tgt.to(dev()), loss=S)
    torch.cuda.synchronize()
    part = m.flat_grads.detach().clone()
    for (name, p), (off, numel) in zip(m.named_parameters(), m._param_ranges):
        if name.startswith("encoder."):
            assert p.grad is None and part[off:off + numel].abs().max().item() == 0.0, name
        else:
            ref = full[off:off + numel]
            assert (part[off:off + numel] - ref).abs().max().item() <= 1e-5 * ref.abs().max().item() + 1e-12, name


def test_fused_step_against_the_float64_arbiter():
    """fp32, classes = 3: the fused step's loss against seglosses_ref applied to the oracle model's float64 logits"""
    O = _O()
    classes, N, S_ = 3, 8, 64
    O.set_seed(42)
    ref = O.OracleUnet(classes=classes)
    m = _model(classes)
    x, tgt, mode, S = _step_inputs(classes, N=N, S=S_)
    ref.train()
    ref64 = copy.deepcopy(ref).double()
    with torch.no_grad():
        lg64 = ref64(x.double())
    rf = R.evaluate(lg64, tgt, S.spec(classes))
    m.zero_grad(set_to_none=True)
    out = m.loss_and_backward(x.to(dev()), tgt.to(dev()), dtype=torch.float32, loss=S)
    torch.cuda.synchronize()
    want = R.components(rf)
    print("fused %s against float64: %s" % (out.tolist(), want.tolist()))
    assert abs(out[0].item() - float(want[0])) <= 1e-4 * abs(float(want[0]))
    assert (m.last_logits.cpu().double() - lg64).abs().max().item() <= 1e-3 * lg64.abs().max().item()


# ------------------------------------------------------------------------------------------ (6) launch families
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


OLD_LOSS_TAGS = {"bce_dice_loss", "multilabel_loss", "multiclass_loss"}


@pytest.mark.parametrize("classes", [1, 3])
def test_launch_families(classes):
    x, tgt, mode, S = _step_inputs(classes)
    x, tgt = x.to(dev()), tgt.to(dev())
    m = _model(classes)
    fam = _families(lambda: m.loss_and_backward(x, tgt, dtype=torch.bfloat16, loss=S))
    assert "seg_loss" in fam and fam["seg_loss"]["n"] == 1 and not (OLD_LOSS_TAGS & set(fam)), sorted(fam)
    y_def = (tgt == 1).float() if classes == 1 else tgt.clamp_max(classes - 1)
    fam = _families(lambda: m.loss_and_backward(x, y_def, dtype=torch.bfloat16, mode=None if classes == 1 else "multiclass"))
    assert "seg_loss" not in fam and (OLD_LOSS_TAGS & set(fam)), sorted(fam)
    lg = torch.randn(2, classes, 64, 64, device=dev(), requires_grad=True)
    fam = _families(lambda: S(lg, tgt).backward())
    assert set(fam) == {"seg_loss"} and fam["seg_loss"]["n"] == 1         # ONE call for the whole sum


# ------------------------------------------------------------------------------------------ (7) metrics with ignore_index
def _ulp_close(a, b, ulps=1):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.all(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)) <= ulps)


@pytest.mark.parametrize("Cc", [2, 5, 16])
def test_seg_metrics_with_ignore_index(Cc):
    for si, (N, H, W) in enumerate(K.SHAPES):
        x, t = K.make_inputs("multiclass", Cc, N, H, W, True)
        valid = (t != K.IGN).reshape(N, 1, -1)
        arg = x.reshape(N, Cc, -1).argmax(dim=1, keepdim=True)
        cls = torch.arange(Cc).view(1, Cc, 1)
        pred, tg = (arg == cls) & valid, (t.reshape(N, 1, -1) == cls) & valid
        tp = (pred & tg).sum(-1, dtype=torch.int64)
        fp = pred.sum(-1, dtype=torch.int64) - tp
        fn = tg.sum(-1, dtype=torch.int64) - tp
        want = ER.scores(tp.numpy(), fp.numpy(), fn.numpy())
        md, mu, dc, uc = Ls.seg_metrics(x.to(dev()), t.to(dev()), "multiclass", ignore_index=K.IGN)
        got = np.array([md, mu] + dc + uc, dtype=np.float32)
        assert _ulp_close(got, want[:2 + 2 * Cc]), np.abs(got - want[:2 + 2 * Cc]).max()
        with pytest.raises(vk.VkError, match="label"):                   # without ignore_index the same target is refused, as before
            vk.multiclass.seg_metrics(x.to(dev()), t.to(dev()), "multiclass")
        t2 = t.clone()
        t2[0, 0, 0], t2[N - 1, H - 1, W - 1] = Cc, -3
        n_bad = 2
        with pytest.raises(vk.VkError, match="%d label" % n_bad):
            Ls.seg_metrics(x.to(dev()), t2.to(dev()), "multiclass", ignore_index=K.IGN)
        clean = t.clone()
        clean[clean == K.IGN] = 0
        assert Ls.seg_metrics(x.to(dev()), clean.to(dev()), "multiclass") == vk.multiclass.seg_metrics(x.to(dev()), clean.to(dev()), "multiclass")
