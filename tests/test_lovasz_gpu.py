"""vk.lovasz on the MI355X (-m gpu): the sort / scan / apply core through vk_lovasz_flat with no tolerance on the order, the hinge and
softmax losses through vk_lovasz_loss against the float64 reference of tests/lovasz_ref.py, the MCC term of vk_seg_loss, the autograd
modules, the fused step and the launch families.

Bars: loss values within 1e-5 |ref| + 1e-6 (the project's bar, tests/test_seglosses_gpu.py); hinge and flat gradients per element
within 1e-5 grad_scale |ref_i| (at most eight fp32 roundings is about 5e-7; a foreground / background rank swap changes an element by
the factor I / (U - 1), far outside); softmax gradients by norm, ||dev - gs ref|| / ||gs ref|| <= max(8 d0, 1e-6) with d0 measured per
case on the CPU (tests/lovasz_cases.py); a second call bit-identical."""
import copy
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import lovasz_cases as LK
import lovasz_ref as LR
import seglosses_cases as K
import seglosses_ref as R

pytestmark = pytest.mark.gpu
vk = importlib.import_module("vickers-hardness-unet_amd")
Ls, Lv, L_ = vk.seglosses, vk.lovasz, vk._lib


def dev():
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _value_ok(got, want):
    return abs(got - want) <= 1e-5 * abs(want) + 1e-6


# ------------------------------------------------------------------------------------------ (1) the flat core
def _flat(e, f):
    L = vk.lib()
    S, Ln = e.shape
    ed, fd = torch.from_numpy(e).to(dev()), torch.from_numpy(f).to(dev())
    ws = torch.empty(L.vk_lovasz_flat_workspace_bytes(S, Ln), dtype=torch.uint8, device=dev())
    out = torch.full((S,), 5.0, device=dev())
    derr = torch.full((S, Ln), 7.0, device=dev())
    rank = torch.full((S, Ln), 9, dtype=torch.int32, device=dev())
    L_.check(L.vk_lovasz_flat(ed.data_ptr(), fd.data_ptr(), S, Ln, ws.data_ptr(), ws.numel(), out.data_ptr(), derr.data_ptr(),
                              rank.data_ptr(), _stream()), "vk_lovasz_flat")
    torch.cuda.synchronize()
    return out.cpu().numpy(), derr.cpu().numpy(), rank.cpu().numpy().view(np.uint32)


def _flat_cases():
    rng = np.random.default_rng(11)
    big = (1 << 22) + 3
    med = 3 * 4096 + 17

    def flags(S, Ln, p=0.1, ign=0.0):
        f = (rng.random((S, Ln)) < p).astype(np.uint8)
        if ign:
            f[rng.random((S, Ln)) < ign] = 2
        return f

    yield "random-big-S1", rng.standard_normal((1, big)).astype(np.float32), flags(1, big)
    yield "random-big-S5-ignored", rng.standard_normal((5, big)).astype(np.float32), flags(5, big, 0.3, 1.0 / 3.0)
    yield "all-equal", np.full((2, med), 0.75, np.float32), flags(2, med, 0.5)
    yield "ascending", np.tile(np.linspace(-2, 3, med, dtype=np.float32), (2, 1)), flags(2, med)
    yield "descending", np.tile(np.linspace(3, -2, med, dtype=np.float32), (1, 1)), flags(1, med)
    yield "signed-wide", (rng.standard_normal((3, med)) * np.exp(rng.uniform(-30, 30, (3, med)))).astype(np.float32), flags(3, med, 0.2)
    yield "quantised", (np.round(rng.standard_normal((2, med)) * 4) / 4).astype(np.float32), flags(2, med, 0.3, 0.2)
    yield "G0", rng.standard_normal((2, med)).astype(np.float32), np.zeros((2, med), np.uint8)
    yield "GL", rng.standard_normal((2, med)).astype(np.float32), np.ones((2, med), np.uint8)
    yield "L1", np.array([[0.5], [-0.5], [2.0]], np.float32), np.array([[1], [0], [2]], np.uint8)
    yield "all-ignored", rng.standard_normal((1, 100)).astype(np.float32), np.full((1, 100), 2, np.uint8)


@pytest.mark.parametrize("name,e,f", list(_flat_cases()), ids=[c[0] for c in _flat_cases()])
def test_flat_permutation_is_exact(name, e, f):
    loss, derr, rank = _flat(e, f)
    r_loss, r_derr, r_rank = LR.flat(e, f)
    assert np.array_equal(rank, r_rank), (name, int((rank != r_rank).sum()))
    for s in range(e.shape[0]):
        assert _value_ok(float(loss[s]), r_loss[s]), (name, s, loss[s], r_loss[s])
    assert (np.abs(derr - r_derr) <= 1e-5 * np.abs(r_derr)).all(), (name, np.abs(derr - r_derr).max())
    assert (derr[f == 2] == 0).all() and (derr[e <= 0] == 0).all()
    loss2, derr2, rank2 = _flat(e, f)
    assert np.array_equal(loss, loss2) and np.array_equal(derr, derr2) and np.array_equal(rank, rank2)


# ------------------------------------------------------------------------------------------ (2), (3) vk_lovasz_loss
def _cfg(mode, per_image, ign):
    return Lv.LovaszLoss(mode, per_image=per_image, ignore_index=ign).cfg


def _loss(cfg, x, tgt, grad_scale=1.0, prefill=None):
    L = vk.lib()
    N, Cc, H, W = x.shape
    xd = x.to(dev()).contiguous()
    td = (tgt.to(dev()) if cfg.mode == L_.VK_LOSS_MULTICLASS else tgt.to(dev()).float().expand_as(xd)).contiguous()
    ws = torch.empty(L.vk_lovasz_workspace_bytes(cfg, N, Cc, H * W), dtype=torch.uint8, device=dev())
    assert ws.numel() > 0
    out = torch.full((4,), 5.0, device=dev())
    dl = torch.full_like(xd, 7.0) if prefill is None else prefill.to(dev()).clone()
    L_.check(L.vk_lovasz_loss(cfg, N, Cc, H * W, xd.data_ptr(), td.data_ptr(), ws.data_ptr(), ws.numel(), out.data_ptr(), dl.data_ptr(),
                              grad_scale, 0 if prefill is None else 1, _stream()), "vk_lovasz_loss")
    torch.cuda.synchronize()
    return out.cpu().numpy(), dl.cpu().numpy()


@pytest.mark.parametrize("case", LK.HINGE, ids=LK.ident)
def test_hinge_against_float64(case):
    mode, Cc, per_image, ignore, si, quant = case
    x, y = LK.inputs(mode, Cc, ignore, si, quant)
    ign = LK.IGN if ignore else None
    cfg = _cfg(mode, per_image, ign)(Cc)
    v, g = LR.hinge(x.numpy(), y.numpy(), per_image, ign)
    yb = np.broadcast_to(y.numpy(), x.shape)
    e = 1.0 - x.numpy() * (2 * yb - 1)
    zero = (e <= 0) | (yb == LK.IGN if ignore else False)
    last = None
    for gs in (1.0, 1024.0):
        out, dl = _loss(cfg, x, y, gs)
        print("hinge %s gs=%g value %.9g ref %.9g max rel grad err %.3e" % (
            LK.ident(case), gs, out[0], v, (np.abs(dl - gs * g) / np.maximum(np.abs(gs * g), 1e-300))[g != 0].max()))
        assert _value_ok(float(out[0]), v) and out[1] == 0
        assert (np.abs(dl - gs * g) <= 1e-5 * gs * np.abs(g)).all()
        assert (dl[zero] == 0).all() and zero.any()
        last = (out, dl, gs)
    out2, dl2 = _loss(cfg, x, y, last[2])
    assert np.array_equal(out2, last[0]) and np.array_equal(dl2, last[1])
    pre = torch.full_like(x, 0.5)
    _, acc = _loss(cfg, x, y, 1.0, prefill=pre)
    _, one = _loss(cfg, x, y, 1.0)
    assert np.array_equal(acc, (0.5 + one).astype(np.float32))
    if ignore:
        assert (acc[yb == LK.IGN] == 0.5).all()


@pytest.mark.parametrize("case", LK.SOFTMAX, ids=LK.ident)
def test_softmax_against_float64(case):
    Cc, per_image, ignore, si, quant = case
    x, t = LK.inputs("multiclass", Cc, ignore, si, quant)
    ign = LK.IGN if ignore else None
    cfg = _cfg("multiclass", per_image, ign)(Cc)
    v, g, present = LR.softmax(x.numpy(), t.numpy(), per_image, ign)
    d0 = LK.softmax_d0(x, t, per_image, ign)
    bar = max(8 * d0, 1e-6)
    gmax = np.abs(g).max()
    last = None
    for gs in (1.0, 1024.0):
        out, dl = _loss(cfg, x, t, gs)
        rel = np.linalg.norm(dl - gs * g) / np.linalg.norm(gs * g)
        print("softmax %s gs=%g d0 %.3e bar %.3e rel %.3e value %.9g ref %.9g" % (LK.ident(case), gs, d0, bar, rel, out[0], v))
        assert _value_ok(float(out[0]), v) and out[1] == 0
        assert rel <= bar
        assert np.abs(dl.sum(axis=1)).max() <= 1e-6 * gs * gmax
        if ignore:
            dead = (t == LK.IGN).unsqueeze(1).expand_as(x).numpy()
            assert dead.any() and (dl[dead] == 0).all()
        last = (out, dl, gs)
    out2, dl2 = _loss(cfg, x, t, last[2])
    assert np.array_equal(out2, last[0]) and np.array_equal(dl2, last[1])
    assert all(1 not in pr for pr in present)            # class 1 is absent: it adds no term of its own (the value bar above sees it)
    if per_image:                                        # per-image = the batch form run image by image
        vals, grads = [], []
        bcfg = _cfg("multiclass", False, ign)(Cc)
        for n in range(x.shape[0]):
            o, d = _loss(bcfg, x[n:n + 1], t[n:n + 1], 1.0)
            vals.append(float(o[0]))
            grads.append(d / x.shape[0])
        o, d = _loss(cfg, x, t, 1.0)
        assert abs(float(o[0]) - np.mean(vals)) <= 1e-6 * abs(np.mean(vals)) + 1e-7
        assert np.abs(d - np.concatenate(grads)).max() <= 1e-6 * np.abs(d).max()
    pre = torch.full_like(x, 0.5)
    _, acc = _loss(cfg, x, t, 1.0, prefill=pre)
    _, one = _loss(cfg, x, t, 1.0)
    assert np.array_equal(acc, (0.5 + one).astype(np.float32))


def test_bad_label_is_counted_and_nothing_faults():
    x, t = LK.inputs("multiclass", 4, True, 0, False)
    t = t.clone()
    t.view(-1)[[5, 77, 1234]] = torch.tensor([4, -3, 10 ** 12])
    cfg = _cfg("multiclass", False, LK.IGN)(4)
    out, dl = _loss(cfg, x, t)
    assert np.isnan(out[0]) and out[1] == 3
    assert (dl.reshape(x.shape[0], 4, -1)[0][:, [5, 77, 1234]] == 0).all()
    with pytest.raises(vk.VkError, match="3 label"):
        Lv.LovaszLoss("multiclass", ignore_index=LK.IGN)(x.to(dev()), t.to(dev()))


def test_empty_segments_are_zero():
    x, y = LK.inputs("binary", 1, False, 0, False)
    y = torch.full_like(y, float(LK.IGN))
    out, dl = _loss(_cfg("binary", True, LK.IGN)(1), x, y)
    assert out[0] == 0 and (dl == 0).all()
    x, t = LK.inputs("multiclass", 3, False, 0, False)
    t = torch.full_like(t, LK.IGN)
    out, dl = _loss(_cfg("multiclass", False, LK.IGN)(3), x, t)
    assert out[0] == 0 and out[1] == 0 and (dl == 0).all()


# ------------------------------------------------------------------------------------------ (4) MCC
def _seg_call(cfg, x, tgt, gs=1.0):
    L = vk.lib()
    N, Cc, H, W = x.shape
    xd = x.to(dev()).contiguous()
    td = tgt.to(dev()).float().expand_as(xd).contiguous()
    ws = torch.empty(L.vk_seg_loss_workspace_bytes(N, Cc, H * W), dtype=torch.uint8, device=dev())
    out = torch.full((8,), 5.0, device=dev())
    dl = torch.full_like(xd, 7.0)
    L_.check(L.vk_seg_loss(cfg, N, Cc, H * W, xd.data_ptr(), td.data_ptr(), ws.data_ptr(), ws.numel(), out.data_ptr(), dl.data_ptr(), gs,
                           _stream()), "vk_seg_loss")
    torch.cuda.synchronize()
    return out.cpu().numpy(), dl.cpu().numpy()


@pytest.mark.parametrize("ignore", [False, True])
def test_mcc_alone_and_in_a_sum(ignore):
    ign = LK.IGN if ignore else None
    for si in (0, 1):
        x, y = LK.inputs("binary", 1, ignore, si, False)
        v, g = LR.mcc(x.numpy(), y.numpy(), 1e-5, ign)
        alone = Lv.MCCLoss() if not ignore else Lv.MCCLoss() + 0.0 * Ls.DiceLoss("binary", ignore_index=ign)
        out, dl = _seg_call(alone.cfg(1), x, y)
        assert _value_ok(float(out[7]), v) and _value_ok(float(out[0]), v)
        assert np.abs(dl - g).max() <= 1e-4 * np.abs(g).max()
        five = (Ls.SoftBCEWithLogitsLoss(ignore_index=ign, smooth_factor=0.1) + 0.5 * Ls.FocalLoss("binary", ignore_index=ign)
                + Ls.DiceLoss("binary", ignore_index=ign) + 0.25 * Ls.TverskyLoss("binary", alpha=0.3, beta=0.7, ignore_index=ign))
        spec = five.spec(1)
        rf = R.evaluate(x, y, spec)
        for gs in (1.0, 1024.0):
            out, dl = _seg_call((five + 0.7 * Lv.MCCLoss()).cfg(1), x, y, gs)
            want = float(rf["total"]) + 0.7 * v
            gref = rf["dlogits"].numpy().reshape(x.shape) + 0.7 * g
            assert _value_ok(float(out[0]), want) and _value_ok(float(out[7]), v)
            assert np.abs(dl - gs * gref).max() <= 1e-4 * gs * np.abs(gref).max()
        out, _ = _seg_call(five.cfg(1), x, y)
        assert out[7] == 0


# ------------------------------------------------------------------------------------------ (5) modules and the fused step
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_autograd_module(dtype):
    x, y = LK.inputs("multilabel", 4, True, 0, False)
    lov = Lv.LovaszLoss("multilabel", per_image=True, ignore_index=LK.IGN)
    lg = x.to(dev()).to(dtype).requires_grad_()
    loss = lov(lg, y.to(dev()))
    (3.0 * loss).backward()
    v, g = LR.hinge(lg.detach().float().cpu().numpy(), y.numpy(), True, LK.IGN)
    assert _value_ok(loss.item(), v) and lg.grad.dtype == dtype
    tol = 1e-5 if dtype == torch.float32 else 2.0 ** -8
    assert (np.abs(lg.grad.float().cpu().numpy() - 3.0 * g) <= tol * 3.0 * np.abs(g)).all()
    S = Ls.BCEWithLogitsLoss() + Ls.DiceLoss("multilabel") + 0.5 * lov
    lg = x.to(dev()).requires_grad_()
    tot = S(lg, y.to(dev()))
    tot.backward()
    rf = R.evaluate(x, y, S.seg.spec(4))
    v, g = LR.hinge(x.numpy(), y.numpy(), True, LK.IGN)
    assert _value_ok(tot.item(), float(rf["total"]) + 0.5 * v)
    gref = rf["dlogits"].numpy().reshape(x.shape) + 0.5 * g
    assert np.abs(lg.grad.cpu().numpy() - gref).max() <= 1e-4 * np.abs(gref).max()
    assert S.last_components.shape == (8,) and _value_ok(S.last_components[7].item(), v)


def _O():
    from oracle import unet_oracle as O
    return O


def _model(classes):
    O = _O()
    O.set_seed(42)
    return vk.multiclass.Unet(encoder_weights=None, classes=classes).to(dev()).train()


def _step_inputs(classes, N=2, S=64, seed=97):
    x, _ = _O().synthetic_batch(N, S, seed=1234)
    if classes == 1:
        _, tgt = K.make_inputs("binary", 1, N, S, S, False, seed=seed)
        return x, tgt, Ls.BCEWithLogitsLoss() + 0.5 * Lv.LovaszLoss("binary")
    _, tgt = K.make_inputs("multiclass", classes, N, S, S, True, seed=seed)
    return x, tgt, (Ls.CrossEntropyLoss(ignore_index=K.IGN) + Ls.DiceLoss("multiclass", ignore_index=K.IGN)
                    + Lv.LovaszLoss("multiclass", per_image=True, ignore_index=K.IGN))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("classes", [1, 3])
def test_loss_and_backward_equals_autograd(classes, dtype):
    x, tgt, S = _step_inputs(classes)
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
    assert l_f.shape == (8,) and torch.isfinite(l_f).all()
    assert abs(l_f[0].item() - l_a.item()) <= 1e-5 * abs(l_a.item())
    assert ((g_f - g_a).norm() / g_a.norm()).item() <= 1e-5
    assert torch.equal(S.last_components, l_f) and l_f[7].item() > 0 and l_f[1].item() > 0
    assert tuple(m.last_logits.shape) == (x.shape[0], classes) + tuple(x.shape[2:])
    _, g_s = fused(scale=256.0)
    assert ((g_s - 256.0 * g_f).norm() / (256.0 * g_f).norm()).item() <= 1e-5
    # two seeded steps are bit-identical
    l_2, g_2 = fused()
    assert torch.equal(l_2, l_f) and torch.equal(g_2, g_f)
    assert len(ptrs) == 1
    # a plain vk.seglosses sum keeps its 6-entry result
    m.load_state_dict(sd)
    m.zero_grad(set_to_none=True)
    assert m.loss_and_backward(x, tgt, dtype=dtype, loss=S.seg).shape == (6,)


def test_lovasz_alone_and_frozen_encoder_step():
    x, tgt, _ = _step_inputs(1)
    x, tgt = x.to(dev()), tgt.to(dev())
    S = Lv.LovaszLoss("binary", per_image=True)
    m = _model(1)
    sd = copy.deepcopy(m.state_dict())
    for p in m.encoder.parameters():
        p.requires_grad_(False)
    m.zero_grad(set_to_none=True)
    out = m.loss_and_backward(x, tgt, loss=S)
    torch.cuda.synchronize()
    g_f = m.flat_grads.detach().clone()
    m.load_state_dict(sd)
    m.zero_grad(set_to_none=True)
    loss = S(m(x), tgt)
    loss.backward()
    torch.cuda.synchronize()
    g_a = m.flat_grads.detach().clone()
    assert out.shape == (8,) and abs(out[0].item() - loss.item()) <= 1e-5 * abs(loss.item()) and out[0].item() == out[7].item()
    assert (out[1:7] == 0).all()
    assert g_a.norm().item() > 0 and ((g_f - g_a).norm() / g_a.norm()).item() <= 1e-5
    frozen = [p for p in m.encoder.parameters()]
    assert all(p.grad is None or not p.grad.any() for p in frozen)


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


def test_launch_families():
    x, tgt, S = _step_inputs(1)
    lg = torch.randn(2, 1, 64, 64, device=dev(), requires_grad=True)
    fam = _families(lambda: S(lg, tgt.to(dev())).backward())
    assert set(fam) == {"seg_loss", "lovasz"} and fam["lovasz"]["n"] == 1 and fam["seg_loss"]["n"] == 1, sorted(fam)
    fam = _families(lambda: Lv.LovaszLoss("binary")(lg, tgt.to(dev())).backward())
    assert set(fam) == {"lovasz"}, sorted(fam)
    m = _model(1)
    m.loss_and_backward(x.to(dev()), tgt.to(dev()), dtype=torch.bfloat16, loss=S.seg)          # the first step also repacks the weights
    base = _families(lambda: m.loss_and_backward(x.to(dev()), tgt.to(dev()), dtype=torch.bfloat16, loss=S.seg))
    fam = _families(lambda: m.loss_and_backward(x.to(dev()), tgt.to(dev()), dtype=torch.bfloat16, loss=S))
    assert set(fam) == set(base) | {"lovasz"} and fam["lovasz"]["n"] == 1, sorted(set(fam) ^ set(base))
