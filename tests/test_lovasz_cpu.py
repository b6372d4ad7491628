"""vk.lovasz, the parts that need no GPU: the float64 reference (tests/lovasz_ref.py) against torch autograd of smp's formulas written
naively (float cumsums, torch.sort(stable=True, descending=True)), the closed-form Jaccard increments, the MCC term, constructors,
refusals, the loss algebra and the host-side argument checks of the C ABI."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import lovasz_cases as LK
import lovasz_ref as LR
import seglosses_ref as R

vk = importlib.import_module("vickers-hardness-unet_amd")


@pytest.fixture(scope="module")
def Lv():
    return vk.lovasz


def _lovasz_grad(gs):
    gts = gs.sum()
    inter = gts - gs.cumsum(0)
    union = gts + (1.0 - gs).cumsum(0)
    jac = 1.0 - inter / union
    if gs.numel() > 1:
        jac[1:] = jac[1:] - jac[:-1]
    return jac


def _naive_hinge(xd, y, per_image, ign):
    y = y.double().expand_as(xd)
    segs = [(xd[n], y[n]) for n in range(xd.shape[0])] if per_image else [(xd, y)]
    tot = xd.sum() * 0.0
    for lg, lab in segs:
        lg, lab = lg.reshape(-1), lab.reshape(-1)
        if ign is not None:
            keep = lab != ign
            lg, lab = lg[keep], lab[keep]
        if lg.numel() == 0:
            continue
        errors = 1.0 - lg * (2.0 * lab - 1.0)
        errors = errors + (errors.detach().float().double() - errors.detach())      # the error is an fp32 number (one rounding)
        perm = torch.sort(errors.detach().float(), stable=True, descending=True).indices
        tot = tot + torch.dot(torch.relu(errors[perm]), _lovasz_grad(lab[perm]))
    return tot / len(segs)


def _naive_softmax(xd, t, per_image, ign):
    p = torch.softmax(xd, dim=1)
    Cc = xd.shape[1]
    segs = [(p[n:n + 1], t[n:n + 1]) for n in range(xd.shape[0])] if per_image else [(p, t)]
    tot = xd.sum() * 0.0
    for pp, tt in segs:
        pp = pp.permute(0, 2, 3, 1).reshape(-1, Cc)
        tt = tt.reshape(-1)
        if ign is not None:
            keep = tt != ign
            pp, tt = pp[keep], tt[keep]
        losses = []
        for c in range(Cc):
            fg = (tt == c).double()
            if fg.sum() == 0:
                continue
            errors = (fg - pp[:, c]).abs()
            perm = torch.sort(errors.detach(), stable=True, descending=True).indices
            losses.append(torch.dot(errors[perm], _lovasz_grad(fg[perm])))
        if losses:
            tot = tot + sum(losses) / len(losses)
    return tot / len(segs), p.detach()


@pytest.mark.parametrize("case", LK.HINGE, ids=LK.ident)
def test_hinge_ref_equals_autograd_of_the_naive_formulas(case):
    mode, Cc, per_image, ignore, si, quant = case
    assert Cc in (1, 4, 16)
    x, y = LK.inputs(mode, Cc, ignore, si, quant)
    ign = LK.IGN if ignore else None
    xd = x.double().requires_grad_()
    nv = _naive_hinge(xd, y, per_image, ign)
    nv.backward()
    v, g = LR.hinge(x.numpy(), y.numpy(), per_image, ign)
    assert abs(v - nv.item()) <= 1e-12 * abs(nv.item()) + 1e-15
    gmax = xd.grad.abs().max().item()
    assert gmax > 0 and np.abs(g - xd.grad.numpy()).max() <= 1e-10 * gmax
    if ignore:
        dead = (y == LK.IGN).expand_as(x).numpy()
        assert dead.any() and (g[dead] == 0).all()
    if quant:
        e = 1.0 - x.numpy() * (2 * np.broadcast_to(y.numpy(), x.shape) - 1)
        assert np.unique(e).size < e.size // 8          # massive ties


@pytest.mark.parametrize("case", LK.SOFTMAX, ids=LK.ident)
def test_softmax_ref_equals_autograd_of_the_naive_formulas(case):
    Cc, per_image, ignore, si, quant = case
    x, t = LK.inputs("multiclass", Cc, ignore, si, quant)
    ign = LK.IGN if ignore else None
    xd = x.double().requires_grad_()
    nv, p = _naive_softmax(xd, t, per_image, ign)
    nv.backward()
    v, g, present = LR.softmax(x.numpy(), t.numpy(), per_image, ign, probs=p.numpy())
    assert abs(v - nv.item()) <= 1e-12 * abs(nv.item()) + 1e-15
    gmax = xd.grad.abs().max().item()
    assert gmax > 0 and np.abs(g - xd.grad.numpy()).max() <= 1e-10 * gmax
    assert all(1 not in pr for pr in present)                 # class 1 is absent from these inputs
    assert np.abs(g.sum(axis=1)).max() <= 1e-12 * gmax
    if ignore:
        dead = (t == LK.IGN).unsqueeze(1).expand_as(x).numpy()
        assert dead.any() and (g[dead] == 0).all()
    d0 = LK.softmax_d0(x, t, per_image, ign)
    print("d0 %s = %.3e" % (LK.ident(case), d0))
    assert d0 < 1e-3


def test_closed_form_increments_equal_the_cumsum_form():
    rng = np.random.default_rng(5)
    n = 5000
    cases = [np.zeros(n, int), np.ones(n, int), np.array([0]), np.array([1]), (rng.random(n) < 0.1).astype(int),
             (rng.random(n) < 0.5).astype(int), (rng.random(7) < 0.5).astype(int)]
    for g in cases:
        a, b = LR.dj_closed(g), LR.dj_cumsum(g)
        assert a.shape == b.shape and np.abs(a - b).max() <= 1e-15, np.abs(a - b).max()
        assert abs(a.sum() - (1.0 if g.size else 0.0)) <= 1e-12 or g.sum() == g.size      # J_{n-1} = 1 unless every entry is foreground
    assert LR.dj_closed(np.zeros(4, int)).tolist() == [1.0, 0.0, 0.0, 0.0]


def test_flat_reference_order_is_stable_and_descending():
    e = np.array([[0.5, -1.0, 0.5, 2.0, 0.5, -0.0, 0.0]], np.float32)
    f = np.array([[1, 0, 2, 0, 0, 1, 1]], np.uint8)
    loss, derr, rank = LR.flat(e, f)
    assert rank[0].tolist() == [1, 5, 0xFFFFFFFF, 0, 2, 4, 3]
    assert derr[0][2] == 0 and derr[0][1] == 0


@pytest.mark.parametrize("ignore", [False, True])
def test_mcc_ref_equals_autograd(Lv, ignore):
    x, y = LK.inputs("binary", 1, ignore, 0, False)
    ign = LK.IGN if ignore else None
    eps = 1e-5
    xd = x.double().requires_grad_()
    m = (y != LK.IGN).double() if ignore else torch.ones_like(xd)
    yy = y.double() * m
    p = torch.sigmoid(xd)
    tp = (p * yy * m).sum() + eps
    tn = ((1 - p) * (1 - yy) * m).sum() + eps
    fp = (p * (1 - yy) * m).sum() + eps
    fn = ((1 - p) * yy * m).sum() + eps
    loss = 1.0 - (tp * tn - fp * fn) / torch.sqrt((tp + fp) * (tp + fn) * (tn + fp) * (tn + fn))
    loss.backward()
    v, g = LR.mcc(x.numpy(), y.numpy(), eps, ign)
    assert abs(v - loss.item()) <= 1e-12 * abs(loss.item())
    assert np.abs(g - xd.grad.numpy()).max() <= 1e-10 * xd.grad.abs().max().item()


def test_mcc_joins_the_fused_configuration(Lv):
    Ls = vk.seglosses
    S = Ls.BCEWithLogitsLoss() + Ls.DiceLoss("binary") + 0.5 * Lv.MCCLoss(eps=1e-4)
    cfg = S.cfg(1)
    assert cfg.terms == 1 | 4 | 32 and cfg.w_mcc == 0.5 and abs(cfg.mcc_eps - 1e-4) < 1e-10 and cfg.mode == 0
    assert C.sizeof(vk._lib.vk_seg_loss_cfg) == vk.lib().vk_seg_loss_cfg_size() == cfg.struct_size
    assert Ls.KINDS[5] == "mcc" and S.spec(1)["terms"]["mcc"] == dict(eps=1e-4, w=0.5)
    with pytest.raises(ValueError, match="mode"):
        Lv.MCCLoss() + Ls.DiceLoss("multilabel")
    with pytest.raises(ValueError, match="mode"):
        Lv.MCCLoss() + Ls.CrossEntropyLoss()
    with pytest.raises(ValueError, match="one channel"):
        Lv.MCCLoss().cfg(3)
    with pytest.raises(ValueError, match="kind"):
        Lv.MCCLoss() + Lv.MCCLoss()
    with pytest.raises(ValueError, match="eps"):
        Lv.MCCLoss(eps=0.0)
    # the C side: bit 5 only in binary mode, bit 6 refused
    L = vk.lib()
    ws = 1 << 20
    for mode, Cc, terms, ok in [(0, 1, 32, True), (1, 1, 32, False), (1, 3, 4 | 32, False), (0, 1, 64, False)]:
        c = Ls.DiceLoss("binary").cfg(1)
        c.mode, c.terms, c.w_mcc, c.mcc_eps = mode, terms, 1.0, 1e-5
        rc = L.vk_seg_loss(c, 2, Cc, 64, None, None, None, ws, None, None, 1.0, None)
        msg = L.vk_last_error_string()
        assert rc < 0 and ((b"null" in msg) if ok else (b"mcc" in msg or b"terms" in msg)), (mode, Cc, terms, msg)


def test_constructors_refusals_and_algebra(Lv):
    Ls = vk.seglosses
    NI = NotImplementedError
    with pytest.raises(NI, match="Lovasz"):
        Ls.LovaszLoss("binary")
    with pytest.raises(NI, match="MCC"):
        Ls.MCCLoss()
    with pytest.raises(NI, match="from_logits"):
        Lv.LovaszLoss("binary", from_logits=False)
    with pytest.raises(ValueError, match="mode"):
        Lv.LovaszLoss("ternary")
    with pytest.raises(ValueError, match="ignore_index"):
        Lv.LovaszLoss("binary", ignore_index=2.5)
    lov = Lv.LovaszLoss("binary", per_image=True, ignore_index=255)
    cfg = lov.cfg(1)
    assert (cfg.struct_size, cfg.mode, cfg.per_image, cfg.has_ignore, cfg.ignore_index) == (vk.lib().vk_lovasz_cfg_size(), 0, 1, 1, 255)
    assert C.sizeof(vk._lib.vk_lovasz_cfg) == vk.lib().vk_lovasz_cfg_size()
    with pytest.raises(ValueError, match="one channel"):
        lov.cfg(3)
    with pytest.raises(ValueError, match="C >= 2"):
        Lv.LovaszLoss("multiclass").cfg(1)
    seg = Ls.BCEWithLogitsLoss() + 0.5 * Ls.DiceLoss("binary")
    for S in (seg + lov, lov + seg, sum([seg, lov])):
        assert isinstance(S, Lv.LossSum) and S.w == 1.0 and S.mode == "binary" and S.ignore_index == 255
        assert S.seg.ignore_index == 255 and S.seg.mode == "binary" and S.seg_cfg(1).terms == 1 | 4 and S.seg_cfg(1).has_ignore == 1
    assert seg.ignore_index is None                       # the operand is not changed
    H = 0.5 * lov
    assert isinstance(H, Lv.LossSum) and H.w == 0.5 and H.seg is None and H.seg_cfg(1) is None and (lov * 0.5).w == 0.5
    D = 2.0 * (seg + 0.25 * lov)
    assert D.w == 0.5 and [w for w, _ in D.seg.terms] == [2.0, 1.0]
    A = (lov + Ls.BCEWithLogitsLoss()) + Ls.FocalLoss("binary")
    assert sorted(t.kind for _, t in A.seg.terms) == ["focal", "pix"]
    assert isinstance(Lv.MCCLoss() + lov, Lv.LossSum)
    with pytest.raises(ValueError, match="two Lovasz"):
        lov + Lv.LovaszLoss("binary")
    with pytest.raises(ValueError, match="two Lovasz"):
        (seg + lov) + 0.5 * lov
    with pytest.raises(ValueError, match="mode"):
        Ls.DiceLoss("multilabel") + lov
    with pytest.raises(ValueError, match="BCE"):
        Ls.BCEWithLogitsLoss() + Lv.LovaszLoss("multiclass")
    with pytest.raises(ValueError, match="ignore_index"):
        Ls.DiceLoss("binary", ignore_index=7) + lov
    with pytest.raises(TypeError):
        lov + 1.0
    with pytest.raises(TypeError):
        lov * "2"
    with pytest.raises(ValueError, match="finite"):
        lov * float("inf")
    # the pinned refusals of vk.seglosses are what they were
    with pytest.raises(TypeError):
        seg + 1.0
    m = vk.multiclass.Unet(encoder_weights=None, classes=3)
    with pytest.raises(TypeError):
        m.loss_and_backward(torch.zeros(1, 3, 64, 64), torch.zeros(1, 64, 64, dtype=torch.int64), loss=torch.nn.CrossEntropyLoss())
    with pytest.raises(ValueError, match="one channel"):
        m.loss_and_backward(torch.zeros(1, 3, 64, 64), torch.zeros(1, 64, 64, dtype=torch.int64), loss=lov)


def test_cpu_tensors_are_refused(Lv):
    lov = Lv.LovaszLoss("multiclass")
    with pytest.raises(vk.VkError, match="no CPU fallback"):
        lov(torch.zeros(2, 3, 8, 8, requires_grad=True), torch.zeros(2, 8, 8, dtype=torch.int64))
    with pytest.raises(vk.VkError, match="no CPU fallback"):
        (vk.seglosses.BCEWithLogitsLoss() + Lv.LovaszLoss("binary"))(torch.zeros(2, 1, 8, 8), torch.zeros(2, 1, 8, 8))
    with pytest.raises(ValueError, match="int64"):
        lov(torch.zeros(2, 3, 8, 8), torch.zeros(2, 8, 8))
    with pytest.raises(ValueError, match="broadcast"):
        Lv.LovaszLoss("multilabel")(torch.zeros(2, 3, 8, 8), torch.zeros(2, 2, 8, 8))


def _lcfg(mode=0, per_image=0, has_ignore=0, ignore=0, size=None):
    c = vk._lib.vk_lovasz_cfg()
    c.struct_size = C.sizeof(c) if size is None else size
    c.mode, c.per_image, c.has_ignore, c.ignore_index = mode, per_image, has_ignore, ignore
    return c


def test_workspace_bytes():
    L = vk.lib()
    assert L.vk_lovasz_workspace_bytes(_lcfg(0), 2, 1, 64 * 64) >= 2 * 8 * 2 * 64 * 64
    assert L.vk_lovasz_workspace_bytes(_lcfg(2, 1), 2, 4, 64 * 64) >= 2 * 8 * 2 * 64 * 64 + 4 * 2 * 4 * 64 * 64
    assert L.vk_lovasz_workspace_bytes(_lcfg(1, 1, 1, 255), 3, 16, 33 * 47) > 0
    for cfg, N, Cc, HW in [(_lcfg(0), 2, 2, 64), (_lcfg(2), 2, 1, 64), (_lcfg(1), 2, 17, 64), (_lcfg(1), 0, 1, 64), (_lcfg(1), 2, 1, 0),
                           (_lcfg(3), 2, 1, 64), (_lcfg(0, size=8), 2, 1, 64), (_lcfg(1), 4, 16, 1 << 25), (_lcfg(0, per_image=2), 2, 1, 64)]:
        assert L.vk_lovasz_workspace_bytes(cfg, N, Cc, HW) == 0
    assert L.vk_lovasz_workspace_bytes(None, 2, 1, 64) == 0
    assert L.vk_lovasz_flat_workspace_bytes(5, (1 << 22) + 3) > 5 * 16 * (1 << 22)
    assert L.vk_lovasz_flat_workspace_bytes(0, 8) == 0 and L.vk_lovasz_flat_workspace_bytes(2, 0) == 0
    assert L.vk_lovasz_flat_workspace_bytes(2, 1 << 30) == 0


def test_host_side_argument_errors():
    L = vk.lib()
    err = L.vk_last_error_string
    big = 1 << 40

    def loss(cfg, N=2, Cc=1, HW=64, x=8, t=8, ws=8, wsb=big, out=8, gs=1.0, acc=0):
        return L.vk_lovasz_loss(cfg, N, Cc, HW, x, t, ws, wsb, out, None, gs, acc, None)

    for kw, word in [(dict(cfg=None), b"null configuration"), (dict(cfg=_lcfg(0, size=4)), b"struct_size"), (dict(cfg=_lcfg(5)), b"mode"),
                     (dict(cfg=_lcfg(0), Cc=2), b"binary"), (dict(cfg=_lcfg(2)), b"multiclass"), (dict(cfg=_lcfg(1), Cc=17), b"1..16"),
                     (dict(cfg=_lcfg(1), HW=0), b"shape"), (dict(cfg=_lcfg(1), N=4, Cc=16, HW=1 << 25), b"2^31"),
                     (dict(cfg=_lcfg(0), x=None), b"null argument"), (dict(cfg=_lcfg(0), out=None), b"null argument"),
                     (dict(cfg=_lcfg(0), wsb=64), b"workspace"), (dict(cfg=_lcfg(0), gs=float("nan")), b"grad_scale"),
                     (dict(cfg=_lcfg(0), acc=2), b"accumulate"), (dict(cfg=_lcfg(0, per_image=3)), b"per_image")]:
        assert loss(**kw) < 0 and word in err(), (kw, err())

    def flat(e=8, f=8, S=1, Ln=64, ws=8, wsb=big, out=8):
        return L.vk_lovasz_flat(e, f, S, Ln, ws, wsb, out, None, None, None)

    for kw, word in [(dict(S=0), b"shape"), (dict(Ln=0), b"shape"), (dict(S=2, Ln=1 << 30), b"shape"), (dict(e=None), b"null"),
                     (dict(f=None), b"null"), (dict(out=None), b"null"), (dict(wsb=128), b"workspace"), (dict(ws=4), b"workspace")]:
        assert flat(**kw) < 0 and word in err(), (kw, err())
    assert L.vk_unet_loss_lovasz(None, None, _lcfg(0), 1.0, 8, 8, 8, big, 8, 1.0, None) < 0 and b"vk_unet_loss_lovasz" in err()
