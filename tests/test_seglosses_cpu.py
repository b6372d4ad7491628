"""vk.seglosses, the parts that need no GPU: the float64 closed form (tests/seglosses_ref.py) against torch autograd of the smp
formulas written naively and against torch.nn.functional; the constructors, their refusals and the LossSum algebra; the ctypes mirror
of vk_seg_loss_cfg and the host-side argument checks of vk_seg_loss."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import multiclass_ref as MR
import seglosses_cases as K
import seglosses_ref as R


@pytest.fixture(scope="module")
def Ls(vk):
    return vk.seglosses


# ------------------------------------------------------------------------------------------ the smp formulas, naively, for autograd
def _smp_score(kind, p, y, o):
    dims = (0, 2)
    inter = (p * y).sum(dims)
    if kind == "dice":
        card = (p + y).sum(dims)
        return (2.0 * inter + o["smooth"]) / (card + o["smooth"]).clamp_min(o["eps"])
    if kind == "jaccard":
        union = (p + y).sum(dims) - inter
        return (inter + o["smooth"]) / (union + o["smooth"]).clamp_min(o["eps"])
    fp = (p * (1.0 - y)).sum(dims)
    fn = ((1 - p) * y).sum(dims)
    return (inter + o["smooth"]) / (inter + o["alpha"] * fp + o["beta"] * fn + o["smooth"]).clamp_min(o["eps"])


def _smp_focal(x, y, alpha, gamma):
    """smp focal_loss_with_logits, reduction 'mean', on flat tensors"""
    logpt = F.binary_cross_entropy_with_logits(x, y, reduction="none")
    pt = torch.exp(-logpt)
    loss = (1.0 - pt).pow(gamma) * logpt
    if alpha is not None:
        loss = loss * (alpha * y + (1 - alpha) * (1 - y))
    return loss.mean()


def naive(x, target, spec):
    """dict of the unweighted term values and the total, differentiable w.r.t. x (float64 [N,C,H,W])"""
    N, Cc = x.shape[:2]
    mode, ign, terms = spec["mode"], spec["ignore_index"], spec["terms"]
    out = {}
    if mode == "multiclass":
        t = target
        mask = (t != ign) if ign is not None else torch.ones_like(t, dtype=torch.bool)
    else:
        yf = target.double().expand_as(x)
        mask = (yf != ign) if ign is not None else torch.ones_like(yf, dtype=torch.bool)
    if "pix" in terms:
        o = terms["pix"]
        sf = o["smooth_factor"]
        if mode == "multiclass":
            logp = torch.log_softmax(x, dim=1)
            tt = torch.where(mask, t, torch.zeros_like(t))
            nll = -logp.gather(1, tt.unsqueeze(1)).squeeze(1).masked_fill(~mask, 0.0)
            smooth = -logp.sum(dim=1).masked_fill(~mask, 0.0)
            den = mask.sum() if o["denom"] == "valid" else mask.numel()
            out["pix"] = (1 - sf) * nll.sum() / den + sf / Cc * smooth.sum() / den
        else:
            ys = (1 - yf) * sf + yf * (1 - sf)
            pw = None if o["pos_weight"] is None else torch.tensor(o["pos_weight"], dtype=torch.float64).view(1, Cc, 1, 1)
            l = F.binary_cross_entropy_with_logits(x, ys, pos_weight=pw, reduction="none") * mask
            out["pix"] = l.sum() / (mask.sum() if o["denom"] == "valid" else mask.numel())
    if "focal" in terms:
        o = terms["focal"]
        if mode == "multiclass":
            out["focal"] = sum(_smp_focal(x[:, c][mask], (t == c).double()[mask], o["alpha"], o["gamma"]) for c in range(Cc))
        else:
            out["focal"] = _smp_focal(x[mask], yf[mask], o["alpha"], o["gamma"])
    for kind in ("dice", "jaccard", "tversky"):
        if kind not in terms:
            continue
        o = terms[kind]
        if mode == "multiclass":
            p = torch.softmax(x, dim=1).reshape(N, Cc, -1) * mask.reshape(N, 1, -1)
            y = F.one_hot((t * mask).long(), Cc).permute(0, 3, 1, 2).reshape(N, Cc, -1).double() * mask.reshape(N, 1, -1)
        else:
            p = (torch.sigmoid(x) * mask).reshape(N, Cc, -1)
            y = (yf * mask).reshape(N, Cc, -1)
        score = _smp_score(kind, p, y, o)
        loss = -torch.log(score.clamp_min(o["eps"])) if o["log_loss"] else 1.0 - score
        loss = loss * (y.sum((0, 2)) > 0).double()
        if o["classes"] is not None:
            loss = loss[o["classes"]]
        loss = loss.mean()
        out[kind] = loss ** o["gamma"] if kind == "tversky" else loss
    out["total"] = sum(terms[k]["w"] * out[k] for k in terms)
    return out


@pytest.mark.parametrize("name", K.case_names())
@pytest.mark.parametrize("mode,Cc", K.MODE_C)
def test_ref_equals_autograd_of_the_naive_formulas(Ls, mode, Cc, name):
    for si, (N, H, W) in enumerate(K.SHAPES):
        ign = K.ignored(name, si)
        x, tgt = K.make_inputs(mode, Cc, N, H, W, ign)
        spec = K.build(Ls, name, mode, Cc, ign).spec(Cc)
        xd = x.double().requires_grad_()
        nv = naive(xd, tgt, spec)
        nv["total"].backward()
        rf = R.evaluate(x, tgt, spec)
        for k in ("total",) + R.KINDS:
            if k in nv:
                assert abs(float(rf[k]) - float(nv[k].detach())) <= 1e-12 * abs(float(nv[k].detach())) + 1e-15, (k, float(rf[k]), float(nv[k].detach()))
            else:
                assert float(rf[k]) == 0.0
        gmax = xd.grad.abs().max().item()
        assert gmax > 0
        assert (rf["dlogits"] - xd.grad).abs().max().item() <= 1e-10 * gmax
        if ign:
            dead = (tgt == K.IGN) if mode != "multiclass" else (tgt == K.IGN).unsqueeze(1).expand_as(x)
            assert dead.any() and (rf["dlogits"][dead] == 0).all()


@pytest.mark.parametrize("Cc", [2, 5])
def test_cross_entropy_is_torch(Ls, Cc):
    x, t = K.make_inputs("multiclass", Cc, 2, 33, 47, True)
    for kw in (dict(), dict(ignore_index=K.IGN), dict(ignore_index=K.IGN, label_smoothing=0.1), dict(label_smoothing=0.2)):
        tt = t if "ignore_index" in kw else t.clamp_max(Cc - 1)
        xd = x.double().requires_grad_()
        want = F.cross_entropy(xd, tt, **kw)
        want.backward()
        rf = R.evaluate(x, tt, Ls.CrossEntropyLoss(**kw)._as_sum().spec(Cc))
        assert abs(float(rf["total"]) - float(want.detach())) <= 1e-12 * abs(float(want.detach()))
        assert (rf["dlogits"] - xd.grad).abs().max().item() <= 1e-10 * xd.grad.abs().max().item()


@pytest.mark.parametrize("mode,Cc", [("binary", 1), ("multilabel", 4)])
def test_bce_with_logits_is_torch(Ls, mode, Cc):
    x, y = K.make_inputs(mode, Cc, 2, 33, 47, False)
    for pw in (None, 3.0, [0.5 + c for c in range(Cc)]):
        xd = x.double().requires_grad_()
        pwt = None if pw is None else torch.tensor(pw, dtype=torch.float64).reshape(-1).view(1, -1, 1, 1)
        want = F.binary_cross_entropy_with_logits(xd, y.double(), pos_weight=pwt)
        want.backward()
        rf = R.evaluate(x, y, Ls.BCEWithLogitsLoss(pos_weight=pw)._as_sum().spec(Cc))
        assert abs(float(rf["total"]) - float(want.detach())) <= 1e-12 * abs(float(want.detach()))
        assert (rf["dlogits"] - xd.grad).abs().max().item() <= 1e-10 * xd.grad.abs().max().item()


@pytest.mark.parametrize("mode,Cc", [("multilabel", 4), ("multiclass", 5)])
def test_default_dice_equals_multiclass_ref(Ls, mode, Cc):
    x, tgt = K.make_inputs(mode, Cc, 3, 40, 56, False)
    px = Ls.CrossEntropyLoss() if mode == "multiclass" else Ls.BCEWithLogitsLoss()
    rf = R.evaluate(x, tgt, (px + Ls.DiceLoss(mode)).spec(Cc))
    total, pix, dice, dl = (MR.multiclass if mode == "multiclass" else MR.multilabel)(x, tgt)
    assert abs(float(rf["dice"]) - float(dice)) <= 1e-14 and abs(float(rf["pix"]) - float(pix)) <= 1e-13
    assert abs(float(rf["total"]) - float(total)) <= 1e-13
    assert (rf["dlogits"] - dl).abs().max().item() <= 1e-12 * dl.abs().max().item()


def test_everything_ignored_is_zero_not_nan(Ls):
    for mode, Cc in (("multilabel", 4), ("multiclass", 3)):
        x, tgt = K.make_inputs(mode, Cc, 2, 33, 47, True)
        tgt = torch.full_like(tgt, K.IGN)
        for name in K.case_names():
            rf = R.evaluate(x, tgt, K.build(Ls, name, mode, Cc, True).spec(Cc))
            if name == "pix_soft":
                continue            # mean over ALL entries: zero as well, checked below
            assert float(rf["total"]) == 0.0 and (rf["dlogits"] == 0).all(), name
        rf = R.evaluate(x, tgt, K.build(Ls, "pix_soft", mode, Cc, True).spec(Cc))
        assert float(rf["total"]) == 0.0 and (rf["dlogits"] == 0).all()


# ------------------------------------------------------------------------------------------ constructors, refusals, algebra
def test_accepted_constructors_build(Ls):
    for mode, Cc in K.MODE_C:
        for name in K.case_names():
            for ign in (False, True):
                S = K.build(Ls, name, mode, Cc, ign)._as_sum()
                spec = S.spec(Cc)
                alone = S.mode is None                # a BCE term on its own: binary or multilabel by C
                assert spec["mode"] == ("binary" if alone and Cc == 1 else mode)
                assert spec["ignore_index"] == (K.IGN if ign else (-100 if name == "pix_nn" and mode == "multiclass" else None))
                cfg = S.cfg(Cc)
                assert cfg.struct_size == C.sizeof(cfg) and cfg.terms != 0
    d = Ls.DiceLoss("multiclass", classes=[2, 0], log_loss=True, smooth=1.0, ignore_index=7, eps=1e-6)
    assert d.opts == dict(smooth=1.0, eps=1e-6, log_loss=True, classes=[0, 2]) and d.ignore_index == 7 and d.kind == "dice"
    j = Ls.JaccardLoss("binary", None, False, True, 0.0, 1e-7)           # smp's positional order: eps is the sixth
    assert j.opts["eps"] == 1e-7 and j.ignore_index is None
    t = Ls.TverskyLoss("multilabel", None, False, True, 0.0, None, 1e-7, 0.3, 0.7, 2.0)
    assert (t.opts["alpha"], t.opts["beta"], t.opts["gamma"]) == (0.3, 0.7, 2.0)
    f = Ls.FocalLoss("binary", 0.25, 2.0, 255)
    assert f.opts == dict(alpha=0.25, gamma=2.0) and f.ignore_index == 255
    assert Ls.SoftBCEWithLogitsLoss().ignore_index == -100 and Ls.SoftCrossEntropyLoss().ignore_index == -100
    assert Ls.SoftBCEWithLogitsLoss(ignore_index=None).ignore_index is None
    assert Ls.CrossEntropyLoss().opts["denom"] == "valid" and Ls.SoftCrossEntropyLoss().opts["denom"] == "all"
    assert Ls.BCEWithLogitsLoss(pos_weight=torch.ones(1, 3, 1, 1) * 2).opts["pos_weight"] == [2.0, 2.0, 2.0]
    cfg = (Ls.BCEWithLogitsLoss(pos_weight=2.0) + Ls.DiceLoss("multilabel")).cfg(3)
    assert list(cfg.pos_weight)[:4] == [2.0, 2.0, 2.0, 0.0] and cfg.has_pos_weight == 1 and cfg.mode == 1 and cfg.terms == 1 | 4
    assert Ls.BCEWithLogitsLoss()._as_sum().cfg(1).mode == 0 and Ls.BCEWithLogitsLoss()._as_sum().cfg(4).mode == 1    # alone: by C
    cfg = Ls.DiceLoss("multiclass", classes=[0, 2])._as_sum().cfg(3)
    assert cfg.dice_classes == 0b101


def test_refusals(Ls):
    NI = NotImplementedError
    for ctor in (Ls.DiceLoss, Ls.JaccardLoss, Ls.TverskyLoss):
        with pytest.raises(NI, match="from_logits"):
            ctor("binary", from_logits=False)
        with pytest.raises(ValueError, match="mode"):
            ctor("other")
    with pytest.raises(NI, match="reduction"):
        Ls.FocalLoss("binary", reduction="sum")
    with pytest.raises(NI, match="reduction"):
        Ls.FocalLoss("binary", reduction=None)
    with pytest.raises(NI, match="normalized"):
        Ls.FocalLoss("binary", normalized=True)
    with pytest.raises(NI, match="reduced_threshold"):
        Ls.FocalLoss("binary", reduced_threshold=0.5)
    for g in (0.5, -1.0, 0.99):
        with pytest.raises(NI, match="gamma"):
            Ls.FocalLoss("binary", gamma=g)
    for g in (0.0, 0.5, 0.99):
        with pytest.raises(NI, match="gamma"):
            Ls.TverskyLoss("binary", gamma=g)
    Ls.FocalLoss("binary", gamma=0.0), Ls.FocalLoss("binary", gamma=1.0), Ls.TverskyLoss("binary", gamma=1.0)
    with pytest.raises(NI, match="weight"):
        Ls.SoftBCEWithLogitsLoss(weight=torch.ones(3))
    with pytest.raises(NI, match="reduction"):
        Ls.SoftBCEWithLogitsLoss(reduction="none")
    with pytest.raises(NI, match="reduction"):
        Ls.SoftCrossEntropyLoss(reduction="sum")
    with pytest.raises(NI, match="dim"):
        Ls.SoftCrossEntropyLoss(dim=-1)
    with pytest.raises(NI, match="Lovasz"):
        Ls.LovaszLoss("binary")
    with pytest.raises(NI, match="MCC"):
        Ls.MCCLoss()


def test_existing_losses_keep_their_refusals(vk):
    with pytest.raises(NotImplementedError):
        vk.multiclass.DiceLoss(mode="multiclass", ignore_index=255)
    with pytest.raises(NotImplementedError):
        vk.DiceLoss(mode="binary", smooth=1.0)
    with pytest.raises(NotImplementedError):
        vk.losses.DiceLoss(mode="binary", log_loss=True)


def test_loss_sum_algebra(Ls):
    a, b = Ls.FocalLoss("multiclass"), Ls.TverskyLoss("multiclass", ignore_index=255)
    S = 2 * a + b
    assert isinstance(S, Ls.LossSum) and [(w, t.kind) for w, t in S.terms] == [(2.0, "focal"), (1.0, "tversky")]
    assert S.mode == "multiclass" and S.ignore_index == 255                 # the term that has none takes the sum's
    assert [w for w, _ in (0.5 * S).terms] == [1.0, 0.5] and [w for w, _ in (S * 3).terms] == [6.0, 3.0]
    S3 = sum([a, b, Ls.CrossEntropyLoss(ignore_index=255)])
    assert set(S3.spec(4)["terms"]) == {"focal", "tversky", "pix"} and S3.spec(4)["terms"]["pix"]["denom"] == "valid"
    assert (Ls.BCEWithLogitsLoss() + Ls.DiceLoss("binary")).spec(1)["mode"] == "binary"
    with pytest.raises(ValueError, match="kind 'focal'"):
        a + Ls.FocalLoss("multiclass", gamma=1.0)
    with pytest.raises(ValueError, match="kind 'pix'"):
        Ls.CrossEntropyLoss() + Ls.SoftCrossEntropyLoss()
    with pytest.raises(ValueError, match="mode"):
        a + Ls.DiceLoss("multilabel")
    with pytest.raises(ValueError, match="mode"):
        Ls.CrossEntropyLoss() + Ls.DiceLoss("binary")
    with pytest.raises(ValueError, match="BCE"):
        Ls.BCEWithLogitsLoss() + Ls.DiceLoss("multiclass")
    with pytest.raises(ValueError, match="ignore_index"):
        Ls.DiceLoss("multiclass", ignore_index=0) + b
    with pytest.raises(ValueError, match="ignore_index"):
        Ls.CrossEntropyLoss() + b                                           # -100 against 255
    with pytest.raises(TypeError):
        a + 1.0
    with pytest.raises(TypeError):
        a * "2"
    with pytest.raises(ValueError, match="pos_weight"):
        Ls.BCEWithLogitsLoss(pos_weight=[1.0, 2.0])._as_sum().spec(3)
    with pytest.raises(ValueError, match="classes"):
        Ls.DiceLoss("multiclass", classes=[0, 5])._as_sum().spec(3)
    with pytest.raises(ValueError, match="binary"):
        Ls.DiceLoss("binary")._as_sum().spec(3)
    with pytest.raises(ValueError, match="multiclass"):
        Ls.DiceLoss("multiclass")._as_sum().spec(1)


def test_modules_check_shapes_then_refuse_cpu_tensors(vk, Ls):
    S = Ls.FocalLoss("multiclass") + Ls.DiceLoss("multiclass")
    with pytest.raises(ValueError, match="int64"):
        S(torch.zeros(2, 3, 8, 8), torch.zeros(2, 8, 8))
    with pytest.raises(ValueError, match="N,C,H,W"):
        S(torch.zeros(2, 3, 8), torch.zeros(2, 8, dtype=torch.int64))
    with pytest.raises(ValueError, match="broadcast"):
        Ls.DiceLoss("multilabel")(torch.zeros(2, 3, 8, 8), torch.zeros(2, 2, 8, 8))
    with pytest.raises(vk.VkError, match="no CPU fallback"):
        S(torch.zeros(2, 3, 8, 8, requires_grad=True), torch.zeros(2, 8, 8, dtype=torch.int64))
    with pytest.raises(vk.VkError, match="no CPU fallback"):
        Ls.DiceLoss("binary")(torch.zeros(2, 1, 8, 8), torch.zeros(2, 1, 8, 8))
    m = vk.multiclass.Unet(encoder_weights=None, classes=3)
    with pytest.raises(ValueError, match="not both"):
        m.loss_and_backward(torch.zeros(1, 3, 64, 64), torch.zeros(1, 64, 64, dtype=torch.int64), mode="multiclass", loss=S)
    with pytest.raises(TypeError):
        m.loss_and_backward(torch.zeros(1, 3, 64, 64), torch.zeros(1, 64, 64, dtype=torch.int64), loss=torch.nn.CrossEntropyLoss())
    with pytest.raises(NotImplementedError):
        Ls.seg_metrics(torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 8, 8), "multilabel", ignore_index=255)
    with pytest.raises(NotImplementedError):
        Ls.seg_metrics(torch.zeros(1, 3, 8, 8), torch.zeros(1, 8, 8, dtype=torch.int64), "multiclass", ignore_index=2)


# ------------------------------------------------------------------------------------------ C ABI, host side
def test_cfg_mirror_has_the_library_size(vk):
    L = vk.lib()
    assert C.sizeof(vk._lib.vk_seg_loss_cfg) == L.vk_seg_loss_cfg_size() > 0
    assert L.vk_seg_loss_workspace_bytes(2, 3, 64 * 64) >= 64 * 8 and L.vk_seg_loss_workspace_bytes(2, 17, 64) == 0
    assert L.vk_seg_loss_workspace_bytes(0, 1, 64) == 0


def test_vk_seg_loss_host_argument_errors(vk, Ls):
    L = vk.lib()

    def call(cfg, Cc, N=2, HW=64, ptrs=False, wsb=1 << 20):
        p = 4096 if ptrs else None
        return L.vk_seg_loss(None if cfg is None else C.byref(cfg), N, Cc, HW, p, p, p, wsb, p, None, 1.0, None)

    good = (Ls.FocalLoss("multiclass") + Ls.TverskyLoss("multiclass")).cfg(3)
    assert call(None, 3) < 0 and b"null configuration" in L.vk_last_error_string()
    assert call(good, 3) < 0 and b"null argument" in L.vk_last_error_string()        # the configuration passes, the buffers do not

    def bad(match, Cc=3, **kw):
        cfg = (Ls.SoftCrossEntropyLoss() + Ls.FocalLoss("multiclass") + Ls.DiceLoss("multiclass") + Ls.JaccardLoss("multiclass")
               + Ls.TverskyLoss("multiclass")).cfg(3)
        for k, v in kw.items():
            setattr(cfg, k, v)
        assert call(cfg, Cc) < 0
        assert match in L.vk_last_error_string(), (match, L.vk_last_error_string())

    bad(b"struct_size", struct_size=4)
    bad(b"bad mode", mode=7)
    bad(b"binary needs C == 1", mode=0)
    bad(b"multiclass needs C >= 2", Cc=1)
    bad(b"classes must be 1..16", Cc=17)
    bad(b"terms", terms=0)
    bad(b"terms", terms=64)
    bad(b"weight is not finite", w_focal=float("nan"))
    bad(b"weight is not finite", w_dice=float("inf"))
    bad(b"smooth_factor", pix_smooth=1.5)
    bad(b"pos_weight", has_pos_weight=1)
    bad(b"focal gamma", focal_gamma=0.5)
    bad(b"dice eps", dice_eps=0.0)
    bad(b"jaccard eps", jaccard_eps=-1.0)
    bad(b"tversky smooth", tversky_smooth=float("nan"))
    bad(b"classes mask", dice_classes=1 << 3)
    bad(b"tversky gamma", tversky_gamma=0.5)
    cfg = Ls.BCEWithLogitsLoss(pos_weight=2.0)._as_sum().cfg(2)
    cfg.pos_weight[1] = float("inf")
    assert call(cfg, 2) < 0 and b"pos_weight[1]" in L.vk_last_error_string()
    assert call(good, 3, N=0, ptrs=True) < 0 and b"bad shape" in L.vk_last_error_string()
    assert call(good, 3, ptrs=True, wsb=8) < 0 and b"workspace" in L.vk_last_error_string()
    # a plan that is not bound refuses before anything is launched
    assert L.vk_unet_loss_cfg(None, C.byref(good), None, None, None, 1.0, None) < 0


def test_plan_scratch_goes_behind_everything(vk):
    """the new scratch is the last region of every plan's workspace (classes == 1 included): the plan grows by at least the loss's
    scratch (vk_unet_workspace_bytes is the only host-visible trace of the layout)"""
    L = vk.lib()
    for classes in (1, 3):
        for training in (0, 1):
            cfg = vk._lib.vk_unet_config(2, 64, vk._lib.VK_BF16, training)
            h = C.c_void_p()
            vk._lib.check(L.vk_unet_create_ex(C.byref(cfg), classes, C.byref(h)))
            try:
                assert L.vk_unet_workspace_bytes(h) >= L.vk_seg_loss_workspace_bytes(2, classes, 64 * 64) > 0
            finally:
                L.vk_unet_destroy(h)
