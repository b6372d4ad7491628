"""vk.keypoints losses, the parts that need no GPU: the float64 restatement (tests/keypoints_loss_ref.py) against torch autograd and
torch.nn.BCEWithLogitsLoss, hand values, positive_threshold on the restated targets, the loss algebra and its refusals, the ctypes
structure, every host-side argument error of vk_kp_loss and vk_unet_loss_kp through the built library, and the argument errors of
ObjectMetrics and Segmenter that come before any device work."""
import ctypes as C
import importlib
import math

import numpy as np
import pytest
import torch

import keypoints_loss_ref as R
import keypoints_ref as KR

vk = importlib.import_module("vickers-hardness-unet_amd")
KP, Ls, L_ = vk.keypoints, vk.seglosses, vk._lib


# ------------------------------------------------------------------------------------------------ the restatement
def _torch_heat(x, y, alpha, beta, thr):
    """the definition written naively on torch float64: log_sigmoid and powers of sigmoid"""
    p = torch.sigmoid(x)
    pos = y >= thr
    e = torch.where(pos, -(1 - p) ** alpha * torch.nn.functional.logsigmoid(x),
                    -(1 - y) ** beta * p ** alpha * torch.nn.functional.logsigmoid(-x))
    return e.sum() / max(int(pos.sum()), 1), int(pos.sum())


@pytest.mark.parametrize("alpha,beta", [(2, 4), (0, 0), (1, 3), (4, 0), (8, 8)])
def test_heat_restatement_equals_float64_autograd(alpha, beta):
    g = torch.Generator().manual_seed(10 * alpha + beta)
    N, Cc, HW = 2, 3, 97
    x = (torch.rand(N, Cc, HW, generator=g, dtype=torch.float64) * 16.0 - 8.0).requires_grad_()
    y = torch.rand(N, Cc, HW, generator=g, dtype=torch.float64)
    y[torch.rand(N, Cc, HW, generator=g) < 0.1] = 1.0
    thr = 0.9
    vals = [_torch_heat(x[:, c], y[:, c], alpha, beta, thr) for c in (0, 2)]
    loss = 0.75 * (vals[0][0] + vals[1][0]) / 2
    loss.backward()
    c = R.cfg(heat=[0, 2], w_heat=0.75, alpha=alpha, beta=beta, thr=thr)
    thr32 = c["thr"]
    assert not ((y.numpy() >= thr) != (y.numpy() >= thr32)).any()           # no entry between 0.9 and float32(0.9)
    r = R.evaluate(x.detach().numpy(), y.numpy(), c)
    assert abs(r["total"] - loss.item()) <= 1e-13 * abs(loss.item())
    assert r["positives"][0] == vals[0][1] and r["positives"][2] == vals[1][1] and r["positives"][1] == 0
    gmax = x.grad.abs().max().item()
    assert gmax > 0 and np.abs(r["grad"] - x.grad.numpy()).max() <= 1e-13 * gmax
    assert (r["grad"][:, 1] == 0).all()


def test_hand_values():
    ln2 = math.log(2.0)
    r = R.evaluate(np.zeros((1, 1, 1)), np.ones((1, 1, 1)), R.cfg(heat=[0], alpha=2, beta=4))
    assert abs(r["heat"] - 0.25 * ln2) <= 1e-15 and r["positives"][0] == 1 and r["total"] == r["heat"]
    r = R.evaluate(np.zeros((1, 1, 1)), np.full((1, 1, 1), 0.5), R.cfg(heat=[0], alpha=2, beta=4))
    assert abs(r["heat"] - (1.0 / 16.0) * (1.0 / 4.0) * ln2) <= 1e-15 and r["positives"][0] == 0          # no positive: divided by 1
    x = np.array([[[0.3, -1.2, 2.0]]])
    y = np.array([[[0.2, 0.0, 0.7]]])
    r = R.evaluate(x, y, R.cfg(heat=[0], alpha=1, beta=1))
    v, _, pos = R.heat_elements(x[:, 0], y[:, 0], R.cfg(heat=[0], alpha=1, beta=1))
    assert not pos.any() and abs(r["heat"] - v.sum()) <= 1e-15


@pytest.mark.parametrize("pw", [None, [3.0, 0.25]])
def test_bce_restatement_equals_torch(pw):
    g = torch.Generator().manual_seed(3)
    N, HW = 2, 61
    x = (torch.rand(N, 3, HW, generator=g, dtype=torch.float64) * 20.0 - 10.0).requires_grad_()
    y = torch.rand(N, 3, HW, generator=g, dtype=torch.float64)
    planes = [0, 2]
    tw = None if pw is None else torch.tensor(pw, dtype=torch.float64).reshape(1, 2, 1)
    loss = 0.5 * torch.nn.BCEWithLogitsLoss(pos_weight=tw)(x[:, planes], y[:, planes])
    loss.backward()
    full = None if pw is None else [pw[0], 1.0, pw[1]]
    r = R.evaluate(x.detach().numpy(), y.numpy(), R.cfg(bce=planes, w_bce=0.5, pos_weight=full))
    assert abs(r["total"] - loss.item()) <= 1e-13 * abs(loss.item()) and abs(r["bce"] - 2.0 * loss.item()) <= 1e-13
    assert np.abs(r["grad"] - x.grad.numpy()).max() <= 1e-13 * x.grad.abs().max().item()
    assert (r["grad"][:, 1] == 0).all() and (r["positives"] == 0).all()


# ------------------------------------------------------------------------------------------------ positive_threshold
@pytest.mark.parametrize("sigma", [2.0, 1.0, 0.25])
def test_positive_threshold_gives_one_to_four_positives_everywhere_in_the_pixel(sigma):
    thr = KP.positive_threshold(sigma)
    tab = KR.gaussian_table(sigma)
    assert thr == float(tab[128]) and 0.0 < thr < 1.0
    size, c = 9, 4
    seen = set()
    for fy in range(16):
        for fx in range(16):
            m = KR.render_vertices([(16 * c + fx - 8, 16 * c + fy - 8)], size, size, tab)
            n = int((m >= np.float32(thr)).sum())
            assert 1 <= n <= 4, (fx, fy, n)
            seen.add(n)
    assert seen == {1, 2, 4}                               # the interior, an edge midway between two pixels, the corner between four
    m = KR.render_vertices([(16 * c, 16 * c)], size, size, tab)
    assert int((m >= np.float32(1.0)).sum()) == 1          # an integer vertex with the default threshold
    m = KR.render_vertices([(16 * c + 1, 16 * c)], size, size, tab)
    assert int((m >= np.float32(1.0)).sum()) == 0          # one sixteenth off: the default threshold finds nothing


def test_positive_threshold_refuses_a_disc_that_ends_before_the_pixel():
    with pytest.raises(ValueError, match="below 12"):
        KP.positive_threshold(0.2)
    with pytest.raises(ValueError, match="below 12"):
        KP.positive_threshold(2.0, cutoff=0.3)
    assert KP.positive_threshold(0.25) == float(KR.gaussian_table(0.25)[128])          # 16 * 3 * 0.25 = 12: the last that fits


# ------------------------------------------------------------------------------------------------ terms and algebra
def test_constructors():
    h = KP.HeatmapFocalLoss()
    assert (h.planes, h.alpha, h.beta, h.pos_threshold) == ((1,), 2, 4, 1.0)
    b = KP.PlaneBCE()
    assert b.planes == (0,) and b.pos_weight is None
    assert KP.PlaneBCE([2, 0], pos_weight=[3.0, 5.0]).pos_weight == {2: 3.0, 0: 5.0}
    assert KP.PlaneBCE([2, 0], pos_weight=4.0).pos_weight == {2: 4.0, 0: 4.0}
    for bad in (dict(planes=[]), dict(planes=[16]), dict(planes=[-1]), dict(planes=[1, 1]), dict(alpha=9), dict(beta=-1), dict(alpha=2.0),
                dict(pos_threshold=0.0), dict(pos_threshold=1.5), dict(pos_threshold=float("nan"))):
        with pytest.raises(ValueError):
            KP.HeatmapFocalLoss(**bad)
    for bad in (dict(planes=[]), dict(planes=[0, 16]), dict(pos_weight=[1.0, 2.0]), dict(pos_weight=0.0), dict(pos_weight=-1.0),
                dict(pos_weight=float("inf"))):
        with pytest.raises(ValueError):
            KP.PlaneBCE(**bad)


def test_algebra_and_configuration():
    heat = KP.HeatmapFocalLoss([1], pos_threshold=0.5)
    bce = KP.PlaneBCE([0], pos_weight=3.0)
    dice = Ls.DiceLoss("multilabel", classes=[0])
    for S in (bce + dice + 0.5 * heat, dice + bce + heat * 0.5, sum([0.5 * heat, dice, bce]), (0.5 * heat + bce) + dice):
        assert isinstance(S, KP.LossSum) and S.heat[0] == 0.5 and S.bce[0] == 1.0 and S.seg.mode == "multilabel"
        c = S.kp_cfg(2)
        assert (c.struct_size, c.heat_planes, c.bce_planes, c.w_heat, c.w_bce, c.alpha, c.beta, c.pos_threshold, c.has_pos_weight) == (
            C.sizeof(L_.vk_kp_loss_cfg), 2, 1, 0.5, 1.0, 2, 4, 0.5, 1)
        assert list(c.pos_weight)[:3] == [3.0, 1.0, 1.0]
        assert S.seg_cfg(2).terms == 4 and S.seg_cfg(2).dice_classes == 1 and S.resolved_mode(2) == "multilabel"
    D = 2.0 * (bce + dice + 0.5 * heat)
    assert D.heat[0] == 1.0 and D.bce[0] == 2.0 and [w for w, _ in D.seg.terms] == [2.0]
    alone = 0.25 * heat
    assert isinstance(alone, KP.LossSum) and alone.seg is None and alone.seg_cfg(2) is None and alone.kp_cfg(2).bce_planes == 0
    assert alone.resolved_mode(1) == "binary" and alone.resolved_mode(3) == "multilabel"
    assert heat.cfg(2).heat_planes == 2 and bce.cfg(1).bce_planes == 1
    one = KP.HeatmapFocalLoss([0]) + Ls.BCEWithLogitsLoss()                   # a mode-less BCE part: binary on one plane
    assert one.resolved_mode(1) == "binary" and one.seg_cfg(1).mode == 0


def test_refusals():
    heat, bce = KP.HeatmapFocalLoss([1]), KP.PlaneBCE([0])
    with pytest.raises(ValueError, match="overlap"):
        KP.HeatmapFocalLoss([0, 1]) + bce
    with pytest.raises(ValueError, match="two heat"):
        heat + KP.HeatmapFocalLoss([2])
    with pytest.raises(ValueError, match="two plane BCE"):
        (heat + bce) + KP.PlaneBCE([2])
    with pytest.raises(ValueError, match="multiclass"):
        Ls.CrossEntropyLoss() + heat
    with pytest.raises(ValueError, match="multiclass"):
        heat + Ls.DiceLoss("multiclass")
    lov = vk.lovasz.LovaszLoss("multilabel")
    for make in (lambda: lov + heat, lambda: heat + lov, lambda: (Ls.BCEWithLogitsLoss() + lov) + bce, lambda: bce + (Ls.DiceLoss("multilabel") + lov)):
        with pytest.raises(ValueError, match="Lovasz"):
            make()
    with pytest.raises(ValueError, match="kind"):
        (heat + Ls.DiceLoss("multilabel")) + Ls.DiceLoss("multilabel")
    with pytest.raises(ValueError, match="mode"):
        (heat + Ls.DiceLoss("multilabel")) + Ls.JaccardLoss("binary")
    with pytest.raises(ValueError, match="plane >= C"):
        heat.cfg(1)
    with pytest.raises(ValueError, match="plane >= C"):
        (KP.PlaneBCE([2]) + KP.HeatmapFocalLoss([0])).kp_cfg(2)
    with pytest.raises(ValueError, match="one channel"):
        (KP.HeatmapFocalLoss([0]) + Ls.DiceLoss("binary")).kp_cfg(2)
    with pytest.raises(TypeError):
        heat + 1.0
    with pytest.raises(TypeError):
        heat * "2"
    with pytest.raises(ValueError, match="finite"):
        heat * float("inf")
    with pytest.raises(TypeError):
        KP.LossSum(torch.nn.BCEWithLogitsLoss(), (1.0, heat), None)
    with pytest.raises(ValueError, match="neither"):
        KP.LossSum(Ls.DiceLoss("multilabel"), None, None)
    with pytest.raises(TypeError):
        KP.LossSum(None, (1.0, bce), None)
    # the refusals of the other front ends are what they were
    with pytest.raises(TypeError):
        Ls.DiceLoss("binary") + 1.0
    with pytest.raises(ValueError, match="two Lovasz"):
        lov + vk.lovasz.LovaszLoss("multilabel")


def test_cpu_tensors_and_wrong_targets_are_refused():
    S = KP.PlaneBCE([0]) + KP.HeatmapFocalLoss([1])
    with pytest.raises(vk.VkError, match="no CPU fallback"):
        S(torch.zeros(2, 2, 8, 8, requires_grad=True), torch.zeros(2, 2, 8, 8))
    with pytest.raises(ValueError, match="broadcast"):
        S(torch.zeros(2, 2, 8, 8), torch.zeros(2, 3, 8, 8))
    with pytest.raises(ValueError, match="plane >= C"):
        S(torch.zeros(2, 1, 8, 8), torch.zeros(2, 1, 8, 8))
    m = vk.multiclass.Unet(encoder_weights=None, classes=2)
    with pytest.raises(vk.VkError, match="no CPU fallback"):                  # the configuration is accepted; the input is refused
        m.loss_and_backward(torch.zeros(1, 3, 64, 64), torch.zeros(1, 2, 64, 64), loss=S)
    with pytest.raises(ValueError, match="not both"):
        m.loss_and_backward(torch.zeros(1, 3, 64, 64), torch.zeros(1, 2, 64, 64), mode="multilabel", loss=S)
    with pytest.raises(ValueError, match="plane >= C"):
        vk.Unet(encoder_weights=None, classes=1).loss_and_backward(torch.zeros(1, 3, 64, 64), torch.zeros(1, 1, 64, 64), loss=S)


# ------------------------------------------------------------------------------------------------ the C ABI on the host
def _kcfg(heat=2, bce=1, w_heat=1.0, w_bce=1.0, alpha=2, beta=4, thr=1.0, has_pw=0, pw=None, size=None):
    c = L_.vk_kp_loss_cfg()
    c.struct_size = C.sizeof(c) if size is None else size
    c.heat_planes, c.bce_planes, c.w_heat, c.w_bce, c.alpha, c.beta, c.pos_threshold, c.has_pos_weight = heat, bce, w_heat, w_bce, alpha, beta, thr, has_pw
    for i in range(16):
        c.pos_weight[i] = 1.0 if pw is None else pw[i] if i < len(pw) else 1.0
    return c


def test_structure_size_and_workspace_bytes():
    L = vk.lib()
    assert C.sizeof(L_.vk_kp_loss_cfg) == L.vk_kp_loss_cfg_size() == 100 and L_.VK_KP_LOSS_MAX_EXP == 8
    assert L.vk_kp_loss_workspace_bytes(1, 1, 1) == 16 * 8 + 16
    assert L.vk_kp_loss_workspace_bytes(2, 2, 4096) == 16 * 8 + 2 * 2 * 2 * 16               # two workgroups per plane
    assert L.vk_kp_loss_workspace_bytes(32, 2, 512 * 512) == 16 * 8 + 32 * 2 * 32 * 16
    for N, Cc, HW in [(0, 1, 8), (1, 0, 8), (1, 17, 8), (1, 1, 0), (-1, 1, 8), (1, 1, (1 << 28) + 1), (4096, 16, 8), (8, 1, 1 << 28),
                      (2, 16, 1 << 26)]:
        assert L.vk_kp_loss_workspace_bytes(N, Cc, HW) == 0, (N, Cc, HW)
    assert L.vk_kp_loss_workspace_bytes(7, 1, 1 << 28) > 0                                    # 7 x 2^28 <= 2^31 - 1


def test_host_side_argument_errors():
    L = vk.lib()
    err = L.vk_last_error_string
    big = 1 << 40
    SENT = 7.0
    x = (C.c_float * 256)(*([SENT] * 256))
    y = (C.c_float * 256)(*([SENT] * 256))
    dl = (C.c_float * 256)(*([SENT] * 256))
    out = (C.c_float * 8)(*([SENT] * 8))
    pos = (C.c_int64 * 16)(*([7] * 16))
    ws = (C.c_double * 64)(*([SENT] * 64))
    A = C.addressof

    def call(cfg, N=2, Cc=2, HW=32, x_=A(x), y_=A(y), ws_=A(ws), wsb=big, out_=A(out), pos_=A(pos), dl_=A(dl), gs=1.0, acc=0):
        return L.vk_kp_loss(cfg, N, Cc, HW, x_, y_, ws_, wsb, out_, pos_, dl_, gs, acc, None)

    nan, inf = float("nan"), float("inf")
    cases = [
        (dict(cfg=None), b"null configuration"), (dict(cfg=_kcfg(size=96)), b"struct_size"), (dict(cfg=_kcfg(), Cc=0), b"1..16"),
        (dict(cfg=_kcfg(heat=1, bce=0), Cc=17), b"1..16"), (dict(cfg=_kcfg(heat=0, bce=0)), b"empty"),
        (dict(cfg=_kcfg(heat=3, bce=1)), b"overlap"), (dict(cfg=_kcfg(heat=4, bce=1)), b"plane >= C"),
        (dict(cfg=_kcfg(heat=2, bce=1 << 16), Cc=16), b"plane >= C"), (dict(cfg=_kcfg(heat=1 << 31, bce=1), Cc=16), b"plane >= C"),
        (dict(cfg=_kcfg(w_heat=nan)), b"weight"), (dict(cfg=_kcfg(w_bce=inf)), b"weight"), (dict(cfg=_kcfg(w_heat=-inf)), b"weight"),
        (dict(cfg=_kcfg(alpha=-1)), b"exponents"), (dict(cfg=_kcfg(alpha=9)), b"exponents"), (dict(cfg=_kcfg(beta=9)), b"exponents"),
        (dict(cfg=_kcfg(beta=-(1 << 31))), b"exponents"),
        (dict(cfg=_kcfg(thr=0.0)), b"pos_threshold"), (dict(cfg=_kcfg(thr=-0.5)), b"pos_threshold"),
        (dict(cfg=_kcfg(thr=1.0000001)), b"pos_threshold"), (dict(cfg=_kcfg(thr=nan)), b"pos_threshold"),
        (dict(cfg=_kcfg(has_pw=2)), b"has_pos_weight"),
        (dict(cfg=_kcfg(has_pw=1, pw=[1.0, 0.0])), b"pos_weight[1]"), (dict(cfg=_kcfg(has_pw=1, pw=[-2.0])), b"pos_weight[0]"),
        (dict(cfg=_kcfg(has_pw=1, pw=[nan])), b"pos_weight[0]"), (dict(cfg=_kcfg(has_pw=1, pw=[1.0, inf])), b"pos_weight[1]"),
        (dict(cfg=_kcfg(), N=0), b"shape"), (dict(cfg=_kcfg(), HW=0), b"shape"), (dict(cfg=_kcfg(), HW=-4), b"shape"),
        (dict(cfg=_kcfg(), N=40000), b"shape"), (dict(cfg=_kcfg(), HW=(1 << 28) + 4), b"shape"),
        (dict(cfg=_kcfg(), N=4, HW=1 << 28), b"2^31"), (dict(cfg=_kcfg(heat=1 << 15, bce=1), N=2, Cc=16, HW=1 << 26), b"2^31"),
        (dict(cfg=_kcfg(), gs=nan), b"grad_scale"), (dict(cfg=_kcfg(), gs=inf), b"grad_scale"),
        (dict(cfg=_kcfg(), acc=2), b"accumulate"), (dict(cfg=_kcfg(), acc=-1), b"accumulate"),
        (dict(cfg=_kcfg(), x_=None), b"null argument"), (dict(cfg=_kcfg(), y_=None), b"null argument"),
        (dict(cfg=_kcfg(), out_=None), b"null argument"), (dict(cfg=_kcfg(), ws_=None), b"null argument"),
        (dict(cfg=_kcfg(), wsb=16 * 8 + 4 * 16 - 1), b"workspace"), (dict(cfg=_kcfg(), wsb=0), b"workspace"),
        (dict(cfg=_kcfg(), ws_=A(ws) + 4), b"workspace"),
    ]
    for kw, word in cases:
        assert call(**kw) == -1 and word in err(), (kw, err())
    # pos_weight beyond C is not looked at; a pos_weight without the flag neither
    assert call(_kcfg(has_pw=1, pw=[1.0, 2.0, nan]), x_=None) == -1 and b"null argument" in err()
    assert call(_kcfg(has_pw=0, pw=[nan]), x_=None) == -1 and b"null argument" in err()
    # vk_unet_loss_kp: the plan and the pointers first
    for args in [(None, None, _kcfg(), 8, 8, 8, big, 8), (8, None, None, 8, 8, 8, big, 8)]:
        assert L.vk_unet_loss_kp(*args, 1.0, None) == -1 and b"vk_unet_loss_kp" in err()
    for buf in (x, y, dl, out, ws):
        assert all(v == SENT for v in buf)
    assert all(v == 7 for v in pos)


def test_unet_loss_kp_argument_errors_on_a_created_plan():
    """A plan is created on the host (nothing is launched); an unbound plan is refused before anything else is looked at."""
    L = vk.lib()
    h = C.c_void_p()
    cfg = L_.vk_unet_config(2, 64, L_.VK_F32, 1, 64)
    assert L.vk_unet_create_ex(C.byref(cfg), 2, C.byref(h)) == 0
    try:
        assert L.vk_unet_loss_kp(h, None, _kcfg(), 8, 8, 8, 1 << 40, 8, 1.0, None) == -1
        assert b"not bound" in L.vk_last_error_string()
    finally:
        L.vk_unet_destroy(h)


# ------------------------------------------------------------------------------------------------ the read-out's front doors
def test_object_metrics_argument_errors():
    OM = vk.instances.ObjectMetrics
    with pytest.raises(ValueError, match="kind"):
        OM(refine=dict(kind="heat"))
    with pytest.raises(ValueError, match="sigma"):
        OM(refine=dict(kind="keypoints"))
    with pytest.raises(ValueError, match="sigma"):
        OM(refine=dict(kind="keypoints", sigma=0.0))
    om = OM(fit="quad", refine=dict(kind="keypoints", sigma=2.0, search=4))
    assert om.refine == dict(search=4) and om.refine_kind == "keypoints" and om.kp_sigma == 2.0
    prob = torch.zeros(1, 16, 16)
    with pytest.raises(ValueError, match="heat"):
        om.update(prob, prob)
    with pytest.raises(ValueError, match="heat"):
        om.update(prob, prob, heat=torch.zeros(1, 8, 8))
    for other in (OM(fit="quad"), OM(fit="quad", refine=dict(method="corner")), OM(fit="quad", refine=dict(kind="subpix", method="corner"))):
        assert other.refine_kind == "subpix" and (other.refine is None or other.refine == dict(method="corner"))
        with pytest.raises(ValueError, match="kind='keypoints'"):
            other.update(prob, prob, heat=prob)
    with pytest.raises(vk.VkError, match="no CPU fallback"):                   # the checks above come first; then the device is asked for
        om.update(prob, prob, heat=prob)


def test_segmenter_argument_errors():
    img = np.zeros((40, 50, 3), np.uint8)
    two = vk.Segmenter(vk.multiclass.Unet(encoder_weights=None, classes=2), img_size=64, device="cpu")
    for call in (two.measure, two.render):
        with pytest.raises(ValueError, match="zoom=False"):
            call(img, method="heatmap")
        with pytest.raises(ValueError, match="zoom=False"):
            call(img, method="heatmap", zoom=True)
    one = vk.Segmenter(vk.Unet(encoder_weights=None, classes=1), img_size=64, device="cpu")
    for call in (one.measure, one.render):
        with pytest.raises(ValueError, match="heatmap plane"):
            call(img, method="heatmap", zoom=False)
