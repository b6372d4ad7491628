"""The loss kernels on the MI355X (-m gpu) at the workgroup counts real batches take: vk_seg_loss, vk_kp_loss, vk_multilabel_loss and
vk_multiclass_loss through the C ABI on the cases of tests/loss_grid_cases.py (nbx in {1, 2, 3, 21, 42, 43, 52, 64}, one to seventeen
trips of the finalize row loops), vk_lovasz_loss past the launch caps of k_lv_bad and k_lv_softmax_bwd, and the fused step at 128 x 128.

Per case: the workspace size equals what the nbx rules predict, and the call runs on exactly that many never-cleared bytes before a
guard; every reported component is within the project's bar of the float64 reference (1e-5 |ref| + 1e-6; keypoints_loss_cases.bounds
for vk_kp_loss); dlogits, prefilled with a sentinel, is finite, written everywhere, exactly 0 on ignored and bad-label pixels and
within 1e-4 grad_scale max|ref| (the bounds grid for vk_kp_loss) at grad_scale 1 and 1024; a second call gives the same bits.
tests/test_loss_grid_cpu.py proves that a dropped or misplaced row of partials cannot stay inside these bars."""
import copy
import ctypes as C
import importlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import keypoints_loss_cases as KC
import loss_grid_cases as G
import lovasz_ref as LR
import multiclass_ref as MR
import seglosses_cases as K
import seglosses_ref as SR

pytestmark = pytest.mark.gpu
vk = importlib.import_module("vickers-hardness-unet_amd")
Ls, Lv, L_ = vk.seglosses, vk.lovasz, vk._lib

SENT = 12345.0                 # no gradient here comes near it
GUARD = 4096                   # bytes after the workspace
GUARD_BYTE = 0xA5
SCALES = (1.0, 1024.0)


def dev():
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream().cuda_stream


class _Workspace:
    """exactly `nbytes` never-cleared bytes (every double a NaN, every count -1), then a guard"""

    def __init__(self, nbytes: int):
        assert nbytes > 0
        self.nbytes = nbytes
        self.buf = torch.full((nbytes + GUARD,), GUARD_BYTE, dtype=torch.uint8, device=dev())
        self.buf[:nbytes] = 0xFF
        assert self.buf.data_ptr() % 16 == 0

    def ptr(self):
        return self.buf.data_ptr()

    def intact(self):
        return bool((self.buf[self.nbytes:] == GUARD_BYTE).all())


def _value_check(tag, got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err, bar = np.abs(got - want), 1e-5 * np.abs(want) + 1e-6
    print("GRID %s values: worst error %.3g of its bar" % (tag, float((err / bar).max())))
    assert (err <= bar).all(), (tag, got.tolist(), want.tolist())


def _grad_check(tag, dl, ref_g, gs, dead=None):
    """dl float32 from the device (prefilled with SENT), ref_g float64 at grad_scale 1"""
    assert np.isfinite(dl).all() and not (dl == np.float32(SENT)).any(), tag
    gmax = float(np.abs(ref_g).max())
    err = float(np.abs(dl.astype(np.float64) - gs * ref_g).max())
    print("GRID %s gs=%g gradient: error %.3g of its bar (max|ref| %.3g)" % (tag, gs, err / (1e-4 * gs * gmax), gmax))
    assert gmax > 0 and err <= 1e-4 * gs * gmax, (tag, gs, err, gmax)
    if dead is not None:
        assert dead.any() and (dl[dead] == 0).all(), tag


# ------------------------------------------------------------------------------------------------ vk_seg_loss
def _seg_call(cfg, N, Cc, HW, xd, td, ws, gs):
    L = vk.lib()
    out = torch.full((8,), 5.0, device=dev())
    dl = torch.full_like(xd, SENT)
    L_.check(L.vk_seg_loss(cfg, N, Cc, HW, xd.data_ptr(), td.data_ptr(), ws.ptr(), ws.nbytes, out.data_ptr(), dl.data_ptr(), gs,
                           _stream()), "vk_seg_loss")
    torch.cuda.synchronize()
    return out.cpu().numpy(), dl.cpu().numpy()


def _seg_setup(case):
    N, Cc, HW = case["N"], case["C"], case["HW"]
    need = vk.lib().vk_seg_loss_workspace_bytes(N, Cc, HW)
    assert need == G.seg_workspace_bytes(N, Cc, HW), (need, G.seg_workspace_bytes(N, Cc, HW))
    x, t = G.inputs(case, True)
    return N, Cc, HW, x, t, torch.from_numpy(x).to(dev()), torch.from_numpy(t).to(dev()), _Workspace(need)


def _check_seg(case, name):
    N, Cc, HW, x, t, xd, td, ws = _seg_setup(case)
    mode = G.seg_mode(case)
    S = K.build(Ls, name, mode, Cc, True)._as_sum()
    cfg, spec = S.cfg(Cc), S.spec(Cc)
    rf = SR.evaluate(torch.from_numpy(x), torch.from_numpy(t), spec)
    want, ref_g = SR.components(rf).numpy(), rf["dlogits"].numpy()
    dead = np.broadcast_to((t == G.IGN)[:, None, :], x.shape) if mode == "multiclass" else t == G.IGN
    tag = "%s %s" % (case["id"], name)
    for gs in SCALES:
        out, dl = _seg_call(cfg, N, Cc, HW, xd, td, ws, gs)
        _value_check(tag, out[:6], want)
        assert out[6] == 0.0 and out[7] == 0.0
        _grad_check(tag, dl, ref_g, gs, dead)
    out2, dl2 = _seg_call(cfg, N, Cc, HW, xd, td, ws, SCALES[-1])
    assert out.tobytes() == out2.tobytes() and dl.tobytes() == dl2.tobytes()
    assert ws.intact()


@pytest.mark.parametrize("case", G.cases("seg_sig") + G.cases("seg_mc"), ids=G.ident)
def test_seg_loss_five_term_sum(case):
    _check_seg(case, "sum5")


@pytest.mark.parametrize("case,name", G.single_term_cases("seg_sig") + G.single_term_cases("seg_mc"),
                         ids=lambda v: v if isinstance(v, str) else G.ident(v))
def test_seg_loss_single_terms(case, name):
    _check_seg(case, name)


def _bad_label_plan(case, family):
    """three out-of-range labels in the shares of three different workgroups of two images (with three workgroups the first one's is
    in its last sweep) -> [(n, pixel, label)]"""
    N, Cc, HW = case["N"], case["C"], case["HW"]
    nbx = G.route(family, N, Cc, HW)["nbx"]
    assert nbx >= 3 and N >= 2
    bxs = (1, 2, 0) if nbx == 3 else (1, nbx // 2, nbx - 1)
    assert len(set(bxs)) == 3
    picks = [(0, bxs[0], 5, Cc), (N - 1, bxs[1], -7, -1), (N - 1, bxs[2], -1, 10 ** 12)]
    return [(n, int(G.share(family, N, Cc, HW, bx)[k]), lab) for n, bx, k, lab in picks]


@pytest.mark.parametrize("case", [G.BY_ID["seg_mc-three-n2c5-hw6148"], G.BY_ID["seg_mc-three-n2c16-hw6147"],
                                  G.BY_ID["seg_mc-cap-n5c2-hw131076"]], ids=G.ident)
def test_seg_loss_bad_labels_past_the_first_share(case):
    N, Cc, HW, x, t, xd, td, ws = _seg_setup(case)
    t2 = t.copy()
    plan = _bad_label_plan(case, "seg_mc")
    for n, i, lab in plan:
        t2[n, i] = lab
    cfg = K.build(Ls, "sum5", "multiclass", Cc, True)._as_sum().cfg(Cc)
    out, dl = _seg_call(cfg, N, Cc, HW, xd, torch.from_numpy(t2).to(dev()), ws, 1024.0)
    assert out[6] == 3.0 and np.isnan(out[:6]).all() and out[7] == 0.0
    assert np.isfinite(dl).all() and not (dl == np.float32(SENT)).any()
    for n, i, _ in plan:
        assert (dl[n, :, i] == 0).all()
    dead = np.broadcast_to((t == G.IGN)[:, None, :], x.shape)
    assert (dl[dead] == 0).all() and (dl != 0).any() and ws.intact()


# ------------------------------------------------------------------------------------------------ vk_kp_loss
def _kcfg(c: dict, Cc: int):
    k = L_.vk_kp_loss_cfg()
    k.struct_size = C.sizeof(k)
    k.heat_planes, k.bce_planes = sum(1 << q for q in c["heat"]), sum(1 << q for q in c["bce"])
    k.w_heat, k.w_bce, k.alpha, k.beta, k.pos_threshold = c["w_heat"], c["w_bce"], c["alpha"], c["beta"], c["thr"]
    k.has_pos_weight = 0 if c["pos_weight"] is None else 1
    for i in range(16):
        k.pos_weight[i] = 1.0 if c["pos_weight"] is None or i >= Cc else c["pos_weight"][i]
    return k


def _kp_call(c, N, Cc, HW, xd, yd, ws, gs, prefill=None):
    L = vk.lib()
    out = torch.full((8,), 5.0, device=dev())
    pos = torch.full((16,), -7, dtype=torch.int64, device=dev())
    dl = torch.full_like(xd, SENT) if prefill is None else torch.from_numpy(prefill).to(dev())
    L_.check(L.vk_kp_loss(_kcfg(c, Cc), N, Cc, HW, xd.data_ptr(), yd.data_ptr(), ws.ptr(), ws.nbytes, out.data_ptr(), pos.data_ptr(),
                          dl.data_ptr(), gs, 0 if prefill is None else 1, _stream()), "vk_kp_loss")
    torch.cuda.synchronize()
    return out.cpu().numpy(), pos.cpu().numpy(), dl.cpu().numpy()


@pytest.mark.parametrize("case", G.cases("kp"), ids=G.ident)
def test_kp_loss(case):
    N, Cc, HW = case["N"], case["C"], case["HW"]
    need = vk.lib().vk_kp_loss_workspace_bytes(N, Cc, HW)
    assert need == G.kp_workspace_bytes(N, Cc, HW), (need, G.kp_workspace_bytes(N, Cc, HW))
    x, y = G.inputs(case)
    c = G.kp_ref_cfg(case)
    xd, yd, ws = torch.from_numpy(x).to(dev()), torch.from_numpy(y).to(dev()), _Workspace(need)
    ruled = sorted(c["heat"] + c["bce"])
    rest = [q for q in range(Cc) if q not in ruled]
    for gs in SCALES:
        ref, bnd = KC.bounds(x, y, c, grad_scale=gs)
        out, pos, dl = _kp_call(c, N, Cc, HW, xd, yd, ws, gs)
        for i, key in enumerate(("total", "heat", "bce")):
            err = abs(float(out[i]) - ref[key])
            print("GRID %s %s: error %.3g of its bound" % (case["id"], key, err / bnd[key] if bnd[key] > 0 else 0.0))
            assert err <= bnd[key], (case["id"], key, out[i], ref[key], err, bnd[key])
        assert (out[3:] == 0).all() and np.array_equal(pos, ref["positives"])
        assert np.isfinite(dl).all() and not (dl == np.float32(SENT)).any()
        err = np.abs(dl.astype(np.float64) - ref["grad"])
        print("GRID %s gs=%g gradient: max error / bound %.3f" % (case["id"], gs, float((err[:, ruled] / bnd["grad"][:, ruled]).max())))
        assert (err[:, ruled] <= bnd["grad"][:, ruled]).all() and (dl[:, rest] == 0).all()
    out2, pos2, dl2 = _kp_call(c, N, Cc, HW, xd, yd, ws, SCALES[-1])
    assert out.tobytes() == out2.tobytes() and dl.tobytes() == dl2.tobytes() and np.array_equal(pos, pos2)
    # accumulate = 1: old + g on the ruled planes (the sum formed in fp32 here), the other planes keep their bytes
    old = np.random.default_rng(HW).standard_normal(x.shape).astype(np.float32)
    out3, _, acc = _kp_call(c, N, Cc, HW, xd, yd, ws, SCALES[-1], prefill=old)
    assert out3.tobytes() == out.tobytes()
    assert acc[:, rest].tobytes() == old[:, rest].tobytes() and np.array_equal(acc[:, ruled], old[:, ruled] + dl[:, ruled])
    assert ws.intact()


# ------------------------------------------------------------------------------------------------ multiclass.hip
def _multi_call(multiclass, N, Cc, HW, xd, td, ws, gs, w_pix, w_dice):
    L = vk.lib()
    out = torch.full((4,), 5.0, device=dev())
    dl = torch.full_like(xd, SENT)
    fn = L.vk_multiclass_loss if multiclass else L.vk_multilabel_loss
    L_.check(fn(N, Cc, HW, xd.data_ptr(), td.data_ptr(), ws.ptr(), ws.nbytes, out.data_ptr(), dl.data_ptr(), gs, w_pix, w_dice, _stream()))
    torch.cuda.synchronize()
    return out.cpu().numpy(), dl.cpu().numpy()


def _multi_setup(case):
    N, Cc, HW = case["N"], case["C"], case["HW"]
    need = vk.lib().vk_multi_loss_workspace_bytes(N, Cc, HW)
    assert need == G.multi_workspace_bytes(N, Cc, HW), (need, G.multi_workspace_bytes(N, Cc, HW))
    x, t = G.inputs(case)
    return N, Cc, HW, x, t, torch.from_numpy(x).to(dev()), torch.from_numpy(t).to(dev()), _Workspace(need)


@pytest.mark.parametrize("case", G.cases("ml") + G.cases("mc"), ids=G.ident)
def test_multilabel_and_multiclass_loss(case):
    multiclass = case["family"] == "mc"
    N, Cc, HW, x, t, xd, td, ws = _multi_setup(case)
    ref_fn = MR.multiclass if multiclass else MR.multilabel
    for weights in G.WEIGHTS:
        tot, pix, dice, ref_g = ref_fn(torch.from_numpy(x), torch.from_numpy(t), *weights)
        tag = "%s w=%s" % (case["id"], weights)
        for gs in SCALES:
            out, dl = _multi_call(multiclass, N, Cc, HW, xd, td, ws, gs, *weights)
            _value_check(tag, out[:3], [tot.item(), pix.item(), dice.item()])
            assert out[3] == 0.0
            _grad_check(tag, dl, ref_g.numpy(), gs)
        out2, dl2 = _multi_call(multiclass, N, Cc, HW, xd, td, ws, SCALES[-1], *weights)
        assert out.tobytes() == out2.tobytes() and dl.tobytes() == dl2.tobytes()
    assert ws.intact()


@pytest.mark.parametrize("case", [G.BY_ID["mc-three-n2c3-hw12292"], G.BY_ID["mc-three-n2c5-hw12808"], G.BY_ID["mc-cap-n5c2-hw212995"]],
                         ids=G.ident)
def test_multiclass_loss_bad_labels_past_the_first_share(case):
    N, Cc, HW, x, t, xd, td, ws = _multi_setup(case)
    t2 = t.copy()
    plan = _bad_label_plan(case, "mc")
    for n, i, lab in plan:
        t2[n, i] = lab
    out, dl = _multi_call(True, N, Cc, HW, xd, torch.from_numpy(t2).to(dev()), ws, 1024.0, 1.0, 1.0)
    assert out[3] == 3.0 and np.isnan(out[:3]).all()
    assert np.isfinite(dl).all() and not (dl == np.float32(SENT)).any() and (dl != 0).any()
    for n, i, _ in plan:
        assert (dl[n, :, i] == 0).all()
    assert ws.intact()


# ------------------------------------------------------------------------------------------------ the Lovasz launch caps
def _lovasz_call(cfg, x, t, gs):
    L = vk.lib()
    N, Cc, H, W = x.shape
    xd, td = x.to(dev()).contiguous(), t.to(dev()).contiguous()
    ws = torch.empty(L.vk_lovasz_workspace_bytes(cfg, N, Cc, H * W), dtype=torch.uint8, device=dev())
    assert ws.numel() > 0
    out = torch.full((4,), 5.0, device=dev())
    dl = torch.full_like(xd, SENT)
    L_.check(L.vk_lovasz_loss(cfg, N, Cc, H * W, xd.data_ptr(), td.data_ptr(), ws.data_ptr(), ws.numel(), out.data_ptr(), dl.data_ptr(),
                              gs, 0, _stream()), "vk_lovasz_loss")
    torch.cuda.synchronize()
    return out.cpu().numpy(), dl.cpu().numpy()


@pytest.mark.parametrize("name", [c[0] for c in G.LOVASZ])
def test_lovasz_softmax_past_the_launch_caps(name):
    """N HW just above 1,024 x 256 (k_lv_bad) and 8,192 x 256 (k_lv_softmax_bwd): the pixels of the second grid-stride trip get their
    gradient, and bad labels there are counted"""
    _, N, Cc, HW, second = next(c for c in G.LOVASZ if c[0] == name)
    x, t = G.lovasz_inputs(name)
    cfg = Lv.LovaszLoss("multiclass", per_image=False, ignore_index=G.IGN).cfg(Cc)
    v, g, present = LR.softmax(x.numpy(), t.numpy(), False, G.IGN)
    assert present == [[0, 1]]
    bar = max(8 * G.LOVASZ_D0[name], 1e-6)
    dead = np.broadcast_to((t == G.IGN).unsqueeze(1).numpy(), x.shape)
    tail = np.arange(second, N * HW) - (N - 1) * HW            # the second trip's pixels, all in the last image
    assert (tail >= 0).all() and np.abs(g[N - 1, :, 0, tail]).max() > 0
    for gs in SCALES:
        out, dl = _lovasz_call(cfg, x, t, gs)
        rel = np.linalg.norm(dl - gs * g) / np.linalg.norm(gs * g)
        print("GRID lovasz %s gs=%g: relative gradient error %.3e, bar %.3e, value %.9g ref %.9g" % (name, gs, rel, bar, out[0], v))
        assert abs(float(out[0]) - v) <= 1e-5 * abs(v) + 1e-6 and out[1] == 0
        assert np.isfinite(dl).all() and not (dl == np.float32(SENT)).any()
        assert rel <= bar
        assert dead.any() and (dl[dead] == 0).all()
        gt = gs * g[N - 1, :, 0, tail]                         # the second trip by itself, per element (a skipped trip leaves the sentinel)
        assert np.abs(dl[N - 1, :, 0, tail] - gt).max() <= 1e-4 * gs * np.abs(g).max()
    out2, dl2 = _lovasz_call(cfg, x, t, SCALES[-1])
    assert out.tobytes() == out2.tobytes() and dl.tobytes() == dl2.tobytes()
    t2 = t.clone()
    bad = [int(tail[0]), int(tail[len(tail) // 2]), int(tail[-1])]
    for i, lab in zip(bad, (Cc, -3, 10 ** 12)):
        t2[N - 1, 0, i] = lab
    out, dl = _lovasz_call(cfg, x, t2, 1.0)
    assert np.isnan(out[0]) and out[1] == 3
    assert np.isfinite(dl).all() and not (dl == np.float32(SENT)).any() and (dl[N - 1, :, 0, bad] == 0).all()


# ------------------------------------------------------------------------------------------------ the fused step at 128 x 128
def _O():
    from oracle import unet_oracle as O
    return O


@pytest.mark.parametrize("which", ["default", "seglosses"])
def test_fused_step_at_128(which):
    """classes = 3 at 2 x 128 x 128, fp32: nbx = 4 in multiclass.hip (the default CE + Dice step) and 8 in seg_loss.hip"""
    O = _O()
    classes, N, S_ = 3, 2, 128
    assert G.multi_nbx(S_ * S_) == 4 and G.seg_nbx(True, N, classes, S_ * S_) == 8
    O.set_seed(42)
    m = vk.multiclass.Unet(encoder_weights=None, classes=classes).to(dev()).train()
    x, _ = O.synthetic_batch(N, S_, seed=1234)
    _, tgt = K.make_inputs("multiclass", classes, N, S_, S_, True, seed=97)
    if which == "default":
        tgt = tgt.clamp_max(classes - 1)                    # the default step has no ignore_index
        module = vk.multiclass.CEDiceLoss()
        kw = dict(mode="multiclass")
    else:
        module = K.build(Ls, "sum5", "multiclass", classes, True)
        kw = dict(loss=module)
    x, tgt_d = x.to(dev()), tgt.to(dev())
    sd = copy.deepcopy(m.state_dict())

    def autograd(loss_fn=None):
        m.load_state_dict(sd)
        m.zero_grad(set_to_none=True)
        with torch.autocast("cuda", enabled=False):
            lg = m(x)
        loss = (loss_fn or module)(lg.float(), tgt_d)
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), m.flat_grads.detach().clone()

    def fused():
        m.load_state_dict(sd)
        m.zero_grad(set_to_none=True)
        out = m.loss_and_backward(x, tgt_d, dtype=torch.float32, **kw)
        torch.cuda.synchronize()
        return out.clone(), m.flat_grads.detach().clone(), m.last_logits.detach().cpu().clone()

    l_a, g_a = autograd()
    l_f, g_f, lg = fused()
    assert tuple(lg.shape) == (N, classes, S_, S_) and torch.isfinite(l_f).all()
    if which == "default":
        tot, ce, dice, _ = MR.multiclass(lg, tgt)
        assert l_f.shape == (3,)
        _value_check("fused default", l_f.cpu().numpy(), [tot.item(), ce.item(), dice.item()])
        assert torch.equal(l_f[0], l_a) and torch.equal(g_f, g_a)            # same kernels, same bits
        # and torch's own cross-entropy beside the Dice module, as tests/test_multiclass_gpu.py holds it at 64 x 64: the head's
        # gradient within 1e-5 by norm, the whole model's within 1e-3 (fp32)
        l_t, g_t = autograd(lambda lg_, tg: F.cross_entropy(lg_, tg) + vk.multiclass.DiceLoss(mode="multiclass")(lg_, tg))
        assert abs(l_t.item() - l_f[0].item()) <= 1e-5 * abs(l_f[0].item())
        h0, h1 = m._param_ranges[-2][0], m._param_ranges[-1][0] + m._param_ranges[-1][1]
        assert ((g_t[h0:h1] - g_f[h0:h1]).norm() / g_f[h0:h1].norm()).item() <= 1e-5
        assert ((g_t - g_f).norm() / g_f.norm()).item() <= 1e-3
    else:
        rf = SR.evaluate(lg, tgt, module.spec(classes))
        assert l_f.shape == (6,)
        _value_check("fused seglosses", l_f.cpu().numpy(), SR.components(rf).numpy())
        assert abs(l_f[0].item() - l_a.item()) <= 1e-5 * abs(l_a.item())
        assert ((g_f - g_a).norm() / g_a.norm()).item() <= 1e-5
    l_2, g_2, _ = fused()
    assert torch.equal(l_2, l_f) and torch.equal(g_2, g_f)
