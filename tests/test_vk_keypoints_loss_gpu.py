"""vk_kp_loss on the MI355X (-m gpu) against the float64 restatement of tests/keypoints_loss_ref.py, within the bounds derived in
tests/keypoints_loss_cases.py; its structure (accumulate, planes without a rule, guards, reproducibility, plane position, grad_scale,
the BCE plane against vk_seg_loss); the autograd module and the fused step (vk_unet_loss_kp); the read-out behind ObjectMetrics and
Segmenter.

Every call of the first two parts goes through the C ABI into sentinel-filled buffers between two guard zones, on a workspace that is
never cleared."""
import copy
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import keypoints_loss_cases as KC
import keypoints_loss_ref as R
import seglosses_ref as SR
import subpix_cases as SC

pytestmark = pytest.mark.gpu
vk = importlib.import_module("vickers-hardness-unet_amd")
KP, Ls, L_ = vk.keypoints, vk.seglosses, vk._lib

GUARD = 64                    # floats: 256 bytes, so a guarded zone keeps the 16-byte alignment of its buffer
SENT = 12345.0
I_SENT = -7


def dev():
    return torch.device("cuda:0")


def _guarded(n, shift=0, dtype=torch.float32, fill=SENT):
    buf = torch.full((n + 2 * GUARD + shift,), fill, dtype=dtype, device=dev())
    return buf, buf[GUARD + shift:GUARD + shift + n]


def _intact(buf, n, shift=0, fill=SENT):
    lo = GUARD + shift
    return bool((buf[:lo] == fill).all()) and bool((buf[lo + n:] == fill).all())


def _kcfg(c: dict, C_: int):
    k = L_.vk_kp_loss_cfg()
    k.struct_size = C.sizeof(k)
    k.heat_planes, k.bce_planes = sum(1 << q for q in c["heat"]), sum(1 << q for q in c["bce"])
    k.w_heat, k.w_bce, k.alpha, k.beta, k.pos_threshold = c["w_heat"], c["w_bce"], c["alpha"], c["beta"], c["thr"]
    k.has_pos_weight = 0 if c["pos_weight"] is None else 1
    for i in range(16):
        k.pos_weight[i] = 1.0 if c["pos_weight"] is None or i >= C_ else c["pos_weight"][i]
    return k


def _call(c: dict, x: np.ndarray, y: np.ndarray, shift=0, grad=True, prefill=None, grad_scale=1.0, positives=True):
    """vk_kp_loss on x, y float32 [N][C][HW] -> (loss_out float32 [8], positives int64 [16] or None, dlogits float32 [N][C][HW] or None).
    shift: every base moved by that many floats (1: the scalar path).  prefill: accumulate = 1 onto these values."""
    L = vk.lib()
    N, Cc, HW = x.shape
    n = x.size
    xb, xd = _guarded(n, shift)
    yb, yd = _guarded(n, shift)
    db, dd = _guarded(n, shift)
    xd.copy_(torch.from_numpy(x.reshape(-1)))
    yd.copy_(torch.from_numpy(y.reshape(-1)))
    if prefill is not None:
        dd.copy_(torch.from_numpy(prefill.reshape(-1)))
    ob, od = _guarded(8)
    pb, pd = _guarded(16, dtype=torch.int64, fill=I_SENT)
    need = L.vk_kp_loss_workspace_bytes(N, Cc, HW)
    assert need > 0
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=dev())          # never cleared: every double a NaN, every count -1
    assert (xd.data_ptr() % 16 == 0) == (shift == 0)
    L_.check(L.vk_kp_loss(_kcfg(c, Cc), N, Cc, HW, xd.data_ptr(), yd.data_ptr(), ws.data_ptr(), need, od.data_ptr(),
                          pd.data_ptr() if positives else None, dd.data_ptr() if grad else None, grad_scale, 0 if prefill is None else 1,
                          torch.cuda.current_stream().cuda_stream), "vk_kp_loss")
    torch.cuda.synchronize()
    assert _intact(xb, n, shift) and _intact(yb, n, shift) and _intact(db, n, shift) and _intact(ob, 8) and _intact(pb, 16, fill=I_SENT)
    assert np.array_equal(xd.cpu().numpy(), x.reshape(-1)) and np.array_equal(yd.cpu().numpy(), y.reshape(-1), equal_nan=True)
    dl = dd.cpu().numpy().reshape(x.shape)
    if not grad:
        assert (dl == np.float32(SENT)).all()
    if not positives:
        assert bool((pd == I_SENT).all())
    return od.cpu().numpy(), pd.cpu().numpy() if positives else None, dl if grad else None


def _targets(kind: str, N: int, Cc: int, HW: int, seed: int):
    """-> (float32 [N][C][HW], the threshold that goes with the kind)"""
    rng = np.random.default_rng(3000 + seed)
    if kind in ("kp", "kp_subpixel"):
        y = np.empty((N, Cc, HW), np.float32)
        counts = torch.full((N,), 2, dtype=torch.int32, device=dev())
        for q in range(Cc):
            v = torch.from_numpy(KC.vertices(N, HW, kind == "kp_subpixel", seed + 17 * q)).to(dev())
            y[:, q] = KP.targets(v, (1, HW), sigma=KC.SIGMA, counts=counts).reshape(N, HW).cpu().numpy()
        thr = 1.0 if kind == "kp" else KP.positive_threshold(KC.SIGMA)
        if HW >= 64:
            assert (y >= np.float32(thr)).any() and (y == 0).any() and ((y > 0) & (y < np.float32(thr))).any()
        return y, thr
    if kind == "random":
        return rng.random((N, Cc, HW)).astype(np.float32), 0.9
    return np.full((N, Cc, HW), 0.0 if kind == "zeros" else 1.0, np.float32), 1.0


def _check(got, ref, bnd, c, name):
    out, pos, dl = got
    for i, key in enumerate(("total", "heat", "bce")):
        err = abs(float(out[i]) - ref[key])
        print("%s %s %.9g ref %.9g err %.3e bound %.3e" % (name, key, out[i], ref[key], err, bnd[key]))
        assert err <= bnd[key], (name, key, out[i], ref[key], err, bnd[key])
    assert (out[3:] == 0).all()
    assert np.array_equal(pos, ref["positives"]), (name, pos, ref["positives"])
    err = np.abs(dl.astype(np.float64) - ref["grad"])
    print("%s gradient: max err / bound %.3f" % (name, float((err / np.maximum(bnd["grad"], 1e-300)).max())))
    ruled = sorted(c["heat"] + c["bce"])
    assert (err[:, ruled] <= bnd["grad"][:, ruled]).all(), (name, float(err.max()))
    rest = [q for q in range(dl.shape[1]) if q not in ruled]
    assert (dl[:, rest] == 0).all()                         # planes with neither rule: all zero with accumulate = 0


# ------------------------------------------------------------------------------------------------ value, positives, gradient
@pytest.mark.parametrize("HW", KC.HWS)
@pytest.mark.parametrize("config", KC.CONFIGS, ids=[c[0] for c in KC.CONFIGS])
def test_value_positives_and_gradient(config, HW):
    name, N, Cc = config[0], config[1], config[2]
    x = KC.logits(N, Cc, HW, seed=HW)
    first = None
    for kind in KC.KINDS:
        y, thr = _targets(kind, N, Cc, HW, seed=HW)
        c = KC.ref_cfg(config, thr)
        ref, bnd = KC.bounds(x, y, c)
        if kind == "zeros":
            assert all(ref["positives"][q] == 0 for q in c["heat"])                    # a plane that is all negative: divided by 1
        if kind == "ones":
            assert all(ref["positives"][q] == N * HW for q in c["heat"])               # every entry positive
        for shift in ((0, 1) if HW % 4 == 0 else (0,)):
            got = _call(c, x, y, shift=shift)
            _check(got, ref, bnd, c, "%s HW=%d %s shift=%d" % (name, HW, kind, shift))
            if first is None:
                first = (c, y, got)
    # a second run on an uncleared workspace gives the same bytes; without dlogits and positives the values are the same
    c, y, got = first
    again = _call(c, x, y)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))
    out, _, _ = _call(c, x, y, grad=False, positives=False)
    assert out.tobytes() == got[0].tobytes()


def test_grad_scale_and_nan_target():
    config = KC.CONFIGS[2]
    x = KC.logits(1, 2, 1028, seed=5)
    y, thr = _targets("kp_subpixel", 1, 2, 1028, seed=5)
    c = KC.ref_cfg(config, thr)
    ref, bnd = KC.bounds(x, y, c, grad_scale=256.0)
    got = _call(c, x, y, grad_scale=256.0)
    _check(got, ref, bnd, c, "grad_scale 256")
    for gs in (1.0, 256.0):                                                            # doubling grad_scale doubles every entry exactly
        one, two = _call(c, x, y, grad_scale=gs)[2], _call(c, x, y, grad_scale=2.0 * gs)[2]
        assert np.array_equal(two, 2.0 * one) and np.abs(one).max() > 0
    y2 = y.copy()
    y2[0, 1, 7] = np.nan                                                               # a NaN target propagates: nothing is checked on the device
    out, _, dl = _call(c, x, y2)
    assert np.isnan(out[0]) and np.isnan(out[1]) and not np.isnan(out[2]) and np.isnan(dl[0, 1, 7]) and not np.isnan(dl[0, 0]).any()


# ------------------------------------------------------------------------------------------------ structure
@pytest.mark.parametrize("HW", [7, 1028, KC.HW_TWO_WORKGROUPS])
@pytest.mark.parametrize("config", [KC.CONFIGS[4], KC.CONFIGS[5], KC.CONFIGS[6]], ids=[KC.CONFIGS[i][0] for i in (4, 5, 6)])
def test_accumulate(config, HW):
    _, N, Cc = config[0], config[1], config[2]
    x = KC.logits(N, Cc, HW, seed=HW + 1)
    y, thr = _targets("random", N, Cc, HW, seed=HW + 1)
    c = KC.ref_cfg(config, thr)
    ruled = sorted(c["heat"] + c["bce"])
    rest = [q for q in range(Cc) if q not in ruled]
    assert rest
    old = np.random.default_rng(HW).standard_normal(x.shape).astype(np.float32)
    for shift in ((0, 1) if HW % 4 == 0 else (0,)):
        out0, pos0, g = _call(c, x, y, shift=shift, grad_scale=2.0)
        out1, pos1, acc = _call(c, x, y, shift=shift, grad_scale=2.0, prefill=old)
        assert out0.tobytes() == out1.tobytes() and np.array_equal(pos0, pos1)
        assert acc[:, rest].tobytes() == old[:, rest].tobytes()                        # planes with neither rule keep their bytes
        assert np.array_equal(acc[:, ruled], old[:, ruled] + g[:, ruled])             # old + g, the sum formed in fp32 here
        assert (g[:, rest] == 0).all() and np.abs(g[:, ruled]).max() > 0


@pytest.mark.parametrize("rule", ["heat", "bce"])
@pytest.mark.parametrize("HW", [7, 1028, KC.HW_TWO_WORKGROUPS + 4])
def test_plane_position(rule, HW):
    """The same data as plane 0 of C = 1 and as plane 3 of C = 5 (beside another plane of the same rule, with the weight doubled so the
    coefficient is the same): the same gradient bytes on that plane, the same value within one fp32 rounding."""
    N = 3
    x1 = KC.logits(N, 1, HW, seed=HW + 2)
    y1, thr = _targets("kp_subpixel", N, 1, HW, seed=HW + 2)
    one = R.cfg(heat=[0] if rule == "heat" else [], bce=[0] if rule == "bce" else [], alpha=2, beta=4, thr=thr, w_heat=0.75, w_bce=0.75,
                pos_weight=[2.0])
    x5 = KC.logits(N, 5, HW, seed=HW + 3)
    y5 = _targets("random", N, 5, HW, seed=HW + 3)[0]
    x5[:, 3], y5[:, 3] = x1[:, 0], y1[:, 0]
    x5[:, 1], y5[:, 1] = x1[:, 0], y1[:, 0]                                            # plane 1: the same data again, so the term's value is the same
    five = R.cfg(heat=[1, 3] if rule == "heat" else [], bce=[1, 3] if rule == "bce" else [], alpha=2, beta=4, thr=thr, w_heat=1.5, w_bce=1.5,
                 pos_weight=[1.0, 2.0, 1.0, 2.0, 1.0])
    o1, p1, g1 = _call(one, x1, y1)
    o5, p5, g5 = _call(five, x5, y5)
    assert g5[:, 3].tobytes() == g1[:, 0].tobytes() and g5[:, 1].tobytes() == g1[:, 0].tobytes() and np.abs(g1).max() > 0
    i = 1 if rule == "heat" else 2
    assert abs(float(o5[i]) - float(o1[i])) <= 2.0 ** -23 * abs(float(o1[i])) and o1[i] > 0
    assert p5[3] == p1[0] and p5[1] == p1[0]


@pytest.mark.parametrize("pw", [None, [3.0, 0.5, 1.0]], ids=["plain", "pos_weight"])
@pytest.mark.parametrize("HW", [7, 1024, 1028, KC.HW_TWO_WORKGROUPS])
def test_bce_planes_equal_the_pixel_term_of_vk_seg_loss(HW, pw):
    """A BCE-only configuration over all planes against vk_seg_loss with only the pix term (mean over all entries, no smoothing, the
    same pos_weight): the same gradient (torch.equal), the value within 2^-23 relative (the partition of the sum may differ)."""
    L = vk.lib()
    N, Cc = 3, 3
    x = KC.logits(N, Cc, HW, seed=HW + 4)
    y = _targets("random", N, Cc, HW, seed=HW + 4)[0]
    c = R.cfg(bce=[0, 1, 2], w_bce=0.75, pos_weight=pw)
    out, _, dl = _call(c, x, y, grad_scale=4.0)
    sc = Ls.SoftBCEWithLogitsLoss(ignore_index=None, pos_weight=pw).cfg(Cc)
    sc.w_pix = 0.75
    assert sc.terms == 1 and sc.pix_denom_valid == 0 and sc.pix_smooth == 0 and sc.has_ignore == 0
    xd, yd = torch.from_numpy(x).to(dev()), torch.from_numpy(y).to(dev())
    ws = torch.empty(L.vk_seg_loss_workspace_bytes(N, Cc, HW), dtype=torch.uint8, device=dev())
    so = torch.full((8,), 5.0, device=dev())
    sdl = torch.full_like(xd, 7.0)
    L_.check(L.vk_seg_loss(sc, N, Cc, HW, xd.data_ptr(), yd.data_ptr(), ws.data_ptr(), ws.numel(), so.data_ptr(), sdl.data_ptr(), 4.0,
                           torch.cuda.current_stream().cuda_stream), "vk_seg_loss")
    torch.cuda.synchronize()
    assert torch.equal(torch.from_numpy(dl), sdl.cpu()) and np.abs(dl).max() > 0
    assert abs(float(out[0]) - so[0].item()) <= 2.0 ** -23 * abs(so[0].item())
    assert abs(float(out[2]) - so[1].item()) <= 2.0 ** -23 * abs(so[1].item())


# ------------------------------------------------------------------------------------------------ module and fused step
def _O():
    from oracle import unet_oracle as O
    return O


def _mask64(N=2):
    m = np.zeros((N, 64, 64), np.float32)
    for b, (cx, cy, rad, ang) in enumerate(((30.0, 31.0, 20.0, 0.2), (34.0, 30.0, 16.0, 0.7))[:N]):
        m[b] = SC.polygon_coverage(64, 64, SC.square_vertices(cx, cy, rad, ang)) >= 0.5
    return m


def _recipe():
    return (KP.PlaneBCE([0]) + Ls.DiceLoss("multilabel", classes=[0])
            + 0.5 * KP.HeatmapFocalLoss([1], pos_threshold=KP.positive_threshold(2.0)))


def _restated(S, x, y):
    """value and gradient of a vk.keypoints.LossSum from the two restatements"""
    Cc = x.shape[1]
    k = S.kp_cfg(Cc)
    c = R.cfg([q for q in range(Cc) if k.heat_planes >> q & 1], [q for q in range(Cc) if k.bce_planes >> q & 1], k.w_heat, k.w_bce, k.alpha,
              k.beta, k.pos_threshold, list(k.pos_weight)[:Cc] if k.has_pos_weight else None)
    N = x.shape[0]
    r = R.evaluate(x.numpy().reshape(N, Cc, -1), y.numpy().reshape(N, Cc, -1), c)
    total, grad = r["total"], r["grad"].reshape(x.shape)
    comps = np.zeros(9)
    if S.seg is not None:
        rf = SR.evaluate(x, y, S.seg.spec(Cc))
        total = total + float(rf["total"])
        grad = grad + rf["dlogits"].numpy().reshape(x.shape)
    comps[0], comps[7], comps[8] = total, r["heat"], r["bce"]
    return total, grad, comps


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_autograd_module(dtype):
    y2 = KP.make_targets(torch.from_numpy(_mask64()).to(dev()), sigma=2.0)
    g = torch.Generator().manual_seed(7)
    x = (torch.randn(2, 2, 64, 64, generator=g) * 3.0)
    for S in (_recipe(), 0.75 * KP.HeatmapFocalLoss([1], alpha=1, beta=2, pos_threshold=KP.positive_threshold(2.0)), KP.PlaneBCE([0, 1], pos_weight=[2.0, 5.0])):
        lg = x.to(dev()).to(dtype).requires_grad_()
        loss = S(lg, y2)
        (3.0 * loss).backward()
        torch.cuda.synchronize()
        total, grad, comps = _restated(S._as_kp_sum(), lg.detach().float().cpu(), y2.cpu())
        assert abs(loss.item() - total) <= 1e-5 * abs(total) + 1e-6 and lg.grad.dtype == dtype
        tol = 1e-4 if dtype == torch.float32 else 2.0 ** -7
        assert np.abs(lg.grad.float().cpu().numpy() - 3.0 * grad).max() <= tol * 3.0 * np.abs(grad).max()
        lc = S._as_kp_sum().last_components if isinstance(S, KP.LossSum) else S._sum.last_components
        assert lc.shape == (9,) and abs(lc[0].item() - total) <= 1e-5 * abs(total) + 1e-6
        assert abs(lc[7].item() - comps[7]) <= 1e-5 * abs(comps[7]) + 1e-6 and abs(lc[8].item() - comps[8]) <= 1e-5 * abs(comps[8]) + 1e-6
    want = _restated(_recipe(), x, y2.cpu())[0]
    with torch.no_grad():                                                              # no gradient asked for: the backward pass is skipped
        assert abs(_recipe()(x.to(dev()), y2).item() - want) <= 1e-5 * abs(want) + 1e-6


def _model(classes=2):
    _O().set_seed(42)
    return vk.multiclass.Unet(encoder_weights=None, classes=classes).to(dev()).train()


def _step_inputs():
    x, _ = _O().synthetic_batch(2, 64, seed=1234)
    return x.to(dev()), KP.make_targets(torch.from_numpy(_mask64()).to(dev()), sigma=2.0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("with_seg", [True, False], ids=["recipe", "kp_only"])
def test_loss_and_backward_equals_autograd(with_seg, dtype):
    """The assertions and tolerances of tests/test_lovasz_gpu.py::test_loss_and_backward_equals_autograd."""
    x, tgt = _step_inputs()
    S = _recipe() if with_seg else KP.PlaneBCE([0], pos_weight=2.0) + 0.5 * KP.HeatmapFocalLoss([1], pos_threshold=KP.positive_threshold(2.0))
    m = _model()
    sd = copy.deepcopy(m.state_dict())
    ptrs = set()

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
    comps_a = S.last_components.clone()
    l_f, g_f = fused()
    assert l_f.shape == (9,) and torch.isfinite(l_f).all()
    assert abs(l_f[0].item() - l_a.item()) <= 1e-5 * abs(l_a.item())
    assert ((g_f - g_a).norm() / g_a.norm()).item() <= 1e-5
    assert torch.equal(S.last_components, l_f) and l_f[7].item() > 0 and l_f[8].item() > 0
    assert ((l_f - comps_a).abs() <= 1e-5 * comps_a.abs()).all()
    assert (l_f[3].item() > 0) == with_seg and (l_f[[1, 2, 4, 5, 6]] == 0).all()
    assert tuple(m.last_logits.shape) == (x.shape[0], 2) + tuple(x.shape[2:])
    _, g_s = fused(scale=256.0)
    assert ((g_s - 256.0 * g_f).norm() / (256.0 * g_f).norm()).item() <= 1e-5
    l_2, g_2 = fused()
    assert torch.equal(l_2, l_f) and torch.equal(g_2, g_f)                             # two fused steps are bit-identical
    assert len(ptrs) == 1                                                              # one result buffer per plan
    # the other loss= routes return what they returned
    m.load_state_dict(sd)
    m.zero_grad(set_to_none=True)
    seg = Ls.BCEWithLogitsLoss() + Ls.DiceLoss("multilabel")
    hard = (tgt >= 0.5).float()
    assert m.loss_and_backward(x, hard, dtype=dtype, loss=seg).shape == (6,)
    m.zero_grad(set_to_none=True)
    assert m.loss_and_backward(x, hard, dtype=dtype, loss=seg + 0.5 * vk.lovasz.LovaszLoss("multilabel")).shape == (8,)


def test_frozen_encoder_step():
    x, tgt = _step_inputs()
    S = _recipe()
    m = _model()
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
    assert out.shape == (9,) and abs(out[0].item() - loss.item()) <= 1e-5 * abs(loss.item())
    assert g_a.norm().item() > 0 and ((g_f - g_a).norm() / g_a.norm()).item() <= 1e-5
    assert all(p.grad is None or not p.grad.any() for p in m.encoder.parameters())


# ------------------------------------------------------------------------------------------------ read-out
def _squares_mask():
    m = np.zeros((2, 96, 160), np.float32)
    for b, (cx, cy, rad, ang) in enumerate(((50.0, 48.0, 30.0, 0.2), (100.0, 50.0, 34.0, 0.7))):
        m[b] = SC.polygon_coverage(96, 160, SC.square_vertices(cx, cy, rad, ang)) >= 0.5
    m[0] = np.maximum(m[0], SC.polygon_coverage(96, 160, SC.square_vertices(125.0, 40.0, 18.0, 0.4)) >= 0.5)
    return m


def test_object_metrics_with_the_heatmap_read_out():
    I = vk.instances
    mask = torch.from_numpy(_squares_mask()).to(dev())
    gt = I.detect_gt(mask, fit="quad", fit_outset_px=0)
    heat = KP.targets(gt, sigma=2.0)                                                   # the heat given as the exact target
    om = I.ObjectMetrics(fit="quad", fit_outset_px=0, refine=dict(kind="keypoints", sigma=2.0, min_peak=0.5), **I.GT_PRESET)
    res = om.update(mask, mask, heat=heat).cpu()
    t = om.totals()
    assert int(t["tp"][0]) == 3 and int(t["fp"][0]) == 0 and int(t["fn"][0]) == 0 and float(t["sum_abs_d"][0]) == 0.0
    assert float(t["max_abs_d"][0]) == 0.0 and om.n_images == 2
    m = om.compute()
    assert m["precision"][0] == 1.0 and m["recall"][0] == 1.0 and m["mean_abs_d"][0] == 0.0
    # by hand: detect, refine, match
    pred = I.detect(mask, fit="quad", fit_outset_px=0, max_components=64, **I.GT_PRESET)
    fine_p = KP.refine(pred, heat, min_peak=0.5)
    fine_g = KP.refine(gt, KP.targets(gt, (96, 160), 2.0), min_peak=0.5)
    assert isinstance(fine_g, vk.subpix.RefinedDetections)
    hand = I.match(fine_p, fine_g, om.thresholds).cpu()
    assert hand.totals.tobytes() == t.tobytes() and hand.per_image.tobytes() == res.per_image.tobytes()
    assert np.array_equal(hand.pair_gt, res.pair_gt) and np.array_equal(hand.pair_derr, res.pair_derr, equal_nan=True)
    recs = fine_g.raw.cpu().numpy().reshape(-1).view(vk.subpix.RECORD_DTYPE).reshape(2, 64)
    boxes = gt.raw.cpu().numpy().reshape(-1).view(gt.record_dtype).reshape(2, 64)
    for b, s in ((0, 0), (0, 1), (1, 0)):
        assert (recs[b, s]["v"] == boxes[b, s]["box"]).all() and not recs[b, s]["flags"].any()      # the integer corners come back
    # the existing forms are what they were
    plain = I.ObjectMetrics(fit="quad", fit_outset_px=0, **I.GT_PRESET)
    plain.update(mask, mask)
    assert int(plain.totals()["tp"][0]) == 3
    assert I.object_metrics(mask, mask, fit="quad", fit_outset_px=0, refine=dict(kind="keypoints", sigma=2.0, min_peak=0.5), heat=heat,
                            **I.GT_PRESET)["mean_abs_d"][0] == 0.0


class _Fixed(torch.nn.Module):
    """A model whose output is a fixed tensor."""

    def __init__(self, planes: torch.Tensor):
        super().__init__()
        self.register_buffer("planes", planes)

    def forward(self, x):
        assert tuple(x.shape[2:]) == tuple(self.planes.shape[2:])
        return self.planes


def _same_rows(a, b):
    assert len(a) == len(b) and len(a) > 0
    for ra, rb in zip(a, b):
        assert sorted(ra) == sorted(rb)
        for k in ra:
            if isinstance(ra[k], np.ndarray):
                assert np.array_equal(ra[k], rb[k]), k
            else:
                assert ra[k] == rb[k], k


def test_segmenter_measure_and_render_with_the_heatmap_read_out():
    S = 128
    m = np.zeros((1, S, S), np.float32)
    m[0] = SC.polygon_coverage(S, S, SC.square_vertices(60.0, 66.0, 30.0, 0.3)) >= 0.5
    mask = torch.from_numpy(m).to(dev())
    heat = KP.targets(vk.instances.detect_gt(mask, fit="quad", fit_outset_px=0), sigma=2.0)
    planes = torch.stack([16.0 * mask - 8.0, 12.0 * heat - 6.0], dim=1)              # logits [1, 2, S, S]
    seg = vk.Segmenter(_Fixed(planes), img_size=S, device=dev())
    img = np.zeros((90, 150, 3), np.uint8)
    aff = vk.subpix.letterbox_affine(90, 150, S, "centered")
    _, lists = KP.postprocess(torch.sigmoid(planes), fit="quad", affine=aff)
    rows = seg.measure(img, fit="quad", method="heatmap", zoom=False)
    _same_rows(rows, lists[0])
    assert rows[0]["d_mean"] > 0 and "zoom_status" not in rows[0]
    _, lists7 = KP.postprocess(torch.sigmoid(planes), fit="quad", method="centroid", affine=aff, refine_args=dict(cwin=2))
    _same_rows(seg.measure(img, fit="quad", method="heatmap", zoom=False, refine_args=dict(method="centroid", cwin=2)), lists7[0])
    out = seg.render(img, fit="quad", method="heatmap", zoom=False)
    _same_rows(out[0], lists[0])
    assert all(v.shape == (90, 150, 3) and v.dtype == np.uint8 for v in out[1:])
    with pytest.raises(ValueError, match="zoom=False"):
        seg.measure(img, method="heatmap")
    one = vk.Segmenter(_Fixed(planes[:, :1].contiguous()), img_size=S, device=dev())
    with pytest.raises(ValueError, match="heatmap plane"):
        one.measure(img, method="heatmap", zoom=False)
    _same_rows(one.measure(img, fit="quad", zoom=False), seg.measure(img, fit="quad", zoom=False))       # the default method: plane 0 alone
