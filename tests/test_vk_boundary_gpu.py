"""vk.boundary on the MI355X: vk_edt_sq, vk_boundary_phi, vk_boundary_stats and vk_boundary_loss against the numpy restatement of
boundary_ref.py, then the Python layer.  Distances are integers: those comparisons are EXACT.  Outputs of the C ABI go into
sentinel-filled buffers with a guard zone on both sides; every output element must be overwritten and no guard element touched.

The bounds of the loss on random logits follow from K_FUNC of tests/tail_cases.py (the measured error of the sigmoid expression, in
units of 2^-24 relative) and are written out at _loss_bounds."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import boundary_cases as BC
import boundary_ref as R
from conftest import GOLDEN
from tail_cases import K_FUNC, P_FLOOR, TINY, U32

pytestmark = pytest.mark.gpu
vk = importlib.import_module("vickers-hardness-unet_amd")
L = vk._lib
B = vk.boundary
DEV = torch.device("cuda:0")
GUARD = 256
I_SENTINEL = -7               # no d^2
F_SENTINEL = 12345.0          # no phi: sqrt(d^2) = 12345 needs d^2 beyond the largest map; no gradient of these tests either
SITE_CODE = {"fg": L.VK_EDT_FG, "bg": L.VK_EDT_BG, "edge": L.VK_EDT_EDGE}
FORMS = (("auto", 0), ("search", L.VK_EDT_ROWS_SEARCH), ("envelope", L.VK_EDT_ROWS_ENVELOPE))


def _guarded(numel, dtype, fill):
    buf = torch.full((numel + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + numel]


def _guards_intact(buf, numel, fill):
    return bool((buf[:GUARD] == fill).all() and (buf[GUARD + numel:] == fill).all())


def _edt(src: np.ndarray, sites: int, threshold=0.5, again=False):
    """vk_edt_sq through the C ABI into guarded buffers -> int32 numpy of the shape of src."""
    b, h, w = src.shape
    t = torch.from_numpy(src).to(DEV)
    kind = L.VK_EDT_SRC_U8 if src.dtype == np.uint8 else L.VK_EDT_SRC_F32
    n = b * h * w
    dbuf, d2 = _guarded(n, torch.int32, I_SENTINEL)
    need = int(L.lib().vk_edt_workspace_bytes(b, h, w))
    assert need == 4 * n
    wbuf, ws = _guarded(n, torch.int32, I_SENTINEL)
    outs = []
    for _ in range(2 if again else 1):
        L.check(L.lib().vk_edt_sq(b, h, w, t.data_ptr(), kind, threshold, sites, d2.data_ptr(), ws.data_ptr(), need, L.current_stream()), "vk_edt_sq")
        torch.cuda.synchronize()
        assert _guards_intact(dbuf, n, I_SENTINEL) and _guards_intact(wbuf, n, I_SENTINEL), "write beyond a buffer"
        outs.append(d2.view(b, h, w).cpu().numpy())
        assert (outs[-1] != I_SENTINEL).all(), "output not fully overwritten"
    if again:
        assert np.array_equal(outs[0], outs[1]), "a second call into the same buffers differs"
    return outs[0]


# ------------------------------------------------------------------------------------------------ the transform
@pytest.mark.parametrize("shape", BC.GPU_SHAPES, ids=["%dx%d" % s for s in BC.GPU_SHAPES])
def test_edt_equals_the_restatement(shape):
    h, w = shape
    pats = BC.patterns(h, w)
    u8 = np.stack([m for _, m in pats])
    f32 = np.stack([BC.as_f32(m, seed=i) for i, (_, m) in enumerate(pats)])
    for s in BC.SITES:
        want = R.edt_sq(u8, s)
        for form, bit in FORMS:
            got = _edt(u8, SITE_CODE[s] | bit, again=(form == "auto"))
            for i, (name, _) in enumerate(pats):
                assert np.array_equal(got[i], want[i]), (shape, s, form, name, np.argwhere(got[i] != want[i])[:4])
            got = _edt(f32, SITE_CODE[s] | bit)
            assert np.array_equal(got, want), (shape, s, form, "f32")
    # uint8 foreground is "!= 0", whatever the value; another fp32 threshold moves the foreground
    assert np.array_equal(_edt(u8 * np.uint8(255), L.VK_EDT_FG), R.edt_sq(u8, "fg"))
    assert np.array_equal(_edt(f32, L.VK_EDT_FG, threshold=0.95), np.full(u8.shape, R.NONE, np.int32))


def test_edt_batch_with_an_empty_image_in_the_middle():
    a, b = BC.random_pair(33, 65)
    src = np.stack([a, np.zeros_like(a), b])
    for s in BC.SITES:
        for _, bit in FORMS:
            got = _edt(src, SITE_CODE[s] | bit, again=True)
            assert np.array_equal(got, R.edt_sq(src, s)), s
            if s != "bg":
                assert (got[1] == R.NONE).all() and (got[0] != R.NONE).all() and (got[2] != R.NONE).all()


def test_edt_real_mask_512():
    m = BC.letterboxed(BC.real_mask(GOLDEN, 5), 512)[None]
    assert 1000 < m.sum() < 512 * 512 // 2
    for s in BC.SITES:
        want = R.edt_sq(m, s)
        for _, bit in FORMS:
            assert np.array_equal(_edt(m, SITE_CODE[s] | bit), want), s
    t = torch.from_numpy(m).to(DEV)
    assert torch.equal(B.edt_sq(t, "edge").cpu(), torch.from_numpy(R.edt_sq(m, "edge")))
    assert torch.equal(B.edt_sq(t.bool(), "fg", rows="envelope").cpu(), torch.from_numpy(R.edt_sq(m, "fg")))
    assert torch.equal(B.signed_distance(t).cpu(), torch.from_numpy(R.phi(m[0]))[None])


# ------------------------------------------------------------------------------------------------ phi
D2_MAX = 2 * 4095 * 4095                    # 33,538,050


@pytest.mark.parametrize("side", ["background", "foreground"])
def test_phi_is_exact_on_every_d2(side):
    """Every integer d^2 from 0 to 2 * 4095^2, fed directly as the map: phi must equal numpy's float64 square root cast to float32.  This
    also says that the device's fp64 square root is correctly rounded."""
    b, h, w = 2, 4096, 4096
    n = b * h * w
    assert n > D2_MAX
    vals = torch.arange(n, dtype=torch.int32, device=DEV).clamp_(max=D2_MAX)
    zeros = torch.zeros(n, dtype=torch.int32, device=DEV)
    pbuf, phi = _guarded(n, torch.float32, F_SENTINEL)
    d_fg, d_bg = (vals, zeros) if side == "background" else (zeros, vals)
    L.check(L.lib().vk_boundary_phi(b, h, w, d_fg.data_ptr(), d_bg.data_ptr(), phi.data_ptr(), L.current_stream()), "vk_boundary_phi")
    torch.cuda.synchronize()
    assert _guards_intact(pbuf, n, F_SENTINEL)
    got = phi.cpu().numpy()
    v = np.minimum(np.arange(n, dtype=np.int64), D2_MAX)
    root = np.sqrt(v.astype(np.float64))
    if side == "background":
        want = np.where(v > 0, root, 1.0).astype(np.float32)          # d2_fg = d2_bg = 0 reads as a foreground pixel: 1 - sqrt(0)
    else:
        want = (1.0 - root).astype(np.float32)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (side, bad.size, bad[:8], got[bad[:8]], want[bad[:8]])


def test_phi_of_maps_and_of_empty_and_full_images():
    a, b = BC.random_pair(33, 65)
    src = np.stack([a, np.zeros_like(a), np.ones_like(a), b])
    n = src.size
    d_fg = torch.from_numpy(_edt(src, L.VK_EDT_FG)).to(DEV)
    d_bg = torch.from_numpy(_edt(src, L.VK_EDT_BG)).to(DEV)
    pbuf, phi = _guarded(n, torch.float32, F_SENTINEL)
    L.check(L.lib().vk_boundary_phi(4, 33, 65, d_fg.data_ptr(), d_bg.data_ptr(), phi.data_ptr(), L.current_stream()), "vk_boundary_phi")
    torch.cuda.synchronize()
    got = phi.view(4, 33, 65).cpu().numpy()
    assert _guards_intact(pbuf, n, F_SENTINEL)
    assert np.array_equal(got, np.stack([R.phi(m) for m in src])) and (got[1] == 0).all() and (got[2] == 0).all() and (got[0] != 0).any()
    assert torch.equal(B.signed_distance(torch.from_numpy(src).to(DEV)).cpu(), torch.from_numpy(got))
    f = torch.from_numpy(np.stack([BC.as_f32(m) for m in src])).to(DEV).view(2, 2, 33, 65)
    assert torch.equal(B.signed_distance(f).cpu().view(4, 33, 65), torch.from_numpy(got))


# ------------------------------------------------------------------------------------------------ the statistics
def _stats(pred: np.ndarray, gt: np.ndarray, tol2=BC.TOL2, band2=BC.BAND2, pt=0.5, gtt=0.5):
    """vk_boundary_stats through the C ABI, twice into guarded buffers -> the records (numpy structured array)."""
    b, h, w = pred.shape
    p, g = torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV)
    kinds = [L.VK_EDT_SRC_U8 if a.dtype == np.uint8 else L.VK_EDT_SRC_F32 for a in (pred, gt)]
    need = int(L.lib().vk_boundary_stats_workspace_bytes(b, h, w))
    assert need % 8 == 0
    wbuf, ws = _guarded(need // 8, torch.int64, I_SENTINEL)
    words = b * B.RECORD_DTYPE.itemsize // 8
    obuf, out = _guarded(words, torch.int64, I_SENTINEL)
    t2 = (C.c_int32 * 8)(*tol2)
    runs = []
    for _ in range(2):
        L.check(L.lib().vk_boundary_stats(b, h, w, p.data_ptr(), kinds[0], pt, g.data_ptr(), kinds[1], gtt, len(tol2), t2, band2, out.data_ptr(),
                                          ws.data_ptr(), need, L.current_stream()), "vk_boundary_stats")
        torch.cuda.synchronize()
        assert _guards_intact(obuf, words, I_SENTINEL) and _guards_intact(wbuf, need // 8, I_SENTINEL), "write beyond a buffer"
        runs.append(out.cpu().numpy().tobytes())
    assert runs[0] == runs[1], "two runs differ in their bits"
    recs = np.frombuffer(runs[0], dtype=B.RECORD_DTYPE)
    assert (recs["reserved"] == 0).all()
    return recs


def _check_record(rec, want, name):
    for f in R.STAT_INT_FIELDS:
        assert int(rec[f]) == want[f], (name, f, int(rec[f]), want[f])
    for tag, n in (("pg", want["n_pred"]), ("gp", want["n_gt"])):
        assert rec["within_" + tag].tolist() == want["within_" + tag], (name, tag)
        s = want["sum_" + tag]
        print(name, "sum_" + tag, float(rec["sum_" + tag]), s)
        assert abs(float(rec["sum_" + tag]) - s) <= (n + 1) * 2.0 ** -53 * s, (name, tag, float(rec["sum_" + tag]), s)


def test_stats_on_the_cpu_cases():
    cases = BC.pair_cases()
    recs = _stats(np.stack([p for _, p, _ in cases]), np.stack([g for _, _, g in cases]))
    for rec, (name, p, g) in zip(recs, cases):
        _check_record(rec, R.stats(p, g, tol2=BC.TOL2, band2=BC.BAND2), name)
    assert recs[0]["max2_pg"] == 25 and recs[0]["n_pred"] == 76 and recs[0]["q95_2_pg"] == 17
    assert abs((recs[0]["sum_pg"] + recs[0]["sum_gp"]) / 152 - 3.2316540947811) < 1e-12


@pytest.mark.parametrize("shape", [(33, 65), (96, 200)], ids=["33x65", "96x200"])
def test_stats_on_random_pairs(shape):
    pairs = [BC.random_pair(*shape, seed=s) for s in (5, 6, 7)]
    pred = np.stack([p for p, _ in pairs])
    gt = np.stack([g for _, g in pairs])
    for rec, (p, g) in zip(_stats(pred, gt), pairs):
        _check_record(rec, R.stats(p, g, tol2=BC.TOL2, band2=BC.BAND2), shape)
    # fp32 prediction with its own threshold against a uint8 label; eight tolerances, another band
    prob = np.stack([BC.as_f32(p, threshold=0.3) for p in pred])
    tol2 = (0, 1, 2, 4, 9, 16, 100, 40000)
    for rec, (p, g) in zip(_stats(prob, gt, tol2=tol2, band2=9, pt=0.3), pairs):
        _check_record(rec, R.stats(p, g, tol2=tol2, band2=9), shape)


def test_stats_on_a_real_mask_shifted():
    m = BC.letterboxed(BC.real_mask(GOLDEN, 2), 256)
    s = BC.shifted(m, 2, 1)
    rec = _stats(s[None], m[None])[0]
    want = R.stats(s, m, tol2=BC.TOL2, band2=BC.BAND2)
    _check_record(rec, want, "real")
    assert 0 < want["max2_pg"] <= 5 and want["n_pred"] > 100


# ------------------------------------------------------------------------------------------------ the loss
LOSS_SHAPE = (2, 3, 37, 29)                 # count = 6438: vectors of four with a tail of two, seven workgroups


def _phi_for_loss():
    rng = np.random.default_rng(3)
    maps = []
    for i in range(LOSS_SHAPE[0] * LOSS_SHAPE[1]):
        a, b = BC.random_pair(LOSS_SHAPE[2], LOSS_SHAPE[3], seed=20 + i)
        maps.append(a if rng.random() < 0.5 else b)
    return np.stack([R.phi(m) for m in maps]).reshape(LOSS_SHAPE)


def _loss(x: np.ndarray, phi: np.ndarray, grad_scale=1.0, want_grad=True, shift=0):
    """vk_boundary_loss through the C ABI; shift: offset of every tensor in floats (1: no 16-byte alignment, the scalar path)."""
    n, c = x.shape[0], x.shape[1]
    count = x.size

    def dev(a):
        t = torch.empty(count + shift, dtype=torch.float32, device=DEV)
        t[shift:] = torch.from_numpy(np.ascontiguousarray(a, np.float32).ravel()).to(DEV)
        return t[shift:]

    xd, fd = dev(x), dev(phi)
    gbuf = torch.full((count + 2 * GUARD + shift,), F_SENTINEL, dtype=torch.float32, device=DEV)
    g = gbuf[GUARD + shift:GUARD + shift + count]
    lbuf, out = _guarded(1, torch.float32, F_SENTINEL)
    ws = torch.empty(L.VK_BOUNDARY_LOSS_WS_BYTES // 8, dtype=torch.float64, device=DEV)
    L.check(L.lib().vk_boundary_loss(n, c, count // (n * c), xd.data_ptr(), fd.data_ptr(), grad_scale, g.data_ptr() if want_grad else None,
                                     out.data_ptr(), ws.data_ptr(), L.VK_BOUNDARY_LOSS_WS_BYTES, L.current_stream()), "vk_boundary_loss")
    torch.cuda.synchronize()
    lo = GUARD + shift
    assert bool((gbuf[:lo] == F_SENTINEL).all() and (gbuf[lo + count:] == F_SENTINEL).all()) and _guards_intact(lbuf, 1, F_SENTINEL)
    gn = g.cpu().numpy().reshape(x.shape)
    assert (gn != np.float32(F_SENTINEL)).all() if want_grad else (gn == np.float32(F_SENTINEL)).all()
    return np.float32(out.item()), gn


@pytest.mark.parametrize("shift", [0, 1], ids=["vector", "scalar"])
def test_loss_at_zero_logits_is_exact(shift):
    phi = _phi_for_loss()
    assert (phi > 0).any() and (phi < 0).any()
    v, g = _loss(np.zeros(LOSS_SHAPE, np.float32), phi, shift=shift)
    f64 = phi.astype(np.float64)
    assert v == np.float32(0.5 * f64.sum() / phi.size), (v, 0.5 * f64.sum() / phi.size)
    assert np.array_equal(g, (f64 / 4 / phi.size).astype(np.float32))
    v3, g3 = _loss(np.zeros(LOSS_SHAPE, np.float32), phi, grad_scale=3.0, shift=shift)
    assert v3 == v and np.array_equal(g3, (f64 * 0.25 * 3.0 / phi.size).astype(np.float32))
    assert _loss(np.zeros(LOSS_SHAPE, np.float32), phi, want_grad=False, shift=shift)[0] == v


def _loss_bounds(x, phi):
    """Counted along k_bl_main.  p and 1 - p are r = 1 / (1 + e) or e r, e = expf(-|x|): the sigmoid expression (K_FUNC x 2^-24 relative,
    P_FLOOR absolute where expf underflows) and at most one more fp32 product, so (K_FUNC + 1) x 2^-24 each.
      value: p phi and the sums are fp64 (2^-53 per operation: 1e-12 relative to sum |p phi| covers them); the mean is rounded once to
             fp32: sum |p phi| (K_FUNC + 1) 2^-24 / count + max |phi| P_FLOOR + 2^-24 |value|.
      gradient: p (1 - p) is one fp32 product of two such factors, (2 (K_FUNC + 1) + 1) x 2^-24; the rest is fp64 and one rounding to
             fp32: |g| (2 (K_FUNC + 1) + 2) 2^-24, with 1e-6 relative for the second-order terms, plus |phi| P_FLOOR / count; where a
             factor or the result is subnormal in fp32 the error is a multiple of the spacing TINY instead: |phi| (K_FUNC + 2) TINY /
             count for the product and TINY for the last rounding."""
    p = R.sigmoid64(x)
    f = np.abs(phi.astype(np.float64))
    v, g = R.loss(x, phi)
    bv = ((p * f).sum() * ((K_FUNC + 1.0) * U32 * (1.0 + 1e-6) + 1e-12) / x.size + f.max() * P_FLOOR + U32 * abs(v))
    bg = np.abs(g) * (2.0 * (K_FUNC + 1.0) + 2.0) * U32 * (1.0 + 1e-6) + f * (P_FLOOR + (K_FUNC + 2.0) * TINY) / x.size + TINY
    return v, g, bv, bg


@pytest.mark.parametrize("shift", [0, 1], ids=["vector", "scalar"])
def test_loss_on_random_logits(shift):
    phi = _phi_for_loss()
    rng = np.random.default_rng(11)
    x = (rng.normal(size=LOSS_SHAPE) * 4.0).astype(np.float32)
    x.ravel()[:6] = (-100.0, 100.0, -30.0, 30.0, 0.0, -0.0)
    v, g = _loss(x, phi, shift=shift)
    rv, rg, bv, bg = _loss_bounds(x, phi)
    print("value", float(v), rv, "err", abs(float(v) - rv), "bound", bv)
    err = np.abs(g.astype(np.float64) - rg)
    print("gradient: max err / bound", float((err / np.maximum(bg, 1e-300)).max()))
    assert abs(float(v) - rv) <= bv
    assert (err <= bg).all(), (err.max(), np.argmax(err - bg))
    v2, g2 = _loss(x, phi, shift=shift)
    assert v2.tobytes() == v.tobytes() and g2.tobytes() == g.tobytes(), "two runs differ in their bits"


def test_boundary_loss_module_through_autograd():
    phi = _phi_for_loss()
    rng = np.random.default_rng(12)
    x = (rng.normal(size=LOSS_SHAPE) * 3.0).astype(np.float32)
    v, g = _loss(x, phi)
    logits = torch.from_numpy(x).to(DEV).requires_grad_(True)
    dist = torch.from_numpy(phi).to(DEV)
    loss = vk.BoundaryLoss()(logits, dist=dist)
    assert loss.shape == () and loss.item() == v
    loss.backward()
    assert torch.equal(logits.grad.cpu(), torch.from_numpy(g))
    # phi built from the target under no_grad; a weighted sum with another loss backpropagates
    y = torch.from_numpy(np.stack([BC.random_pair(64, 64, seed=s)[0] for s in (1, 2)])).to(DEV).float().view(2, 1, 64, 64)
    l2 = torch.randn(2, 1, 64, 64, device=DEV, requires_grad=True)
    bl = vk.BoundaryLoss()(l2, y)
    assert bl.item() == vk.BoundaryLoss()(l2.detach(), dist=B.signed_distance(y)).item()
    total = vk.DiceLoss(mode="binary")(l2, y) + 0.01 * bl
    total.backward()
    gd = l2.grad.clone()
    l2.grad = None
    vk.DiceLoss(mode="binary")(l2, y).backward()
    g_dice = l2.grad.clone()
    l2.grad = None
    vk.BoundaryLoss()(l2, y).backward()
    assert torch.isfinite(gd).all() and (l2.grad != 0).any()
    assert torch.allclose(gd, g_dice + 0.01 * l2.grad, rtol=1e-6, atol=1e-12)
    with torch.no_grad():
        assert not vk.BoundaryLoss()(l2, y).requires_grad


# ------------------------------------------------------------------------------------------------ metrics
def test_metrics_over_uneven_batches_equal_their_union():
    cases = BC.pair_cases()
    pred = torch.from_numpy(np.stack([p for _, p, _ in cases])).to(DEV)
    gt = torch.from_numpy(np.stack([g for _, _, g in cases])).to(DEV)
    n = len(cases)
    scale = np.linspace(1.0, 2.0, n)
    whole = B.surface_metrics(pred, gt, tolerances=BC.TOLERANCES, band=2, scale=scale)
    bm = vk.BoundaryMetrics(tolerances=BC.TOLERANCES, band=2)
    bm.update(pred[:2], gt[:2], scale=scale[:2])
    bm.update(pred[2:], gt[2:], scale=scale[2:])
    assert bm.n_images == n and bm.n_batches == 2
    got = bm.compute()
    for key in ("hd", "hd95", "assd", "boundary_iou"):
        assert np.array_equal(got[key], whole[key]), key
        assert got["mean"][key] == whole["mean"][key] or (np.isnan(got["mean"][key]) and np.isnan(whole["mean"][key])), key
    for t in BC.TOLERANCES:
        assert np.array_equal(got["nsd"][t], whole["nsd"][t]) and got["mean"]["nsd"][t] == whole["mean"]["nsd"][t]
    for i, (name, p, g) in enumerate(cases):
        want = R.metrics(R.stats(p, g, tol2=BC.TOL2, band2=BC.BAND2), 3, scale[i])
        assert whole["hd"][i] == want["hd"] and whole["hd95"][i] == want["hd95"] and whole["boundary_iou"][i] == want["boundary_iou"], name
        assert whole["assd"][i] == want["assd"] or abs(whole["assd"][i] - want["assd"]) <= 1e-13 * want["assd"], name
        assert [whole["nsd"][t][i] for t in BC.TOLERANCES] == want["nsd"], name
    assert whole["hd"][0] == 5.0 * scale[0]
    # probabilities and logits in front of the same masks
    prob = torch.from_numpy(np.stack([BC.as_f32(p) for _, p, _ in cases])).to(DEV)
    assert np.array_equal(B.surface_metrics(prob, gt, band=2, scale=scale)["hd"], whole["hd"])
    logit = torch.where(pred != 0, 2.0, -2.0)
    assert np.array_equal(B.surface_metrics(logit, gt, band=2, scale=scale, from_logits=True)["assd"], whole["assd"])
    bm.reset()
    assert bm.n_images == 0
