"""vk.copypaste on the MI355X: vk_cp_boxes, vk_cp_alpha and vk_cp_paste against the numpy restatement of copypaste_ref.py, then
InstanceBank / CopyPaste end to end on a small built dataset.  Integer arithmetic throughout: every comparison is EXACT
(np.array_equal / torch.equal).  Outputs of the C ABI go into sentinel-filled buffers with a guard zone on both sides; every output
byte must be overwritten and no guard byte touched."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import copypaste_cases as CC
import copypaste_ref as R
import geom_cases as GC
import instances_ref as IR

pytestmark = pytest.mark.gpu
vk = importlib.import_module("vickers-hardness-unet_amd")
L = vk._lib
DEV = torch.device("cuda:0")
GUARD = 256           # bytes / elements on either side of an output
SENTINEL = 7          # no value of a {0,1} map; alpha and RGB are compared with the reference
I_SENTINEL = -(2 ** 31)


def _guarded(numel, dtype, fill):
    """(whole buffer, the view between the two guard zones)."""
    buf = torch.full((numel + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + numel]


def _guards_intact(buf, numel, fill):
    return bool((buf[:GUARD] == fill).all() and (buf[GUARD + numel:] == fill).all())


# ------------------------------------------------------------------------------------------------ boxes and alpha
@pytest.mark.parametrize("case", CC.slot_map_cases(), ids=[c[0] for c in CC.slot_map_cases()])
def test_boxes_and_alpha(case):
    _, slots, M = case
    B, h, w = slots.shape
    sl = torch.from_numpy(slots).to(DEV)
    bbuf, boxes = _guarded(B * M * 5, torch.int32, I_SENTINEL)
    kbuf, kept = _guarded(B * h * w, torch.uint8, SENTINEL)
    abuf, alpha = _guarded(B * h * w, torch.uint8, SENTINEL)
    st = L.current_stream()
    L.check(L.lib().vk_cp_boxes(B, h, w, sl.data_ptr(), M, boxes.data_ptr(), st), "vk_cp_boxes")
    L.check(L.lib().vk_cp_alpha(B, h, w, sl.data_ptr(), kept.data_ptr(), alpha.data_ptr(), st), "vk_cp_alpha")
    torch.cuda.synchronize()
    assert _guards_intact(bbuf, B * M * 5, I_SENTINEL) and _guards_intact(kbuf, B * h * w, SENTINEL) and _guards_intact(abuf, B * h * w, SENTINEL)
    want_k, want_a = R.kept_alpha_ref(slots)
    assert np.array_equal(boxes.view(B, M, 5).cpu().numpy(), R.boxes_ref(slots, M))
    assert np.array_equal(kept.view(B, h, w).cpu().numpy(), want_k)
    assert np.array_equal(alpha.view(B, h, w).cpu().numpy(), want_a)
    # a second call into the same buffer gives the same boxes: the call initialises them itself
    L.check(L.lib().vk_cp_boxes(B, h, w, sl.data_ptr(), M, boxes.data_ptr(), st), "vk_cp_boxes")
    assert np.array_equal(boxes.view(B, M, 5).cpu().numpy(), R.boxes_ref(slots, M))


# ------------------------------------------------------------------------------------------------ paste
@pytest.fixture(scope="module")
def stores():
    return {S: CC.stores(S) for S in CC.PASTE_SIZES}


def _paste(S, host, base, pastes):
    """vk_cp_paste through the C ABI into guarded, sentinel-filled outputs -> numpy (rgb, mask)."""
    images, masks, kept, alpha = (torch.from_numpy(a).to(DEV) for a in host)
    n = len(base)
    counts, recs = vk.copypaste._recs_array(pastes)
    rbuf, rgb = _guarded(n * S * S * 3, torch.uint8, SENTINEL)
    mbuf, msk = _guarded(n * S * S, torch.uint8, SENTINEL)
    dbuf, rdev = _guarded(L.vk_cp_recs_dev_bytes(n) // 4, torch.int32, I_SENTINEL)
    bi = torch.tensor(base, dtype=torch.int32, device=DEV)
    L.check(L.lib().vk_cp_paste(n, S, images.shape[0], images.data_ptr(), masks.data_ptr(), kept.data_ptr(), alpha.data_ptr(), bi.data_ptr(),
                                counts, recs, rdev.data_ptr(), rgb.data_ptr(), msk.data_ptr(), L.current_stream()), "vk_cp_paste")
    torch.cuda.synchronize()
    assert _guards_intact(rbuf, n * S * S * 3, SENTINEL) and _guards_intact(mbuf, n * S * S, SENTINEL), "write beyond the outputs"
    assert _guards_intact(dbuf, L.vk_cp_recs_dev_bytes(n) // 4, I_SENTINEL), "write beyond the record scratch"
    m = msk.view(n, S, S).cpu().numpy()
    assert np.isin(m, (0, 1)).all(), "mask not fully overwritten"
    return rgb.view(n, S, S, 3).cpu().numpy(), m


@pytest.mark.parametrize("S", CC.PASTE_SIZES)
def test_paste(S, stores):
    base, pastes = CC.paste_cases(S)
    want_rgb, want_m = R.compose_ref(*stores[S], base, pastes)
    rgb, m = _paste(S, stores[S], base, pastes)
    for j in range(len(base)):
        assert np.array_equal(m[j], want_m[j]), (S, j)
        assert np.array_equal(rgb[j], want_rgb[j]), (S, j, np.argwhere((rgb[j] != want_rgb[j]).any(axis=2))[:4])
    # the sentinel is a legal RGB value: run again over another fill, so that a pixel left unwritten shows in one of the two
    images, masks, kept, alpha = (torch.from_numpy(a).to(DEV) for a in stores[S])
    n = len(base)
    counts, recs = vk.copypaste._recs_array(pastes)
    out = torch.full((n, S, S, 3), 200, dtype=torch.uint8, device=DEV)
    om = torch.full((n, S, S), 200, dtype=torch.uint8, device=DEV)
    rdev = torch.empty(L.vk_cp_recs_dev_bytes(n) // 4, dtype=torch.int32, device=DEV)
    bi = torch.tensor(base, dtype=torch.int32, device=DEV)
    L.check(L.lib().vk_cp_paste(n, S, CC.N_ITEMS, images.data_ptr(), masks.data_ptr(), kept.data_ptr(), alpha.data_ptr(), bi.data_ptr(), counts,
                                recs, rdev.data_ptr(), out.data_ptr(), om.data_ptr(), L.current_stream()), "vk_cp_paste")
    assert np.array_equal(out.cpu().numpy(), want_rgb) and np.array_equal(om.cpu().numpy(), want_m)


def test_paste_single_sample_and_largest_count(stores):
    """n = 1 with eight records, and the same records one sample each: a sample depends on its own list alone."""
    S = 36
    base, pastes = CC.paste_cases(S)
    rgb, m = _paste(S, stores[S], [base[1]], [pastes[1]])
    want_rgb, want_m = R.compose_ref(*stores[S], [base[1]], [pastes[1]])
    assert np.array_equal(rgb, want_rgb) and np.array_equal(m, want_m)
    singles = [[r] for r in pastes[4][:6]]
    rgb, m = _paste(S, stores[S], [base[4]] * 6, singles)
    want_rgb, want_m = R.compose_ref(*stores[S], [base[4]] * 6, singles)
    assert np.array_equal(rgb, want_rgb) and np.array_equal(m, want_m)


# ------------------------------------------------------------------------------------------------ end to end
S_DS = 64
SHAPES = [(64, 64), (40, 64), (64, 48), (30, 30), (64, 64)]


def _raws():
    rng = np.random.default_rng(77)
    imgs = [rng.integers(0, 256, size=(h, w, 3)).astype(np.uint8) for h, w in SHAPES]
    masks = [np.zeros((h, w), np.uint8) for h, w in SHAPES]
    masks[0][8:26, 6:24] = 255                      # 18 x 18 = 324 px: a donor under the default min_area of 200
    masks[0][40:60, 36:58] = 255                    # a second one, far from the first
    masks[1][10:30, 20:44] = 1
    masks[2][5:25, 4:20] = 255                      # two whose grown boxes meet: neither gives
    masks[2][5:25, 27:44] = 255
    masks[2][50:53, 40:43] = 255                    # and a small one
    masks[4][20:50, 10:50] = 255                    # item 3 holds nothing
    return imgs, masks


@pytest.fixture(scope="module")
def built():
    imgs, masks = _raws()
    ds = vk.DeviceDataset(imgs, masks, img_size=S_DS, device=DEV, names=["i%d" % i for i in range(len(imgs))])
    bank = vk.InstanceBank(ds)
    return ds, bank


def _bank_ref(ds, **kw):
    masks = ds.masks.cpu().numpy()
    cfg = GC.Cfg(thresh=0.5, k=1, min_area=1, cap=256)
    slots = np.stack([IR.slot_map_ref(m.astype(np.float32), cfg)[0] for m in masks])
    counts = np.array([IR.slot_map_ref(m.astype(np.float32), cfg)[1] for m in masks])
    kept, alpha = R.kept_alpha_ref(slots)
    boxes = R.boxes_ref(slots, 256)
    return boxes, counts, kept, alpha, R.records_ref(boxes, counts, ds.content, ds.S, **kw)


def test_bank_equals_the_restatement(built):
    ds, bank = built
    assert ds.content.dtype == np.int32 and ds.content.shape == (5, 4) and ds.content[0].tolist() == [0, 0, 64, 64]
    for i, (top, left, nh, nw) in enumerate(ds.content.tolist()):
        m = ds.masks[i].cpu().numpy()
        inside = np.zeros_like(m, bool)
        inside[top:top + nh, left:left + nw] = True
        assert not m[~inside].any() and (nh == S_DS or nw == S_DS)
    boxes, counts, kept, alpha, records = _bank_ref(ds)
    assert counts.tolist() == [2, 1, 3, 0, 1]
    assert np.array_equal(bank.boxes, boxes) and np.array_equal(bank.counts, counts)
    assert np.array_equal(bank.kept.cpu().numpy(), kept) and np.array_equal(bank.alpha.cpu().numpy(), alpha)
    assert bank.records.dtype == R.RECORD_DT and np.array_equal(bank.records, records)
    assert bank.records["donor"].tolist() == [1, 1, 1, 0, 0, 0, 1] and len(bank.donors) == 4
    small = vk.InstanceBank(ds, max_components=2, margin=2, min_area=5)
    assert np.array_equal(small.records, _bank_ref(ds, max_components=2, margin=2, min_area=5)[4])
    assert small.records["donor"].tolist() == [1, 1, 1, 0, 0, 0, 1]          # item 2 holds three components: more than two


def _draws(n):
    sm = vk.AugmentSampler(seed=3)
    return [sm.sample() for _ in range(n)]


def test_batch_without_pastes_is_the_dataset_batch(built):
    ds, bank = built
    cp = vk.CopyPaste(ds, bank)
    idx = [4, 0, 2, 2, 3, 1]
    d = _draws(len(idx))
    x, y, names = cp.batch(idx, draws=d, pastes=[[]] * len(idx))
    x0, y0, names0 = ds.batch(idx, draws=d)
    assert torch.equal(x, x0) and torch.equal(y, y0) and names == names0 == ["i%d" % i for i in idx]
    x, y, _ = cp.batch(idx)                         # neither sampler: the validation pipeline
    x0, y0, _ = ds.batch(idx)
    assert torch.equal(x, x0) and torch.equal(y, y0)


def test_batch_with_pastes_is_augment_over_the_restatement(built):
    ds, bank = built
    cp = vk.CopyPaste(ds, bank)
    cps = vk.CopyPasteSampler(bank, seed=9, p=1.0, max_pastes=3, scale=(0.5, 1.25))
    idx = [3, 0, 1, 4, 3, 2]
    pastes = [cps.sample(i) for i in idx]
    assert sum(len(p) for p in pastes) >= 4
    d = _draws(len(idx))
    x, y, _ = cp.batch(idx, draws=d, pastes=pastes)
    x2, y2, _ = cp.batch(idx, draws=d, pastes=pastes)
    assert torch.equal(x, x2) and torch.equal(y, y2)
    rgb, msk = cp.compose(idx, pastes)
    _, _, kept, alpha, _ = _bank_ref(ds)
    want_rgb, want_m = R.compose_ref(ds.images.cpu().numpy(), ds.masks.cpu().numpy(), kept, alpha, idx, pastes)
    assert np.array_equal(rgb.cpu().numpy(), want_rgb) and np.array_equal(msk.cpu().numpy(), want_m)
    assert any((want_m[j] != ds.masks[i].cpu().numpy()).any() for j, i in enumerate(idx))
    # vk_augment_batch over the restatement's buffers, index 0..n-1
    n, S = len(idx), ds.S
    r_dev, m_dev = torch.from_numpy(want_rgb).to(DEV), torch.from_numpy(want_m).to(DEV)
    xe = torch.empty(n, 3, S, S, dtype=torch.float32, device=DEV)
    ye = torch.empty(n, 1, S, S, dtype=torch.float32, device=DEV)
    ws_bytes = int(L.lib().vk_augment_workspace_bytes(n, S))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    pdev = torch.empty(n * C.sizeof(L.vk_aug_params), dtype=torch.uint8, device=DEV)
    L.check(L.lib().vk_augment_batch(n, S, n, r_dev.data_ptr(), m_dev.data_ptr(), torch.arange(n, dtype=torch.int32, device=DEV).data_ptr(),
                                     vk.augment._params_array(d, S), pdev.data_ptr(), ds._tables.data_ptr(), ws.data_ptr(), ws_bytes, xe.data_ptr(),
                                     ye.data_ptr(), L.current_stream()), "vk_augment_batch")
    assert torch.equal(x, xe) and torch.equal(y, ye)


def test_loader_and_argument_errors(built):
    ds, bank = built
    cp = vk.CopyPaste(ds, bank)
    cps = vk.CopyPasteSampler(bank, seed=2, p=1.0)
    batches = list(cp.loader(batch_size=2, shuffle=True, sampler=vk.AugmentSampler(seed=1, clahe="skip"), cp_sampler=cps, seed=4))
    assert [b[0].shape[0] for b in batches] == [2, 2, 1] and batches[0][0].shape == (2, 3, S_DS, S_DS) and batches[0][1].shape == (2, 1, S_DS, S_DS)
    assert sorted(sum((b[2] for b in batches), [])) == ["i%d" % i for i in range(5)]
    assert all(set(torch.unique(b[1]).tolist()) <= {0.0, 1.0} and torch.isfinite(b[0]).all() for b in batches)
    good = R.rec(0, 2, 4, 26, 26, 0, 30, 30, 26, 26)
    with pytest.raises(ValueError):
        cp.compose([5], [[]])
    with pytest.raises(ValueError):
        cp.compose([0, 1], [[]])
    with pytest.raises(ValueError):
        cp.compose([], [])
    with pytest.raises(ValueError, match="at most 8"):
        cp.compose([0], [[good] * 9])
    with pytest.raises(ValueError):
        cp.batch([0, 1], draws=_draws(1))
    with pytest.raises(ValueError):
        list(cp.loader(batch_size=0))
    for bad, word in ((dict(donor=5), "donor 5"), (dict(sw=64), "donor box"), (dict(d4=8), "d4 8"), (dict(dw=129), "destination size"),
                      (dict(dy0=-129), "destination origin")):
        with pytest.raises(vk.VkError, match=word):
            cp.compose([0], [[good, dict(good, **bad)]])
    other = vk.DeviceDataset(*[v[:1] for v in _raws()], img_size=32, device=DEV)
    with pytest.raises(ValueError, match="this dataset"):
        vk.CopyPaste(other, bank)
