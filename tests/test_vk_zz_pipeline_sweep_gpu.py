"""The augmentation, letterbox, pre/post-processing and metric kernels on the built cases of tests/pipeline_cases.py (-m gpu), against
oracle/augment_oracle.py, oracle/prepost_oracle.py and integer counts.  Every comparison is equality, with two stated exceptions:
probabilities pass through expf and keep the 2e-6 bar of tests/test_prepost_gpu.py, and the soft-target metric sums carry a bar derived
from the kernel's own accumulation.  No pixel is exempted.  tests/test_pipeline_cases_cpu.py proves the cases.  DESIGN.md 41."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import pipeline_cases as PC
from oracle import prepost_oracle as P

pytestmark = pytest.mark.gpu
vk = importlib.import_module("vickers-hardness-unet_amd")
L = vk._lib
DEV = torch.device("cuda:0")
G = PC.GUARD


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Guarded:
    """`nbytes` of device memory inside a larger allocation filled with 0xA5, 512 guard bytes either side (+ `shift` bytes in front)."""

    def __init__(self, nbytes, shift=0, fill=PC.FILL):
        self.n, self.off = int(nbytes), G + shift
        self.buf = torch.full((self.n + 2 * G + shift,), PC.FILL, dtype=torch.uint8, device=DEV)
        if fill != PC.FILL:
            self.buf[self.off:self.off + self.n] = fill
        self.ptr = self.buf.data_ptr() + self.off

    def body(self, dtype=np.uint8):
        return self.buf[self.off:self.off + self.n].cpu().numpy().view(dtype)

    def guards_ok(self):
        return bool((self.buf[:self.off] == PC.FILL).all()) and bool((self.buf[self.off + self.n:] == PC.FILL).all())


# ======================================================================================================= A. augmentation
_DS = {}


def _dataset(S):
    if S not in _DS:
        items = PC.items(S)
        ds = vk.DeviceDataset([np.ascontiguousarray(im[:, :, ::-1]) for _, im, _ in items], [m for _, _, m in items], img_size=S, device=DEV,
                              names=[n for n, _, _ in items])
        for i, (_, im, m) in enumerate(items):          # S x S sources take the copy path: the store is the built image itself
            assert np.array_equal(ds.images[i].cpu().numpy(), im) and np.array_equal(ds.masks[i].cpu().numpy(), m)
        _DS[S] = (items, ds)
    return _DS[S]


AUG_PARAMS = [(S, n) for S in PC.AUG_SIZES for n in PC.image_names(S)]


@pytest.mark.parametrize("S,name", AUG_PARAMS, ids=[f"{S}-{n}" for S, n in AUG_PARAMS])
def test_augment_equals_oracle(S, name):
    """The full d4 x rotation x photo x noise product and the rotation / RBC / noise / CLAHE families in ONE vk_augment_batch call per
    (S, image); every sample equals the oracle, and the properties that need no oracle hold on the device's own results."""
    items, ds = _dataset(S)
    i = [n for n, _, _ in items].index(name)
    _, img, m = items[i]
    draws = PC.all_draws(S)
    x, y, _ = ds.batch([i] * len(draws), draws=draws)
    xs, ys = x.cpu().numpy(), y.cpu().numpy()
    for j, d in enumerate(draws):
        xo, yo = PC.augment_ref(img, m, d)
        assert np.array_equal(ys[j], yo), (S, name, d["name"])
        assert np.array_equal(xs[j], xo), (S, name, d["name"], float(np.abs(xs[j] - xo).max()))
    at = PC.by_name(draws)
    plain = at["plain"]
    assert np.array_equal(xs[at["p-d40-r0-none-n0"]], xs[plain])
    assert np.array_equal(xs[at["rot-x(1,0)"]], xs[plain]) and np.array_equal(ys[at["rot-x(1,0)"]], ys[plain])
    for n, k in PC.EXACT_ROT_K.items():
        assert np.array_equal(xs[at["rot-" + n]], np.rot90(xs[plain], k, axes=(1, 2))), n
        assert np.array_equal(ys[at["rot-" + n]], np.rot90(ys[plain], k, axes=(1, 2))), n
    assert np.array_equal(xs[at["rbc(1,0)"]], xs[plain])
    assert set(np.unique(ys).tolist()) <= {0.0, 1.0}


def test_noise_field_is_the_seed_alone():
    """Two batch slots with one seed carry one noise field: a constant image under different D4 draws, masks and slots."""
    items, ds = _dataset(16)
    c = [n for n, _, _ in items].index("const137")
    noise = dict(noise_scale=PC.NOISE_SCALES[1], noise_seed=2 ** 31)
    draws = [dict(PC.IDENTITY, **noise), dict(PC.IDENTITY), dict(PC.IDENTITY, d4=4, **noise), dict(PC.IDENTITY, photo=3, blur_ksize=5, **noise),
             dict(PC.IDENTITY, d4=1, noise_scale=noise["noise_scale"], noise_seed=2 ** 31 + 1)]
    x, _, _ = ds.batch([c] * 5, draws=draws)
    assert torch.equal(x[0], x[2]) and torch.equal(x[0], x[3])              # blur and rot90 leave a constant image alone
    assert not torch.equal(x[0], x[1]) and not torch.equal(x[0], x[4])      # the noise is there, and another seed is another field
    # the constant 0 and 255 images: the field clipped from one side, as the oracle clips it
    for name in ("const0", "const255"):
        i = [n for n, _, _ in items].index(name)
        xn, _, _ = ds.batch([i], draws=[dict(PC.IDENTITY, **noise)])
        assert np.array_equal(xn[0].cpu().numpy(), PC.augment_ref(items[i][1], items[i][2], dict(PC.IDENTITY, **noise))[0])
        assert len(torch.unique(xn[0, 0])) > 1


@pytest.mark.parametrize("S", [16, 128])
@pytest.mark.parametrize("clahe", ["none", "some", "all"])
def test_batch_equals_single_sample_batches(S, clahe):
    """A batch of k draws equals k one-sample batches slot for slot (CLAHE workspace slot indexing), with repeated items."""
    items, ds = _dataset(S)
    at, draws = PC.by_name(PC.all_draws(S)), PC.all_draws(S)
    pick = {"none": ["p-d44-r1-blur5-n1", "plain", "rbc(0.8,0.2)", "p-d46-r1-none-n1", "rot-m(45)", "p-d42-r0-blur3-n0"],
            "some": ["p-d44-r1-blur5-n1", "clahe-2", "plain", "clahe-40-d4_1-rot", "p-d45-r1-clahe-n1", "rot-m(45)"],
            "all": ["clahe-1", "clahe-1.37-d4_1-rot", "clahe-2", "p-d46-r0-clahe-n1", "clahe-40", "p-d43-r1-clahe-n0"]}[clahe]
    ds_draws = [draws[at[n]] for n in pick]
    idx = [0, 6, 0, 7, 9, 6]                                                # random, levels, random, tiles, levels33, levels
    x, y, _ = ds.batch(idx, draws=ds_draws)
    x, y = x.clone(), y.clone()
    for j in range(len(idx)):
        xj, yj, _ = ds.batch([idx[j]], draws=[ds_draws[j]])
        assert torch.equal(xj[0], x[j]) and torch.equal(yj[0], y[j]), (j, pick[j])
        xo, yo = PC.augment_ref(items[idx[j]][1], items[idx[j]][2], ds_draws[j])
        assert np.array_equal(xj[0].cpu().numpy(), xo) and np.array_equal(yj[0].cpu().numpy(), yo), (j, pick[j])


def test_batches_of_1_and_70_and_the_clamped_index():
    """n = 1; n = 70 at S = 8, above the 64-entry initial parameter buffer, followed by a smaller batch on the same dataset; item indices
    -5 and 99 are items 0 and n_items - 1 exactly."""
    items = PC.items(8)
    ds = vk.DeviceDataset([np.ascontiguousarray(im[:, :, ::-1]) for _, im, _ in items], [m for _, _, m in items], img_size=8, device=DEV)
    draws = PC.all_draws(8)
    n_items = len(items)

    def check(idx, dr):
        x, y, _ = ds.batch(idx, draws=dr)
        xs, ys = x.cpu().numpy(), y.cpu().numpy()
        for j, (i, d) in enumerate(zip(idx, dr)):
            xo, yo = PC.augment_ref(items[i][1], items[i][2], d)
            assert np.array_equal(xs[j], xo) and np.array_equal(ys[j], yo), (len(idx), j, d["name"])

    check([4], [draws[17]])
    assert ds._params_dev.numel() == 64 * C.sizeof(L.vk_aug_params)
    idx70 = [(3 * j) % n_items for j in range(70)]
    check(idx70, [draws[(11 * j) % len(draws)] for j in range(70)])
    assert ds._params_dev.numel() == 70 * C.sizeof(L.vk_aug_params)
    check([1, 8, 8], [draws[5], draws[140 % len(draws)], draws[33]])
    d3 = [draws[9], draws[40], draws[77]]
    lo, _, _ = ds.batch([-5, -1, 0], draws=d3)
    lo = lo.clone()
    z, _, _ = ds.batch([0, 0, 0], draws=d3)
    assert torch.equal(lo, z)
    hi, yh, _ = ds.batch([99, n_items, 2 ** 31 - 1], draws=d3)
    hi, yh = hi.clone(), yh.clone()
    last, yl, _ = ds.batch([n_items - 1] * 3, draws=d3)
    assert torch.equal(hi, last) and torch.equal(yh, yl)


def _augment_abi(ds, S, idx, draws, ws_fill):
    lib, n = L.lib(), len(idx)
    arr = vk.augment._params_array(draws, S)
    x, y = Guarded(n * 3 * S * S * 4), Guarded(n * S * S * 4)
    ws_bytes = int(lib.vk_augment_workspace_bytes(n, S))
    ws = Guarded(ws_bytes, fill=ws_fill)
    pdev = torch.empty(n * C.sizeof(L.vk_aug_params), dtype=torch.uint8, device=DEV)
    index = torch.tensor(idx, dtype=torch.int32, device=DEV)
    L.check(lib.vk_augment_batch(n, S, len(ds), ds.images.data_ptr(), ds.masks.data_ptr(), index.data_ptr(), arr, pdev.data_ptr(),
                                 ds._tables.data_ptr(), ws.ptr, ws_bytes, x.ptr, y.ptr, L.current_stream()), "vk_augment_batch")
    torch.cuda.synchronize()
    assert x.guards_ok() and y.guards_ok() and ws.guards_ok()
    return x.body(np.float32).reshape(n, 3, S, S), y.body(np.float32).reshape(n, 1, S, S), ws.body()


@pytest.mark.parametrize("S", [16, 136])
def test_augment_c_abi_guards_and_workspace(S):
    """x, y and the workspace inside 0xA5-filled allocations: no byte outside them changes; the workspace is untouched when no sample
    draws CLAHE, and only the CLAHE samples' own slots are written when some do; the result does not depend on what it held."""
    items, ds = _dataset(S)
    at, draws = PC.by_name(PC.all_draws(S)), PC.all_draws(S)
    idx = [0, 7, 6, 9, 0]
    no = [draws[at[n]] for n in ("p-d44-r1-blur5-n1", "plain", "rbc(1.2,-0.2)", "p-d42-r0-blur3-n0", "rot-m(-137.5)")]
    x, y, ws = _augment_abi(ds, S, idx, no, PC.FILL)
    assert (ws == PC.FILL).all()
    xa, ya, _ = ds.batch(idx, draws=no)
    assert np.array_equal(x, xa.cpu().numpy()) and np.array_equal(y, ya.cpu().numpy())
    some = [no[0], draws[at["clahe-1.37-d4_1-rot"]], no[2], draws[at["clahe-40"]], no[4]]
    x1, y1, ws1 = _augment_abi(ds, S, idx, some, PC.FILL)
    x0, y0, ws0 = _augment_abi(ds, S, idx, some, 0)
    assert x1.tobytes() == x0.tobytes() and y1.tobytes() == y0.tobytes()
    per = S * S * 4 + 64 * 256
    for j in range(5):
        slot1, slot0 = ws1[j * per:(j + 1) * per], ws0[j * per:(j + 1) * per]
        if j in (1, 3):
            assert np.array_equal(slot1, slot0)                             # every byte of a CLAHE sample's slot is written
        else:
            assert (slot1 == PC.FILL).all() and (slot0 == 0).all()
    for j, d in enumerate(some):
        xo, yo = PC.augment_ref(items[idx[j]][1], items[idx[j]][2], d)
        assert np.array_equal(x1[j], xo) and np.array_equal(y1[j], yo), j


# ======================================================================================================= B. dataset letterbox
@pytest.mark.parametrize("S", PC.LB_SIZES)
def test_dataset_letterbox(S):
    src = PC.lb_sources(S)
    imgs, masks = [PC.bgr_image(h, w) for h, w in src], [PC.raw_mask(h, w) for h, w in src]
    ds = vk.DeviceDataset(imgs, masks, img_size=S, device=DEV)
    for i, (h, w) in enumerate(src):
        sq, m = PC.letterbox_ref(imgs[i], masks[i], S)
        assert np.array_equal(ds.images[i].cpu().numpy(), sq), (S, h, w)
        got = ds.masks[i].cpu().numpy()
        assert np.array_equal(got, m) and set(np.unique(got).tolist()) <= {0, 1}, (S, h, w)
        nh, nw, top, left = P.geometry_train(h, w, S)[1:]
        assert tuple(ds.content[i]) == (top, left, nh, nw)


@pytest.mark.parametrize("h,w,S", PC.LB_REFUSED)
def test_dataset_letterbox_refuses_an_empty_resize(h, w, S):
    """geometry_train gives nh = 0: refused on the host before any launch, for the dataset and for both C entry points."""
    with pytest.raises(vk.VkError, match="non-positive"):
        vk.DeviceDataset([PC.bgr_image(h, w)], [PC.raw_mask(h, w)], img_size=S, device=DEV)
    nh, nw, top, left = P.geometry_train(h, w, S)[1:]
    out = Guarded(S * S * 3)
    src = _dev(PC.bgr_image(h, w))
    for fn, stride in ((L.lib().vk_letterbox_u8, 3 * w), (L.lib().vk_letterbox_mask_u8, w)):
        d = L.vk_letterbox_desc(h, w, stride, S, nh, nw, top, left, 0)
        assert fn(C.byref(d), src.data_ptr(), out.ptr, L.current_stream()) != 0
    torch.cuda.synchronize()
    assert (out.body() == PC.FILL).all() and out.guards_ok()


@pytest.mark.parametrize("S", PC.LB_SIZES)
def test_letterbox_u8_c_abi(S):
    """Explicit descriptors (odd top / left, the copy path away from the train geometry), pad_value 0 / 114 / 255, rows 5 bytes apart
    with 0xA5 between them, outputs between guard bytes."""
    lib, st = L.lib(), L.current_stream()
    for h, w in PC.lb_sources(S):
        img, m = PC.bgr_image(h, w), PC.raw_mask(h, w)
        flat_i, stride_i = PC.strided(img)
        flat_m, stride_m = PC.strided(m)
        d_img, d_msk, d_img_s, d_msk_s = _dev(img), _dev(m), _dev(flat_i), _dev(flat_m)
        geos = [tuple(P.geometry_train(h, w, S)[1:])] + PC.odd_geometries(h, w, S)
        for (nh, nw, top, left) in geos:
            for pad in (0, 114, 255):
                sq, mm = PC.letterbox_ref(img, m, S, (nh, nw, top, left), pad)
                for src_i, si, src_m, sm in ((d_img, 3 * w, d_msk, w), (d_img_s, stride_i, d_msk_s, stride_m)):
                    oi, om = Guarded(S * S * 3), Guarded(S * S)
                    d = L.vk_letterbox_desc(h, w, si, S, nh, nw, top, left, pad)
                    L.check(lib.vk_letterbox_u8(C.byref(d), src_i.data_ptr(), oi.ptr, st), "vk_letterbox_u8")
                    d = L.vk_letterbox_desc(h, w, sm, S, nh, nw, top, left, pad)
                    L.check(lib.vk_letterbox_mask_u8(C.byref(d), src_m.data_ptr(), om.ptr, st), "vk_letterbox_mask_u8")
                    torch.cuda.synchronize()
                    assert np.array_equal(oi.body().reshape(S, S, 3), sq), (S, h, w, nh, nw, top, left, pad, si)
                    assert np.array_equal(om.body().reshape(S, S), mm), (S, h, w, nh, nw, top, left, pad, sm)
                    assert oi.guards_ok() and om.guards_ok()


# ======================================================================================================= C. pre / post-processing
@pytest.mark.parametrize("conv", PC.CONVENTIONS)
@pytest.mark.parametrize("size", PC.PRE_SIZES)
def test_preprocess(size, conv):
    """The letterbox shapes at 8 and 67 under the three conventions, through the wrapper and through the C ABI with padded rows and a
    guarded output; a geometry with an empty side is refused."""
    lib, st = L.lib(), L.current_stream()
    for h, w in PC.pre_sources():
        img = PC.bgr_image(h, w)
        if PC.post_geometry(h, w, size, conv) is None:
            with pytest.raises(vk.VkError, match="non-positive"):
                vk.prepost.preprocess(img, size, conv, DEV)
            continue
        want, geo = P.preprocess(img, size, conv)
        x, meta = vk.prepost.preprocess(img, size, conv, DEV)
        assert meta[1][1:] == geo and meta[2] == (h, w)
        assert np.array_equal(x[0].cpu().numpy(), want), (h, w)
        flat, stride = PC.strided(img)
        out = Guarded(3 * size * size * 4)
        d = L.vk_letterbox_desc(h, w, stride, size, *geo, 0)
        L.check(lib.vk_letterbox_preprocess(C.byref(d), _dev(flat).data_ptr(), out.ptr, st), "vk_letterbox_preprocess")
        torch.cuda.synchronize()
        assert np.array_equal(out.body(np.float32).reshape(3, size, size), want) and out.guards_ok(), (h, w)


POST_PARAMS = [(S, i, conv) for S in PC.POST_SHAPES for i in range(len(PC.POST_SHAPES[S])) for conv in PC.CONVENTIONS]


def _post_abi(which, desc, lg, thr, nbytes, shift):
    lib, out = L.lib(), Guarded(nbytes, shift=shift)
    if which == "mask":
        L.check(lib.vk_letterbox_postprocess_mask(C.byref(desc), lg.data_ptr(), float(thr), out.ptr, L.current_stream()), "mask")
    else:
        L.check(lib.vk_letterbox_postprocess_prob(C.byref(desc), lg.data_ptr(), out.ptr, L.current_stream()), "prob")
    torch.cuda.synchronize()
    assert out.guards_ok()
    return out.body(np.uint8 if which == "mask" else np.float32)


@pytest.mark.parametrize("S,i,conv", POST_PARAMS, ids=[f"{S}-{PC.POST_SHAPES[S][i][0]}x{PC.POST_SHAPES[S][i][1]}-{c}" for S, i, c in POST_PARAMS])
def test_postprocess(S, i, conv, monkeypatch):
    """Built logits (every multiple of 1/8 in [-20, 20], 0, +-88, +-100, +-inf, NaN) through the per-pixel and the windowed kernel, into
    outputs that are 16-byte aligned and outputs shifted by one element (the scalar store path with w % 4 == 0): masks EQUAL the
    oracle at thresholds 0, 0.45, 0.5 and 1 with no exempted pixel (the CPU file proves no logit used is within 2 ulp of expf of a
    threshold); probabilities within 2e-6, NaN where the oracle has NaN, and the two kernels agree bit for bit."""
    h, w = PC.POST_SHAPES[S][i]
    lg = PC.logit_map(S, i)
    geo = P.GEOMETRY[conv](h, w, S)
    nh, nw, top, left = geo[1:]
    desc = L.vk_letterbox_desc(h, w, 0, S, nh, nw, top, left, 0)
    t = _dev(lg)
    with np.errstate(all="ignore"):
        want_m = {thr: P.postprocess_mask(lg, nh, nw, top, left, (h, w), thr) for thr in PC.POST_THRESHOLDS}
        want_p = P.postprocess_prob(lg, nh, nw, top, left, (h, w))
    probs = {}
    for window in ("0", "1"):
        monkeypatch.setenv("VK_PP_WINDOW", window)
        for shift in (0, 1):
            for thr in PC.POST_THRESHOLDS:
                m = _post_abi("mask", desc, t, thr, h * w, shift).reshape(h, w)
                assert np.array_equal(m, want_m[thr]), (window, shift, thr, int((m != want_m[thr]).sum()))
        for shift in (0, 4):
            pr = _post_abi("prob", desc, t, 0.0, h * w * 4, shift).reshape(h, w)
            assert np.array_equal(np.isnan(pr), np.isnan(want_p)), (window, shift)
            ok = ~np.isnan(want_p)
            assert ok.any() and float(np.abs(pr[ok] - want_p[ok]).max()) <= 2e-6, (window, shift)
            assert pr[ok].min() >= 0.0 and pr[ok].max() <= 1.0
            probs[(window, shift)] = pr
    first = probs[("0", 0)]
    for k, pr in probs.items():
        assert np.array_equal(pr, first, equal_nan=True), k                 # per-pixel and windowed, aligned and shifted: the same bits
    wm = vk.prepost.postprocess_mask(t, (geo[0], geo, (h, w)), 0.5).cpu().numpy()     # the wrapper, whichever kernel it picks itself
    assert np.array_equal(wm, want_m[0.5])


# ======================================================================================================= D. metrics
def _metrics(pred, tgt, **kw):
    n = pred.shape[0]
    out = vk.seg_metrics_device(pred.view(n, 1, 1, -1), tgt.view(n, 1, 1, -1), **kw).cpu().numpy()
    return out[2::2], out[3::2], out[0], out[1], out


def _check_metrics(pred, tgt, hit, tgt_np, what, **kw):
    dice, iou, md, mu = PC.met_ref(*PC.met_counts(hit, tgt_np))
    gd, gu, gmd, gmu, out = _metrics(pred, tgt, **kw)
    assert np.array_equal(gd, dice) and np.array_equal(gu, iou), what
    assert gmd == md and gmu == mu, (what, float(gmd), float(md), float(gmu), float(mu))
    assert np.array_equal(_metrics(pred, tgt, **kw)[4], out), what                     # a second call: the same bytes


@pytest.mark.parametrize("n,per", PC.MET_SHAPES)
def test_metrics_equal_integer_counts(n, per):
    """Probabilities on the lattice k/16 with values ON every threshold (misses under the strict >), logits with exact zeros (misses
    at 0.5), one empty target, one empty prediction, one full image; per-image values and batch means EQUAL the reference built from
    int64 counts (the finalize sums in a fixed order, and the float64 mean of at most 4096 float32 values rounds to the same float32
    whatever the order: the orders differ by about 1e-16 relative, a float32 rounding boundary is 6e-8 wide)."""
    prob, tgt = PC.met_inputs(n, per)
    dp, dt = _dev(prob), _dev(tgt)
    for thr in PC.MET_THRESHOLDS:
        _check_metrics(dp, dt, prob > np.float32(thr), tgt, ("prob", thr), threshold=thr)
    lg = PC.met_logits(n, per)
    dl = _dev(lg)
    vals = (np.arange(17) - 8) / 2.0
    for thr in PC.MET_THRESHOLDS:
        table = (1.0 / (1.0 + np.exp(-vals)) > thr)          # the CPU file: no value within 1e-2 of a threshold but 0 at 0.5, whose
        assert bool(table[8]) == (thr < 0.5)                  # sigmoid is exactly 0.5 in float32 and in float64: a miss under the strict >
        hit = table[(lg * 2).astype(np.int64) + 8]
        _check_metrics(dl, dt, hit, tgt, ("logits", thr), threshold=thr, from_logits=True)


@pytest.mark.parametrize("which", ["both", "pred", "target"])
def test_metrics_from_an_unaligned_base(which):
    """(2, 4096) from a base one float past a 16-byte boundary: a per_image divisible by 4 with vec_ok = 0, so the scalar loop covers
    the whole image and there is no tail."""
    n, per = 2, 4096
    prob, tgt = PC.met_inputs(n, per)

    def place(a, off):
        big = torch.zeros(n * per + 8, dtype=torch.float32, device=DEV)
        v = big.flatten()[off:off + n * per].view(n, 1, 64, 64)
        v.copy_(torch.from_numpy(a).view(n, 1, 64, 64))
        assert v.data_ptr() % 16 == (4 * off) % 16 and v.is_contiguous()
        return v

    dp, dt = place(prob, 1 if which in ("both", "pred") else 0), place(tgt, 1 if which in ("both", "target") else 0)
    for thr in PC.MET_THRESHOLDS:
        _check_metrics(dp, dt, prob > np.float32(thr), tgt, (which, thr), threshold=thr)
    aligned = _metrics(_dev(prob), _dev(tgt), threshold=0.5)[4]
    assert np.array_equal(_metrics(dp, dt, threshold=0.5)[4], aligned)


def test_metrics_soft_targets():
    """Targets k/8 on (3, 257), reference in float64.  The bar is the kernel's own accumulation, not a fit: 257 elements over 256 threads
    is at most k = 2 elements per thread, so each float32 partial of I = sum hit * t and T = sum t carries at most k roundings
    (relative k * 2^-24; P counts hits and is exact), the float64 reduction adds nothing at this size, and (float) of each sum is one
    more.  Dice = (2 I + eps) / ((P + T) + eps) then rounds four times (2 I is exact), so its relative error is at most
    (2 (k + 1) + 4) 2^-24 = 10 * 2^-24.  IoU = (I + eps) / (((P + T) - I) + eps): I <= min(P, T) gives (P + T) - I >= (P + T) / 2, so
    errors in P + T reach the denominator at most doubled and those in I at most once: (k + 1) + [2 (k + 2) + (k + 1) + 2] + 2 =
    (4 k + 10) 2^-24 = 18 * 2^-24."""
    n, per, k = 3, 257, 2
    prob, _ = PC.met_inputs(n, per)
    tgt = PC.met_soft_targets(n, per)
    for thr in PC.MET_THRESHOLDS:
        hit = (prob > np.float32(thr)).astype(np.float64)
        t64 = tgt.astype(np.float64)
        I, Pn, T = (hit * t64).sum(1), hit.sum(1), t64.sum(1)
        dice, iou = (2 * I + PC.EPS) / (Pn + T + PC.EPS), (I + PC.EPS) / (Pn + T - I + PC.EPS)
        gd, gu, gmd, gmu, _ = _metrics(_dev(prob), _dev(tgt), threshold=thr)
        u = 2.0 ** -24
        assert (np.abs(gd - dice) <= (2 * (k + 1) + 4) * u * np.abs(dice)).all(), (thr, gd, dice)
        assert (np.abs(gu - iou) <= (4 * k + 10) * u * np.abs(iou)).all(), (thr, gu, iou)
        assert abs(gmd - dice.mean()) <= 11 * u * dice.mean() and abs(gmu - iou.mean()) <= 19 * u * iou.mean()      # + the mean's one rounding
