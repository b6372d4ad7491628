"""vk.patches on the MI355X: the foreground index, the origins and the crop of vk_patch_batch and PatchDataset.batch against the numpy
restatements of patches_ref.py.  Byte / index work and float32 arithmetic in a fixed order: every comparison is EXACT
(np.array_equal).  Outputs of the C ABI go into sentinel-filled buffers with a guard zone; every output byte must be overwritten."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import patches_cases as PC
import patches_ref as R
from oracle import augment_oracle as A

pytestmark = pytest.mark.gpu
vk = importlib.import_module("vickers-hardness-unet_amd")
DEV = torch.device("cuda:0")
GUARD = 64
SENTINEL = 7          # no value of a {0,1} mask; the RGB check below is on the guard zone and on equality with the reference
I_SENTINEL = -(2 ** 31)


@pytest.fixture(scope="module")
def raws():
    return PC.items()


def _dataset(raws, S):
    return vk.PatchDataset(raws[0], raws[1], patch_size=S, device=DEV, names=["i%d" % i for i in range(len(raws[0]))])


@pytest.fixture(scope="module")
def datasets(raws):
    return {S: _dataset(raws, S) for S in sorted(set(PC.ORIGIN_SIZES) | set(PC.CROP_SIZES))}


def _patch_guarded(ds, draws, force_general=False):
    """vk_patch_batch through the C ABI into sentinel-filled buffers with a guard zone; numpy (rgb, mask, origins)."""
    n, S = len(draws), ds.S
    rgb = torch.full((n * S * S * 3 + GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
    msk = torch.full((n * S * S + GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
    org = torch.full((2 * n + GUARD,), I_SENTINEL, dtype=torch.int32, device=DEV)
    pdev = torch.empty(n * 32, dtype=torch.uint8, device=DEV)
    vk._lib.check(vk.lib().vk_patch_batch(n, S, len(ds), ds._items_dev.data_ptr(), ds.images.data_ptr(), ds.masks.data_ptr(),
                                          ds.rowcum.data_ptr(), vk.patches._patch_array(draws), pdev.data_ptr(),
                                          vk._lib.VK_PATCH_FORCE_GENERAL if force_general else 0, org.data_ptr(), rgb.data_ptr(),
                                          msk.data_ptr(), vk._lib.current_stream()), "vk_patch_batch")
    torch.cuda.synchronize()
    assert (rgb[n * S * S * 3:] == SENTINEL).all() and (msk[n * S * S:] == SENTINEL).all() and (org[2 * n:] == I_SENTINEL).all(), \
        "write beyond the outputs"
    m, o = msk[:n * S * S].view(n, S, S).cpu().numpy(), org[:2 * n].view(n, 2).cpu().numpy()
    assert np.isin(m, (0, 1)).all() and (o != I_SENTINEL).all(), "output not fully overwritten"
    return rgb[:n * S * S * 3].view(n, S, S, 3).cpu().numpy(), m, o


def _check_against_ref(raws, ds, draws, got, label):
    rgb, m, org = got
    for j, d in enumerate(draws):
        want_rgb, want_m, want_o = R.patch_ref(raws[0][d["item"]], raws[1][d["item"]], d, ds.S)
        assert tuple(org[j]) == want_o, (label, j, d)
        assert np.array_equal(m[j], want_m), (label, j, d)
        assert np.array_equal(rgb[j], want_rgb), (label, j, d)


def test_index_and_store(raws, datasets):
    ds = datasets[64]
    assert len(ds) == 6 and ds.images.dtype == torch.uint8 and ds.rowcum.dtype == torch.int32
    for i, (img, m) in enumerate(zip(*raws)):
        assert ds.items[i].img_off % 4 == 0 and ds.items[i].msk_off % 4 == 0
        want = R.rowcum_ref(m)
        assert np.array_equal(ds.rowcum_of(i).cpu().numpy(), want), i
        assert ds.fg_counts[i] == int(want[-1]) == int((m > 0).sum())
        assert np.array_equal(ds.image(i).cpu().numpy(), img) and ds.image(i).data_ptr() == ds.images.data_ptr() + ds.items[i].img_off
        assert np.array_equal(ds.mask(i).cpu().numpy(), (m > 0).astype(np.float32)[None, None])
    assert ds.fg_counts[0] == 0 and ds.fg_counts[1] == 1 and ds.fg_counts[3] == 1 and ds.fg_counts[4] == 1


def test_index_of_a_tall_item_and_unaligned_rows():
    """More than 256 rows per scan thread's share (h = 1000: four rows per thread) and a width that leaves every row at another byte
    alignment (w = 67), foreground dense enough that a miscounted head or tail byte shows."""
    rng = np.random.default_rng(1)
    masks = [(rng.random((1000, 67)) < 0.5).astype(np.uint8) * 255, (rng.random((3, 1030)) < 0.5).astype(np.uint8)]
    ds = vk.PatchDataset([np.zeros(m.shape + (3,), np.uint8) for m in masks], masks, patch_size=8, device=DEV)
    for i, m in enumerate(masks):
        assert np.array_equal(ds.rowcum_of(i).cpu().numpy(), R.rowcum_ref(m)), i


@pytest.mark.parametrize("S", PC.ORIGIN_SIZES)
def test_origins(raws, datasets, S):
    ds, draws = datasets[S], PC.origin_draws(raws[1], S)
    _, _, org = _patch_guarded(ds, draws)
    for j, d in enumerate(draws):
        y0, x0, _ = R.origin_ref(raws[1][d["item"]], d["k"], d["oy"], d["ox"], S)
        assert tuple(org[j]) == (y0, x0), (j, d)


@pytest.mark.parametrize("S", PC.CROP_SIZES)
def test_crop(raws, datasets, S):
    ds, draws = datasets[S], PC.crop_draws(raws[1], S)
    got = _patch_guarded(ds, draws)
    _check_against_ref(raws, ds, draws, got, "crop")
    # the forced general path gives the bits of the copy path at identity (and changes nothing elsewhere)
    forced = _patch_guarded(ds, draws, force_general=True)
    for a, b in zip(got, forced):
        assert np.array_equal(a, b)
    # the Python entry point returns the same, and keeps the origins
    rgb, m, org = ds.crop(draws)
    assert np.array_equal(rgb.cpu().numpy(), got[0]) and np.array_equal(m.cpu().numpy(), got[1])
    assert ds.last_origins is org and np.array_equal(org.cpu().numpy(), got[2])


def test_batch_combined_draws(raws, datasets):
    S = 96
    ds, draws = datasets[S], PC.batch_draws(S)
    idx = [p["item"] for p, _ in draws]
    x, y, names = ds.batch(idx, draws=draws)
    assert x.shape == (len(idx), 3, S, S) and y.shape == (len(idx), 1, S, S) and names == ["i%d" % i for i in idx]
    x2, y2, _ = ds.batch(idx, draws=draws)
    assert torch.equal(x, x2) and torch.equal(y, y2)
    xs, ys = x.cpu().numpy(), y.cpu().numpy()
    for j, (p, a) in enumerate(draws):
        xo, yo = R.batch_ref(raws[0][p["item"]], raws[1][p["item"]], p, a, S)
        assert np.array_equal(ys[j], yo), j
        assert np.array_equal(xs[j], xo), (j, np.abs(xs[j] - xo).max())


def test_batch_without_sampler_is_the_centred_slice_normalised(raws, datasets):
    S = 64
    ds = datasets[S]
    idx = [2, 0, 5, 4, 1]
    x, y, _ = ds.batch(idx)
    org = ds.last_origins.cpu().numpy()
    for j, i in enumerate(idx):
        h, w = PC.SHAPES[i]
        y0 = (h - S) // 2 if h >= S else -((S - h) // 2)
        x0 = (w - S) // 2 if w >= S else -((S - w) // 2)
        assert tuple(org[j]) == (y0, x0)
        bgr, m = R.slice_ref(raws[0][i], raws[1][i], y0, x0, S)
        assert np.array_equal(x[j].cpu().numpy(), A.normalize_chw(np.ascontiguousarray(bgr[..., ::-1])))
        assert np.array_equal(y[j, 0].cpu().numpy(), m.astype(np.float32))


def test_realistic_shape_with_sampled_draws():
    """4 patches of 512 x 512 from a 1300 x 1948 image, draws from PatchSampler(seed=0); and the loader protocol."""
    h, w, S = 1300, 1948, 512
    img = PC.image(h, w, 42)
    yy, xx = np.mgrid[0:h, 0:w]
    mask = ((np.abs(xx - 1500) + np.abs(yy - 400)) < 130).astype(np.uint8) * 255
    ds = vk.PatchDataset([img], [mask], patch_size=S, device=DEV)
    assert ds.fg_counts == [int((mask > 0).sum())]
    sm = vk.PatchSampler(seed=0)
    draws = [sm.sample(0, h, w, ds.fg_counts[0], S) for _ in range(4)]
    x, y, _ = ds.batch([0] * 4, draws=draws)
    for j, (p, a) in enumerate(draws):
        xo, yo = R.batch_ref(img, mask, p, a, S)
        assert np.array_equal(y[j].cpu().numpy(), yo) and np.array_equal(x[j].cpu().numpy(), xo), (j, p, a)
    batches = list(ds.loader(batch_size=2, patches_per_image=3, sampler=sm, seed=1))
    assert [b[0].shape[0] for b in batches] == [2, 1] and batches[0][0].shape == (2, 3, S, S) and batches[0][2] == ["0", "0"]


def test_offsets_beyond_2_31():
    """A hand-built item table whose one small image and mask sit behind byte 2^31 of an uninitialised 2.2 GB store."""
    h, w, S = 45, 83, 32
    img, m = PC.image(h, w, 9), (np.random.default_rng(9).random((h, w)) < 0.2).astype(np.uint8)
    total = 2_200_000_000
    store = torch.empty(total, dtype=torch.uint8, device=DEV)
    io, mo = 2 ** 31 + 4096, 2 ** 31 + 1_000_000
    store[io:io + h * w * 3].copy_(torch.from_numpy(img).view(-1))
    store[mo:mo + h * w].copy_(torch.from_numpy(m).view(-1))
    L = vk._lib
    items = (L.vk_patch_item * 1)(L.vk_patch_item(io, mo, h, w, 0))
    items_dev = torch.empty(32, dtype=torch.uint8, device=DEV)
    rowcum = torch.full((h + GUARD,), I_SENTINEL, dtype=torch.int32, device=DEV)
    L.check(L.lib().vk_patch_index(1, items, items_dev.data_ptr(), total, store.data_ptr(), total, rowcum.data_ptr(), h, L.current_stream()))
    draws = [PC.patch(0, 17, 5, 9), PC.patch(0, -1, 13, 51), PC.patch(0, 100, 31, 0, 1.25, 30.0), PC.patch(0, -1, 0, 0, 2.0, -137.5)]
    n = len(draws)
    rgb = torch.full((n * S * S * 3 + GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
    msk = torch.full((n * S * S + GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
    org = torch.full((2 * n + GUARD,), I_SENTINEL, dtype=torch.int32, device=DEV)
    pdev = torch.empty(n * 32, dtype=torch.uint8, device=DEV)
    L.check(L.lib().vk_patch_batch(n, S, 1, items_dev.data_ptr(), store.data_ptr(), store.data_ptr(), rowcum.data_ptr(),
                                   vk.patches._patch_array(draws), pdev.data_ptr(), 0, org.data_ptr(), rgb.data_ptr(), msk.data_ptr(),
                                   L.current_stream()))
    torch.cuda.synchronize()
    assert np.array_equal(rowcum[:h].cpu().numpy(), R.rowcum_ref(m)) and (rowcum[h:] == I_SENTINEL).all()
    assert (rgb[n * S * S * 3:] == SENTINEL).all() and (msk[n * S * S:] == SENTINEL).all() and (org[2 * n:] == I_SENTINEL).all()
    for j, d in enumerate(draws):
        want_rgb, want_m, want_o = R.patch_ref(img, m, d, S)
        assert tuple(org[2 * j:2 * j + 2].tolist()) == want_o
        assert np.array_equal(msk[j * S * S:(j + 1) * S * S].view(S, S).cpu().numpy(), want_m), j
        assert np.array_equal(rgb[j * S * S * 3:(j + 1) * S * S * 3].view(S, S, 3).cpu().numpy(), want_rgb), j


def test_patches_train_and_native_validation(raws, datasets):
    """The use: patches into one training step; an item's image through tiled inference, its mask into the metrics."""
    S = 64
    ds = datasets[S]
    torch.manual_seed(42)
    model = vk.Unet(encoder_name="resnet34", encoder_weights=None, in_channels=3, classes=1, activation=None).to(DEV)
    opt = vk.adamw_for(model, lr=5e-5, weight_decay=1e-4)
    x, y, _ = ds.batch([2, 5, 1, 3], sampler=vk.PatchSampler(seed=0))
    assert set(torch.unique(y).tolist()) <= {0.0, 1.0} and torch.isfinite(x).all()
    model.train()
    opt.zero_grad(set_to_none=True)
    loss = model.loss_and_backward(x, y)
    opt.step()
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all() and torch.isfinite(model.flat_params).all()
    model.eval()
    prob = vk.Segmenter(model, img_size=S, device=DEV).infer_tiled(ds.image(2), overlap=16, tta="none", batch=16)
    assert prob.shape == PC.SHAPES[2] and np.isfinite(prob).all()
    dice, iou = vk.seg_metrics(torch.from_numpy(prob).to(DEV)[None, None], ds.mask(2))
    assert np.isfinite(dice) and np.isfinite(iou) and 0.0 <= iou <= dice <= 1.0


def test_argument_errors(raws, datasets):
    ds = datasets[64]
    with pytest.raises(ValueError):
        ds.batch([6])
    with pytest.raises(ValueError):
        ds.batch([0, 1], draws=[(PC.patch(0), PC.AUG_IDENTITY)])
    with pytest.raises(ValueError):
        ds.crop([])
    with pytest.raises(ValueError):
        ds.crop([PC.patch(9)])
    with pytest.raises(vk.VkError, match="zoom"):
        ds.crop([PC.patch(0, zoom=5.0)])
    with pytest.raises(vk.VkError, match="rotation"):
        ds.crop([dict(PC.patch(0), cos_a=0.5, sin_a=0.5)])
    with pytest.raises(vk.VkError, match="photo"):
        ds.batch([0], draws=[(PC.patch(0), dict(PC.AUG_IDENTITY, photo=4))])
    with pytest.raises(ValueError):
        vk.PatchDataset(raws[0][:1], raws[1][:1], patch_size=0, device=DEV)
    with pytest.raises(ValueError):
        vk.PatchDataset([np.zeros((4, 4), np.uint8)], [np.zeros((4, 4), np.uint8)], device=DEV)
    with pytest.raises(ValueError):
        list(ds.loader(batch_size=0))
