"""Host side of vk.patches (no GPU): the conditions the numpy restatement of patches_ref.py rests on (it is the oracle's rotation when
the window is the image, and the zero-padded slice at identity), the origin rule, PatchSampler, and the argument checks of
vk_patch_index / vk_patch_batch through the loaded library."""
import ctypes as C
import math

import numpy as np
import pytest

import patches_cases as PC
import patches_ref as R
from oracle import augment_oracle as A


# ------------------------------------------------------------------------------------------------ the reference's own conditions
@pytest.mark.parametrize("S", [37, 64, 96])
def test_crop_ref_of_the_whole_image_is_the_oracle_rotation(S):
    img = PC.image(S, S, S)
    mask = (np.random.default_rng(S).random((S, S)) < 0.3).astype(np.uint8)
    for ang in PC.ANGLES:
        a = math.radians(ang)
        want_img, want_m = A.rotate(img, mask, math.cos(a), math.sin(a))
        got_img, got_m = R.crop_ref(img, mask, 0, 0, S, 1.0, math.cos(a), math.sin(a))
        assert np.array_equal(got_img, want_img) and np.array_equal(got_m, want_m), ang


IDENTITY_CASES = [
    # h, w, S, y0, x0
    (37, 53, 16, 5, 9), (37, 53, 64, -13, -5), (64, 200, 96, -16, 104), (1, 1, 8, -3, -3), (5, 259, 64, -29, 195),
    (2048, 3072, 512, 1536, 2560), (33, 16384, 64, -15, 16320),
]


@pytest.mark.parametrize("h,w,S,y0,x0", IDENTITY_CASES)
def test_crop_ref_at_identity_is_the_zero_padded_slice(h, w, S, y0, x0):
    rng = np.random.default_rng(h + w)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    mask = (rng.random((h, w)) < 0.3).astype(np.uint8) * 200
    got_img, got_m = R.crop_ref(img, mask, y0, x0, S)
    want_img, want_m = R.slice_ref(img, mask, y0, x0, S)
    assert np.array_equal(got_img, want_img) and np.array_equal(got_m, want_m)
    assert set(np.unique(got_m)) <= {0, 1}


def test_rowcum_ref_counts_rows():
    _, masks = PC.items()
    for m in masks:
        rc = R.rowcum_ref(m)
        assert rc.dtype == np.int32 and rc.shape == (m.shape[0],) and rc[-1] == (m > 0).sum()
        assert (np.diff(np.concatenate([[0], rc])) == (m > 0).sum(axis=1)).all()
    assert R.rowcum_ref(masks[0])[-1] == 0 and R.rowcum_ref(masks[1])[-2] == 0 and R.rowcum_ref(masks[1])[-1] == 1


@pytest.mark.parametrize("S", [8, 31, 64])
def test_origin_ref_keeps_window_and_pixel_inside(S):
    rng = np.random.default_rng(S)
    for h, w in ((S, S), (S + 1, 3 * S), (100, 70), (307, 205)):
        if h < S or w < S:
            continue
        m = (rng.random((h, w)) < 0.05).astype(np.uint8)
        m[h - 1, w - 1] = m[0, 0] = 1
        count = int(m.sum())
        for k in (0, 1, count // 2, count - 1, count + 5):
            for oy, ox in ((0, 0), (S - 1, S - 1), (0, S - 1), (S // 2, S // 3)):
                y0, x0, (py, px) = R.origin_ref(m, k, oy, ox, S)
                assert 0 <= y0 <= h - S and 0 <= x0 <= w - S
                assert y0 <= py < y0 + S and x0 <= px < x0 + S and m[py, px]
        y0, x0, pick = R.origin_ref(m, -1, h, w, S)          # an origin past the image is pulled back
        assert (y0, x0, pick) == (h - S, w - S, None)


def test_origin_ref_centres_a_small_image():
    m = np.ones((5, 259), np.uint8)
    for k, oy, ox in ((-1, 0, 0), (3, 63, 0), (700, 0, 63)):
        y0, x0, _ = R.origin_ref(m, k, oy, ox, 64)
        assert y0 == -((64 - 5) // 2) == -29 and 0 <= x0 <= 259 - 64
    assert R.origin_ref(np.zeros((1, 1), np.uint8), 0, 9, 9, 8)[:2] == (-3, -3)
    assert R.origin_ref(np.ones((7, 3), np.uint8), 2, 1, 1, 4)[:2] == (0, 0)      # (0, 2) - (1, 1), clamped; x centred: -((4 - 3) // 2) = 0


# ------------------------------------------------------------------------------------------------ PatchSampler
def test_patch_sampler_is_deterministic_and_in_range(vk):
    S = 64
    a, b = vk.PatchSampler(seed=3), vk.PatchSampler(seed=3)
    args = [(0, 37, 53, 0), (1, 307, 205, 2345), (2, 2048, 3072, 100000), (3, 5, 259, 50)]
    seen_fg = seen_bg = 0
    for t in range(400):
        item, h, w, cnt = args[t % 4]
        pa, aa = a.sample(item, h, w, cnt, S)
        pb, ab = b.sample(item, h, w, cnt, S)
        assert pa == pb and aa == ab
        assert pa["item"] == item and 0.8 <= pa["zoom"] <= 1.25
        assert abs(pa["cos_a"] ** 2 + pa["sin_a"] ** 2 - 1.0) < 1e-9
        if pa["k"] >= 0:
            seen_fg += 1
            assert cnt > 0 and pa["k"] < cnt and 0 <= pa["oy"] < S and 0 <= pa["ox"] < S
        else:
            seen_bg += 1
            assert pa["k"] == -1 and 0 <= pa["oy"] <= max(h - S, 0) and 0 <= pa["ox"] <= max(w - S, 0)
    assert seen_fg > 100 and seen_bg > 100
    assert vk.PatchSampler(seed=4).sample(1, 307, 205, 2345, S) != vk.PatchSampler(seed=3).sample(1, 307, 205, 2345, S)
    assert all(vk.PatchSampler(seed=5, p_fg=0.0).sample(1, 307, 205, 2345, S)[0]["k"] == -1 for _ in range(5))
    for bad in (dict(p_fg=1.5), dict(zoom=(0.1, 1.0)), dict(zoom=(1.5, 1.0)), dict(zoom=(1.0, 5.0))):
        with pytest.raises(ValueError):
            vk.PatchSampler(seed=0, **bad)


def test_patch_sampler_moves_the_rotation_out_of_the_aug_draw(vk):
    ps, plain = vk.PatchSampler(seed=11), vk.AugmentSampler(seed=11)
    rotated = 0
    for _ in range(300):
        p, a = ps.sample(0, 307, 205, 77, 64)
        want = plain.sample()
        assert (a["rotate"], a["cos_a"], a["sin_a"]) == (0, 1.0, 0.0)           # never in both
        if want["rotate"]:
            rotated += 1
            assert (p["cos_a"], p["sin_a"]) == (want["cos_a"], want["sin_a"])
        else:
            assert (p["cos_a"], p["sin_a"]) == (1.0, 0.0)
        assert {k: v for k, v in a.items() if k not in ("rotate", "cos_a", "sin_a")} == \
               {k: v for k, v in want.items() if k not in ("rotate", "cos_a", "sin_a")}
    assert 120 < rotated < 240                                                   # Rotate(p=0.6) keeps its own probability


# ------------------------------------------------------------------------------------------------ the library
def test_library_exports_the_patch_symbols(vk):
    L = vk.lib()
    assert hasattr(L, "vk_patch_index") and hasattr(L, "vk_patch_batch")
    assert C.sizeof(vk._lib.vk_patch_item) == 32 and C.sizeof(vk._lib.vk_patch_params) == 32
    assert vk.patches.PatchDataset is vk.PatchDataset and vk.patches.PatchSampler is vk.PatchSampler


def _index_rc(vk, items, images_bytes=1 << 20, masks_bytes=1 << 20, rows=1 << 12, masks=True):
    """vk_patch_index on host buffers: a failed check returns before anything is read, written or put on a stream."""
    L = vk.lib()
    arr = (vk._lib.vk_patch_item * len(items))(*[vk._lib.vk_patch_item(*it) for it in items])
    dev, msk, rows_buf = np.full(64 * len(items) + 64, 7, np.uint8), np.full(64, 9, np.uint8), np.full(64, 5, np.int32)
    rc = L.vk_patch_index(len(items), arr, dev.ctypes.data, images_bytes, msk.ctypes.data if masks else None, masks_bytes, rows_buf.ctypes.data,
                          rows, None)
    assert (dev == 7).all() and (msk == 9).all() and (rows_buf == 5).all()
    return rc, L.vk_last_error_string().decode()


def test_patch_index_argument_errors(vk):
    ok = (0, 0, 10, 12, 0)
    for items, kw, word in (
            ([(0, 0, 0, 12, 0)], {}, "size"), ([(0, 0, 10, 16385, 0)], {}, "size"), ([(2, 0, 10, 12, 0)], {}, "multiples of 4"),
            ([(0, 6, 10, 12, 0)], {}, "multiples of 4"), ([(-4, 0, 10, 12, 0)], {}, "negative"), ([ok], dict(images_bytes=359), "image"),
            ([ok], dict(masks_bytes=119), "mask"), ([ok], dict(rows=9), "row table"), ([ok, (360, 120, 10, 12, 5)], dict(rows=14), "row table"),
            ([ok], dict(masks=False), "null")):
        rc, err = _index_rc(vk, items, **kw)
        assert rc == -1 and word in err, (items, kw, err)
    L = vk.lib()
    assert L.vk_patch_index(0, None, None, 0, None, 0, None, 0, None) == -1
    assert L.vk_patch_index(1, None, None, 0, None, 0, None, 0, None) == -1


def _batch_rc(vk, n=1, S=8, n_items=2, flags=0, null=None, **draw):
    L = vk.lib()
    d = dict(item=0, k=-1, oy=0, ox=0, zoom=1.0, cos_a=1.0, sin_a=0.0)
    d.update(draw)
    arr = vk.patches._patch_array([d] * max(n, 1))
    bufs = {name: np.full(64, 7, np.uint8) for name in ("items", "images", "masks", "rowcum", "pdev", "origins", "rgb", "mask_out")}
    ptr = {name: (None if name == null else b.ctypes.data) for name, b in bufs.items()}
    rc = L.vk_patch_batch(n, S, n_items, ptr["items"], ptr["images"], ptr["masks"], ptr["rowcum"], arr, ptr["pdev"], flags, ptr["origins"],
                          ptr["rgb"], ptr["mask_out"], None)
    assert all((b == 7).all() for b in bufs.values())
    return rc, L.vk_last_error_string().decode()


def test_patch_batch_argument_errors(vk):
    for kw, word in ((dict(n=0), "batch"), (dict(n=65536), "batch"), (dict(S=0), "patch size"), (dict(S=16385), "patch size"),
                     (dict(item=2), "item"), (dict(item=-1), "item"), (dict(zoom=0.2), "zoom"), (dict(zoom=4.5), "zoom"),
                     (dict(zoom=float("nan")), "zoom"), (dict(cos_a=1.0, sin_a=0.1), "rotation"), (dict(cos_a=float("nan")), "rotation"),
                     (dict(oy=-1), "offset"), (dict(flags=2), "flags"), (dict(null="origins"), "null"), (dict(null="images"), "null"),
                     (dict(null="rowcum"), "null"), (dict(null="mask_out"), "null")):
        rc, err = _batch_rc(vk, **kw)
        assert rc == -1 and word in err, (kw, err)


def test_patch_dataset_refuses_the_cpu_and_bad_items(vk):
    img, m = np.zeros((4, 4, 3), np.uint8), np.zeros((4, 4), np.uint8)
    with pytest.raises(vk.VkError):
        vk.PatchDataset([img], [m], device="cpu")
    with pytest.raises(ValueError):
        vk.PatchDataset([img], [m, m], device="cpu")
    with pytest.raises(ValueError):
        vk.PatchDataset([], [], device="cpu")
