"""vk.micrographs on the MI355X: vk_mg_render against the numpy restatement of micrographs_ref.py, byte for byte, into sentinel-filled
buffers with a guard zone on both sides; then determinism, MicrographDataset's batches against vk_augment_batch called by the test, and
detect_gt on the rendered masks against truth().  Integer arithmetic throughout: every comparison is EXACT."""
import ctypes as C
import importlib

import numpy as np
import pytest
import torch

import micrographs_cases as MC
import micrographs_ref as R

pytestmark = pytest.mark.gpu
vk = importlib.import_module("vickers-hardness-unet_amd")
L = vk._lib
M = vk.micrographs
DEV = torch.device("cuda:0")
GUARD = 256
I_SENTINEL = -(2 ** 31)
_REF = {}


def _ref(key, scenes, S):
    """The restatement of a case, computed once and left unchanged."""
    if key not in _REF:
        rgb, msk = R.render_batch_ref(scenes, S)
        rgb.setflags(write=False)
        msk.setflags(write=False)
        _REF[key] = (rgb, msk)
    return _REF[key]


def _guarded(numel, dtype, fill):
    buf = torch.full((numel + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + numel]


def _intact(buf, numel, fill):
    return bool((buf[:GUARD] == fill).all() and (buf[GUARD + numel:] == fill).all())


def _render_abi(scenes, S, fill):
    """vk_mg_render through the C ABI into guarded outputs filled with ``fill`` -> numpy (rgb, mask)."""
    arr = M._scene_array(scenes)
    n = arr.shape[0]
    rbuf, rgb = _guarded(n * S * S * 3, torch.uint8, fill)
    mbuf, msk = _guarded(n * S * S, torch.uint8, fill)
    words = int(L.lib().vk_mg_scenes_dev_bytes(n)) // 4
    sbuf, sdev = _guarded(words, torch.int32, I_SENTINEL)
    L.check(L.lib().vk_mg_render(n, S, arr.ctypes.data, sdev.data_ptr(), words * 4, rgb.data_ptr(), msk.data_ptr(), L.current_stream()), "vk_mg_render")
    torch.cuda.synchronize()
    assert _intact(rbuf, n * S * S * 3, fill) and _intact(mbuf, n * S * S, fill), "write beyond the outputs"
    assert _intact(sbuf, words, I_SENTINEL), "write beyond the scene scratch"
    m = msk.view(n, S, S).cpu().numpy()
    assert np.isin(m, (0, 1)).all(), "mask not fully overwritten"
    return rgb.view(n, S, S, 3).cpu().numpy(), m


def _check(key, scenes, S):
    want_rgb, want_m = _ref(key, scenes, S)
    # the sentinel is a legal pixel value: two fills, so that a byte left unwritten shows in one of them
    for fill in (7, 200):
        rgb, m = _render_abi(scenes, S, fill)
        for j in range(len(scenes)):
            assert np.array_equal(m[j], want_m[j]), (key, j, np.argwhere(m[j] != want_m[j])[:4])
            assert np.array_equal(rgb[j], want_rgb[j]), (key, j, np.argwhere((rgb[j] != want_rgb[j]).any(axis=2))[:4])


@pytest.mark.parametrize("case", MC.render_cases(), ids=[c[0] for c in MC.render_cases()])
def test_render_equals_the_restatement(case):
    name, S, scenes = case
    _check(name, scenes, S)
    want_rgb, want_m = _ref(name, scenes, S)
    if any(int(s["n_indents"]) for s in scenes):
        assert want_m.any()
    assert want_rgb.shape == (len(scenes), S, S, 3)


def test_render_default_scene_at_512():
    s = vk.SceneSampler(seed=3).sample()
    assert int(s["n_indents"]) >= 1 and int(s["n_scratches"]) >= 8
    _check("default 512", [s], 512)


# ------------------------------------------------------------------------------------------------ determinism and batching
def test_rendering_twice_gives_equal_bytes():
    name, S, scenes = [c for c in MC.render_cases() if c[0] == "S80 three scenes"][0]
    a = [t.clone() for t in M.render(scenes, S, DEV)]
    b = M.render(scenes, S, DEV)
    assert a[0].data_ptr() != b[0].data_ptr() and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    want_rgb, want_m = _ref(name, scenes, S)
    assert np.array_equal(b[0].cpu().numpy(), want_rgb) and np.array_equal(b[1].cpu().numpy(), want_m)
    assert b[0].shape == (3, S, S, 3) and b[1].shape == (3, S, S) and b[0].dtype == b[1].dtype == torch.uint8
    rgb1, m1 = M.render(np.stack(scenes)[1:2], S, DEV)                      # a structured array goes in as it is
    assert np.array_equal(rgb1.cpu().numpy(), want_rgb[1:2]) and np.array_equal(m1.cpu().numpy(), want_m[1:2])


@pytest.fixture(scope="module")
def ds():
    return vk.MicrographDataset(8, size=64, seed=5, device=DEV, sampler_kwargs=dict(max_indents=2, half_diag=(0.08, 0.16)))


def _draws(n):
    sm = vk.AugmentSampler(seed=3)
    return [sm.sample() for _ in range(n)]


def test_batch_does_not_depend_on_the_order(ds):
    d = _draws(2)
    x, y, names = ds.batch([3, 1], draws=d)
    x2, y2, names2 = ds.batch([1, 3], draws=d[::-1])
    assert torch.equal(x, x2.flip(0)) and torch.equal(y, y2.flip(0)) and names == names2[::-1] == ["mg000003", "mg000001"]
    assert not torch.equal(x[0], x[1])
    xv, yv, _ = ds.batch([3, 1])                                             # no sampler: the validation pipeline
    assert torch.equal(yv[:, 0], ds.masks([3, 1]).float()) and yv.sum() > 0
    assert np.array_equal(ds.images([3]).cpu().numpy()[0], R.render_ref(ds.scene(3), 64)[0])


def test_batch_is_augment_over_the_rendered_buffers(ds):
    idx = [6, 0, 2, 2, 7, 5]
    d = _draws(len(idx))
    assert any(int(p["photo"]) == vk.augment.PHOTO_CLAHE for p in d) and any(int(p["rotate"]) for p in d)
    x, y, names = ds.batch(idx, draws=d)
    n, S = len(idx), ds.S
    assert x.shape == (n, 3, S, S) and y.shape == (n, 1, S, S) and x.dtype == y.dtype == torch.float32 and names == [ds.names[i] for i in idx]
    rgb, msk = M.render([ds.scene(i) for i in idx], S, DEV)
    xe = torch.empty(n, 3, S, S, dtype=torch.float32, device=DEV)
    ye = torch.empty(n, 1, S, S, dtype=torch.float32, device=DEV)
    ws_bytes = int(L.lib().vk_augment_workspace_bytes(n, S))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    pdev = torch.empty(n * C.sizeof(L.vk_aug_params), dtype=torch.uint8, device=DEV)
    tables = torch.from_numpy(vk.augment.color_tables()).to(DEV)
    L.check(L.lib().vk_augment_batch(n, S, n, rgb.data_ptr(), msk.data_ptr(), torch.arange(n, dtype=torch.int32, device=DEV).data_ptr(),
                                     vk.augment._params_array(d, S), pdev.data_ptr(), tables.data_ptr(), ws.data_ptr(), ws_bytes, xe.data_ptr(),
                                     ye.data_ptr(), L.current_stream()), "vk_augment_batch")
    assert torch.equal(x, xe) and torch.equal(y, ye)
    assert set(torch.unique(y).tolist()) <= {0.0, 1.0} and torch.isfinite(x).all()
    batches = list(ds.loader(batch_size=3, shuffle=True, sampler=vk.AugmentSampler(seed=1, clahe="skip"), seed=4))
    assert [b[0].shape[0] for b in batches] == [3, 3, 2] and sorted(sum((b[2] for b in batches), [])) == ds.names
    with pytest.raises(ValueError):
        ds.batch([0, 1], draws=_draws(1))
    with pytest.raises(ValueError):
        ds.batch([8])
    with pytest.raises(ValueError):
        list(ds.loader(batch_size=0))
    bad = ds.scene(0).copy()
    bad["blur_r"] = 4
    with pytest.raises(vk.VkError, match="blur radius 4"):
        M.render([bad], 64, DEV)
    with pytest.raises(ValueError):
        M.render([bad], 8, DEV)


def test_detect_gt_finds_the_indentations_of_truth():
    S = 128
    s = MC.two_indent_scene(S)
    truth = M.truth(s)
    assert len(truth) == 2
    _, mask = M.render([s], S, DEV)
    det = vk.instances.detect_gt(mask, max_components=8)
    assert det.counts.tolist() == [2]
    rows = det.records()[0]
    slots = det.slots[0].cpu().numpy()
    X, Y = np.meshgrid(16 * np.arange(S, dtype=np.int64), 16 * np.arange(S, dtype=np.int64))
    sets = [R.inside(s["indents"][k], X, Y) for k in range(2)]
    assert not (sets[0] & sets[1]).any()
    seen = set()
    for slot, row in enumerate(rows):
        px = slots == slot
        k = [i for i in range(2) if np.array_equal(px, sets[i])]
        assert len(k) == 1, "a component is not the pixel set of one indentation"
        seen.add(k[0])
        assert int(row["area"]) == int(sets[k[0]].sum())
        x0, y0, x1, y1 = truth[k[0]]["box"]
        ys, xs = np.nonzero(px)
        assert np.ceil(x0) <= xs.min() and xs.max() <= np.floor(x1) and np.ceil(y0) <= ys.min() and ys.max() <= np.floor(y1)
    assert seen == {0, 1} and (slots >= 0).sum() == mask.sum().item()
