"""vk.tiling on the MI355X: vk_tile_preprocess / vk_tile_blend against the numpy restatements of tiling_ref.py (bit for bit where the
arithmetic is fp32 + - * / only, within tiling_cases.prob_bound where the device's expf is in the chain), and Segmenter.infer_tiled end
to end against the same model run view by view."""
import importlib

import numpy as np
import pytest
import torch

import tiling_cases as TC
import tiling_ref as R

pytestmark = pytest.mark.gpu
vk = importlib.import_module("vickers-hardness-unet_amd")
DEV = torch.device("cuda:0")
GUARD = 64
F_SENTINEL, U_SENTINEL = float("nan"), 7      # NaN: no finite input produces it (an integer sentinel can be a lattice logit)


def _blend_guarded(lg, case, tta, mode, thresh):
    """vk.tiling.tile_blend into sentinel-filled buffers with a guard zone behind [C][h][w]; returns numpy (map, mask)."""
    grid = vk.tiling.tile_grid(case.h, case.w, case.T, case.overlap)
    n = lg.shape[1] * case.h * case.w
    fbuf = torch.full((n + GUARD,), F_SENTINEL, dtype=torch.float32, device=DEV)
    ubuf = torch.full((n + GUARD,), U_SENTINEL, dtype=torch.uint8, device=DEV)
    shape = (lg.shape[1], case.h, case.w)
    out, mask = vk.tiling.tile_blend(torch.from_numpy(lg).to(DEV), grid, tta, mode, thresh, out=fbuf[:n].view(shape), mask=ubuf[:n].view(shape))
    torch.cuda.synchronize()
    assert torch.isnan(fbuf[n:]).all() and (ubuf[n:] == U_SENTINEL).all(), "write beyond [C][h][w]"
    out, mask = out.cpu().numpy(), mask.cpu().numpy()
    assert not np.isnan(out).any() and np.isin(mask, (0, 255)).all(), "output not fully overwritten"
    return out, mask


@pytest.mark.parametrize("tta", TC.TTAS)
@pytest.mark.parametrize("case", TC.CASES, ids=TC.CASE_IDS)
def test_preprocess_bit_exact(case, tta):
    img = TC.image(case)
    grid = vk.tiling.tile_grid(case.h, case.w, case.T, case.overlap)
    for pad in (0, 114):
        want = R.preprocess_ref(img, case.T, case.overlap, tta, pad)
        nv = len(R.TTA_VIEWS[tta])
        buf = torch.full((want.size + GUARD,), F_SENTINEL, dtype=torch.float32, device=DEV)
        got = vk.tiling.tile_preprocess(img, grid, tta, DEV, pad_value=pad)
        again = vk.tiling.tile_preprocess(torch.from_numpy(img), grid, tta, DEV, pad_value=pad)
        assert got.shape == (case.ntiles * nv, 3, case.T, case.T) == want.shape
        assert torch.equal(got, again)
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
        # straight through the C ABI into a guarded buffer: nothing behind [ntiles*nviews][3][T][T] is written
        import ctypes as C
        d = vk.tiling._desc(grid, tta, stride=3 * case.w, pad_value=pad)
        src = torch.from_numpy(img).to(DEV)
        vk._lib.check(vk.lib().vk_tile_preprocess(C.byref(d), src.data_ptr(), buf.data_ptr(), vk._lib.current_stream()))
        torch.cuda.synchronize()
        assert torch.isnan(buf[want.size:]).all() and torch.equal(buf[:want.size].view(got.shape), got)


def test_preprocess_one_tile_equals_letterbox_preprocess():
    for T in (16, 32, 64):
        img = np.random.default_rng(T).integers(0, 256, (T, T, 3), dtype=np.uint8)
        x = vk.tiling.tile_preprocess(img, vk.tiling.tile_grid(T, T, T, 0), "none", DEV)
        y, _ = vk.prepost.preprocess(img, T, "pad_br", DEV)
        assert torch.equal(x, y)


@pytest.mark.parametrize("tta", TC.TTAS)
@pytest.mark.parametrize("case", TC.CASES, ids=TC.CASE_IDS)
def test_blend_logit_mode_bit_exact(case, tta):
    nv, nc = len(R.TTA_VIEWS[tta]), TC.max_cover(case)
    for C in TC.CLASSES:
        inputs = [("random", TC.random_logits(case, tta, C, seed=C))]
        if case.lattice:
            inputs.append(("lattice", TC.lattice_logits(case, tta, C, seed=C)))
        for kind, lg in inputs:
            args = (lg, case.h, case.w, case.T, case.overlap, tta, "logit")
            want = R.blend_ref(*args, np.float32)
            got, mask = _blend_guarded(lg, case, tta, "logit", TC.THRESH)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (C, kind)
            got2, mask2 = _blend_guarded(lg, case, tta, "logit", TC.THRESH)
            assert np.array_equal(got.view(np.uint32), got2.view(np.uint32)) and np.array_equal(mask, mask2)
            w64 = R.blend_ref(*args, np.float64)
            if kind == "lattice":
                assert np.array_equal(got, w64.astype(np.float32)), (C, kind)
            band = TC.mask_band(R.sigmoid(w64), TC.logit_mask_bound(nv, nc, float(np.abs(lg).max())))
            assert band.mean() <= 0.01
            assert np.array_equal(mask[~band], R.mask_ref(w64, "logit", TC.THRESH)[~band]), (C, kind)


@pytest.mark.parametrize("tta", TC.TTAS)
@pytest.mark.parametrize("case", TC.CASES, ids=TC.CASE_IDS)
def test_blend_prob_mode_within_bound(case, tta):
    nv, nc = len(R.TTA_VIEWS[tta]), TC.max_cover(case)
    bound = TC.prob_bound(nv, nc)
    for C in TC.CLASSES:
        lg = TC.random_logits(case, tta, C, seed=10 + C)
        want = R.blend_ref(lg, case.h, case.w, case.T, case.overlap, tta, "prob", np.float64)
        got, mask = _blend_guarded(lg, case, tta, "prob", TC.THRESH)
        err = np.abs(got.astype(np.float64) - want).max()
        print(f"{case.name} {tta} C={C}: max|p - p64| = {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (C, err, bound)
        assert got.min() >= 0.0 and got.max() <= 1.0
        band = TC.mask_band(want, bound)
        assert band.mean() <= 0.01
        assert np.array_equal(mask[~band], R.mask_ref(want, "prob", TC.THRESH)[~band]), C
        got2, mask2 = _blend_guarded(lg, case, tta, "prob", TC.THRESH)
        assert np.array_equal(got.view(np.uint32), got2.view(np.uint32)) and np.array_equal(mask, mask2)


def test_blend_single_outputs():
    """Either output alone (the other pointer NULL) gives the same bits as both together."""
    case, tta = TC.CASES[3], "d4"
    lg = TC.random_logits(case, tta, 3)
    grid = vk.tiling.tile_grid(case.h, case.w, case.T, case.overlap)
    t = torch.from_numpy(lg).to(DEV)
    both_out, both_mask = vk.tiling.tile_blend(t, grid, tta, "prob", 0.5)
    assert torch.equal(vk.tiling.tile_blend(t, grid, tta, "prob"), both_out)
    assert torch.equal(vk.tiling.tile_blend(t, grid, tta, "prob", 0.5, values=False), both_mask)


@pytest.mark.parametrize("T", [8, 16, 32])
def test_blend_is_d4_equivariant(T):
    """One tile covering a square image: the view stack of the image transformed by g is the stack permuted by v -> g o v, and its
    blend is the transformed map.  Integer logits, so the eight-term sums are exact and the equality holds bit for bit."""
    case = TC.Case("square", T, T, T, 0)
    lg = TC.lattice_logits(case, "d4", 3, seed=T)
    grid = vk.tiling.tile_grid(T, T, T, 0)
    base = vk.tiling.tile_blend(torch.from_numpy(lg).to(DEV), grid, "d4", "logit").cpu().numpy()
    for g in range(8):
        perm = [R.compose(g, v) for v in range(8)]
        got = vk.tiling.tile_blend(torch.from_numpy(lg[perm]).to(DEV), grid, "d4", "logit").cpu().numpy()
        i0, j0 = R.view_index(g, T)
        assert np.array_equal(got, base[:, i0, j0]), g


# ------------------------------------------------------------------------------------------------ end to end, with the model
E2E = dict(h=100, w=150, T=64, overlap=16)


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(42)
    return vk.Unet(encoder_name="resnet34", encoder_weights=None, in_channels=3, classes=1, activation=None).to(DEV).eval()


@pytest.fixture(scope="module")
def e2e_image():
    return np.random.default_rng(5).integers(0, 256, (E2E["h"], E2E["w"], 3), dtype=np.uint8)


@pytest.mark.parametrize("tta", ["none", "d4"])
def test_infer_tiled_end_to_end(model, e2e_image, tta):
    h, w, T, ov = E2E["h"], E2E["w"], E2E["T"], E2E["overlap"]
    seg = vk.Segmenter(model, img_size=T, device=DEV)
    got = seg.infer_tiled(e2e_image, overlap=ov, tta=tta, batch=16)
    assert got.shape == (h, w) and got.dtype == np.float32
    # numpy crops -> reference pre-processing -> the model view by view -> reference blend
    x = torch.from_numpy(R.preprocess_ref(e2e_image, T, ov, tta)).to(DEV)
    with torch.no_grad():
        lg = torch.cat([model(x[i:i + 1]) for i in range(x.shape[0])]).cpu().numpy()
    want = R.blend_ref(lg, h, w, T, ov, tta, "prob", np.float32)[0]
    err = np.abs(got - want).max()
    print(f"infer_tiled {tta}: max|p - p_ref| = {err:.3e}")
    assert err <= 1e-3          # the project's fp32 end-to-end tolerance (test_prepost_gpu.py): logits agree to 1e-3, sigmoid' <= 1/4
    mask = vk.predict_mask_tiled(model, e2e_image, DEV, tile=T, overlap=ov, tta=tta, thresh=0.5)
    assert mask.shape == (h, w) and mask.dtype == np.uint8
    differ = mask != R.mask_ref(want, "prob", 0.5)
    with np.errstate(divide="ignore"):
        ref_logit = np.log(want.astype(np.float64) / (1.0 - want.astype(np.float64)))      # the logit of the blended probability
    assert not differ.any() or np.abs(ref_logit[differ]).max() <= 1e-3, int(differ.sum())


def test_infer_tiled_one_exact_tile_equals_postprocess_prob(model):
    T = 64
    img = np.random.default_rng(6).integers(0, 256, (T, T, 3), dtype=np.uint8)
    got = vk.Segmenter(model, img_size=T, device=DEV).infer_tiled(img, overlap=0, tta="none", batch=16)
    grid = vk.tiling.tile_grid(T, T, T, 0)
    x = vk.tiling.tile_preprocess(img, grid, "none", DEV)
    with torch.no_grad():
        lg = model(torch.cat([x, x.new_zeros(15, 3, T, T)]))[:1]
    meta = (1.0, (1.0, T, T, 0, 0), (T, T))
    want = vk.prepost.postprocess_prob(lg[0, 0], meta)
    assert torch.equal(vk.tiling.tile_blend(lg, grid, "none", "prob")[0], want)
    assert np.array_equal(got, want.cpu().numpy())


def test_infer_tiled_multiclass():
    torch.manual_seed(42)
    m = vk.multiclass.Unet(encoder_name="resnet34", encoder_weights=None, in_channels=3, classes=3, activation=None).to(DEV).eval()
    img = np.random.default_rng(7).integers(0, 256, (70, 90, 3), dtype=np.uint8)
    seg = vk.multiclass.Segmenter(m, mode="multiclass", img_size=64, device=DEV)
    out = seg.infer_tiled(img, overlap=16, tta="hflip", blend="logit", batch=8)
    assert out.shape == (3, 70, 90) and out.dtype == np.float32 and np.isfinite(out).all()
    with pytest.raises(NotImplementedError, match='blend="logit"'):
        seg.infer_tiled(img, overlap=16, blend="prob")
    probs = vk.multiclass.Segmenter(m, mode="multilabel", img_size=64, device=DEV).infer_tiled(img, overlap=16, blend="prob", batch=8)
    assert probs.shape == (3, 70, 90) and probs.min() >= 0.0 and probs.max() <= 1.0
