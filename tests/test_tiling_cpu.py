"""Host side of vk.tiling (no GPU): the grid rule, the view algebra, the two numpy restatements of the blend against each other and
against the bounds of tiling_cases.py, and the argument checks of vk_tile_preprocess / vk_tile_blend through the loaded library."""
import ctypes as C
import itertools

import numpy as np
import pytest

import tiling_cases as TC
import tiling_ref as R


# ------------------------------------------------------------------------------------------------ grid
AXES = [(L, T, ov) for T, ov in ((8, 0), (8, 4), (16, 4), (16, 8), (32, 6), (512, 64)) for L in (1, T - 1, T, T + 1, 2 * T - ov, 2 * T - ov + 1, 5 * T + 3)]


@pytest.mark.parametrize("L,T,ov", AXES)
def test_axis_origins_cover_and_last_tile_is_flush(vk, L, T, ov):
    org = vk.tiling.axis_origins(L, T, ov)
    assert list(org) == R.axis_origins(L, T, ov)
    s = T - ov
    assert len(org) == (1 if L <= T else -(-(L - T) // s) + 1)
    assert org[0] == 0 and all(b > a for a, b in zip(org, org[1:]))
    covered = np.zeros(max(L, T), bool)
    for o in org:
        covered[o:o + T] = True
    assert covered[:L].all()
    assert org[-1] + T == max(L, T)                      # flush with the edge; padding only where L < T
    assert all(o == i * s for i, o in enumerate(org[:-1]))
    cover = sum(np.pad(np.ones(T, int), (o, max(L, T) - o - T)) for o in org)
    assert cover.max() <= 3


def test_overlap_zero_partitions_a_multiple_of_the_tile(vk):
    g = vk.tiling.tile_grid(48, 32, tile=16, overlap=0)
    assert g.ys == (0, 16, 32) and g.xs == (0, 16) and g.ntiles == 6 and g.origin(3) == (16, 16)
    assert (R.cover_count(48, 32, 16, 0) == 1).all()


def test_grid_limits_raise(vk):
    tg = vk.tiling.tile_grid
    tg(64, 64, 8, 0)                                       # 8 origins
    tg(8 + 63 * 8, 8, 8, 0)                                # exactly 64 origins
    for bad in ((8 + 63 * 8 + 1, 8, 8, 0), (8, 8 + 63 * 4 + 1, 8, 4), (64, 64, 16, 9), (64, 64, 16, -1), (64, 64, 0, 0),
                (64, 64, 4097, 0), (0, 5, 8, 0)):
        with pytest.raises(ValueError):
            tg(*bad)
    with pytest.raises(ValueError):
        vk.tiling._views("rot90")


# ------------------------------------------------------------------------------------------------ views
def test_views_are_distinct_and_invert(vk):
    T = 5
    maps = []
    for v in range(8):
        i0, j0 = R.view_index(v, T)
        maps.append((i0 * T + j0).tobytes())
        i, j = R.inverse_index(v, T)
        assert (i0[i, j] == np.arange(T)[:, None]).all() and (j0[i, j] == np.arange(T)[None, :]).all()
        for a, b in itertools.product(range(T), range(T)):
            assert vk.tiling.view_map(v, T, a, b) == (i0[a, b], j0[a, b])
            assert vk.tiling.view_inverse(v, T, *vk.tiling.view_map(v, T, a, b)) == (a, b)
    assert len(set(maps)) == 8


def test_view_sets_are_closed(vk):
    assert vk.tiling.TTA_VIEWS == R.TTA_VIEWS
    for name, views in R.TTA_VIEWS.items():
        assert len(views) in (1, 2, 4, 8)
        assert {R.compose(g, v) for g in views for v in views} == set(views), name
    # the views agree with numpy's own flips and transposition
    a = np.arange(12 * 12).reshape(12, 12)
    want = {0: a, 1: a[:, ::-1], 2: a[::-1], 3: a[::-1, ::-1], 4: a.T, 5: a[:, ::-1].T, 6: a[::-1].T, 7: a[::-1, ::-1].T}
    for v in range(8):
        assert (a[R.view_index(v, 12)] == want[v]).all(), v


# ------------------------------------------------------------------------------------------------ the two references
@pytest.mark.parametrize("tta", TC.TTAS)
@pytest.mark.parametrize("case", TC.CASES, ids=TC.CASE_IDS)
def test_constant_logits_blend_to_the_constant(case, tta):
    """Exactly, where the arithmetic allows it: an integer constant on a power-of-two ramp (every product and sum is exact), and
    logit 0 in prob mode (sigmoid 0.5).  On any other ramp the weights are rounded, and the constant comes back within the bound."""
    n = case.ntiles * len(R.TTA_VIEWS[tta])
    for dt in (np.float32, np.float64):
        zero = np.zeros((n, 2, case.T, case.T), np.float32)
        seven = np.full((n, 2, case.T, case.T), -7.0, np.float32)
        p = R.blend_ref(zero, case.h, case.w, case.T, case.overlap, tta, "prob", dt)
        l = R.blend_ref(seven, case.h, case.w, case.T, case.overlap, tta, "logit", dt)
        if case.lattice:
            assert (p == 0.5).all() and (l == -7.0).all()
        else:
            nv, nc = len(R.TTA_VIEWS[tta]), TC.max_cover(case)
            assert np.abs(p - 0.5).max() <= TC.prob_bound(nv, nc) and np.abs(l + 7.0).max() <= TC.logit_bound(nv, nc, 7.0)


@pytest.mark.parametrize("tta", TC.TTAS)
@pytest.mark.parametrize("case", [c for c in TC.CASES if c.lattice], ids=[c.name for c in TC.CASES if c.lattice])
def test_lattice_float32_equals_float64(case, tta):
    lg = TC.lattice_logits(case, tta, 3)
    a = R.blend_ref(lg, case.h, case.w, case.T, case.overlap, tta, "logit", np.float32)
    b = R.blend_ref(lg, case.h, case.w, case.T, case.overlap, tta, "logit", np.float64)
    assert a.dtype == np.float32 and (a == b.astype(np.float32)).all()


@pytest.mark.parametrize("tta", TC.TTAS)
@pytest.mark.parametrize("case", TC.CASES, ids=TC.CASE_IDS)
def test_float32_within_rounding_bound_and_mask_band_is_thin(case, tta):
    nv, nc = len(R.TTA_VIEWS[tta]), TC.max_cover(case)
    lg = TC.random_logits(case, tta, 3)
    args = (lg, case.h, case.w, case.T, case.overlap, tta)
    p32, p64 = R.blend_ref(*args, "prob", np.float32), R.blend_ref(*args, "prob", np.float64)
    bound = TC.prob_bound(nv, nc)
    assert np.abs(p32 - p64).max() <= bound
    band = TC.mask_band(p64, bound)
    assert band.mean() <= 0.01
    assert (R.mask_ref(p32, "prob", TC.THRESH)[~band] == R.mask_ref(p64, "prob", TC.THRESH)[~band]).all()
    l32, l64 = R.blend_ref(*args, "logit", np.float32), R.blend_ref(*args, "logit", np.float64)
    mag = float(np.abs(lg).max())
    assert np.abs(l32 - l64).max() <= TC.logit_bound(nv, nc, mag)
    assert TC.mask_band(R.sigmoid(l64), TC.logit_mask_bound(nv, nc, mag)).mean() <= 0.01


def test_preprocess_ref_is_the_letterbox_expression():
    """One tile, no view: the reference is crop + pad + the normalisation written out per channel."""
    c = TC.CASES[1]
    img = TC.image(c)
    x = R.preprocess_ref(img, c.T, c.overlap, "none", pad_value=3)
    assert x.shape == (1, 3, c.T, c.T) and x.dtype == np.float32
    y, xx, k = 2, 5, 0
    want = (np.float32(img[y, xx, 2]) / np.float32(255) - np.float32(0.485)) / np.float32(0.229)
    assert x[0, k, y, xx] == want
    pad = (np.float32(3) / np.float32(255) - np.float32(0.406)) / np.float32(0.225)
    assert x[0, 2, c.T - 1, c.T - 1] == pad


# ------------------------------------------------------------------------------------------------ argument checks of the library
def _desc(vk, h=33, w=47, T=16, ov=4, tta="d4", classes=1):
    g = vk.tiling.tile_grid(h, w, T, ov)
    return vk.tiling._desc(g, tta, stride=3 * w, classes=classes), g


def _call_both(vk, d, out_arg=True, mask_arg=True, pre=True):
    """Both entry points on host buffers: a failed check returns before anything is read or written (so only descriptors that fail
    may come here; pre=False where the pre-processing would accept the descriptor)."""
    L = vk.lib()
    src = np.full(16, 9, np.uint8)
    x = np.full(16, 7.0, np.float32)
    lg = np.full(16, 5.0, np.float32)
    out = np.full(16, 3.0, np.float32)
    mask = np.full(16, 2, np.uint8)
    rc_pre = L.vk_tile_preprocess(C.byref(d), src.ctypes.data, x.ctypes.data, None) if pre else None
    err_pre = L.vk_last_error_string().decode()
    rc_blend = L.vk_tile_blend(C.byref(d), vk._lib.VK_BLEND_PROB, lg.ctypes.data, 0.5, out.ctypes.data if out_arg else None,
                               mask.ctypes.data if mask_arg else None, None)
    err_blend = L.vk_last_error_string().decode()
    assert (x == 7.0).all() and (out == 3.0).all() and (mask == 2).all()
    return rc_pre, err_pre, rc_blend, err_blend


def test_err_arg_bad_overlap(vk):
    d, _ = _desc(vk)
    d.overlap = 9
    rc_pre, err_pre, rc_blend, err_blend = _call_both(vk, d)
    assert rc_pre == rc_blend == -1 and "overlap" in err_pre and "overlap" in err_blend


def test_err_arg_too_many_origins(vk):
    d, _ = _desc(vk)
    d.ny = 65
    rc_pre, err_pre, rc_blend, err_blend = _call_both(vk, d)
    assert rc_pre == rc_blend == -1 and "origins" in err_pre and "origins" in err_blend


def test_err_arg_origins_off_the_rule(vk):
    d, _ = _desc(vk)
    d.ys[1] += 1
    rc_pre, _, rc_blend, err = _call_both(vk, d)
    assert rc_pre == rc_blend == -1 and "origins" in err
    d, _ = _desc(vk)
    d.view_mask = 0x05
    rc_pre, _, rc_blend, err = _call_both(vk, d)
    assert rc_pre == rc_blend == -1 and "view mask" in err


def test_err_arg_seventeen_classes_and_null_outputs(vk):
    d, _ = _desc(vk, classes=17)
    _, _, rc_blend, err = _call_both(vk, d, pre=False)
    assert rc_blend == -1 and "C = 17" in err
    d, _ = _desc(vk)
    _, _, rc_blend, err = _call_both(vk, d, out_arg=False, mask_arg=False, pre=False)
    assert rc_blend == -1 and "null" in err
    L = vk.lib()
    assert L.vk_tile_preprocess(None, None, None, None) == -1 and L.vk_tile_blend(None, 0, None, 0.5, None, None, None) == -1


def test_python_entry_points_refuse_wrong_shapes(vk):
    import torch
    g = vk.tiling.tile_grid(33, 47, 16, 4)
    with pytest.raises(ValueError):
        vk.tiling.tile_blend(torch.zeros(g.ntiles * 8, 1, 16, 15), g, "d4")
    with pytest.raises(ValueError):
        vk.tiling.tile_blend(torch.zeros(g.ntiles, 1, 16, 16), g, "d4")
    with pytest.raises(vk.VkError):
        vk.tiling.tile_blend(torch.zeros(g.ntiles, 1, 16, 16), g, "none")      # a CPU tensor: no fallback
    with pytest.raises(ValueError):
        vk.tiling.tile_blend(torch.zeros(g.ntiles, 1, 16, 16), g, "none", mode="softmax")
