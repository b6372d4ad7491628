"""No GPU: the cases of tests/pipeline_cases.py are what their names claim, the CLAHE cases reach the branches they were built for, the
oracle stages the sweep leans on agree with independent scalar twins, no logit used sits within expf's rounding of a threshold, and
the metric reference agrees with the oracle's dice_coef / iou_coef.  DESIGN.md 41."""
import math

import numpy as np
import pytest
import torch

import pipeline_cases as PC
from oracle import augment_oracle as A
from oracle import prepost_oracle as P

F = np.float32


# ------------------------------------------------------------------------------------------------ A. images, masks, draws
@pytest.mark.parametrize("S", PC.AUG_SIZES)
def test_images_and_masks_are_what_they_claim(S):
    for n in PC.IMAGE_NAMES:
        a = PC.image(n, S)
        assert a.shape == (S, S, 3) and a.dtype == np.uint8, n
    for v in (0, 137, 255):
        assert (PC.image(f"const{v}", S) == v).all()
    c = PC.image("checker", S)
    for ch in range(3):
        assert len(np.unique(c[..., ch])) == 2 and (c[0, 0, ch] == c[1, 1, ch]) and (c[0, 0, ch] != c[0, 1, ch])
    r = PC.image("ramp", S)
    assert (r == r[0:1]).all() and (np.diff(r[0, :, 0].astype(int)) >= 0).all() and r[0, 0, 0] == 0 and r[0, -1, 0] == 255
    lv = PC.image("levels", S)
    assert (lv[..., 0] == lv[..., 1]).all() and (lv[..., 0] == lv[..., 2]).all()
    flat = lv[..., 0].ravel()
    assert np.array_equal(flat, (np.arange(S * S) % 256).astype(np.uint8))
    if S * S >= 256:
        assert np.array_equal(np.bincount(flat[:256], minlength=256), np.ones(256, int))     # every LUT entry is read
    t = PC.image("tiles", S)
    if S % 8 == 0:
        ts = S // 8
        blocks = t[..., 0].reshape(8, ts, 8, ts)
        assert (blocks == blocks[:, :1, :, :1]).all() and len(np.unique(blocks[:, 0, :, 0])) == 64
    k = PC.image("corners", S)
    lit = np.argwhere(k.any(-1))
    assert sorted(map(tuple, lit)) == [(0, 0), (0, S - 1), (S - 1, 0), (S - 1, S - 1)]
    assert len({tuple(k[y, x]) for y, x in lit}) == 4
    for n in PC.MASK_NAMES:
        m = PC.mask(n, S)
        assert m.shape == (S, S) and m.dtype == np.uint8 and set(np.unique(m)) <= {0, 1}, n
    assert PC.mask("zeros", S).sum() == 0 and PC.mask("ones", S).sum() == S * S and PC.mask("corners", S).sum() == 4
    assert 0 < PC.mask("random", S).sum() < S * S
    ck = PC.mask("checker", S)
    assert ck[0, 0] == 0 and ck[0, 1] == 1 and ck[1, 0] == 1 and ck[1, 1] == 0
    assert len(PC.items(S)) == len(PC.IMAGE_NAMES) and {n for n, _, _ in PC.items(S)} == set(PC.IMAGE_NAMES)


def test_sizes_hit_the_tile_edges_they_were_chosen_for():
    S = PC.AUG_SIZES
    assert min(S) == 8 and {9, 13} <= set(S) and all(s % 4 for s in (9, 13, 66, 67, 130))        # ragged last row block
    assert [s - 64 for s in (66, 67)] == [2, 3] and 130 - 128 == 2                                # a last column at most the apron + 1
    assert all(s < 64 for s in (8, 9, 13, 16, 24))                                                 # below one tile width
    ts2 = {(s // 8) ** 2 for s in S if s % 8 == 0}
    assert {1, 256, 289} <= ts2                                                                    # one pixel; one trip exactly; 33 more


@pytest.mark.parametrize("S", PC.AUG_SIZES)
def test_draw_lists(S):
    prod, fam = PC.product_draws(S), PC.family_draws(S)
    assert len(prod) == (140 if S % 8 == 0 else 112)
    combos = {(d["d4"], d["rotate"], d["photo"], d["blur_ksize"] if d["photo"] == 3 else 0, d["noise_scale"] > 0) for d in prod}
    assert len(combos) == len(prod)
    names = [d["name"] for d in prod + fam]
    assert len(set(names)) == len(names)
    exact = {(d["cos_a"], d["sin_a"]) for d in fam if d["rotate"] and d["name"].startswith("rot-x")}
    assert exact == {(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)}
    libm = {d["name"] for d in fam if d["name"].startswith("rot-m(") and d["photo"] == 0}
    assert len(libm) == 7
    assert sorted((d["alpha"], d["beta"]) for d in fam if d["photo"] == 1) == sorted(PC.RBC_CORNERS)
    assert {d["noise_seed"] for d in fam if d["noise_scale"] > 0} == {0, 1, 2 ** 31, 2 ** 32 - 1}
    assert {d["clahe_clip"] for d in fam if d["photo"] == 2} == (set(PC.CLAHE_CLIPS) if S % 8 == 0 else set())
    assert all(d["photo"] != 2 for d in prod + fam) or S % 8 == 0
    for d in prod + fam:                                                   # what the host validates
        assert 0 <= d["noise_scale"] < 1 and (not d["rotate"] or abs(F(d["cos_a"]) ** 2 + F(d["sin_a"]) ** 2 - 1) < 1e-3)


@pytest.mark.parametrize("S", [8, 9, 16])
def test_exact_rotations_are_rot90_on_the_oracle(S):
    """The properties the device test asserts without an oracle hold on the oracle: (1, 0) is the identity, the other exact pairs are
    np.rot90, RBC (1, 0) is no photometric transform, and the noise field depends on the seed alone."""
    img, m = PC.image("random", S), PC.mask("random", S)
    x0, y0 = A.augment(img, m, PC.IDENTITY)
    for n, (c, s) in PC.EXACT_ROT.items():
        x, y = A.augment(img, m, dict(PC.IDENTITY, rotate=1, cos_a=c, sin_a=s))
        k = PC.EXACT_ROT_K.get(n, 0)
        assert np.array_equal(x, np.rot90(x0, k, axes=(1, 2))) and np.array_equal(y, np.rot90(y0, k, axes=(1, 2))), n
    x, _ = A.augment(img, m, dict(PC.IDENTITY, photo=1, alpha=1.0, beta=0.0))
    assert np.array_equal(x, x0)
    g = dict(PC.IDENTITY, noise_scale=PC.NOISE_SCALES[0], noise_seed=7)
    mid = PC.image("const137", S)
    xa, _ = A.augment(mid, m, g)
    xb, _ = A.augment(mid, PC.mask("zeros", S), dict(g, d4=4))
    assert np.array_equal(xa, xb) and not np.array_equal(xa, A.augment(mid, m, PC.IDENTITY)[0])


# ------------------------------------------------------------------------------------------------ CLAHE reach
def test_clahe_cases_reach_every_branch():
    """Over (S, image, clip): tiles with clipped == 0, with residual == 0 after clipping, and with residual > 0 all occur, at ts^2 = 1,
    256 and 289; a constant tile puts all of ts^2 in one bin."""
    seen = {}
    for S in (8, 16, 128, 136):
        names = PC.image_names(S) if S in PC.AUG_ALL_IMAGES_AT else ("random", "const137", "tiles")
        for n in names:
            for clip in PC.CLAHE_CLIPS:
                st = PC.clahe_case_stats(PC.image(n, S), clip)
                seen[(S, n, clip)] = (any(c == 0 for c, _ in st), any(c > 0 and r == 0 for c, r in st), any(r > 0 for _, r in st))
    assert any(v[0] for v in seen.values()) and any(v[1] for v in seen.values()) and any(v[2] for v in seen.values())
    for S in (16, 128, 136):                       # at every tile area above one pixel, within the size's own cases
        mine = [v for k, v in seen.items() if k[0] == S]
        assert any(v[0] for v in mine) and any(v[2] for v in mine), S
    assert seen[(136, "levels33", 1.0)][1] and {c for c, _ in PC.clahe_case_stats(PC.image("levels33", 136), 1.0)} == {256}
    assert seen[(136, "tiles", 1.0)][2] and seen[(136, "const137", 2.0)][2]              # 289 - limit in one bin: residual on
    c, r = PC.clahe_case_stats(PC.image("const137", 136), 1.0)[0]
    assert c == 289 - A.clahe_limit(1.0, 136) and r == c % 256
    # S = 8: one pixel per tile, limit 1: nothing is ever clipped
    assert all(c == 0 for c, _ in PC.clahe_case_stats(PC.image("random", 8), 40.0)) and A.clahe_limit(40.0, 8) == 1


# ------------------------------------------------------------------------------------------------ scalar twins
@pytest.mark.parametrize("S", [8, 9, 13])
@pytest.mark.parametrize("k", [3, 5])
def test_blur_twin(S, k):
    for n in ("random", "corners", "checker"):
        img = PC.image(n, S)
        assert np.array_equal(A.gaussian_blur(img, k), PC.blur_twin(img, k)), n


@pytest.mark.parametrize("S", [8, 9, 16])
def test_rotation_twin(S):
    img, m = PC.image("random", S), PC.mask("random", S)
    pairs = list(PC.EXACT_ROT.values()) + [PC.ROT_33] + [(math.cos(math.radians(a)), math.sin(math.radians(a))) for a in PC.LIBM_ANGLES]
    for c, s in pairs:
        oi, om = A.rotate(img, m, c, s)
        assert np.array_equal(om, PC.rotate_mask_twin(m, c, s)), (c, s)
        assert np.array_equal(oi, PC.rotate_image_twin(img, c, s)), (c, s)
    # border rule: a one-pixel image corner rotated by 45 degrees leaves the frame; taps outside contribute 0, never a clamped pixel
    ones = np.full((S, S, 3), 255, np.uint8)
    oi, om = A.rotate(ones, PC.mask("ones", S), math.cos(math.pi / 4), math.sin(math.pi / 4))
    assert (oi[0, 0] == 0).all() and om[0, 0] == 0 and (oi[S // 2, S // 2] == 255).all()


@pytest.mark.parametrize("S", [8, 16])
def test_clahe_lut_twin(S):
    ts = S // 8
    for n in ("random", "const137", "levels"):
        L = A.rgb_to_lab_u8(PC.image(n, S), A.color_tables())[..., 0]
        for clip in PC.CLAHE_CLIPS:
            limit = A.clahe_limit(clip, S)
            # the oracle's LUT of a tile, read back through a plane made of that tile alone: with 64 equal tiles the four-LUT
            # interpolation returns lut[v] itself
            for ty, tx in ((0, 0), (3, 5), (7, 7)):
                tile = L[ty * ts:(ty + 1) * ts, tx * ts:(tx + 1) * ts]
                lut = PC.clahe_tile_stats(tile, limit)[2]
                plane = np.tile(tile, (8, 8))
                assert np.array_equal(A.clahe_u8(np.ascontiguousarray(plane), limit), lut[plane]), (n, clip, ty, tx)


def test_clahe_lut_twin_with_residual():
    """A tile that takes both residual branches: 16 x 16 pixels of one level at limit 3 leaves clipped = 253, residual 253, step 1."""
    tile = np.full((16, 16), 9, np.uint8)
    c, r, lut = PC.clahe_tile_stats(tile, 3)
    assert (c, r) == (253, 253)
    plane = np.tile(tile, (8, 8))
    assert np.array_equal(A.clahe_u8(plane, 3), lut[plane])
    tile2 = np.full((17, 17), 200, np.uint8)                              # clipped 289 - 1 = 288: batch 1, residual 32, step 8
    c, r, lut = PC.clahe_tile_stats(tile2, 1)
    assert (c, r) == (288, 32)
    plane = np.tile(tile2, (8, 8))
    assert np.array_equal(A.clahe_u8(plane, 1), lut[plane])


@pytest.mark.parametrize("seed", PC.NOISE_SEEDS)
def test_noise_counter_twin(seed):
    for S in (8, 13):
        got = A.noise_isum(seed, S)
        for y, x, ch in ((0, 0, 0), (0, 1, 2), (S - 1, S - 1, 2), (S // 2, 3, 1), (1, 0, 0)):
            assert int(got[y, x, ch]) == PC.noise_isum_twin(seed, S, y, x, ch)
    want = np.array([[[PC.noise_isum_twin(seed, 8, y, x, c) for c in range(3)] for x in range(8)] for y in range(8)])
    assert np.array_equal(A.noise_isum(seed, 8), want)


# ------------------------------------------------------------------------------------------------ B. letterbox cases
def test_letterbox_cases_cover_the_paths():
    geo = {(h, w, S): P.geometry_train(h, w, S)[1:] for S in PC.LB_SIZES for h, w in PC.lb_sources(S)}
    assert all(nh > 0 and nw > 0 for nh, nw, _, _ in geo.values())
    assert geo[(24, 24, 24)] == (24, 24, 0, 0)                                            # identity
    assert geo[(24, 12, 24)] == (24, 12, 0, 6)                                            # copy path with left > 0
    assert geo[(48, 24, 24)] == (24, 12, 0, 6)                                            # exact x 2 reduction
    assert geo[(1, 1, 8)][:2] == (8, 8) and geo[(3, 5, 24)][:2] == (14, 24) and geo[(7, 7, 67)][:2] == (67, 67)      # upscale
    assert geo[(2048, 37, 67)][:2] == (67, 1) and geo[(37, 2048, 67)][:2] == (1, 67)      # strong reduction to one column / row
    for h, w, S in PC.LB_REFUSED:
        assert 0 in P.geometry_train(h, w, S)[1:3]
    m = PC.raw_mask(25, 13)
    assert set(np.unique(m)) == {0, 1, 2, 255}
    sq, mm = PC.letterbox_ref(PC.bgr_image(25, 13), m, 24)
    assert set(np.unique(mm)) <= {0, 1} and sq.shape == (24, 24, 3)
    nh, nw, top, left = P.geometry_train(25, 13, 24)[1:]
    assert np.array_equal(mm[top:top + nh, left:left + nw], P.resize_nearest((m > 0).astype(np.uint8), nw, nh))
    img = PC.bgr_image(24, 12)
    assert np.array_equal(PC.letterbox_ref(img, PC.raw_mask(24, 12), 24)[0][:, 6:18], img[:, :, ::-1])      # the copy path swaps BGR
    assert len({tuple(img[3, 4])}) == 1 and len(set(img[0, 0].tolist())) == 3
    odd = [g for S in PC.LB_SIZES for h, w in PC.lb_sources(S) for g in PC.odd_geometries(h, w, S)]
    assert any(t % 2 and l % 2 for _, _, t, l in odd) and len(odd) >= 12
    assert any(g[:2] == (3, 5) for g in PC.odd_geometries(3, 5, 24))                      # copy path at (1, 3)
    flat, stride = PC.strided(img)
    assert stride == 12 * 3 + 5 and np.array_equal(flat.reshape(24, stride)[:, :36].reshape(24, 12, 3), img)
    assert (flat.reshape(24, stride)[:, 36:] == PC.FILL).all()


def test_pre_and_post_cases():
    refused = [(h, w, S, c) for S in PC.PRE_SIZES for h, w in PC.pre_sources() for c in PC.CONVENTIONS
               if PC.post_geometry(h, w, S, c) is None]
    assert (2048, 37, 8, "pad_br") in refused and len(refused) < 20          # these are asserted to be refused, not skipped
    for S, shapes in PC.POST_SHAPES.items():
        assert {w % 4 for _, w in shapes} == {0, 1, 2, 3} and shapes[0] == (S, S)
        for c in PC.CONVENTIONS:
            assert P.GEOMETRY[c](S, S, S)[1:3] == (S, S)
            assert all(PC.post_geometry(h, w, S, c) is not None for h, w in shapes)
    # every lattice value and every special occurs: in each map from 67 up, over the case list at 8
    want = set(PC.LATTICE.tolist())
    for S in (67, 256):
        lg = PC.logit_map(S, 3)
        assert want <= set(lg[np.isfinite(lg)].tolist())
    at8 = np.concatenate([PC.logit_map(8, i).ravel() for i in range(len(PC.POST_SHAPES[8]))])
    assert want <= set(at8[np.isfinite(at8)].tolist())
    for S in PC.POST_SHAPES:
        lg = PC.logit_map(S, 1).ravel()
        assert np.isnan(lg).sum() == 1 and np.isposinf(lg).sum() == 1 and np.isneginf(lg).sum() == 1
        assert {0.0, 88.0, -88.0, 100.0, -100.0} <= set(lg[np.isfinite(lg)].tolist())


def test_threshold_margin():
    """The condition under which masks can be demanded EQUAL: for every logit value used and every threshold, the oracle's mask bit is
    the same when exp(-x) is moved by -2 .. +2 ulp in float32.  expf on the device is then free to round either way."""
    v = PC.logit_values()
    for thr in PC.POST_THRESHOLDS:
        base = PC.mask_bit(v, thr)
        with np.errstate(over="ignore", invalid="ignore"):
            assert np.array_equal(base, P.sigmoid_f32(v) >= F(thr))
        for u in (-2, -1, 1, 2):
            assert np.array_equal(PC.mask_bit(v, thr, u), base), (thr, u, v[PC.mask_bit(v, thr, u) != base])
    # what the extremes were listed for: thresholds 0 and 1 are met with equality (>= true, > false)
    assert PC.mask_bit(np.array([-100, -np.inf, 17, 20, 88, np.inf], F), 0.0).all()
    with np.errstate(over="ignore"):
        assert (P.sigmoid_f32(np.array([-100, -np.inf], F)) == 0).all() and (P.sigmoid_f32(np.array([17, 20, 88, np.inf], F)) == 1).all()
    assert PC.mask_bit(np.array([17, 20, 88, np.inf], F), 1.0).all() and not PC.mask_bit(np.array([16.5, 0, -88], F), 1.0).any()
    assert PC.mask_bit(np.array([0.0], F), 0.5).all() and not PC.mask_bit(np.array([np.nan], F), 0.0).any()


def test_tiny_logits_fail_the_margin():
    """+-1e-30 (in the issue's list) cannot be held to equality at 0.5: a +2 ulp exp gives 1 / (2 + 2^-22) < 0.5.  They are left out."""
    x = PC.DROPPED_SPECIALS
    assert PC.mask_bit(x, 0.5).all() and not PC.mask_bit(x, 0.5, 2).any()
    assert not set(x.tolist()) & set(PC.logit_values().tolist())


# ------------------------------------------------------------------------------------------------ D. metric reference
@pytest.mark.parametrize("n,per", [s for s in PC.MET_SHAPES if s[0] * s[1] <= 1 << 16])
def test_metric_reference_against_the_oracle(n, per):
    from oracle import unet_oracle as O
    prob, tgt = PC.met_inputs(n, per)
    assert set(np.unique(tgt)) <= {0.0, 1.0} and tgt[0].sum() == 0
    if per >= 17:
        assert all((prob == F(t)).any() for t in PC.MET_THRESHOLDS)                      # a probability ON every threshold
    I, Pn, T = PC.met_counts(prob > F(0.5), tgt)
    if n > 1:
        assert Pn[1] == 0
    if n > 2:
        assert I[2] == Pn[2] == T[2] == per
    dice, iou, md, mu = PC.met_ref(I, Pn, T)
    tp, tt = torch.from_numpy(prob).view(n, 1, 1, per), torch.from_numpy(tgt).view(n, 1, 1, per)
    assert abs(float(md) - O.dice_coef(tp, tt)) <= 2e-7 and abs(float(mu) - O.iou_coef(tp, tt)) <= 2e-7
    pred = (tp > 0.5).float()
    i2, p2, t2 = (pred * tt).sum(dim=(1, 2, 3)), pred.sum(dim=(1, 2, 3)), tt.sum(dim=(1, 2, 3))
    assert np.array_equal(dice, ((2 * i2 + 1e-7) / (p2 + t2 + 1e-7)).numpy())            # test_seg_metrics_shapes_vs_oracle's spelling
    assert np.array_equal(iou, ((i2 + 1e-7) / (p2 + t2 - i2 + 1e-7)).numpy())
    # threshold equality is a miss, at every threshold
    for thr in PC.MET_THRESHOLDS:
        hit = prob > F(thr)
        assert not hit[prob == F(thr)].any()


def test_metric_logits_have_margin():
    lg = PC.met_logits(3, 257)
    assert (lg == 0).any() and set(np.unique(lg).tolist()) == {k / 2 for k in range(-8, 9)}
    s64 = 1.0 / (1.0 + np.exp(-lg.astype(np.float64)))
    for thr in PC.MET_THRESHOLDS:
        gap = np.abs(s64 - thr)
        assert (gap[lg != 0] > 1e-2).all()                 # expf's last bits cannot move any of them across a threshold
    with np.errstate(over="ignore"):
        assert (P.sigmoid_f32(np.zeros(1, F)) == F(0.5)).all()                           # exactly on 0.5: a miss under the strict >


def test_metric_grid_cases():
    """The launch geometry the shapes were chosen for, restated from vk_seg_metrics: bx = min(ceil(per / per_wg), ceil(4096 / n))."""
    def bx(n, per, vec):
        return max(1, min(-(-per // (256 * (16 if vec else 4))), -(-4096 // n)))
    assert bx(2048, 16384, True) == 2 < -(-16384 // 4096)                                   # the cap binds: 2 workgroups, not 4
    assert bx(4096, 1024, True) == 1 == -(-4096 // 4096)                                    # the cap at its floor of 1
    assert bx(2, 4096, True) == 1 and bx(2, 4096, False) == 4        # unaligned base: scalar loop over all 4096, four workgroups
    assert 65 > 64 and 130 > 128                                                            # finalize strides of 64: 2 and 3 trips
    t = PC.met_soft_targets(3, 257)
    assert set(np.unique(t).tolist()) == {k / 8 for k in range(9)}
