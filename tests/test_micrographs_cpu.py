"""The restatement of vk.micrographs (tests/micrographs_ref.py) proved on its own, without a GPU: the mask against exact rational
point-in-quadrilateral, the facets as a partition of the mask, the identities of the image model (empty scene, blur, whole-pixel shifts,
zero noise), the noise term's exact range and its mean, truth() by hand, the sampler's invariants and the two dataset conditions, the
overflow bound at the extreme admitted coordinates; then every argument error of the entry points through the built library.  No
tolerance appears: everything is equality or a derived bound."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import micrographs_cases as MC
import micrographs_ref as R


def _grid(S, pad=0):
    ys, xs = np.meshgrid(np.arange(-pad, S + pad, dtype=np.int64), np.arange(-pad, S + pad, dtype=np.int64), indexing="ij")
    return 16 * xs, 16 * ys


def _tri2(a, b, c):
    return abs((b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0]))


SMALL_QUADS = [
    ("lattice diamond: vertices on pixel centres, edges through pixel centres", MC.diamond(16 * 6, 16 * 6, 16 * 5), 14),
    ("vertex on the pixel centre (12, 6)", MC.diamond(16 * 6, 16 * 6, 16 * 6), 16),
    ("sixteenths", MC.indent((16 * 11 + 3, 16 * 5 + 9, 16 * 1 + 1, 16 * 6 - 7), (16 * 6 + 5, 16 * 12 - 2, 16 * 5, 16 * 1 + 11), 16 * 6, 16 * 6), 14),
    ("axis-aligned square: an edge along a pixel row", MC.indent((16 * 9, 16 * 9, 16 * 3, 16 * 3), (16 * 2, 16 * 8, 16 * 8, 16 * 2), 16 * 5, 16 * 6), 12),
    ("clipped by the frame", MC.indent((16 * 20, 16 * 30 + 7, 16 * 2 + 1, -16 * 6 - 5), (16 * 0, 16 * 12 + 3, 16 * 31, 16 * 14), 16 * 10, 16 * 13), 34),
]


# ------------------------------------------------------------------------------------------------ mask and facets
@pytest.mark.parametrize("case", SMALL_QUADS, ids=[c[0] for c in SMALL_QUADS])
def test_mask_is_exact_point_in_quadrilateral(case):
    """A pixel centre lies inside or on the quadrilateral iff the four triangles it spans with the edges add up to the quadrilateral:
    exact rationals, no orientation convention."""
    _, q, S = case
    X, Y = _grid(S)
    got = R.inside(q, X, Y)
    v = [(Fraction(int(q["vx"][i]), 16), Fraction(int(q["vy"][i]), 16)) for i in range(4)]
    area2 = _tri2(v[0], v[1], v[2]) + _tri2(v[0], v[2], v[3])
    n_edge = 0
    for y in range(S):
        for x in range(S):
            p = (Fraction(x), Fraction(y))
            parts = [_tri2(p, v[i], v[(i + 1) & 3]) for i in range(4)]
            assert bool(got[y, x]) == (sum(parts) == area2), (x, y)
            n_edge += bool(got[y, x]) and 0 in parts
    assert got.any() and not got.all()
    if "pixel cent" in case[0] or "pixel row" in case[0]:
        assert n_edge >= 4                                       # pixel centres exactly on the outline count as inside
    if "(12, 6)" in case[0]:
        assert got[6, 12] and not got[6, 13] and not got[5, 12]


@pytest.mark.parametrize("case", SMALL_QUADS, ids=[c[0] for c in SMALL_QUADS])
def test_facets_partition_the_mask(case):
    _, q, S = case
    X, Y = _grid(S, pad=3)
    f, n = R.facet_ids(q, X, Y)
    apex = (X == int(q["ax"])) & (Y == int(q["ay"]))
    assert (n[~apex] == 1).all() and (n[apex] == 0).all() and (f[apex] == 0).all()       # one wedge per point; the apex itself: facet 0
    s = MC.scene(S, [q], tex_amp=0)
    _, mask, facet = R.ideal(s, S)
    assert ((facet >= 0) == mask).all() and set(np.unique(facet[mask])) <= {0, 1, 2, 3}
    assert len(np.unique(facet[mask])) == 4
    # a point of facet i lies in the triangle apex, v_i, v_(i+1): exact areas
    a = (Fraction(int(q["ax"]), 16), Fraction(int(q["ay"]), 16))
    v = [(Fraction(int(q["vx"][i]), 16), Fraction(int(q["vy"][i]), 16)) for i in range(4)]
    ys, xs = np.nonzero(mask)
    for y, x in list(zip(ys, xs))[::3]:
        i = int(facet[y, x])
        p = (Fraction(int(x) - 3), Fraction(int(y) - 3))
        tri = (a, v[i], v[(i + 1) & 3])
        assert _tri2(p, tri[0], tri[1]) + _tri2(p, tri[1], tri[2]) + _tri2(p, tri[2], tri[0]) == _tri2(*tri)


def test_shade_runs_linearly_from_the_edge_to_the_apex():
    q = MC.indent((16 * 40, 16 * 20, 16 * 0, 16 * 20), (16 * 20, 16 * 40, 16 * 20, 16 * 0), 16 * 20, 16 * 20, shade=(100, 100, 100, 100), slope=(64, 64, 64, 64),
                  ridge=0, ridge_hw=0, halo_r=0)
    s = MC.scene(41, [q], tex_amp=0, vig=0, grad=(0, 0), tint=(256, 256, 256))
    img, mask, _ = R.ideal(s, 41, pad=0)
    assert img[20, 20, 0] == 100 + 64 and img[20, 40, 0] == 100 and img[0, 20, 0] == 100          # apex, two vertices
    assert img[20, 30, 0] == 100 + 32 and img[10, 20, 0] == 100 + 32                              # half way along two ridges
    assert img[25, 35, 0] == 100 and mask[25, 35] and not mask[25, 36]                            # on the edge x + y = 60


# ------------------------------------------------------------------------------------------------ identities of the image model
def test_empty_scene_is_the_base_colour():
    for base, tint in ((131, (256, 200, 300)), (0, (256, 256, 256)), (255, (1024, 0, 128)), (300, (256, 256, 256))):
        for S in (16, 21):
            rgb, mask = R.render_ref(R.blank_scene(base, tint), S)
            want = [min(255, max(0, (base * t + 128) >> 8)) for t in tint]
            assert (rgb == np.array(want, np.uint8)).all() and not mask.any() and rgb.shape == (S, S, 3)


def test_blur():
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (22, 30, 3)).astype(np.int64)
    assert np.array_equal(R.blur(img, 0), img[3:-3, 3:-3])
    for r in range(4):
        assert sum(R.BINOMIAL[r]) == 4 ** r and len(R.BINOMIAL[r]) == 2 * r + 1
        for v in (0, 1, 77, 255):
            assert (R.blur(np.full((20, 20, 3), v, np.int64), r) == v).all()
        out = R.blur(img, r)
        assert out.shape == (16, 24, 3) and out.min() >= 0 and out.max() <= 255
    # radius 1 by hand at one pixel
    p = img[9:12, 14:17, 1]
    assert R.blur(img, 1)[7, 12, 1] == (int((p * np.outer([1, 2, 1], [1, 2, 1])).sum()) + 8) >> 4


def _shifted(s, dx, dy):
    t = s.copy()
    for k in range(int(t["n_indents"])):
        t["indents"][k]["vx"] += 16 * dx; t["indents"][k]["vy"] += 16 * dy
        t["indents"][k]["ax"] += 16 * dx; t["indents"][k]["ay"] += 16 * dy
    for name in ("scratches", "blobs"):
        for k in range(int(t["n_" + name])):
            t[name][k]["x"] += 16 * dx; t[name][k]["y"] += 16 * dy
    for k in range(int(t["n_rects"])):
        for f, d in (("x0", dx), ("x1", dx), ("y0", dy), ("y1", dy)):
            t["rects"][k][f] += d
    for f, d in (("grad_cx", dx), ("vig_cx", dx), ("grad_cy", dy), ("vig_cy", dy)):
        t[f] += d
    return t


@pytest.mark.parametrize("blur_r", [0, 2, 3])
def test_whole_pixel_shift_of_every_record_shifts_the_image(blur_r):
    S = 48
    s = MC.full_scene(S, 11, blur_r=blur_r)
    s["tex_amp"], s["noise_amp"] = 0, 0
    a, ma = R.render_ref(s, S)
    assert ma.any() and len(np.unique(a)) > 50
    for dx, dy in ((5, 0), (-3, 7), (0, -9)):
        b, mb = R.render_ref(_shifted(s, dx, dy), S)
        ya, yb, xa, xb = max(0, -dy), min(S, S - dy), max(0, -dx), min(S, S - dx)
        assert np.array_equal(b[ya + dy:yb + dy, xa + dx:xb + dx], a[ya:yb, xa:xb]), (dx, dy)
        assert np.array_equal(mb[ya + dy:yb + dy, xa + dx:xb + dx], ma[ya:yb, xa:xb]), (dx, dy)


def test_noise_amplitude_zero_changes_nothing_and_noise_never_touches_the_mask():
    S = 40
    s = MC.full_scene(S, 2)
    quiet = s.copy()
    quiet["noise_amp"] = 0
    a, ma = R.render_ref(quiet, S)
    other = quiet.copy()
    other["noise_seed"] = 12345
    b, mb = R.render_ref(other, S)
    assert np.array_equal(a, b) and np.array_equal(ma, mb)
    c, mc = R.render_ref(s, S)
    assert np.array_equal(mc, ma) and not np.array_equal(c, a)
    t = R.noise_term(S, int(s["noise_seed"]))
    bound = (510 * int(s["noise_amp"]) + 128) >> 8
    assert np.abs(c.astype(np.int64) - a.astype(np.int64)).max() <= bound
    assert t.shape == (S, S, 3)


def test_noise_term_range_and_mean():
    """t is a sum of four bytes minus 510.  Four independent uniform bytes have variance 4 (256^2 - 1) / 12 = 21845 exactly, so the mean
    over the n = 512^2 values of one plane has standard deviation sqrt(21845 / n); the seed is fixed and the test deterministic."""
    assert R.NOISE_VAR == 21845 and Fraction(4 * (256 ** 2 - 1), 12) == 21845
    n = 512 * 512
    for seed in (0xC0FFEE, 0):
        t = R.noise_term(512, seed)
        assert t.min() >= -510 and t.max() <= 510
        for c in range(3):
            total = int(t[..., c].sum())
            print("noise plane", seed, c, "mean", total / n, "bound", 3.5 * (21845 / n) ** 0.5)
            assert total * total * n <= Fraction(49, 4) * 21845 * n * n          # |mean| <= 3.5 sigma / sqrt(n), in exact arithmetic
        assert len(np.unique(t)) > 700
    assert not np.array_equal(R.noise_term(64, 1), R.noise_term(64, 2))


def test_mix_is_the_32_bit_hash():
    def mix1(h):
        h &= 0xFFFFFFFF
        h ^= h >> 16; h = (h * 0x7feb352d) & 0xFFFFFFFF; h ^= h >> 15; h = (h * 0x846ca68b) & 0xFFFFFFFF; h ^= h >> 16
        return h
    vals = [0, 1, 2, 0xFFFFFFFF, 0x80000000, 123456789]
    assert [int(v) for v in R.mix(np.array(vals, np.uint64))] == [mix1(v) for v in vals]
    assert mix1(0) == 0 and mix1(1) != 1
    assert int(R.lattice(np.array([-1]), np.array([2]), 7)[0]) == mix1((0xFFFFFFFF * 0x9E3779B1 + 2 * 0x85EBCA77 + 7) & 0xFFFFFFFF) & 255


# ------------------------------------------------------------------------------------------------ truth
def test_truth_by_hand(vk):
    sq = MC.diamond(16 * 10, 16 * 12, 16 * 4)                        # lattice square on its corner: diagonals 8, area 32
    kite = MC.indent((16 * 30 + 8, 16 * 20, 16 * 14, 16 * 20), (16 * 20, 16 * 26 + 4, 16 * 20, 16 * 17), 16 * 22, 16 * 20)
    s = MC.scene(64, [sq, kite])
    for fn in (vk.micrographs.truth, R.truth_ref):
        t = fn(s)
        assert len(t) == 2
        assert t[0]["vertices"].tolist() == [[14.0, 12.0], [10.0, 16.0], [6.0, 12.0], [10.0, 8.0]]
        assert t[0]["d1"] == 8.0 and t[0]["d2"] == 8.0 and t[0]["d_mean"] == 8.0 and t[0]["area"] == 32.0 and t[0]["box"] == (6.0, 8.0, 14.0, 16.0)
        assert t[1]["vertices"].tolist() == [[30.5, 20.0], [20.0, 26.25], [14.0, 20.0], [20.0, 17.0]]
        assert t[1]["d1"] == 16.5 and t[1]["d2"] == 9.25 and t[1]["d_mean"] == 12.875 and t[1]["area"] == 0.5 * 16.5 * 9.25
        assert t[1]["box"] == (14.0, 17.0, 30.5, 26.25)
    assert vk.micrographs.truth(R.blank_scene()) == []


# ------------------------------------------------------------------------------------------------ sampler and dataset
def _boxes(s):
    return [(int(q["vx"].min()), int(q["vy"].min()), int(q["vx"].max()), int(q["vy"].max())) for q in s["indents"][:int(s["n_indents"])]]


def test_package_layouts_are_the_restatements(vk):
    M = vk.micrographs
    assert M.SCENE_DTYPE == R.SCENE_DT and M.INDENT_DTYPE == R.INDENT_DT and M.SCRATCH_DTYPE == R.SCRATCH_DT and M.BLOB_DTYPE == R.BLOB_DT
    assert M.RECT_DTYPE == R.RECT_DT and C.sizeof(vk._lib.vk_mg_scene) == R.SCENE_DT.itemsize == 3200
    assert (M.MAX_INDENTS, M.MAX_SCRATCHES, M.MAX_BLOBS, M.MAX_RECTS) == (R.MAX_INDENTS, R.MAX_SCRATCHES, R.MAX_BLOBS, R.MAX_RECTS) == (8, 64, 8, 4)
    assert (M.MIN_SIDE, M.MAX_SIDE, M.COORD_MARGIN) == (R.MIN_SIDE, R.MAX_SIDE, R.COORD_MARGIN) == (16, 1024, 8192)
    assert M.blank_scene(7, (1, 2, 3)).tobytes() == R.blank_scene(7, (1, 2, 3)).tobytes()
    for name in ("micrographs", "SceneSampler", "MicrographDataset"):
        assert name in vk.__all__ and hasattr(vk, name)
    L = vk.lib()
    assert hasattr(L, "vk_mg_render") and L.vk_mg_scenes_dev_bytes(3) == 9600 and L.vk_mg_scenes_dev_bytes(0) == 0


def test_built_cases_are_admitted(vk):
    seen = set()
    for name, S, scenes in MC.render_cases() + [("two", 128, [MC.two_indent_scene()])]:
        for s in scenes:
            for q in s["indents"][:int(s["n_indents"])]:
                assert vk.micrographs.quad_ok(q["vx"], q["vy"], q["ax"], q["ay"]), name
                assert min(q["vx"].min(), q["vy"].min()) >= -R.COORD_MARGIN and max(q["vx"].max(), q["vy"].max()) <= 16 * S + R.COORD_MARGIN
            seen.add((S, len(scenes), int(s["blur_r"])))
    assert {S for S, _, _ in seen} == {16, 20, 80, 128} and {n for _, n, _ in seen} == {1, 3} and {0, 3} <= {b for _, _, b in seen}
    full = MC.full_scene(80, 6)
    assert (int(full["n_indents"]), int(full["n_scratches"]), int(full["n_blobs"]), int(full["n_rects"])) == (8, 64, 8, 4)
    assert not vk.micrographs.quad_ok((0, 16, 0, -16), (16, 0, -16, 0), 0, 0)                  # counter-clockwise
    assert not vk.micrographs.quad_ok((16, 0, -16, 0), (0, 16, 0, -16), 16, 0)                 # the apex on a vertex


def test_sampler_invariants(vk):
    S = 256
    kw = dict(size=S, max_indents=5, margin=7, gap=4)
    sm = vk.SceneSampler(seed=5, **kw)
    counts = []
    for _ in range(150):
        s = sm.sample()
        n = int(s["n_indents"])
        counts.append(n)
        assert s.dtype == R.SCENE_DT and 1 <= n <= 5 and 8 <= int(s["n_scratches"]) <= 40 and 0 <= int(s["n_blobs"]) <= 4 and int(s["n_rects"]) <= 3
        assert 1 <= int(s["blur_r"]) <= 3 and 3 <= int(s["noise_amp"]) <= 9
        bx = _boxes(s)
        for q, b in zip(s["indents"][:n], bx):
            assert vk.micrographs.quad_ok(q["vx"], q["vy"], q["ax"], q["ay"])
            assert b[0] >= 16 * 7 and b[1] >= 16 * 7 and b[2] <= 16 * (S - 1 - 7) and b[3] <= 16 * (S - 1 - 7)
            d1, d2 = np.hypot(float(q["vx"][2] - q["vx"][0]), float(q["vy"][2] - q["vy"][0])), np.hypot(float(q["vx"][3] - q["vx"][1]), float(q["vy"][3] - q["vy"][1]))
            assert abs(d2 / d1 - 1.0) <= 0.04 + 4 * 0.02 + 0.01                                 # asymmetry of a few per cent, plus the jitter
        for i in range(n):
            for j in range(i):
                a, b = bx[i], bx[j]
                assert not (a[0] - 64 <= b[2] and b[0] <= a[2] + 64 and a[1] - 64 <= b[3] and b[1] <= a[3] + 64)
    assert max(counts) == 5 and min(counts) == 1
    a, b, c = vk.SceneSampler(seed=11, **kw), vk.SceneSampler(seed=11, **kw), vk.SceneSampler(seed=12, **kw)
    sa, sb, sc = [a.sample().tobytes() for _ in range(20)], [b.sample().tobytes() for _ in range(20)], [c.sample().tobytes() for _ in range(20)]
    assert sa == sb and sa != sc and len(set(sa)) == 20
    # the draw order does not depend on the outcome: a generator passed in is advanced, the sampler's own is not
    g = np.random.default_rng(3)
    first = a.sample(g).tobytes()
    assert a.sample(np.random.default_rng(3)).tobytes() == first and a.sample(g).tobytes() != first and a.sample().tobytes() == b.sample().tobytes()
    assert all(int(vk.SceneSampler(seed=1, size=64, p_empty=1.0).sample()["n_indents"]) == 0 for _ in range(5))
    for bad in (dict(size=15), dict(size=1025), dict(max_indents=0), dict(max_indents=9), dict(p_empty=1.5), dict(half_diag=(0.0, 0.1)), dict(half_diag=(0.2, 0.1)),
                dict(scratches=(0, 65)), dict(max_blobs=9), dict(tries=0), dict(margin=-1)):
        with pytest.raises(ValueError):
            vk.SceneSampler(**bad)


def test_default_scenes_have_the_foreground_of_the_real_masks_and_neighbours(vk):
    """Over the first 256 scenes of seed 0 at the defaults: every mask's foreground share lies in the range recorded for the real masks
    (0.11 % to 27 %), and more than half of the non-empty scenes hold at least two indentations.  The share is counted
    on the restatement's mask rule (pixel centres inside or on the outline); the sampler keeps the boxes apart, so the counts add."""
    sm = vk.SceneSampler(seed=0)
    S = sm.S
    assert S == 512
    shares, counts = [], []
    for _ in range(256):
        s = sm.sample()
        n = int(s["n_indents"])
        px = 0
        for q, b in zip(s["indents"][:n], _boxes(s)):
            xs = np.arange(max(0, b[0] // 16), min(S - 1, b[2] // 16 + 1) + 1, dtype=np.int64)
            ys = np.arange(max(0, b[1] // 16), min(S - 1, b[3] // 16 + 1) + 1, dtype=np.int64)
            px += int(R.inside(q, 16 * xs[None, :], 16 * ys[:, None]).sum())
        shares.append(Fraction(px, S * S))
        counts.append(n)
    print("foreground share: min %.4f %% max %.4f %%; scenes by count %s" % (100 * float(min(shares)), 100 * float(max(shares)), np.bincount(counts).tolist()))
    assert all(Fraction(11, 10000) <= f <= Fraction(27, 100) for f in shares)
    nonempty = [c for c in counts if c > 0]
    assert 2 * sum(c >= 2 for c in nonempty) > len(nonempty) > 0
    # the count on a box equals the count on the whole frame
    s = vk.SceneSampler(seed=0).sample()
    X, Y = _grid(S)
    assert sum(int(R.inside(q, X, Y).sum()) for q in s["indents"][:int(s["n_indents"])]) == int(shares[0] * S * S)


def test_dataset_items_do_not_depend_on_the_call_order(vk):
    ds = vk.MicrographDataset(50, size=128, seed=7, sampler_kwargs=dict(max_indents=2))
    order = [49, 0, 17, 3, 17, 0]
    a = {i: ds.scene(i).tobytes() for i in order}
    b = {i: ds.scene(i).tobytes() for i in reversed(order)}
    fresh = vk.MicrographDataset(50, size=128, seed=7, sampler_kwargs=dict(max_indents=2))
    assert a == b and all(fresh.scene(i).tobytes() == a[i] for i in a) and len(set(a.values())) == 4
    assert vk.MicrographDataset(50, size=128, seed=8, sampler_kwargs=dict(max_indents=2)).scene(3).tobytes() != a[3]
    want = vk.SceneSampler(size=128, max_indents=2).sample(np.random.default_rng([7, 17]))
    assert want.tobytes() == a[17]
    assert len(ds) == 50 and ds.names[17] == "mg000017" and len(ds.names) == 50
    t = ds.truth(17)
    assert len(t) == int(want["n_indents"]) and all(np.array_equal(x["vertices"], y["vertices"]) for x, y in zip(t, R.truth_ref(want)))
    for bad in (-1, 50):
        with pytest.raises(ValueError):
            ds.scene(bad)
    with pytest.raises(ValueError):
        vk.MicrographDataset(0)
    with pytest.raises(vk.VkError):
        vk.MicrographDataset(4, device="cpu")
    with pytest.raises(vk.VkError):
        vk.micrographs.render([R.blank_scene()], 16, device="cpu")


# ------------------------------------------------------------------------------------------------ overflow
def _worst_products(S):
    """Upper bounds of the int64 products of the formulas when every coordinate sits at an end of its admitted range."""
    lo, hi = -R.COORD_MARGIN, 16 * S + R.COORD_MARGIN
    p_lo, p_hi = 16 * (-R.APRON), 16 * (S - 1 + R.APRON)
    E = hi - lo                                   # a component of an edge or of apex-to-vertex
    Q = max(hi - p_lo, p_hi - lo)                 # a component of pixel minus record point
    cross = 2 * E * Q                             # |a.x b.y - a.y b.x|
    return dict(cross_sq=cross * cross, facet=256 * cross, ridge=32767 ** 2 * 2 * E * E, halo=32767 ** 2 * 2 * E * E, dist_sq=2 * Q * Q,
                scratch_cross_sq=(2 * Q * 16384) ** 2, scratch_lim=32767 ** 2 * 2 * 16384 ** 2, scratch_t=2 * Q * 16384)


def test_every_product_fits_int64_up_to_the_largest_side():
    w = _worst_products(R.MAX_SIDE)
    assert all(v < 2 ** 63 for v in w.values()), w
    assert w["scratch_t"] < 2 ** 31                          # the extent of a scratch is an int32 field
    assert _worst_products(2 * R.MAX_SIDE)["cross_sq"] >= 2 ** 63        # the next power of two does not fit: 1024 is the limit
    # the vignette and the level stay inside int32, which the kernel uses for them
    assert 255 * 2 * (R.MAX_SIDE + R.APRON + 512) ** 2 < 2 ** 31
    # the restatement evaluated at the extremes agrees with Python integers (no silent wrap in numpy's int64)
    S = R.MAX_SIDE
    lo, hi = -R.COORD_MARGIN, 16 * S + R.COORD_MARGIN
    q = MC.indent((lo, hi, hi, lo), (lo, lo, hi, hi), hi - 1, lo + 1, halo_r=32767, ridge_hw=32767)
    pts = [(-48, -48), (16 * (S + 2), -48), (-48, 16 * (S + 2)), (16 * (S + 2), 16 * (S + 2)), (16 * 500, 16 * 77)]
    X, Y = np.array([p[0] for p in pts], np.int64), np.array([p[1] for p in pts], np.int64)
    got = R.inside(q, X, Y)
    f, n = R.facet_ids(q, X, Y)
    for k, (x, y) in enumerate(pts):
        vx, vy, ax, ay = [int(v) for v in q["vx"]], [int(v) for v in q["vy"]], int(q["ax"]), int(q["ay"])
        cs = [(vx[(i + 1) & 3] - vx[i]) * (y - vy[i]) - (vy[(i + 1) & 3] - vy[i]) * (x - vx[i]) for i in range(4)]
        assert all(abs(c) ** 2 < 2 ** 63 for c in cs) and bool(got[k]) == all(c >= 0 for c in cs)
        ca = [(vx[i] - ax) * (y - ay) - (vy[i] - ay) * (x - ax) for i in range(4)]
        assert all(abs(c) ** 2 < 2 ** 63 for c in ca)
        assert [i for i in range(4) if ca[i] >= 0 and ca[(i + 1) & 3] < 0] == [int(f[k])] and n[k] == 1
    s = MC.scene(S, [q], [MC.scratch(hi, lo, 16384, -16384, 32767, 5)], tex_amp=0)
    img, mask, _ = R.ideal(s, 32, pad=3)                  # evaluates every formula with the extreme records on a corner of the frame
    assert mask.all() and img.shape == (38, 38, 3)


# ------------------------------------------------------------------------------------------------ argument errors
def _bufs():
    return dict(scenes_dev=np.full(3 * 800 + 8, 7, np.int32), rgb=np.full(3 * 16 * 16 * 3 + 8, 7, np.uint8), mask=np.full(3 * 16 * 16 + 8, 7, np.uint8))


def test_render_refuses_bad_arguments(vk):
    L = vk.lib()
    b = _bufs()
    good = np.stack([MC.scene(16, [MC.diamond(16 * 6, 16 * 6, 16 * 5)], [MC.scratch(40, 40, 16384, 0, 3, -30)], [np.array((100, 100, 40, 30), R.BLOB_DT)],
                              [MC.rect(1, 1, 5, 5, 1, (1, 2, 3))], blur_r=2, noise_amp=3) for _ in range(3)])

    def call(n=3, S=16, scenes=good, null=None, off=None, dev_bytes=None, edit=None):
        arr = np.ascontiguousarray(scenes.copy())
        if edit is not None:
            edit(arr)
        p = {k: (None if null == k else v.ctypes.data + (off[1] if off and off[0] == k else 0)) for k, v in b.items()}
        host = None if null == "scenes" else arr.ctypes.data + (off[1] if off and off[0] == "scenes" else 0)
        rc = L.vk_mg_render(n, S, host, p["scenes_dev"], 3 * 3200 if dev_bytes is None else dev_bytes, p["rgb"], p["mask"], None)
        assert all((v == 7).all() for v in b.values()), "a buffer was written"
        return rc, L.vk_last_error_string().decode()

    def ind(field, value, at=None, scene=1):
        def f(arr):
            if at is None:
                arr[scene]["indents"][0][field] = value
            else:
                arr[scene]["indents"][0][field][at] = value
        return f

    def top(field, value, scene=2):
        def f(arr):
            arr[scene][field] = value
        return f

    def rec(kind, field, value):
        def f(arr):
            arr[0][kind][0][field] = value
        return f

    def reverse(arr):
        arr[1]["indents"][0]["vx"] = arr[1]["indents"][0]["vx"][::-1].copy()
        arr[1]["indents"][0]["vy"] = arr[1]["indents"][0]["vy"][::-1].copy()

    def dent(arr):                       # vertex 2 pulled through the centre: not convex
        arr[1]["indents"][0]["vx"][2] = 16 * 8

    cases = [(dict(null="scenes"), "null buffer"), (dict(null="scenes_dev"), "null buffer"), (dict(null="rgb"), "null buffer"), (dict(null="mask"), "null buffer"),
             (dict(n=0), "batch 0"), (dict(n=-1), "batch -1"), (dict(n=65536), "batch 65536"), (dict(S=15), "S = 15"), (dict(S=1025), "S = 1025"),
             (dict(S=0), "S = 0"), (dict(dev_bytes=3 * 3200 - 1), "scene scratch"), (dict(dev_bytes=0), "scene scratch"),
             (dict(off=("scenes", 2)), "misaligned"), (dict(off=("scenes_dev", 2)), "misaligned"), (dict(off=("rgb", 1)), "misaligned"),
             (dict(off=("mask", 3)), "misaligned"),
             (dict(edit=top("n_indents", 9)), "scene 2: 9 indentations"), (dict(edit=top("n_indents", -1)), "scene 2: -1 indentations"),
             (dict(edit=top("n_scratches", 65)), "65 scratches"), (dict(edit=top("n_blobs", 9)), "9 blobs"), (dict(edit=top("n_rects", 5)), "5 rects"),
             (dict(edit=top("blur_r", 4)), "blur radius 4"), (dict(edit=top("blur_r", -1)), "blur radius -1"),
             (dict(edit=top("noise_amp", 256)), "noise amplitude 256"), (dict(edit=top("tint", (256, 1025, 256))), "tint"), (dict(edit=top("vig", 256)), "vignette"),
             (dict(edit=top("vig_cx", 16 + 513)), "vignette"), (dict(edit=top("grad_cy", -513)), "gradient"), (dict(edit=top("tex_lu", 9)), "texture"),
             (dict(edit=top("tex_cos", 16385)), "texture"),
             (dict(edit=ind("vx", 16 * 16 + 8193, 0)), "scene 1 indentation 0: vertex 0"), (dict(edit=ind("vy", -8193, 3)), "vertex 3"),
             (dict(edit=ind("vx", 2 ** 31 - 1, 1)), "vertex 1"), (dict(edit=reverse), "not convex and clockwise"), (dict(edit=dent), "not convex and clockwise"),
             (dict(edit=ind("ax", 16 * 12)), "apex"), (dict(edit=ind("ax", 16 * 11)), "apex"), (dict(edit=ind("ay", -2 ** 31)), "apex"),
             (dict(edit=ind("shade", 1025, 2)), "facet 2"), (dict(edit=ind("slope", -1025, 0)), "facet 0"), (dict(edit=ind("ridge_hw", 32768)), "ridge"),
             (dict(edit=ind("ridge_hw", -1)), "ridge"), (dict(edit=ind("halo_r", 15)), "halo"), (dict(edit=ind("halo_r", 32768)), "halo"),
             (dict(edit=rec("scratches", "x", -8193)), "scratch 0: point"), (dict(edit=rec("scratches", "dx", 16385)), "direction"),
             (dict(edit=lambda a: (rec("scratches", "dx", 0)(a), rec("scratches", "dy", 0)(a))), "direction (0, 0)"),
             (dict(edit=rec("scratches", "hw", 32768)), "half width"), (dict(edit=rec("scratches", "depth", 256)), "half width or depth"),
             (dict(edit=rec("blobs", "r", 15)), "blob 0: radius"), (dict(edit=rec("blobs", "y", 16 * 16 + 8193)), "blob 0: centre"),
             (dict(edit=rec("rects", "thickness", -1)), "rect 0: box"), (dict(edit=rec("rects", "x1", 4097)), "rect 0: box"),
             (dict(edit=rec("rects", "color", (0, 256, 0))), "rect 0: colour")]
    for kw, word in cases:
        rc, err = call(**kw)
        assert rc == -1 and word in err and "vk_mg_render" in err, (kw, err)
    # a record behind its count is not looked at: the error is that of the next bad thing
    def behind(arr):
        arr[0]["indents"][1]["vx"][0] = 2 ** 31 - 1
        arr[0]["blur_r"] = 7
    rc, err = call(edit=behind)
    assert rc == -1 and "blur radius 7" in err
    # a quadrilateral on the extreme admitted coordinates passes: the error is the later scene's
    lo, hi = -8192, 16 * 16 + 8192
    def extreme(arr):
        arr[1]["indents"][0]["vx"], arr[1]["indents"][0]["vy"] = (lo, hi, hi, lo), (lo, lo, hi, hi)
        arr[1]["indents"][0]["ax"], arr[1]["indents"][0]["ay"] = hi - 1, lo + 1
        arr[2]["blur_r"] = 5
    rc, err = call(edit=extreme)
    assert rc == -1 and "scene 2: blur radius 5" in err


def test_python_entry_points_refuse_wrong_arguments(vk):
    M = vk.micrographs
    with pytest.raises(ValueError):
        M._scene_array([])
    with pytest.raises(ValueError):
        M._scene_array(np.zeros(0, M.SCENE_DTYPE))
    arr = M._scene_array([R.blank_scene(), R.blank_scene(9)])
    assert arr.shape == (2,) and arr.dtype == M.SCENE_DTYPE and arr.flags.c_contiguous and int(arr[1]["base"]) == 9
    assert M._scene_array(np.zeros((), M.SCENE_DTYPE)).shape == (1,)
