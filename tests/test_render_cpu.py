"""The restatement of vk.render (tests/render_ref.py) proved on its own, without a GPU: segment coverage against exact rational
distances, the float32 blend against exact rational arithmetic, the label digits against "%.1f", the diagonal choice and the rank against
the reference's own expressions, the panels against train.py's expressions written directly in numpy; then the library's glyph table
and every argument error of the four entry points, which the library finds before it touches a stream."""
import ctypes as C
import itertools
import math
from fractions import Fraction

import numpy as np
import pytest

import render_cases as RC
import render_ref as R


# ------------------------------------------------------------------------------------------------ coverage
def _dist2(px, py, ax, ay, bx, by) -> Fraction:
    """The squared distance of P from the segment A-B, exactly."""
    dx, dy = bx - ax, by - ay
    L = dx * dx + dy * dy
    if L == 0:
        return Fraction((px - ax) ** 2 + (py - ay) ** 2)
    s = Fraction((px - ax) * dx + (py - ay) * dy, L)
    s = min(max(s, Fraction(0)), Fraction(1))
    qx, qy = ax + s * dx, ay + s * dy
    return (px - qx) ** 2 + (py - qy) ** 2


def test_coverage_is_the_exact_distance_test():
    """Every segment with end points in a 7 x 7 lattice (a sixth of the ordered pairs per thickness, all of them over the four
    thicknesses together), every pixel of the lattice and a border of two around it."""
    pts = [(x, y) for y in range(7) for x in range(7)]
    pairs = list(itertools.product(pts, pts))
    n = 0
    for t in (1, 2, 3, 8):
        lim = Fraction(t * t, 4)
        for k, (A, B) in enumerate(pairs):
            if t != 2 and k % 6 != t % 6:
                continue
            for py in range(-2, 9):
                for px in range(-2, 9):
                    assert R.seg_covers(px, py, A[0], A[1], B[0], B[1], t) == (_dist2(px, py, A[0], A[1], B[0], B[1]) <= lim), (t, A, B, px, py)
                    n += 1
    assert n > 400000


def test_coverage_at_the_ends_of_the_range():
    """Corners at +-2^20 with pixels in 0..16383: Python integers, so nothing to overflow; the rule is still the distance test."""
    Rm = R.MAX_COORD
    for A, B in (((-Rm, -Rm), (Rm, Rm)), ((Rm, -Rm), (-Rm, Rm)), ((-Rm, 7), (Rm, 8)), ((Rm, Rm), (Rm, Rm))):
        for P in ((0, 0), (16383, 16383), (5, 7), (16383, 0), (100, 101)):
            for t in (1, 8):
                assert R.seg_covers(P[0], P[1], A[0], A[1], B[0], B[1], t) == (_dist2(P[0], P[1], A[0], A[1], B[0], B[1]) <= Fraction(t * t, 4))


# ------------------------------------------------------------------------------------------------ blend
def test_blend_against_exact_arithmetic_at_the_defaults():
    """All 65,536 (base, overlay) byte pairs at alpha 1, beta 0.35: the float32 rule is the exact sequence of float32 roundings; a
    float64 evaluation differs from it on the tie columns only."""
    a = np.repeat(np.arange(256, dtype=np.uint8), 256)
    c = np.tile(np.arange(256, dtype=np.uint8), 256)
    got = R.blend(a, c, 1.0, 0.35).astype(int)
    b32 = Fraction(float(np.float32(0.35)))

    def rne(fr: Fraction) -> int:
        fl = math.floor(fr)
        rem = fr - fl
        return fl + (1 if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and fl % 2 == 1) else 0)

    def f32(fr: Fraction) -> Fraction:
        return Fraction(float(np.float32(float(fr))))                      # float(fr) is exact here: fr has at most 32 significant bits

    exact = np.empty(65536, int)
    q_by_c = [f32(Fraction(int(cc)) * b32) for cc in range(256)]
    for i in range(65536):
        s = f32(Fraction(int(a[i])) + q_by_c[int(c[i])])
        exact[i] = min(max(rne(s), 0), 255)
    assert np.array_equal(got, exact)
    f64 = np.clip(np.rint(a.astype(np.float64) * 1.0 + c.astype(np.float64) * 0.35), 0, 255).astype(int)
    diff = np.flatnonzero(got != f64)
    assert len(diff) == 4
    assert all(int(c[i]) % 20 == 10 for i in diff)                        # 0.35 c is k + 0.5 exactly in the rationals: the tie columns
    # fused and separate multiply-add agree at the defaults
    fused = np.array([min(max(rne(f32(Fraction(int(a[i])) + Fraction(int(c[i])) * b32)), 0), 255) for i in range(0, 65536, 7)])
    assert np.array_equal(fused, got[::7])


def test_blend_saturates_and_rounds_half_even():
    assert R.blend([250], [255], 1.0, 0.35).tolist() == [255]
    assert R.blend([10], [0], -1.0, 0.0).tolist() == [0]
    assert R.blend([1, 3, 5], [0, 0, 0], 0.5, 0.0).tolist() == [0, 2, 2]
    assert R.blend([7], [9], 1.0, 1.0, 0.5).tolist() == [16]


# ------------------------------------------------------------------------------------------------ label
def test_label_digits_equal_percent_one_f():
    rng = np.random.default_rng(11)
    vals = [float(v) for v in RC.D_MEANS if 0.0 <= v < 1.0e6] + [k / 20.0 for k in range(0, 40001)]
    vals += rng.uniform(0.0, 1.0e6, 150000).tolist() + rng.uniform(0.0, 100.0, 100000).tolist() + (10.0 ** rng.uniform(-12, 6, 50000)).tolist()
    vals += [float(np.nextafter(k / 20.0, s)) for k in range(1, 4001, 2) for s in (0.0, 1.0e9)]
    vals += [999999.94, 999999.95, float(np.nextafter(1.0e6, 0.0)), 5e-324, 1e-300]
    bad = [v for v in vals if v < 1.0e6 and R.label_digits_rule(v) != "%.1f" % v]
    assert not bad, bad[:5]
    assert R.label_digits_rule(0.35) == "0.3" and R.label_digits_rule(0.25) == "0.2" and "%d.%d" % divmod(int(np.rint(0.35 * 10)), 10) == "0.4"
    assert R.label_text(3, 0.35) == "#3 mean=0.3px" and R.label_text(12, 1.0e6) == "#12 mean=?px"
    for v in (-1.0, float("nan"), float("inf"), -1e-9):
        assert R.label_text(1, v) == "#1 mean=?px"
    assert len(R.label_text(4096, 999999.96)) <= R.LABEL_MAX and R.label_text(4096, 999999.96) == "#4096 mean=1000000.0px"
    assert set("".join(R.label_text(i, v) for i, v in ((1234567890, 0.5), (1, -1.0)))) <= set(R.GLYPHS)


# ------------------------------------------------------------------------------------------------ diagonals and rank
def _gui_diagonals(box):
    """ui_infer_rectangle.py:426-436 as it stands."""
    box = np.asarray(box).reshape(4, 2).astype(np.int32)
    pairs = []
    for i in range(4):
        for j in range(i + 1, 4):
            d = float(np.linalg.norm(box[i] - box[j]))
            pairs.append((d, i, j))
    pairs.sort(reverse=True, key=lambda x: x[0])
    _, i1, j1 = pairs[0]
    rest = [k for k in range(4) if k not in (i1, j1)]
    return i1, j1, rest[0], rest[1]


def test_integer_diagonals_are_the_guis_choice():
    rng = np.random.default_rng(12)
    boxes = [rng.integers(-R.MAX_COORD, R.MAX_COORD + 1, 8) for _ in range(3000)] + [rng.integers(-40, 41, 8) for _ in range(3000)]
    boxes += [rng.integers(0, 4, 8) for _ in range(3000)]                  # many exact ties
    boxes += [np.asarray(r, np.int64) for c in RC.prim_cases() if c.name == "special_rect" for r in c.recs["box"][0][:11]]
    ties = 0
    for b in boxes:
        # int32 differences of coordinates within +-2^20 do not overflow, as in the GUI
        assert R.diagonals(b) == _gui_diagonals(b), b
        d2 = sorted(((int(b[2 * i]) - int(b[2 * j])) ** 2 + (int(b[2 * i + 1]) - int(b[2 * j + 1])) ** 2 for i, j in R.PAIRS), reverse=True)
        ties += d2[0] == d2[1]
    assert ties > 500
    assert R.diagonals([10, 10, 50, 10, 50, 30, 10, 30]) == (0, 2, 1, 3)


def test_rank_is_the_stable_reverse_sort():
    rng = np.random.default_rng(13)
    for _ in range(200):
        M = int(rng.integers(1, 30))
        recs = RC._records("quad", np.zeros((1, M, 8)), rng.integers(0, 6, (1, M)), np.ones((1, M)), valid=rng.integers(0, 2, (1, M)))
        cnt = int(rng.integers(-2, M + 3))
        p, drawn, skipped = R.primitives_ref(recs, np.array([cnt]), R.COORD_BOX, "box")
        used = min(max(cnt, 0), M)
        dets = [dict(slot=t, area=int(recs[0, t]["area"])) for t in range(used) if recs[0, t]["valid"]]
        dets.sort(key=lambda x: x["area"], reverse=True)
        assert drawn[0] == len(dets) and skipped[0] == 0
        assert [int(v) for v in p[0, :len(dets)]["slot"]] == [d["slot"] for d in dets]
        assert [int(v) for v in p[0, :len(dets)]["rank"]] == list(range(len(dets)))


def test_prim_cases_hold_what_they_promise():
    for c in RC.prim_cases():
        p, drawn, skipped = R.primitives_ref(c.recs, c.counts, c.mode, c.field, c.affine, thickness=c.thickness, text_scale=c.text_scale)
        if c.name.startswith("special"):
            assert skipped[0] >= 3 and drawn[0] + skipped[0] == 12
            continue
        has_valid = "valid" in c.recs.dtype.names
        assert drawn.tolist() == ([0, 0, 9, 17] if has_valid else [0, 0, 11, 20]) and skipped.tolist() == [0, 0, 0, 0]
        texts = {int(r["slot"]): bytes(r["label"][:r["label_len"]]).decode() for r in p[3, :drawn[3]]}
        unknown = {t for t, v in enumerate(RC.D_MEANS) if not 0.0 <= v < 1.0e6}
        assert {t for t, s in texts.items() if "?" in s} == {t for t in unknown if t in texts} and len(unknown) == 4
        assert texts[1].endswith("mean=0.2px") and texts[5].endswith("mean=999999.9px")
        assert all(texts[t].endswith("mean=%.1fpx" % RC.D_MEANS[t]) for t in texts if t < len(RC.D_MEANS) and t not in unknown)
        assert all(tuple(r["color"]) == R.PALETTE[k % 8] for k, r in enumerate(p[3, :drawn[3]]))
    sp = [c for c in RC.prim_cases() if c.name == "special_rect"][0]
    p, drawn, _ = R.primitives_ref(sp.recs, sp.counts, sp.mode, sp.field)
    by_slot = {int(r["slot"]): r for r in p[0, :drawn[0]]}
    assert set(by_slot) == {0, 1, 2, 3, 4, 5, 6, 8}                       # 7, 9, 10 (a NaN centre) and 11 are skipped
    assert tuple(by_slot[2]["diag"]) == (0, 2, 1, 3) and tuple(by_slot[0]["diag"]) == (0, 1, 2, 3) and tuple(by_slot[4]["diag"]) == (0, 1, 2, 3)
    assert tuple(by_slot[5]["anchor"]) == (-3 + 6, -2 - 6)                  # (int)-3.5 = -3


# ------------------------------------------------------------------------------------------------ panels
def test_panels_are_the_references_expressions():
    """train.py:317-345 written directly in numpy, cv2.addWeighted replaced by its documented formula, on random inputs (where no value
    is a NaN or leaves what astype(np.uint8) defines)."""
    rng = np.random.default_rng(14)
    N, H, W = 2, 6, 9
    x = rng.normal(0, 1.3, (N, 3, H, W)).astype(np.float32)
    y = (rng.random((N, 1, H, W)) > 0.5).astype(np.float32)
    pr = rng.random((N, 1, H, W)).astype(np.float32)
    x_np = np.transpose(x, (0, 2, 3, 1))
    x_np = (x_np * np.array([0.229, 0.224, 0.225]) + np.array([0.485, 0.456, 0.406])) * 255.0
    x_np = np.clip(x_np, 0, 255).astype(np.uint8)
    y_np = (y.squeeze(1) * 255).astype(np.uint8)
    pr_np = (pr.squeeze(1) * 255).astype(np.uint8)
    got = R.val_panels_ref(x, y, pr)
    for i in range(N):
        rgb = x_np[i][:, :, ::-1]
        color = np.zeros_like(rgb)
        color[pr_np[i] > 127] = (0, 140, 255)
        s = (rgb.astype(np.float32) * np.float32(1.0) + color.astype(np.float32) * np.float32(0.35)) + np.float32(0.0)
        vis = np.clip(np.rint(s), 0, 255).astype(np.uint8)
        canvas = np.hstack([rgb, np.repeat(y_np[i][..., None], 3, 2), np.repeat(pr_np[i][..., None], 3, 2), vis])
        assert np.array_equal(got[i].reshape(H, 4 * W, 3), canvas)
    assert np.array_equal(R.val_panels_ref(x, y, pr, rgb=True).reshape(N, H, 4 * W, 3), got.reshape(N, H, 4 * W, 3)[..., ::-1])


def test_panel_cases_hold_what_they_promise():
    for c in RC.panel_cases():
        N, _, H, W = c.x.shape
        out = R.val_panels_ref(c.x, c.y, c.prob, color=c.color).reshape(N, H, 4 * W, 3)
        if c.name == "1x1":
            continue
        for k in range(3):
            flat = out[0, :, :W, 2 - k].reshape(-1)
            assert flat[:10].tolist() == [1, 0, 77, 76, 128, 127, 254, 253, 255, 254], (c.name, k, flat[:10])
            assert flat[12:17].tolist() == [0, 255, 0, 255, 0]                 # -5, 9, NaN, inf, -inf
        pd = out[0, :, 2 * W:3 * W, 0].reshape(-1)
        us = np.roll(RC._unit_specials(), 3)
        assert pd[:len(us)].tolist() == R.unit_to_u8(us).tolist() and {127, 128, 0, 255} <= set(pd[:len(us)].tolist())
    assert R.unit_to_u8(np.array([127, 128], np.float32) / np.float32(255)).tolist() == [127, 128]


def test_draw_and_reduce_properties():
    """An empty list is the overlay; the last record wins; reduce with k = 1 is the identity and a block mean otherwise."""
    c = [d for d in RC.draw_cases() if d.name == "40x70_u8"][0]
    vo, vb, vv = R.draw_ref(c.src, c.mask, c.thresh, c.color, 1.0, c.alpha)
    lay = np.zeros_like(c.src)
    lay[c.mask > 0] = c.color
    assert np.array_equal(vo, c.src) and np.array_equal(vv, R.blend(c.src, lay, 1.0, c.alpha)) and set(np.unique(vb)) <= {0, 255}
    do, db, dv = R.draw_ref(c.src, c.mask, c.thresh, c.color, 1.0, c.alpha, prims=c.prims, drawn=c.drawn)
    changed = (do != vo).any(axis=2)
    assert changed.sum() > 300 and np.array_equal(do[changed], db[changed]) and np.array_equal(do[changed], dv[changed])
    # list order: the pixels of the last record that lies inside keep its colours
    last = [p for p in c.prims[:c.drawn] if R.prim_ok(p)][-1]
    layer = R.prim_paint(last, 40, 70)
    assert (layer >= 0).sum() > 50 and np.array_equal(do[layer == 0], np.broadcast_to(last["color"], do[layer == 0].shape))
    for d in RC.draw_cases():                                              # the float64 pre-filter of the restatement loses no pixel
        for p in ([] if d.prims is None else d.prims[:max(d.drawn, 0)]):
            h, w = d.src.shape[:2]
            assert np.array_equal(R.prim_paint(p, h, w), R.prim_paint(p, h, w, prefilter=False))
    img = RC.reduce_images()[2]
    assert np.array_equal(R.reduce_ref(img, 1), img)
    r = R.reduce_ref(img, 16)
    assert r.shape == (3, 5, 3) and r[0, 0].tolist() == ((img[:16, :16].astype(int).reshape(-1, 3).sum(0) + 128) // 256).tolist()
    assert r[2, 4].tolist() == ((img[32:, 64:].astype(int).reshape(-1, 3).sum(0) + 3) // 6).tolist()


# ------------------------------------------------------------------------------------------------ the library without a GPU
def test_glyph_table_and_exports(vk):
    L = vk.lib()
    for name in ("vk_render_val_panels", "vk_render_primitives", "vk_render_draw", "vk_render_reduce", "vk_render_glyph"):
        assert hasattr(L, name) and name in vk._lib.SIGNATURES
    assert "render" in vk.__all__ and hasattr(vk.Segmenter, "render")
    assert set(vk._lib.RENDER_CHARS) == set(R.GLYPHS)
    for ch, rows in R.GLYPHS.items():
        assert vk.render.glyph(ch) == rows, ch
    rows = (C.c_uint8 * 7)()
    for ch in "AMPX-,:+":
        assert L.vk_render_glyph(ord(ch), rows) == -1 and "no glyph" in L.vk_last_error_string().decode()
    assert L.vk_render_glyph(ord("0"), None) == -1
    assert vk.render.PALETTE == R.PALETTE and vk.render.DIAG_COLOR == R.DIAG_COLOR
    assert vk._lib.VK_RENDER_MAX_COORD == R.MAX_COORD and vk._lib.VK_RENDER_LABEL_MAX == R.LABEL_MAX
    assert (vk._lib.VK_RENDER_COORD_BOX, vk._lib.VK_RENDER_COORD_V, vk._lib.VK_RENDER_COORD_VS) == (R.COORD_BOX, R.COORD_V, R.COORD_VS)


def test_prim_dtype_is_derived_from_the_structure(vk):
    assert C.sizeof(vk._lib.vk_render_prim) == 104 and C.sizeof(vk._lib.vk_render_blend) == 16 and C.sizeof(vk._lib.vk_render_style) == 36
    assert C.sizeof(vk._lib.vk_render_view) == 88
    dt = vk.render.PRIM_DTYPE
    assert dt.itemsize == R.PRIM_DT.itemsize and dt.names == R.PRIM_DT.names
    for n in dt.names:
        assert dt.fields[n][1] == R.PRIM_DT.fields[n][1] and dt.fields[n][0] == R.PRIM_DT.fields[n][0], n


def _bufs():
    return dict(x=np.full(4096, 7, np.float32), y=np.full(4096, 7, np.float32), pr=np.full(4096, 7, np.float32), out=np.full(8192, 7, np.uint8),
                recs=np.full(3 * 4 * 104 // 8, 7, np.int64), counts=np.full(4, 7, np.int32), aff=np.full(16, 7.0, np.float64),
                prims=np.full(3 * 4 * 13, 7, np.int64), drawn=np.full(4, 7, np.int32), skipped=np.full(4, 7, np.int32),
                views=np.full(64, 7, np.int64), src=np.full(4096, 7, np.uint8), dst=np.full(4096, 7, np.uint8))


def _untouched(b):
    return all((v == 7).all() for v in b.values())


def _ptr(b, names, null, off):
    return {k: (None if null == k else b[k].ctypes.data + (off[1] if off and off[0] == k else 0)) for k in names}


def test_val_panels_refuses_bad_arguments(vk):
    L = vk.lib()
    b = _bufs()

    def call(N=2, H=5, W=7, stride=84, flags=0, alpha=1.0, mean=(0.5, 0.5, 0.5), null=None, off=None):
        p = _ptr(b, ("x", "y", "pr", "out"), null, off)
        bl = vk._lib.vk_render_blend((C.c_uint8 * 3)(0, 140, 255), 0, alpha, 0.35, 0.0)
        rc = L.vk_render_val_panels(N, H, W, p["x"], p["y"], p["pr"], None if null == "mean" else (C.c_double * 3)(*mean), (C.c_double * 3)(1, 1, 1),
                                    None if null == "blend" else C.byref(bl), flags, p["out"], stride, None)
        assert _untouched(b)
        return rc, L.vk_last_error_string().decode()

    for kw, word in ((dict(N=0), "N = 0"), (dict(N=65536), "N = 65536"), (dict(H=0), "size"), (dict(W=16385), "size"), (dict(stride=83), "row stride"),
                     (dict(stride=2 ** 31 + 1), "row stride"), (dict(flags=2), "unknown flags"), (dict(alpha=float("nan")), "blend weights"),
                     (dict(alpha=float("inf")), "blend weights"), (dict(mean=(0.5, float("nan"), 0.5)), "not finite"), (dict(null="x"), "null buffer"),
                     (dict(null="y"), "null buffer"), (dict(null="pr"), "null buffer"), (dict(null="out"), "null buffer"), (dict(null="mean"), "null buffer"),
                     (dict(null="blend"), "null blend"), (dict(off=("x", 2)), "misaligned"), (dict(off=("pr", 1)), "misaligned")):
        rc, err = call(**kw)
        assert rc == -1 and word in err, (kw, err)


def test_primitives_refuses_bad_arguments(vk):
    L = vk.lib()
    b = _bufs()

    def call(batch=3, stride=104, box=8, valid=48, diag=96, center=40, mode=0, M=4, thickness=2, text_scale=2, null=None, off=None):
        p = _ptr(b, ("recs", "counts", "aff", "prims", "drawn", "skipped"), null, off)
        st = vk._lib.vk_render_style()
        st.thickness, st.text_scale = thickness, text_scale
        rc = L.vk_render_primitives(batch, p["recs"], stride, box, valid, diag, center, mode, p["counts"], M, p["aff"],
                                    None if null == "style" else C.byref(st), p["prims"], p["drawn"], p["skipped"], None)
        assert _untouched(b)
        return rc, L.vk_last_error_string().decode()

    for kw, word in ((dict(batch=0), "batch"), (dict(batch=65536), "batch"), (dict(M=0), "max_components"), (dict(M=4097), "max_components"),
                     (dict(mode=3), "coordinate mode"), (dict(mode=-1), "coordinate mode"), (dict(stride=100), "record stride"),
                     (dict(box=4), "record stride"), (dict(box=80), "record stride"), (dict(box=10), "record stride"),
                     (dict(mode=1, box=44), "record stride"), (dict(mode=2, box=48), "record stride"), (dict(valid=4), "valid offset"),
                     (dict(valid=104), "valid offset"), (dict(valid=50), "valid offset"), (dict(diag=100), "diag offset"), (dict(diag=0), "diag offset"),
                     (dict(diag=104), "diag offset"), (dict(center=-1), "center offset"), (dict(center=100), "center offset"),
                     (dict(thickness=0), "thickness"), (dict(thickness=9), "thickness"), (dict(text_scale=0), "text_scale"),
                     (dict(text_scale=9), "text_scale"), (dict(null="recs"), "null buffer"), (dict(null="counts"), "null buffer"),
                     (dict(null="style"), "null buffer"), (dict(null="prims"), "null buffer"), (dict(null="drawn"), "null buffer"),
                     (dict(null="skipped"), "null buffer"), (dict(off=("recs", 4)), "misaligned"), (dict(off=("counts", 2)), "misaligned"),
                     (dict(off=("aff", 4)), "misaligned"), (dict(off=("prims", 4)), "misaligned"), (dict(off=("skipped", 1)), "misaligned")):
        rc, err = call(**kw)
        assert rc == -1 and word in err, (kw, err)
    # the modes that do not read the centre accept any centre offset: the check that follows them is reached (a null buffer)
    rc, err = call(mode=2, box=16, valid=8, diag=96, center=-1, null="recs")
    assert rc == -1 and "null buffer" in err


def test_draw_refuses_bad_arguments(vk):
    L = vk.lib()
    b = _bufs()

    def call(batch=1, kind=0, thresh=0.5, flags=0, M=4, alpha=1.0, view=None, prims=True, null=None, off=None):
        p = _ptr(b, ("views", "prims", "drawn"), null, off)
        v = dict(src=4096, src_stride=21, mask=8192, mask_stride=7 if kind == 0 else 28, out=(256, 512, 1024), out_stride=(21, 21, 21), h=5, w=7)
        v.update(view or {})
        tab = vk._lib.vk_render_view(v["src"], v["src_stride"], v["mask"], v["mask_stride"], (C.c_uint64 * 3)(*v["out"]),
                                     (C.c_int64 * 3)(*v["out_stride"]), v["h"], v["w"])
        bl = vk._lib.vk_render_blend((C.c_uint8 * 3)(0, 0, 255), 0, alpha, 0.35, 0.0)
        rc = L.vk_render_draw(batch, None if null == "tab" else C.byref(tab), p["views"], kind, thresh, None if null == "blend" else C.byref(bl),
                              p["prims"] if prims else None, p["drawn"], M, flags, None)
        assert _untouched(b)
        return rc, L.vk_last_error_string().decode()

    for kw, word in ((dict(batch=0), "batch"), (dict(batch=65536), "batch"), (dict(null="tab"), "null buffer"), (dict(null="views"), "null buffer"),
                     (dict(off=("views", 4)), "misaligned"), (dict(kind=2), "mask kind"), (dict(kind=1, thresh=float("nan")), "thresh"),
                     (dict(null="blend"), "null blend"), (dict(alpha=float("nan")), "blend weights"), (dict(flags=2), "unknown flags"),
                     (dict(null="drawn"), "null buffer"), (dict(M=0), "max_components"), (dict(M=4097), "max_components"),
                     (dict(off=("prims", 4)), "misaligned"), (dict(off=("drawn", 2)), "misaligned"), (dict(view=dict(h=0)), "size"),
                     (dict(view=dict(w=16385, src_stride=3 * 16385)), "size"), (dict(view=dict(src=0)), "null address"),
                     (dict(view=dict(mask=0)), "null address"), (dict(view=dict(src_stride=20)), "row stride"),
                     (dict(view=dict(mask_stride=6)), "mask row stride"), (dict(kind=1, view=dict(mask_stride=27)), "mask row stride"),
                     (dict(kind=1, view=dict(mask_stride=30)), "mask row stride"), (dict(kind=1, view=dict(mask=8194)), "mask row stride"),
                     (dict(view=dict(out_stride=(21, 20, 21))), "output 1"), (dict(view=dict(out=(0, 0, 0))), "no output")):
        rc, err = call(**kw)
        assert rc == -1 and word in err, (kw, err)


def test_reduce_refuses_bad_arguments(vk):
    L = vk.lib()
    b = _bufs()

    def call(h=5, w=7, k=2, sstride=21, dstride=12, null=None):
        p = _ptr(b, ("src", "dst"), null, None)
        rc = L.vk_render_reduce(h, w, k, p["src"], sstride, p["dst"], dstride, None)
        assert _untouched(b)
        return rc, L.vk_last_error_string().decode()

    for kw, word in ((dict(h=0), "size"), (dict(w=0), "size"), (dict(h=16385), "size"), (dict(k=0), "k = 0"), (dict(k=17), "k = 17"),
                     (dict(sstride=20), "source row stride"), (dict(dstride=11), "output row stride"), (dict(null="src"), "null buffer"),
                     (dict(null="dst"), "null buffer")):
        rc, err = call(**kw)
        assert rc == -1 and word in err, (kw, err)


def test_python_entry_points_refuse_wrong_arguments(vk):
    import torch
    Rn = vk.render
    dets = vk.geometry.Detections("rect", None, torch.zeros(1, 2, 96, dtype=torch.uint8), torch.zeros(1, dtype=torch.int32), None, 2)
    with pytest.raises(vk.VkError, match="no CPU fallback"):
        Rn.primitives(dets)
    with pytest.raises(ValueError, match="coords"):
        Rn.primitives(dets, coords="vs")
    with pytest.raises(ValueError, match="Detections"):
        Rn.primitives("no")
    with pytest.raises(vk.VkError, match="no CPU fallback"):
        Rn.val_panels(torch.zeros(1, 3, 4, 4), torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 4))
    with pytest.raises(ValueError, match="order"):
        Rn.val_panels(torch.zeros(1, 3, 4, 4), torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 4), order="gbr")
    with pytest.raises(ValueError, match="prob"):
        Rn.val_panels(torch.zeros(1, 3, 4, 4), torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4, 5))
    with pytest.raises(ValueError, match="colour"):
        Rn._blend((0, 0, 256), 1.0, 0.35)
    with pytest.raises(ValueError, match="palette"):
        Rn._style(((0, 0, 0),) * 7, (0, 0, 255), 2, 2)
