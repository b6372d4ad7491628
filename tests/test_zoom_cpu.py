"""The restatement of vk.zoom (tests/zoom_ref.py) proved on its own, without a GPU: the gather against the properties the resampling
rule promises, the windows against values worked out by hand, the merge against built tables, the whole chain against analytic truth
on rendered squares; then every argument error of the three entry points, which the library finds before it touches a stream."""
import ctypes as C
import math

import numpy as np
import pytest

import subpix_ref as SR
import zoom_cases as ZC
import zoom_ref as Z

U = 2.0 ** -53                   # unit roundoff of float64


# ------------------------------------------------------------------------------------------------ gather
@pytest.mark.parametrize("s", [0.25, 0.5, 1.0, 1.75, 2.0, 3.5, 8.0, 63.9])
def test_weights_sum_to_f(s):
    """In exact arithmetic the weights of an axis telescope to b - a.  Every weight is one subtraction of numbers that min / max pick
    exactly (error <= U * weight <= U), the T-term running sum adds <= (T - 1) * U * f, and b = fl(a + f) is off by <= U * |b|."""
    f = max(s, 1.0)
    for O in (0.0, 0.37, -17.25, 1000.5, 1.0e6 + 1.0 / 3.0):
        a, b, i0, i1 = Z.axis_spans(O, 33, s, f)
        idx, wt = Z.axis_weights(a, b, i0, i1)
        assert (wt >= 0.0).all() and (wt <= 1.0).all() and (i1 - i0 <= math.ceil(f) + 1).all()
        for x in range(33):
            T = int(i1[x] - i0[x]) + 1
            tot = 0.0
            for t in range(T):
                tot = tot + float(wt[t, x])
            assert abs(tot - f) <= U * (T + (T - 1) * f + abs(float(b[x]))), (s, O, x)
            assert (wt[T:, x] == 0.0).all() and not np.signbit(wt[T:, x]).any()


def test_constant_image_gives_the_constant():
    img = np.full((37, 53, 3), 0, np.uint8)
    img[:] = (17, 130, 251)
    for s in ZC.GATHER_SCALES:
        S = 9
        X0, Y0 = 1.3, 2.7                                              # the window stays inside the image up to s = 3.5
        if X0 + S * s > 53 or Y0 + S * s > 37:
            continue
        v = Z.gather_one(img, X0, Y0, s, S)
        assert np.array_equal(np.rint(v), np.broadcast_to(np.array([17.0, 130.0, 251.0]), v.shape)), s
        assert np.abs(v - np.array([17.0, 130.0, 251.0])).max() <= 255.0 * 64 * U * max(s, 1.0) ** 2


def test_scale_one_integer_origin_is_the_source():
    img = ZC.gather_images()[2]
    v = Z.gather_one(img, 5.0, 3.0, 1.0, 16)
    assert np.array_equal(v, img[3:19, 5:21].astype(np.float64))
    # and through the quantisation and normalisation: the bits of the letterbox expression for that byte
    out = Z.gather_ref([img], np.array([(0, 0, 0, 0, 5.0, 3.0, 1.0)], Z.WINDOW_DT), 1, 16)[0]
    from oracle import prepost_oracle as PO
    assert out.tobytes() == PO.normalise_nchw(img[3:19, 5:21]).tobytes()


@pytest.mark.parametrize("s", [0.25, 0.5, 0.8, 1.0])
def test_small_scales_are_bilinear(s):
    img = ZC.gather_images()[2].astype(np.float64)
    X0, Y0, S = 3.3, 4.15, 12
    v = Z.gather_one(ZC.gather_images()[2], X0, Y0, s, S)
    for y in range(S):
        for x in range(S):
            u, w = X0 + (x + 0.5) * s - 0.5, Y0 + (y + 0.5) * s - 0.5
            i, j = math.floor(u), math.floor(w)
            fx, fy = u - i, w - j
            exp = (img[j, i] * (1 - fx) + img[j, i + 1] * fx) * (1 - fy) + (img[j + 1, i] * (1 - fx) + img[j + 1, i + 1] * fx) * fy
            # a handful of roundings of numbers <= 255 on either side
            assert np.abs(v[y, x] - exp).max() <= 255.0 * 32 * U, (s, x, y)


@pytest.mark.parametrize("s", [2, 3, 4])
def test_integer_scales_are_block_means(s):
    img = ZC.gather_images()[3]
    S, X0, Y0 = 8, 7, 5
    v = Z.gather_one(img, float(X0), float(Y0), float(s), S)
    blocks = img[Y0:Y0 + S * s, X0:X0 + S * s].astype(np.int64).reshape(S, s, S, s, 3).sum(axis=(1, 3))
    assert np.array_equal(v, blocks.astype(np.float64) / float(s * s))       # integer sums below 2^53 are exact in float64


def _supersampled(img, X0, Y0, s, x, y, ss=16):
    f = max(s, 1.0)
    ax, ay = X0 + (x + 0.5) * s - f / 2, Y0 + (y + 0.5) * s - f / 2
    off = (np.arange(ss) + 0.5) / ss * f
    ii = np.floor(ax + off).astype(int)
    jj = np.floor(ay + off).astype(int)
    return img[np.ix_(jj, ii)].astype(np.float64).mean(axis=(0, 1))


@pytest.mark.parametrize("s,X0,Y0", [(1.75, 3.21, 2.9), (3.5, 1.13, 0.77), (2.6, 4.5, 3.25), (1.0, 2.4, 6.6), (0.5, 5.31, 7.77)])
def test_fractional_windows_against_supersampling(s, X0, Y0):
    """Midpoint sampling of a piecewise-constant function on a 16-point grid per axis errs only in the cells a pixel boundary cuts:
    per boundary at most half a cell, (f / 32) of the length f, times the jump across it.  With at most nb = ceil(f) + 1 boundaries
    per axis and jumps <= J the error of the mean is <= 2 * nb * J / 32.  J = 255 for random bytes; the ramp image has J = 3."""
    S = 6
    f = max(s, 1.0)
    nb = math.ceil(f) + 1
    yy, xx = np.mgrid[0:64, 0:96]
    ramp = (np.stack([2 * xx + yy, xx + 3 * yy, (3 * xx + 2 * yy) // 2], axis=2) // 3).astype(np.uint8)
    J_ramp = int(max(np.abs(np.diff(ramp.astype(int), axis=0)).max(), np.abs(np.diff(ramp.astype(int), axis=1)).max()))
    assert J_ramp <= 3
    for img, J in ((ZC.gather_images()[3], 255), (ramp, J_ramp)):
        v = Z.gather_one(img, X0, Y0, s, S)
        for y in range(S):
            for x in range(S):
                exp = _supersampled(img, X0, Y0, s, x, y)
                assert np.abs(v[y, x] - exp).max() <= 2.0 * nb * J / 32.0 + 1e-9, (s, x, y, v[y, x], exp)
                scalar, _, _ = Z.gather_pixel_scalar(img, X0, Y0, s, x, y)
                assert v[y, x].tolist() == scalar                          # the vectorised form is the scalar rule, bit for bit


def test_vectorised_gather_is_the_scalar_rule_at_the_borders():
    """Windows that leave the image on every side, with a pad value: the two forms of the restatement give the same bits."""
    img = ZC.gather_images()[1]                                            # 5 x 7
    for s, X0, Y0 in ((0.5, -1.3, -0.8), (1.0, -2.0, 3.0), (1.75, 2.2, -3.1), (3.5, -4.0, -5.5), (8.0, -20.0, -9.0)):
        v = Z.gather_one(img, X0, Y0, s, 5, pad=114)
        for y in range(5):
            for x in range(5):
                assert v[y, x].tolist() == Z.gather_pixel_scalar(img, X0, Y0, s, x, y, pad=114)[0], (s, x, y)
    far = Z.gather_one(img, 50.0, 50.0, 2.0, 4, pad=114)
    assert np.array_equal(np.rint(far), np.full((4, 4, 3), 114.0))


def test_invalid_windows_give_the_pad_value():
    S = 8
    win = ZC.gather_windows(S)
    imgs = ZC.gather_images()
    bad = [k for k in range(len(win)) if not Z.window_ok(win[k], len(imgs))]
    assert len(bad) == 8
    out = Z.gather_ref(imgs, win[bad], len(bad), S, pad=114)
    pad = Z.quantise_normalise(np.full((1, 3), 114.0))[:, 0]
    assert all((out[:, k] == pad[k]).all() for k in range(3))


# ------------------------------------------------------------------------------------------------ windows
def test_windows_by_hand():
    p = Z.params(S=64)
    # axis-aligned square, half side 20, centre (150, 100): e = 20, s = 1.5 * 40 / 64 = 0.9375 -> clamped to 1; X0 = 150.5 - 32
    st, X0, Y0, s = Z.window_of(ZC._sq(150, 100, 20), (0.0, 0.0, 1.0), (200, 300), p)
    assert (st, X0, Y0, s) == (Z.SCALE_CLAMPED_LO, 118.5, 68.5, 1.0)
    # half side 40: s = 1.5 * 80 / 64 = 1.875, the window spans 120 source pixels around (160.5, 120.5)
    st, X0, Y0, s = Z.window_of(ZC._sq(160, 120, 40), (0.0, 0.0, 1.0), (240, 320), p)
    assert (st, X0, Y0, s) == (0, 100.5, 60.5, 1.875)
    # the same square turned by 45 degrees (corners on the axes at distance 40) fills the same window
    st, X0, Y0, s = Z.window_of([100, 60, 140, 100, 100, 140, 60, 100], (0.0, 0.0, 1.0), (200, 300), p)
    assert (st, X0, Y0, s) == (0, 100.5 - 60.0, 100.5 - 60.0, 1.875)
    # through a letterbox row: map corners (52..76, 52..76), 16 rows of border, 8 source pixels per map pixel
    st, X0, Y0, s = Z.window_of(ZC._sq(64, 64, 12), (0.0, 16.0, 8.0), (768, 1024), Z.params(S=128))
    assert (st, X0, Y0, s) == (0, 512.5 - 144.0, 384.5 - 144.0, 2.25)


@pytest.mark.parametrize("case", ZC.window_cases(), ids=[c.name for c in ZC.window_cases()])
def test_window_cases(case):
    recs = ZC.records(case.kind, case.boxes, case.valid)
    sent = np.full(case.params["max_windows"] * Z.WINDOW_DT.itemsize, 0xA5, np.uint8).view(Z.WINDOW_DT)
    win, n = Z.windows_ref(recs, case.counts, case.affine, case.sizes, case.params, out=sent)
    used = [min(max(int(c), 0), 4) for c in case.counts]
    slots = [(b, t) for b in range(3) for t in range(used[b]) if case.valid is None or case.valid[b, t]]
    assert n == min(len(slots), case.params["max_windows"])
    assert [(int(w["map"]), int(w["slot"])) for w in win[:n]] == slots[:n]
    assert (win[n:].view(np.uint8) == 0xA5).all()
    by_key = {(int(w["map"]), int(w["slot"])): w for w in win[:n]}
    for key, bits in case.expect.items():
        if key in by_key:
            assert int(by_key[key]["status"]) == bits, (case.name, key, by_key[key])
    for w in win[:n]:
        assert case.params["s_min"] <= w["s"] <= case.params["s_max"] and w["pad"] == 0
        h, wd = case.sizes[w["map"]]
        span = case.params["S"] * w["s"]
        inside = w["X0"] >= 0 and w["Y0"] >= 0 and w["X0"] + span <= wd and w["Y0"] + span <= h
        assert bool(w["status"] & Z.CLIPPED) == (not inside)


def test_every_status_bit_of_the_windows_is_reached():
    seen = 0
    for case in ZC.window_cases():
        win, n = Z.windows_ref(ZC.records(case.kind, case.boxes, case.valid), case.counts, case.affine, case.sizes, case.params)
        for w in win[:n]:
            seen |= int(w["status"])
    assert seen == Z.CLIPPED | Z.SCALE_CLAMPED_LO | Z.SCALE_CLAMPED_HI


def test_window_affine_maps_pixel_centres():
    win = np.array([(0, 0, 0, 0, 100.5, 60.5, 1.875), (1, 2, 0, 0, -7.25, 3.0, 0.5)], Z.WINDOW_DT)
    aff = Z.window_affine_ref(win)
    for k in range(2):
        ox, oy, inv = aff[k]
        for x in (0, 1, 17, 63):
            assert abs((x - ox) * inv - (win[k]["X0"] + (x + 0.5) * win[k]["s"] - 0.5)) <= 1e-12 * 2000
            assert abs((x - oy) * inv - (win[k]["Y0"] + (x + 0.5) * win[k]["s"] - 0.5)) <= 1e-12 * 2000


# ------------------------------------------------------------------------------------------------ merge
def test_containment_is_exact_on_edges_and_corners():
    assert Z.contains_centre([32, 10, 60, 10, 60, 50, 32, 50], 64)          # on the left edge
    assert Z.contains_centre([32, 32, 60, 32, 60, 60, 32, 60], 64)          # on a corner
    assert not Z.contains_centre([33, 10, 60, 10, 60, 50, 33, 50], 64)
    assert Z.contains_centre([12, 52, 52, 52, 52, 12, 12, 12], 64)          # the other orientation
    assert Z.contains_centre([16, 16, 17, 16, 17, 17, 16, 17], 33)          # S odd: the centre (16.5, 16.5) inside a unit square
    assert not Z.contains_centre([15, 15, 16, 15, 16, 16, 15, 16], 33)


@pytest.mark.parametrize("kind", ["rect", "quad"])
def test_merge_table(kind):
    t = ZC.merge_table(kind)
    sent_q = np.full(t.coarse.shape + (SR.QUAD_DT.itemsize,), 0xA5, np.uint8).reshape(-1).view(SR.QUAD_DT).reshape(t.coarse.shape)
    out, status, scale = Z.merge_ref(ZC.MERGE_S, ZC.MERGE_AGREE, t.win, t.n, t.recs2, t.counts2, t.quads2, t.counts, t.coarse, out=sent_q)
    keys = {(int(w["map"]), int(w["slot"])): k for k, w in enumerate(t.win)}
    for (b, s), (st, target) in t.expect.items():
        k = keys.get((b, s))
        bits = int(t.win[k]["status"]) if k is not None else 0
        assert int(status[b, s]) == st | bits, ((b, s), int(status[b, s]))
        assert scale[b, s] == (t.win[k]["s"] if k is not None else 0.0)
        if st == Z.ZOOMED:
            exp = t.quads2[k, target].copy()
            exp["label"], exp["area"] = t.coarse[b, s]["label"], t.coarse[b, s]["area"]
            assert out[b, s].tobytes() == exp.tobytes()
        else:
            assert out[b, s].tobytes() == t.coarse[b, s].tobytes()
    # slots behind the count keep what the buffer held; no windows at all is the coarse answer everywhere
    out, status, scale = Z.merge_ref(ZC.MERGE_S, ZC.MERGE_AGREE, t.win, t.n, t.recs2, t.counts2, t.quads2, np.array([3, 5, 2]), t.coarse, out=sent_q)
    assert (out[2, 2:].view(np.uint8) == 0xA5).all() and status[2, 2] == Z.NO_WINDOW and scale[2, 2] == 0.0
    out, status, scale = Z.merge_ref(ZC.MERGE_S, ZC.MERGE_AGREE, t.win[:0], 0, None, None, None, t.counts, t.coarse)
    assert out.tobytes() == t.coarse.tobytes() and (status == Z.NO_WINDOW).all() and (scale == 0.0).all()


# ------------------------------------------------------------------------------------------------ accuracy against analytic truth
@pytest.mark.parametrize("method", ["corner", "lines"])
def test_zoom_chain_against_truth(method):
    """Squares rendered at 768 x 1024, first pass on their 128-pixel letterbox (8 source pixels per map pixel), second pass on one
    128-pixel window each, all through the restatements.  The diagonal of the zoom chain is held to the window's s times the bound
    tests/test_subpix_cpu.py holds subpix_ref to on a map, and must beat the coarse chain on every one of the N_DRAWS scenes."""
    scenes = ZC.accuracy_scenes()
    assert len(scenes) == ZC.N_DRAWS
    for sc in scenes:
        prob = ZC.first_pass_prob(sc.img)[None]
        res = ZC.chain_ref([sc.img], prob, method)
        assert res["n"] == 1 and int(res["counts"][0]) == 1 and int(res["status"][0, 0]) & Z.ZOOMED, (sc.squares, res["status"])
        s = float(res["scale"][0, 0])
        assert 1.0 < s < 8.0
        err_zoom = abs(float(res["out"][0, 0]["d_mean"]) - sc.d_true[0])
        err_coarse = abs(float(res["coarse"][0, 0]["d_mean"]) - sc.d_true[0])
        print("zoom chain %s: s = %.3f, |d - d_true| = %.3f source px (bound %.3f), coarse %.3f" % (method, s, err_zoom, s * ZC.SUBPIX_BOUND[method], err_coarse))
        assert err_zoom <= s * ZC.SUBPIX_BOUND[method], (method, sc.squares, err_zoom, s)
        assert err_zoom < err_coarse, (method, sc.squares, err_zoom, err_coarse)
        # the vertices come back in source pixel coordinates: each within the same bound of a true vertex
        from subpix_cases import square_vertices
        truth = square_vertices(*sc.squares[0])
        vs = res["out"][0, 0]["vs"].reshape(4, 2)
        for v in vs:
            assert np.hypot(*(truth - v).T).min() <= 2.0 * s * ZC.SUBPIX_BOUND[method]


# ------------------------------------------------------------------------------------------------ argument errors
def test_library_exports_and_python_exports(vk):
    L = vk.lib()
    for name in ("vk_zoom_windows", "vk_zoom_gather", "vk_zoom_merge"):
        assert hasattr(L, name) and name in vk._lib.SIGNATURES
    assert "zoom" in vk.__all__ and "ZoomedDetections" in vk.__all__ and hasattr(vk.Segmenter, "measure")
    assert vk.zoom.WINDOW_DTYPE == Z.WINDOW_DT and C.sizeof(vk._lib.vk_zoom_window) == 40 and C.sizeof(vk._lib.vk_zoom_image) == 24
    assert C.sizeof(vk._lib.vk_zoom_params) == 32
    assert vk.zoom.STATUS == dict(clipped=Z.CLIPPED, scale_clamped_lo=Z.SCALE_CLAMPED_LO, scale_clamped_hi=Z.SCALE_CLAMPED_HI, zoomed=Z.ZOOMED,
                                  no_target=Z.NO_TARGET, refine_failed=Z.REFINE_FAILED, disagrees=Z.DISAGREES, no_window=Z.NO_WINDOW)
    assert vk._lib.VK_ZOOM_FAIL_MASK == Z.FAIL_MASK == sum(vk.subpix.FLAGS.values())


def _bufs():
    return dict(recs=np.full(3 * 4 * 96 // 8, 7, np.int64), counts=np.full(4, 7, np.int32), sizes=np.full(8, 7, np.int32),
                win=np.full(64 * 5, 7, np.int64), nwin=np.full(2, 7, np.int32), aff=np.full(16, 7.0, np.float64),
                out=np.full(4096, 7, np.float32), tab_dev=np.full(16, 7, np.int64), quads=np.full(3 * 4 * 25, 7, np.int64),
                coarse=np.full(3 * 4 * 25, 7, np.int64), outq=np.full(3 * 4 * 25, 7, np.int64), status=np.full(16, 7, np.int32),
                scale=np.full(16, 7.0, np.float64))


def _untouched(b):
    return all((v == 7).all() for v in b.values())


def test_windows_refuses_bad_arguments(vk):
    L = vk.lib()
    b = _bufs()

    def call(S=64, margin=1.5, s_min=1.0, s_max=32.0, max_windows=8, batch=3, stride=96, box=8, valid=-1, M=4, null=None, off=None, par=True):
        p = vk._lib.vk_zoom_params(S, max_windows, margin, s_min, s_max)
        ptr = {k: (None if null == k else b[k].ctypes.data + (off[1] if off and off[0] == k else 0)) for k in ("recs", "counts", "sizes", "win", "nwin", "aff")}
        rc = L.vk_zoom_windows(C.byref(p) if par else None, batch, ptr["recs"], stride, box, valid, ptr["counts"], M, ptr["aff"], ptr["sizes"],
                               ptr["win"], ptr["nwin"], None)
        assert _untouched(b)
        return rc, L.vk_last_error_string().decode()

    for kw, word in ((dict(par=False), "null parameters"), (dict(S=0), "S = 0"), (dict(S=16385), "S = 16385"), (dict(s_min=0.2), "s_min"),
                     (dict(s_min=2.0, s_max=1.5), "s_min"), (dict(s_max=64.5), "s_max"), (dict(s_min=float("nan")), "s_min"),
                     (dict(margin=0.99), "margin"), (dict(margin=8.5), "margin"), (dict(margin=float("nan")), "margin"),
                     (dict(max_windows=0), "max_windows"), (dict(max_windows=65536), "max_windows"), (dict(batch=0), "batch"),
                     (dict(batch=65536), "batch"), (dict(M=0), "max_components"), (dict(M=4097), "max_components"),
                     (dict(null="recs"), "null buffer"), (dict(null="counts"), "null buffer"), (dict(null="sizes"), "null buffer"),
                     (dict(null="win"), "null buffer"), (dict(null="nwin"), "null buffer"), (dict(stride=94), "record stride"),
                     (dict(box=4), "record stride"), (dict(box=72), "record stride"), (dict(valid=4), "valid offset"),
                     (dict(valid=96), "valid offset"), (dict(off=("counts", 2)), "misaligned"), (dict(off=("win", 4)), "misaligned"),
                     (dict(off=("aff", 4)), "misaligned"), (dict(off=("recs", 1)), "misaligned")):
        rc, err = call(**kw)
        assert rc == -1 and word in err, (kw, err)


def test_gather_refuses_bad_arguments(vk):
    L = vk.lib()
    b = _bufs()

    def call(n=2, S=8, n_images=2, pad=0, flags=0, null=None, off=None, img=None):
        tab = (vk._lib.vk_zoom_image * 2)(vk._lib.vk_zoom_image(4096, 5, 7, 21), vk._lib.vk_zoom_image(8192, 1, 1, 8))
        if img is not None:
            tab[1] = vk._lib.vk_zoom_image(*img)
        ptr = {k: (None if null == k else b[k].ctypes.data + (off[1] if off and off[0] == k else 0)) for k in ("win", "tab_dev", "out")}
        rc = L.vk_zoom_gather(n, S, ptr["win"], n_images, None if null == "tab" else tab, ptr["tab_dev"], pad, flags, ptr["out"], None)
        assert _untouched(b)
        return rc, L.vk_last_error_string().decode()

    for kw, word in ((dict(n=0), "windows"), (dict(n=65536), "windows"), (dict(S=0), "S = 0"), (dict(S=16385), "S = 16385"),
                     (dict(n_images=0), "images"), (dict(pad=-1), "pad_value"), (dict(pad=256), "pad_value"), (dict(flags=2), "unknown flags"),
                     (dict(null="win"), "null buffer"), (dict(null="tab"), "null buffer"), (dict(null="tab_dev"), "null buffer"),
                     (dict(null="out"), "null buffer"), (dict(off=("win", 4)), "misaligned"), (dict(off=("out", 2)), "misaligned"),
                     (dict(img=(0, 4, 4, 12)), "null address"), (dict(img=(64, 0, 4, 12)), "size"), (dict(img=(64, 4, 16385, 3 * 16385)), "size"),
                     (dict(img=(64, 4, 4, 11)), "row stride")):
        rc, err = call(**kw)
        assert rc == -1 and word in err, (kw, err)


def test_merge_refuses_bad_arguments(vk):
    L = vk.lib()
    b = _bufs()

    def call(S=64, agree=0.25, n=2, stride=96, box=8, valid=-1, M2=4, batch=3, M=4, null=None, off=None):
        names = ("win", "recs", "counts", "quads", "sizes", "coarse", "outq", "status", "scale")
        ptr = {k: (None if null == k else b[k].ctypes.data + (off[1] if off and off[0] == k else 0)) for k in names}
        rc = L.vk_zoom_merge(S, agree, n, ptr["win"], ptr["recs"], stride, box, valid, ptr["counts"], M2, ptr["quads"], batch, M, ptr["sizes"],
                             ptr["coarse"], ptr["outq"], ptr["status"], ptr["scale"], None)
        assert _untouched(b)
        return rc, L.vk_last_error_string().decode()

    for kw, word in ((dict(S=0), "S = 0"), (dict(agree=-0.1), "agree"), (dict(agree=float("nan")), "agree"), (dict(agree=float("inf")), "agree"),
                     (dict(n=-1), "windows"), (dict(n=65536), "windows"), (dict(batch=0), "batch"), (dict(M=0), "max_components"),
                     (dict(M=4097), "max_components"), (dict(null="sizes"), "null buffer"), (dict(null="coarse"), "null buffer"),
                     (dict(null="outq"), "null buffer"), (dict(null="status"), "null buffer"), (dict(null="scale"), "null buffer"),
                     (dict(null="win"), "null second-pass"), (dict(null="recs"), "null second-pass"), (dict(null="counts"), "null second-pass"),
                     (dict(null="quads"), "null second-pass"), (dict(M2=0), "max_components2"), (dict(stride=90), "record stride"),
                     (dict(valid=2), "valid offset"), (dict(off=("status", 2)), "misaligned"), (dict(off=("scale", 4)), "misaligned"),
                     (dict(off=("quads", 4)), "misaligned second-pass"), (dict(off=("recs", 2)), "misaligned second-pass")):
        rc, err = call(**kw)
        assert rc == -1 and word in err, (kw, err)


def test_python_entry_points_refuse_wrong_arguments(vk):
    import torch
    Zm = vk.zoom
    dets = vk.geometry.Detections("rect", None, torch.zeros(1, 2, 96, dtype=torch.uint8), torch.zeros(1, dtype=torch.int32), None, 2)
    with pytest.raises(vk.VkError, match="no CPU fallback"):
        Zm.windows(dets, [[8, 8]])
    with pytest.raises(ValueError, match="Detections"):
        Zm.windows("no", [[8, 8]])
    with pytest.raises(ValueError, match="uint8 BGR"):
        Zm._image_table([torch.zeros(4, 4, 3)])
    with pytest.raises(vk.VkError, match="no CPU fallback"):
        Zm._image_table([torch.zeros(4, 4, 3, dtype=torch.uint8)])
    with pytest.raises(ValueError, match="uint8 BGR"):
        Zm._image_table([torch.zeros(4, 4, dtype=torch.uint8)])
    with pytest.raises(ValueError, match="images for"):
        Zm.refine_detections(None, [], dets, torch.zeros(1, 8, 8))
