"""Host side of vk.keypoints (no GPU): the restatement (tests/keypoints_ref.py) on its own, against analytic truth and brute force, on
the reference's own label masks, and the C ABI: exports, layouts, defaults and every argument check of the four entry points through
the loaded library, with sentinel-filled host buffers that must come back untouched.

Measured on the closed form with the float32 table when this file was written (256 positions of the 1/16 grid inside a pixel, the
largest error in either axis; see test_estimators_against_truth, which prints them):
  parabola  sigma 1.5: 0.0300 px    sigma 2: 0.0169 px    sigma 3: 0.0075 px
  centroid  cwin 3, floor_frac 0.25, sigma 2: 0.0219 px"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import geom_cases as GC
import instances_cases as IC
import keypoints_cases as KC
import keypoints_ref as R
import subpix_cases as SC
from conftest import GOLDEN


# ------------------------------------------------------------------------------------------------ the table
def test_table_entries_and_lengths(vk):
    for sigma, n in ((2.0, 9217), (4.0, 36865), (1.5, 72 * 72 + 1), (0.02, 2)):
        t = R.gaussian_table(sigma)
        assert t.dtype == np.float32 and len(t) == n and t[0] == 1.0
        for k in (0, 1, min(7, n - 1), n // 2, n - 1):
            assert t[k] == np.float32(math.exp(-(k / 256.0) / (2.0 * sigma * sigma)))
        assert (np.diff(t) <= 0).all()
        assert vk.keypoints.gaussian_table(sigma).numpy().tobytes() == t.tobytes()
        assert vk.keypoints.table_radius16(sigma) == R.radius16(sigma) == math.isqrt(n - 1)
    assert R.radius16(4.0) == R.MAX_RADIUS16 == vk._lib.VK_KP_MAX_RADIUS16
    assert vk.keypoints.gaussian_table(2.0) is vk.keypoints.gaussian_table(2.0)          # cached
    for bad in (0.0, -1.0, float("nan"), 4.01):
        with pytest.raises(ValueError):
            vk.keypoints.gaussian_table(bad)


# ------------------------------------------------------------------------------------------------ targets
def _one(pts, h=16, w=16, r16=96, vert_type=R.VERT_F64):
    v = np.array(pts, np.float64).reshape(1, -1, 8)
    if vert_type == R.VERT_F64:
        return R.targets_ref(KC.bare_records(v), [v.shape[1]], h, w, KC.table(r16), "v", R.VERT_F64)[0]
    return R.targets_ref(SC.records("rect", v.astype(np.int32)), [v.shape[1]], h, w, KC.table(r16), "box", R.VERT_I32)[0]


def test_targets_value_one_at_an_integer_vertex_and_symmetry():
    m = _one([(5, 7)] * 4, vert_type=R.VERT_I32)
    assert m[7, 5] == 1.0 and m.max() == 1.0 and (m[7, 5] > np.delete(m.reshape(-1), 7 * 16 + 5)).all()
    assert m[7, 4] == m[7, 6] == m[6, 5] == m[8, 5] == KC.table(96)[256]
    c = _one([(8, 8)] * 4, h=17, w=17, vert_type=R.VERT_I32)
    assert c.tobytes() == c[::-1].tobytes() == c[:, ::-1].tobytes() == c.T.tobytes()                 # mirror symmetry
    a, b = _one([(4.25, 6.5)] * 4, h=13, w=17), _one([(16 - 4.25, 6.5)] * 4, h=13, w=17)
    assert a.tobytes() == b[:, ::-1].tobytes()


def test_targets_maximum_of_two_overlapping_discs():
    a, b = _one([(5.25, 6.0)] * 4), _one([(8.5, 7.75)] * 4)
    both = _one([(5.25, 6.0), (8.5, 7.75)] * 2)
    assert both.tobytes() == np.maximum(a, b).tobytes() and (both > a).any() and (both > b).any()


def test_targets_cutoff_is_exact():
    t = KC.table(8)
    m = _one([(3.5, 3.0)] * 4, r16=8)                        # X = 56: pixels 3 and 4 are at D = 64 = table_len - 1
    assert m[3, 3] == m[3, 4] == t[64] and t[64] > 0 and np.count_nonzero(m) == 2
    m = _one([(3.5, 3.0625)] * 4, r16=8)                     # D = 64 + 1 = table_len: outside
    assert np.count_nonzero(m) == 0
    m = _one([(3.5625, 3.0)] * 4, r16=8)                     # D = 81 from pixel 3, 49 from pixel 4
    assert m[3, 3] == 0 and m[3, 4] == t[49] and np.count_nonzero(m) == 1


def test_targets_rounding_rule_of_the_float64_vertices():
    for v, X in ((3.0 + 1 / 32, 49), (3.0 - 1 / 32, 48), (-1 / 32, 0), (-3 / 32, -1), (0.49999, 8), (2.0 ** -60, 0)):      # halves of 1/16 go up
        assert R.fixed_vertices(KC.bare_records([[[v] * 8]]), [1], "v", R.VERT_F64)[0][0] == (X, X), v
    assert math.floor((3.0 + 1 / 32) * 16.0 + 0.5) == 49


def test_targets_skip_rules():
    good = [3.0, 3.0] * 4
    for bad in (float("nan"), float("inf"), -float("inf"), 1048576.0625, -1e300):
        v = np.array([[good, good]], np.float64)
        v[0, 1, 2] = bad
        assert len(R.fixed_vertices(KC.bare_records(v), [2], "v", R.VERT_F64)[0]) == 7, bad
    v = np.array([[[1048576.0, -1048576.0] * 4]])
    assert len(R.fixed_vertices(KC.bare_records(v), [1], "v", R.VERT_F64)[0]) == 4                    # the limit itself is allowed
    recs = SC.records("quad", np.full((1, 3, 8), 4, np.int32), [[1, 0, 1]])
    assert [len(R.fixed_vertices(recs, [c], "box", R.VERT_I32)[0]) for c in (-1, 0, 1, 2, 3, 9)] == [0, 0, 4, 4, 8, 8]
    empty = R.targets_ref(recs, [-1], 5, 5, KC.table(96))
    assert empty.shape == (1, 5, 5) and not empty.any()


def test_target_cases_say_what_they_claim():
    cases = {c.name: c for c in KC.target_cases()}
    assert {(c.h, c.w) for c in cases.values()} >= {(1, 1), (1, 7), (7, 1), (16, 16), (16, 64), (24, 20), (72, 80)}
    assert {c.r16 for c in cases.values()} == {8, 96, 192} and {c.vert_type for c in cases.values()} == {0, 1}
    assert cases["many_r96"].recs.shape == (1, 1024) and cases["batch3_counts"].counts.tolist() == [-1, 0, 9]
    e = cases["cutoff_r8"].expected()[0]
    assert e[3, 3] == KC.table(8)[64] and e[8, 8] == 0 and e[8, 9] == 0 and e[3, 12] == 0 and e[3, 13] == KC.table(8)[49]
    e = cases["batch3_counts"].expected()
    assert not e[0].any() and not e[1].any() and e[2].any()
    assert cases["int32_extremes"].expected()[0][3, 3] == 1.0
    e = cases["64x16_corners"].expected()[0]
    assert e[0, 0] == e[0, 63] == e[15, 0] == e[15, 63] == 1.0 and e[7, 63] > 0 and e[15, 30] > 0


# ------------------------------------------------------------------------------------------------ analytic truth
@pytest.mark.parametrize("name,method,sigma,bound", [("parabola", R.PARABOLA, 1.5, 0.035), ("parabola", R.PARABOLA, 2.0, 0.02),
                                                      ("parabola", R.PARABOLA, 3.0, 0.02), ("centroid", R.CENTROID, 2.0, 0.025)])
def test_estimators_against_truth(name, method, sigma, bound):
    worst_peak, worst = KC.estimator_errors(sigma, method, cwin=3, floor_frac=0.25)
    print("%s sigma %.1f: worst |estimate - vertex| = %.4f px, worst |peak pixel - vertex| = %.4f px" % (name, sigma, worst, worst_peak))
    assert worst_peak <= 0.5
    assert worst <= bound, (name, sigma, worst)


# ------------------------------------------------------------------------------------------------ refine
def test_refine_ties_borders_and_flags():
    flat = np.full((8, 8), 0.5, np.float32)
    assert R.find_peak(flat, 4, 4, 2) == (2, 2, np.float32(0.5)) and R.find_peak(flat, 0, 7, 2)[:2] == (0, 5)
    x, y, f, it, pk = R.refine_vertex(flat, 4, 4, R.kp_params(search=2))
    assert (x, y, f, it, pk) == (2.0, 2.0, R.AT_EDGE, 1, (2, 2))
    m = KC.heat_of(12, 12, [(0.0, 5.25)])                     # on the map's left border: no offset in x, one in y
    x, y, f, it, pk = R.refine_vertex(m, 1, 6, R.kp_params(search=3))
    assert x == 0.0 and pk == (0, 5) and 5.0 < y < 5.5 and f == 0 and it == 1
    assert R.refine_vertex(m, 9, 9, R.kp_params(search=2))[2:4] == (R.NO_PEAK, 0)
    assert R.refine_vertex(m, 40, -40, R.kp_params(search=2))[:4] == (40.0, -40.0, R.NO_PEAK, 0)      # no pixel in the window
    nan = np.full((6, 6), np.nan, np.float32)
    assert R.refine_vertex(nan, 3, 3, R.kp_params())[:4] == (3.0, 3.0, R.NO_PEAK, 0)
    nan[2, 4] = 0.8
    assert R.refine_vertex(nan, 3, 3, R.kp_params())[:2] == (4.0, 2.0)                                # NaN neighbours: offset 0
    assert R.refine_vertex(nan, 3, 3, R.kp_params(R.CENTROID))[:2] == (4.0, 2.0)
    # a quadrilateral whose sides are shorter than the search window: all four find one peak
    heat = KC.heat_of(24, 24, [(10.0, 10.0)])
    v, vs, flags, iters, d1, d2, dm = R.refine_one(heat, [9, 9, 11, 9, 11, 11, 9, 11], R.kp_params(search=4))
    assert flags == [R.SHARED] * 4 and iters == [0] * 4 and v == [9.0, 9.0, 11.0, 9.0, 11.0, 11.0, 9.0, 11.0]


def test_built_refine_cases():
    flags = 0
    kinds = set()
    for c in KC.refine_cases():
        sent = np.full(c.recs.shape + (R.QUAD_DT.itemsize,), 0xA5, np.uint8).reshape(-1).view(R.QUAD_DT).reshape(c.recs.shape)
        out = R.refine_ref(c.heat, c.recs, c.counts, c.params, c.affine, out=sent)
        assert out.tobytes() == R.refine_ref(c.heat, c.recs, c.counts, c.params, c.affine, out=sent).tobytes()
        B, M = c.recs.shape
        seen = 0
        for b in range(B):
            used = min(max(int(c.counts[b]), 0), M)
            assert out[b, used:].tobytes() == sent[b, used:].tobytes()
            for o, r in zip(out[b, :used], c.recs[b, :used]):
                assert o["label"] == r["label"] and o["area"] == r["area"] and o["reserved"] == 0
                if not o["valid"]:
                    assert o.tobytes()[12:] == bytes(R.QUAD_DT.itemsize - 12)
                    continue
                seen |= int(np.bitwise_or.reduce(o["flags"]))
                for q in range(4):
                    keeps = o["flags"][q] & (R.NO_PEAK | R.SHARED)
                    assert o["iters"][q] == (0 if keeps else 1)
                    if keeps:
                        assert (o["v"][2 * q:2 * q + 2] == r["box"][2 * q:2 * q + 2]).all()
        assert seen & c.expect_flags == c.expect_flags, (c.name, seen)
        flags |= seen
        kinds.add(c.recs.dtype.itemsize)
    assert flags == R.NO_PEAK | R.AT_EDGE | R.SHARED and kinds == {96, 104, 40}


def test_targets_then_refine_returns_the_integer_vertices():
    """On a target rendered from int32 vertices at least 2 search + 2 apart, refine returns v == box exactly and the record's own
    diagonals: the value at a vertex is 1.0, its neighbours are equal in pairs, so both offsets are 0 / den = 0."""
    rng = np.random.default_rng(3)
    search = 6
    boxes = np.array([[[10, 12, 60, 9, 64, 50, 8, 55], [30, 25, 45, 26, 44, 40, 29, 41]]], np.int32)
    recs = SC.records("rect", boxes)
    heat = R.targets_ref(recs, [2], 64, 80, KC.table(96))
    for method in (R.PARABOLA, R.CENTROID):
        jit = boxes + rng.integers(-search + 1, search, boxes.shape).astype(np.int32)
        out = R.refine_ref(heat, SC.records("rect", jit), [2], R.kp_params(method, search=search))
        assert (out["flags"] == 0).all() and (out["iters"] == 1).all()
        assert (out["v"] == boxes).all()
        for s in range(2):
            d1, d2, dm = R.SR.diagonals([float(c) for c in boxes[0, s]], 1.0)
            assert (out[0, s]["d1"], out[0, s]["d2"], out[0, s]["d_mean"]) == (d1, d2, dm)


# ------------------------------------------------------------------------------------------------ the reference's own label masks
def test_real_masks_targets_then_refine():
    n_valid = 0
    p = R.kp_params(search=3)
    for idx in range(8):
        m = IC.real_mask(GOLDEN, idx)
        sy, sx = max(1, m.shape[0] // 256), max(1, m.shape[1] // 256)
        m = np.ascontiguousarray(m[::sy, ::sx]).astype(np.float32)
        cfg = GC.Cfg(thresh=0.5, k=1, min_area=30, cap=16, outset=2)
        _, _, recs = GC.MapRef(m, cfg).expected("quad", cfg)
        r = recs[None]
        heat = R.targets_ref(r, [len(recs)], m.shape[0], m.shape[1], KC.table(96))
        out = R.refine_ref(heat, r, [len(recs)], p)
        assert out.tobytes() == R.refine_ref(R.targets_ref(r, [len(recs)], m.shape[0], m.shape[1], KC.table(96)), r, [len(recs)], p).tobytes()
        for s in range(len(recs)):
            o = out[0, s]
            assert o["valid"] == int(recs[s]["valid"] != 0)
            if not o["valid"]:
                continue
            n_valid += 1
            moved = np.abs(o["v"] - recs[s]["box"].astype(np.float64)).reshape(4, 2).max(axis=1)
            for q in range(4):
                assert moved[q] == 0.0 or o["flags"][q] != 0, (idx, s, q, moved[q], o["flags"][q])
                if o["flags"][q] & (R.NO_PEAK | R.SHARED):
                    assert moved[q] == 0.0
    assert n_valid >= 8


# ------------------------------------------------------------------------------------------------ peaks
def _brute_peaks(m, min_peak, r):
    h, w = m.shape
    out = []
    for y in range(h):
        for x in range(w):
            p = m[y, x]
            if not float(p) >= min_peak:
                continue
            ok = True
            for j in range(max(0, y - r), min(h, y + r + 1)):
                for i in range(max(0, x - r), min(w, x + r + 1)):
                    q = m[j, i]
                    if q > p or (q == p and (j, i) < (y, x)):
                        ok = False
            if ok:
                out.append((x, y))
    return out


def test_peak_cases():
    cases = {c.name: c for c in KC.peak_cases()}
    with np.errstate(invalid="ignore"):
        for c in cases.values():
            sent = np.full((c.heat.shape[0], c.max_peaks, 16), 0xA5, np.uint8).reshape(-1).view(R.PEAK_DT).reshape(c.heat.shape[0], c.max_peaks)
            out, counts = R.peaks_ref(c.heat, c.min_peak, c.r, c.max_peaks, out=sent)
            for b in range(c.heat.shape[0]):
                want = _brute_peaks(c.heat[b], c.min_peak, c.r)
                n = min(len(want), c.max_peaks)
                assert counts[b] == len(want), c.name
                assert [(int(o["x"]), int(o["y"])) for o in out[b, :n]] == want[:n] and (out[b, :n]["reserved"] == 0).all()
                assert all(o["value"] == c.heat[b, o["y"], o["x"]] for o in out[b, :n])
                assert out[b, n:].tobytes() == sent[b, n:].tobytes()
    res = {n: R.peaks_ref(c.heat, c.min_peak, c.r, c.max_peaks) for n, c in cases.items()}
    assert res["1x1_peak"][1].tolist() == [1] and res["1x1_below"][1].tolist() == [0] and res["1x1_nan"][1].tolist() == [0]
    assert res["plateau_r1"][1][0] == res["plateau_r2"][1][0] == res["plateau_r8"][1][0] == 1             # a plateau wider than the window: one peak
    assert [(o["x"], o["y"]) for o in res["plateau_r8"][0][0, :1]] == [(3, 2)]                            # its raster-first pixel
    assert res["equal_across_the_edge_r2"][1][0] == 5 and res["equal_across_the_edge_r3"][1][0] == 3 and res["equal_across_the_edge_r8"][1][0] == 1
    assert res["min_peak_met_with_equality"][1].tolist() == [1] and res["min_peak_met_with_equality"][0][0, 0]["x"] == 3
    assert (9, 4) in [(o["x"], o["y"]) for o in res["nan_and_inf"][0][0, :res["nan_and_inf"][1][0]]]
    assert res["70x40_exceeded"][1][0] == res["70x40_r1"][1][0] > 5
    assert res["batch3"][1][1] == 0 and len(set(res["batch3"][1].tolist())) == 3


def test_vertex_metrics(vk):
    K = vk.keypoints
    gt = np.array([[10.0, 10.0], [30.0, 10.0], [30.0, 30.0], [10.0, 30.0]])
    pk = np.zeros(4, K.PEAK_DTYPE)
    pk["x"], pk["y"] = [10, 31, 50, 11], [11, 10, 50, 10]       # (11, 10) and (10, 11) both 1.0 from gt 0: the lower peak index wins
    m = K.vertex_metrics(pk, gt, tol_px=2.0)
    assert (m["tp"], m["fp"], m["fn"]) == (2, 2, 2) and m["precision"] == 0.5 and m["recall"] == 0.5 and m["mean_dist"] == 1.0
    assert K.vertex_metrics(np.zeros((0, 2)), gt)["recall"] == 0.0 and K.vertex_metrics(np.zeros((0, 2)), gt)["precision"] == 1.0
    assert K.vertex_metrics(gt, gt, 0.0)["tp"] == 4


# ------------------------------------------------------------------------------------------------ the C ABI without a GPU
def test_library_and_python_exports(vk):
    L, K = vk._lib, vk.keypoints
    lib = vk.lib()
    for name in ("vk_kp_targets", "vk_kp_peaks_workspace_bytes", "vk_kp_peaks", "vk_kp_refine"):
        assert hasattr(lib, name) and name in L.SIGNATURES
    assert "keypoints" in vk.__all__
    assert C.sizeof(L.vk_kp_peak) == 16 and np.dtype(L.vk_kp_peak) == R.PEAK_DT == K.PEAK_DTYPE
    assert C.sizeof(L.vk_kp_params) == 32 and (L.vk_kp_params.min_peak.offset, L.vk_kp_params.floor_frac.offset) == (16, 24)
    assert K.FLAGS == dict(no_peak=R.NO_PEAK, at_edge=R.AT_EDGE, shared=R.SHARED) and not set(K.FLAGS.values()) & set(vk.subpix.FLAGS.values())
    assert L.SUBPIX_FLAGS == vk.subpix.FLAGS and len(vk.subpix.FLAGS) == 7
    p = K.params()
    assert (p.method, p.search, p.cwin, p.min_peak, p.floor_frac) == (0, 6, 3, 0.3, 0.25)
    assert K.params("centroid").method == 1
    assert (L.VK_KP_MAX_NMS, L.VK_KP_MAX_SEARCH, L.VK_KP_MAX_CWIN) == (R.MAX_NMS, R.MAX_SEARCH, R.MAX_CWIN)
    assert lib.vk_kp_peaks_workspace_bytes(1, 1, 1) == 260 and lib.vk_kp_peaks_workspace_bytes(3, 40, 70) == 3 * 3 * 260
    assert lib.vk_kp_peaks_workspace_bytes(2, 1 << 15, 1 << 15) == 2 * (1 << 20) * 260


class _Bufs:
    """Host buffers filled with a sentinel; every call must leave them as they were."""

    def __init__(self):
        self.b = dict(records=np.full(96, 7, np.int64), counts=np.full(4, 7, np.int32), table=np.full(80, 7, np.float32),
                      out=np.full(256, 7.0), heat=np.full(128, 7, np.float32), affine=np.full(8, 7.0), ws=np.full(2048, 7, np.int32))

    def ptr(self, name, null=None, off=None):
        if null == name:
            return None
        return self.b[name].ctypes.data + (off[1] if off and off[0] == name else 0)

    def check(self):
        for name, b in self.b.items():
            assert (b == 7).all(), name


def _targets(vk, null=None, off=None, **kw):
    a = dict(batch=1, h=8, w=8, stride=96, voff=8, vtype=0, valid_off=-1, cap=2, table_len=65, istride=64, flags=0)
    a.update(kw)
    B = _Bufs()
    rc = vk.lib().vk_kp_targets(a["batch"], a["h"], a["w"], B.ptr("records", null, off), a["stride"], a["voff"], a["vtype"], a["valid_off"],
                                B.ptr("counts", null, off), a["cap"], B.ptr("table", null, off), a["table_len"], B.ptr("out", null, off),
                                a["istride"], a["flags"], None)
    B.check()
    return rc, vk.lib().vk_last_error_string().decode()


def _peaks(vk, null=None, off=None, **kw):
    a = dict(batch=1, h=8, w=8, istride=64, min_peak=0.3, r=2, max_peaks=4, ws_bytes=260)
    a.update(kw)
    B = _Bufs()
    rc = vk.lib().vk_kp_peaks(a["batch"], a["h"], a["w"], B.ptr("heat", null, off), a["istride"], a["min_peak"], a["r"], a["max_peaks"],
                              B.ptr("out", null, off), B.ptr("counts", null, off), B.ptr("ws", null, off), a["ws_bytes"], None)
    B.check()
    return rc, vk.lib().vk_last_error_string().decode()


def _refine(vk, null=None, off=None, **kw):
    a = dict(batch=1, h=8, w=8, istride=64, stride=96, box_off=8, valid_off=-1, cap=2)
    pkw = {k: kw.pop(k) for k in list(kw) if k in ("method", "search", "cwin", "min_peak", "floor_frac")}
    a.update(kw)
    p = vk.keypoints.params(**{k: v for k, v in pkw.items() if k != "method"})
    p.method = pkw.get("method", 0)
    B = _Bufs()
    rc = vk.lib().vk_kp_refine(None if null == "params" else C.byref(p), a["batch"], a["h"], a["w"], B.ptr("heat", null, off), a["istride"],
                               B.ptr("records", null, off), a["stride"], a["box_off"], a["valid_off"], B.ptr("counts", null, off), a["cap"],
                               B.ptr("affine", null, off), B.ptr("out", null, off), None)
    B.check()
    return rc, vk.lib().vk_last_error_string().decode()


_MAPS = ((dict(batch=0), "batch"), (dict(batch=65536), "batch"), (dict(h=0), "map size"), (dict(w=-1), "map size"),
         (dict(h=1 << 15, w=(1 << 15) + 1, istride=1 << 31), "2^30"), (dict(istride=63), "image stride"), (dict(istride=1 << 41), "image stride"))


def test_targets_refuses_bad_arguments(vk):
    for kw, word in _MAPS + ((dict(cap=0), "max_components = 0"), (dict(cap=4097), "max_components = 4097"), (dict(vtype=2), "vertex type 2"),
                             (dict(vtype=-1), "vertex type -1"), (dict(stride=38), "record stride"), (dict(stride=36), "record stride"),
                             (dict(voff=6), "record stride"), (dict(voff=68), "record stride"), (dict(voff=1 << 40), "record stride"),
                             (dict(stride=1 << 21), "record stride"), (dict(vtype=1, stride=100), "record stride"), (dict(vtype=1, voff=12), "record stride"),
                             (dict(vtype=1, voff=40), "record stride"), (dict(valid_off=-2), "valid offset"), (dict(valid_off=94), "valid offset"),
                             (dict(valid_off=96), "valid offset"), (dict(table_len=0), "table_len = 0"), (dict(table_len=1), "table_len = 1"),
                             (dict(table_len=64), "table_len = 64"), (dict(table_len=66), "table_len = 66"), (dict(table_len=193 * 193 + 1), "table_len"),
                             (dict(table_len=-5), "table_len = -5"), (dict(flags=3), "flags = 3"), (dict(flags=-1), "flags = -1"),
                             (dict(flags=2, table_len=124 * 124 + 1), "LDS path"), (dict(off=("records", 2)), "misaligned"),
                             (dict(vtype=1, off=("records", 4)), "misaligned"), (dict(off=("counts", 1)), "misaligned"),
                             (dict(off=("table", 2)), "misaligned"), (dict(off=("out", 2)), "misaligned")):
        rc, err = _targets(vk, **kw)
        assert rc == -1 and word in err, (kw, err)
    for name in ("records", "counts", "table", "out"):
        rc, err = _targets(vk, null=name)
        assert rc == -1 and "null" in err, name


def test_peaks_refuses_bad_arguments(vk):
    for kw, word in _MAPS + ((dict(min_peak=float("nan")), "min_peak"), (dict(min_peak=float("inf")), "min_peak"), (dict(r=0), "nms_radius = 0"),
                             (dict(r=9), "nms_radius = 9"), (dict(max_peaks=0), "max_peaks = 0"), (dict(max_peaks=4097), "max_peaks = 4097"),
                             (dict(ws_bytes=259), "workspace"), (dict(ws_bytes=0), "workspace"), (dict(batch=2, istride=64), "workspace"),
                             (dict(off=("heat", 2)), "misaligned"), (dict(off=("out", 2)), "misaligned"), (dict(off=("counts", 1)), "misaligned"),
                             (dict(off=("ws", 3)), "misaligned")):
        rc, err = _peaks(vk, **kw)
        assert rc == -1 and word in err, (kw, err)
    for name in ("heat", "out", "counts", "ws"):
        rc, err = _peaks(vk, null=name)
        assert rc == -1 and "null" in err, name
    lib = vk.lib()
    for args in ((0, 8, 8), (65536, 8, 8), (1, 0, 8), (1, 8, -1), (1, 1 << 15, (1 << 15) + 1)):
        assert lib.vk_kp_peaks_workspace_bytes(*args) == 0, args


def test_refine_refuses_bad_arguments(vk):
    for kw, word in _MAPS + ((dict(method=2), "method 2"), (dict(method=-1), "method -1"), (dict(search=0), "search = 0"), (dict(search=32), "search = 32"),
                             (dict(cwin=0), "cwin = 0"), (dict(cwin=8), "cwin = 8"), (dict(min_peak=float("nan")), "min_peak"),
                             (dict(min_peak=-float("inf")), "min_peak"), (dict(floor_frac=1.0), "floor_frac"), (dict(floor_frac=-0.1), "floor_frac"),
                             (dict(floor_frac=float("nan")), "floor_frac"), (dict(cap=0), "max_components = 0"), (dict(cap=4097), "max_components = 4097"),
                             (dict(stride=38), "record stride"), (dict(stride=36), "record stride"), (dict(box_off=6), "record stride"),
                             (dict(box_off=4), "record stride"), (dict(box_off=68), "record stride"), (dict(box_off=1 << 40), "record stride"),
                             (dict(valid_off=-2), "valid offset"), (dict(valid_off=94), "valid offset"), (dict(valid_off=96), "valid offset"),
                             (dict(valid_off=4), "valid offset"), (dict(off=("heat", 2)), "misaligned"), (dict(off=("records", 2)), "misaligned"),
                             (dict(off=("counts", 1)), "misaligned"), (dict(off=("out", 4)), "misaligned"), (dict(off=("affine", 4)), "misaligned")):
        rc, err = _refine(vk, **kw)
        assert rc == -1 and word in err, (kw, err)
    for name in ("params", "heat", "records", "counts", "out"):
        rc, err = _refine(vk, null=name)
        assert rc == -1 and "null" in err, name


def test_python_entry_points_refuse_wrong_arguments(vk):
    K, I = vk.keypoints, vk.instances
    heat = torch.rand(2, 8, 8)
    z8, z32 = torch.zeros(2, 8, 8, dtype=torch.uint8), torch.zeros(2, 8, 8, dtype=torch.int32)
    dets = I.Detections("rect", z8, torch.zeros(2, 4, 96, dtype=torch.uint8), torch.zeros(2, dtype=torch.int32), z32, 4)
    for call in (lambda: K.refine(dets, heat), lambda: K.targets(dets), lambda: K.peaks(heat), lambda: K.make_targets(torch.zeros(2, 1, 8, 8)),
                 lambda: K.postprocess(torch.rand(2, 2, 8, 8)), lambda: K.targets(torch.zeros(2, 3, 4, 2, dtype=torch.float64), (8, 8),
                                                                                  counts=torch.zeros(2, dtype=torch.int32))):
        with pytest.raises(vk.VkError, match="no CPU fallback"):
            call()
    for call in (lambda: K.refine(None, heat), lambda: K.params("corner"), lambda: K.targets(torch.zeros(2, 3, 4, 2)), lambda: K.targets(heat),
                 lambda: K.targets(torch.zeros(2, 3, 4, 2, dtype=torch.float64)), lambda: K.peaks(heat[0]), lambda: K.peaks(heat.double()),
                 lambda: K.make_targets(torch.zeros(2, 2, 8, 8)), lambda: K.postprocess(heat), lambda: K.targets(dets, table="l2")):
        with pytest.raises(ValueError):
            call()
