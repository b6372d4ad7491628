"""Proves the cases of tests/geom_cases.py on the references alone (no GPU): this file checks the cases, not the kernels.  Every
condition DESIGN.md section 23 relies on is recomputed here: component counts and areas of the built topologies (against an
independent flood fill), the lattice polygons' hulls and exact ties, the border lengths of the capacity cases, the branch each named
shape takes, the special values of the threshold maps, and that the module's own pieces (component split, column-extreme prefilter,
cropped fit, quad_fit) equal the oracle's."""
from collections import deque

import numpy as np
import pytest

import geom_cases as GC
from oracle import geometry_oracle as G
from oracle import quad_oracle as Q

F = np.float32


def flood_fill(mask):
    """Independent twin of geometry_oracle.label8: plain breadth-first flood fill in raster order, 8-connected."""
    h, w = mask.shape
    lab = np.zeros((h, w), np.int32)
    areas = [0]
    for y in range(h):
        for x in range(w):
            if not mask[y, x] or lab[y, x]:
                continue
            n = len(areas)
            lab[y, x] = n
            todo, cnt = deque([(y, x)]), 0
            while todo:
                cy, cx = todo.popleft()
                cnt += 1
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        yy, xx = cy + dy, cx + dx
                        if 0 <= yy < h and 0 <= xx < w and mask[yy, xx] and not lab[yy, xx]:
                            lab[yy, xx] = n
                            todo.append((yy, xx))
            areas.append(cnt)
    return lab, np.array(areas, dtype=np.int64)


TOPO = GC.topology_cases()


@pytest.mark.parametrize("case", TOPO, ids=[c.name for c in TOPO])
def test_topology_has_its_stated_components(case):
    prob = case.probs()[0]
    mask = prob > 0
    assert prob.shape in ((GC.TOPO_H, GC.TOPO_W), (GC.TOPO_W, GC.TOPO_H)) and GC.TOPO_W > 128
    lab, areas = flood_fill(mask)
    lab_o, areas_o = G.label8(mask.astype(np.uint8) * 255)
    assert np.array_equal(lab, lab_o) and np.array_equal(areas[1:], areas_o[1:])
    # ids 1..N in the order of each component's first pixel
    firsts = [int(np.flatnonzero(lab.ravel() == i)[0]) for i in range(1, len(areas))]
    assert firsts == sorted(firsts)
    exp = case.expect
    assert len(areas) - 1 == exp["ncomp"]
    if "areas" in exp:
        assert areas[1:].tolist() == exp["areas"]
    if "areas_sorted" in exp:
        assert sorted(areas[1:].tolist()) == exp["areas_sorted"]
    if exp.get("single"):
        assert int(areas[1]) == int(mask.sum()) > 0
    if "@" in case.name:
        return
    ref = GC.MapRef(prob, case.cfg)
    assert ref.n == exp["ncomp"] and np.array_equal(ref.clean(1) > 0, mask)


def test_topology_details():
    """What each shape is built for."""
    s = GC.serpentine()
    assert s.sum() == 19 * GC.TOPO_W + 18 and s[:, 64].sum() == 19           # fills the map: every other row + one joint per gap
    for m in (GC.spiral(), s):                                                 # one-pixel paths: two ends, every other pixel has two edge neighbours
        p = np.pad(m, 1).astype(int)
        nb = (p[:-2, 1:-1] + p[2:, 1:-1] + p[1:-1, :-2] + p[1:-1, 2:])[m]
        assert sorted(np.bincount(nb).tolist()) == sorted([0, 2, int(m.sum()) - 2]), np.bincount(nb)
    assert GC.checker()[1::2, 0::2].sum() == 0                                 # no two pixels of the checker touch by an edge
    c = GC.checker()
    assert not (c[:, 1:] & c[:, :-1]).any() and not (c[1:] & c[:-1]).any()
    for anti in (False, True):                                                 # staircases: no edge contacts, one diagonal kind only
        m = GC.stairs(anti)
        assert not (m[:, 1:] & m[:, :-1]).any() and not (m[1:] & m[:-1]).any()
        assert not ((m[1:, 1:] & m[:-1, :-1]) if anti else (m[1:, :-1] & m[:-1, 1:])).any()
    d = GC.dots()
    assert d.sum() == 19 * 66 and d[:, :64].sum(axis=1).max() == 32            # 32 roots in one 64-pixel stretch
    r = GC.rings()
    assert not r[3, 3:-3].any() and not r[3:-3, 3].any()                       # the one-pixel gap between the rings
    t = GC.teeth_63_64_65()
    assert t[10, 63] and not t[10, 64] and t[20, 64] and not t[20, 65] and t[30, 65]
    assert GC.comb(True, 0)[-1].all() and not GC.comb(True, 0)[0].any() and GC.comb(False, 1)[0].all()
    assert GC.bars().all(axis=1)[0::2].all() and not GC.bars()[1::2].any()


def test_edge_shapes_and_limits():
    shapes = GC.edge_shapes()
    assert all(h != w for h, w in shapes) and all((w, h) in shapes for h, w in shapes)
    for h in GC.EDGE_H:
        for w in GC.EDGE_W:
            assert h == w or (h, w) in shapes
    assert {h % 4 for h, _ in shapes} == {0, 1, 2, 3} and {1, 63, 64, 65} <= {w for _, w in shapes}
    by = {c.name: c for c in GC.limit_cases()}
    assert by["line_4096x1"].probs().shape == (1, GC.GEOM_MAX_H, 1) and by["zigzag_4096x3"].probs().shape == (1, GC.GEOM_MAX_H, 3)
    assert by["noise_1x16384"].probs().shape == (1, 1, 16384)
    rows = by["rows_3x16384"].probs()[0]
    assert rows.shape == (3, 16384) and rows[0].all()
    z = GC.zigzag()
    assert (z.sum(axis=1) == 1).all() and GC.MapRef(z.astype(F), GC.Cfg()).n == 1
    assert GC.MapRef(GC.full_height_line().astype(F), GC.Cfg()).areas[1] == GC.GEOM_MAX_H


def test_compaction_cases():
    by = {c.name: c for c in GC.compaction_cases()}
    ref = GC.MapRef(by["dots_130x130@cap4096"].probs()[0], GC.Cfg())
    assert ref.n == 4225 and (ref.areas[1:] == 1).all()
    clean, count, recs = ref.expected("rect", by["dots_130x130@cap4096"].cfg)
    assert count == 4225 and len(recs) == 4096 and recs["label"].tolist() == list(range(1, 4097)) and int((clean > 0).sum()) == 4225
    # slot 4095 is the dot of raster rank 4095: row 2 * (4095 // 65), column 2 * (4095 % 65)
    assert recs["box"][4095].tolist() == [2 * (4095 % 65), 2 * (4095 // 65)] * 4
    for cap in (1, 4095):
        assert len(ref.expected("rect", by[f"dots_130x130@cap{cap}"].cfg)[2]) == cap
    n = 520 * 520
    nchunk = (n + 1023) // 1024
    per = (nchunk + 255) // 256
    assert nchunk == 265 and per == 2 and nchunk % per == 1 and n % 1024 != 0       # uneven ranges with a short tail, ragged last chunk
    big = GC.MapRef(by["noise_520x520"].probs()[0], GC.Cfg())
    assert big.n > 4096 and len(big.kept(9)) < 4096                                  # one call overflows the list, the other does not
    assert by["dots_1x128"].probs()[0, 0, :64].sum() == 32 and by["dots_1x2048"].probs()[0, 0, :1024].sum() == 512


HULLS = [c for c in GC.hull_cases() if "K" in c.expect]


@pytest.mark.parametrize("K,j", GC.CHORDS)
def test_chord_polygon_has_its_only_minimal_edge_on_the_second_stride_trip(K, j):
    q = GC.chord_polygon(K, j)
    m = GC.chord_map(K, j)
    assert len(G.label8(m.astype(np.uint8))[1]) == 2
    ys, xs = np.nonzero(m)
    hull = G.convex_hull(GC.column_extremes(np.stack([xs, ys], axis=1)))
    assert len(q) == j + 1 > 256 and np.array_equal(hull, q + [2, 1])
    ea = GC.edge_areas(hull)
    assert np.flatnonzero(ea == ea.min()).tolist() == [j] and j >= 256          # unique, and beyond the first 256 edges
    first_trip = int(np.argmin(ea[:256]))                                       # what a single trip would answer: another rectangle
    a, b = hull[first_trip], hull[first_trip + 1]
    d = (b - a).astype(F)
    ln = np.sqrt(F(F(d[0] * d[0]) + F(d[1] * d[1])), dtype=F)
    assert G.min_area_rect(hull)["u"] != (F(d[0] / ln), F(d[1] / ln))


@pytest.mark.parametrize("case", HULLS, ids=[c.name for c in HULLS])
def test_lattice_polygon_hull_and_ties(case):
    K, corner = case.expect["K"], case.expect["corner"]
    poly = GC.lattice_polygon(K)
    nvert = {4: 48, 10: 256, 11: 336, 14: 512}[K]
    assert len(poly) == nvert
    m = case.probs()[0] > 0
    lab, areas = G.label8(m.astype(np.uint8))
    assert len(areas) == 2
    ys, xs = np.nonzero(m)
    pts = np.stack([xs, ys], axis=1)
    hull = G.convex_hull(GC.column_extremes(pts))
    off = 0 if corner else 3
    assert np.array_equal(hull, poly + off)                      # vertex set and canonical order
    if corner:
        assert m[0].any() and m[:, 0].any()
    if K <= 10:                                                  # the prefilter changes nothing (all pixels through the oracle's hull)
        assert np.array_equal(G.convex_hull(pts), hull)
    ea = GC.edge_areas(hull)
    ties = np.flatnonzero(ea == ea.min())
    assert len(ties) >= 2
    if nvert > 64:
        assert len({int(i) // 64 for i in ties}) >= 2, ties      # exact ties in different waves of the calipers' reduction
    if K == 10:
        assert ties.tolist() == [29, 33, 93, 97, 157, 161, 221, 225]
    if K >= 11:
        assert nvert > 256 and ties[0] < 256 <= ties[-1]         # a tie between the first and the second stride trip
    rect = G.min_area_rect(hull)                                 # the oracle takes the first of them
    i, j = int(ties[0]), (int(ties[0]) + 1) % nvert
    d = (hull[j] - hull[i]).astype(F)
    ln = np.sqrt(F(F(d[0] * d[0]) + F(d[1] * d[1])), dtype=F)
    assert rect["u"] == (F(d[0] / ln), F(d[1] / ln))


def test_contour_capacity_cases():
    for case in GC.capacity_cases():
        W = case.expect["contour_n"] // 2
        m = case.probs()[0] > 0
        assert m.shape == (8, W + 2)
        ys, xs = np.nonzero(m)
        cnt = GC.fit_contour(xs, ys, 8, W + 2, 0)
        assert len(cnt) == 2 * W and (len(cnt) > GC.GQ_NC) == bool(case.expect["flags"])
        rec = GC.MapRef(case.probs()[0], case.cfg).quad(1, 0)
        assert rec["contour_n"] == 2 * W and rec["flags"] == case.expect["flags"] and rec["hull_n"] == len(Q.convex_hull_cv(cnt))
        if not case.expect["flags"]:                             # within capacity: the module's fit is the oracle's
            tr = {}
            q = Q.robust_quadrilateral_from_contour(cnt, trace=tr)
            assert rec["valid"] == (q is not None) and rec["branch"] == GC.BRANCH[tr["branch"]] and rec["n_candidates"] == tr["n_candidates"]
        else:                                                    # beyond: the hull alone, as the oracle would fit the hull's points
            q, branch, ncand = GC.quad_fit(cnt, use_contour=False)
            assert rec["valid"] == 1 and rec["branch"] == GC.BRANCH[branch] and ncand >= 1


def _quad_cases():
    return [c for c in GC.degenerate_cases() + GC.branch_cases() if "quad" in c.paths] + [c for c in TOPO if c.name.endswith("-base")]


@pytest.mark.parametrize("case", _quad_cases(), ids=[f"{c.family}-{c.name}" for c in _quad_cases()])
def test_quad_fit_is_the_oracles_and_named_branches_occur(case):
    """quad_fit with the border candidate equals robust_quadrilateral_from_contour; the cropped fit equals the fit on the whole map;
    the degenerate and named shapes take the stated path in the oracle."""
    prob = case.probs()[0]
    ref = GC.MapRef(prob, case.cfg)
    kk = max(3, 2 * case.cfg.outset + 1)
    for label in range(1, min(ref.n, 40) + 1):
        xs, ys = ref.pixels(label)
        sel = (ref.labels == label).astype(np.uint8) * np.uint8(255)
        whole = G.dilate(sel, G.ellipse_kernel(kk)) if case.cfg.outset > 0 else sel
        cnt = Q.trace_external_contour(whole)
        assert np.array_equal(cnt, GC.fit_contour(xs, ys, ref.h, ref.w, case.cfg.outset))
        tr = {}
        q = Q.robust_quadrilateral_from_contour(cnt, trace=tr) if len(cnt) >= 4 else None
        got, branch, ncand = GC.quad_fit(cnt)
        assert (q is None) == (got is None) and (q is None or np.array_equal(q, got))
        assert (branch, ncand) == ((tr["branch"], tr["n_candidates"]) if tr else ("none", 0))
    want = case.expect.get("quad")
    if want:
        assert ref.n == 1
        rec = ref.quad(1, case.cfg.outset)
        for key, v in want.items():
            assert rec[key] == (GC.BRANCH[v] if key == "branch" else v), (case.name, key, rec)
        if want == {"valid": 0}:                                 # a border of fewer than four points: no fit is attempted
            assert rec["contour_n"] < 4 and rec["branch"] == 0 and rec["n_candidates"] == 0


def test_every_branch_is_named_once():
    names = {c.expect["quad"]["branch"] for c in GC.branch_cases()}
    assert names == {"extremes", "subsample", "none"}


def test_degenerate_rectangles():
    """m == 1 and m == 2 in the oracle: what include/vk_unet.h documents for them."""
    by = {c.name: c for c in GC.degenerate_cases()}
    r = GC.MapRef(by["pixel-plain"].probs()[0], GC.Cfg()).rect(1)
    assert r["hull_n"] == 1 and r["box"].tolist() == [64, 4] * 4 and (r["rw"], r["rh"], r["ux"], r["uy"]) == (0, 0, 1, 0)
    assert (r["d1"], r["d2"], r["d_mean"]) == (0.0, 0.0, 0.0)
    for kind, u in (("horizontal", (1, 0)), ("vertical", (0, 1))):
        for n in (2, 7, 250):
            r = GC.MapRef(by[f"{kind}{n}-plain"].probs()[0], GC.Cfg()).rect(1)
            assert r["hull_n"] == 2 and r["area"] == n and (r["ux"], r["uy"]) == u and r["rw"] == n - 1 and r["rh"] == 0
            assert r["d1"] == n - 1 and r["d2"] == n - 1                 # the box collapses onto the segment: both "diagonals" are it
    for kind in ("diagonal", "antidiagonal"):
        for n in (2, 7, 250):
            r = GC.MapRef(by[f"{kind}{n}-plain"].probs()[0], GC.Cfg()).rect(1)
            assert r["hull_n"] == 2 and r["area"] == n and 0 <= float(r["rh"]) < 1e-4 and abs(float(r["rw"]) - (n - 1) * 2 ** 0.5) < 1e-3
    # truncation of a coordinate just below an integer shows in the int32 box, so bits matter
    r = GC.MapRef(by["antidiagonal7-plain"].probs()[0], GC.Cfg()).rect(1)
    assert r["box"].tolist() == [66, 2, 60, 8, 60, 8, 66, 2]          # the segment runs from (66, 3) to (60, 9): 2.9999..., 8.9999... truncated
    r = GC.MapRef(by["corner_diagonal2-plain"].probs()[0], GC.Cfg()).rect(1)
    assert r["box"].tolist() == [0] * 8 and r["d1"] == 0.0             # (1, 1) comes out as 0.99999994: the box collapses to the corner
    r2 = GC.MapRef(by["square2-plain"].probs()[0], GC.Cfg()).rect(1)
    assert r2["hull_n"] == 4 and r2["area"] == 4


def test_threshold_maps_hold_every_special_value_on_both_sides():
    for t in GC.THRESHOLDS:
        m = GC.threshold_map(t)
        sv = GC.special_values(t)
        b = GC.bits(m)
        for v in sv:
            assert (b == GC.bits(np.array([v], dtype=F))[0]).sum() >= 3, (t, v)       # by bit pattern: NaN and -0 count
        mask = G.binarize(m, t) > 0
        assert mask.any() and (~mask).any()
        ft = F(t)
        assert mask[b == GC.bits(np.array([ft]))[0]].all()                            # at the threshold: foreground
        assert mask[m == np.nextafter(ft, F(np.inf))].all() and not mask[m == np.nextafter(ft, F(-np.inf))].any()
        assert not mask[np.isnan(m)].any() and mask[m == np.inf].all() and not mask[m == -np.inf].any()
        assert bool(mask[(m == 0)].all()) == (t <= 0.0)                               # +0 and -0 are foreground only for t = 0
        # the fused form is binarize followed by the oracle's erosion / dilation
        k = G.ellipse_kernel(3)
        assert np.array_equal(GC.front(m, GC.Cfg(thresh=t, k=3, oi=1, ci=0))[0], G.dilate(G.erode(G.binarize(m, t), k), k))


def test_morphology_maps():
    maps = GC.morph_maps() > 0
    assert maps[1].all() and maps[2][1:-1, 1:-1].all() and maps[2].sum() == 38 * 68
    for case in GC.morph_cases():
        refs = [GC.MapRef(p, case.cfg) for p in case.probs()]
        assert refs[1].mask.all(), case.name                     # outside pixels never win: all foreground stays all foreground
        assert case.cfg.oi <= 16 and case.cfg.ci <= 16 and max(case.cfg.oi, case.cfg.ci) > 2


def test_composition_equals_the_oracles_own():
    """With the reference's floor of 200 px the composed reference is the oracle's postprocess_*_multi."""
    rng = np.random.default_rng(3)
    prob = np.clip(rng.normal(0.2, 0.15, size=(96, 161)), 0, 1).astype(F)
    prob[10:40, 5:45] = 0.9
    prob[50:95, 100:161] = 0.8
    prob[45:60, 60:75] = 0.95
    for kind, fn, thresh in (("rect", G.postprocess_minarearect_multi, 0.5), ("quad", Q.postprocess_quadrilateral_multi, 0.45)):
        cfg = GC.Cfg(thresh=thresh, k=3, oi=1, ci=1, min_area=200, cap=64, outset=2)
        clean_o, dets_o = fn(prob, bin_thresh=thresh)
        clean, count, recs = GC.MapRef(prob, cfg).expected(kind, cfg)
        assert np.array_equal(clean, clean_o) and count == len(dets_o) == 3
        dets_o.sort(key=lambda d: d["label"])
        for r, d in zip(recs, dets_o):
            assert r["label"] == d["label"] and r["area"] == d["area"] and np.array_equal(r["box"].reshape(4, 2), d["box"])
            assert (r["d1"], r["d2"], r["d_mean"]) == (d["d1"], d["d2"], d["d_mean"])
            assert (float(r["cx"]), float(r["cy"])) == (float(F(d["center"][0])), float(F(d["center"][1])))
            if kind == "quad":
                assert r["valid"] == 1 and r["branch"] == GC.BRANCH[d["branch"]] and r["contour_n"] == len(d["contour"])
            else:
                assert r["hull_n"] == len(d["hull"])


def test_case_list_is_complete_and_names_are_unique():
    cases = GC.all_cases()
    names = [f"{c.family}-{c.name}" for c in cases]
    assert len(names) == len(set(names))
    assert {c.family for c in cases} == {"topology", "edges", "limits", "compaction", "hull", "degenerate", "branches", "capacity",
                                         "morphology", "threshold", "batch"}
    assert GC.batch_case().probs().shape == (5, GC.TOPO_H, GC.TOPO_W)
