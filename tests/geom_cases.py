"""Built cases and composed references for the geometry kernels of csrc/geometry.hip (vk_geom_minarearect, vk_geom_quadrilateral): no
GPU is needed to import this module; tests/test_geom_cases_cpu.py proves the cases on the references alone, tests/test_geom_sweep_gpu.py
runs the kernels on them.  Same method as tests/conv_lattice.py and tests/tail_cases.py.

Everything the kernels do is integer work or float32 in a fixed order, so every comparison is equality: clean mask, counts, label ids,
areas, hull sizes, int32 corners, centre / size / direction as float32 BIT PATTERNS, float64 diagonals; for the 4-vertex fit also valid,
branch, candidate count, border length, flags and the float64 quality.

REFERENCES are composed from the oracle's stages (binarize, open_close, label8, convex_hull, min_area_rect, diagonals; for the fit
dilate, trace_external_contour, convex_hull_cv, approxPolyDP, the quality ranking) because the oracle's postprocess_*_multi fix the
area floor at 200 px.  Three things are this module's own and are proved by the CPU file:
  * components are split by one stable sort of the label image (not one `labels == i` scan per component);
  * a component of more than HULL_PREFILTER pixels reaches convex_hull as its per-COLUMN extremes (the device works from per-ROW
    extremes, so hull agreement stays a check of two different reductions);
  * the fit of one component runs on the component's bounding box grown by the dilation radius and clipped to the map, and
    `quad_fit` restates robust_quadrilateral_from_contour so that the border candidate can be left out: what the kernel documents for a
    border longer than its 16,384-point buffer (flags bit 0).  With the border candidate in, quad_fit must equal the oracle.

The ctypes helper `run_device` mirrors geometry.py's calls with a free min_area and max_components, fills `dets` and `counts` with 0xA5
bytes, places `clean` inside a larger buffer, fills the workspace with 0xA5 too and appends a 256-byte guard to every buffer."""
from __future__ import annotations

import ctypes as C
import importlib
import math
from collections import OrderedDict
from dataclasses import dataclass, field
from types import SimpleNamespace
from typing import Callable

import numpy as np

from oracle import geometry_oracle as G
from oracle import quad_oracle as Q

F = np.float32
GQ_NC = 16384                 # capacity of the border buffer of k_geom_quad (include/vk_unet.h: flags bit 0)
GEOM_MAX_H = 4096
SENT = 0xA5
GUARD = 256
HULL_PREFILTER = 20000
BRANCH = {"none": 0, "bisection": 1, "subsample": 2, "extremes": 3}

DET_DT = np.dtype([("label", "<i4"), ("area", "<i4"), ("box", "<i4", (8,)), ("cx", "<f4"), ("cy", "<f4"), ("rw", "<f4"), ("rh", "<f4"),
                   ("ux", "<f4"), ("uy", "<f4"), ("hull_n", "<i4"), ("reserved", "<i4"), ("d1", "<f8"), ("d2", "<f8"), ("d_mean", "<f8")])
QUAD_DT = np.dtype([("label", "<i4"), ("area", "<i4"), ("box", "<i4", (8,)), ("cx", "<f4"), ("cy", "<f4"), ("valid", "<i4"),
                    ("branch", "<i4"), ("n_candidates", "<i4"), ("contour_n", "<i4"), ("hull_n", "<i4"), ("flags", "<i4"),
                    ("quality", "<f8"), ("d1", "<f8"), ("d2", "<f8"), ("d_mean", "<f8")])
assert DET_DT.itemsize == 96 and QUAD_DT.itemsize == 104


@dataclass(frozen=True)
class Cfg:
    thresh: float = 0.5
    k: int = 1                # morph_kernel
    oi: int = 0
    ci: int = 0
    min_area: int = 1
    cap: int = 4096           # max_components
    outset: int = 0           # fit_outset_px (4-vertex fit only)


@dataclass(frozen=True)
class Case:
    """One call of the C ABI: `build()` -> float32 [B][h][w] (or [h][w]).  `paths`: which entry points run on it.  `expect`: what the
    CPU file proves about the case on the reference alone (component count, areas, branch names ...)."""
    name: str
    family: str
    build: Callable[[], np.ndarray] = field(compare=False, repr=False)
    cfg: Cfg = Cfg()
    paths: tuple = ("rect",)
    expect: dict = field(default_factory=dict, compare=False, repr=False)

    def probs(self) -> np.ndarray:
        p = np.asarray(self.build())
        p = p.astype(np.float32) if p.dtype != np.float32 else p
        return np.ascontiguousarray(p[None] if p.ndim == 2 else p)


# ================================================================================================ references
def front(prob: np.ndarray, cfg: Cfg):
    """steps 1-3 on one map: (mask uint8 {0, 255}, labels int32, areas int64 [N + 1])."""
    mask = G.binarize(prob, cfg.thresh)
    if cfg.k > 1 and (cfg.oi or cfg.ci):
        mask = G.open_close(mask, cfg.k, cfg.oi, cfg.ci)
    labels, areas = G.label8(mask)
    return mask, labels, areas


def column_extremes(pts: np.ndarray) -> np.ndarray:
    """For every x the points of smallest and of largest y: a subset with the same convex hull."""
    o = np.lexsort((pts[:, 1], pts[:, 0]))
    p = pts[o]
    first = np.r_[True, p[1:, 0] != p[:-1, 0]]
    last = np.r_[first[1:], True]
    return p[first | last]


def edge_areas(hull: np.ndarray) -> np.ndarray:
    """float32 area of the enclosing rectangle on every hull edge, operation by operation as geometry_oracle.min_area_rect forms it
    (that function keeps only the winner; the CPU file needs all of them to count exact ties)."""
    m = len(hull)
    hx, hy = hull[:, 0].astype(F), hull[:, 1].astype(F)
    out = np.empty(m, dtype=F)
    for i in range(m):
        j = (i + 1) % m
        dx, dy = F(hx[j] - hx[i]), F(hy[j] - hy[i])
        ln = np.sqrt(F(F(dx * dx) + F(dy * dy)), dtype=F)
        ux, uy = F(dx / ln), F(dy / ln)
        vx, vy = F(-uy), ux
        s = (hx * ux).astype(F) + (hy * uy).astype(F)
        t = (hx * vx).astype(F) + (hy * vy).astype(F)
        out[i] = F(F(s.max() - s.min()) * F(t.max() - t.min()))
    return out


def rect_record(label: int, area: int, xs: np.ndarray, ys: np.ndarray) -> np.ndarray:
    pts = np.stack([xs, ys], axis=1)
    if len(pts) > HULL_PREFILTER:
        pts = column_extremes(pts)
    hull = G.convex_hull(pts)
    rect = G.min_area_rect(hull)
    box = rect["corners"].astype(np.int32)
    d1, d2 = G.diagonals(box)
    r = np.zeros((), dtype=DET_DT)
    r["label"], r["area"], r["box"], r["hull_n"] = label, area, box.reshape(8), len(hull)
    r["cx"], r["cy"] = rect["center"]
    r["rw"], r["rh"] = rect["size"]
    r["ux"], r["uy"] = rect["u"]
    r["d1"], r["d2"], r["d_mean"] = d1, d2, 0.5 * (d1 + d2)
    return r


def quad_fit(cnt: np.ndarray, use_contour: bool = True, max_iter: int = Q.MAX_ITER):
    """quad_oracle.robust_quadrilateral_from_contour restated from the oracle's own pieces, with one switch: use_contour=False leaves
    the border polygon out of the bisection and of the sub-sampling (the hull candidate and both fall-backs still run).
    Returns (quad float32 [4][2] or None, branch name, number of candidates)."""
    pts = np.asarray(cnt).reshape(-1, 2).astype(F)
    if pts.shape[0] < 4:
        return None, "none", 0
    hull = Q.convex_hull_cv(pts.astype(np.int32)).astype(F)
    polys = ([pts] if use_contour else []) + [hull]

    def ok(cand):
        return Q.poly_area(cand) > 10 and Q.is_convex_quad(cand)

    def bisect(poly):
        peri = Q.arc_length_closed(poly)
        lo, hi = 0.001 * peri, 0.08 * peri
        for _ in range(max_iter):
            mid = 0.5 * (lo + hi)
            appr = Q.approx_poly_dp_closed(poly, mid)
            if len(appr) == 4:
                cand = Q.order_quad_cw(appr)
                if ok(cand):
                    return cand
                lo = mid
            elif len(appr) > 4:
                lo = mid
            else:
                hi = mid
            if abs(hi - lo) < 1e-6:
                break
        return None

    cands, branch = [c for c in (bisect(p) for p in polys) if c is not None], "bisection"
    if not cands:
        branch = "subsample"
        for poly in polys:
            appr = Q.approx_poly_dp_closed(poly, 0.01 * Q.arc_length_closed(poly))
            k = len(appr)
            if k > 4:
                for s in range(min(12, k)):
                    cand = Q.order_quad_cw(appr[np.arange(s, s + 4) % k])
                    if ok(cand):
                        cands.append(cand)
    if not cands:
        branch = "extremes"
        xs, ys = hull[:, 0], hull[:, 1]
        raw = np.array([hull[int(np.argmin(ys))], hull[int(np.argmax(xs))], hull[int(np.argmax(ys))], hull[int(np.argmin(xs))]], dtype=F)
        cand = Q.order_quad_cw(raw)
        if Q.poly_area(cand) > 10:
            cands.append(cand)
    if not cands:
        return None, "none", 0
    best, best_key = None, None
    for q in cands:
        key = (Q.quad_quality(q), Q.poly_area(q))
        if best is None or key > best_key:
            best, best_key = q, key
    return best, branch, len(cands)


def fit_contour(xs: np.ndarray, ys: np.ndarray, h: int, w: int, outset: int) -> np.ndarray:
    """External border of one component dilated by the fit element, traced on the component's bounding box grown by the element's
    radius and clipped to the map (the dilation exists inside the map only), in map coordinates."""
    kk = max(3, 2 * outset + 1) if outset > 0 else 1
    r = kk // 2
    y0, y1 = max(int(ys.min()) - r, 0), min(int(ys.max()) + r, h - 1)
    x0, x1 = max(int(xs.min()) - r, 0), min(int(xs.max()) + r, w - 1)
    sub = np.zeros((y1 - y0 + 1, x1 - x0 + 1), dtype=np.uint8)
    sub[ys - y0, xs - x0] = 255
    if outset > 0:
        sub = G.dilate(sub, G.ellipse_kernel(kk))
    return Q.trace_external_contour(sub) + np.array([x0, y0], dtype=np.int32)


def quad_record(label: int, area: int, xs, ys, h: int, w: int, outset: int) -> np.ndarray:
    cnt = fit_contour(xs, ys, h, w, outset)
    over = len(cnt) > GQ_NC
    quad, branch, ncand = quad_fit(cnt, use_contour=not over)
    r = np.zeros((), dtype=QUAD_DT)
    r["label"], r["area"], r["contour_n"], r["hull_n"] = label, area, len(cnt), len(Q.convex_hull_cv(cnt))
    r["flags"] = 1 if over else 0
    r["n_candidates"] = ncand
    if quad is not None:
        box = Q.order_quad_cw(quad).astype(np.int32)
        d1, d2 = Q.quad_diagonals(box)
        r["valid"], r["branch"], r["box"] = 1, BRANCH[branch], box.reshape(8)
        r["cx"], r["cy"] = F(float(np.mean(box[:, 0]))), F(float(np.mean(box[:, 1])))
        r["quality"] = Q.quad_quality(quad)
        r["d1"], r["d2"], r["d_mean"] = d1, d2, 0.5 * (d1 + d2)
    return r


class MapRef:
    """Reference of ONE map under one Cfg's front end; records are made on demand and kept, so calls that differ in min_area or
    max_components only (and the two entry points) share the labelling and the per-component work."""

    def __init__(self, prob: np.ndarray, cfg: Cfg):
        self.h, self.w = prob.shape
        self.mask, self.labels, self.areas = front(prob, cfg)
        self.n = len(self.areas) - 1
        self._order = np.argsort(self.labels.ravel(), kind="stable")
        self._bounds = np.cumsum(self.areas)
        self._rect, self._quad = {}, {}

    def pixels(self, label: int):
        idx = self._order[self._bounds[label - 1]:self._bounds[label]]
        return idx % self.w, idx // self.w

    def kept(self, min_area: int):
        return [i for i in range(1, self.n + 1) if self.areas[i] >= min_area]

    def clean(self, min_area: int) -> np.ndarray:
        keep = self.areas >= min_area
        keep[0] = False
        return keep[self.labels].astype(np.uint8) * np.uint8(255)

    def rect(self, label: int) -> np.ndarray:
        if label not in self._rect:
            xs, ys = self.pixels(label)
            self._rect[label] = rect_record(label, int(self.areas[label]), xs, ys)
        return self._rect[label]

    def quad(self, label: int, outset: int) -> np.ndarray:
        if (label, outset) not in self._quad:
            xs, ys = self.pixels(label)
            self._quad[(label, outset)] = quad_record(label, int(self.areas[label]), xs, ys, self.h, self.w, outset)
        return self._quad[(label, outset)]

    def expected(self, kind: str, cfg: Cfg):
        """(clean, count, records [min(count, cap)] in label order) of one call."""
        kept = self.kept(cfg.min_area)
        listed = kept[:cfg.cap]
        if kind == "rect":
            recs = np.array([self.rect(i) for i in listed], dtype=DET_DT).reshape(-1)
        else:
            recs = np.array([self.quad(i, cfg.outset) for i in listed], dtype=QUAD_DT).reshape(-1)
        return self.clean(cfg.min_area), len(kept), recs


_REFS: OrderedDict = OrderedDict()


def map_refs(case: Case):
    """[MapRef per map] of a case, shared by every test on a case with the same maps and front end (a few are kept)."""
    key = (case.family, case.name.split("@")[0], case.cfg.thresh, case.cfg.k, case.cfg.oi, case.cfg.ci)
    if key not in _REFS:
        _REFS[key] = [MapRef(p, case.cfg) for p in case.probs()]
        while len(_REFS) > 4:
            _REFS.popitem(last=False)
    return _REFS[key]


# ================================================================================================ the device call
def run_device(kind: str, probs: np.ndarray, cfg: Cfg, device="cuda:0"):
    """vk_geom_minarearect (kind "rect") / vk_geom_quadrilateral ("quad") as geometry.py calls them, into sentinel-filled buffers.
    Returns clean uint8 [B][h][w], counts int32 [B], recs structured [B][cap], raw uint8 [B][cap][record bytes], guards_ok."""
    import torch

    L = importlib.import_module("vickers-hardness-unet_amd._lib")
    lib = L.lib()
    dev = torch.device(device)
    t = torch.from_numpy(np.ascontiguousarray(probs, dtype=np.float32)).to(dev)
    B, h, w = (int(v) for v in t.shape)
    desc = L.vk_geom_desc(h, w, float(cfg.thresh), int(cfg.k), int(cfg.oi), int(cfg.ci), int(cfg.min_area), int(cfg.cap))
    nbytes = int(lib.vk_geom_workspace_bytes(C.byref(desc), B))
    assert nbytes > 0, lib.vk_last_error_string()
    dt = DET_DT if kind == "rect" else QUAD_DT
    n, nrec = B * h * w, B * cfg.cap * dt.itemsize

    def sentinel(nb):
        return torch.full((nb + 2 * GUARD,), SENT, dtype=torch.uint8, device=dev)

    ws, cbuf, dbuf, nbuf = sentinel(nbytes), sentinel(n), sentinel(nrec), sentinel(4 * B)
    args = (B, t.data_ptr(), cbuf.data_ptr() + GUARD, dbuf.data_ptr() + GUARD, nbuf.data_ptr() + GUARD, ws.data_ptr() + GUARD, nbytes,
            L.current_stream())
    if kind == "rect":
        L.check(lib.vk_geom_minarearect(C.byref(desc), *args), "vk_geom_minarearect")
    else:
        L.check(lib.vk_geom_quadrilateral(C.byref(desc), int(cfg.outset), *args), "vk_geom_quadrilateral")
    torch.cuda.synchronize()

    def guards(buf, nb):
        return bool((buf[:GUARD] == SENT).all().item()) and bool((buf[GUARD + nb:] == SENT).all().item())

    ok = guards(ws, nbytes) and guards(cbuf, n) and guards(dbuf, nrec) and guards(nbuf, 4 * B)
    clean = cbuf[GUARD:GUARD + n].reshape(B, h, w).cpu().numpy()
    raw = dbuf[GUARD:GUARD + nrec].cpu().numpy().reshape(B, cfg.cap, dt.itemsize)
    counts = nbuf[GUARD:GUARD + 4 * B].cpu().numpy().view(np.int32).copy()
    recs = raw.reshape(-1).view(dt).reshape(B, cfg.cap)
    return SimpleNamespace(clean=clean, counts=counts, recs=recs, raw=raw, guards_ok=ok)


def bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def assert_records_equal(got: np.ndarray, exp: np.ndarray, tag=""):
    """Every field, floats by bit pattern; the message names the first record and field that differ."""
    assert got.shape == exp.shape, (tag, got.shape, exp.shape)
    if got.tobytes() == exp.tobytes():
        return
    for name in got.dtype.names:
        g, e = got[name], exp[name]
        same = (bits(g) == bits(e)) if g.dtype.kind == "f" else (g == e)
        if not np.all(same):
            i = int(np.argwhere(~same.reshape(len(got), -1).all(axis=1))[0, 0])
            raise AssertionError(f"{tag}: record {i} (label {int(exp['label'][i])}) field {name}: device {g[i]!r} != reference {e[i]!r}"
                                 f" (device {got[i]}, reference {exp[i]})")
    raise AssertionError(f"{tag}: records differ in padding bytes")


def check_call(kind: str, case: Case, res, refs=None):
    """Holds one device call against the references of its maps: clean, counts, the listed records, untouched slots, guards."""
    refs = refs if refs is not None else map_refs(case)
    cfg = case.cfg
    assert res.guards_ok, f"{case.name}: a guard byte outside clean / dets / counts / workspace was written"
    for b, ref in enumerate(refs):
        clean, count, recs = ref.expected(kind, cfg)
        tag = f"{case.name}[{kind}] map {b}"
        assert int(res.counts[b]) == count, (tag, int(res.counts[b]), count)
        assert np.array_equal(res.clean[b], clean), (tag, "clean differs at", np.argwhere(res.clean[b] != clean)[:4].tolist())
        nl = min(count, cfg.cap)
        assert_records_equal(res.recs[b, :nl], recs, tag)
        assert bool((res.raw[b, nl:] == SENT).all()), f"{tag}: a slot at or above min(counts, max_components) = {nl} was written"


# ================================================================================================ builders: topologies
TOPO_H, TOPO_W = 37, 131


def serpentine(h=TOPO_H, w=TOPO_W):
    m = np.zeros((h, w), bool)
    m[0::2] = True
    for i, y in enumerate(range(1, h, 2)):
        m[y, w - 1 if i % 2 == 0 else 0] = True
    return m


def spiral(h=TOPO_H, w=TOPO_W):
    """One-pixel rectangular spiral with one-pixel gaps, walked from the top-left corner inwards."""
    m = np.zeros((h, w), bool)
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = True

    def free(yy, xx):
        """(yy, xx) may be entered: inside the map, and the cell after it in the same direction is not already set"""
        if not (0 <= yy < h and 0 <= xx < w) or m[yy, xx]:
            return False
        y2, x2 = yy + dy, xx + dx
        return not (0 <= y2 < h and 0 <= x2 < w and m[y2, x2])

    turns = 0
    while turns < 2:
        if free(y + dy, x + dx):
            y, x = y + dy, x + dx
            m[y, x] = True
            turns = 0
        else:
            dy, dx = dx, -dy          # turn right on screen: E -> S -> W -> N
            turns += 1
    return m


def comb(spine_bottom: bool, phase: int, h=TOPO_H, w=TOPO_W):
    m = np.zeros((h, w), bool)
    m[:, phase::2] = True
    m[0 if spine_bottom else h - 1] = False
    m[h - 1 if spine_bottom else 0] = True
    return m


def teeth_63_64_65(h=TOPO_H, w=TOPO_W):
    """Spine on the bottom row; three adjacent teeth of different heights at x = 63, 64, 65 (either side of the wave boundary) and
    two lone ones at x = 61 and x = 67 that reach the top."""
    m = np.zeros((h, w), bool)
    m[h - 1] = True
    m[5:, 63] = True
    m[15:, 64] = True
    m[25:, 65] = True
    m[:, 61] = True
    m[:, 67] = True
    return m


def checker(h=TOPO_H, w=TOPO_W):
    yy, xx = np.mgrid[0:h, 0:w]
    return (xx + yy) % 2 == 0


def dots(h=TOPO_H, w=TOPO_W):
    yy, xx = np.mgrid[0:h, 0:w]
    return (xx % 2 == 0) & (yy % 2 == 0)


def stairs(anti: bool, h=TOPO_H, w=TOPO_W):
    """Parallel one-pixel diagonals three columns apart: every component hangs together through one kind of diagonal union only."""
    yy, xx = np.mgrid[0:h, 0:w]
    return ((xx + yy) if anti else (xx - yy)) % 3 == 0


def stairs_areas(anti: bool, h=TOPO_H, w=TOPO_W):
    """Areas in label order, from the construction: the line x - y = c (or x + y = c) holds one pixel per row it crosses."""
    out = []
    for c in (range(0, h + w - 1, 3) if anti else range(-((h - 1) // 3) * 3, w, 3)):
        ys = [y for y in range(h) if 0 <= ((c - y) if anti else (c + y)) < w]
        x0 = (c - ys[0]) if anti else (c + ys[0])
        out.append((ys[0], x0, len(ys)))
    return [n for _, _, n in sorted(out)]


def rings(h=TOPO_H, w=TOPO_W):
    m = np.zeros((h, w), bool)
    for d in (2, 4):
        m[d, d:w - d] = m[h - 1 - d, d:w - d] = True
        m[d:h - d, d] = m[d:h - d, w - 1 - d] = True
    return m


def letter_u(h=TOPO_H, w=TOPO_W):
    m = np.zeros((h, w), bool)
    m[:, 1] = m[:, w - 2] = True
    m[h - 1, 1:w - 1] = True
    return m


def letter_w(h=TOPO_H, w=TOPO_W):
    m = letter_u(h, w)
    m[3:, 64] = True
    return m


def bars(h=TOPO_H, w=TOPO_W):
    m = np.zeros((h, w), bool)
    m[0::2] = True
    return m


def _ring_area(h, w, d):
    return 2 * ((h - 2 * d) + (w - 2 * d)) - 4


# name -> (builder, areas in label order for the base orientation)
TOPOLOGIES = {
    "serpentine": (serpentine, None),
    "spiral": (spiral, None),
    "comb_spine_bottom": (lambda: comb(True, 0), None),
    "comb_spine_top": (lambda: comb(False, 1), None),
    "teeth_63_64_65": (teeth_63_64_65, None),
    "checker_diagonals_only": (checker, None),
    "isolated_dots": (dots, [1] * (((TOPO_H + 1) // 2) * ((TOPO_W + 1) // 2))),
    "stairs_diagonal": (lambda: stairs(False), stairs_areas(False)),
    "stairs_antidiagonal": (lambda: stairs(True), stairs_areas(True)),
    "nested_rings": (rings, [_ring_area(TOPO_H, TOPO_W, 2), _ring_area(TOPO_H, TOPO_W, 4)]),
    "letter_u": (letter_u, None),
    "letter_w": (letter_w, None),
    "full_width_bars": (bars, [TOPO_W] * ((TOPO_H + 1) // 2)),
    "all_foreground": (lambda: np.ones((TOPO_H, TOPO_W), bool), [TOPO_H * TOPO_W]),
    "all_background": (lambda: np.zeros((TOPO_H, TOPO_W), bool), []),
}
VARIANTS = {"base": lambda m: m, "transposed": lambda m: m.T, "mirrored": lambda m: m[:, ::-1]}


def topology_cases():
    out = []
    for name, (fn, areas) in TOPOLOGIES.items():
        for vname, vf in VARIANTS.items():
            exp = {"ncomp": len(areas) if areas is not None else 1}
            if areas is not None and (vname == "base" or len(set(areas)) <= 1):
                exp["areas"] = areas
            elif areas is not None:
                exp["areas_sorted"] = sorted(areas)
            else:
                exp["single"] = True                      # one component holding every foreground pixel
            # 1,254 dots are 1,254 full fits on the host: the fit sees them through a list of 200 (below), the rectangle path sees all
            paths = ("rect",) if name == "isolated_dots" else ("rect", "quad")
            out.append(Case(f"{name}-{vname}", "topology", (lambda fn=fn, vf=vf: vf(fn())), Cfg(outset=1), paths, exp))
    out.append(Case("isolated_dots-base@cap200", "topology", dots, Cfg(cap=200, outset=1), ("quad",), {"ncomp": len(TOPOLOGIES["isolated_dots"][1])}))
    return out


# ================================================================================================ builders: map edges, limits
EDGE_H = (1, 2, 3, 5, 7, 37, 130)
EDGE_W = (1, 2, 63, 64, 65, 127, 129)
DENSITIES = (0.3, 0.55, 0.9)


def noise(h, w, density, seed):
    return np.random.default_rng(seed).random((h, w)) < density


def edge_shapes():
    s = []
    for a in EDGE_H:
        for b in EDGE_W:
            if a != b:
                s += [(a, b), (b, a)]
    return sorted(set(s))


def edge_cases():
    """Per map size one batch of three seeded Bernoulli maps (densities 0.3, 0.55, 0.9), called with min_area 1 and 3; the fit runs
    on the min_area 3 call with a one-pixel outset, so its dilation meets every map border."""
    out = []
    for h, w in edge_shapes():
        build = (lambda h=h, w=w: np.stack([noise(h, w, d, 1000 * h + w + i) for i, d in enumerate(DENSITIES)]))
        out.append(Case(f"noise_{h}x{w}@area1", "edges", build, Cfg(min_area=1)))
        out.append(Case(f"noise_{h}x{w}@area3", "edges", build, Cfg(min_area=3, outset=1), ("rect", "quad")))
    return out


def full_height_line():
    return np.ones((GEOM_MAX_H, 1), bool)


def zigzag():
    m = np.zeros((GEOM_MAX_H, 3), bool)
    m[np.arange(GEOM_MAX_H), np.array([0, 1, 2, 1])[np.arange(GEOM_MAX_H) % 4]] = True
    return m


def one_row():
    return noise(1, 16384, 0.55, 16384)


def three_rows():
    m = np.zeros((3, 16384), bool)
    m[0] = True                                     # one run across the whole row: 256 waves joined through lane 0
    m[1] = noise(1, 16384, 0.02, 31)[0]
    m[2] = noise(1, 16384, 0.5, 32)[0]
    return m


def limit_cases():
    return [Case("line_4096x1", "limits", full_height_line, Cfg(cap=4), ("rect", "quad"), {"ncomp": 1}),
            Case("zigzag_4096x3", "limits", zigzag, Cfg(cap=4), ("rect", "quad"), {"ncomp": 1}),
            Case("noise_1x16384", "limits", one_row, Cfg(cap=4096)),
            Case("rows_3x16384", "limits", three_rows, Cfg(cap=4096))]


# ================================================================================================ builders: compaction
def compaction_cases():
    d130 = lambda: dots(130, 130)                                                               # noqa: E731
    exp = {"ncomp": 65 * 65}
    return [Case("dots_130x130@cap4096", "compaction", d130, Cfg(cap=4096), ("rect",), exp),
            Case("dots_130x130@cap1", "compaction", d130, Cfg(cap=1), ("rect", "quad"), exp),
            Case("dots_130x130@cap4095", "compaction", d130, Cfg(cap=4095), ("rect",), exp),
            Case("noise_520x520", "compaction", lambda: noise(520, 520, 0.3, 520), Cfg(cap=4096), ("rect",), {"nchunk": 265}),
            Case("noise_520x520@area9", "compaction", lambda: noise(520, 520, 0.3, 520), Cfg(min_area=9, cap=4096), ("rect",)),
            Case("dots_1x128", "compaction", lambda: dots(1, 128), Cfg(cap=64), ("rect",), {"ncomp": 64, "roots_per_64": 32}),
            Case("dots_1x2048", "compaction", lambda: dots(1, 2048), Cfg(cap=4096), ("rect",), {"ncomp": 1024, "roots_per_1024": 512})]


# ================================================================================================ builders: hull and calipers
def lattice_polygon(K: int) -> np.ndarray:
    """Convex lattice polygon whose edges are ALL primitive vectors (dx, dy), |dx|, |dy| <= K, sorted by angle and summed: int64 [n][2]
    (x, y) shifted to touch x = 0 and y = 0, in the canonical order of geometry_oracle.convex_hull (from the top-most then left-most
    vertex, down the left side).  The edge set is invariant under the eight symmetries of the square, so the polygon is."""
    vec = [(dx, dy) for dx in range(-K, K + 1) for dy in range(-K, K + 1) if math.gcd(dx, dy) == 1]
    # on screen (y down) the canonical walk leaves the top-left vertex leftwards-and-down and ends along the top edge, direction
    # (-1, 0): edge directions by increasing angle measured from (-1, 0), turning towards +y, with (-1, 0) itself last
    v = np.array(vec, dtype=np.int64)
    ang = np.arctan2(v[:, 1], -v[:, 0])
    v = v[np.argsort(np.where(ang <= 0, ang + 2 * np.pi, ang), kind="stable")]
    p = np.concatenate([np.zeros((1, 2), np.int64), np.cumsum(v, axis=0)[:-1]])
    p -= p.min(axis=0)
    start = min(range(len(p)), key=lambda i: (p[i, 1], p[i, 0]))
    return np.roll(p, -start, axis=0)


def fill_convex(poly: np.ndarray, h: int, w: int, ox: int = 0, oy: int = 0) -> np.ndarray:
    """Scanline fill of a convex lattice polygon (boundary included) with integer arithmetic: per row the smallest and largest
    x that any edge or vertex reaches on that row."""
    lo = np.full(h, w, dtype=np.int64)
    hi = np.full(h, -1, dtype=np.int64)
    n = len(poly)
    for i in range(n):
        (xa, ya), (xb, yb) = poly[i], poly[(i + 1) % n]
        if ya == yb:
            y = ya + oy
            lo[y] = min(lo[y], min(xa, xb) + ox)
            hi[y] = max(hi[y], max(xa, xb) + ox)
            continue
        if ya > yb:
            xa, ya, xb, yb = xb, yb, xa, ya
        ys = np.arange(ya, yb + 1)
        num = xa * (yb - ya) + (ys - ya) * (xb - xa)          # x * (yb - ya) on the edge at row ys
        den = yb - ya
        fl, ce = num // den, -((-num) // den)
        # a convex polygon lies on one side of each edge: the row's interior starts at ceil on a left edge, ends at floor on a right edge;
        # taking min over ceil and max over floor of all edges crossing the row gives exactly the lattice points inside
        np.minimum.at(lo, ys + oy, ce + ox)
        np.maximum.at(hi, ys + oy, fl + ox)
    xs = np.arange(w)[None, :]
    return (xs >= lo[:, None]) & (xs <= hi[:, None])


def polygon_map(K: int, corner: bool) -> np.ndarray:
    p = lattice_polygon(K)
    e = int(p.max()) + 1
    if corner:                                          # off-centre, touching the top-left corner of a map with a ragged far side
        return fill_convex(p, e + 5, e + 7)
    return fill_convex(p, e + 6, e + 6, 3, 3)


def chord_polygon(K: int, j: int) -> np.ndarray:
    """Vertices 0 .. j of the lattice polygon closed by one chord (edge j, from vertex j back to vertex 0): the symmetry that gives
    every minimal edge of the full polygon a tied twin of lower index is gone, and for the (K, j) of CHORDS the chord is the ONLY
    minimal edge of the calipers, at an index that the 256-thread stride loop reaches on its second trip."""
    q = lattice_polygon(K)[:j + 1].copy()
    return q - q.min(axis=0)


CHORDS = ((11, 270), (14, 400))


def chord_map(K: int, j: int) -> np.ndarray:
    q = chord_polygon(K, j)
    return fill_convex(q, int(q[:, 1].max()) + 4, int(q[:, 0].max()) + 6, 2, 1)


def hull_cases(ks=(4, 10, 11, 14)):
    out = [Case(f"chord_K{K}_j{j}", "hull", (lambda K=K, j=j: chord_map(K, j)), Cfg(cap=2), ("rect",), {"chord": (K, j), "ncomp": 1})
           for K, j in CHORDS]
    for K in ks:
        for corner in (False, True):
            paths = ("rect", "quad") if K <= 10 else ("rect",)
            out.append(Case(f"lattice_K{K}_{'corner' if corner else 'centred'}", "hull", (lambda K=K, c=corner: polygon_map(K, c)),
                            Cfg(cap=2, outset=0), paths, {"K": K, "corner": corner, "ncomp": 1}))
    return out


# ================================================================================================ builders: degenerate components
def _line(kind: str, n: int):
    h, w = n + 9, n + 71
    m = np.zeros((h, w), bool)
    i = np.arange(n)
    if kind == "horizontal":
        m[3, 60 + i] = True
    elif kind == "vertical":
        m[3 + i, 64] = True
    elif kind == "diagonal":
        m[3 + i, 60 + i] = True
    else:
        m[3 + i, 60 + n - 1 - i] = True
    return m


def _small(kind: str):
    m = np.zeros((9, 71), bool)
    if kind == "pixel":
        m[4, 64] = True
    elif kind == "square2":
        m[4:6, 63:65] = True
    else:                                               # two-pixel diagonal in the map corner
        m[0, 0] = m[1, 1] = True
    return m


def degenerate_cases():
    out = []
    shapes = [("pixel", lambda: _small("pixel"), {"valid": 0}), ("square2", lambda: _small("square2"), {"branch": "none", "n_candidates": 0}),
              ("corner_diagonal2", lambda: _small("corner"), {"valid": 0})]
    for kind in ("horizontal", "vertical", "diagonal", "antidiagonal"):
        for n in (2, 7, 250):
            shapes.append((f"{kind}{n}", (lambda kind=kind, n=n: _line(kind, n)), {"valid": 0}))
    for name, fn, quad in shapes:
        out.append(Case(f"{name}-plain", "degenerate", fn, Cfg(cap=4), ("rect", "quad"), {"ncomp": 1, "quad": quad}))
        out.append(Case(f"{name}-close1", "degenerate", fn, Cfg(k=3, oi=0, ci=1, cap=4), ("rect", "quad"), {}))
    return out


def flat_triangle():
    """tests/test_quad_cpu.py::test_extreme_point_fallback as a mask: a 101-pixel row with one pixel under its middle."""
    m = np.zeros((5, 110), bool)
    m[1, 3:104] = True
    m[2, 53] = True
    return m


def pentagon():
    """tests/test_quad_cpu.py::test_pentagon_falls_to_subsampling_and_ranking_is_stable, at a smaller radius."""
    S = 90
    yy, xx = np.mgrid[0:S, 0:S].astype(np.float64)
    pts = [(45 + 35 * math.cos(0.2 + 2 * math.pi * k / 5), 45 + 35 * math.sin(0.2 + 2 * math.pi * k / 5)) for k in range(5)]
    m = np.ones((S, S), bool)
    for i in range(5):
        a, b = pts[i], pts[(i + 1) % 5]
        m &= ((b[0] - a[0]) * (yy - a[1]) - (b[1] - a[1]) * (xx - a[0])) >= 0
    return m


def branch_cases():
    return [Case("flat_triangle", "branches", flat_triangle, Cfg(cap=2), ("quad",), {"quad": {"valid": 1, "branch": "extremes"}}),
            Case("pentagon", "branches", pentagon, Cfg(cap=2, outset=2), ("quad",), {"quad": {"valid": 1, "branch": "subsample"}}),
            Case("square2", "branches", lambda: _small("square2"), Cfg(cap=2), ("quad",), {"quad": {"valid": 0, "branch": "none", "n_candidates": 0}})]


# ================================================================================================ builders: contour capacity
def crenellated_bar(W: int):
    m = np.zeros((8, W + 2), bool)
    m[2:6, 1:W + 1] = True
    m[1, 1:W + 1:2] = True
    m[6, 1:W + 1:2] = True
    return m


def capacity_cases():
    return [Case("crenellated_8000", "capacity", lambda: crenellated_bar(8000), Cfg(cap=2), ("rect", "quad"), {"contour_n": 16000, "flags": 0}),
            Case("crenellated_9000", "capacity", lambda: crenellated_bar(9000), Cfg(cap=2), ("quad",), {"contour_n": 18000, "flags": 1})]


# ================================================================================================ builders: morphology, threshold
MORPH_ITERS = ((16, 0), (0, 16), (3, 3), (16, 16))


def morph_maps():
    frame = np.ones((40, 70), bool)
    frame[0] = frame[-1] = False
    frame[:, 0] = frame[:, -1] = False
    return np.stack([noise(40, 70, 0.7, 4070), np.ones((40, 70), bool), frame])


def morph_cases():
    return [Case(f"k{k}_open{oi}_close{ci}", "morphology", morph_maps, Cfg(k=k, oi=oi, ci=ci), ("rect",), {"all_fg_map": 1})
            for k in (3, 5, 7) for oi, ci in MORPH_ITERS]


THRESHOLDS = (0.45, 0.5, 0.0, 1.0)


def special_values(t: float) -> np.ndarray:
    ft = F(t)
    return np.array([ft, np.nextafter(ft, F(np.inf)), np.nextafter(ft, F(-np.inf)), np.nan, np.inf, -np.inf, 0.0, -0.0], dtype=F)


def threshold_map(t: float) -> np.ndarray:
    """13 x 67: every special value many times, in seeded random places, among plain 0.25 / 0.75 pixels."""
    rng = np.random.default_rng(int(t * 100) + 7)
    vals = np.concatenate([special_values(t), np.array([0.25, 0.75] * 4, dtype=F)])
    return vals[rng.integers(0, len(vals), size=(13, 67))]


def threshold_cases():
    out = []
    for t in THRESHOLDS:
        build = (lambda t=t: threshold_map(t))
        out.append(Case(f"t{t}-binarize", "threshold", build, Cfg(thresh=t), ("rect",), {"t": t}))
        out.append(Case(f"t{t}-fused_open", "threshold", build, Cfg(thresh=t, k=3, oi=1, ci=0), ("rect",), {"t": t}))
        out.append(Case(f"t{t}-fused_close", "threshold", build, Cfg(thresh=t, k=3, oi=0, ci=1), ("rect",), {"t": t}))
    return out


# ================================================================================================ builders: batch isolation
def batch_maps():
    return np.stack([np.ones((TOPO_H, TOPO_W), bool), np.zeros((TOPO_H, TOPO_W), bool), serpentine(), dots(), noise(TOPO_H, TOPO_W, 0.5, 5)])


def batch_case():
    return Case("batch5_37x131", "batch", batch_maps, Cfg(cap=300, outset=1), ("rect", "quad"))       # the dots overflow the list


def all_cases():
    return (topology_cases() + edge_cases() + limit_cases() + compaction_cases() + hull_cases() + degenerate_cases() + branch_cases()
            + capacity_cases() + morph_cases() + threshold_cases() + [batch_case()])
