"""Built cases for vk.keypoints.  No GPU is needed to import this module: tests/test_keypoints_cpu.py checks the restatement
(tests/keypoints_ref.py) on them, tests/test_vk_keypoints_gpu.py holds the kernels to the restatement's bytes on them.

The maps are the smallest at which the kernels can go wrong: one pixel, one row, one column, exactly one 64 x 16 tile, partial tiles in
either direction, several tiles; a 1,024-pixel chunk of the peak kernels and more than one."""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache

import numpy as np

import keypoints_ref as R
import subpix_cases as SC

BARE_DT = np.dtype([("v", "<f8", (8,))])                      # a bare [B][M][8] vertex array: stride 64, no valid field
COMPACT_DT = np.dtype([("label", "<i4"), ("area", "<i4"), ("box", "<i4", (8,))])      # the least vk_kp_refine reads: stride 40
assert BARE_DT.itemsize == 64 and COMPACT_DT.itemsize == 40


def quad_records(v, valid=None) -> np.ndarray:
    """v float64 [B][M][8] -> vk_subpix_quad records with a pattern in the fields the calls do not read."""
    v = np.asarray(v, np.float64)
    B, M = v.shape[:2]
    raw = np.full((B, M, R.QUAD_DT.itemsize), 0x5A, np.uint8)
    r = raw.reshape(-1).view(R.QUAD_DT).reshape(B, M)
    r["v"] = v
    r["valid"] = 1 if valid is None else np.asarray(valid, np.int32)
    r["label"] = 1 + np.arange(M)[None, :]
    return r


def bare_records(v) -> np.ndarray:
    v = np.ascontiguousarray(np.asarray(v, np.float64))
    return v.reshape(v.shape[0], v.shape[1], 8).view(BARE_DT).reshape(v.shape[0], v.shape[1])


def compact_records(boxes) -> np.ndarray:
    boxes = np.asarray(boxes, np.int32)
    B, M = boxes.shape[:2]
    r = np.zeros((B, M), COMPACT_DT)
    r["box"] = boxes
    r["label"] = 1 + np.arange(M)[None, :] + 100 * np.arange(B)[:, None]
    r["area"] = 7 + 3 * np.arange(M)[None, :]
    return r


@lru_cache(maxsize=None)
def table(r16: int) -> np.ndarray:
    """R16 = 8: a steep table that ends after half a pixel; 96: sigma 2 at cutoff 3; 192: sigma 4, the largest."""
    return R.table_of_radius(r16, {8: 0.25, 96: 2.0, 192: 4.0}[r16])


# ------------------------------------------------------------------------------------------------ targets
@dataclass
class TargetCase:
    name: str
    h: int
    w: int
    recs: np.ndarray            # structured [B][M]
    counts: np.ndarray
    field: str                  # "box" (int32) or "v" (float64)
    vert_type: int
    r16: int

    def expected(self) -> np.ndarray:
        return R.targets_ref(self.recs, self.counts, self.h, self.w, table(self.r16), self.field, self.vert_type)


def _boxes(pts):
    """A flat list of (x, y) -> boxes [1][M][8], the last record padded with its own last point."""
    pts = list(pts)
    while len(pts) % 4:
        pts.append(pts[-1])
    return np.array(pts).reshape(1, -1, 8)


@lru_cache(maxsize=None)
def target_cases():
    out = []
    rng = np.random.default_rng(7)

    def add_i32(name, h, w, boxes, counts, r16, kind="rect", valid=None):
        boxes = np.asarray(boxes, np.int32)
        out.append(TargetCase(name, h, w, SC.records(kind, boxes, valid), np.asarray(counts, np.int32), "box", R.VERT_I32, r16))

    def add_f64(name, h, w, v, counts, r16, valid=None, bare=False):
        v = np.asarray(v, np.float64)
        recs = bare_records(v) if bare else quad_records(v, valid)
        out.append(TargetCase(name, h, w, recs, np.asarray(counts, np.int32), "v", R.VERT_F64, r16))

    # one pixel, one row, one column
    add_i32("1x1_on", 1, 1, _boxes([(0, 0), (1, 0), (0, 1), (5, 5)]), [1], 96)
    add_f64("1x1_near", 1, 1, _boxes([(0.4375, -0.25), (3.0, 0.0), (-6.0, 0.0), (0.0, 6.0625)]), [1], 96)
    add_i32("1x7", 1, 7, _boxes([(0, 0), (6, 0), (3, 2), (-4, 0)]), [1], 96)
    add_f64("7x1", 7, 1, _boxes([(0.0, 0.5), (0.0625, 6.0), (2.0, 3.0), (-1.0, -1.0)]), [1], 192, bare=True)
    # exactly at and one step past the cutoff, R16 = 8: D = 64 is the last entry, D = 65 = 8^2 + 1^2 is outside
    add_f64("cutoff_r8", 16, 16, _boxes([(3.5, 3.0), (8.5, 8.0625), (12.5625, 3.0), (3.0, 12.5)]), [1], 8, bare=True)
    add_i32("cutoff_r8_i32", 16, 16, _boxes([(3, 3), (15, 15), (0, 15), (16, 7)]), [1], 8)
    # one full tile, vertices on its corners and outside the map with the disc reaching in
    corners = [(0, 0), (63, 0), (0, 15), (63, 15), (-5, -5), (68, 7), (30, 21), (30, -6), (64, 16), (-6, 8), (200, 8), (31, 8)]
    add_i32("64x16_corners", 16, 64, _boxes(corners), [3], 96)
    add_f64("64x16_corners_f64", 16, 64, _boxes([(x + 0.28125, y - 0.4375) for x, y in corners]), [3], 96, valid=[[1, 0, 1]])
    # partial tiles both ways, several tiles; vertices on tile corners
    tile_pts = [(63, 15), (64, 16), (64, 15), (63, 16), (0, 16), (19, 23), (10, 5), (79, 71), (40, 40), (127, 31), (64, 48), (5, 70)]
    add_i32("20x24", 24, 20, _boxes(tile_pts[4:8] + [(19, 0), (0, 23), (9, 12), (25, 29)]), [2], 96, kind="quad", valid=[[1, 1]])
    add_i32("80x72_r96", 72, 80, _boxes(tile_pts), [3], 96, kind="quad", valid=[[1, 1, 1]])
    add_i32("80x72_r192", 72, 80, _boxes(tile_pts), [3], 192)
    add_f64("80x72_f64_r192", 72, 80, _boxes([(x + 0.53125, y + 0.96875) for x, y in tile_pts]), [3], 192)
    # B = 3: counts -1, 0, above the cap; valid == 0; non-finite and far coordinates
    b3 = rng.integers(-8, 88, size=(3, 3, 8))
    add_i32("batch3_counts", 72, 80, b3, [-1, 0, 9], 96)
    add_i32("batch3_valid", 72, 80, b3, [3, 2, 1], 96, kind="quad", valid=[[1, 0, 1], [0, 1, 1], [0, 0, 0]])
    v3 = rng.uniform(-8, 88, size=(3, 3, 8))
    v3[0, 0, 0], v3[0, 1, 3], v3[1, 0, 4], v3[1, 1, 1], v3[2, 0, 6], v3[2, 1, 7] = np.nan, np.inf, -np.inf, 1048576.5, -1048577.0, 1e300
    v3[2, 2, 0:2] = (1048576.0, 3.0)                                              # allowed, and far from everything
    add_f64("batch3_nonfinite", 72, 80, v3, [3, 3, 3], 96)
    add_f64("batch3_bare", 20, 24, rng.uniform(-3, 27, size=(3, 2, 8)), [2, 1, 5], 96, bare=True)
    big = np.array([[[2**31 - 1, 0, -2**31, 5, 7, 2**31 - 1, 7, -2**31], [3, 3, 4, 4, 5, 5, 6, 6]]])
    add_i32("int32_extremes", 16, 16, big, [2], 192)
    # 1,024 records on one tile: 4,096 vertices, sixteen rounds of the tile list
    many = rng.integers(-10, 26, size=(1, 1024, 8))
    add_i32("many_r8", 16, 16, many, [1024], 8)
    add_i32("many_r96", 16, 16, many, [1024], 96, kind="quad", valid=(rng.random((1, 1024)) < 0.9).astype(np.int32))
    return tuple(out)


# ------------------------------------------------------------------------------------------------ peaks
@dataclass
class PeakCase:
    name: str
    heat: np.ndarray            # float32 [B][h][w]
    min_peak: float
    r: int
    max_peaks: int


@lru_cache(maxsize=None)
def peak_cases():
    out = []
    rng = np.random.default_rng(11)

    def add(name, heat, min_peak=0.3, r=2, max_peaks=64):
        heat = np.ascontiguousarray(heat, np.float32)
        out.append(PeakCase(name, heat[None] if heat.ndim == 2 else heat, float(min_peak), r, max_peaks))

    add("1x1_peak", [[0.5]], r=1)
    add("1x1_below", [[0.25]], r=8)
    add("1x1_nan", [[np.nan]], r=1)
    m3 = np.array([[0.5, 0.5, 0.1], [0.5, 0.9, 0.9], [0.1, 0.9, 0.3]], np.float32)
    add("3x3_ties_r1", m3, r=1)
    add("3x3_ties_r8", m3, r=8)
    plateau = np.zeros((9, 17), np.float32)
    plateau[2:7, 3:14] = 0.75                                                     # wider than the window at r = 1 and r = 2
    add("plateau_r1", plateau, r=1)
    add("plateau_r2", plateau, r=2)
    add("plateau_r8", plateau, r=8)
    edge = np.zeros((9, 17), np.float32)
    edge[4, 2], edge[4, 5], edge[4, 4 + 9], edge[1, 2], edge[8, 16] = 0.6, 0.6, 0.6, 0.6, 0.6       # equal values at distance 3, 8, ...
    add("equal_across_the_edge_r2", edge, r=2)
    add("equal_across_the_edge_r3", edge, r=3)
    add("equal_across_the_edge_r8", edge, r=8)
    eq = np.zeros((9, 17), np.float32)
    eq[3, 3], eq[6, 12] = np.float32(0.3), np.nextafter(np.float32(0.3), np.float32(0))
    add("min_peak_met_with_equality", eq, min_peak=float(np.float32(0.3)), r=2)
    nan = rng.random((9, 17)).astype(np.float32)
    nan[4, 8], nan[0, 0], nan[8, 16] = np.nan, np.nan, np.inf
    nan[4, 9] = 2.0                                                               # a peak beside a NaN
    add("nan_and_inf", nan, min_peak=0.5, r=2)
    noise = rng.random((40, 70)).astype(np.float32)
    add("70x40_r1", noise, min_peak=0.2, r=1, max_peaks=4096)
    add("70x40_r8", noise, min_peak=0.2, r=8, max_peaks=64)
    add("70x40_exceeded", noise, min_peak=0.2, r=1, max_peaks=5)
    b3 = rng.random((3, 40, 70)).astype(np.float32)
    b3[1] = 0.0
    b3[2, :, 35:] *= 0.1
    add("batch3", b3, min_peak=0.3, r=2, max_peaks=40)
    return tuple(out)


# ------------------------------------------------------------------------------------------------ refine
@dataclass
class RefineCase:
    name: str
    heat: np.ndarray            # float32 [B][h][w]
    recs: np.ndarray            # structured [B][M]
    counts: np.ndarray
    params: dict
    affine: np.ndarray | None = None
    expect_flags: int = 0


def heat_of(h, w, pts, r16=96) -> np.ndarray:
    """The target of float64 points on one map."""
    return R.render_vertices([(int(np.floor(x * 16.0 + 0.5)), int(np.floor(y * 16.0 + 0.5))) for x, y in pts], h, w, table(r16))


@lru_cache(maxsize=None)
def refine_cases():
    out = []
    rng = np.random.default_rng(13)
    P = R.kp_params

    def add(name, heat, recs, counts, params, **kw):
        heat = np.ascontiguousarray(heat, np.float32)
        out.append(RefineCase(name, heat[None] if heat.ndim == 2 else heat, recs, np.asarray(counts, np.int32), params, **kw))

    sq = [(10.3125, 9.75), (40.5, 10.0625), (41.0, 38.9375), (9.6875, 39.5)]
    heat = heat_of(48, 56, sq)
    near = np.rint(np.array(sq) + rng.uniform(-2.5, 2.5, (4, 2))).astype(np.int32).reshape(1, 1, 8)
    for kind, recs in (("rect", SC.records("rect", near)), ("quad", SC.records("quad", near)), ("compact", compact_records(near))):
        for mname, m in (("parabola", R.PARABOLA), ("centroid", R.CENTROID)):
            add(f"square_{kind}_{mname}", heat, recs, [1], P(m))
    add("centroid_cwin7_floor0", heat, SC.records("rect", near), [1], P(R.CENTROID, cwin=7, floor_frac=0.0))
    add("centroid_cwin1", heat, SC.records("rect", near), [1], P(R.CENTROID, cwin=1, floor_frac=0.5, search=31))
    # every flag: the peak on the border of the window, nothing in the window, all four vertices on one peak
    far = np.array([[[16, 10, 40, 4, 41, 39, 30, 30]]])
    add("at_edge_and_no_peak", heat, SC.records("rect", far), [1], P(search=6), expect_flags=R.AT_EDGE | R.NO_PEAK)
    tiny = np.array([[[9, 9, 11, 9, 11, 11, 9, 11]]])
    add("shared", heat, SC.records("quad", tiny), [1], P(search=4), expect_flags=R.SHARED)
    add("min_peak_above_everything", heat, SC.records("rect", near), [1], P(min_peak=1.5), expect_flags=R.NO_PEAK)
    # the window clipped at each map edge, corners outside the map, the peak on the map's border
    bord = heat_of(24, 20, [(0.0, 5.25), (19.0, 7.5), (8.25, 0.0), (11.5, 23.0), (0.0, 0.0), (19.0, 23.0)])
    boxes = np.array([[[1, 4, 18, 9, 7, 1, 12, 22], [-2, -3, 21, 25, -40, 5, 3, 60], [2**31 - 1, 0, -2**31, 0, 0, 2**31 - 1, 0, -2**31]]])
    for mname, m in (("parabola", R.PARABOLA), ("centroid", R.CENTROID)):
        add(f"clipped_{mname}", bord, SC.records("rect", boxes), [3], P(m, search=5), expect_flags=R.NO_PEAK)
    # NaN and huge values in the map, ties.  No infinity: inf - inf is a NaN whose sign bit is the hardware's, so there is no byte to hold to
    bad = heat_of(24, 20, [(5.0, 5.0), (14.0, 5.0), (14.0, 17.0), (5.0, 17.0)]).copy()
    bad[5, 6], bad[17, 14], bad[4, 14], bad[17, 6] = np.nan, np.nan, 3e38, -3e38
    b4 = np.array([[[5, 5, 14, 5, 14, 17, 5, 17]]])
    for mname, m in (("parabola", R.PARABOLA), ("centroid", R.CENTROID)):
        add(f"nonfinite_{mname}", bad, SC.records("rect", b4), [1], P(m, search=3))
    add("all_nan", np.full((8, 8), np.nan, np.float32), SC.records("rect", np.array([[[2, 2, 5, 2, 5, 5, 2, 5]]])), [1], P(), expect_flags=R.NO_PEAK)
    flat = np.full((8, 8), 0.5, np.float32)
    add("flat_ties", flat, SC.records("rect", np.array([[[6, 6, 1, 6, 6, 1, 7, 7]]])), [1], P(search=2), expect_flags=R.AT_EDGE)
    add("1x1", np.array([[0.9]], np.float32), SC.records("rect", np.array([[[0, 0, 1, 0, 0, 1, 9, 9]]])), [1], P(search=1),
        expect_flags=R.SHARED | R.NO_PEAK)
    # B = 3, counts 0 / above the cap / negative, valid == 0, an affine row per map
    pts3 = [[(12.3, 10.1), (60.2, 12.6), (58.9, 50.4), (10.7, 48.8)], [(20.5, 20.5), (40.25, 21.0), (41.0, 44.0), (19.0, 43.5)], [(5.0, 5.0), (70.0, 6.0), (69.0, 60.0), (6.0, 61.0)]]
    h3 = np.stack([heat_of(72, 80, p) for p in pts3])
    bx = np.stack([np.stack([np.rint(np.array(p) + rng.uniform(-2, 2, (4, 2))).astype(np.int32).reshape(8) for _ in range(3)]) for p in pts3])
    aff = np.array([[0.0, 12.5, 6.0], [3.0, 0.0, 1.5], [0.0, 0.0, 1.0]])
    valid = np.array([[1, 0, 1], [1, 1, 1], [0, 1, 1]], np.int32)
    for mname, m in (("parabola", R.PARABOLA), ("centroid", R.CENTROID)):
        add(f"batch3_{mname}", h3, SC.records("quad", bx, valid), [3, 0, 7], P(m))
        add(f"batch3_{mname}_affine", h3, SC.records("quad", bx, valid), [2, 3, -1], P(m), affine=aff)
    return tuple(out)


# ------------------------------------------------------------------------------------------------ analytic truth
def estimator_errors(sigma: float, method: int, cwin: int = 3, floor_frac: float = 0.25, size: int = 33):
    """One vertex at each of the 256 positions of the 1/16 grid inside pixel (16, 16) of a size x size map -> (largest |peak - vertex|
    over both axes, largest Euclidean distance of the estimate from the vertex)."""
    tab = R.gaussian_table(sigma)
    p = R.kp_params(method, search=2, cwin=cwin, floor_frac=floor_frac, min_peak=0.3)
    c = size // 2
    worst_peak = worst = 0.0
    for fy in range(16):
        for fx in range(16):
            X, Y = 16 * c + fx, 16 * c + fy
            m = R.render_vertices([(X, Y)], size, size, tab)
            x, y, flags, iters, pk = R.refine_vertex(m, c, c, p)
            assert flags == 0 and iters == 1
            tx, ty = X / 16.0, Y / 16.0
            worst_peak = max(worst_peak, abs(pk[0] - tx), abs(pk[1] - ty))
            worst = max(worst, float(np.hypot(x - tx, y - ty)))
    return worst_peak, worst
