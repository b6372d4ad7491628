"""Built cases for vk.subpix.  No GPU is needed to import this module: tests/test_subpix_cpu.py proves the restatement
(tests/subpix_ref.py) on them against analytic truth, tests/test_vk_subpix_gpu.py runs the kernel on them.

Two families.  `square_draws`: 128 x 128 maps of one rotated square whose true vertices are known, rendered as the exact fraction of
every pixel the square covers (8 x 8 supersampling; pixel i covers [i - 1/2, i + 1/2]), optionally blurred.  `gpu_cases`: hand-built
records on small maps, chosen so that every branch of both estimators is taken: the sizes are the smallest at which the kernel can
go wrong (one pixel, a map smaller than the window, vertices on the border and outside it, every flag)."""
from __future__ import annotations

from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

import subpix_ref as R

DET_DT = np.dtype([("label", "<i4"), ("area", "<i4"), ("box", "<i4", (8,)), ("cx", "<f4"), ("cy", "<f4"), ("rw", "<f4"), ("rh", "<f4"),
                   ("ux", "<f4"), ("uy", "<f4"), ("hull_n", "<i4"), ("reserved", "<i4"), ("d1", "<f8"), ("d2", "<f8"), ("d_mean", "<f8")])
QUADFIT_DT = np.dtype([("label", "<i4"), ("area", "<i4"), ("box", "<i4", (8,)), ("cx", "<f4"), ("cy", "<f4"), ("valid", "<i4"),
                       ("branch", "<i4"), ("n_candidates", "<i4"), ("contour_n", "<i4"), ("hull_n", "<i4"), ("flags", "<i4"),
                       ("quality", "<f8"), ("d1", "<f8"), ("d2", "<f8"), ("d_mean", "<f8")])
assert DET_DT.itemsize == 96 and QUADFIT_DT.itemsize == 104
SEED = 20250314
N_DRAWS = 32


# ------------------------------------------------------------------------------------------------ rendering with known truth
def polygon_coverage(h: int, w: int, verts: np.ndarray, ss: int = 8) -> np.ndarray:
    """float32 [h][w]: the fraction of the ss x ss sample points of every pixel that lie inside the convex polygon `verts` [n][2]
    (x, y), whatever its orientation."""
    off = (np.arange(ss) + 0.5) / ss - 0.5
    xs = (np.arange(w)[:, None] + off[None, :]).reshape(-1)
    ys = (np.arange(h)[:, None] + off[None, :]).reshape(-1)
    X, Y = np.meshgrid(xs, ys)
    n = len(verts)
    pos = np.ones(X.shape, bool)
    neg = np.ones(X.shape, bool)
    for k in range(n):
        ax, ay = verts[k]
        bx, by = verts[(k + 1) % n]
        cr = (bx - ax) * (Y - ay) - (by - ay) * (X - ax)
        pos &= cr >= 0
        neg &= cr <= 0
    inside = pos | neg
    return inside.reshape(h, ss, w, ss).mean(axis=(1, 3)).astype(np.float32)


def square_vertices(cx: float, cy: float, radius: float, angle: float) -> np.ndarray:
    a = angle + np.arange(4) * (np.pi / 2)
    return np.stack([cx + radius * np.cos(a), cy + radius * np.sin(a)], axis=1)


def blur(m: np.ndarray, sigma: float) -> np.ndarray:
    if sigma <= 0:
        return m
    from scipy import ndimage
    return ndimage.gaussian_filter(m.astype(np.float64), sigma, mode="nearest").astype(np.float32)


@dataclass
class Draw:
    prob: np.ndarray            # float32 [128][128]
    truth: np.ndarray           # float64 [4][2]
    box: np.ndarray             # int32 [8]: the start vertices
    d_true: float               # both diagonals: 2 * circumradius
    d_start: float              # d_mean of the start vertices


@lru_cache(maxsize=None)
def square_draws(sigma: float, n: int = N_DRAWS, seed: int = SEED):
    """Centre (64, 64) + U(-3, 3)^2, circumradius U(30, 45), angle U(0, pi / 2), start = rint(truth + U(-1.5, 1.5))."""
    rng = np.random.default_rng(seed + int(round(10 * sigma)))
    out = []
    for _ in range(n):
        cx, cy = 64.0 + rng.uniform(-3, 3), 64.0 + rng.uniform(-3, 3)
        rad, ang = rng.uniform(30, 45), rng.uniform(0, np.pi / 2)
        truth = square_vertices(cx, cy, rad, ang)
        prob = blur(polygon_coverage(128, 128, truth), sigma)
        start = np.rint(truth + rng.uniform(-1.5, 1.5, size=(4, 2))).astype(np.int32)
        box = start.reshape(8)
        out.append(Draw(prob, truth, box, 2.0 * rad, R.diagonals([float(c) for c in box], 1.0)[2]))
    return tuple(out)


def bowed_square(h: int, w: int, cx: float, cy: float, radius: float, angle: float, sag: float, ss: int = 4) -> np.ndarray:
    """A square whose sides bow by `sag` pixels at mid-side (outward for sag > 0): the intersection / union test per sample point of a
    parabola over every side.  The vertices stay where they are."""
    v = square_vertices(cx, cy, radius, angle)
    off = (np.arange(ss) + 0.5) / ss - 0.5
    xs = (np.arange(w)[:, None] + off[None, :]).reshape(-1)
    ys = (np.arange(h)[:, None] + off[None, :]).reshape(-1)
    X, Y = np.meshgrid(xs, ys)
    inside = np.ones(X.shape, bool)
    for k in range(4):
        a, b = v[k], v[(k + 1) % 4]
        d = b - a
        L = float(np.hypot(*d))
        t = ((X - a[0]) * d[0] + (Y - a[1]) * d[1]) / (L * L)          # 0 .. 1 along the side
        nrm = np.array([d[1], -d[0]]) / L
        if nrm @ (a - np.array([cx, cy])) < 0:
            nrm = -nrm
        dist = (X - a[0]) * nrm[0] + (Y - a[1]) * nrm[1]               # > 0 outside the straight side
        inside &= dist <= sag * 4.0 * t * (1.0 - t)
    return inside.reshape(h, ss, w, ss).mean(axis=(1, 3)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ hand-built records for the kernel
def records(kind: str, boxes, valid=None) -> np.ndarray:
    """boxes [B][M][8] -> structured [B][M] of the rectangle ("rect") or the quadrilateral ("quad") fit's layout, the fields the call
    does not read filled with a pattern."""
    boxes = np.asarray(boxes, np.int32)
    B, M = boxes.shape[:2]
    dt = DET_DT if kind == "rect" else QUADFIT_DT
    raw = np.full((B, M, dt.itemsize), 0x5A, np.uint8)
    r = raw.reshape(-1).view(dt).reshape(B, M)
    r["box"] = boxes
    r["label"] = 1 + np.arange(M)[None, :] + 100 * np.arange(B)[:, None]
    r["area"] = 7 + 3 * np.arange(M)[None, :]
    if kind == "quad":
        r["valid"] = 1 if valid is None else np.asarray(valid, np.int32)
    return r


@dataclass
class Case:
    name: str
    prob: np.ndarray            # float32 [B][h][w]
    boxes: np.ndarray           # int32 [B][M][8]
    counts: np.ndarray          # int32 [B]
    params: dict
    kind: str = "rect"
    valid: np.ndarray | None = None
    affine: np.ndarray | None = None
    expect_flags: int = 0       # bits that must show somewhere in the reference's result (the case says what it claims)
    note: str = field(default="")


def _rot_square_map(h, w, cx, cy, rad, ang, sigma):
    return blur(polygon_coverage(h, w, square_vertices(cx, cy, rad, ang)), sigma)


def _start(truth, shift=0.0):
    return np.rint(np.asarray(truth) + shift).astype(np.int32).reshape(8)


def gpu_cases():
    C, Ln = R.corner_params, R.lines_params
    out = []
    rng = np.random.default_rng(99)

    def add(name, prob, boxes, counts, params, **kw):
        prob = np.ascontiguousarray(prob, np.float32)
        if prob.ndim == 2:
            prob = prob[None]
        boxes = np.asarray(boxes, np.int32)
        if boxes.ndim == 2:
            boxes = boxes[None]
        out.append(Case(name, prob, boxes, np.asarray(counts, np.int32).reshape(-1), params, **kw))

    # one pixel and a map smaller than any window
    one = np.array([[0.7]], np.float32)
    add("1x1_corner", one, [[0, 0, 0, 0, 0, 0, 0, 0]], [1], C(win=2), expect_flags=R.SINGULAR)
    add("1x1_lines", one, [[0, 0, 9, 0, 9, 9, 0, 9]], [1], Ln(reach=1, n_stations=3), expect_flags=R.NO_EDGE)
    m4 = np.array([[0, 0, 0, 0], [0, 1, 1, 0], [0, 1, 0.5, 0], [0, 0, 0, 0]], np.float32)
    for win in (2, 15):
        add(f"4x4_corner_win{win}", m4, [[1, 1, 2, 1, 2, 2, 1, 2], [0, 0, 3, 0, 3, 3, 0, 3]], [2], C(win=win))
    add("4x4_lines", m4, [[0, 0, 3, 0, 3, 3, 0, 3], [-5, -5, 8, -5, 8, 8, -5, 8]], [2], Ln(reach=15, n_stations=32), expect_flags=R.SHORT_SIDE)
    # 32 x 32: flat, NaN / inf, one-pixel blob, binary mask
    flat = np.full((32, 32), 0.25, np.float32)
    sq32 = [[8, 8, 24, 8, 24, 24, 8, 24], [0, 0, 31, 0, 31, 31, 0, 31]]
    add("flat_corner", flat, sq32, [2], C(), expect_flags=R.SINGULAR)
    add("flat_lines", flat, sq32, [2], Ln(), expect_flags=R.NO_EDGE)
    bad = _rot_square_map(32, 32, 16, 15.5, 10, 0.3, 1.0).copy()
    bad[5, 7], bad[20, 21], bad[25, 24], bad[16, 26] = np.nan, np.inf, -np.inf, np.nan
    tb = square_vertices(16, 15.5, 10, 0.3)
    for nm, pr in (("corner", C()), ("corner_zz2", C(zero_zone=2)), ("lines", Ln(reach=6)), ("lines_r15", Ln(reach=15, n_stations=32))):
        add(f"nonfinite_{nm}", bad, [_start(tb), _start(tb, 1.0)], [2], pr)
    blob = np.zeros((32, 32), np.float32)
    blob[13, 17] = 1.0
    add("blob_corner", blob, [[17, 13, 18, 13, 18, 14, 17, 14], [15, 11, 19, 11, 19, 15, 15, 15]], [2], C(win=2))
    add("blob_corner_iter1", blob, [[15, 11, 19, 11, 19, 15, 15, 15]], [1], C(win=5, max_iter=1), expect_flags=R.NOT_CONVERGED)
    binm = (_rot_square_map(32, 32, 15, 16, 11, 0.6, 0.0) >= 0.5).astype(np.float32)
    tq = square_vertices(15, 16, 11, 0.6)
    for zz in (-1, 0, 2):
        add(f"binary_corner_zz{zz}", binm, [_start(tq), _start(tq, -1.0)], [2], C(win=5, zero_zone=zz))
    for lvl in (0.45, 0.5):
        add(f"binary_lines_level{lvl}", binm, [_start(tq), _start(tq, -1.0)], [2], Ln(level=lvl, reach=4, n_stations=7))
    # 40 x 56: blurred rotated square, vertices near and on the border, a corner of the map, a start far from any edge
    sq = _rot_square_map(40, 56, 27.3, 19.6, 19.0, 0.2, 1.0)
    ts = square_vertices(27.3, 19.6, 19.0, 0.2)
    far = [20, 20, 34, 20, 34, 30, 20, 30]                                # inside the square: nothing within reach
    edge = [0, 0, 55, 0, 55, 39, 0, 39]                                   # the map's own corners
    near = [3, 4, 50, 2, 52, 36, 5, 35]
    for nm, pr, fl in (("corner_w2", C(win=2), 0), ("corner_w5", C(), 0), ("corner_w15", C(win=15), 0), ("corner_w5_zz0_it1", C(zero_zone=0, max_iter=1), 0),
                       ("lines", Ln(), R.NO_EDGE), ("lines_r1_n3", Ln(reach=1, n_stations=3), 0),
                       ("lines_r15_n32", Ln(reach=15, n_stations=32, level=0.45), 0), ("lines_shift1", Ln(max_shift=0.25), R.RESTORED)):
        add(f"square_{nm}", sq, [_start(ts), _start(ts, 1.3), far, edge, near], [5], pr, expect_flags=fl)
    # RESTORED for the corner method: gradients on one side only, a window's width away
    ramp = np.zeros((40, 56), np.float32)
    ramp[:, 30:] = 1.0
    ramp[20:, :] = np.maximum(ramp[20:, :], 0.5)
    add("corner_restored", blur(ramp, 1.0), [[26, 16, 27, 24, 33, 17, 25, 23]], [1], C(win=5, max_iter=40))
    # a rhombus, a side shorter than 8, parallel sides
    rh = polygon_coverage(40, 56, np.array([[28.0, 4.5], [49.5, 20.0], [28.0, 35.5], [6.5, 20.0]]))
    rb = [28, 4, 50, 20, 28, 36, 6, 20]
    add("rhombus_corner", blur(rh, 1.0), [rb], [1], C())
    add("rhombus_lines", blur(rh, 1.0), [rb], [1], Ln())
    add("short_side", blur(rh, 1.0), [[28, 4, 33, 8, 28, 36, 6, 20]], [1], Ln(), expect_flags=R.SHORT_SIDE)
    bar = np.zeros((40, 56), np.float32)
    bar[15:25, :] = 1.0                                                    # a band: the two sides at a vertex on it are one line
    add("parallel_sides", blur(bar, 1.0), [[28, 14, 50, 14, 28, 33, 6, 14]], [1], Ln(lo=0.1, hi=0.6), expect_flags=R.PARALLEL)
    # 96 x 160: batch 3, counts 0 / equal to / above the capacity, both layouts, valid = 0, affine
    big = np.stack([_rot_square_map(96, 160, 50 + 30 * b, 48, 30 + 3 * b, 0.15 + 0.3 * b, float(b % 2)) for b in range(3)])
    tv = [square_vertices(50 + 30 * b, 48, 30 + 3 * b, 0.15 + 0.3 * b) for b in range(3)]
    boxes = np.stack([np.stack([_start(tv[b], rng.uniform(-1.5, 1.5, (4, 2))) for _ in range(3)]) for b in range(3)])
    aff = np.array([[0.0, 12.5, 6.0], [3.0, 0.0, 1.5], [0.0, 0.0, 1.0]])
    for kind in ("rect", "quad"):
        valid = np.array([[1, 0, 1], [1, 1, 1], [0, 1, 1]], np.int32) if kind == "quad" else None
        for nm, pr in (("corner", C()), ("lines", Ln())):
            add(f"batch3_{kind}_{nm}", big, boxes, [3, 0, 7], pr, kind=kind, valid=valid)
            add(f"batch3_{kind}_{nm}_affine", big, boxes, [2, 3, -1], pr, kind=kind, valid=valid, affine=aff)
    return out


def sweep_sigmas_sags():
    """What DESIGN.md quotes: the signed error of d_mean in pixels over 12 draws, (estimator, sigma, sag) -> (mean, worst |error|)."""
    res = {}
    rng = np.random.default_rng(5)
    draws = [(64 + rng.uniform(-3, 3), 64 + rng.uniform(-3, 3), rng.uniform(30, 45), rng.uniform(0, np.pi / 2), rng.uniform(-1.5, 1.5, (4, 2)))
             for _ in range(12)]
    for sigma in (0.0, 1.0, 2.0):
        for sag in (-2.0, 0.0, 2.0):
            if sag != 0.0 and sigma != 1.0:
                continue
            for name, p in (("corner", R.corner_params()), ("lines", R.lines_params())):
                errs = []
                for cx, cy, rad, ang, jit in draws:
                    truth = square_vertices(cx, cy, rad, ang)
                    m = blur(polygon_coverage(128, 128, truth) if sag == 0.0 else bowed_square(128, 128, cx, cy, rad, ang, sag), sigma)
                    box = np.rint(truth + jit).astype(np.int32).reshape(8)
                    errs.append(R.refine_one(m, [int(c) for c in box], p)[6] - 2.0 * rad)
                res[(name, sigma, sag)] = (float(np.mean(errs)), float(np.max(np.abs(errs))))
    return res
