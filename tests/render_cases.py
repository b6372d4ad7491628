"""Built cases for vk.render.  No GPU is needed to import this module: tests/test_render_cpu.py proves the restatement
(tests/render_ref.py) on its own, tests/test_vk_render_gpu.py runs the kernels on these cases.

Families: `panel_cases` (inputs whose de-normalised value lands on an integer, one ulp below it, outside 0..255 and on NaN; maps on the
> 127 edge), `prim_cases` (hand-built records of the three layouts: rank ties, a wrapping palette, invalid slots, odd counts, degenerate
and tied boxes, every kind of d_mean, an affine row, corners on either side of the coordinate range), `draw_cases` (small maps with
overlapping, tile-crossing, clipped and outlying detections) and `reduce_images`."""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache

import numpy as np

import render_ref as R
import subpix_ref as SR
from subpix_cases import DET_DT, QUADFIT_DT

SEED = 20251020
D_MEANS = (0.0, 0.25, 0.35, 9.95, 99.95, 999999.94, 1.0e6, -1.0, float("nan"), float("inf"))


# ------------------------------------------------------------------------------------------------ panels
@dataclass
class PanelCase:
    name: str
    x: np.ndarray               # float32 [N][3][H][W]
    y: np.ndarray               # float32 [N][1][H][W]
    prob: np.ndarray
    color: tuple
    pad: int                    # bytes behind the 12 W of a row


def _x_for(v: float, k: int) -> np.float32:
    """A float32 x whose de-normalised float64 value is as near v as float32 allows."""
    return np.float32((v / 255.0 - R.MEAN[k]) / R.STD[k])


def _x_on_integer(target: int, k: int):
    """(x, x_below): float32 inputs of plane k whose value (((double)x * std) + mean) * 255.0 is >= target by the least amount and the
    float32 just before it, which gives a value below target: the two sides of a truncation step."""
    def val(x):
        return ((float(x) * R.STD[k]) + R.MEAN[k]) * 255.0
    x = _x_for(float(target), k)
    while val(x) < target:
        x = np.nextafter(x, np.float32(np.inf))
    while val(np.nextafter(x, np.float32(-np.inf))) >= target:
        x = np.nextafter(x, np.float32(-np.inf))
    return x, np.nextafter(x, np.float32(-np.inf))


def _special_values(k: int):
    vals = []
    for target in (1, 77, 128, 254, 255):
        vals.extend(_x_on_integer(target, k))
    # an exact integer: x = 0 gives mean * 255 (not an integer); -mean / std gives about 0; far outside on both sides; NaN, inf
    vals.extend([np.float32(0.0), np.float32(-R.MEAN[k] / R.STD[k]), np.float32(-5.0), np.float32(9.0), np.float32("nan"), np.float32("inf"),
                 np.float32("-inf")])
    return np.array(vals, np.float32)


def _unit_specials():
    a127, a128 = np.float32(127.0) / np.float32(255.0), np.float32(128.0) / np.float32(255.0)
    return np.array([0.0, 1.0, a127, a128, np.nextafter(a128, np.float32(0)), np.nextafter(a128, np.float32(1)), 0.5, np.float32("nan"), -0.25, 1.5,
                     np.float32("inf"), 0.999999], np.float32)


@lru_cache(maxsize=None)
def panel_cases():
    rng = np.random.default_rng(SEED)
    out = []
    for name, (N, H, W), color, pad in (("1x1", (1, 1, 1), (0, 140, 255), 0), ("2x5x7", (2, 5, 7), (10, 30, 255), 5), ("1x9x33", (1, 9, 33), (0, 140, 255), 3)):
        x = rng.normal(0.0, 1.2, (N, 3, H, W)).astype(np.float32)
        y = (rng.random((N, 1, H, W)) > 0.5).astype(np.float32)
        prob = rng.random((N, 1, H, W)).astype(np.float32)
        n = H * W
        for k in range(3):
            sp = _special_values(k)
            flat = x[0, k].reshape(-1)
            flat[:min(n, len(sp))] = sp[:n] if name != "1x1" else sp[k:k + 1]
        us = _unit_specials()
        for t, shift in ((y, 0), (prob, 3)):
            flat = t[0, 0].reshape(-1)
            m = min(n, len(us))
            flat[:m] = np.roll(us, shift)[:m]
        if name == "1x1":
            prob[0, 0, 0, 0] = np.float32(128.0) / np.float32(255.0)       # the overlay is on
        out.append(PanelCase(name, x, y, prob, color, pad))
    return tuple(out)


# ------------------------------------------------------------------------------------------------ primitives
@dataclass
class PrimCase:
    name: str
    recs: np.ndarray            # structured [B][M]
    counts: np.ndarray
    mode: int
    field: str                  # where the corners are
    affine: np.ndarray | None = None
    thickness: int = 2
    text_scale: int = 2


def _sq(cx, cy, r):
    return [cx - r, cy - r, cx + r, cy - r, cx + r, cy + r, cx - r, cy + r]


def _fill(dt, B, M):
    raw = np.full((B, M, dt.itemsize), 0x5A, np.uint8)
    return raw.reshape(-1).view(dt).reshape(B, M)


def _records(kind: str, boxes, areas, d_means, valid=None, centers=None):
    """boxes [B][M][8] -> records of the rect / quad fit or of vk_subpix_quad ("v" / "vs": the boxes go to that field as doubles with a
    fraction added, the other field holds something else)."""
    boxes = np.asarray(boxes, np.float64)
    B, M = boxes.shape[:2]
    if kind in ("rect", "quad"):
        r = _fill(DET_DT if kind == "rect" else QUADFIT_DT, B, M)
        r["box"] = boxes.astype(np.int32)
        ctr = boxes.reshape(B, M, 4, 2).mean(axis=2) + 0.375 if centers is None else np.asarray(centers, np.float64)
        r["cx"], r["cy"] = ctr[..., 0].astype(np.float32), ctr[..., 1].astype(np.float32)
        if kind == "quad":
            r["valid"] = 1 if valid is None else np.asarray(valid, np.int32)
    else:
        r = _fill(SR.QUAD_DT, B, M)
        frac = np.array([0.5, -0.5, 0.25, 1.5, -0.49, 0.51, 2.5, -1.5])      # ties of rint on both parities among them
        r[kind] = boxes + frac
        r["vs" if kind == "v" else "v"] = boxes[..., ::-1] * 3.0 + 1000.0
        r["valid"] = 1 if valid is None else np.asarray(valid, np.int32)
    r["label"] = 1 + np.arange(M)[None, :] + 100 * np.arange(B)[:, None]
    r["area"] = np.asarray(areas, np.int32)
    r["d_mean"] = np.asarray(d_means, np.float64)
    return r


@lru_cache(maxsize=None)
def prim_cases():
    rng = np.random.default_rng(SEED + 1)
    out = []
    # B = 4, M = 20: counts 0, negative, 11 and above max_components (every slot used: 20 > 17 drawn, the palette wraps twice)
    B, M = 4, 20
    ctr = rng.integers(20, 200, (B, M, 2))
    rad = rng.integers(3, 30, (B, M))
    boxes = np.array([[_sq(int(c[0]), int(c[1]), int(r)) for c, r in zip(cr, rr)] for cr, rr in zip(ctr, rad)])
    # general quadrilaterals in map 3
    boxes[3] += rng.integers(-6, 7, (M, 8))
    areas = rng.integers(10, 5000, (B, M))
    areas[2, 1] = areas[2, 4] = areas[2, 7] = 777                          # a rank tie among three slots
    areas[3, 0:6] = 50                                                     # and among the six first
    d = rng.uniform(0.0, 700.0, (B, M))
    d[3, :len(D_MEANS)] = D_MEANS
    valid = np.ones((B, M), np.int32)
    valid[2, 3] = valid[2, 5] = valid[3, 2] = valid[3, 11] = valid[3, 12] = 0  # invalid slots between valid ones
    counts = np.array([0, -4, 11, 23], np.int32)                          # with the invalid slots: 9 and 17 drawn
    for kind in ("rect", "quad"):
        out.append(PrimCase("box_" + kind, _records(kind, boxes, areas, d, valid), counts, R.COORD_BOX, "box"))
    for kind in ("v", "vs"):
        out.append(PrimCase("subpix_" + kind, _records(kind, boxes, areas, d, valid), counts, R.COORD_V if kind == "v" else R.COORD_VS, kind,
                            thickness=3, text_scale=1))
    aff = np.array([[0.0, 0.0, 1.0], [3.0, -2.0, 2.0], [0.0, 16.0, 8.0], [-7.25, 26.5, 5.859375]])
    out.append(PrimCase("affine_quad", _records("quad", boxes, areas, d, valid), counts, R.COORD_BOX, "box", affine=aff, thickness=8, text_scale=3))
    out.append(PrimCase("affine_v", _records("v", boxes, areas, d, valid), counts, R.COORD_V, "v", affine=aff, thickness=1))
    out.append(PrimCase("affine_ignored_vs", _records("vs", boxes, areas, d, valid), counts, R.COORD_VS, "vs", affine=aff))
    # degenerate and tied boxes, and the coordinate range: B = 1, M = 12
    Rm = R.MAX_COORD
    special = np.array([[[40, 40, 40, 40, 40, 40, 40, 40],                  # four equal corners
                         [10, 10, 20, 20, 30, 30, 50, 12],                  # three collinear
                         [10, 10, 50, 10, 50, 30, 10, 30],                  # a rectangle: (0,2) and (1,3) tie, (0,2) wins
                         [50, 10, 50, 30, 10, 30, 10, 10],                  # the same from another corner
                         [0, 0, 30, 0, 0, 0, 30, 0],                        # two pairs of equal corners: (0,1) (0,3) (1,2) (2,3) tie
                         [-30, -20, 15, -25, 20, 18, -28, 22],              # negative coordinates
                         [Rm, 5, Rm - 10, 5, Rm - 10, 25, Rm, 25],          # a corner exactly on the range: drawn
                         [Rm + 1, 5, Rm - 10, 5, Rm - 10, 25, Rm, 25],      # one past it: skipped
                         [-Rm, -Rm, 10 - Rm, -Rm, 10 - Rm, 10 - Rm, -Rm, 10 - Rm],    # on the range on the other side
                         [-Rm - 1, 0, 10, 0, 10, 10, 0, 10],                # past it
                         [5, 5, 9, 5, 9, 9, 5, 9],
                         [2 ** 31 - 1, 0, 10, 0, 10, 10, -2 ** 31, 10]]])   # the ends of int32
    sa = np.array([[5, 6, 7, 7, 9, 1, 2, 3, 4, 5, 6, 7]])
    sd = np.array([[12.05, 0.05, 0.15, 2.5, 1e-300, 123456.75, 1.0, 2.0, 3.0, 4.0, 999999.95, 5.0]])
    sc = np.tile(np.array([[[30.5, 31.5]]]), (1, 12, 1))
    sc[0, 5] = (-3.5, -2.5)                                                 # truncation toward zero of a negative centre
    sc[0, 10] = (float("nan"), 7.0)                                        # a NaN centre: skipped
    out.append(PrimCase("special_rect", _records("rect", special, sa, sd, centers=sc), np.array([12], np.int32), R.COORD_BOX, "box"))
    sv = _records("vs", np.clip(special, -2 ** 30, 2 ** 30), sa, sd)
    sv["vs"][0, 10, 3] = float("nan")
    sv["vs"][0, 11, 0] = float("inf")
    out.append(PrimCase("special_vs", sv, np.array([12], np.int32), R.COORD_VS, "vs"))
    return tuple(out)


# ------------------------------------------------------------------------------------------------ draw
@dataclass
class DrawCase:
    name: str
    src: np.ndarray             # uint8 [h][w][3]
    mask: np.ndarray            # uint8 or float32 [h][w]
    thresh: float
    prims: np.ndarray | None    # R.PRIM_DT [M]
    drawn: int
    color: tuple = (0, 0, 255)
    alpha: float = 0.35


def _prims(boxes, centers, d_means, thickness, text_scale, areas=None):
    """A drawing list from the restatement of vk_render_primitives on rect records of one map."""
    M = len(boxes)
    recs = _records("rect", [boxes], [areas if areas is not None else list(range(M, 0, -1))], [d_means], centers=[centers])
    p, drawn, _ = R.primitives_ref(recs, np.array([M], np.int32), R.COORD_BOX, "box", thickness=thickness, text_scale=text_scale)
    return p[0], int(drawn[0])


@lru_cache(maxsize=None)
def draw_cases():
    rng = np.random.default_rng(SEED + 2)
    out = []

    def image(h, w):
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)

    def fmask(h, w, thresh):
        m = rng.random((h, w)).astype(np.float32)
        m.reshape(-1)[::3] = np.float32(thresh)                             # thresh hit exactly: not foreground
        m.reshape(-1)[1::7] = np.nextafter(np.float32(thresh), np.float32(2))
        return m

    def umask(h, w):
        return (rng.integers(0, 3, (h, w)) * 127 + (rng.integers(0, 2, (h, w)))).astype(np.uint8) * (rng.random((h, w)) > 0.4)

    # 1 x 1: a detection that covers the pixel, and an empty list
    p, n = _prims([_sq(0, 0, 0)], [(0.0, 0.0)], [1.0], 1, 1)
    out.append(DrawCase("1x1_point", image(1, 1), np.array([[200]], np.uint8), 0.5, p, n))
    out.append(DrawCase("1x1_empty", image(1, 1), np.array([[0.75]], np.float32), 0.75, None, 0))
    # 20 x 45: every thickness; overlapping detections; labels cut by the right and the top edge; one partly, one wholly outside
    boxes = [[5, 4, 30, 6, 28, 17, 3, 15], _sq(22, 10, 6), [-8, -5, 12, -3, 10, 9, -6, 8], _sq(200, 300, 9), [36, 2, 52, 5, 50, 25, 34, 18]]
    ctrs = [(16.5, 10.5), (22.0, 10.0), (2.0, 2.0), (200.0, 300.0), (38.0, 9.0)]
    for t in (1, 2, 3, 8):
        p, n = _prims(boxes, ctrs, [12.34, 0.35, 99.95, 5.0, float("nan")], t, 1)
        out.append(DrawCase("20x45_t%d" % t, image(20, 45), fmask(20, 45, 0.5), 0.5, p, n))
    # 40 x 70: more than one tile in both directions, text scale 2, a uint8 mask, a non-default colour whose 0.35 c is a tie
    boxes = [[6, 5, 60, 9, 57, 33, 4, 30], _sq(33, 20, 9), [28, -6, 75, 12, 60, 47, 20, 30], _sq(35, 8, 3), _sq(-40, -40, 5), [31, 0, 33, 39, 32, 39, 30, 0]]
    ctrs = [(30.0, 19.0), (33.0, 20.0), (45.0, 21.0), (52.0, 10.0), (-40.0, -40.0), (31.5, 19.5)]
    p, n = _prims(boxes, ctrs, [321.05, 45.25, 7.0, 1000.0, 3.0, 0.0], 2, 2)
    out.append(DrawCase("40x70_u8", image(40, 70), umask(40, 70), 0.5, p, n, color=(10, 30, 50)))
    p, n = _prims(boxes, ctrs, [321.05, 45.25, 7.0, 1000.0, 3.0, 0.0], 3, 1, areas=[1, 2, 3, 4, 5, 6])
    out.append(DrawCase("40x70_f32_reversed", image(40, 70), fmask(40, 70, 0.25), 0.25, p, n, alpha=0.5))
    out.append(DrawCase("40x70_empty", image(40, 70), umask(40, 70), 0.5, None, 0))
    # a list whose count says fewer than it holds, and a record the draw must refuse (a corner beyond the range)
    p, n = _prims(boxes, ctrs, [1.0] * 6, 2, 1)
    p = p.copy()
    p[1]["corner"][0] = R.MAX_COORD + 1
    out.append(DrawCase("40x70_refused_and_short", image(40, 70), umask(40, 70), 0.5, p, n - 2))
    return tuple(out)


ROW_PAD = 5                      # bytes behind every row of a strided image
REDUCE_SIZES = ((1, 1), (5, 7), (33, 70))
REDUCE_K = (1, 2, 3, 16)


@lru_cache(maxsize=None)
def reduce_images():
    rng = np.random.default_rng(SEED + 3)
    return tuple(rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in REDUCE_SIZES)
