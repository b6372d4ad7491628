"""TEST INFRASTRUCTURE — built images, masks and draws for vk.patches; everything is generated from seeds.

Items (h x w) and their foreground (mask values are random non-zero bytes: the store binarises them):
  0   37 x  53  empty mask                                           width 53: no multiple of 4
  1   64 x 200  one pixel, in the last column of the last row        width 200: no multiple of 64
  2  307 x 205  a diamond cut by empty rows (every third row kept)   more rows than one scan thread per row
  3   96 x  96  one pixel at (0, 0)
  4    1 x   1  its one pixel
  5    5 x 259  rows 0 and 2 full, row 4 scattered, 1 and 3 empty    width 259: five 64-pixel pieces, no multiple of 256"""
from __future__ import annotations

import math

import numpy as np

SHAPES = [(37, 53), (64, 200), (307, 205), (96, 96), (1, 1), (5, 259)]
ANGLES = [30.0, -137.5, 90.0, 180.0, 12.25]
ZOOMS = [0.5, 0.8, 1.25, 2.0]
ORIGIN_SIZES = (64, 96)
CROP_SIZES = (37, 64, 70, 96)          # 37, 70: patch rows that do not start on a dword; 70: a last tile of 6 pixels

AUG_IDENTITY = dict(d4=0, rotate=0, cos_a=1.0, sin_a=0.0, photo=0, alpha=1.0, beta=0.0, blur_ksize=3, noise_scale=0.0, noise_seed=0,
                    clahe_clip=1.0)


def image(h: int, w: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    img[..., 1] = ((yy * 3 + xx * 2) % 256).astype(np.uint8)        # a channel that tells a shifted pixel from its neighbour
    return img


def mask(i: int) -> np.ndarray:
    h, w = SHAPES[i]
    rng = np.random.default_rng(100 + i)
    val = rng.integers(1, 256, (h, w), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    if i == 0:
        on = np.zeros((h, w), bool)
    elif i == 1:
        on = (yy == h - 1) & (xx == w - 1)
    elif i == 2:
        on = ((np.abs(xx - w / 2) + np.abs(yy - h / 2)) < 70) & (yy % 3 == 0)
    elif i == 3:
        on = (yy == 0) & (xx == 0)
    elif i == 4:
        on = np.ones((h, w), bool)
    else:
        on = (yy == 0) | (yy == 2) | ((yy == 4) & (rng.random((h, w)) < 0.1))
    return np.where(on, val, 0).astype(np.uint8)


def items():
    return [image(h, w, i) for i, (h, w) in enumerate(SHAPES)], [mask(i) for i in range(len(SHAPES))]


def patch(item, k=-1, oy=0, ox=0, zoom=1.0, angle=None):
    a = math.radians(angle) if angle is not None else 0.0
    return dict(item=item, k=k, oy=oy, ox=ox, zoom=zoom, cos_a=math.cos(a) if angle is not None else 1.0,
                sin_a=math.sin(a) if angle is not None else 0.0)


def origin_draws(masks, S):
    """k in {0, 1, count // 2, count - 1, count (clamped), -1} x offsets in {0, S - 1}^2, for every item."""
    out = []
    for i, m in enumerate(masks):
        count = int((m > 0).sum())
        for k in (0, 1, count // 2, count - 1, count, -1):
            for oy in (0, S - 1):
                for ox in (0, S - 1):
                    out.append(patch(i, max(k, -1), oy, ox))
    return out


TRANSFORMS = ([("identity", 1.0, None)] + [("rot%g" % a, 1.0, a) for a in ANGLES] + [("zoom%g" % z, z, None) for z in ZOOMS]
              + [("rot%g_zoom%g" % (a, z), z, a) for a, z in zip(ANGLES, ZOOMS + [0.8])])


def crop_draws(masks, S):
    """Every transform at three windows per item: flush with the top-left corner, flush with the bottom-right corner (a rotated or
    zoomed-out footprint hangs over the edges there; an item smaller than S hangs over by itself) and on a foreground pixel."""
    out = []
    for i, m in enumerate(masks):
        h, w = m.shape
        count = int((m > 0).sum())
        for _, z, a in TRANSFORMS:
            out.append(patch(i, -1, 0, 0, z, a))
            out.append(patch(i, -1, max(h - S, 0), max(w - S, 0), z, a))
            out.append(patch(i, count // 2, S // 3, S - 1 - S // 5, z, a))
    return out


def batch_draws(S):
    """Combined (patch, aug) draws for PatchDataset.batch, CLAHE, blur and noise among them."""
    a = AUG_IDENTITY
    return [
        (patch(2, 40, 10, 20, 1.0, None), dict(a)),
        (patch(2, 500, 50, 60, 1.25, 30.0), dict(a, d4=4, photo=2, clahe_clip=1.37)),
        (patch(5, 300, 3, 90, 0.8, -137.5), dict(a, d4=1, photo=3, blur_ksize=5)),
        (patch(1, 0, S - 1, S - 1, 2.0, 12.25), dict(a, d4=6, photo=1, alpha=1.17, beta=-0.08, noise_scale=5.0 / 65536.0, noise_seed=99)),
        (patch(3, -1, 0, 0, 0.5, 90.0), dict(a, photo=3, blur_ksize=3, noise_scale=6.5 / 65536.0, noise_seed=4_000_000_000)),
        (patch(0, -1, 0, 0, 1.0, 180.0), dict(a, d4=2, photo=2, clahe_clip=2.0, noise_scale=3.0 / 65536.0, noise_seed=17)),
        (patch(4, 0, 5, 7, 1.0, None), dict(a, d4=5)),
    ]
