"""TEST INFRASTRUCTURE — numpy restatement of vk.patches (csrc/patches.hip): the foreground row index, the origin rule, the crop
(written like oracle/augment_oracle.py: rotate, one ``.astype(float32)`` after every operation, with the zoom and the window origin
inserted) and the whole batch (crop -> RGB -> oracle.augment_oracle.augment)."""
from __future__ import annotations

import numpy as np

from oracle import augment_oracle as A

F = np.float32


def rowcum_ref(mask: np.ndarray) -> np.ndarray:
    """int32 [h]: foreground pixels (m > 0) of rows 0..r."""
    return np.cumsum((mask > 0).sum(axis=1, dtype=np.int64)).astype(np.int32)


def clamp_origin(o: int, L: int, S: int) -> int:
    return min(max(o, 0), L - S) if L >= S else -((S - L) // 2)


def origin_ref(mask: np.ndarray, k: int, oy: int, ox: int, S: int):
    """(y0, x0) of the window; also the chosen foreground pixel (py, px), or None."""
    h, w = mask.shape
    fg = np.flatnonzero(mask.reshape(-1) > 0)                  # raster order
    pick = None
    if k >= 0 and fg.size > 0:
        py, px = divmod(int(fg[min(k, fg.size - 1)]), w)
        pick = (py, px)
        y0, x0 = py - oy, px - ox
    else:
        y0, x0 = oy, ox
    return clamp_origin(y0, h, S), clamp_origin(x0, w, S), pick


def crop_ref(img_bgr: np.ndarray, mask: np.ndarray, y0: int, x0: int, S: int, zoom: float = 1.0, cos_a: float = 1.0, sin_a: float = 0.0):
    """uint8 BGR [h][w][3], mask [h][w] -> (uint8 BGR [S][S][3], {0,1} [S][S]): the S x S window at (y0, x0), rotated and zoomed about
    its centre in the source image; taps outside the image read 0.  (BGR: the caller reverses the channels.)"""
    h, w = mask.shape
    al, be, zm = F(cos_a), F(sin_a), F(zoom)
    c = (F(S) * F(0.5) - F(0.5)).astype(F)
    ys, xs = np.meshgrid(np.arange(S, dtype=F), np.arange(S, dtype=F), indexing="ij")
    dx, dy = (xs - c).astype(F), (ys - c).astype(F)
    cx, cy = (F(x0) + c).astype(F), (F(y0) + c).astype(F)
    sx = ((((al * dx).astype(F) - (be * dy).astype(F)).astype(F) * zm).astype(F) + cx).astype(F)
    sy = ((((be * dx).astype(F) + (al * dy).astype(F)).astype(F) * zm).astype(F) + cy).astype(F)
    x0f, y0f = np.floor(sx), np.floor(sy)
    fx, fy = (sx - x0f).astype(F), (sy - y0f).astype(F)
    xi0, yi0 = x0f.astype(np.int64), y0f.astype(np.int64)

    def tap(yy, xx):
        ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        v = img_bgr[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)].astype(F)
        return np.where(ok[..., None], v, F(0))

    w0x, w0y = (F(1) - fx).astype(F)[..., None], (F(1) - fy).astype(F)[..., None]
    w1x, w1y = fx[..., None], fy[..., None]
    top = ((tap(yi0, xi0) * w0x).astype(F) + (tap(yi0, xi0 + 1) * w1x).astype(F)).astype(F)
    bot = ((tap(yi0 + 1, xi0) * w0x).astype(F) + (tap(yi0 + 1, xi0 + 1) * w1x).astype(F)).astype(F)
    val = ((top * w0y).astype(F) + (bot * w1y).astype(F)).astype(F)
    out = np.clip(np.rint(val), 0, 255).astype(np.uint8)
    xi, yi = np.floor((sx + F(0.5)).astype(F)).astype(np.int64), np.floor((sy + F(0.5)).astype(F)).astype(np.int64)
    okm = (yi >= 0) & (yi < h) & (xi >= 0) & (xi < w)
    m = np.where(okm, mask[np.clip(yi, 0, h - 1), np.clip(xi, 0, w - 1)] > 0, False).astype(np.uint8)
    return out, m


def slice_ref(img_bgr: np.ndarray, mask: np.ndarray, y0: int, x0: int, S: int):
    """The zero-padded S x S slice at (y0, x0): what the crop is at identity."""
    h, w = mask.shape
    out, m = np.zeros((S, S, 3), np.uint8), np.zeros((S, S), np.uint8)
    ya, yb, xa, xb = max(y0, 0), min(y0 + S, h), max(x0, 0), min(x0 + S, w)
    if ya < yb and xa < xb:
        out[ya - y0:yb - y0, xa - x0:xb - x0] = img_bgr[ya:yb, xa:xb]
        m[ya - y0:yb - y0, xa - x0:xb - x0] = mask[ya:yb, xa:xb] > 0
    return out, m


def patch_ref(img_bgr: np.ndarray, mask: np.ndarray, p: dict, S: int):
    """One sample of vk_patch_batch: (uint8 RGB [S][S][3], {0,1} [S][S], (y0, x0))."""
    y0, x0, _ = origin_ref(mask, p["k"], p["oy"], p["ox"], S)
    bgr, m = crop_ref(img_bgr, mask, y0, x0, S, p["zoom"], p["cos_a"], p["sin_a"])
    return np.ascontiguousarray(bgr[..., ::-1]), m, (y0, x0)


def batch_ref(img_bgr: np.ndarray, mask: np.ndarray, patch: dict, aug: dict, S: int):
    """One sample of PatchDataset.batch: (x float32 [3][S][S], y float32 [1][S][S])."""
    rgb, m, _ = patch_ref(img_bgr, mask, patch, S)
    return A.augment(rgb, m, aug)
