"""Restatement of vk.zoom (csrc/zoom.hip: vk_zoom_windows, vk_zoom_gather, vk_zoom_merge) on the host, for bit-for-bit comparison.
No GPU is needed.  Written from the rules in include/vk_unet.h, not from the kernels.

Python floats and numpy float64 elementwise `+ - * /` are IEEE float64 and round once, so these are the device's operations.  The
gather is vectorised over the output pixels but never over a sum: the taps of an axis are walked one by one in ascending order, and a
tap beyond a pixel's last one gets the weight +0.0, whose product with a byte is +0.0 and leaves the non-negative sum as it is."""
from __future__ import annotations

import math

import numpy as np

import subpix_ref as SR

CLIPPED, SCALE_CLAMPED_LO, SCALE_CLAMPED_HI = 1, 2, 4
ZOOMED, NO_TARGET, REFINE_FAILED, DISAGREES, NO_WINDOW = 16, 32, 64, 128, 256
FAIL_MASK = 0x7F
MAX_ORIGIN = 1073741824.0

WINDOW_DT = np.dtype([("map", "<i4"), ("slot", "<i4"), ("status", "<i4"), ("pad", "<i4"), ("X0", "<f8"), ("Y0", "<f8"), ("s", "<f8")])
assert WINDOW_DT.itemsize == 40
MEAN = np.array([0.485, 0.456, 0.406], np.float32)
STD = np.array([0.229, 0.224, 0.225], np.float32)


def params(S=512, margin=1.5, s_min=1.0, s_max=32.0, max_windows=65535):
    return dict(S=int(S), margin=float(margin), s_min=float(s_min), s_max=float(s_max), max_windows=int(max_windows))


# ------------------------------------------------------------------------------------------------ windows
def window_of(box, aff, size, p):
    """One valid record -> (status bits, X0, Y0, s).  box: 8 ints; aff: (ox, oy, inv); size: (h, w)."""
    ox, oy, inv = (float(a) for a in aff)
    sx = [(float(box[2 * q]) - ox) * inv for q in range(4)]
    sy = [(float(box[2 * q + 1]) - oy) * inv for q in range(4)]
    cx = (((sx[0] + sx[1]) + sx[2]) + sx[3]) * 0.25
    cy = (((sy[0] + sy[1]) + sy[2]) + sy[3]) * 0.25
    e = 0.0
    for q in range(4):
        dx, dy = abs(sx[q] - cx), abs(sy[q] - cy)
        e = dx if dx > e else e
        e = dy if dy > e else e
    S = float(p["S"])
    raw = (p["margin"] * (2.0 * e)) / S
    s, status = raw, 0
    if not raw >= p["s_min"]:
        s, status = p["s_min"], status | SCALE_CLAMPED_LO
    if raw > p["s_max"]:
        s, status = p["s_max"], status | SCALE_CLAMPED_HI
    X0 = (cx + 0.5) - (S * s) * 0.5
    Y0 = (cy + 0.5) - (S * s) * 0.5
    h, w = float(size[0]), float(size[1])
    if not (X0 >= 0.0 and Y0 >= 0.0 and X0 + S * s <= w and Y0 + S * s <= h):
        status |= CLIPPED
    return status, X0, Y0, s


def windows_ref(recs: np.ndarray, counts, affine, sizes, p: dict, out=None):
    """recs structured [B][M] (`box`, and `valid` for the quadrilateral fit) -> (WINDOW_DT [max_windows], n): the first n written, the
    rest as `out` had them (zeros when None)."""
    B, M = recs.shape
    cap = p["max_windows"]
    out = np.zeros(cap, WINDOW_DT) if out is None else out.copy()
    has_valid = "valid" in recs.dtype.names
    n = 0
    for b in range(B):
        aff = (0.0, 0.0, 1.0) if affine is None else tuple(float(a) for a in affine[b])
        for t in range(min(max(int(counts[b]), 0), M)):
            r = recs[b, t]
            if has_valid and int(r["valid"]) == 0:
                continue
            if n < cap:
                status, X0, Y0, s = window_of([int(c) for c in r["box"]], aff, sizes[b], p)
                o = np.zeros((), WINDOW_DT)
                o["map"], o["slot"], o["status"], o["X0"], o["Y0"], o["s"] = b, t, status, X0, Y0, s
                out[n] = o
            n += 1
    return out, min(n, cap)


def window_affine_ref(win: np.ndarray) -> np.ndarray:
    X0, Y0, s = win["X0"].astype(np.float64), win["Y0"].astype(np.float64), win["s"].astype(np.float64)
    half = s * 0.5
    return np.stack([-((X0 + half) - 0.5) / s, -((Y0 + half) - 0.5) / s, s], axis=1)


# ------------------------------------------------------------------------------------------------ gather
def axis_spans(O: float, n: int, s: float, f: float):
    """a[x], b[x] float64 and the first / last tap i0[x], i1[x] of the n output pixels of one axis."""
    x = np.arange(n, dtype=np.float64)
    a = (O + (x + 0.5) * s) - f * 0.5
    b = a + f
    return a, b, np.floor(a).astype(np.int64), np.floor(b).astype(np.int64)


def axis_weights(a: np.ndarray, b: np.ndarray, i0: np.ndarray, i1: np.ndarray):
    """(idx [T][n] int64, wt [T][n] float64): tap t of pixel x is source pixel idx[t][x] with weight min(b, i + 1) - max(a, i); +0.0
    beyond the pixel's last tap."""
    T = int((i1 - i0).max()) + 1
    idx = i0[None, :] + np.arange(T, dtype=np.int64)[:, None]
    fi = idx.astype(np.float64)
    wt = np.minimum(b[None, :], fi + 1.0) - np.maximum(a[None, :], fi)
    wt = np.where(idx <= i1[None, :], wt, 0.0)
    return idx, wt


def quantise_normalise(values: np.ndarray) -> np.ndarray:
    """float64 [..., 3] BGR -> float32 [3, ...] RGB planes: rint, clamp, ((float)q / 255.f - mean) / std in float32."""
    q = np.clip(np.rint(values), 0, 255).astype(np.float32)
    out = np.empty((3,) + values.shape[:-1], np.float32)
    for k in range(3):
        f = q[..., 2 - k] / np.float32(255.0)
        out[k] = (f - MEAN[k]) / STD[k]
    return out


def gather_one(img: np.ndarray, X0: float, Y0: float, s: float, S: int, pad: int = 0) -> np.ndarray:
    """One valid window of one uint8 BGR image [h][w][3] -> float64 [S][S][3]: the unquantised area means."""
    h, w = img.shape[:2]
    f = s if s > 1.0 else 1.0
    ax, bx, i0, i1 = axis_spans(X0, S, s, f)
    ay, by, j0, j1 = axis_spans(Y0, S, s, f)
    xi, wx = axis_weights(ax, bx, i0, i1)
    yi, wy = axis_weights(ay, by, j0, j1)
    c0, c1, r0, r1 = int(i0.min()), int(xi.max()), int(j0.min()), int(yi.max())
    # the footprint [r0, r1] x [c0, c1] with pad_value outside the image
    foot = np.full((r1 - r0 + 1, c1 - c0 + 1, 3), float(pad), np.float64)
    ya, yb, xa, xb = max(r0, 0), min(r1 + 1, h), max(c0, 0), min(c1 + 1, w)
    if yb > ya and xb > xa:
        foot[ya - r0:yb - r0, xa - c0:xb - c0] = img[ya:yb, xa:xb].astype(np.float64)
    rows = np.zeros((foot.shape[0], S, 3), np.float64)
    for t in range(xi.shape[0]):                                   # columns ascending within a row
        rows = rows + wx[t][None, :, None] * foot[:, xi[t] - c0, :]
    tot = np.zeros((S, S, 3), np.float64)
    cols = np.arange(S)
    for t in range(yi.shape[0]):                                   # rows ascending
        tot = tot + wy[t][:, None, None] * rows[yi[t] - r0][:, cols, :]
    return tot / (f * f)


def window_ok(win, n_images: int) -> bool:
    X0, Y0, s, m = float(win["X0"]), float(win["Y0"]), float(win["s"]), int(win["map"])
    return 0 <= m < n_images and s >= 0.25 and s <= 64.0 and abs(X0) <= MAX_ORIGIN and abs(Y0) <= MAX_ORIGIN


def gather_ref(images, win: np.ndarray, n: int, S: int, pad: int = 0) -> np.ndarray:
    """images: list of uint8 [h][w][3]; win: WINDOW_DT [>= n] -> float32 [n][3][S][S]."""
    out = np.empty((n, 3, S, S), np.float32)
    for k in range(n):
        if window_ok(win[k], len(images)):
            v = gather_one(images[int(win[k]["map"])], float(win[k]["X0"]), float(win[k]["Y0"]), float(win[k]["s"]), S, pad)
        else:
            v = np.full((S, S, 3), float(pad), np.float64)
        out[k] = quantise_normalise(v)
    return out


def gather_pixel_scalar(img: np.ndarray, X0: float, Y0: float, s: float, x: int, y: int, pad: int = 0):
    """One output pixel by plain Python loops, the rule as the header states it: (value[3] float64, weights x, weights y)."""
    h, w = img.shape[:2]
    f = s if s > 1.0 else 1.0
    ax = (X0 + (float(x) + 0.5) * s) - f * 0.5
    bx = ax + f
    ay = (Y0 + (float(y) + 0.5) * s) - f * 0.5
    by = ay + f
    wxs = [(i, min(bx, float(i + 1)) - max(ax, float(i))) for i in range(math.floor(ax), math.floor(bx) + 1)]
    wys = [(j, min(by, float(j + 1)) - max(ay, float(j))) for j in range(math.floor(ay), math.floor(by) + 1)]
    tot = [0.0, 0.0, 0.0]
    for j, wy in wys:
        row = [0.0, 0.0, 0.0]
        for i, wx in wxs:
            inside = 0 <= j < h and 0 <= i < w
            for c in range(3):
                row[c] = row[c] + wx * (float(img[j, i, c]) if inside else float(pad))
        for c in range(3):
            tot[c] = tot[c] + wy * row[c]
    return [t / (f * f) for t in tot], [v for _, v in wxs], [v for _, v in wys]


# ------------------------------------------------------------------------------------------------ merge
def contains_centre(box, S: int) -> bool:
    """The int32 polygon box[8] contains (S / 2, S / 2): integer cross products on doubled coordinates, an edge counts as inside."""
    P = int(S)
    pos = neg = True
    for q in range(4):
        q1 = (q + 1) & 3
        ax, ay, bx, by = 2 * int(box[2 * q]), 2 * int(box[2 * q + 1]), 2 * int(box[2 * q1]), 2 * int(box[2 * q1 + 1])
        cr = (bx - ax) * (P - ay) - (by - ay) * (P - ax)
        pos = pos and cr >= 0
        neg = neg and cr <= 0
    return pos or neg


def merge_ref(S: int, agree: float, win: np.ndarray, n: int, recs2, counts2, quads2, counts, coarse: np.ndarray, out=None, status=None,
              scale=None):
    """win WINDOW_DT [>= n]; recs2 structured [n][M2] (None when n == 0), counts2 [n], quads2 QUAD_DT [n][M2]; counts [B]; coarse
    QUAD_DT [B][M] -> (out QUAD_DT [B][M], status int32 [B][M], scale float64 [B][M])."""
    B, M = coarse.shape
    out = np.zeros((B, M), SR.QUAD_DT) if out is None else out.copy()
    status = np.zeros((B, M), np.int32) if status is None else status.copy()
    scale = np.zeros((B, M), np.float64) if scale is None else scale.copy()
    where = {(int(win[k]["map"]), int(win[k]["slot"])): k for k in range(n - 1, -1, -1)}      # the first of equal keys, as a lower bound finds
    for b in range(B):
        used = min(max(int(counts[b]), 0), M)
        for t in range(M):
            if t >= used:
                status[b, t], scale[b, t] = NO_WINDOW, 0.0
                continue
            k = where.get((b, t))
            if k is None:
                out[b, t], status[b, t], scale[b, t] = coarse[b, t], NO_WINDOW, 0.0
                continue
            scale[b, t] = win[k]["s"]
            M2 = recs2.shape[1]
            has_valid = "valid" in recs2.dtype.names
            target, best = -1, 0
            for u in range(min(max(int(counts2[k]), 0), M2)):
                r = recs2[k, u]
                if (has_valid and int(r["valid"]) == 0) or int(quads2[k, u]["valid"]) == 0:
                    continue
                if not contains_centre(r["box"], S):
                    continue
                if target < 0 or int(r["area"]) > best:
                    target, best = u, int(r["area"])
            if target < 0:
                st = NO_TARGET
            else:
                q2 = quads2[k, target]
                dc = float(coarse[b, t]["d_mean"])
                if int(np.bitwise_or.reduce(q2["flags"])) & FAIL_MASK:
                    st = REFINE_FAILED
                elif not abs(float(q2["d_mean"]) - dc) <= agree * dc:
                    st = DISAGREES
                else:
                    st = ZOOMED
            if st == ZOOMED:
                o = quads2[k, target].copy()
                o["label"], o["area"] = coarse[b, t]["label"], coarse[b, t]["area"]
                out[b, t] = o
            else:
                out[b, t] = coarse[b, t]
            status[b, t] = st | int(win[k]["status"])
    return out, status, scale
