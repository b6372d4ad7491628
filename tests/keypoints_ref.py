"""Restatement of vk.keypoints (csrc/keypoints.hip: vk_kp_targets, vk_kp_peaks, vk_kp_refine) on the host, for comparison of bytes.
No GPU is needed.

Distances are int64 (numpy) or Python ints; float64 expressions are Python floats evaluated as include/vk_unet.h writes them, every
sum an explicit loop in the stated order; the table comes from Python's math.exp.  The maps are float32 and every value is converted
to float64 before it is used, which is exact."""
from __future__ import annotations

import math

import numpy as np

import subpix_ref as SR

VERT_I32, VERT_F64 = 0, 1
PARABOLA, CENTROID = 0, 1
NO_PEAK, AT_EDGE, SHARED = 128, 256, 512
MAX_RADIUS16, MAX_NMS, MAX_SEARCH, MAX_CWIN = 192, 8, 31, 7
COORD_LIMIT = 1048576.0                      # 2^20

QUAD_DT = SR.QUAD_DT
PEAK_DT = np.dtype([("x", "<i4"), ("y", "<i4"), ("value", "<f4"), ("reserved", "<i4")])
assert PEAK_DT.itemsize == 16


# ------------------------------------------------------------------------------------------------ table
def radius16(sigma: float, cutoff: float = 3.0) -> int:
    return int(math.ceil(16.0 * cutoff * sigma))


def gaussian_table(sigma: float, cutoff: float = 3.0) -> np.ndarray:
    """float32 [R16^2 + 1]: table[k] = float32(exp(-(k / 256) / (2 sigma^2)))."""
    r16 = radius16(sigma, cutoff)
    s2 = 2.0 * sigma * sigma
    return np.array([math.exp(-(k / 256.0) / s2) for k in range(r16 * r16 + 1)], np.float64).astype(np.float32)


def table_of_radius(r16: int, sigma: float) -> np.ndarray:
    """A table of a chosen R16 (the kernel only needs table_len = R16^2 + 1)."""
    s2 = 2.0 * sigma * sigma
    return np.array([math.exp(-(k / 256.0) / s2) for k in range(r16 * r16 + 1)], np.float64).astype(np.float32)


# ------------------------------------------------------------------------------------------------ targets
def fixed_vertices(recs: np.ndarray, counts, field: str, vert_type: int):
    """Per map the used vertices in ascending (slot, q) as Python int pairs (X, Y) in 1/16 pixel."""
    B, M = recs.shape
    has_valid = "valid" in recs.dtype.names
    out = []
    for b in range(B):
        vs = []
        for t in range(min(max(int(counts[b]), 0), M)):
            r = recs[b, t]
            if has_valid and int(r["valid"]) == 0:
                continue
            c = r[field].reshape(8)
            for q in range(4):
                if vert_type == VERT_I32:
                    vs.append((16 * int(c[2 * q]), 16 * int(c[2 * q + 1])))
                else:
                    x, y = float(c[2 * q]), float(c[2 * q + 1])
                    if not (abs(x) <= COORD_LIMIT and abs(y) <= COORD_LIMIT):         # a NaN fails
                        continue
                    vs.append((int(math.floor(x * 16.0 + 0.5)), int(math.floor(y * 16.0 + 0.5))))
        out.append(vs)
    return out


def render_vertices(verts, h: int, w: int, table: np.ndarray) -> np.ndarray:
    """One map from its fixed-point vertices.  A vertex further than R16 from every pixel in an axis contributes nothing (its D is at
    least table_len whatever its size), which keeps the int64 squares exact."""
    n = len(table)
    r16 = int(math.isqrt(n - 1))
    best = np.zeros((h, w), np.float32)
    xs, ys = 16 * np.arange(w, dtype=np.int64), 16 * np.arange(h, dtype=np.int64)
    for X, Y in verts:
        if X < -r16 or X > 16 * (w - 1) + r16 or Y < -r16 or Y > 16 * (h - 1) + r16:
            continue
        dx, dy = xs - X, ys - Y
        D = (dy * dy)[:, None] + (dx * dx)[None, :]
        inside = D < n
        v = table[np.where(inside, D, 0)]
        with np.errstate(invalid="ignore"):
            take = inside & (v > best)                                                # a NaN never wins
        best = np.where(take, v, best)
    return best


def targets_ref(recs: np.ndarray, counts, h: int, w: int, table: np.ndarray, field: str = "box", vert_type: int = VERT_I32) -> np.ndarray:
    """recs structured [B][M] with `field` (int32[8] or float64[8]) and perhaps `valid` -> float32 [B][h][w]."""
    return np.stack([render_vertices(v, h, w, table) for v in fixed_vertices(recs, counts, field, vert_type)])


# ------------------------------------------------------------------------------------------------ peaks
def is_peak(m: np.ndarray, x: int, y: int, min_peak: float, r: int) -> bool:
    h, w = m.shape
    p = m[y, x]
    if not (float(p) >= min_peak):
        return False
    for j in range(max(y - r, 0), min(y + r, h - 1) + 1):
        for i in range(max(x - r, 0), min(x + r, w - 1) + 1):
            q = m[j, i]
            if q > p:
                return False
            if q == p and (j < y or (j == y and i < x)):
                return False
    return True


def peaks_ref(heat: np.ndarray, min_peak: float, r: int, max_peaks: int, out=None):
    """heat float32 [B][h][w] -> (PEAK_DT [B][max_peaks], counts int32 [B]); the slots at or above min(count, max_peaks) as `out`
    had them (zeros without it)."""
    B, h, w = heat.shape
    out = np.zeros((B, max_peaks), PEAK_DT) if out is None else out.copy()
    counts = np.zeros(B, np.int32)
    with np.errstate(invalid="ignore"):
        for b in range(B):
            m = heat[b]
            n = 0
            cand = np.argwhere(m.astype(np.float64) >= min_peak)                      # raster order
            for y, x in cand:
                if is_peak(m, int(x), int(y), min_peak, r):
                    if n < max_peaks:
                        out[b, n] = (int(x), int(y), m[y, x], 0)
                    n += 1
            counts[b] = n
    return out, counts


# ------------------------------------------------------------------------------------------------ refine
def kp_params(method=PARABOLA, search=6, cwin=3, min_peak=0.3, floor_frac=0.25):
    return dict(method=int(method), search=int(search), cwin=int(cwin), min_peak=float(min_peak), floor_frac=float(floor_frac))


def find_peak(m: np.ndarray, sx: int, sy: int, search: int):
    """-> (px, py, value) of the largest non-NaN value in the clipped window, raster-first among equals; None without one."""
    h, w = m.shape
    x0, x1, y0, y1 = max(sx - search, 0), min(sx + search, w - 1), max(sy - search, 0), min(sy + search, h - 1)
    best = None
    for j in range(y0, y1 + 1):
        for i in range(x0, x1 + 1):
            p = m[j, i]
            if p != p:
                continue
            if best is None or p > best[2]:
                best = (i, j, p)
    return best


def refine_vertex(m: np.ndarray, sx: int, sy: int, p: dict):
    """-> (x, y, flags, iters, peak pixel or None)."""
    h, w = m.shape
    pk = find_peak(m, sx, sy, p["search"])
    if pk is None or float(pk[2]) < p["min_peak"]:
        return float(sx), float(sy), NO_PEAK, 0, None
    px, py, cv = pk
    S = p["search"]
    flags = AT_EDGE if (px == sx - S or px == sx + S or py == sy - S or py == sy + S) else 0
    c = float(cv)
    if p["method"] == PARABOLA:
        ox = oy = 0.0
        if 0 < px < w - 1:
            l, r = float(m[py, px - 1]), float(m[py, px + 1])
            den = (l - c) + (r - c)
            if den < 0.0:
                ox = 0.5 * (l - r) / den
        if 0 < py < h - 1:
            l, r = float(m[py - 1, px]), float(m[py + 1, px])
            den = (l - c) + (r - c)
            if den < 0.0:
                oy = 0.5 * (l - r) / den
        return float(px) + ox, float(py) + oy, flags, 1, (px, py)
    fl = p["floor_frac"] * c
    cw = p["cwin"]
    sw = sx_ = sy_ = 0.0
    for j in range(max(py - cw, 0), min(py + cw, h - 1) + 1):
        for i in range(max(px - cw, 0), min(px + cw, w - 1) + 1):
            d = float(m[j, i]) - fl
            g = d if d > 0.0 else 0.0
            sw = sw + g
            sx_ = sx_ + g * float(i - px)
            sy_ = sy_ + g * float(j - py)
    if sw > 0.0:
        with np.errstate(all="ignore"):
            qx, qy = float(np.float64(px) + np.float64(sx_) / np.float64(sw)), float(np.float64(py) + np.float64(sy_) / np.float64(sw))
        return qx, qy, flags, 1, (px, py)
    return float(px), float(py), flags, 1, (px, py)


def refine_one(m: np.ndarray, box, p: dict, affine=(0.0, 0.0, 1.0)):
    """One valid record -> (v[8], vs[8], flags[4], iters[4], d1, d2, d_mean)."""
    ox, oy, inv = (float(a) for a in affine)
    res = [refine_vertex(m, int(box[2 * q]), int(box[2 * q + 1]), p) for q in range(4)]
    v, flags, iters = [0.0] * 8, [0] * 4, [0] * 4
    shared = set()
    for a in range(4):
        for c in range(a + 1, 4):
            if res[a][4] is not None and res[a][4] == res[c][4]:
                shared |= {a, c}
    for q in range(4):
        x, y, f, it, _ = res[q]
        if q in shared:
            x, y, f, it = float(box[2 * q]), float(box[2 * q + 1]), f | SHARED, 0
        v[2 * q], v[2 * q + 1], flags[q], iters[q] = x, y, f, it
    vs = [0.0] * 8
    with np.errstate(all="ignore"):
        for q in range(4):
            vs[2 * q], vs[2 * q + 1] = (v[2 * q] - ox) * inv, (v[2 * q + 1] - oy) * inv
        return (v, vs, flags, iters) + SR.diagonals(v, inv)


def refine_ref(heat: np.ndarray, recs: np.ndarray, counts, p: dict, affine=None, out=None) -> np.ndarray:
    """heat float32 [B][h][w]; recs structured [B][M] with `label`, `area`, `box` (and perhaps `valid`); -> QUAD_DT [B][M], the slots
    at or above min(count, M) as `out` had them."""
    B, M = recs.shape
    out = np.zeros((B, M), QUAD_DT) if out is None else out.copy()
    has_valid = "valid" in recs.dtype.names
    for b in range(B):
        aff = (0.0, 0.0, 1.0) if affine is None else tuple(float(a) for a in affine[b])
        for s in range(min(max(int(counts[b]), 0), M)):
            r = recs[b, s]
            o = np.zeros((), QUAD_DT)
            o["label"], o["area"] = r["label"], r["area"]
            valid = int(r["valid"] != 0) if has_valid else 1
            o["valid"] = valid
            if valid:
                v, vs, flags, iters, d1, d2, dm = refine_one(heat[b], [int(c) for c in r["box"]], p, aff)
                o["v"], o["vs"], o["flags"], o["iters"], o["d1"], o["d2"], o["d_mean"] = v, vs, flags, iters, d1, d2, dm
            out[b, s] = o
    return out
