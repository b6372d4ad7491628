"""Restatement of vk.subpix (csrc/subpix.hip, vk_subpix_refine) on the host, for bit-for-bit comparison.  No GPU is needed.

Python floats are IEEE float64 and `+ - * /`, `abs`, `math.sqrt` and `math.floor` round once, so these are the device's operations;
every sum below is an explicit loop in the order include/vk_unet.h states (numpy's pairwise `sum` is not that order).  The map is
float32 and every sample is converted to float64 before it is used, which is exact."""
from __future__ import annotations

import math

import numpy as np

CORNER, LINES = 0, 1
SINGULAR, LEFT_MAP, NOT_CONVERGED, RESTORED, SHORT_SIDE, NO_EDGE, PARALLEL = 1, 2, 4, 8, 16, 32, 64
MAX_WIN, MAX_REACH, MAX_STATIONS, MIN_SIDE = 15, 15, 32, 8.0
DBL_EPS2 = 2.220446049250313e-16 * 2.220446049250313e-16
INF = float("inf")

QUAD_DT = np.dtype([("label", "<i4"), ("area", "<i4"), ("valid", "<i4"), ("reserved", "<i4"), ("flags", "<i4", (4,)), ("iters", "<i4", (4,)),
                    ("v", "<f8", (8,)), ("vs", "<f8", (8,)), ("d1", "<f8"), ("d2", "<f8"), ("d_mean", "<f8")])
assert QUAD_DT.itemsize == 200 and QUAD_DT.fields["d_mean"][1] == 192


def corner_params(win=5, zero_zone=-1, max_iter=40, eps=1e-3):
    return dict(method=CORNER, win=int(win), zero_zone=int(zero_zone), max_iter=int(max_iter), eps=float(eps))


def lines_params(lo=0.1, hi=0.5, n_stations=12, reach=6, level=0.5, max_shift=None):
    return dict(method=LINES, lo=float(lo), hi=float(hi), n_stations=int(n_stations), reach=int(reach), level=float(level),
                max_shift=float(reach if max_shift is None else max_shift))


def weight_table(win: int):
    """wt[k] = exp(-((k - win) / win)^2), k = 0 .. 2 win: the only transcendental of the method, evaluated on the host."""
    return [math.exp(-(((k - win) / win) * ((k - win) / win))) for k in range(2 * win + 1)]


def _finite(v: float) -> bool:
    return abs(v) <= 1.7976931348623157e308


def sample(m: np.ndarray, x: float, y: float) -> float:
    """Bilinear sample of one float32 map [h][w]; NaN coordinates are clamped to 0 like anything that is not above 0."""
    h, w = m.shape
    x = x if x > 0.0 else 0.0
    x = x if x < float(w - 1) else float(w - 1)
    y = y if y > 0.0 else 0.0
    y = y if y < float(h - 1) else float(h - 1)
    x0 = min(int(math.floor(x)), w - 2) if w > 1 else 0
    y0 = min(int(math.floor(y)), h - 2) if h > 1 else 0
    x1 = x0 + 1 if w > 1 else 0
    y1 = y0 + 1 if h > 1 else 0
    fx, fy = x - float(x0), y - float(y0)
    p00, p01, p10, p11 = float(m[y0, x0]), float(m[y0, x1]), float(m[y1, x0]), float(m[y1, x1])
    top = p00 * (1.0 - fx) + p01 * fx
    bot = p10 * (1.0 - fx) + p11 * fx
    return top * (1.0 - fy) + bot * fy


# ------------------------------------------------------------------------------------------------ corner
def corner_vertex(m: np.ndarray, sx: float, sy: float, p: dict, wt):
    """-> (x, y, flags, iters)."""
    h, w = m.shape
    win, zz, max_iter, eps2 = p["win"], p["zero_zone"], p["max_iter"], p["eps"] * p["eps"]
    n = 2 * win + 3
    qx, qy = sx, sy
    flags = iters = 0
    while True:
        S = [[sample(m, qx + float(i - win - 1), qy + float(j - win - 1)) for i in range(n)] for j in range(n)]
        a = b = c = bb1 = bb2 = 0.0
        for j in range(2 * win + 1):                     # rows top to bottom
            ra = rb = rc = r1 = r2 = 0.0
            py = float(j - win)
            for i in range(2 * win + 1):                 # left to right
                px = float(i - win)
                mk = wt[j] * wt[i]
                if zz >= 0 and abs(i - win) <= zz and abs(j - win) <= zz:
                    mk = 0.0
                gx = S[j + 1][i + 2] - S[j + 1][i]
                gy = S[j + 2][i + 1] - S[j][i + 1]
                gxx, gxy, gyy = gx * gx, gx * gy, gy * gy
                ra = ra + mk * gxx
                rb = rb + mk * gxy
                rc = rc + mk * gyy
                r1 = r1 + mk * (gxx * px + gxy * py)
                r2 = r2 + mk * (gxy * px + gyy * py)
            a, b, c, bb1, bb2 = a + ra, b + rb, c + rc, bb1 + r1, bb2 + r2
        det = a * c - b * b
        if not (abs(det) > DBL_EPS2) or not _finite(det):
            flags |= SINGULAR
            break
        stx = (c * bb1 - b * bb2) / det
        sty = (a * bb2 - b * bb1) / det
        qx, qy = qx + stx, qy + sty
        iters += 1
        if stx * stx + sty * sty <= eps2:
            break
        if not (qx >= 0.0 and qx < float(w) and qy >= 0.0 and qy < float(h)):
            flags |= LEFT_MAP
            break
        if iters >= max_iter:
            flags |= NOT_CONVERGED
            break
    if not (abs(qx - sx) <= float(win) and abs(qy - sy) <= float(win)):
        qx, qy = sx, sy
        flags |= RESTORED
    return qx, qy, flags, iters


# ------------------------------------------------------------------------------------------------ lines
def crossing(g, level: float, reach: int):
    """g[t + reach], t = -reach .. reach -> (position, found): the crossing g_t >= level > g_{t+1} of least |position|, the smaller t on
    a tie.  A NaN sample never satisfies a compare and a NaN position never wins."""
    best, best_abs = 0.0, INF
    for t in range(-reach, reach):
        g0, g1 = g[t + reach], g[t + reach + 1]
        if g0 >= level and level > g1:
            pos = float(t) + (g0 - level) / (g0 - g1)
            if abs(pos) < best_abs:
                best, best_abs = pos, abs(pos)
    return best, best_abs < INF


def tls_line(xs, ys):
    """Total least squares through the points in their order -> (cx, cy, vx, vy)."""
    n = float(len(xs))
    sx = sy = 0.0
    for x, y in zip(xs, ys):
        sx, sy = sx + x, sy + y
    cx, cy = sx / n, sy / n
    sxx = syy = sxy = 0.0
    for x, y in zip(xs, ys):
        dx, dy = x - cx, y - cy
        sxx, syy, sxy = sxx + dx * dx, syy + dy * dy, sxy + dx * dy
    hs, hd = (sxx + syy) * 0.5, (sxx - syy) * 0.5
    lam = hs + math.sqrt(hd * hd + sxy * sxy)
    if abs(lam - sxx) > abs(lam - syy):
        return cx, cy, sxy, lam - sxx
    return cx, cy, lam - syy, sxy


def side_line(m: np.ndarray, box, i: int, j: int, cx: float, cy: float, p: dict):
    """The side from start vertex i towards start vertex j -> (flags, n_crossings, line or None)."""
    vx, vy = float(box[2 * i]), float(box[2 * i + 1])
    dx, dy = float(box[2 * j]) - vx, float(box[2 * j + 1]) - vy
    L = math.sqrt(dx * dx + dy * dy)
    if L < MIN_SIDE:
        return SHORT_SIDE, 0, None
    nx, ny = dy / L, -dx / L
    if nx * (vx - cx) + ny * (vy - cy) < 0.0:
        nx, ny = -nx, -ny
    ns, R = p["n_stations"], p["reach"]
    xs, ys = [], []
    for k in range(ns):
        f = p["lo"] + ((p["hi"] - p["lo"]) * float(k)) / float(ns - 1)
        stx, sty = vx + dx * f, vy + dy * f
        g = [sample(m, stx + float(t) * nx, sty + float(t) * ny) for t in range(-R, R + 1)]
        pos, found = crossing(g, p["level"], R)
        if found:
            xs.append(stx + pos * nx)
            ys.append(sty + pos * ny)
    if len(xs) < 3:
        return NO_EDGE, len(xs), None
    return 0, len(xs), tls_line(xs, ys)


def lines_vertex(m: np.ndarray, box, i: int, p: dict):
    """-> (x, y, flags, crossings found on the two sides)."""
    sx, sy = float(box[2 * i]), float(box[2 * i + 1])
    cx = (((float(box[0]) + float(box[2])) + float(box[4])) + float(box[6])) * 0.25
    cy = (((float(box[1]) + float(box[3])) + float(box[5])) + float(box[7])) * 0.25
    f1, n1, l1 = side_line(m, box, i, (i + 1) & 3, cx, cy, p)
    f2, n2, l2 = side_line(m, box, i, (i + 3) & 3, cx, cy, p)
    flags = f1 | f2
    if flags:
        return sx, sy, flags, n1 + n2
    c1x, c1y, v1x, v1y = l1
    c2x, c2y, v2x, v2y = l2
    den = v1x * v2y - v1y * v2x
    if not (den * den > 1e-6 * ((v1x * v1x + v1y * v1y) * (v2x * v2x + v2y * v2y))):
        return sx, sy, PARALLEL, n1 + n2
    ex, ey = c2x - c1x, c2y - c1y
    s = (ex * v2y - ey * v2x) / den
    qx, qy = c1x + s * v1x, c1y + s * v1y
    if not (abs(qx - sx) <= p["max_shift"] and abs(qy - sy) <= p["max_shift"]):
        return sx, sy, RESTORED, n1 + n2
    return qx, qy, 0, n1 + n2


# ------------------------------------------------------------------------------------------------ records
def diagonals(v, inv_scale: float):
    """The existing records' rule on float64 vertices: the longest of the six pairs (the first on a tie), then the other two."""
    dmax, i1, j1 = -1.0, 0, 1
    for a in range(4):
        for c in range(a + 1, 4):
            dx, dy = v[2 * a] - v[2 * c], v[2 * a + 1] - v[2 * c + 1]
            d = math.sqrt(dx * dx + dy * dy)
            if d > dmax:
                dmax, i1, j1 = d, a, c
    r = [q for q in range(4) if q != i1 and q != j1]
    ex, ey = v[2 * r[0]] - v[2 * r[1]], v[2 * r[0] + 1] - v[2 * r[1] + 1]
    d1 = dmax * inv_scale
    d2 = math.sqrt(ex * ex + ey * ey) * inv_scale
    return d1, d2, 0.5 * (d1 + d2)


def refine_one(m: np.ndarray, box, p: dict, affine=(0.0, 0.0, 1.0), wt=None):
    """One valid record -> (v[8], vs[8], flags[4], iters[4], d1, d2, d_mean)."""
    ox, oy, inv = (float(a) for a in affine)
    if p["method"] == CORNER and wt is None:
        wt = weight_table(p["win"])
    v, flags, iters = [0.0] * 8, [0] * 4, [0] * 4
    for i in range(4):
        if p["method"] == CORNER:
            x, y, f, it = corner_vertex(m, float(box[2 * i]), float(box[2 * i + 1]), p, wt)
        else:
            x, y, f, it = lines_vertex(m, box, i, p)
        v[2 * i], v[2 * i + 1], flags[i], iters[i] = x, y, f, it
    vs = [0.0] * 8
    for i in range(4):
        vs[2 * i], vs[2 * i + 1] = (v[2 * i] - ox) * inv, (v[2 * i + 1] - oy) * inv
    return (v, vs, flags, iters) + diagonals(v, inv)


def refine_ref(prob: np.ndarray, recs: np.ndarray, counts, p: dict, affine=None, out=None, wt=None) -> np.ndarray:
    """prob float32 [B][h][w]; recs structured [B][M] with `label`, `area`, `box` (and `valid` for the quadrilateral fit); counts [B].
    -> QUAD_DT [B][M]: slots 0 .. min(count, M) - 1 written, the rest as `out` had them (zeros when `out` is None)."""
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
                v, vs, flags, iters, d1, d2, dm = refine_one(prob[b], [int(c) for c in r["box"]], p, aff, wt)
                o["v"], o["vs"], o["flags"], o["iters"], o["d1"], o["d2"], o["d_mean"] = v, vs, flags, iters, d1, d2, dm
            out[b, s] = o
    return out
