"""A numpy restatement of vk.render's four entry points, written from include/vk_unet.h (not from the kernels): the float32 blend in
explicit np.float32 steps, segment coverage in Python integers, the label through "%.1f", and a hand-written copy of the glyph table.
tests/test_render_cpu.py proves it on its own; tests/test_vk_render_gpu.py holds the device to its bytes."""
from __future__ import annotations

from fractions import Fraction

import numpy as np

MAX_COORD = 1 << 20
LABEL_MAX = 24
COORD_BOX, COORD_V, COORD_VS = 0, 1, 2
PRIM_DT = np.dtype([("rank", "<i4"), ("slot", "<i4"), ("corner", "<i4", (8,)), ("anchor", "<i4", (2,)), ("bbox", "<i4", (4,)), ("diag", "u1", (4,)),
                    ("color", "u1", (3,)), ("label_len", "u1"), ("diag_color", "u1", (3,)), ("thickness", "u1"), ("text_scale", "u1"),
                    ("pad", "u1", (3,)), ("label", "u1", (LABEL_MAX,))])
assert PRIM_DT.itemsize == 104

PALETTE = ((0, 255, 0), (255, 0, 0), (0, 255, 255), (255, 0, 255), (0, 165, 255), (255, 255, 0), (147, 20, 255), (50, 205, 50))
DIAG_COLOR = (0, 0, 255)
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))

# 5 x 7, top row first, '#' = a set cell
_GLYPH_ART = {
    "0": (".###.", "#...#", "#..##", "#.#.#", "##..#", "#...#", ".###."),
    "1": ("..#..", ".##..", "..#..", "..#..", "..#..", "..#..", ".###."),
    "2": (".###.", "#...#", "....#", "...#.", "..#..", ".#...", "#####"),
    "3": ("#####", "...#.", "..#..", "...#.", "....#", "#...#", ".###."),
    "4": ("...#.", "..##.", ".#.#.", "#..#.", "#####", "...#.", "...#."),
    "5": ("#####", "#....", "####.", "....#", "....#", "#...#", ".###."),
    "6": ("..##.", ".#...", "#....", "####.", "#...#", "#...#", ".###."),
    "7": ("#####", "....#", "...#.", "..#..", ".#...", ".#...", ".#..."),
    "8": (".###.", "#...#", "#...#", ".###.", "#...#", "#...#", ".###."),
    "9": (".###.", "#...#", "#...#", ".####", "....#", "...#.", ".##.."),
    "#": (".#.#.", ".#.#.", "#####", ".#.#.", "#####", ".#.#.", ".#.#."),
    " ": (".....", ".....", ".....", ".....", ".....", ".....", "....."),
    "m": (".....", ".....", "##.#.", "#.#.#", "#.#.#", "#...#", "#...#"),
    "e": (".....", ".....", ".###.", "#...#", "#####", "#....", ".###."),
    "a": (".....", ".....", ".###.", "....#", ".####", "#...#", ".####"),
    "n": (".....", ".....", "#.##.", "##..#", "#...#", "#...#", "#...#"),
    "=": (".....", ".....", "#####", ".....", "#####", ".....", "....."),
    ".": (".....", ".....", ".....", ".....", ".....", ".##..", ".##.."),
    "p": (".....", ".....", "####.", "#...#", "####.", "#....", "#...."),
    "x": (".....", ".....", "#...#", ".#.#.", "..#..", ".#.#.", "#...#"),
    "?": (".###.", "#...#", "....#", "...#.", "..#..", ".....", "..#.."),
}
GLYPHS = {ch: [sum(1 << (4 - c) for c in range(5) if row[c] == "#") for row in art] for ch, art in _GLYPH_ART.items()}


# ------------------------------------------------------------------------------------------------ bytes
def f64_to_u8(v: np.ndarray) -> np.ndarray:
    """0 unless v > 0 (a NaN), 255 for v >= 255, else truncation."""
    v = np.asarray(v, np.float64)
    with np.errstate(invalid="ignore"):
        pos = v > 0.0
        return np.where(pos, np.where(v >= 255.0, 255, np.where(pos, v, 0.0).clip(0.0, 255.0).astype(np.int64)), 0).astype(np.uint8)


def unit_to_u8(p: np.ndarray) -> np.ndarray:
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.asarray(p, np.float32) * np.float32(255.0)
        assert v.dtype == np.float32
        pos = v > 0
        return np.where(pos, np.where(v >= 255, 255, np.where(pos, v, 0).clip(0, 255).astype(np.int64)), 0).astype(np.uint8)


def blend(a: np.ndarray, c: np.ndarray, alpha, beta, gamma=0.0) -> np.ndarray:
    """sat_u8(rint(((float)a * alpha + (float)c * beta) + gamma)) in float32, every step rounded on its own."""
    p = np.asarray(a, np.uint8).astype(np.float32) * np.float32(alpha)
    q = np.asarray(c, np.uint8).astype(np.float32) * np.float32(beta)
    r = np.rint((p + q) + np.float32(gamma))
    assert r.dtype == np.float32
    return np.where(r > 0, np.where(r >= 255, 255, r), 0).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ panels
def val_panels_ref(x, y, prob, mean=MEAN, std=STD, color=(0, 140, 255), alpha=1.0, beta=0.35, gamma=0.0, rgb=False, out=None, row_stride=None):
    """x float32 [N][3][H][W], y, prob float32 [N][1][H][W] -> uint8 [N][H][row_stride]; only the first 12 W bytes of a row are written."""
    x = np.asarray(x, np.float32)
    N, _, H, W = x.shape
    row_stride = 12 * W if row_stride is None else row_stride
    res = np.zeros((N, H, row_stride), np.uint8) if out is None else out.copy()
    base = np.zeros((N, H, W, 3), np.uint8)
    for k in range(3):
        v = ((x[:, k].astype(np.float64) * np.float64(std[k])) + np.float64(mean[k])) * 255.0
        base[..., 2 - k] = f64_to_u8(v)
    gt = unit_to_u8(np.asarray(y, np.float32).reshape(N, H, W))
    pd = unit_to_u8(np.asarray(prob, np.float32).reshape(N, H, W))
    lay = np.where((pd > 127)[..., None], np.asarray(color, np.uint8), np.uint8(0)).astype(np.uint8)
    vis = blend(base, lay, alpha, beta, gamma)
    panels = [base, np.repeat(gt[..., None], 3, axis=-1), np.repeat(pd[..., None], 3, axis=-1), vis]
    for i, p in enumerate(panels):
        res[:, :, 3 * W * i:3 * W * (i + 1)] = (p[..., ::-1] if rgb else p).reshape(N, H, 3 * W)
    return res


# ------------------------------------------------------------------------------------------------ primitives
def label_text(idx: int, d: float) -> str:
    d = float(d)
    if d >= 0.0 and d < 1.0e6:
        return "#%d mean=%spx" % (idx, ("%.1f" % d).lstrip("-"))
    return "#%d mean=?px" % idx


def label_digits_rule(d: float) -> str:
    """The header's rule for the digits, with the fused multiply-add replaced by exact rational arithmetic (the residual of a float64
    product is a float64)."""
    hi = d * 10.0
    lo = float(Fraction(d) * 10 - Fraction(hi))
    assert Fraction(lo) == Fraction(d) * 10 - Fraction(hi)
    f = float(np.floor(hi))
    r = ((hi - f) - 0.5) + lo
    n = int(f)
    if r > 0.0 or (r == 0.0 and n % 2 == 1):
        n += 1
    return "%d.%d" % (n // 10, n % 10)


def diagonals(corner) -> tuple:
    """(i1, j1, i2, j2): the first pair of largest squared distance in integers, then the other two corners."""
    c = [int(v) for v in corner]
    best, bi, bj = -1, 0, 1
    for i, j in PAIRS:
        d2 = (c[2 * i] - c[2 * j]) ** 2 + (c[2 * i + 1] - c[2 * j + 1]) ** 2
        if d2 > best:
            best, bi, bj = d2, i, j
    rest = [k for k in range(4) if k not in (bi, bj)]
    return bi, bj, rest[0], rest[1]


def _rint(v: float) -> int:
    return int(np.rint(np.float64(v)))


def primitives_ref(recs: np.ndarray, counts, mode: int, coord_field: str, affine=None, palette=PALETTE, diag_color=DIAG_COLOR, thickness=2,
                   text_scale=2, out=None):
    """recs structured [B][M] (fields label, area, the corners in `coord_field`, d_mean, and valid where the layout has one; cx, cy in
    BOX mode) -> (PRIM_DT [B][M], drawn int32 [B], skipped int32 [B]).  Slots from drawn[b] on keep what `out` holds."""
    B, M = recs.shape
    res = np.zeros((B, M), PRIM_DT) if out is None else out.copy()
    drawn, skipped = np.zeros(B, np.int32), np.zeros(B, np.int32)
    for b in range(B):
        used = min(max(int(counts[b]), 0), M)
        ox, oy, inv = (0.0, 0.0, 1.0) if affine is None or mode == COORD_VS else (float(v) for v in affine[b])
        rows = []
        for t in range(used):
            r = recs[b, t]
            if "valid" in recs.dtype.names and int(r["valid"]) == 0:
                continue
            c = r[coord_field]
            m = [(float(c[q]) - (ox if q % 2 == 0 else oy)) * inv for q in range(8)]
            if mode == COORD_BOX:
                cx, cy = (float(r["cx"]) - ox) * inv, (float(r["cy"]) - oy) * inv
            else:
                cx = (((m[0] + m[2]) + m[4]) + m[6]) * 0.25
                cy = (((m[1] + m[3]) + m[5]) + m[7]) * 0.25
            if not all(abs(v) <= MAX_COORD for v in m + [cx, cy]):         # a NaN fails
                skipped[b] += 1
                continue
            rows.append((t, int(r["area"]), [_rint(v) for v in m], (int(cx) + 6, int(cy) - 6), float(r["d_mean"])))
        drawn[b] = len(rows)
        order = sorted(rows, key=lambda e: e[1], reverse=True)            # stable: the lower slot first on equal area
        for rank, (t, area, X, A, d) in enumerate(order):
            p = np.zeros((), PRIM_DT)
            p["rank"], p["slot"], p["corner"], p["anchor"] = rank, t, X, A
            p["diag"] = diagonals(X)
            p["color"], p["diag_color"] = palette[rank % 8], diag_color
            p["thickness"], p["text_scale"] = thickness, text_scale
            text = label_text(rank + 1, d).encode()
            p["label_len"] = len(text)
            p["label"][:len(text)] = np.frombuffer(text, np.uint8)
            pad = (thickness + 1) // 2
            xs, ys = X[0::2], X[1::2]
            p["bbox"] = (min(min(xs) - pad, A[0]), min(min(ys) - pad, A[1] - 7 * text_scale + 1),
                         max(max(xs) + pad, A[0] + 6 * text_scale * len(text) - 1), max(max(ys) + pad, A[1]))
            res[b, rank] = p
    return res, drawn, skipped


# ------------------------------------------------------------------------------------------------ draw
def seg_covers(px: int, py: int, ax: int, ay: int, bx: int, by: int, t: int) -> bool:
    """4 * dist^2(P, segment A-B) <= t^2 in Python integers."""
    dx, dy, ex, ey = bx - ax, by - ay, px - ax, py - ay
    L, u = dx * dx + dy * dy, ex * dx + ey * dy
    if L == 0 or u <= 0:
        return 4 * (ex * ex + ey * ey) <= t * t
    if u >= L:
        return 4 * ((px - bx) ** 2 + (py - by) ** 2) <= t * t
    cr = dx * ey - dy * ex
    return 4 * cr * cr <= t * t * L


def prim_ok(p) -> bool:
    return (1 <= int(p["thickness"]) <= 8 and 1 <= int(p["text_scale"]) <= 8 and int(p["label_len"]) <= LABEL_MAX
            and all(int(v) < 4 for v in p["diag"]) and all(abs(int(v)) <= MAX_COORD for v in p["corner"])
            and all(abs(int(v)) <= 2 * MAX_COORD for v in p["anchor"]))


def _near(xs, ys, ax, ay, bx, by, reach):
    """float64 estimate: the pixels within `reach` of the segment (a pre-filter only; the decision is seg_covers')."""
    dx, dy = float(bx - ax), float(by - ay)
    L = dx * dx + dy * dy
    s = np.clip(((xs - ax) * dx + (ys - ay) * dy) / L, 0.0, 1.0) if L > 0 else 0.0
    return np.hypot(xs - ax - s * dx, ys - ay - s * dy) <= reach


def prim_paint(p, h: int, w: int, prefilter: bool = True):
    """int8 [h][w]: -1 where record p paints nothing, 0 where it leaves its colour, 1 the diagonal colour: sides, then diagonals, then
    text over them.  Every decision is made in Python integers; `prefilter` only leaves out pixels that a float64 estimate puts more than
    a pixel beyond the reach of every segment and outside the text (tests/test_render_cpu.py shows that it loses none)."""
    layer = np.full((h, w), -1, np.int8)                                   # 0 colour, 1 diag colour
    x0, y0, x1, y1 = (int(v) for v in p["bbox"])
    xa, ya, xb, yb = max(x0, 0), max(y0, 0), min(x1, w - 1), min(y1, h - 1)
    if xa > xb or ya > yb:
        return layer
    C = [int(v) for v in p["corner"]]
    t, ts, n = int(p["thickness"]), int(p["text_scale"]), int(p["label_len"])
    d = [int(v) for v in p["diag"]]
    ax, ay = (int(v) for v in p["anchor"])
    text = bytes(p["label"][:n]).decode("latin1")
    sides = [(q, (q + 1) & 3) for q in range(4)]
    diags = [(d[0], d[1]), (d[2], d[3])]
    ys, xs = np.mgrid[ya:yb + 1, xa:xb + 1].astype(np.float64)
    cand = np.zeros(ys.shape, bool) if prefilter else np.ones(ys.shape, bool)
    if prefilter:
        for i, j in sides + diags:
            cand |= _near(xs, ys, C[2 * i], C[2 * i + 1], C[2 * j], C[2 * j + 1], 0.5 * t + 1.0)
        cand |= (xs >= ax) & (xs < ax + 6 * ts * n) & (ys > ay - 7 * ts) & (ys <= ay)
    for iy, ix in zip(*np.nonzero(cand)):
        X, Y = xa + int(ix), ya + int(iy)
        for i, j in sides:
            if seg_covers(X, Y, C[2 * i], C[2 * i + 1], C[2 * j], C[2 * j + 1], t):
                layer[Y, X] = 0
        for i, j in diags:
            if seg_covers(X, Y, C[2 * i], C[2 * i + 1], C[2 * j], C[2 * j + 1], t):
                layer[Y, X] = 1
        u, v = X - ax, Y - (ay - 7 * ts + 1)
        if 0 <= u < 6 * ts * n and 0 <= v < 7 * ts:
            cell, row = u // ts, v // ts
            k, c = cell // 6, cell % 6
            g = GLYPHS.get(text[k])
            if c < 5 and g is not None and (g[row] >> (4 - c)) & 1:
                layer[Y, X] = 0
    return layer


def draw_ref(src: np.ndarray, mask: np.ndarray, thresh=0.5, color=(0, 0, 255), alpha=1.0, beta=0.35, gamma=0.0, prims=None, drawn=0):
    """src uint8 [h][w][3], mask uint8 (nonzero) or float32 (> thresh) -> (vis_o, vis_b, vis_v), the first `drawn` records of `prims`
    painted over each in list order."""
    h, w = src.shape[:2]
    fg = (mask != 0) if mask.dtype == np.uint8 else (np.asarray(mask, np.float32) > np.float32(thresh))
    lay = np.where(fg[..., None], np.asarray(color, np.uint8), np.uint8(0)).astype(np.uint8)
    vis = [src.copy(), np.repeat(np.where(fg, 255, 0).astype(np.uint8)[..., None], 3, axis=-1), blend(src, lay, alpha, beta, gamma)]
    n = 0 if prims is None else min(max(int(drawn), 0), len(prims))
    for k in range(n):
        p = prims[k]
        if not prim_ok(p):
            continue
        layer = prim_paint(p, h, w)
        for v in vis:
            v[layer == 0] = p["color"]
            v[layer == 1] = p["diag_color"]
    return vis


# ------------------------------------------------------------------------------------------------ reduce
def reduce_ref(img: np.ndarray, k: int) -> np.ndarray:
    h, w = img.shape[:2]
    oh, ow = -(-h // k), -(-w // k)
    out = np.zeros((oh, ow, 3), np.uint8)
    for Y in range(oh):
        for X in range(ow):
            blk = img[Y * k:min(Y * k + k, h), X * k:min(X * k + k, w)].astype(np.int64).reshape(-1, 3)
            n = blk.shape[0]
            out[Y, X] = (blk.sum(axis=0) + n // 2) // n
    return out
