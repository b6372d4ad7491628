"""numpy restatement of vk.micrographs (csrc/micrographs.hip): integer arithmetic only, int64 throughout, the formulas of
include/vk_unet.h written once.  ``render_ref`` gives the bytes ``vk_mg_render`` must give; the pieces (``ideal``, ``blur``,
``noise_term``, ``inside``, ``facet_ids``) are what tests/test_micrographs_cpu.py proves on their own."""
import numpy as np

MAX_INDENTS, MAX_SCRATCHES, MAX_BLOBS, MAX_RECTS = 8, 64, 8, 4
MIN_SIDE, MAX_SIDE, COORD_MARGIN = 16, 1024, 8192
APRON = 3
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
M32 = np.uint64(0xFFFFFFFF)

INDENT_DT = np.dtype([("vx", "<i4", (4,)), ("vy", "<i4", (4,)), ("ax", "<i4"), ("ay", "<i4"), ("shade", "<i4", (4,)), ("slope", "<i4", (4,)),
                      ("ridge", "<i4"), ("ridge_hw", "<i4"), ("halo_r", "<i4"), ("halo_depth", "<i4"), ("reserved", "<i4", (2,))])
SCRATCH_DT = np.dtype([(f, "<i4") for f in ("x", "y", "dx", "dy", "hw", "depth", "t0", "t1")])
BLOB_DT = np.dtype([(f, "<i4") for f in ("x", "y", "r", "dark")])
RECT_DT = np.dtype([("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("thickness", "<i4"), ("color", "<i4", (3,))])
SCENE_DT = np.dtype([("n_indents", "<i4"), ("n_scratches", "<i4"), ("n_blobs", "<i4"), ("n_rects", "<i4"), ("base", "<i4"), ("tint", "<i4", (3,)),
                     ("grad_x", "<i4"), ("grad_y", "<i4"), ("grad_cx", "<i4"), ("grad_cy", "<i4"), ("vig_cx", "<i4"), ("vig_cy", "<i4"),
                     ("vig", "<i4"), ("tex_amp", "<i4"), ("tex_cos", "<i4"), ("tex_sin", "<i4"), ("tex_lu", "<i4"), ("tex_lv", "<i4"),
                     ("tex_seed", "<u4"), ("blur_r", "<i4"), ("noise_amp", "<i4"), ("noise_seed", "<u4"), ("reserved", "<i4", (8,)),
                     ("indents", INDENT_DT, (MAX_INDENTS,)), ("scratches", SCRATCH_DT, (MAX_SCRATCHES,)), ("blobs", BLOB_DT, (MAX_BLOBS,)),
                     ("rects", RECT_DT, (MAX_RECTS,))])
BINOMIAL = {0: (1,), 1: (1, 2, 1), 2: (1, 4, 6, 4, 1), 3: (1, 6, 15, 20, 15, 6, 1)}
NOISE_VAR = 4 * (256 * 256 - 1) // 12          # variance of the sum of four uniform bytes: 4 (256^2 - 1) / 12 = 21845, exactly


def blank_scene(base=128, tint=(256, 256, 256)):
    """A scene with no record, no gradient, vignette, texture, blur or noise: the constant (base tint + 128) >> 8."""
    s = np.zeros((), SCENE_DT)
    s["base"], s["tint"] = base, tint
    s["tex_cos"] = 16384
    return s


def mix(h):
    h = h.astype(np.uint64) & M32
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x7feb352d)) & M32
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x846ca68b)) & M32
    h ^= h >> np.uint64(16)
    return h


def _u32(a):
    return np.asarray(a, np.int64).astype(np.uint64) & M32


def lattice(i, j, seed):
    return (mix(_u32(i) * np.uint64(0x9E3779B1) + _u32(j) * np.uint64(0x85EBCA77) + np.uint64(int(seed)))
            & np.uint64(255)).astype(np.int64)


def texture(s, x, y):
    """T of the pixels (x, y) (int64 arrays of whole pixels)."""
    amp = int(s["tex_amp"])
    if amp == 0:
        return np.zeros(np.broadcast(x, y).shape, np.int64)
    c, sn, lu, lv, seed = int(s["tex_cos"]), int(s["tex_sin"]), int(s["tex_lu"]), int(s["tex_lv"]), int(s["tex_seed"])
    u, v = x * c + y * sn, y * c - x * sn
    iu, fu = u >> (14 + lu), (u >> (6 + lu)) & 255
    iv, fv = v >> (14 + lv), (v >> (6 + lv)) & 255
    top = lattice(iu, iv, seed) * (256 - fu) + lattice(iu + 1, iv, seed) * fu
    bot = lattice(iu, iv + 1, seed) * (256 - fu) + lattice(iu + 1, iv + 1, seed) * fu
    val = (top * (256 - fv) + bot * fv + 32768) >> 16
    return ((val - 128) * amp) >> 8


def _cr(ax, ay, bx, by):
    return ax * by - ay * bx


def inside(ind, X, Y):
    """Pixel centres (X, Y) in 1/16 pixel inside or on the quadrilateral."""
    vx, vy = ind["vx"].astype(np.int64), ind["vy"].astype(np.int64)
    m = np.ones(np.broadcast(X, Y).shape, bool)
    for i in range(4):
        j = (i + 1) & 3
        m &= _cr(vx[j] - vx[i], vy[j] - vy[i], X - vx[i], Y - vy[i]) >= 0
    return m


def facet_ids(ind, X, Y):
    """The facet of every point (whether inside or not): the one wedge between two apex-to-vertex rays; the apex itself: 0."""
    vx, vy, ax, ay = ind["vx"].astype(np.int64), ind["vy"].astype(np.int64), int(ind["ax"]), int(ind["ay"])
    c = [_cr(vx[i] - ax, vy[i] - ay, X - ax, Y - ay) for i in range(4)]
    f = np.zeros(np.broadcast(X, Y).shape, np.int64)
    n = np.zeros_like(f)
    for i in range(4):
        hit = (c[i] >= 0) & (c[(i + 1) & 3] < 0)
        f = np.where(hit, i, f)
        n += hit
    return f, n


def _falloff(R, d2):
    R2 = R * R
    return np.minimum(256, np.maximum(R2 - d2, 0) // (R2 >> 8))


def ideal(s, S, pad=APRON):
    """(image int64 [S + 2 pad, S + 2 pad, 3] in 0..255, mask bool, facet id or -1) over the pixels -pad .. S + pad - 1."""
    ys, xs = np.meshgrid(np.arange(-pad, S + pad, dtype=np.int64), np.arange(-pad, S + pad, dtype=np.int64), indexing="ij")
    X, Y = 16 * xs, 16 * ys
    T = texture(s, xs, ys)
    L = int(s["base"]) + ((int(s["grad_x"]) * (xs - int(s["grad_cx"])) + int(s["grad_y"]) * (ys - int(s["grad_cy"]))) >> 8)
    L = L - ((int(s["vig"]) * ((xs - int(s["vig_cx"])) ** 2 + (ys - int(s["vig_cy"])) ** 2)) >> 16) + T
    for k in range(int(s["n_scratches"])):
        r = s["scratches"][k]
        dx, dy, hw = int(r["dx"]), int(r["dy"]), int(r["hw"])
        qx, qy = X - int(r["x"]), Y - int(r["y"])
        c, t = qx * dy - qy * dx, qx * dx + qy * dy
        L = L + np.where((c * c <= hw * hw * (dx * dx + dy * dy)) & (t >= int(r["t0"])) & (t <= int(r["t1"])), int(r["depth"]), 0)
    for k in range(int(s["n_blobs"])):
        b = s["blobs"][k]
        R = int(b["r"])
        d2 = (X - int(b["x"])) ** 2 + (Y - int(b["y"])) ** 2
        L = L - np.where(d2 < R * R, (int(b["dark"]) * _falloff(R, d2)) >> 8, 0)
    mask = np.zeros(L.shape, bool)
    facet = np.full(L.shape, -1, np.int64)
    for k in range(int(s["n_indents"])):
        ind = s["indents"][k]
        vx, vy, ax, ay = ind["vx"].astype(np.int64), ind["vy"].astype(np.int64), int(ind["ax"]), int(ind["ay"])
        m = inside(ind, X, Y)
        f, _ = facet_ids(ind, X, Y)
        lin = np.zeros(L.shape, np.int64)
        for i in range(4):
            j = (i + 1) & 3
            ex, ey = vx[j] - vx[i], vy[j] - vy[i]
            ce, ca = _cr(ex, ey, X - vx[i], Y - vy[i]), _cr(ex, ey, ax - vx[i], ay - vy[i])
            kk = (256 * np.maximum(ce, 0)) // ca
            lin = np.where(f == i, int(ind["shade"][i]) + ((int(ind["slope"][i]) * kk) >> 8), lin)
        ridge = np.zeros(L.shape, bool)
        hw = int(ind["ridge_hw"])
        qx, qy = X - ax, Y - ay
        for i in range(4):
            wx, wy = vx[i] - ax, vy[i] - ay
            w2, dot, c = wx * wx + wy * wy, qx * wx + qy * wy, _cr(wx, wy, qx, qy)
            ridge |= (dot >= 0) & (dot <= w2) & (c * c <= hw * hw * w2)
        Lin = lin + (T >> 1) + np.where(ridge, int(ind["ridge"]), 0)
        R = int(ind["halo_r"])
        if R > 0:
            d2 = None
            for i in range(4):
                j = (i + 1) & 3
                ex, ey = vx[j] - vx[i], vy[j] - vy[i]
                px, py = X - vx[i], Y - vy[i]
                e2, dot, c = ex * ex + ey * ey, px * ex + py * ey, _cr(ex, ey, px, py)
                d = np.where(dot <= 0, px * px + py * py, np.where(dot >= e2, (X - vx[j]) ** 2 + (Y - vy[j]) ** 2, (c * c) // e2))
                d2 = d if d2 is None else np.minimum(d2, d)
            Lout = L - np.where(d2 < R * R, (int(ind["halo_depth"]) * _falloff(R, d2)) >> 8, 0)
        else:
            Lout = L
        L = np.where(m, Lin, Lout)
        facet = np.where(m, f, facet)
        mask |= m
    tint = s["tint"].astype(np.int64)
    img = np.clip((L[..., None] * tint[None, None, :] + 128) >> 8, 0, 255)
    return img, mask, facet


def blur(img, r):
    """The separable binomial of radius r over [h, w, c] int64, 'valid' part shrunk by APRON on every side (r <= APRON)."""
    w = BINOMIAL[int(r)]
    r = int(r)
    h, wd = img.shape[0] - 2 * APRON, img.shape[1] - 2 * APRON
    rows = sum(w[k] * img[:, APRON - r + k:APRON - r + k + wd] for k in range(2 * r + 1))
    acc = sum(w[k] * rows[APRON - r + k:APRON - r + k + h] for k in range(2 * r + 1))
    return (acc + ((16 ** r) >> 1)) >> (4 * r)


def noise_term(S, seed):
    """t [S, S, 3]: the sum of the four bytes of the counter hash minus 510, in -510 .. 510."""
    idx = np.arange(S * S * 3, dtype=np.uint64)
    h = mix(idx * np.uint64(0x9E3779B1) + np.uint64(int(seed)))
    t = (h & np.uint64(255)) + ((h >> np.uint64(8)) & np.uint64(255)) + ((h >> np.uint64(16)) & np.uint64(255)) + (h >> np.uint64(24))
    return t.astype(np.int64).reshape(S, S, 3) - 510


def render_ref(s, S):
    """One scene (a SCENE_DT record) -> (uint8 [S, S, 3], uint8 {0, 1} [S, S])."""
    img, mask, _ = ideal(s, S)
    out = blur(img, int(s["blur_r"]))
    amp = int(s["noise_amp"])
    if amp:
        out = np.clip(out + ((noise_term(S, int(s["noise_seed"])) * amp + 128) >> 8), 0, 255)
    ys, xs = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    for k in range(int(s["n_rects"])):
        r = s["rects"][k]
        x0, y0, x1, y1, th = (int(r[f]) for f in ("x0", "y0", "x1", "y1", "thickness"))
        hit = (xs >= x0) & (xs <= x1) & (ys >= y0) & (ys <= y1)
        if th > 0:
            hit &= ~((xs >= x0 + th) & (xs <= x1 - th) & (ys >= y0 + th) & (ys <= y1 - th))
        out = np.where(hit[..., None], r["color"].astype(np.int64)[None, None, :], out)
    return out.astype(np.uint8), mask[APRON:APRON + S, APRON:APRON + S].astype(np.uint8)


def render_batch_ref(scenes, S):
    out = [render_ref(s, S) for s in scenes]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def truth_ref(s):
    """Per indentation: vertices float64 [4, 2] in pixels, d1, d2, d_mean, the shoelace area and the inclusive box (x0, y0, x1, y1)."""
    out = []
    for k in range(int(s["n_indents"])):
        ind = s["indents"][k]
        v = np.stack([ind["vx"], ind["vy"]], axis=1).astype(np.float64) / 16.0
        d1, d2 = float(np.hypot(*(v[2] - v[0]))), float(np.hypot(*(v[3] - v[1])))
        x, y = v[:, 0], v[:, 1]
        area = 0.5 * abs(float(np.dot(x, np.roll(y, -1)) - np.dot(y, np.roll(x, -1))))
        out.append(dict(vertices=v, d1=d1, d2=d2, d_mean=0.5 * (d1 + d2), area=area,
                        box=(float(x.min()), float(y.min()), float(x.max()), float(y.max()))))
    return out
