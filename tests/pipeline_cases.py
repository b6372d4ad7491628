"""Built cases for the kernels that feed every training step and score every validation pass: csrc/augment.hip (k_augment,
k_clahe_tiles, k_letterbox_u8, k_letterbox_mask_u8), csrc/prepost.hip (k_letterbox_pre / _mask / _prob / _post<>) and csrc/metrics.hip
(k_seg_counts<>, k_seg_finalize).  Builders and host references only: numpy, no device.  tests/test_pipeline_cases_cpu.py proves on the
references alone that every case is what its name claims; tests/test_vk_zz_pipeline_sweep_gpu.py runs them on the device.  DESIGN.md 41."""
from __future__ import annotations

import itertools
import math
from fractions import Fraction

import numpy as np

from oracle import augment_oracle as A
from oracle import prepost_oracle as P

F = np.float32
GUARD = 512                      # guard bytes either side of a buffer handed to the C ABI
FILL = 0xA5

# ======================================================================================================= A. augmentation
# 8: the host's minimum; 9, 13: ragged last row block (S % 4 != 0); 66, 67: a second 64-wide tile column of 2 / 3 pixels, so the
# 2-pixel blur apron straddles the column boundary; 130: a third column 2 wide; 128 / 136: CLAHE tile area 256 (one trip of the
# 256-thread loop, exactly) / 289 (a second trip of 33 pixels); 16, 24, 72: one, one and two columns with S % 8 == 0.
AUG_SIZES = (8, 9, 13, 16, 24, 66, 67, 72, 128, 130, 136)
AUG_ALL_IMAGES_AT = (16, 67, 136)
IMAGE_NAMES = ("random", "const0", "const137", "const255", "checker", "ramp", "levels", "tiles", "corners", "levels33")
MASK_NAMES = ("random", "zeros", "ones", "corners", "checker")


def image(name: str, S: int) -> np.ndarray:
    """uint8 RGB [S][S][3], the letterboxed store's layout."""
    yy, xx = np.mgrid[0:S, 0:S]
    if name == "random":
        return np.random.default_rng(1000 + S).integers(0, 256, (S, S, 3), dtype=np.uint8)
    if name.startswith("const"):
        return np.full((S, S, 3), int(name[5:]), np.uint8)
    if name == "checker":                                       # two levels, a different pair per channel
        c = ((yy + xx) & 1).astype(np.uint8)
        return np.stack([c * 200 + 20, c * 3 + 250, 255 - c * 255], -1).astype(np.uint8)
    if name == "ramp":                                          # horizontal: constant down every column
        r = (xx * 255 // max(S - 1, 1)).astype(np.uint8)
        return np.stack([r, 255 - r, r // 2], -1).astype(np.uint8)
    if name == "levels":                                        # every level once per 256 pixels, all channels alike
        v = ((yy * S + xx) % 256).astype(np.uint8)
        return np.stack([v, v, v], -1)
    if name == "tiles":                                         # each of the 8 x 8 CLAHE tiles its own level
        ts = max(S // 8, 1)
        ty, tx = np.minimum(yy // ts, 7), np.minimum(xx // ts, 7)
        v = ((ty * 8 + tx) * 4 + 1).astype(np.uint8)
        return np.stack([v, v, v], -1)
    if name == "levels33":                                      # 33 grey levels in every 17 x 17 tile of S = 136: at limit 1 the
        v = (((yy * S + xx) % 33) * 7).astype(np.uint8)         # clipped count is 289 - 33 = 256, residual exactly 0
        return np.stack([v, v, v], -1)
    if name == "corners":                                       # one bright pixel at each corner, a different colour each
        a = np.zeros((S, S, 3), np.uint8)
        a[0, 0], a[0, -1], a[-1, 0], a[-1, -1] = (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255)
        return a
    raise KeyError(name)


def mask(name: str, S: int) -> np.ndarray:
    """uint8 {0, 1} [S][S]."""
    yy, xx = np.mgrid[0:S, 0:S]
    if name == "random":
        return np.random.default_rng(2000 + S).integers(0, 2, (S, S), dtype=np.uint8)
    if name == "zeros":
        return np.zeros((S, S), np.uint8)
    if name == "ones":
        return np.ones((S, S), np.uint8)
    if name == "corners":
        m = np.zeros((S, S), np.uint8)
        m[0, 0] = m[0, -1] = m[-1, 0] = m[-1, -1] = 1
        return m
    if name == "checker":
        return ((yy + xx) & 1).astype(np.uint8)
    raise KeyError(name)


def image_names(S: int):
    return IMAGE_NAMES if S in AUG_ALL_IMAGES_AT else ("random",)


def items(S: int):
    """The dataset of one size: [(name, image RGB, mask)], every image paired with a mask family in turn."""
    return [(n, image(n, S), mask(MASK_NAMES[i % len(MASK_NAMES)], S)) for i, n in enumerate(IMAGE_NAMES)]


IDENTITY = dict(d4=0, rotate=0, cos_a=1.0, sin_a=0.0, photo=0, alpha=1.0, beta=0.0, blur_ksize=3, noise_scale=0.0, noise_seed=0,
                clahe_clip=1.0)
ROT_33 = (math.cos(math.radians(33.3)), math.sin(math.radians(33.3)))
PHOTOS = (("none", dict(photo=0)), ("rbc", dict(photo=1, alpha=1.17, beta=-0.08)), ("blur3", dict(photo=3, blur_ksize=3)),
          ("blur5", dict(photo=3, blur_ksize=5)), ("clahe", dict(photo=2, clahe_clip=1.37)))
NOISE_ON = dict(noise_scale=math.sqrt(10.0) / 65536.0, noise_seed=12345)
EXACT_ROT = {"x(1,0)": (1.0, 0.0), "x(0,1)": (0.0, 1.0), "x(-1,0)": (-1.0, 0.0), "x(0,-1)": (0.0, -1.0)}
EXACT_ROT_K = {"x(0,1)": 1, "x(-1,0)": 2, "x(0,-1)": 3}       # the np.rot90 an exact pair equals
LIBM_ANGLES = (0.0, 90.0, 180.0, 270.0, 45.0, 1e-3, -137.5)
RBC_CORNERS = ((0.8, -0.2), (0.8, 0.2), (1.2, -0.2), (1.2, 0.2), (1.0, 0.0))
NOISE_SEEDS = (0, 1, 2 ** 31, 2 ** 32 - 1)
NOISE_SCALES = (math.sqrt(10.0) / 65536.0, math.sqrt(50.0) / 65536.0, 0.999)
CLAHE_CLIPS = (1.0, 1.37, 2.0, 40.0)


def _d(name, **kw):
    return dict(IDENTITY, name=name, **kw)


def product_draws(S: int):
    """d4 x rotation x photo x noise: 7 x 2 x 5 x 2 = 140, 112 where S % 8 != 0 (no CLAHE)."""
    out = []
    for d4, rot, (pn, ph), noise in itertools.product(range(7), (0, 1), PHOTOS, (0, 1)):
        if pn == "clahe" and S % 8:
            continue
        kw = dict(d4=d4, **ph)
        if rot:
            kw.update(rotate=1, cos_a=ROT_33[0], sin_a=ROT_33[1])
        if noise:
            kw.update(NOISE_ON)
        out.append(_d(f"p-d4{d4}-r{rot}-{pn}-n{noise}", **kw))
    return out


def family_draws(S: int):
    """Rotation pairs with exact zero components and libm's pairs (alone, and under a rot90 + 5-tap blur), the RBC corners, the noise
    seeds x scales, the CLAHE clips (alone, and under a flip + rotation)."""
    out = [_d("plain")]
    pairs = dict(EXACT_ROT)
    pairs.update({f"m({a:g})": (math.cos(math.radians(a)), math.sin(math.radians(a))) for a in LIBM_ANGLES})
    for n, (c, s) in pairs.items():
        out.append(_d(f"rot-{n}", rotate=1, cos_a=c, sin_a=s))
        out.append(_d(f"rot-{n}-d4_6-blur5", rotate=1, cos_a=c, sin_a=s, d4=6, photo=3, blur_ksize=5))
    for a, b in RBC_CORNERS:
        out.append(_d(f"rbc({a:g},{b:g})", photo=1, alpha=a, beta=b))
    for seed, sc in itertools.product(NOISE_SEEDS, NOISE_SCALES):
        out.append(_d(f"noise-{seed}-{sc:.3g}", noise_scale=sc, noise_seed=seed))
    out.append(_d("noise-1-again-blur3", noise_scale=NOISE_SCALES[0], noise_seed=1, photo=3, blur_ksize=3))
    if S % 8 == 0:
        for clip in CLAHE_CLIPS:
            out.append(_d(f"clahe-{clip:g}", photo=2, clahe_clip=clip))
            out.append(_d(f"clahe-{clip:g}-d4_1-rot", photo=2, clahe_clip=clip, d4=1, rotate=1, cos_a=ROT_33[0], sin_a=ROT_33[1]))
    return out


def all_draws(S: int):
    return product_draws(S) + family_draws(S)


def by_name(draws):
    return {d["name"]: i for i, d in enumerate(draws)}


def augment_ref(img_rgb: np.ndarray, m: np.ndarray, d: dict):
    return A.augment(img_rgb, m, d)


# ---- scalar twins of the oracle's stages (plain Python; compared with the oracle at S <= 16 by the CPU file)
def reflect101(i: int, n: int) -> int:
    if i < 0:
        i = -i
    if i >= n:
        i = 2 * (n - 1) - i
    return i


def blur_twin(img: np.ndarray, k: int) -> np.ndarray:
    """Binomial blur in exact rationals, BORDER_REFLECT_101 spelled out, round half up."""
    w = {3: (1, 2, 1), 5: (1, 4, 6, 4, 1)}[k]
    tot, r, S = sum(w) ** 2, k // 2, img.shape[0]
    out = np.zeros_like(img)
    for y in range(S):
        for x in range(S):
            for c in range(3):
                acc = Fraction(0)
                for i in range(k):
                    for j in range(k):
                        acc += Fraction(w[i] * w[j], tot) * int(img[reflect101(y + i - r, S), reflect101(x + j - r, S), c])
                out[y, x, c] = math.floor(acc + Fraction(1, 2))
    return out


def rotate_taps_twin(S: int, cos_a: float, sin_a: float):
    """Per output pixel: (y0, x0) of the top-left bilinear tap, (yi, xi) of the nearest tap, float32 throughout.  A tap outside
    [0, S) contributes the border value 0."""
    al, be, c = F(cos_a), F(sin_a), F(S / 2.0 - 0.5)
    taps = np.zeros((S, S, 4), np.int64)
    for y in range(S):
        for x in range(S):
            dx, dy = F(F(x) - c), F(F(y) - c)
            sx = F(F(F(al * dx) - F(be * dy)) + c)
            sy = F(F(F(be * dx) + F(al * dy)) + c)
            taps[y, x] = (math.floor(sy), math.floor(sx), math.floor(F(sy + F(0.5))), math.floor(F(sx + F(0.5))))
    return taps


def rotate_mask_twin(m: np.ndarray, cos_a: float, sin_a: float) -> np.ndarray:
    S = m.shape[0]
    taps = rotate_taps_twin(S, cos_a, sin_a)
    out = np.zeros_like(m)
    for y in range(S):
        for x in range(S):
            yi, xi = taps[y, x, 2:]
            if 0 <= yi < S and 0 <= xi < S:
                out[y, x] = m[yi, xi]
    return out


def rotate_image_twin(img: np.ndarray, cos_a: float, sin_a: float) -> np.ndarray:
    S = img.shape[0]
    al, be, c = F(cos_a), F(sin_a), F(S / 2.0 - 0.5)
    out = np.zeros_like(img)

    def tap(yy, xx, ch):
        return F(img[yy, xx, ch]) if 0 <= yy < S and 0 <= xx < S else F(0)

    for y in range(S):
        for x in range(S):
            dx, dy = F(F(x) - c), F(F(y) - c)
            sx = F(F(F(al * dx) - F(be * dy)) + c)
            sy = F(F(F(be * dx) + F(al * dy)) + c)
            x0, y0 = math.floor(sx), math.floor(sy)
            fx, fy = F(sx - F(x0)), F(sy - F(y0))
            for ch in range(3):
                top = F(F(tap(y0, x0, ch) * F(F(1) - fx)) + F(tap(y0, x0 + 1, ch) * fx))
                bot = F(F(tap(y0 + 1, x0, ch) * F(F(1) - fx)) + F(tap(y0 + 1, x0 + 1, ch) * fx))
                val = F(F(top * F(F(1) - fy)) + F(bot * fy))
                out[y, x, ch] = min(max(int(np.rint(val)), 0), 255)
    return out


def clahe_tile_stats(tile: np.ndarray, limit: int):
    """(clipped, residual, lut uint8 [256]) of one tile, OpenCV's clip / redistribute / cdf in plain loops."""
    h = [0] * 256
    for v in tile.ravel().tolist():
        h[v] += 1
    clipped = sum(max(b - limit, 0) for b in h)
    h = [min(b, limit) + clipped // 256 for b in h]
    residual = clipped % 256
    if residual:
        step = max(256 // residual, 1)
        i, left = 0, residual
        while i < 256 and left > 0:
            h[i] += 1
            i += step
            left -= 1
    scale = F(255.0) / F(tile.size)
    lut, cdf = np.zeros(256, np.uint8), 0
    for v in range(256):
        cdf += h[v]
        lut[v] = min(max(int(np.rint(F(F(cdf) * scale))), 0), 255)
    return clipped, residual, lut


def clahe_case_stats(img_rgb: np.ndarray, clip: float):
    """[(clipped, residual)] over the 64 tiles of the undistorted image's L plane."""
    S = img_rgb.shape[0]
    ts, limit = S // 8, A.clahe_limit(clip, S)
    L = A.rgb_to_lab_u8(img_rgb, A.color_tables())[..., 0]
    return [clahe_tile_stats(L[ty * ts:(ty + 1) * ts, tx * ts:(tx + 1) * ts], limit)[:2] for ty in range(8) for tx in range(8)]


M64 = (1 << 64) - 1


def splitmix64_twin(z: int) -> int:
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def noise_isum_twin(seed: int, S: int, y: int, x: int, ch: int) -> int:
    cnt = (y * S + x) * 3 + ch
    base = ((((seed & 0xFFFFFFFF) << 32) | cnt) * 3) & M64
    tot = 0
    for j in range(3):
        z = splitmix64_twin((base + j) & M64)
        tot += (z & 0xFFFF) + ((z >> 16) & 0xFFFF) + ((z >> 32) & 0xFFFF) + (z >> 48)
    return tot


# ======================================================================================================= B. dataset letterbox
LB_SIZES = (8, 24, 67)
LB_SOURCES = ((1, 1), (3, 5), (7, 7), (48, 24), (25, 13))         # at every size
LB_SOURCES_AT = {24: ((24, 24), (24, 12)), 67: ((2048, 37), (37, 2048))}
LB_REFUSED = ((1, 50, 8),)                                          # (h, w, S): geometry_train gives nh = 0


def lb_sources(S: int):
    return LB_SOURCES + LB_SOURCES_AT.get(S, ())


def bgr_image(h: int, w: int) -> np.ndarray:
    """uint8 BGR [h][w][3]: noise with one smooth channel, the three channels never alike (a BGR swap shows)."""
    img = np.random.default_rng(h * 7 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    img[..., 1] = ((yy * 3 + xx * 2) % 256).astype(np.uint8)
    img[0, 0] = (1, 2, 3)
    return img


def raw_mask(h: int, w: int) -> np.ndarray:
    """uint8 [h][w] with the values {0, 1, 2, 255} mixed: everything above 0 is foreground."""
    return np.array([0, 1, 2, 255], np.uint8)[np.random.default_rng(h * 11 + w).integers(0, 4, (h, w))]


def letterbox_ref(img_bgr, m, S, geo=None, pad_value=0):
    """(uint8 RGB [S][S][3], {0,1} [S][S]) as the dataset pipeline stores them; geo = (nh, nw, top, left), the train one by default."""
    h, w = img_bgr.shape[:2]
    nh, nw, top, left = geo if geo is not None else P.geometry_train(h, w, S)[1:]
    sq = P.letterbox(img_bgr, S, nh, nw, top, left, pad_value)[:, :, ::-1]
    out = np.zeros((S, S), np.uint8)
    out[top:top + nh, left:left + nw] = P.resize_nearest((m > 0).astype(np.uint8), nw, nh)
    return np.ascontiguousarray(sq), out


def odd_geometries(h: int, w: int, S: int):
    """Explicit descriptors beside the train convention: the train size at odd (top, left) where it fits, the source's own size
    (copy path) at an odd offset where it fits."""
    _, nh, nw, top, left = P.geometry_train(h, w, S)
    out = []
    for t, l in ((1, 1), (S - nh, S - nw), (1, 0)):
        if 0 <= t <= S - nh and 0 <= l <= S - nw and (t, l) != (top, left):
            out.append((nh, nw, t, l))
    if h <= S - 1 and w <= S - 3 and (h, w) != (nh, nw):
        out.append((h, w, 1, 3))
    return sorted(set(out))


def strided(a: np.ndarray, extra: int = 5) -> tuple:
    """The rows of a [h][w] or [h][w][3] uint8 array laid `extra` bytes apart, FILL in the padding -> (flat uint8, stride)."""
    h = a.shape[0]
    row = a.reshape(h, -1)
    buf = np.full((h, row.shape[1] + extra), FILL, np.uint8)
    buf[:, :row.shape[1]] = row
    return buf.ravel(), row.shape[1] + extra


# ======================================================================================================= C. pre / post-processing
PRE_SIZES = (8, 67)
CONVENTIONS = ("pad_br", "centered", "train")


def pre_sources():
    return LB_SOURCES + LB_SOURCES_AT[24] + LB_SOURCES_AT[67]


POST_SHAPES = {          # S: original (h, w); widths cover w % 4 = 0, 1, 2, 3, the first entry is the copy path for every convention
    8: ((8, 8), (5, 9), (13, 6), (7, 11), (16, 12), (3, 5), (1, 1)),
    67: ((67, 67), (100, 64), (90, 133), (50, 67), (61, 130), (67, 66)),
    256: ((256, 256), (300, 400), (511, 513), (200, 258), (257, 255), (1001, 333)),
}
POST_THRESHOLDS = (0.0, 0.45, 0.5, 1.0)
LATTICE = np.arange(-160, 161, dtype=np.int64).astype(F) / F(8)             # multiples of 1/8 in [-20, 20]: 321 values
SPECIALS = np.array([0.0, 88.0, -88.0, 100.0, -100.0, np.inf, -np.inf, np.nan], F)
# +-1e-30 is in the issue's list and is left out: exp(-x) there is 1 to within half an ulp, and a +2 ulp answer from expf would move
# sigmoid below 0.5 (test_pipeline_cases_cpu.py::test_tiny_logits_fail_the_margin shows it), so equality could not be demanded of them.
DROPPED_SPECIALS = np.array([1e-30, -1e-30], F)


def logit_values() -> np.ndarray:
    return np.concatenate([LATTICE, SPECIALS])


def logit_map(S: int, case_index: int = 0) -> np.ndarray:
    """float32 [S][S]: the specials at fixed positions, the lattice in the other pixels, walked with a stride coprime to 321 (every
    value occurs once S * S >= 329; at S = 8 a map holds 56 consecutive lattice values starting at 56 * case_index, so the seven
    S = 8 cases cover the lattice between them)."""
    lg = np.zeros(S * S, F)
    step = (S * S) // len(SPECIALS)
    at = np.arange(len(SPECIALS)) * step + step // 2
    rest = np.ones(S * S, bool)
    rest[at] = False
    r = np.arange(S * S - len(SPECIALS), dtype=np.int64)
    lg[rest] = LATTICE[((r * 7 if len(r) >= len(LATTICE) else r) + 56 * case_index) % len(LATTICE)]
    lg[at] = SPECIALS
    return lg.reshape(S, S)


def exp_perturbed(x: np.ndarray, ulps: int) -> np.ndarray:
    """exp(-x) in float32 moved by `ulps` units in the last place; exact results (exp(-0) = 1, exp(-inf) = 0, inf, nan) stay: C
    Annex F and IEEE 754 fix them for every implementation."""
    with np.errstate(over="ignore"):
        e = np.exp(-x.astype(F), dtype=F)
    exact = (x == 0) | ~np.isfinite(e) | (e == 0)
    moved = e.copy()
    for _ in range(abs(ulps)):
        moved = np.nextafter(moved, F(np.inf) if ulps > 0 else F(0)).astype(F)
    return np.where(exact, e, moved).astype(F)


def mask_bit(x: np.ndarray, thr: float, ulps: int = 0) -> np.ndarray:
    with np.errstate(invalid="ignore"):
        return (F(1) / (F(1) + exp_perturbed(x, ulps))).astype(F) >= F(thr)


def post_geometry(h: int, w: int, S: int, conv: str):
    geo = P.GEOMETRY[conv](h, w, S)
    return geo if geo[1] > 0 and geo[2] > 0 else None


# ======================================================================================================= D. metrics
MET_SHAPES = ((1, 1), (1, 3), (3, 255), (3, 256), (3, 257), (2, 4096), (65, 16), (130, 16), (2048, 16384), (4096, 1024))
MET_THRESHOLDS = (0.25, 0.5, 0.75)
EPS = 1e-7


def met_inputs(n: int, per: int):
    """(prob float32 [n][per] on the lattice k/16 with every threshold present, target 0/1).  Image 0: empty target; image 1: empty
    prediction (0.25 everywhere: on the lowest threshold, a miss); image 2: full prediction and target."""
    i = np.arange(per, dtype=np.int32)[None, :]
    b = np.arange(n, dtype=np.int32)[:, None]
    prob = (((i * 7 + b * 3) % 17).astype(F) / F(16)).astype(F)
    tgt = (((i * 5 + b) % 3) == 0).astype(F)
    tgt[0] = 0
    if n > 1:
        prob[1] = 0.25
    if n > 2:
        prob[2] = 1.0
        tgt[2] = 1.0
    return prob, tgt


def met_logits(n: int, per: int) -> np.ndarray:
    """Multiples of 1/2 in [-4, 4], exact zeros among them (sigmoid = 0.5: a miss at 0.5)."""
    i = np.arange(per, dtype=np.int32)[None, :]
    b = np.arange(n, dtype=np.int32)[:, None]
    return ((((i * 7 + b * 3) % 17) - 8).astype(F) / F(2)).astype(F)


def met_counts(hit: np.ndarray, tgt: np.ndarray):
    """Integer counts I, P, T per image in int64."""
    hit, t = np.asarray(hit, bool), np.asarray(tgt) != 0
    return (np.count_nonzero(hit & t, axis=1).astype(np.int64), np.count_nonzero(hit, axis=1).astype(np.int64),
            np.count_nonzero(t, axis=1).astype(np.int64))


def met_ref(I, Pn, T, eps: float = EPS):
    """Per-image Dice / IoU in float32 in the reference's order ((2 I + eps) / (P + T + eps), (I + eps) / (P + T - I + eps)) and
    the batch means: a float64 mean (exactly summed) rounded once."""
    I, Pn, T, e = np.asarray(I).astype(F), np.asarray(Pn).astype(F), np.asarray(T).astype(F), F(eps)
    card = (Pn + T).astype(F)
    dice = ((F(2) * I + e).astype(F) / (card + e).astype(F)).astype(F)
    iou = ((I + e).astype(F) / ((card - I).astype(F) + e).astype(F)).astype(F)
    md = F(math.fsum(dice.astype(np.float64).tolist()) / len(dice))
    mu = F(math.fsum(iou.astype(np.float64).tolist()) / len(iou))
    return dice, iou, md, mu


def met_soft_targets(n: int, per: int) -> np.ndarray:
    i = np.arange(per, dtype=np.int64)[None, :]
    b = np.arange(n, dtype=np.int64)[:, None]
    return (((i * 3 + b * 5) % 9).astype(F) / F(8)).astype(F)
