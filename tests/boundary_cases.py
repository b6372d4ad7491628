"""Built cases of vk.boundary, shared by test_boundary_cpu.py and test_vk_boundary_gpu.py.  numpy only."""
import numpy as np

CPU_SHAPES = [(1, 1), (1, 37), (29, 1), (7, 5), (33, 65), (40, 40)]
LINE_SIZES = (1, 63, 64, 65, 1100)            # one wave of columns, one more, one less; several 256-pixel row strides
GPU_SHAPES = sorted({(1, n) for n in LINE_SIZES} | {(n, 1) for n in LINE_SIZES} | {(7, 5), (33, 65), (96, 200), (64, 64)})
SITES = ("fg", "bg", "edge")
TOLERANCES = (1.0, 2.0, 3.0)
TOL2 = (1, 4, 9)
BAND2 = 4


def patterns(h: int, w: int, seed: int = 0):
    """[(name, uint8 {0, 1} [h][w])]: empty, full, one site in each corner (the longest search), a checkerboard, random at densities
    0.5 and 0.01, one horizontal and one vertical line."""
    rng = np.random.default_rng([seed, h, w])
    out = [("empty", np.zeros((h, w), np.uint8)), ("full", np.ones((h, w), np.uint8))]
    for name, (y, x) in (("corner00", (0, 0)), ("corner01", (0, w - 1)), ("corner10", (h - 1, 0)), ("corner11", (h - 1, w - 1))):
        m = np.zeros((h, w), np.uint8)
        m[y, x] = 1
        out.append((name, m))
    yy, xx = np.mgrid[0:h, 0:w]
    out.append(("checker", ((yy + xx) & 1).astype(np.uint8)))
    out.append(("random0.5", (rng.random((h, w)) < 0.5).astype(np.uint8)))
    out.append(("random0.01", (rng.random((h, w)) < 0.01).astype(np.uint8)))
    m = np.zeros((h, w), np.uint8)
    m[h // 3, :] = 1
    out.append(("hline", m))
    m = np.zeros((h, w), np.uint8)
    m[:, (2 * w) // 3] = 1
    out.append(("vline", m))
    return out


def as_f32(mask: np.ndarray, threshold: float = 0.5, seed: int = 1) -> np.ndarray:
    """A float32 map whose foreground (v > threshold) is ``mask``: background pixels include values exactly AT the threshold,
    foreground pixels the next float32 above it."""
    rng = np.random.default_rng(seed)
    t = np.float32(threshold)
    pick = rng.integers(0, 2, size=mask.shape).astype(bool)
    lo = np.where(pick, t, np.float32(0.1)).astype(np.float32)
    hi = np.where(pick, np.nextafter(t, np.float32(2.0)), np.float32(0.9)).astype(np.float32)
    return np.where(mask != 0, hi, lo).astype(np.float32)


def squares_pair():
    """Two 20 x 20 squares in a 48 x 48 map, offset by (4, 3): max2 = 25, 76 edge pixels each, q95_2 = 17, ASSD 3.2316540947811..."""
    a = np.zeros((48, 48), np.uint8)
    b = np.zeros((48, 48), np.uint8)
    a[10:30, 10:30] = 1
    b[14:34, 13:33] = 1
    return a, b


def pair_cases():
    """[(name, pred, gt)] uint8: the hand case and the degenerate pairs."""
    a, b = squares_pair()
    z = np.zeros((48, 48), np.uint8)
    one = z.copy()
    one[20, 31] = 1
    border = z.copy()
    border[0:12, 30:48] = 1                      # touches the top and the right border: those sides are no boundary
    full = np.ones((48, 48), np.uint8)
    return [("squares", a, b), ("identical", a, a), ("pred empty", z, b), ("gt empty", a, z), ("both empty", z, z), ("one pixel", one, b),
            ("border", border, a), ("full vs square", full, a), ("full vs full", full, full)]


def random_pair(h: int, w: int, seed: int = 5):
    """Blobs rather than noise: a few discs, and the same discs moved and resized."""
    rng = np.random.default_rng([seed, h, w])
    yy, xx = np.mgrid[0:h, 0:w]
    a = np.zeros((h, w), bool)
    b = np.zeros((h, w), bool)
    for _ in range(4):
        cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(3, min(h, w) / 3)
        a |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
        b |= (yy - cy - rng.uniform(-3, 3)) ** 2 + (xx - cx - rng.uniform(-3, 3)) ** 2 <= (r + rng.uniform(-2, 2)) ** 2
    return a.astype(np.uint8), b.astype(np.uint8)


def real_mask(golden_dir, idx: int) -> np.ndarray:
    """uint8 {0, 1} [h][w]: mask idx of tests/golden/real_masks.npz (bit-packed rows)."""
    z = np.load(golden_dir / "real_masks.npz")
    h, w = (int(v) for v in z[f"shape_{idx}"])
    return np.unpackbits(z[f"bits_{idx}"], axis=1)[:, :w].reshape(h, w).astype(np.uint8)


def letterboxed(mask: np.ndarray, S: int) -> np.ndarray:
    """``mask`` scaled to fit S x S (nearest sample at pixel centres) and centred on zeros."""
    h, w = mask.shape
    s = S / max(h, w)
    nh, nw = max(1, int(round(h * s))), max(1, int(round(w * s)))
    ys = np.minimum(((np.arange(nh) + 0.5) * h / nh).astype(int), h - 1)
    xs = np.minimum(((np.arange(nw) + 0.5) * w / nw).astype(int), w - 1)
    out = np.zeros((S, S), np.uint8)
    top, left = (S - nh) // 2, (S - nw) // 2
    out[top:top + nh, left:left + nw] = mask[ys][:, xs]
    return out


def shifted(mask: np.ndarray, dy: int, dx: int) -> np.ndarray:
    out = np.zeros_like(mask)
    h, w = mask.shape
    out[max(dy, 0):h + min(dy, 0), max(dx, 0):w + min(dx, 0)] = mask[max(-dy, 0):h + min(-dy, 0), max(-dx, 0):w + min(-dx, 0)]
    return out
