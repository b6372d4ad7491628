"""vk.boundary restated in numpy: what vk_edt_sq, vk_boundary_phi, vk_boundary_stats and vk_boundary_loss compute.
Distances are integers; the square roots and the loss are float64.  numpy only."""
import numpy as np

NONE = 2 ** 31 - 1            # VK_EDT_NONE
INF = 1 << 30                 # "no site in this column"
MAX_SIDE = 4096
STAT_INT_FIELDS = ("n_pred", "n_gt", "area_pred", "area_gt", "max2_pg", "max2_gp", "q95_2_pg", "q95_2_gp", "band_inter", "band_union", "flags")


def foreground(src: np.ndarray, threshold: float = 0.5) -> np.ndarray:
    """bool map: != 0 for uint8, v > threshold (compared in float32) for float32."""
    src = np.asarray(src)
    if src.dtype == np.uint8:
        return src != 0
    return src.astype(np.float32) > np.float32(threshold)


def edge_of(fg: np.ndarray) -> np.ndarray:
    """The inner boundary: foreground pixels with a 4-neighbour inside the image in the background (outside counts as foreground)."""
    p = np.pad(fg.astype(bool), 1, constant_values=True)
    full = p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:]
    return fg.astype(bool) & ~full


def sites_of(fg: np.ndarray, sites: str) -> np.ndarray:
    return {"fg": fg.astype(bool), "bg": ~fg.astype(bool), "edge": edge_of(fg)}[sites]


def edt_brute(site: np.ndarray) -> np.ndarray:
    """All pairs: int64 [h][w], NONE where the image holds no site."""
    h, w = site.shape
    ys, xs = np.nonzero(site)
    if len(ys) == 0:
        return np.full((h, w), NONE, np.int64)
    yy, xx = np.mgrid[0:h, 0:w]
    out = np.full((h, w), NONE, np.int64)
    for a in range(0, len(ys), 256):
        d = (yy[..., None] - ys[a:a + 256]) ** 2 + (xx[..., None] - xs[a:a + 256]) ** 2
        out = np.minimum(out, d.min(axis=2))
    return out


def column_pass(site: np.ndarray) -> np.ndarray:
    """g^2: the squared distance to the nearest site of the same column, INF where the column holds none."""
    h, w = site.shape
    far = 1 << 14
    g = np.full((h, w), far, np.int64)
    run = np.full(w, far, np.int64)
    for y in range(h):
        run = np.where(site[y], 0, np.minimum(run + 1, far))
        g[y] = run
    run = np.full(w, far, np.int64)
    for y in range(h - 1, -1, -1):
        run = np.where(site[y], 0, np.minimum(run + 1, far))
        g[y] = np.minimum(g[y], run)
    return np.where(g >= far, INF, g * g)


def edt_separable(site: np.ndarray) -> np.ndarray:
    """Columns, then min over x' of (x - x')^2 + g^2(x') per row, offset by offset; it stops once dx^2 reaches the largest value left,
    beyond which no pixel can improve: exact."""
    g2 = column_pass(site)
    w = site.shape[1]
    out = g2.copy()
    for d in range(1, w):
        dd = d * d
        if dd >= out.max():
            break
        out[:, d:] = np.minimum(out[:, d:], g2[:, :-d] + dd)
        out[:, :-d] = np.minimum(out[:, :-d], g2[:, d:] + dd)
    return np.where(out >= INF, NONE, out)


def edt_sq(src: np.ndarray, sites: str = "fg", threshold: float = 0.5, brute: bool = False) -> np.ndarray:
    """int32 [h][w] or [b][h][w] of vk_edt_sq."""
    src = np.asarray(src)
    if src.ndim == 3:
        return np.stack([edt_sq(s, sites, threshold, brute) for s in src])
    site = sites_of(foreground(src, threshold), sites)
    return (edt_brute(site) if brute else edt_separable(site)).astype(np.int32)


def phi_from_d2(d2_fg: np.ndarray, d2_bg: np.ndarray) -> np.ndarray:
    """float32 map of vk_boundary_phi from the two maps (any shape)."""
    a, b = np.asarray(d2_fg, np.int64), np.asarray(d2_bg, np.int64)
    out = np.zeros(a.shape, np.float32)
    bgp = (a > 0) & (a != NONE)
    out[bgp] = np.sqrt(a[bgp].astype(np.float64)).astype(np.float32)
    fgp = (a <= 0) & (b != NONE)
    out[fgp] = (1.0 - np.sqrt(b[fgp].astype(np.float64))).astype(np.float32)
    return out


def phi(target: np.ndarray, threshold: float = 0.5) -> np.ndarray:
    return phi_from_d2(edt_sq(target, "fg", threshold), edt_sq(target, "bg", threshold))


def nearest_rank(n: int) -> int:
    """1-based rank of the 95th percentile among n sorted values."""
    return (95 * n + 99) // 100


def stats(pred: np.ndarray, gt: np.ndarray, pred_threshold: float = 0.5, gt_threshold: float = 0.5, tol2=(1, 4, 9), band2: int = 4) -> dict:
    """The vk_boundary_rec of one image as a dict (within_* are lists of 8)."""
    pf, gf = foreground(pred, pred_threshold), foreground(gt, gt_threshold)
    pe, ge = edge_of(pf), edge_of(gf)
    d_to_g, d_to_p = edt_separable(ge), edt_separable(pe)
    r = dict(n_pred=int(pe.sum()), n_gt=int(ge.sum()), area_pred=int(pf.sum()), area_gt=int(gf.sum()))
    defined = r["n_pred"] > 0 and r["n_gt"] > 0
    for tag, own, d in (("pg", pe, d_to_g), ("gp", ge, d_to_p)):
        v = np.sort(d[own]) if defined else np.zeros(0, np.int64)
        r["max2_" + tag] = int(v[-1]) if defined else -1
        r["q95_2_" + tag] = int(v[nearest_rank(len(v)) - 1]) if defined else -1
        r["sum_" + tag] = float(np.sqrt(v.astype(np.float64)).sum()) if defined else 0.0
        r["within_" + tag] = [int((v <= tol2[k]).sum()) if k < len(tol2) and defined else 0 for k in range(8)]
    pb = pf & (edt_separable(~pf) <= band2)
    gb = gf & (edt_separable(~gf) <= band2)
    r["band_inter"], r["band_union"] = int((pb & gb).sum()), int((pb | gb).sum())
    r["flags"] = (1 if r["area_pred"] == 0 else 0) | (2 if r["area_gt"] == 0 else 0)
    return r


def metrics(r: dict, n_tol: int, scale: float = 1.0) -> dict:
    """hd, hd95, assd, nsd[k], boundary_iou of one record: both boundaries empty -> distances 0, ratios 1; one empty -> inf and 0."""
    n_p, n_g = r["n_pred"], r["n_gt"]
    if n_p == 0 and n_g == 0:
        return dict(hd=0.0, hd95=0.0, assd=0.0, nsd=[1.0] * n_tol, boundary_iou=1.0)
    if n_p == 0 or n_g == 0:
        return dict(hd=float("inf"), hd95=float("inf"), assd=float("inf"), nsd=[0.0] * n_tol, boundary_iou=0.0)
    return dict(hd=scale * float(np.sqrt(max(r["max2_pg"], r["max2_gp"]))), hd95=scale * float(np.sqrt(max(r["q95_2_pg"], r["q95_2_gp"]))),
                assd=scale * (r["sum_pg"] + r["sum_gp"]) / (n_p + n_g),
                nsd=[(r["within_pg"][k] + r["within_gp"][k]) / (n_p + n_g) for k in range(n_tol)],
                boundary_iou=r["band_inter"] / r["band_union"] if r["band_union"] else 1.0)


def sigmoid64(x: np.ndarray) -> np.ndarray:
    x = np.asarray(x, np.float64)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def loss(logits: np.ndarray, phi_map: np.ndarray, grad_scale: float = 1.0):
    """(value, gradient) in float64: mean of sigmoid(x) phi, and grad_scale phi p (1 - p) / count, with 1 - p = sigmoid(-x) taken
    directly (1.0 - p cancels for large x)."""
    p, q = sigmoid64(logits), sigmoid64(-np.asarray(logits, np.float64))
    f = np.asarray(phi_map, np.float64)
    return float((p * f).sum() / p.size), ((f * (p * q)) * grad_scale) / p.size
