"""Restatement of vk.copypaste (csrc/copypaste.hip, vickers-hardness-unet_amd/copypaste.py) in numpy, for byte-for-byte comparison.
No GPU is needed.  Everything is integer arithmetic in int64, written the way include/vk_unet.h states it: boxes and areas of a slot
map, the 7 x 7 binomial alpha, the fixed-point bilinear paste in list order, and the host records of the instance bank."""
from __future__ import annotations

import numpy as np

B7 = np.array([1, 6, 15, 20, 15, 6, 1], np.int64)
MAX_PASTES = 8
REC_FIELDS = ("donor", "sx0", "sy0", "sw", "sh", "d4", "dx0", "dy0", "dw", "dh")
RECORD_DT = np.dtype([(f, "<i4") for f in ("item", "slot", "x0", "y0", "x1", "y1", "area", "donor")])


# ------------------------------------------------------------------------------------------------ boxes
def boxes_ref(slots: np.ndarray, max_slots: int) -> np.ndarray:
    """int32 [B][h][w] -> int32 [B][max_slots][5] = x0, y0, x1, y1 (inclusive), area; an empty slot is (w, h, -1, -1, 0)."""
    B, h, w = slots.shape
    out = np.empty((B, max_slots, 5), np.int32)
    out[:] = (w, h, -1, -1, 0)
    for b in range(B):
        for s in np.unique(slots[b]):
            if 0 <= s < max_slots:
                ys, xs = np.nonzero(slots[b] == s)
                out[b, s] = (xs.min(), ys.min(), xs.max(), ys.max(), len(xs))
    return out


# ------------------------------------------------------------------------------------------------ alpha
def acc_ref(kept: np.ndarray) -> np.ndarray:
    """{0,1} [h][w] -> int64 [h][w]: the 7 x 7 binomial sum, taps outside the map 0."""
    h, w = kept.shape
    p = np.zeros((h + 6, w + 6), np.int64)
    p[3:3 + h, 3:3 + w] = kept
    rows = sum(int(B7[d]) * p[:, d:d + w] for d in range(7))
    return sum(int(B7[d]) * rows[d:d + h] for d in range(7))


def alpha_of(acc: np.ndarray) -> np.ndarray:
    return np.minimum(255, (acc * 2040 + 2048) >> 12).astype(np.uint8)


def kept_alpha_ref(slots: np.ndarray):
    """int32 [B][h][w] -> (kept, alpha), uint8 [B][h][w] each."""
    kept = (slots >= 0).astype(np.uint8)
    return kept, np.stack([alpha_of(acc_ref(k)) for k in kept])


# ------------------------------------------------------------------------------------------------ paste
def turned(P: np.ndarray, d4: int) -> np.ndarray:
    return np.rot90(P[:, ::-1] if d4 & 4 else P, d4 & 3)


def axis_src(t: int, d: int) -> np.ndarray:
    """Source coordinate (x 256) of every destination index 0..d-1 on an axis of source length t."""
    i = np.arange(d, dtype=np.int64)
    return np.clip(((2 * i + 1) * t * 256) // (2 * d) - 128, 0, (t - 1) * 256)


def resample(T: np.ndarray, U: np.ndarray, V: np.ndarray) -> np.ndarray:
    """T [th][tw] or [th][tw][C] -> int64 [dh][dw](...): the fixed-point bilinear of the header."""
    T = T.astype(np.int64)
    th, tw = T.shape[:2]
    x0, fx, y0, fy = U >> 8, U & 255, V >> 8, V & 255
    x1, y1 = np.minimum(x0 + 1, tw - 1), np.minimum(y0 + 1, th - 1)
    fx, fy = fx[None, :], fy[:, None]
    if T.ndim == 3:
        fx, fy = fx[..., None], fy[..., None]
    top = T[y0][:, x0] * (256 - fx) + T[y0][:, x1] * fx
    bot = T[y1][:, x0] * (256 - fx) + T[y1][:, x1] * fx
    return (top * (256 - fy) + bot * fy + 32768) >> 16


def rendered(images, kept, alpha, rec):
    """The whole destination box of one record: (val int64 [dh][dw][3], a int64 [dh][dw], k uint8 [dh][dw])."""
    r = {f: int(rec[f]) for f in REC_FIELDS}
    box = (slice(r["sy0"], r["sy0"] + r["sh"]), slice(r["sx0"], r["sx0"] + r["sw"]))
    T_rgb, T_a, T_k = (turned(m[r["donor"]][box], r["d4"]) for m in (images, alpha, kept))
    th, tw = T_a.shape
    U, V = axis_src(tw, r["dw"]), axis_src(th, r["dh"])
    ky, kx = np.minimum((V + 128) >> 8, th - 1), np.minimum((U + 128) >> 8, tw - 1)
    return resample(T_rgb, U, V), resample(T_a, U, V), T_k[ky][:, kx]


def paste(cur: np.ndarray, m: np.ndarray, images, kept, alpha, rec) -> None:
    """One record onto ``cur`` int64 [S][S][3] and ``m`` uint8 [S][S], in place; the box is clipped to the image."""
    S = cur.shape[0]
    dx0, dy0, dw, dh = (int(rec[f]) for f in ("dx0", "dy0", "dw", "dh"))
    ya, yb, xa, xb = max(dy0, 0), min(dy0 + dh, S), max(dx0, 0), min(dx0 + dw, S)
    if ya >= yb or xa >= xb:
        return
    val, a, k = rendered(images, kept, alpha, rec)
    src = (slice(ya - dy0, yb - dy0), slice(xa - dx0, xb - dx0))
    dst = (slice(ya, yb), slice(xa, xb))
    a = a[src][..., None]
    cur[dst] = (a * val[src] + (255 - a) * cur[dst] + 127) // 255
    m[dst] |= k[src]


def compose_ref(images: np.ndarray, masks: np.ndarray, kept: np.ndarray, alpha: np.ndarray, base_index, pastes):
    """Stores uint8 [n_items][S][S](3) -> (rgb uint8 [n][S][S][3], mask uint8 [n][S][S]); ``pastes[k]`` is the record list of sample k."""
    n, S = len(base_index), images.shape[1]
    rgb, msk = np.empty((n, S, S, 3), np.uint8), np.empty((n, S, S), np.uint8)
    for j, (b, recs) in enumerate(zip(base_index, pastes)):
        cur, m = images[b].astype(np.int64), masks[b].copy()
        for rec in recs:
            paste(cur, m, images, kept, alpha, rec)
        assert cur.min() >= 0 and cur.max() <= 255
        rgb[j], msk[j] = cur.astype(np.uint8), m
    return rgb, msk


def rec(donor, sx0, sy0, sw, sh, d4, dx0, dy0, dw, dh) -> dict:
    return dict(zip(REC_FIELDS, (donor, sx0, sy0, sw, sh, d4, dx0, dy0, dw, dh)))


# ------------------------------------------------------------------------------------------------ the bank's host records
def default_min_area(S: int) -> int:
    return max(200, int(0.0008 * S * S))


def meets(a, b) -> bool:
    """Two inclusive boxes (x0, y0, x1, y1) share a pixel."""
    return a[0] <= b[2] and b[0] <= a[2] and a[1] <= b[3] and b[1] <= a[3]


def records_ref(boxes: np.ndarray, counts, content, S: int, max_components: int = 16, margin: int = 4, min_area=None) -> np.ndarray:
    """boxes int32 [n][M][5], counts [n], content [n][4] = (top, left, nh, nw) -> RECORD_DT rows, item then slot ascending."""
    if min_area is None:
        min_area = default_min_area(S)
    M = boxes.shape[1]
    rows = []
    for i in range(boxes.shape[0]):
        top, left, nh, nw = (int(v) for v in content[i])
        used = min(max(int(counts[i]), 0), M)
        grown = []
        for s in range(used):
            x0, y0, x1, y1, _ = (int(v) for v in boxes[i, s])
            grown.append((max(x0 - margin, left), max(y0 - margin, top), min(x1 + margin, left + nw - 1), min(y1 + margin, top + nh - 1)))
        for s in range(used):
            alone = not any(meets(grown[s], grown[o]) for o in range(used) if o != s)
            donor = int(counts[i]) <= max_components and int(boxes[i, s, 4]) >= min_area and alone
            rows.append((i, s) + grown[s] + (int(boxes[i, s, 4]), int(donor)))
    return np.array(rows, RECORD_DT) if rows else np.zeros(0, RECORD_DT)
