"""Restatement in numpy of csrc/tiling.hip (vk_tile_preprocess, vk_tile_blend), operation by operation and in the kernels' order.

`dtype=np.float32` rounds after every operation exactly where the kernels do (contraction is off there), so the pre-processing and the
logit-mode blend agree with the device bit for bit; the prob mode differs by the device's expf.  `dtype=np.float64` is the same chain
in double: the yardstick of the rounding bound (tiling_cases.prob_bound) and, on lattice inputs, equal to the float32 result."""
import numpy as np

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
TTA_VIEWS = {"none": (0,), "hflip": (0, 1), "flips": (0, 1, 2, 3), "d4": (0, 1, 2, 3, 4, 5, 6, 7)}


def axis_origins(length, tile, overlap):
    s = tile - overlap
    n = 1 if length <= tile else -(-(length - tile) // s) + 1
    return [min(i * s, max(length - tile, 0)) for i in range(n)]


def view_index(v, T):
    """(i0, j0) index arrays with A_v = A[i0, j0]."""
    i, j = np.meshgrid(np.arange(T), np.arange(T), indexing="ij")
    a, b = (j, i) if v & 4 else (i, j)
    return (T - 1 - a if v & 2 else a), (T - 1 - b if v & 1 else b)


def inverse_index(v, T):
    """(i, j) index arrays with A = A_v[i, j]: where view v shows tile pixel (ty, tx)."""
    ty, tx = np.meshgrid(np.arange(T), np.arange(T), indexing="ij")
    a = T - 1 - ty if v & 2 else ty
    b = T - 1 - tx if v & 1 else tx
    return (b, a) if v & 4 else (a, b)


def compose(g, v, T=5):
    """u with view_u = (view v of the image transformed by g): pi_u = pi_g o pi_v."""
    gi, gj = view_index(g, T)
    vi, vj = view_index(v, T)
    ci, cj = gi[vi, vj], gj[vi, vj]
    for u in range(8):
        ui, uj = view_index(u, T)
        if (ui == ci).all() and (uj == cj).all():
            return u
    raise AssertionError("D4 is not closed?")


def crops(img, T, overlap, pad_value=0):
    """The padded uint8 tiles [ntiles, T, T, 3] in tile order t = iy * nx + ix."""
    h, w = img.shape[:2]
    out = []
    for y0 in axis_origins(h, T, overlap):
        for x0 in axis_origins(w, T, overlap):
            a = np.full((T, T, 3), pad_value, np.uint8)
            c = img[y0:y0 + T, x0:x0 + T]
            a[:c.shape[0], :c.shape[1]] = c
            out.append(a)
    return np.stack(out)


def normalise(tiles_u8):
    """uint8 BGR [..., T, T, 3] -> float32 RGB planes [..., 3, T, T] with k_letterbox_pre's expression."""
    planes = []
    for k in range(3):
        f = tiles_u8[..., 2 - k].astype(np.float32) / np.float32(255.0)
        planes.append((f - np.float32(MEAN[k])) / np.float32(STD[k]))
    return np.stack(planes, axis=-3)


def preprocess_ref(img, T, overlap, tta, pad_value=0):
    views = TTA_VIEWS[tta]
    out = []
    for a in crops(img, T, overlap, pad_value):
        for v in views:
            i0, j0 = view_index(v, T)
            out.append(normalise(a[i0, j0]))
    return np.stack(out)


def window(T, overlap, dtype):
    R = overlap if overlap > 0 else 1
    t = np.arange(T)
    return np.minimum(np.minimum(t + 1, T - t), R).astype(dtype) / dtype(R)


def sigmoid(x):
    one = x.dtype.type(1)
    with np.errstate(over="ignore"):
        return one / (one + np.exp(-x))


def cover_count(h, w, T, overlap):
    n = np.zeros((h, w), np.int64)
    for y0 in axis_origins(h, T, overlap):
        for x0 in axis_origins(w, T, overlap):
            n[y0:y0 + T, x0:x0 + T] += 1
    return n


def blend_ref(logits, h, w, T, overlap, tta, mode, dtype=np.float32):
    """logits float32 [ntiles*nviews, C, T, T] -> [C, h, w] in `dtype`, in vk_tile_blend's order."""
    views = TTA_VIEWS[tta]
    nv = len(views)
    C = logits.shape[1]
    w1 = window(T, overlap, dtype)
    acc = np.zeros((C, h, w), dtype)
    wsum = np.zeros((h, w), dtype)
    q1 = np.zeros((C, h, w), dtype)
    t = 0
    for y0 in axis_origins(h, T, overlap):
        for x0 in axis_origins(w, T, overlap):
            hh, ww = min(T, h - y0), min(T, w - x0)
            total = None
            for k, v in enumerate(views):
                i, j = inverse_index(v, T)
                lv = logits[t * nv + k][:, i, j].astype(dtype)
                f = sigmoid(lv) if mode == "prob" else lv
                total = f if total is None else total + f
            q = (total * dtype(1.0 / nv))[:, :hh, :ww]
            wt = w1[:hh, None] * w1[None, :ww]
            sl = (slice(None), slice(y0, y0 + hh), slice(x0, x0 + ww))
            acc[sl] = acc[sl] + wt * q
            wsum[sl[1:]] = wsum[sl[1:]] + wt
            q1[sl] = q
            t += 1
    val = np.where(cover_count(h, w, T, overlap) == 1, q1, acc / wsum)
    if mode == "prob":
        val = np.minimum(np.maximum(val, dtype(0)), dtype(1))
    return val


def mask_ref(val, mode, thresh):
    p = sigmoid(val) if mode == "logit" else val
    return np.where(p >= val.dtype.type(thresh), 255, 0).astype(np.uint8)
