"""Float64 reference of vk.lovasz (numpy): the fp32 sort key exactly as the device forms it, a stable order by (key descending, flat
index ascending), the Jaccard increments in closed form from an integer prefix count, and the analytic gradient.  Also the MCC term."""
import numpy as np


def key_u32(e32):
    """fp32 errors -> uint32 keys whose ascending order is error descending (bit patterns in radix order); 0xFFFFFFFF is reserved"""
    b = np.ascontiguousarray(e32, dtype=np.float32).view(np.uint32)
    asc = np.where(b >> 31 != 0, ~b, b | np.uint32(0x80000000))
    return np.minimum(~asc, np.uint32(0xFFFFFFFE))


def order_fp32(e32, valid):
    """indices of the valid entries in sorted order (error descending, index ascending among equal keys)"""
    k = key_u32(e32).astype(np.uint64)
    k[~valid] = 0xFFFFFFFF
    perm = np.argsort(k, kind="stable")
    return perm[: int(valid.sum())]


def order_f64(e, valid):
    perm = np.argsort(np.where(valid, -e, np.inf), kind="stable")
    return perm[: int(valid.sum())]


def dj_closed(g):
    """Jaccard increments of a sorted 0/1 vector (integer prefix count, float64 division)"""
    g = np.asarray(g).astype(np.int64)
    n = g.size
    if n == 0:
        return np.zeros(0)
    G = int(g.sum())
    if G == 0:
        out = np.zeros(n)
        out[0] = 1.0
        return out
    c = np.cumsum(g)
    k1 = np.arange(1, n + 1, dtype=np.int64)
    U = (G + k1 - c).astype(np.float64)
    I = (G - c).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        bg = I / (U * (U - 1.0))
    return np.where(g == 1, 1.0 / U, bg)


def dj_cumsum(g):
    """smp's lovasz_grad: two float cumsums, then differences"""
    g = np.asarray(g, dtype=np.float64)
    if g.size == 0:
        return np.zeros(0)
    gts = g.sum()
    inter = gts - np.cumsum(g)
    union = gts + np.cumsum(1.0 - g)
    jac = 1.0 - inter / union
    jac[1:] = jac[1:] - jac[:-1]
    return jac


def flat(errors, flag):
    """vk_lovasz_flat: errors fp32 [S, L], flag uint8 [S, L] -> (loss [S] f64, derr [S, L] f64, rank [S, L] uint32)"""
    errors = np.asarray(errors, dtype=np.float32)
    S, L = errors.shape
    loss = np.zeros(S)
    derr = np.zeros((S, L))
    rank = np.full((S, L), 0xFFFFFFFF, dtype=np.uint32)
    for s in range(S):
        valid = flag[s] < 2
        perm = order_fp32(errors[s], valid)
        d = dj_closed(flag[s][perm] == 1)
        e = errors[s][perm].astype(np.float64)
        loss[s] = float((np.maximum(e, 0.0) * d).sum())
        derr[s][perm] = np.where(e > 0, d, 0.0)
        rank[s][perm] = np.arange(perm.size, dtype=np.uint32)
    return loss, derr, rank


def hinge(x, y, per_image=False, ignore_index=None):
    """x fp32 [N, C, H, W], y broadcastable 0/1 (or ignore_index) -> (value f64, dlogits f64 in x's shape)"""
    x = np.asarray(x, dtype=np.float32)
    y = np.broadcast_to(np.asarray(y, dtype=np.float32), x.shape)
    N = x.shape[0]
    S = N if per_image else 1
    xs, ys = x.reshape(S, -1), y.reshape(S, -1)
    grad = np.zeros(xs.shape)
    total = 0.0
    for s in range(S):
        valid = (ys[s] != np.float32(ignore_index)) if ignore_index is not None else np.ones(ys[s].shape, bool)
        sgn = (2.0 * ys[s] - 1.0).astype(np.float32)
        e32 = (np.float32(1.0) - xs[s] * sgn).astype(np.float32)
        perm = order_fp32(e32, valid)
        if perm.size == 0:
            continue
        d = dj_closed(ys[s][perm] == 1)
        e = e32[perm].astype(np.float64)
        total += float((np.maximum(e, 0.0) * d).sum())
        grad[s][perm] = np.where(e > 0, -sgn[perm].astype(np.float64) * d, 0.0)
    return total / S, (grad / S).reshape(x.shape)


def softmax_probs(x):
    x = np.asarray(x, dtype=np.float64)
    z = x - x.max(axis=1, keepdims=True)
    ez = np.exp(z)
    return ez / ez.sum(axis=1, keepdims=True)


def softmax(x, t, per_image=False, ignore_index=None, fp32_probs=False, probs=None):
    """x fp32 [N, C, H, W], t int64 [N, H, W] -> (value, dlogits f64, per-segment present class lists).  fp32_probs: the errors are
    formed and ordered from the probabilities rounded to fp32 (what a device can hold) instead of the float64 ones.  probs: float64 probabilities to use instead of computing them."""
    x = np.asarray(x)
    N, C = x.shape[:2]
    p = (softmax_probs(x) if probs is None else np.asarray(probs, dtype=np.float64)).reshape(N, C, -1)
    HW = p.shape[2]
    t = np.asarray(t).reshape(N, HW)
    S = N if per_image else 1
    valid_all = (t >= 0) & (t < C)
    if ignore_index is not None:
        valid_all &= t != ignore_index
    Gm = np.zeros((N, C, HW))
    total = 0.0
    present_all = []
    for s in range(S):
        imgs = [s] if per_image else list(range(N))
        tt = t[imgs].reshape(-1)
        valid = valid_all[imgs].reshape(-1)
        present = [c for c in range(C) if np.any((tt == c) & valid)]
        present_all.append(present)
        if not present:
            continue
        seg = 0.0
        for c in present:
            pc = p[imgs, c].reshape(-1)
            fg = ((tt == c) & valid)
            if fp32_probs:
                e32 = np.abs(fg.astype(np.float32) - pc.astype(np.float32)).astype(np.float32)
                perm = order_fp32(e32, valid)
                e = e32.astype(np.float64)
            else:
                e = np.abs(fg.astype(np.float64) - pc)
                perm = order_f64(e, valid)
            d = dj_closed(fg[perm])
            seg += float((e[perm] * d).sum())
            g = np.zeros(tt.size)
            g[perm] = np.where(e[perm] > 0, np.where(fg[perm], -1.0, 1.0) * d, 0.0) / len(present)
            Gm[imgs, c] = g.reshape(len(imgs), HW)
        total += seg / len(present)
    dot = (Gm * p).sum(axis=1, keepdims=True)
    grad = p * (Gm - dot) / S
    grad = grad * valid_all[:, None, :]
    return total / S, grad.reshape(x.shape), present_all


def mcc(x, y, eps=1e-5, ignore_index=None):
    """x [N, 1, H, W] logits, y 0/1 (or ignore_index) -> (value, dlogits), float64"""
    x = np.asarray(x, dtype=np.float64)
    y = np.broadcast_to(np.asarray(y, dtype=np.float64), x.shape)
    m = (y != ignore_index).astype(np.float64) if ignore_index is not None else np.ones_like(x)
    if m.sum() == 0:
        return 0.0, np.zeros_like(x)
    yy = y * m
    p = 1.0 / (1.0 + np.exp(-x))
    I, P, T, M = (p * yy).sum(), (p * m).sum(), yy.sum(), m.sum()
    tp, fp, fn, tn = I + eps, P - I + eps, T - I + eps, M - P - T + I + eps
    A, B, Cn, D = tp + fp, tp + fn, tn + fp, tn + fn
    num, den = tp * tn - fp * fn, np.sqrt(A * B * Cn * D)
    a = -(M + 4 * eps) / den
    b = B / den + 0.5 * (num / den) * (1.0 / A - 1.0 / D)
    return 1.0 - num / den, m * (a * yy + b) * p * (1.0 - p)
