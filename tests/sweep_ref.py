"""numpy restatement of vk.sweep (csrc/sweep.hip), operation by operation: the arbiter of tests/test_sweep_cpu.py and
tests/test_vk_sweep_gpu.py.

Histogram: bin(pv) = #{k : pv > thr[k]} (strict; NaN compares false everywhere, so bin 0; +inf bin K), per plane and target value.
Curves: int64 suffix sums; per (k, image, class) k_seg_finalize_multi's fp32 expressions; batch means in float64 in k_seg_finalize's
order (member i of the batch goes to partial i % 64, the 64 partials are added in order, one rounding to fp32); the mean over classes
as the float64 mean of the rounded class scores; the epoch score as the sequential float64 sum over the groups divided by G; the micro
curve, AP and AUC in float64 with k ascending.  Loops run where the order matters and are vectorised only ACROSS independent results."""
import numpy as np

from oracle import prepost_oracle as P

F32, F64, I64 = np.float32, np.float64, np.int64


def default_thresholds():
    return (np.arange(1, 100) / 100).astype(F32)


def bins(pv, thr):
    """#{k : pv > thr[k]} for every element.  searchsorted(side="left") counts thr[k] < pv, and sends NaN to K: NaN goes to 0 by hand."""
    pv = np.asarray(pv, dtype=F32)
    b = np.searchsorted(np.asarray(thr, dtype=F32), pv, side="left").astype(np.int64)
    b[np.isnan(pv)] = 0
    return b


def prediction_value(x, from_logits):
    x = np.asarray(x, dtype=F32)
    return P.sigmoid_f32(x) if from_logits else x


def validity(target, ignore_index=None):
    """(valid, positive, bad count): 1 positive, 0 negative, ignore_index skipped silently, anything else skipped and counted."""
    t = np.asarray(target)
    tf = t.astype(F32)
    ign = (tf == F32(ignore_index)) if ignore_index is not None else np.zeros(t.shape, bool)
    pos = (tf == 1) & ~ign
    valid = (pos | (tf == 0)) & ~ign
    return valid, pos, int((~valid & ~ign).sum())


def hist_ref(pred, target, thr, from_logits=False, ignore_index=None):
    """pred, target [N, C, ...] -> (hist int32 [N, C, 2, K + 1], bad)."""
    thr = np.asarray(thr, dtype=F32)
    K = thr.size
    x = np.asarray(pred, dtype=F32)
    N, C = x.shape[:2]
    pv = prediction_value(x.reshape(N, C, -1), from_logits)
    valid, pos, bad = validity(np.asarray(target).reshape(N, C, -1), ignore_index)
    b = bins(pv, thr)
    hist = np.zeros((N, C, 2, K + 1), np.int64)
    for n in range(N):
        for c in range(C):
            for t in (0, 1):
                sel = valid[n, c] & (pos[n, c] == bool(t))
                hist[n, c, t] = np.bincount(b[n, c][sel], minlength=K + 1)
    return hist.astype(np.int32), bad


def direct_counts(pred, target, thr_k, from_logits=False, ignore_index=None):
    """(I, P, T, valid) int64 [N, C] at ONE threshold, evaluated directly: pred = (pv > thr_k) & valid."""
    x = np.asarray(pred, dtype=F32)
    N, C = x.shape[:2]
    pv = prediction_value(x.reshape(N, C, -1), from_logits)
    valid, pos, _ = validity(np.asarray(target).reshape(N, C, -1), ignore_index)
    hit = (pv > F32(thr_k)) & valid
    return ((hit & pos).sum(-1).astype(I64), hit.sum(-1).astype(I64), (pos & valid).sum(-1).astype(I64), valid.sum(-1).astype(I64))


def suffix_counts(hist):
    """hist [N, C, 2, K + 1] -> (I, P) int64 [K, N, C] (sums over the bins above k), T and valid int64 [N, C]."""
    h = np.asarray(hist).astype(I64)
    K = h.shape[-1] - 1
    both = h[:, :, 0] + h[:, :, 1]
    # reversed cumulative sums: entry b = sum over bins >= b; the bins above k start at k + 1
    sa = np.cumsum(both[..., ::-1], axis=-1)[..., ::-1]
    si = np.cumsum(h[:, :, 1][..., ::-1], axis=-1)[..., ::-1]
    Pk = np.moveaxis(sa[..., 1:K + 1], -1, 0)
    Ik = np.moveaxis(si[..., 1:K + 1], -1, 0)
    return Ik, Pk, si[..., 0], sa[..., 0]


def scores(tp, fp, fn, eps):
    """k_seg_finalize_multi's per-image expressions, fp32, in its order."""
    eps = F32(eps)
    I = tp.astype(F32)
    card = (tp + fp).astype(F32) + (tp + fn).astype(F32)
    dice = (F32(2) * I + eps) / (card + eps)
    iou = (I + eps) / ((card - I) + eps)
    return dice.astype(F32), iou.astype(F32)


def mean64(vals, members):
    """k_seg_finalize's mean over `members` (image indices, in order) of fp32 `vals` [..., N, ...] along axis 1 of [K, N, C]: member m
    goes to float64 partial m % 64, the partials are added in order, the quotient is rounded once.  Vectorised over (k, c) only."""
    K, _, C = vals.shape
    acc = np.zeros((64, K, C), F64)
    for m, i in enumerate(members):
        acc[m % 64] += vals[:, i, :].astype(F64)
    s = np.zeros((K, C), F64)
    for j in range(64):
        s = s + acc[j]
    with np.errstate(invalid="ignore", divide="ignore"):
        return (s / F64(len(members))).astype(F32)


def class_mean(cls_scores):
    """fp32 [K, C] -> fp32 [K]: the float64 mean of the rounded class scores, summed in class order, rounded once."""
    K, C = cls_scores.shape
    s = np.zeros(K, F64)
    for c in range(C):
        s = s + cls_scores[:, c].astype(F64)
    return (s / F64(C)).astype(F32)


def ratio(num, den, empty):
    with np.errstate(invalid="ignore", divide="ignore"):
        r = num.astype(F64) / den.astype(F64)
    return np.where(den == 0, F64(empty), r)


def first_best(v):
    """Lowest index of the maximum along axis 0 under a strict comparison, as the device loop."""
    best = np.zeros(v.shape[1:], np.int64)
    cur = v[0].copy()
    for k in range(1, v.shape[0]):
        better = v[k] > cur
        best = np.where(better, k, best)
        cur = np.where(better, v[k], cur)
    return best.astype(np.int32)


def curves_ref(hist, groups=None, n_groups=0, eps=1e-7):
    """Every output of vk_sweep_curves, by name, with the device's shapes and dtypes."""
    hist = np.asarray(hist)
    N, C = hist.shape[:2]
    K = hist.shape[-1] - 1
    Ik, Pk, T, valid = suffix_counts(hist)
    tp, fp, fn = Ik, Pk - Ik, T[None] - Ik
    tn = valid[None] - tp - fp - fn
    out = {"stats": np.stack([tp, fp, fn, tn], axis=1).astype(I64)}                       # [K, 4, N, C]
    dice, iou = scores(tp, fp, fn, eps)
    out["per_image"] = np.stack([dice, iou], axis=-1)                                     # [K, N, C, 2]
    out["dice"], out["iou"] = mean64(dice, range(N)), mean64(iou, range(N))
    out["mean_dice"], out["mean_iou"] = class_mean(out["dice"]), class_mean(out["iou"])
    ms = out["stats"].sum(axis=2).transpose(1, 0, 2)                                      # [4, K, C], integers: any order
    out["micro_stats"] = ms
    mtp, mfp, mfn, mtn = ms
    out["precision"] = ratio(mtp, mtp + mfp, 1.0)
    out["recall"] = ratio(mtp, mtp + mfn, 1.0)
    out["f1"] = ratio(2 * mtp, 2 * mtp + mfp + mfn, 1.0)
    out["micro_iou"] = ratio(mtp, mtp + mfp + mfn, 1.0)
    out["fpr"] = ratio(mfp, mfp + mtn, 0.0)
    ap, auc = np.zeros(C, F64), np.zeros(C, F64)
    xp, yp = np.ones(C, F64), np.ones(C, F64)
    for k in range(K):
        rn = out["recall"][k + 1] if k + 1 < K else np.zeros(C, F64)
        ap = ap + (out["recall"][k] - rn) * out["precision"][k]
        auc = auc + ((xp - out["fpr"][k]) * (yp + out["recall"][k])) * F64(0.5)
        xp, yp = out["fpr"][k], out["recall"][k]
    auc = auc + ((xp - F64(0.0)) * (yp + F64(0.0))) * F64(0.5)
    out["ap"], out["auc"] = ap, auc
    out["best_dice"], out["best_iou"], out["best_f1"] = first_best(out["dice"]), first_best(out["iou"]), first_best(out["f1"])
    out["best_mean"] = np.array([first_best(out["mean_dice"]), first_best(out["mean_iou"])], np.int32)
    if groups is not None:
        G = int(n_groups)
        groups = np.asarray(groups)
        gd, gu = np.zeros((G, K, C), F32), np.zeros((G, K, C), F32)
        gmd, gmu = np.zeros((G, K), F32), np.zeros((G, K), F32)
        for g in range(G):
            members = [i for i in range(N) if groups[i] == g]          # ascending image index, numbered from 0
            gd[g], gu[g] = mean64(dice, members), mean64(iou, members)
            gmd[g], gmu[g] = class_mean(gd[g]), class_mean(gu[g])
        out.update(group_dice=gd, group_iou=gu, group_mean_dice=gmd, group_mean_iou=gmu)
        for name, src in (("epoch_dice", gd), ("epoch_iou", gu), ("epoch_mean_dice", gmd), ("epoch_mean_iou", gmu)):
            s = np.zeros(src.shape[1:], F64)
            for g in range(G):                                         # sequential: np.mean sums pairwise
                s = s + src[g].astype(F64)
            out[name] = s / F64(G)
    return out


def sweep_ref(pred, target, thr, from_logits=False, ignore_index=None, groups=None, n_groups=0, eps=1e-7):
    hist, bad = hist_ref(pred, target, thr, from_logits, ignore_index)
    return curves_ref(hist, groups, n_groups, eps), hist, bad
