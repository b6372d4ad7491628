"""numpy restatement of vk.multiclass's validation metrics and inference post-processing, the arbiter of
tests/test_multiclass_eval_{cpu,gpu}.py.

Metrics: the reference's dice_coef / iou_coef (train.py:230-281) per class.  Counts per (image, class) are exact integers; scores are
fp32 with the reference's operation order, batch means in float64 in k_seg_finalize's order (image i goes to partial i % 64, the 64
partials are added in order) and rounded once.  Post-processing: oracle.prepost_oracle's single-plane formulas applied per class
plane, softmax as shift-by-max, expf, class-order sum, divide."""
import numpy as np

from oracle import prepost_oracle as P

F32 = np.float32


def counts(logits, target, mode, threshold=0.5, from_logits=True):
    """logits [N, C, ...]; target [N, C, ...] (multilabel) or int [N, ...] (multiclass).
    Returns (tp, fp, fn, tn) int64 [N, C] and the number of bad labels."""
    x = np.asarray(logits, dtype=F32)
    N, C = x.shape[:2]
    x = x.reshape(N, C, -1)
    if mode == "multilabel":
        t = np.asarray(target, dtype=F32).reshape(N, C, -1)
        p = P.sigmoid_f32(x) if from_logits else x
        pred = p > F32(threshold)
        valid = (t == 0) | (t == 1)
        tgt = (t == 1) & valid
        pred = pred & valid
        bad = int((~valid).sum())
    elif mode == "multiclass":
        t = np.asarray(target, dtype=np.int64).reshape(N, -1)
        valid = (t >= 0) & (t < C)
        arg = np.argmax(x, axis=1)                     # first maximum: ties to the lowest index
        cls = np.arange(C).reshape(1, C, 1)
        pred = (arg[:, None, :] == cls) & valid[:, None, :]
        tgt = (t[:, None, :] == cls) & valid[:, None, :]
        valid = np.broadcast_to(valid[:, None, :], pred.shape)
        bad = int((~valid[:, 0]).sum())
    else:
        raise ValueError(mode)
    tp = (pred & tgt).sum(-1).astype(np.int64)
    fp = pred.sum(-1).astype(np.int64) - tp
    fn = tgt.sum(-1).astype(np.int64) - tp
    tn = valid.sum(-1).astype(np.int64) - tp - fp - fn
    return (tp, fp, fn, tn), bad


def _mean_f64(vals_f32):
    """k_seg_finalize's batch mean of fp32 values: 64 fp64 partials (value i into partial i % 64, in order), added in order, / n."""
    n = len(vals_f32)
    acc = [0.0] * 64
    for i, v in enumerate(vals_f32):
        acc[i % 64] += float(v)
    s = 0.0
    for a in acc:
        s += a
    return F32(s / n)


def scores(tp, fp, fn, eps=1e-7):
    """(out, per_image) with out = [mean dice, mean iou, dice_c[C], iou_c[C], per_image [N][C][2]] as the device returns it."""
    eps = F32(eps)
    I = tp.astype(F32)
    card = (tp + fp).astype(F32) + (tp + fn).astype(F32)
    dice = (F32(2) * I + eps) / (card + eps)
    iou = (I + eps) / ((card - I) + eps)
    N, C = tp.shape
    dc = np.array([_mean_f64(dice[:, c]) for c in range(C)], dtype=F32)
    uc = np.array([_mean_f64(iou[:, c]) for c in range(C)], dtype=F32)
    md = F32(sum(float(v) for v in dc) / C)
    mu = F32(sum(float(v) for v in uc) / C)
    per = np.stack([dice, iou], axis=-1).astype(F32)
    return np.concatenate([[md, mu], dc, uc, per.reshape(-1)]).astype(F32)


def softmax_f32(planes):
    """[C, H, W] fp32 -> softmax over the classes: shift by the max, exp, sum in class order, divide (all fp32)."""
    x = np.asarray(planes, dtype=F32)
    m = x.max(axis=0)
    e = np.exp((x - m).astype(F32), dtype=F32)
    s = np.zeros_like(m)
    for c in range(x.shape[0]):
        s = (s + e[c]).astype(F32)
    return (e / s).astype(F32)


def postprocess_labels(logits_csq, nh, nw, top, left, orig_hw):
    lab = np.argmax(np.asarray(logits_csq, dtype=F32), axis=0).astype(np.uint8)
    return P.resize_nearest(np.ascontiguousarray(lab[top:top + nh, left:left + nw]), orig_hw[1], orig_hw[0])


def postprocess_masks(logits_csq, nh, nw, top, left, orig_hw, thresh=0.5):
    return np.stack([P.postprocess_mask(lg, nh, nw, top, left, orig_hw, thresh) for lg in np.asarray(logits_csq, dtype=F32)])


def postprocess_probs(logits_csq, nh, nw, top, left, orig_hw, mode):
    x = np.asarray(logits_csq, dtype=F32)
    prob = P.sigmoid_f32(x) if mode == "multilabel" else softmax_f32(x)
    out = []
    for pc in prob:
        crop = np.ascontiguousarray(pc[top:top + nh, left:left + nw])
        if crop.shape != tuple(orig_hw):
            crop = P.resize_linear_f32(crop, orig_hw[1], orig_hw[0])
        out.append(np.clip(crop, 0.0, 1.0).astype(F32))
    return np.stack(out)
