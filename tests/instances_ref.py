"""Restatement of vk.instances (csrc/instances.hip, vk_geom_slot_map) on the host, for bit-for-bit comparison.  No GPU is needed.

The slot map is built from the oracle's stages (binarize, open_close, label8), the area filter and the raster rank among the kept
components; the table with np.add.at; every float sum is an explicit Python loop over float64 scalars in ascending pred slot, then
ascending image (numpy's pairwise `sum` is not that order).  Python floats are IEEE float64 and `/`, `*`, `+`, `-`, `abs` round once,
so these are the device's operations."""
from __future__ import annotations

import numpy as np

import geom_cases as GC

INT_FIELDS = ("tp", "fp", "fn", "n_rel", "n_pred_used", "n_gt_used", "n_split", "n_merge", "overflow_pred", "overflow_gt", "n_images")
FLOAT_FIELDS = ("sum_iou", "sum_abs_d", "sum_rel_d", "sum_signed_rel_d", "sum_hv_rel", "max_abs_d")
STATS_DT = np.dtype([(f, "<i8") for f in INT_FIELDS] + [(f, "<f8") for f in FLOAT_FIELDS])
DEFAULT_THR = np.arange(0.5, 1.0, 0.05)


# ------------------------------------------------------------------------------------------------ slot map
def slot_map_from_labels(labels: np.ndarray, areas: np.ndarray, min_area: int, cap: int):
    """(slots int32 [h][w], count): label ids are in raster order of the first pixel, so the rank among kept labels is the slot."""
    n = len(areas) - 1
    keep = areas >= min_area
    keep[0] = False
    rank = np.cumsum(keep) - 1                       # rank of a kept label among the kept ones
    lut = np.full(n + 1, -1, np.int32)
    for i in range(1, n + 1):
        if keep[i]:
            lut[i] = rank[i] if rank[i] < cap else -2
    return lut[labels].astype(np.int32), int(keep.sum())


def slot_map_ref(prob: np.ndarray, cfg: GC.Cfg):
    _, labels, areas = GC.front(prob, cfg)
    return slot_map_from_labels(labels, areas, cfg.min_area, cfg.cap)


# ------------------------------------------------------------------------------------------------ contingency
def index_of(slots: np.ndarray, M: int) -> np.ndarray:
    s = slots.astype(np.int64)
    return np.where((s >= 0) & (s < M), s + 1, 0)


def contingency_ref(pred_slots: np.ndarray, gt_slots: np.ndarray, Mp: int, Mg: int) -> np.ndarray:
    """[B][h][w] x 2 -> int32 [B][Mp + 1][Mg + 1]."""
    B = pred_slots.shape[0]
    table = np.zeros((B, Mp + 1, Mg + 1), np.int32)
    for b in range(B):
        np.add.at(table[b], (index_of(pred_slots[b], Mp).ravel(), index_of(gt_slots[b], Mg).ravel()), 1)
    return table


def contingency_brute(pred_slots: np.ndarray, gt_slots: np.ndarray, Mp: int, Mg: int) -> np.ndarray:
    """One map, by pixel sets."""
    h, w = pred_slots.shape
    sets_p = [set() for _ in range(Mp + 1)]
    sets_g = [set() for _ in range(Mg + 1)]
    for y in range(h):
        for x in range(w):
            p, g = int(pred_slots[y, x]), int(gt_slots[y, x])
            sets_p[p + 1 if 0 <= p < Mp else 0].add((y, x))
            sets_g[g + 1 if 0 <= g < Mg else 0].add((y, x))
    return np.array([[len(a & c) for c in sets_g] for a in sets_p], np.int32)


# ------------------------------------------------------------------------------------------------ matching
def candidates(table: np.ndarray, npu: int, ngu: int):
    """One table -> [(pred slot, GT slot)] with 3 I > Ap + Ag in Python integers, every qualifying pair listed (uniqueness is proved by
    the CPU tests, not assumed)."""
    Ap = [int(v) for v in table.astype(np.int64).sum(axis=1)]
    Ag = [int(v) for v in table.astype(np.int64).sum(axis=0)]
    out = []
    for i in range(1, npu + 1):
        for j in range(1, ngu + 1):
            if 3 * int(table[i, j]) > Ap[i] + Ag[j]:
                out.append((i - 1, j - 1))
    return out, Ap, Ag


def match_ref(table: np.ndarray, n_pred, n_gt, thr, dp=None, dg=None):
    """table [B][Mp + 1][Mg + 1], counts [B], thr [K] float64, dp [B][Mp] / dg [B][Mg] float64 or None.
    -> dict(pair_gt [B][Mp], pair_iou, pair_derr, per_image STATS_DT [B][K])."""
    B, Mp, Mg = table.shape[0], table.shape[1] - 1, table.shape[2] - 1
    thr = [float(t) for t in np.asarray(thr, np.float64)]
    K = len(thr)
    has_d = dp is not None and dg is not None
    pair_gt = np.full((B, Mp), -1, np.int32)
    pair_iou = np.zeros((B, Mp), np.float64)
    pair_derr = np.zeros((B, Mp), np.float64)
    per = np.zeros((B, K), STATS_DT)
    for b in range(B):
        cp, cg = int(n_pred[b]), int(n_gt[b])
        npu, ngu = min(max(cp, 0), Mp), min(max(cg, 0), Mg)
        cand, Ap, Ag = candidates(table[b], npu, ngu)
        dps, dgs = {}, {}
        for s, t in cand:
            I = int(table[b, s + 1, t + 1])
            U = Ap[s + 1] + Ag[t + 1] - I
            pair_gt[b, s] = max(int(pair_gt[b, s]), t)
            pair_iou[b, s] = float(I) / float(U)
            if has_d:
                dps[s], dgs[s] = float(dp[b, s]), float(dg[b, t])
                pair_derr[b, s] = dps[s] - dgs[s]
        touch = table[b, 1:npu + 1, 1:ngu + 1] > 0
        n_split = int((touch.sum(axis=0) >= 2).sum())
        n_merge = int((touch.sum(axis=1) >= 2).sum())
        for k in range(K):
            tp = n_rel = 0
            s_iou = s_abs = s_rel = s_srel = s_hv = mx = 0.0
            for s in range(npu):
                if pair_gt[b, s] < 0 or not (float(pair_iou[b, s]) > thr[k]):
                    continue
                tp += 1
                s_iou = s_iou + float(pair_iou[b, s])
                if has_d:
                    e = dps[s] - dgs[s]
                    a = abs(e)
                    s_abs = s_abs + a
                    if a > mx:
                        mx = a
                    if dgs[s] > 0.0 and dps[s] > 0.0:
                        n_rel += 1
                        s_rel = s_rel + a / dgs[s]
                        s_srel = s_srel + e / dgs[s]
                        r = dgs[s] / dps[s]
                        s_hv = s_hv + (r * r - 1.0)
            per[b, k] = (tp, npu - tp, ngu - tp, n_rel, npu, ngu, n_split, n_merge, int(cp > Mp), int(cg > Mg), 1,
                         s_iou, s_abs, s_rel, s_srel, s_hv, mx)
    return dict(pair_gt=pair_gt, pair_iou=pair_iou, pair_derr=pair_derr, per_image=per)


def totals_ref(per_image: np.ndarray, start=None) -> np.ndarray:
    """per_image [B][K] -> [K]: image after image, every float sum sequential."""
    B, K = per_image.shape
    tot = np.zeros(K, STATS_DT) if start is None else start.copy()
    for k in range(K):
        ints = {f: int(tot[k][f]) for f in INT_FIELDS}
        flts = {f: float(tot[k][f]) for f in FLOAT_FIELDS}
        for b in range(B):
            r = per_image[b, k]
            for f in INT_FIELDS:
                ints[f] += int(r[f])
            for f in FLOAT_FIELDS[:-1]:
                flts[f] = flts[f] + float(r[f])
            if float(r["max_abs_d"]) > flts["max_abs_d"]:
                flts["max_abs_d"] = float(r["max_abs_d"])
        for f in INT_FIELDS:
            tot[k][f] = ints[f]
        for f in FLOAT_FIELDS:
            tot[k][f] = flts[f]
    return tot


def _div(num: float, den: float, empty: float) -> float:
    return empty if den == 0 else num / den


def summarize_ref(totals: np.ndarray, thr=None) -> dict:
    """The dictionary of ObjectMetrics.compute(), scalar by scalar."""
    K = len(totals)
    names = ("precision", "recall", "f1", "rq", "sq", "pq", "mean_abs_d", "mean_rel_d", "mean_signed_rel_d", "mean_hv_rel", "max_abs_d")
    out = {n: np.zeros(K, np.float64) for n in names}
    for k in range(K):
        t = totals[k]
        tp, fp, fn, n_rel = float(t["tp"]), float(t["fp"]), float(t["fn"]), float(t["n_rel"])
        out["precision"][k] = _div(tp, tp + fp, 1.0)
        out["recall"][k] = _div(tp, tp + fn, 1.0)
        out["f1"][k] = out["rq"][k] = _div(2.0 * tp, 2.0 * tp + fp + fn, 1.0)
        out["sq"][k] = _div(float(t["sum_iou"]), tp, float("nan"))
        out["pq"][k] = _div(float(t["sum_iou"]), tp + 0.5 * fp + 0.5 * fn, 1.0)
        out["mean_abs_d"][k] = _div(float(t["sum_abs_d"]), tp, float("nan"))
        out["mean_rel_d"][k] = _div(float(t["sum_rel_d"]), n_rel, float("nan"))
        out["mean_signed_rel_d"][k] = _div(float(t["sum_signed_rel_d"]), n_rel, float("nan"))
        out["mean_hv_rel"][k] = _div(float(t["sum_hv_rel"]), n_rel, float("nan"))
        out["max_abs_d"][k] = float(t["max_abs_d"])
    for f in ("tp", "fp", "fn", "n_rel", "n_split", "n_merge", "overflow_pred", "overflow_gt", "n_images"):
        out[f] = totals[f].astype(np.int64)
    out["n_pred"], out["n_gt"] = totals["n_pred_used"].astype(np.int64), totals["n_gt_used"].astype(np.int64)
    if thr is not None:
        out["iou_thresholds"] = np.asarray(thr, np.float64).copy()
    return out


# ------------------------------------------------------------------------------------------------ end to end
def detect_ref(probs: np.ndarray, cfg: GC.Cfg, fit: str):
    """[B][h][w] -> (slots int32 [B][h][w], counts [B], d_mean float64 [B][cap] (0 above the list), records per map)."""
    B = probs.shape[0]
    slots = np.zeros(probs.shape, np.int32)
    counts = np.zeros(B, np.int64)
    d = np.zeros((B, cfg.cap), np.float64)
    recs = []
    for b in range(B):
        ref = GC.MapRef(probs[b], cfg)
        slots[b], counts[b] = slot_map_from_labels(ref.labels, ref.areas, cfg.min_area, cfg.cap)
        _, _, r = ref.expected(fit, cfg)
        d[b, :len(r)] = r["d_mean"]
        recs.append(r)
    return slots, counts, d, recs


def object_metrics_ref(probs: np.ndarray, targets: np.ndarray, pred_cfg: GC.Cfg, fit: str = "rect", thr=DEFAULT_THR, start=None):
    """-> (dictionary of compute(), totals, per_image, table).  The target goes through the ground-truth preset (threshold 0.5, no
    morphology, min_area 1) with the prediction's capacity and fit."""
    gt_cfg = GC.Cfg(thresh=0.5, k=1, oi=0, ci=0, min_area=1, cap=pred_cfg.cap, outset=pred_cfg.outset)
    ps, pc, pd, _ = detect_ref(probs, pred_cfg, fit)
    gs, gc, gd, _ = detect_ref(targets.astype(np.float32), gt_cfg, fit)
    table = contingency_ref(ps, gs, pred_cfg.cap, gt_cfg.cap)
    m = match_ref(table, pc, gc, thr, pd, gd)
    tot = totals_ref(m["per_image"], start)
    return summarize_ref(tot, thr), tot, m["per_image"], table
