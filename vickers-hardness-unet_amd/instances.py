"""Object-level validation: how many indentations were found, and how far off are their diagonals (csrc/instances.hip,
``vk_geom_slot_map`` / ``vk_inst_contingency`` / ``vk_inst_match``).

The value this project measures is the pair of diagonals of each indentation, and hardness goes as 1 / d^2: a 1 % error of the mean
diagonal is a 2 % error of HV.  Pixel Dice averages that away (a map with Dice 0.97 can miss a small indentation, report two
touching ones as one, or put every diagonal 3 % long), so this module is the object-level companion of ``vk.seg_metrics`` and
``vk.sweep``::

    om = vk.ObjectMetrics(fit="rect")
    for x, y in loader:
        om.update(torch.sigmoid(model(x))[:, 0], y[:, 0])     # no host synchronisation
    m = om.compute()                                          # one read-back
    m["pq"][0], m["mean_rel_d"][0], m["mean_hv_rel"][0]       # at IoU > 0.5

``detect`` (``vk.geometry.detect``, the same object) runs the geometry post-processing and keeps everything on the device, with the
label map as slots of the detection list; ``contingency`` counts the pixels of every (pred slot, GT slot) pair of two such results
in one pass; ``match`` pairs the objects (IoU > 1/2, which makes the pairing unique) and sums the statistics of the matched pairs at
every IoU threshold.
Integer counts and IEEE float64 in a fixed order: an epoch's totals do not depend on how it was cut into batches.  One foreground
class per call, at most 256 objects per map and side.  CUDA tensors only: there is no CPU fallback."""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from . import _lib as L
from . import geometry as G
from ._lib import VkError
from .geometry import Detections, detect

__all__ = ["DEFAULT_IOU_THRESHOLDS", "GT_PRESET", "STATS_DTYPE", "Detections", "MatchResult", "ObjectMetrics", "detect", "detect_gt",
           "contingency", "match", "object_metrics", "summarize"]

MAX_SLOTS = 256
MAX_THRESHOLDS = 16
DEFAULT_IOU_THRESHOLDS = np.arange(0.5, 1.0, 0.05)             # float64: 0.5, 0.55, ... 0.95
DEFAULT_IOU_THRESHOLDS.setflags(write=False)
GT_PRESET = dict(bin_thresh=0.5, min_area=1, morph_kernel=1)    # a 0/1 mask as it is: no morphology, every component kept
STATS_DTYPE = np.dtype(L.vk_inst_stats)


def _iou_thresholds(thresholds) -> np.ndarray:
    if thresholds is None:
        return DEFAULT_IOU_THRESHOLDS
    if isinstance(thresholds, torch.Tensor):
        thresholds = thresholds.detach().cpu().numpy()
    thr = np.ascontiguousarray(np.asarray(thresholds, dtype=np.float64))
    if thr.ndim != 1 or not 1 <= thr.size <= MAX_THRESHOLDS:
        raise ValueError("expected 1 to %d IoU thresholds in one dimension, got shape %s" % (MAX_THRESHOLDS, thr.shape))
    if not np.isfinite(thr).all():
        raise ValueError("IoU thresholds must be finite")
    if not (thr[1:] > thr[:-1]).all():
        raise ValueError("IoU thresholds must be strictly ascending")
    if not ((thr >= 0.5) & (thr < 1.0)).all():
        raise ValueError("IoU thresholds must be in [0.5, 1): below 0.5 a pairing is not unique")
    return thr


def detect_gt(mask: torch.Tensor, fit: str = "rect", fit_outset_px: int = G.FIT_OUTSET_PX, max_components: int = 64) -> Detections:
    """``detect`` with the ground-truth preset: a 0/1 mask [B, h, w] (any dtype) is taken as it is."""
    if isinstance(mask, torch.Tensor) and not mask.is_cuda:
        raise VkError("masks are on %s: this package runs on an MI355X only and has no CPU fallback" % mask.device)
    return detect(mask.float(), fit=fit, fit_outset_px=fit_outset_px, max_components=max_components, **GT_PRESET)


def _pair(pred: Detections, gt: Detections):
    if not isinstance(pred, Detections) or not isinstance(gt, Detections):
        raise ValueError("expected two Detections (vk.instances.detect)")
    if pred.slots is None or gt.slots is None:
        raise ValueError("matching needs the slot maps: these Detections were made with detect(slots=False)")
    if tuple(pred.slots.shape) != tuple(gt.slots.shape) or pred.slots.device != gt.slots.device:
        raise ValueError("prediction %s and ground truth %s differ in shape or device" % (tuple(pred.slots.shape), tuple(gt.slots.shape)))
    if pred.max_components > MAX_SLOTS or gt.max_components > MAX_SLOTS:
        raise ValueError("matching takes at most %d slots per map and side (max_components %d / %d)"
                         % (MAX_SLOTS, pred.max_components, gt.max_components))
    if not pred.slots.is_cuda:
        raise VkError("slot maps are on %s: no CPU fallback in this package" % pred.slots.device)


def contingency(pred: Detections, gt: Detections) -> torch.Tensor:
    """-> int32 [B, Mp + 1, Mg + 1] on the device: table[b, i, j] = pixels of map b in pred slot i - 1 and GT slot j - 1, index 0 = none.
    Every table sums to h w.  No host synchronisation."""
    _pair(pred, gt)
    B, h, w = (int(v) for v in pred.slots.shape)
    table = torch.empty(B, pred.max_components + 1, gt.max_components + 1, dtype=torch.int32, device=pred.slots.device)
    L.check(L.lib().vk_inst_contingency(B, h, w, pred.slots.data_ptr(), gt.slots.data_ptr(), pred.max_components, gt.max_components,
                                        table.data_ptr(), L.current_stream()), "vk_inst_contingency")
    return table


class MatchResult:
    """``table`` int32 [B, Mp + 1, Mg + 1]; per pred slot ``pair_gt`` int32 [B, Mp] (GT slot or -1), ``pair_iou`` and ``pair_derr``
    float64 [B, Mp]; ``per_image`` [B, K] and ``totals`` [K] ``vk_inst_stats`` records (uint8 tensors on the device, structured numpy
    arrays of ``STATS_DTYPE`` after ``.cpu()``); ``thresholds`` float64 [K]."""

    def __init__(self, thresholds, table, pair_gt, pair_iou, pair_derr, per_image, totals):
        self.thresholds, self.table, self.pair_gt, self.pair_iou, self.pair_derr = thresholds, table, pair_gt, pair_iou, pair_derr
        self.per_image, self.totals = per_image, totals

    def cpu(self) -> "MatchResult":
        """The same on the host (numpy), from one synchronisation."""
        if isinstance(self.table, np.ndarray):
            return self
        k = len(self.thresholds)
        per = self.per_image.cpu().numpy().reshape(-1).view(STATS_DTYPE).reshape(-1, k)
        tot = self.totals.cpu().numpy().reshape(-1).view(STATS_DTYPE).reshape(k)
        return MatchResult(self.thresholds, self.table.cpu().numpy(), self.pair_gt.cpu().numpy(), self.pair_iou.cpu().numpy(),
                           self.pair_derr.cpu().numpy(), per, tot)

    def metrics(self) -> Dict[str, np.ndarray]:
        return summarize(self.cpu().totals, self.thresholds)


def _match_call(B, Mp, Mg, table, n_pred, n_gt, thr, dp, sp, dg, sg, totals, device):
    k = int(thr.size)
    rec = STATS_DTYPE.itemsize
    pair_gt = torch.empty(B, Mp, dtype=torch.int32, device=device)
    pair_iou = torch.empty(B, Mp, dtype=torch.float64, device=device)
    pair_derr = torch.empty(B, Mp, dtype=torch.float64, device=device)
    per_image = G._record_buffer((B, k), rec, device)
    acc = totals is not None
    if acc:
        if totals.dtype != torch.uint8 or tuple(totals.shape) != (k, rec) or not totals.is_contiguous() or totals.device != device:
            raise ValueError("totals must be the uint8 [%d, %d] tensor of an earlier match on %s" % (k, rec, device))
    else:
        totals = G._record_buffer((k,), rec, device)
    L.check(L.lib().vk_inst_match(B, Mp, Mg, table.data_ptr(), n_pred.data_ptr(), n_gt.data_ptr(), k, thr.ctypes.data, dp, sp, dg, sg,
                                  pair_gt.data_ptr(), pair_iou.data_ptr(), pair_derr.data_ptr(), per_image.data_ptr(), totals.data_ptr(),
                                  1 if acc else 0, L.current_stream()), "vk_inst_match")
    return MatchResult(thr, table, pair_gt, pair_iou, pair_derr, per_image, totals)


def match(pred: Detections, gt: Detections, iou_thresholds=None, totals: Optional[torch.Tensor] = None,
          table: Optional[torch.Tensor] = None) -> MatchResult:
    """Pairs the objects of two ``Detections`` and sums the matched pairs' statistics at every IoU threshold; no host synchronisation.
    ``totals`` of an earlier result is added to in place (image after image, so the bits do not depend on the batching)."""
    thr = _iou_thresholds(iou_thresholds)
    _pair(pred, gt)
    if table is None:
        table = contingency(pred, gt)
    B = int(pred.slots.shape[0])
    return _match_call(B, pred.max_components, gt.max_components, table, pred.counts, gt.counts, thr,
                       pred.raw.data_ptr() + pred.diag_offset, pred.record_bytes, gt.raw.data_ptr() + gt.diag_offset, gt.record_bytes,
                       totals, pred.slots.device)


def _ratio(num, den, empty):
    out = np.full(len(den), empty, np.float64)
    nz = den != 0
    out[nz] = num[nz] / den[nz]
    return out


def summarize(totals: np.ndarray, thresholds=None) -> Dict[str, np.ndarray]:
    """``totals`` (structured [K], ``STATS_DTYPE``) -> the metrics per threshold, float64 on the host.  With a zero denominator
    precision, recall, f1, rq and pq are 1.0, sq and the diagonal means NaN."""
    t = np.asarray(totals).reshape(-1)
    tp, fp, fn, n_rel = (t[f].astype(np.float64) for f in ("tp", "fp", "fn", "n_rel"))
    f1 = _ratio(2.0 * tp, 2.0 * tp + fp + fn, 1.0)
    out = {"precision": _ratio(tp, tp + fp, 1.0), "recall": _ratio(tp, tp + fn, 1.0), "f1": f1, "rq": f1.copy(),
           "sq": _ratio(t["sum_iou"], tp, np.nan), "pq": _ratio(t["sum_iou"], tp + 0.5 * fp + 0.5 * fn, 1.0),
           "mean_abs_d": _ratio(t["sum_abs_d"], tp, np.nan), "mean_rel_d": _ratio(t["sum_rel_d"], n_rel, np.nan),
           "mean_signed_rel_d": _ratio(t["sum_signed_rel_d"], n_rel, np.nan), "mean_hv_rel": _ratio(t["sum_hv_rel"], n_rel, np.nan),
           "max_abs_d": t["max_abs_d"].astype(np.float64)}
    for f in ("tp", "fp", "fn", "n_rel", "n_split", "n_merge", "overflow_pred", "overflow_gt", "n_images"):
        out[f] = t[f].astype(np.int64)
    out["n_pred"], out["n_gt"] = t["n_pred_used"].astype(np.int64), t["n_gt_used"].astype(np.int64)
    if thresholds is not None:
        out["iou_thresholds"] = np.asarray(thresholds, np.float64).copy()
    return out


class ObjectMetrics:
    """The object metrics over an epoch: ``update(prob, target)`` per validation batch of any size, ``compute()`` at the end.
    ``update`` synchronises with nothing; ``compute`` reads the totals back once.  ``pred_args`` go to ``detect`` for the prediction;
    the target is detected with the ground-truth preset.  ``refine``: None, or a dict of ``vk.subpix.refine`` arguments (``method``,
    ``affine``, its parameters): then the corners of both the prediction's and the target's records are refined below a pixel before
    the diagonals are compared.  ``refine=dict(kind="keypoints", sigma=..., **refine_args)``: the vertex heatmap read-out instead;
    ``update`` then takes the predicted heatmap as ``heat``, the prediction's records go through ``vk.keypoints.refine(pred, heat,
    **refine_args)`` and the target's through the same call on the exact heatmap of their own integer corners
    (``vk.keypoints.targets(gt, shape, sigma)``), which returns those corners as ``RefinedDetections``.  ``kind="subpix"`` or no
    ``kind`` is ``vk.subpix.refine``."""

    def __init__(self, fit: str = "rect", iou_thresholds=None, max_components: int = 64, fit_outset_px: int = G.FIT_OUTSET_PX,
                 refine: Optional[dict] = None, **pred_args):
        G._fit(fit)
        if not 1 <= int(max_components) <= MAX_SLOTS:
            raise ValueError("max_components %r outside 1..%d" % (max_components, MAX_SLOTS))
        if refine is not None and not isinstance(refine, dict):
            raise ValueError("refine must be None or a dict of vk.subpix.refine arguments, got %r" % (refine,))
        self.thresholds = _iou_thresholds(iou_thresholds)
        self.refine = None if refine is None else dict(refine)
        self.refine_kind, self.kp_sigma = "subpix", None
        if self.refine is not None and "kind" in self.refine:
            self.refine_kind = self.refine.pop("kind")
            if self.refine_kind not in ("subpix", "keypoints"):
                raise ValueError("refine kind must be 'subpix' or 'keypoints', got %r" % (self.refine_kind,))
            if self.refine_kind == "keypoints":
                if "sigma" not in self.refine:
                    raise ValueError("refine=dict(kind='keypoints') needs sigma, the width of the heatmap's bumps in pixels")
                self.kp_sigma = float(self.refine.pop("sigma"))
                if not (self.kp_sigma > 0.0 and self.kp_sigma < float("inf")):
                    raise ValueError("refine sigma must be positive and finite, got %r" % (self.kp_sigma,))
        self.fit, self.max_components, self.fit_outset_px, self.pred_args = fit, int(max_components), int(fit_outset_px), dict(pred_args)
        self.reset()

    def reset(self) -> None:
        self._totals, self._images = None, 0

    @property
    def n_images(self) -> int:
        return self._images

    def update(self, prob: torch.Tensor, target: torch.Tensor, heat: Optional[torch.Tensor] = None) -> MatchResult:
        if not (isinstance(prob, torch.Tensor) and isinstance(target, torch.Tensor)) or prob.dim() != 3 or tuple(prob.shape) != tuple(target.shape):
            raise ValueError("expected prob and target [B, h, w] of one shape")
        keypoints = self.refine_kind == "keypoints"
        if keypoints and heat is None:
            raise ValueError("refine=dict(kind='keypoints') needs update(prob, target, heat=<the predicted heatmap [B, h, w]>)")
        if heat is not None and not keypoints:
            raise ValueError("update(heat=...) needs ObjectMetrics(refine=dict(kind='keypoints', sigma=...))")
        if keypoints and (not isinstance(heat, torch.Tensor) or tuple(heat.shape) != tuple(prob.shape)):
            raise ValueError("expected heat [B, h, w] of the shape of prob")
        if not (prob.is_cuda and target.is_cuda):
            raise VkError("object metrics take CUDA tensors (%s / %s): no CPU fallback in this package" % (prob.device, target.device))
        pred = detect(prob, fit=self.fit, fit_outset_px=self.fit_outset_px, max_components=self.max_components, **self.pred_args)
        gt = detect_gt(target, fit=self.fit, fit_outset_px=self.fit_outset_px, max_components=self.max_components)
        if keypoints:
            from . import keypoints as KP
            pred = KP.refine(pred, heat, **self.refine)
            gt = KP.refine(gt, KP.targets(gt, tuple(prob.shape[1:]), self.kp_sigma), **self.refine)
        elif self.refine is not None:
            from . import subpix
            pred, gt = subpix.refine(pred, prob, **self.refine), subpix.refine(gt, target.float(), **self.refine)
        res = match(pred, gt, self.thresholds, totals=self._totals)
        self._totals = res.totals
        self._images += int(prob.shape[0])
        return res

    def totals(self) -> np.ndarray:
        if self._totals is None:
            raise ValueError("ObjectMetrics.compute() before any update()")
        return self._totals.cpu().numpy().reshape(-1).view(STATS_DTYPE).reshape(len(self.thresholds))

    def compute(self) -> Dict[str, np.ndarray]:
        return summarize(self.totals(), self.thresholds)


def object_metrics(prob: torch.Tensor, target: torch.Tensor, fit: str = "rect", iou_thresholds=None, max_components: int = 64,
                   fit_outset_px: int = G.FIT_OUTSET_PX, refine: Optional[dict] = None, heat: Optional[torch.Tensor] = None,
                   **pred_args) -> Dict[str, np.ndarray]:
    """Everything in one call: detect both, count, match, summarise.  One read-back at the end."""
    om = ObjectMetrics(fit, iou_thresholds, max_components, fit_outset_px, refine=refine, **pred_args)
    om.update(prob, target, heat=heat)
    return om.compute()
