"""Threshold sweep: the validation metrics at EVERY binarisation threshold of a grid from one pass over prediction and target
(csrc/sweep.hip, ``vk_sweep_hist`` / ``vk_sweep_curves``).

Every consumer of the network's output takes a threshold (``seg_metrics``, ``predict_mask``, ``Segmenter``, ``tile_blend``, the geometry
post-processors; the reference's GUIs hand-pick 0.50 and 0.45), and ``vk.seg_metrics`` answers for one threshold per call.  Here one
read of the data leaves a per-image histogram of the prediction over the threshold grid, split by target value; its suffix sums are
the exact integer counts of ``vk.seg_metrics`` for every threshold at once::

    sw = vk.ThresholdSweep()                      # 0.01 ... 0.99, logits in
    for x, y in loader:
        sw.update(model(x), y)                    # no host synchronisation
    thr, dice = sw.compute(batch_mean=True).best("dice")

    hist [N, C, 2, K + 1] int32   hist[n, c, t, b] = elements of plane (n, c) with target t and b = #{k : pv > thr[k]}; pv = sigmoid(x)
                                  for logits (``vk.seg_metrics``' expression), x itself otherwise.  The comparison is strict, NaN
                                  lands in bin 0, +inf in bin K.
    target                        float32 or uint8 (``PatchDataset`` keeps uint8 masks on the device): 1 positive, 0 negative, a value
                                  equal to ``ignore_index`` is skipped, any other value is skipped and counted in ``bad``.

Row k of a ``SweepResult`` (``stats``, ``per_image``, ``dice``, ``iou``, ``mean_dice``, ``mean_iou``) holds the bits that
``vk.seg_metrics_device`` (C = 1) and ``vk.multiclass.seg_metrics_device(mode="multilabel")`` return at ``threshold=thr[k]``.  The micro
curve (``precision``, ``recall``, ``f1``, ``micro_iou``, ``fpr``) comes from the counts pooled over the images, in float64, a ratio with
a zero denominator being 1 (the false-positive rate 0).  ``ap`` (sum of (recall_k - recall_{k+1}) precision_k) and ``auc`` (trapezoid
rule over (fpr, recall), closed by (1, 1) and (0, 0)) see only the grid's operating points: both are limited by the grid, a finer grid
moves them.  Multiclass argmax has no threshold and is out of scope.  CUDA tensors only: there is no CPU fallback."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from ._lib import VkError

__all__ = ["DEFAULT_THRESHOLDS", "sweep_hist", "sweep_curves", "threshold_sweep", "SweepResult", "ThresholdSweep"]

MAX_THRESHOLDS = 1024
MAX_CLASSES = 16
MAX_IMAGES = 65535
DEFAULT_THRESHOLDS = (np.arange(1, 100) / 100).astype(np.float32)      # 0.01 ... 0.99; holds float32(0.5) and float32(0.45)
DEFAULT_THRESHOLDS.setflags(write=False)

_DTYPES = {"stats": torch.int64, "micro_stats": torch.int64, "micro": torch.float64, "ap": torch.float64, "auc": torch.float64,
           "best_dice": torch.int32, "best_iou": torch.int32, "best_f1": torch.int32, "best_mean": torch.int32,
           "epoch_dice": torch.float64, "epoch_iou": torch.float64, "epoch_mean_dice": torch.float64, "epoch_mean_iou": torch.float64}
_thr_cache = {}


def _thresholds(thresholds) -> np.ndarray:
    if thresholds is None:
        return DEFAULT_THRESHOLDS
    if isinstance(thresholds, torch.Tensor):
        thresholds = thresholds.detach().cpu().numpy()
    thr = np.ascontiguousarray(np.asarray(thresholds, dtype=np.float32))
    if thr.ndim != 1 or not 1 <= thr.size <= MAX_THRESHOLDS:
        raise ValueError("expected 1 to %d thresholds in one dimension, got shape %s" % (MAX_THRESHOLDS, thr.shape))
    if not np.isfinite(thr).all():
        raise ValueError("thresholds must be finite")
    if not (thr[1:] > thr[:-1]).all():
        raise ValueError("thresholds must be strictly ascending")
    return thr


def _thr_device(thr: np.ndarray, device) -> torch.Tensor:
    key = (thr.tobytes(), str(device))
    t = _thr_cache.get(key)
    if t is None:
        if len(_thr_cache) >= 16:
            _thr_cache.clear()
        t = _thr_cache[key] = torch.from_numpy(thr.copy()).to(device)
    return t


def _planes(t: torch.Tensor, n: int, c: int) -> Tuple[torch.Tensor, int]:
    """[N, C, L] view (or copy) of t and the distance between its planes, in elements."""
    p = t.detach().reshape(n, c, -1)
    length = p.shape[2]
    s0, s1, s2 = p.stride()
    step = s1 if c > 1 else s0 if n > 1 else length
    if (s2 == 1 or length == 1) and length <= step < 2 ** 31 and (c == 1 or n == 1 or s0 == c * s1):
        return p, step
    return p.contiguous(), length


def sweep_hist(pred: torch.Tensor, target: torch.Tensor, thresholds=None, from_logits: bool = True, ignore_index: Optional[int] = None,
               out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (hist int32 [N, C, 2, K + 1], bad int32 [1]) on the device; no host synchronisation.

    pred [N, C, H, W], [N, C, L] or [H, W] (float); target of the same shape, float32 or uint8.  ``out=(hist, bad)`` of an earlier call
    adds into it, so a plane can be fed in pieces (a slice along the last axis of a contiguous tensor is read in place)."""
    thr = _thresholds(thresholds)
    if pred.dim() == 2:
        n, c = 1, 1
    elif pred.dim() in (3, 4):
        n, c = int(pred.shape[0]), int(pred.shape[1])
    else:
        raise ValueError("expected pred [N, C, H, W], [N, C, L] or [H, W], got %s" % (tuple(pred.shape),))
    if tuple(target.shape) != tuple(pred.shape):
        raise ValueError("target must have pred's shape %s, got %s" % (tuple(pred.shape), tuple(target.shape)))
    if n < 1 or pred.numel() == 0:
        raise ValueError("empty prediction %s" % (tuple(pred.shape),))
    if not 1 <= c <= MAX_CLASSES:
        raise ValueError("expected 1 <= C <= %d class planes, got %d" % (MAX_CLASSES, c))
    if not pred.is_floating_point():
        raise ValueError("pred must be a floating-point tensor, got %s" % pred.dtype)
    if target.dtype not in (torch.float32, torch.uint8):
        raise ValueError("target must be float32 or uint8, got %s" % target.dtype)
    if ignore_index is not None and int(ignore_index) != ignore_index:
        raise ValueError("ignore_index must be an integer, got %r" % (ignore_index,))
    if not (pred.is_cuda and target.is_cuda):
        raise VkError("the threshold sweep takes CUDA tensors (%s / %s): no CPU fallback in this package" % (pred.device, target.device))
    k = int(thr.size)
    p, ps = _planes(pred.to(torch.float32), n, c)
    t, ts = _planes(target, n, c)
    if ps != ts:
        p, t = p.contiguous(), t.contiguous()
        ps = p.shape[2]
    per_plane = int(p.shape[2])
    if out is None:
        hist = torch.empty(n, c, 2, k + 1, dtype=torch.int32, device=p.device)
        bad = torch.empty(1, dtype=torch.int32, device=p.device)
    else:
        hist, bad = out
        if tuple(hist.shape) != (n, c, 2, k + 1) or hist.dtype != torch.int32 or not hist.is_contiguous() or hist.device != p.device:
            raise ValueError("out[0] must be a contiguous int32 %s on %s" % ((n, c, 2, k + 1), p.device))
        if bad.numel() != 1 or bad.dtype != torch.int32 or bad.device != p.device:
            raise ValueError("out[1] must be one int32 on %s" % (p.device,))
    L.check(L.lib().vk_sweep_hist(n * c, per_plane, int(ps), p.data_ptr(), t.data_ptr(), 1 if t.dtype == torch.uint8 else 0,
                                  1 if from_logits else 0, 0 if ignore_index is None else 1, 0 if ignore_index is None else int(ignore_index),
                                  k, thr.ctypes.data, _thr_device(thr, p.device).data_ptr(), 0 if out is None else 1, hist.data_ptr(),
                                  bad.data_ptr(), L.current_stream()), "vk_sweep_hist")
    return hist, bad


class SweepResult:
    """The curves of one sweep, as views into one buffer (device tensors; ``.cpu()`` gives the same on the host).

    K thresholds, N images, C classes, G groups:  ``stats`` int64 [K, 4, N, C] {tp, fp, fn, tn};  ``per_image`` fp32 [K, N, C, 2] {dice, iou};
    ``dice``, ``iou`` fp32 [K, C] and ``mean_dice``, ``mean_iou`` fp32 [K] (batch means);  ``micro_stats`` int64 [4, K, C];  ``precision``,
    ``recall``, ``f1``, ``micro_iou``, ``fpr`` float64 [K, C];  ``ap``, ``auc`` float64 [C];  ``best_dice``, ``best_iou``, ``best_f1`` int32 [C],
    ``best_mean_dice``, ``best_mean_iou`` int32 [] (lowest k of the best value).  With groups: ``group_dice``, ``group_iou`` fp32 [G, K, C],
    ``group_mean_dice``, ``group_mean_iou`` fp32 [G, K], and the means of the batch means ``epoch_dice``, ``epoch_iou`` float64 [K, C],
    ``epoch_mean_dice``, ``epoch_mean_iou`` float64 [K].  ``bad``: the device count of bad target values, when the histogram came with one."""

    def __init__(self, blob: torch.Tensor, layout, dims, thresholds: np.ndarray, bad: Optional[torch.Tensor], base: int = 0):
        self._blob, self._layout, self._dims, self._base = blob, layout, dims, base
        self.thresholds, self.bad = thresholds, bad
        self._host = None
        n, c, k, g = dims
        shapes = {"stats": (k, 4, n, c), "per_image": (k, n, c, 2), "dice": (k, c), "iou": (k, c), "mean_dice": (k,), "mean_iou": (k,),
                  "micro_stats": (4, k, c), "micro": (5, k, c), "ap": (c,), "auc": (c,), "best_dice": (c,), "best_iou": (c,), "best_f1": (c,),
                  "best_mean": (2,)}
        if g:
            shapes.update({"group_dice": (g, k, c), "group_iou": (g, k, c), "group_mean_dice": (g, k), "group_mean_iou": (g, k),
                           "epoch_dice": (k, c), "epoch_iou": (k, c), "epoch_mean_dice": (k,), "epoch_mean_iou": (k,)})
        for name in L.SWEEP_FIELDS:
            shape = shapes.get(name)
            off = getattr(layout, name) - base
            if shape is None or off < 0:
                setattr(self, name, None)
                continue
            dt = _DTYPES.get(name, torch.float32)
            nbytes = int(np.prod(shape)) * torch.empty(0, dtype=dt).element_size()
            setattr(self, name, blob[off:off + nbytes].view(dt).view(shape))
        self.precision, self.recall, self.f1, self.micro_iou, self.fpr = self.micro.unbind(0)
        self.best_mean_dice, self.best_mean_iou = self.best_mean.unbind(0)

    @property
    def n_groups(self) -> int:
        return self._dims[3]

    def cpu(self, per_image: bool = True) -> "SweepResult":
        """The same result on the host, from one read-back (``per_image=False`` leaves ``stats`` and ``per_image`` behind: they are
        K N C 40 bytes, everything else is small)."""
        if self._blob.device.type == "cpu":
            return self
        base = 0 if per_image else int(self._layout.dice)
        blob = self._blob[base - self._base:].to("cpu", non_blocking=True)
        bad = None if self.bad is None else self.bad.cpu()          # synchronises the stream: both copies are complete
        if bad is None:
            torch.cuda.current_stream(self._blob.device).synchronize()
        return SweepResult(blob, self._layout, self._dims, self.thresholds, bad, base)

    def best(self, metric: str = "dice", cls: Optional[int] = None, batch_mean: Optional[bool] = None) -> Tuple[float, float]:
        """(threshold, value) of the best ``metric``: "dice" / "iou" (the mean over the classes, or class ``cls``) or "f1" (micro F1 of
        class ``cls``, 0 by default).  With groups the curve is the mean of the batch means unless ``batch_mean=False``.  One read-back;
        raises VkError when the target held bad values."""
        if metric not in ("dice", "iou", "f1"):
            raise ValueError("metric must be 'dice', 'iou' or 'f1', got %r" % (metric,))
        c = self._dims[1]
        if cls is not None and not 0 <= cls < c:
            raise ValueError("class %r outside [0, %d)" % (cls, c))
        if self._host is None:
            self._host = self.cpu(per_image=False)
        h = self._host
        if h.bad is not None and int(h.bad.item()):
            raise VkError("the sweep's target holds %d value(s) other than 0, 1 or the ignore value" % int(h.bad.item()))
        epoch = self.n_groups > 0 if batch_mean is None else bool(batch_mean)
        if epoch and self.n_groups == 0:
            raise ValueError("batch_mean needs a sweep computed with groups")
        if metric == "f1":
            k = int(h.best_f1[cls or 0])
            return float(self.thresholds[k]), float(h.f1[k, cls or 0])
        if epoch:
            curve = getattr(h, "epoch_mean_" + metric) if cls is None else getattr(h, "epoch_" + metric)[:, cls]
            k = int(np.argmax(curve.numpy()))                       # the first maximum: ties to the lowest k
            return float(self.thresholds[k]), float(curve[k])
        if cls is None:
            k = int(getattr(h, "best_mean_" + metric))
            return float(self.thresholds[k]), float(getattr(h, "mean_" + metric)[k])
        k = int(getattr(h, "best_" + metric)[cls])
        return float(self.thresholds[k]), float(getattr(h, metric)[k, cls])


def sweep_curves(hist: torch.Tensor, thresholds=None, groups=None, eps: float = 1e-7, n_groups: Optional[int] = None,
                 bad: Optional[torch.Tensor] = None) -> SweepResult:
    """hist int32 [N, C, 2, K + 1] of ``sweep_hist`` -> ``SweepResult``; no host synchronisation.

    ``groups``: the validation batch of every image, a sequence of N ints in [0, G) (G = the largest + 1) or an int32 device tensor
    together with ``n_groups``; an image whose value is outside [0, G) belongs to no batch."""
    thr = _thresholds(thresholds)
    if hist.dim() != 4 or hist.shape[2] != 2 or hist.dtype != torch.int32:
        raise ValueError("expected an int32 histogram [N, C, 2, K + 1], got %s %s" % (hist.dtype, tuple(hist.shape)))
    n, c, k = int(hist.shape[0]), int(hist.shape[1]), int(hist.shape[3]) - 1
    if k != thr.size:
        raise ValueError("the histogram has %d bins: expected %d thresholds, got %d" % (k + 1, k, thr.size))
    if not (1 <= n <= MAX_IMAGES and 1 <= c <= MAX_CLASSES):
        raise ValueError("expected 1 <= N <= %d images and 1 <= C <= %d classes, got %d and %d" % (MAX_IMAGES, MAX_CLASSES, n, c))
    if not hist.is_cuda:
        raise VkError("the threshold sweep takes CUDA tensors (%s): no CPU fallback in this package" % hist.device)
    g, grp = 0, None
    if groups is not None:
        if isinstance(groups, torch.Tensor):
            if n_groups is None:
                raise ValueError("a tensor of groups needs n_groups")
            if tuple(groups.shape) != (n,) or groups.dtype != torch.int32:
                raise ValueError("groups must be int32 [%d], got %s %s" % (n, groups.dtype, tuple(groups.shape)))
            g, grp = int(n_groups), groups.to(hist.device).contiguous()
        else:
            a = np.asarray(groups)
            if a.shape != (n,) or a.dtype.kind not in "iu" or (a < 0).any():
                raise ValueError("groups must be %d non-negative ints" % n)
            g = int(a.max()) + 1 if n_groups is None else int(n_groups)
            grp = torch.from_numpy(a.astype(np.int32)).to(hist.device)
        if not 1 <= g <= n:
            raise ValueError("expected 1 <= n_groups <= N = %d, got %d" % (n, g))
    lib = L.lib()
    lay = L.vk_sweep_layout()
    L.check(lib.vk_sweep_curves_layout(n, c, k, g, C.byref(lay)), "vk_sweep_curves_layout")
    blob = torch.empty(int(lay.total_bytes), dtype=torch.uint8, device=hist.device)
    ws = torch.empty(int(lay.workspace_bytes) // 8 + 1, dtype=torch.int64, device=hist.device) if g else None
    h = hist.detach().contiguous()
    L.check(lib.vk_sweep_curves(n, c, k, h.data_ptr(), L.ptr(grp), g, float(eps), L.ptr(ws), int(lay.workspace_bytes), blob.data_ptr(),
                                int(lay.total_bytes), L.current_stream()), "vk_sweep_curves")
    return SweepResult(blob, lay, (n, c, k, g), thr, bad)


def threshold_sweep(pred: torch.Tensor, target: torch.Tensor, thresholds=None, from_logits: bool = True, ignore_index: Optional[int] = None,
                    groups=None, eps: float = 1e-7, n_groups: Optional[int] = None) -> SweepResult:
    """``sweep_hist`` then ``sweep_curves``: every threshold's metrics of one batch."""
    thr = _thresholds(thresholds)
    hist, bad = sweep_hist(pred, target, thr, from_logits, ignore_index)
    return sweep_curves(hist, thr, groups, eps, n_groups, bad)


class ThresholdSweep:
    """The sweep over an epoch: ``update(pred, target)`` per validation batch, ``compute()`` at the end.  Batches may differ in N, H and W
    (the histogram does not depend on the image size), so native-resolution outputs of ``vk.tiling.infer_tiled`` go in one image at a
    time.  Nothing synchronises with the host until a result is read."""

    def __init__(self, thresholds=None, from_logits: bool = True, ignore_index: Optional[int] = None, eps: float = 1e-7):
        self.thresholds = _thresholds(thresholds)
        self.from_logits, self.ignore_index, self.eps = from_logits, ignore_index, eps
        self.reset()

    def reset(self) -> None:
        self._hists, self._groups, self._bad, self._images = [], [], None, 0

    @property
    def n_images(self) -> int:
        return self._images

    @property
    def n_batches(self) -> int:
        return len(self._hists)

    def update(self, pred: torch.Tensor, target: torch.Tensor) -> None:
        hist, bad = sweep_hist(pred, target, self.thresholds, self.from_logits, self.ignore_index)
        if self._hists and hist.shape[1] != self._hists[0].shape[1]:
            raise ValueError("this sweep holds %d class planes per image, got %d" % (self._hists[0].shape[1], hist.shape[1]))
        if self._images + hist.shape[0] > MAX_IMAGES:
            raise ValueError("a sweep holds at most %d images" % MAX_IMAGES)
        self._groups.append(torch.full((hist.shape[0],), len(self._hists), dtype=torch.int32, device=hist.device))
        self._hists.append(hist)
        self._bad = bad if self._bad is None else self._bad + bad
        self._images += int(hist.shape[0])

    def compute(self, batch_mean: bool = False) -> SweepResult:
        """The sweep over every image seen; ``batch_mean=True`` adds the reference's mean of batch means (``epoch_*``, and what
        ``best`` then reads)."""
        if not self._hists:
            raise ValueError("ThresholdSweep.compute() before any update()")
        hist = torch.cat(self._hists)
        if batch_mean:
            return sweep_curves(hist, self.thresholds, torch.cat(self._groups), self.eps, len(self._hists), self._bad)
        return sweep_curves(hist, self.thresholds, None, self.eps, None, self._bad)
