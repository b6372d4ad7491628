"""Vertex heatmaps (csrc/keypoints.hip): the targets of a heatmap plane beside the mask, and its read-out.

Every other estimator of the package reads the four vertices from the mask plane, where a vertex is the end of two soft edges.  Here
the network predicts them directly::

    model = vk.multiclass.Unet(classes=2)                                  # plane 0 the mask, plane 1 the vertex heatmap
    for x, y2, names in vk.keypoints.with_targets(dataset.loader(8)):      # y2 float32 [N, 2, H, W], built on the device
        model.loss_and_backward(x, y2, loss=loss)                          # INTEGRATION.md, "Predicting the vertices"
    probs2 = torch.sigmoid(model(x))
    dets = vk.instances.detect(probs2[:, 0].contiguous(), fit="quad")
    fine = vk.keypoints.refine(dets, probs2[:, 1])                         # RefinedDetections: to match, render and zoom.merge as it is
    vk.keypoints.peaks(probs2[:, 1]).records()                             # or every local maximum, without a mask

The loss such a model is trained with (csrc/kp_loss.hip behind ``vk_kp_loss``): per-plane terms that join a
``vk.seglosses`` sum of mode binary or multilabel, in the module form and in the fused step (``vk_unet_loss_kp``)::

    L = vk.seglosses
    loss = (vk.keypoints.PlaneBCE([0]) + L.DiceLoss("multilabel", classes=[0])
            + w * vk.keypoints.HeatmapFocalLoss([1], pos_threshold=vk.keypoints.positive_threshold(sigma)))

Coordinates are those of the geometry records: pixel (x, y) lies at the point (x, y).  ``vk.micrographs.truth()`` uses the same
convention (its vertices are the renderer's 1/16-pixel fixed point divided by 16), so its vertices go to ``targets`` unconverted.
CUDA tensors only: there is no CPU fallback."""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Iterable, List, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import _lib as L
from . import _lossfn, lovasz, seglosses
from . import geometry as G
from . import instances as I
from . import subpix as SP
from ._lib import VkError

__all__ = ["FLAGS", "PEAK_DTYPE", "HeatmapFocalLoss", "LossSum", "Peaks", "PlaneBCE", "gaussian_table", "make_targets", "params", "peaks",
           "positive_threshold", "postprocess", "refine", "table_radius16", "targets", "vertex_metrics", "with_targets"]

FLAGS = dict(L.KP_FLAGS)                       # beside vk.subpix.FLAGS, in the same per-vertex field
PEAK_DTYPE = np.dtype(L.vk_kp_peak)
_METHODS = {"parabola": L.VK_KP_PARABOLA, "centroid": L.VK_KP_CENTROID}
_TABLE_FLAGS = {None: 0, "memory": L.VK_KP_TABLE_MEMORY, "lds": L.VK_KP_TABLE_LDS}
_tables: Dict[Tuple[float, float, str], torch.Tensor] = {}


def table_radius16(sigma: float, cutoff: float = 3.0) -> int:
    """R16 = ceil(16 * cutoff * sigma): the disc's radius in sixteenths of a pixel."""
    sigma, cutoff = float(sigma), float(cutoff)
    if not (sigma > 0.0 and cutoff > 0.0 and math.isfinite(sigma) and math.isfinite(cutoff)):
        raise ValueError("sigma and cutoff must be positive and finite, got %r, %r" % (sigma, cutoff))
    r16 = int(math.ceil(16.0 * cutoff * sigma))
    if not 1 <= r16 <= L.VK_KP_MAX_RADIUS16:
        raise ValueError("16 * cutoff * sigma = %d outside 1..%d" % (r16, L.VK_KP_MAX_RADIUS16))
    return r16


def gaussian_table(sigma: float, cutoff: float = 3.0, device=None) -> torch.Tensor:
    """float32 [R16^2 + 1]: table[k] = float32(exp(-(k / 256) / (2 sigma^2))), the exp in float64 on the host (no transcendental runs
    on the device), indexed by the squared distance in 1/16 pixels.  Cached per (sigma, cutoff, device); ``device=None`` is the host."""
    r16 = table_radius16(sigma, cutoff)
    key = (float(sigma), float(cutoff), str(device))
    t = _tables.get(key)
    if t is None:
        s2 = 2.0 * float(sigma) * float(sigma)
        host = np.array([math.exp(-(k / 256.0) / s2) for k in range(r16 * r16 + 1)], np.float64).astype(np.float32)
        t = torch.from_numpy(host)
        if device is not None:
            t = t.to(device)
        _tables[key] = t
    return t


def _vertex_source(src, counts):
    """-> (tensor that owns the records, stride, vertex offset, vertex type, valid offset, counts, max_components, map shape or None)."""
    if isinstance(src, SP.RefinedDetections):
        shape = None if src.slots is None else tuple(src.slots.shape[1:])
        return src.raw, 200, int(L.vk_subpix_quad.v.offset), L.VK_KP_VERT_F64, int(L.vk_subpix_quad.valid.offset), src.counts, src.max_components, shape
    if isinstance(src, G.Detections):
        shape = None if src.slots is None else tuple(src.slots.shape[1:])
        return src.raw, src.record_bytes, src.box_offset, L.VK_KP_VERT_I32, src.valid_offset, src.counts, src.max_components, shape
    if isinstance(src, torch.Tensor):
        if src.dim() != 4 or tuple(src.shape[2:]) != (4, 2) or src.dtype != torch.float64:
            raise ValueError("expected Detections, RefinedDetections or a float64 tensor [B, M, 4, 2], got %s %s" % (src.dtype, tuple(src.shape)))
        if counts is None:
            raise ValueError("a vertex tensor needs counts (int32 [B])")
        return src.contiguous(), 64, 0, L.VK_KP_VERT_F64, -1, counts, int(src.shape[1]), None
    raise ValueError("expected Detections, RefinedDetections or a float64 tensor [B, M, 4, 2]")


def _plane(t: torch.Tensor, what: str) -> Tuple[torch.Tensor, int, int, int, int]:
    """A float32 [B, h, w] view whose maps are dense (rows w apart) and one batch stride apart -> (t, B, h, w, image stride)."""
    if not isinstance(t, torch.Tensor) or t.dim() != 3 or t.dtype != torch.float32:
        raise ValueError("%s: expected a float32 tensor [B, h, w]" % what)
    if not t.is_cuda:
        raise VkError("%s is on %s: this package runs on an MI355X only and has no CPU fallback" % (what, t.device))
    B, h, w = (int(v) for v in t.shape)
    if not ((t.stride(2) == 1 or w == 1) and (t.stride(1) == w or h == 1) and (B == 1 or t.stride(0) >= h * w)):
        raise ValueError("%s: strides %s: a map must be dense and the maps one batch stride (>= h w) apart" % (what, tuple(t.stride())))
    return t, B, h, w, (int(t.stride(0)) if B > 1 else h * w)


def targets(dets_or_vertices, shape: Optional[Tuple[int, int]] = None, sigma: float = 2.0, out: Optional[torch.Tensor] = None,
            counts: Optional[torch.Tensor] = None, cutoff: float = 3.0, table: Optional[str] = None) -> torch.Tensor:
    """``vk_kp_targets``: float32 [B, h, w], the maximum over the used vertices of a Gaussian of ``sigma`` pixels cut at ``cutoff``
    sigma, 1.0 at a vertex that lies on a pixel.  ``dets_or_vertices``: ``Detections`` (int32 corners), ``RefinedDetections`` (float64
    ``v``) or a float64 tensor [B, M, 4, 2] with ``counts`` int32 [B].  ``shape``: (h, w); taken from the detections' slot map or from
    ``out`` when left out.  ``out``: a float32 view [B, h, w] that is filled in place, for example ``y2[:, 1]``.  ``table``: None (the
    library's choice), "memory" or "lds" (a measurement switch; the bytes are the same).  No host synchronisation."""
    raw, stride, voff, vtype, valid_off, cnt, M, det_shape = _vertex_source(dets_or_vertices, counts)
    if table not in _TABLE_FLAGS:
        raise ValueError("table must be None, 'memory' or 'lds', got %r" % (table,))
    if not raw.is_cuda:
        raise VkError("vertex records are on %s: this package runs on an MI355X only and has no CPU fallback" % raw.device)
    B = int(raw.shape[0])
    if out is not None:
        out, Bo, h, w, istride = _plane(out, "out")
        if shape is not None and (int(shape[0]), int(shape[1])) != (h, w):
            raise ValueError("shape %s is not that of out %s" % (tuple(shape), (h, w)))
    else:
        if shape is None:
            shape = det_shape
        if shape is None:
            raise ValueError("shape=(h, w) is needed: neither a slot map nor out gives it")
        h, w = int(shape[0]), int(shape[1])
        out = torch.empty(B, h, w, dtype=torch.float32, device=raw.device)
        Bo, istride = B, h * w
    if Bo != B or out.device != raw.device:
        raise ValueError("out holds %d maps on %s, the records %d on %s" % (Bo, out.device, B, raw.device))
    if not isinstance(cnt, torch.Tensor) or cnt.dtype != torch.int32 or tuple(cnt.shape) != (B,) or cnt.device != raw.device:
        raise ValueError("counts must be an int32 tensor [%d] on %s" % (B, raw.device))
    tab = gaussian_table(sigma, cutoff, raw.device)
    with torch.cuda.device(raw.device):
        L.check(L.lib().vk_kp_targets(B, h, w, raw.data_ptr(), stride, voff, vtype, valid_off, cnt.contiguous().data_ptr(), M, tab.data_ptr(),
                                      int(tab.numel()), out.data_ptr(), istride, _TABLE_FLAGS[table], L.current_stream()), "vk_kp_targets")
    return out


def make_targets(mask: torch.Tensor, fit: str = "quad", refine: Optional[dict] = None, sigma: float = 2.0, max_components: int = 64,
                 fit_outset_px: int = 0) -> torch.Tensor:
    """``mask`` [N, 1, H, W] or [N, H, W] in {0, 1} on the device -> ``y2`` float32 [N, 2, H, W]: plane 0 the mask, plane 1 the heatmap
    of the vertices ``vk.instances.detect_gt(mask, fit)`` finds (``fit_outset_px`` 0: the corners of the mask itself), optionally moved by
    ``vk.subpix.refine(..., **refine)`` on the mask first.  No host synchronisation."""
    if not isinstance(mask, torch.Tensor) or mask.dim() not in (3, 4) or (mask.dim() == 4 and mask.shape[1] != 1):
        raise ValueError("expected a mask [N, 1, H, W] or [N, H, W]")
    if not mask.is_cuda:
        raise VkError("masks are on %s: this package runs on an MI355X only and has no CPU fallback" % mask.device)
    m = (mask[:, 0] if mask.dim() == 4 else mask).float().contiguous()
    N, H, W = (int(v) for v in m.shape)
    y2 = torch.empty(N, 2, H, W, dtype=torch.float32, device=m.device)
    y2[:, 0] = m
    dets = I.detect_gt(m, fit=fit, fit_outset_px=fit_outset_px, max_components=max_components)
    if refine is not None:
        dets = SP.refine(dets, m, **refine)
    targets(dets, sigma=sigma, out=y2[:, 1])
    return y2


def with_targets(loader: Iterable, **kw):
    """Wraps any of the package's loaders (``(x, y, names)`` with ``y`` [N, 1, H, W]) and yields ``(x, y2, names)``, ``y2`` by
    ``make_targets(y, **kw)`` on the masks as the loader augmented them."""
    for x, y, names in loader:
        yield x, make_targets(y, **kw), names


# ------------------------------------------------------------------------------------------------ read-out
class Peaks:
    """``raw`` uint8 [B, max_peaks, 16] (``vk_kp_peak`` records in raster order) and ``counts`` int32 [B] (every peak of a map, also
    above ``max_peaks``), on the device."""

    def __init__(self, raw: torch.Tensor, counts: torch.Tensor, max_peaks: int):
        self.raw, self.counts, self.max_peaks = raw, counts, int(max_peaks)

    def records(self) -> List[np.ndarray]:
        """Per map its min(count, max_peaks) records (``PEAK_DTYPE``).  The only method that reads back."""
        host = self.raw.cpu().numpy().reshape(-1).view(PEAK_DTYPE).reshape(self.raw.shape[0], self.max_peaks)
        cnt = self.counts.cpu().numpy()
        return [host[b, :min(int(cnt[b]), self.max_peaks)].copy() for b in range(host.shape[0])]


def peaks(heat: torch.Tensor, min_peak: float = 0.3, nms_radius: int = 2, max_peaks: int = 64) -> Peaks:
    """``vk_kp_peaks``: the local maxima of ``heat`` float32 [B, h, w] (a strided plane such as ``probs2[:, 1]`` is read in place):
    value >= ``min_peak``, nothing larger in the (2 ``nms_radius`` + 1)^2 window and no equal value earlier in it.  No host
    synchronisation."""
    heat, B, h, w, istride = _plane(heat.detach() if isinstance(heat, torch.Tensor) else heat, "heat")
    lib = L.lib()
    nbytes = int(lib.vk_kp_peaks_workspace_bytes(B, h, w))
    dev = heat.device
    ws = torch.empty(max(nbytes, 4) // 4 + 1, dtype=torch.int32, device=dev)
    raw = torch.zeros(B, int(max_peaks) if 1 <= int(max_peaks) <= 4096 else 1, PEAK_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    counts = torch.zeros(B, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        L.check(lib.vk_kp_peaks(B, h, w, heat.data_ptr(), istride, float(min_peak), int(nms_radius), int(max_peaks), raw.data_ptr(),
                                counts.data_ptr(), ws.data_ptr(), ws.numel() * 4, L.current_stream()), "vk_kp_peaks")
    return Peaks(raw, counts, max_peaks)


def params(method: str = "parabola", search: int = 6, cwin: int = 3, min_peak: float = 0.3, floor_frac: float = 0.25) -> L.vk_kp_params:
    """The parameter block of ``refine``: ``method`` "parabola" or "centroid", ``search`` 1..31, ``cwin`` 1..7, ``min_peak`` finite,
    ``floor_frac`` in [0, 1).  The ranges are checked by the library."""
    if method not in _METHODS:
        raise ValueError("method must be 'parabola' or 'centroid', got %r" % (method,))
    p = L.vk_kp_params()
    p.method, p.search, p.cwin, p.min_peak, p.floor_frac = _METHODS[method], int(search), int(cwin), float(min_peak), float(floor_frac)
    return p


def refine(dets: G.Detections, heat: torch.Tensor, method: str = "parabola", affine=None, search: int = 6, cwin: int = 3,
           min_peak: float = 0.3, floor_frac: float = 0.25) -> SP.RefinedDetections:
    """``vk_kp_refine``: moves every corner of ``dets`` to the heatmap peak within ``search`` pixels of it, to a fraction of a pixel by
    a three-point parabola per axis or by the centroid over (2 ``cwin`` + 1)^2 above ``floor_frac`` of the peak.  ``heat``: float32
    [B, h, w], dense or a strided plane (``probs2[:, 1]``).  Returns ``RefinedDetections`` (per-vertex flags: ``FLAGS``), so the result
    goes to ``vk.instances.match``, ``vk.render`` and ``vk.zoom.merge`` unchanged.  ``affine`` as in ``vk.subpix.refine``.  No host
    synchronisation."""
    if not isinstance(dets, G.Detections) or isinstance(dets, SP.RefinedDetections):
        raise ValueError("expected the Detections of vk.instances.detect")
    if dets.slots is None:
        raise ValueError("refinement needs the slot map: these Detections were made with detect(slots=False)")
    p = params(method, search, cwin, min_peak, floor_frac)
    heat, B, h, w, istride = _plane(heat.detach() if isinstance(heat, torch.Tensor) else heat, "heat")
    if not dets.raw.is_cuda:
        raise VkError("detections are on %s: this package runs on an MI355X only and has no CPU fallback" % dets.raw.device)
    if (B, h, w) != tuple(dets.slots.shape) or heat.device != dets.raw.device:
        raise ValueError("the map %s is not the size of the one the detections %s were made from" % ((B, h, w), tuple(dets.slots.shape)))
    aff = SP._affine_tensor(affine, B, heat.device)
    out = G._record_buffer((B, dets.max_components), SP.RECORD_DTYPE.itemsize, heat.device, zero=True)
    with torch.cuda.device(heat.device):
        L.check(L.lib().vk_kp_refine(C.byref(p), B, h, w, heat.data_ptr(), istride, dets.raw.data_ptr(), dets.record_bytes, dets.box_offset,
                                     dets.valid_offset, dets.counts.data_ptr(), dets.max_components, L.ptr(aff), out.data_ptr(),
                                     L.current_stream()), "vk_kp_refine")
    return SP.RefinedDetections(dets, out, method)


def postprocess(probs2: torch.Tensor, fit: str = "quad", method: str = "parabola", affine=None, refine_args: Optional[Dict] = None,
                **detect_args) -> Tuple[torch.Tensor, List[List[Dict]]]:
    """``probs2`` float32 [B, 2, h, w] on the device -> what ``vk.subpix.postprocess`` returns: ``vk.instances.detect`` on plane 0 and
    ``refine`` on plane 1 (read in place), then per map the detection list with ``d1``, ``d2``, ``d_mean`` refined, ``box_subpix``,
    ``box_subpix_map`` and ``subpix_flags`` (``vk.subpix.FLAGS`` and ``FLAGS`` bits) added."""
    if not isinstance(probs2, torch.Tensor) or probs2.dim() != 4 or probs2.shape[1] != 2:
        raise ValueError("expected a float32 tensor [B, 2, h, w]")
    if not probs2.is_cuda:
        raise VkError("probability maps are on %s: this package runs on an MI355X only and has no CPU fallback" % probs2.device)
    probs2 = probs2.detach().float()
    dets = G.detect(probs2[:, 0].contiguous(), fit=fit, **detect_args)
    fine = refine(dets, probs2[:, 1], method=method, affine=affine, **(refine_args or {}))
    counts = dets.counts.cpu().numpy()                    # synchronises; read once for both record lists
    out = []
    for coarse, recs in zip(dets.records(counts), fine.records(counts)):
        by_label = dict(zip(recs["label"].tolist(), recs))
        rows = G._fit(fit).to_dicts(coarse)
        for d in rows:
            r = by_label[d["label"]]
            d.update(d1=float(r["d1"]), d2=float(r["d2"]), d_mean=float(r["d_mean"]), box_subpix=r["vs"].reshape(4, 2).copy(),
                     box_subpix_map=r["v"].reshape(4, 2).copy(), subpix_flags=r["flags"].copy())
        out.append(rows)
    return dets.clean, out


def vertex_metrics(peaks, gt, tol_px: float = 2.0) -> Dict[str, float]:
    """Host side, from two read-back lists of one map: ``peaks`` the records of ``Peaks.records()[b]`` (or an array [n, 2] of (x, y)),
    ``gt`` an array [m, 2].  Greedy nearest matching in a stated order: all pairs within ``tol_px`` (Euclidean) sorted by (distance,
    peak index, gt index); a pair is taken when neither end is taken yet.  -> tp, fp, fn, precision, recall (1.0 where the denominator
    is empty) and mean_dist over the matched pairs (0.0 without one)."""
    if isinstance(peaks, np.ndarray) and peaks.dtype.names:
        pk = np.stack([peaks["x"], peaks["y"]], axis=1).astype(np.float64) if len(peaks) else np.zeros((0, 2))
    else:
        pk = np.asarray(peaks, np.float64).reshape(-1, 2)
    g = np.asarray(gt, np.float64).reshape(-1, 2)
    pairs = []
    for i in range(len(pk)):
        for j in range(len(g)):
            d = math.hypot(pk[i, 0] - g[j, 0], pk[i, 1] - g[j, 1])
            if d <= float(tol_px):
                pairs.append((d, i, j))
    pairs.sort()
    used_p, used_g, dist = set(), set(), []
    for d, i, j in pairs:
        if i not in used_p and j not in used_g:
            used_p.add(i)
            used_g.add(j)
            dist.append(d)
    tp = len(dist)
    fp, fn = len(pk) - tp, len(g) - tp
    return dict(tp=tp, fp=fp, fn=fn, precision=tp / (tp + fp) if tp + fp else 1.0, recall=tp / (tp + fn) if tp + fn else 1.0,
                mean_dist=float(np.mean(dist)) if dist else 0.0)


# ------------------------------------------------------------------------------------------------ losses (csrc/kp_loss.hip)
MAX_ENTRIES = 2 ** 31 - 1
_sizeof = C.sizeof


def positive_threshold(sigma: float, cutoff: float = 3.0) -> float:
    """The ``pos_threshold`` that fits targets built from sub-pixel vertices: ``gaussian_table(sigma, cutoff)[128]``.  ``vk_kp_targets``
    rounds a vertex to 1/16 pixel, so the nearest pixel centre is at most 8 sixteenths away per axis and its squared distance D is at
    most 128: with this threshold every vertex has between one and four positive pixels wherever it lies inside its pixel.  Needs
    16 * cutoff * sigma >= 12, so that D = 128 lies inside the disc."""
    if not 16.0 * float(cutoff) * float(sigma) >= 12.0:
        raise ValueError("positive_threshold: 16 * cutoff * sigma = %g is below 12: the pixel nearest to a vertex can lie outside the disc"
                         % (16.0 * float(cutoff) * float(sigma)))
    return float(gaussian_table(sigma, cutoff)[128])


def _planes(planes, who):
    if isinstance(planes, (int, np.integer)) and not isinstance(planes, bool):
        planes = (int(planes),)
    try:
        out = [int(p) for p in planes]
        ok = bool(out) and all(float(p) == int(p) and not isinstance(p, bool) for p in planes)
    except (TypeError, ValueError):
        out, ok = [], False
    if not ok or min(out) < 0 or max(out) >= _lossfn.MAX_CLASSES or len(set(out)) != len(out):
        raise ValueError("%s: planes must name distinct planes in [0, %d), got %r" % (who, _lossfn.MAX_CLASSES, planes))
    return tuple(sorted(out))


def _mask(planes) -> int:
    return sum(1 << p for p in planes)


class _KpAlgebra:
    """``w * term``, ``term + term`` and ``seg + term`` build a ``vk.keypoints.LossSum``."""

    def _as_kp_sum(self) -> "LossSum":
        raise NotImplementedError

    def __add__(self, other):
        if isinstance(other, (int, float)) and not isinstance(other, bool) and other == 0:
            return self._as_kp_sum()                    # sum([...]) starts from 0
        me = self._as_kp_sum()
        if isinstance(other, lovasz._LovaszAlgebra):
            raise ValueError("a Lovasz term cannot join a vk.keypoints sum: the fused step runs one second part beside vk_seg_loss")
        if isinstance(other, _KpAlgebra):
            o = other._as_kp_sum()
            if me.heat is not None and o.heat is not None:
                raise ValueError("two heat terms in one sum: a sum holds at most one HeatmapFocalLoss")
            if me.bce is not None and o.bce is not None:
                raise ValueError("two plane BCE terms in one sum: a sum holds at most one PlaneBCE")
            seg = me.seg if o.seg is None else o.seg if me.seg is None else me.seg + o.seg
            return LossSum(seg, me.heat or o.heat, me.bce or o.bce)
        if not isinstance(other, seglosses._Algebra):
            return NotImplemented
        return LossSum(other._as_sum() if me.seg is None else me.seg + other, me.heat, me.bce)

    __radd__ = __add__

    def __mul__(self, w):
        w = seglosses._weight(w)
        if w is None:
            return NotImplemented
        me = self._as_kp_sum()
        return LossSum(None if me.seg is None else w * me.seg, None if me.heat is None else (w * me.heat[0], me.heat[1]),
                       None if me.bce is None else (w * me.bce[0], me.bce[1]))

    __rmul__ = __mul__


class _KpTerm(_KpAlgebra, nn.Module):
    def __init__(self):
        super().__init__()
        self._sum = None

    def forward(self, y_pred, y_true):
        if self._sum is None:
            object.__setattr__(self, "_sum", self._as_kp_sum())         # keeps the workspace cache; not a submodule (no cycle)
        return self._sum(y_pred, y_true)

    def cfg(self, C: int):
        return self._as_kp_sum().kp_cfg(C)


class HeatmapFocalLoss(_KpTerm):
    """CornerNet's penalty-reduced focal loss on the planes ``planes`` of logits [N, C, H, W] against a heatmap target in [0, 1]: an
    entry is positive iff y >= ``pos_threshold``; positive -(1 - p)^alpha log p, negative -(1 - y)^beta p^alpha log(1 - p); per plane
    the sum over (N, H, W) divided by max(number of positives, 1); the mean over the planes.  ``alpha``, ``beta``: integers in 0..8.
    The default ``pos_threshold`` 1.0 fits integer vertices only (a vertex off the pixel grid has no entry equal to 1): use
    ``positive_threshold(sigma)`` for the targets of ``make_targets``."""

    def __init__(self, planes=(1,), alpha: int = 2, beta: int = 4, pos_threshold: float = 1.0):
        super().__init__()
        self.planes = _planes(planes, "HeatmapFocalLoss")
        for name, v in (("alpha", alpha), ("beta", beta)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= L.VK_KP_LOSS_MAX_EXP:
                raise ValueError("HeatmapFocalLoss: %s must be an integer in 0..%d, got %r" % (name, L.VK_KP_LOSS_MAX_EXP, v))
        if isinstance(pos_threshold, bool) or not isinstance(pos_threshold, (int, float)) or not 0.0 < float(pos_threshold) <= 1.0:
            raise ValueError("HeatmapFocalLoss: pos_threshold must lie in (0, 1], got %r" % (pos_threshold,))
        self.alpha, self.beta, self.pos_threshold = int(alpha), int(beta), float(pos_threshold)

    def _as_kp_sum(self):
        return LossSum(None, (1.0, self), None)

    def extra_repr(self):
        return "planes=%r, alpha=%d, beta=%d, pos_threshold=%r" % (self.planes, self.alpha, self.beta, self.pos_threshold)


class PlaneBCE(_KpTerm):
    """``torch.nn.BCEWithLogitsLoss(pos_weight)`` on the planes ``planes`` only: the mean over their N H W len(planes) entries.
    ``pos_weight``: None, one positive number for every plane, or one per plane in the order of ``planes`` as given."""

    def __init__(self, planes=(0,), pos_weight=None):
        super().__init__()
        self.planes = _planes(planes, "PlaneBCE")
        given = [int(planes)] if isinstance(planes, (int, np.integer)) else [int(p) for p in planes]
        pw = seglosses._pos_weight_list(pos_weight, "PlaneBCE")
        if pw is not None:
            if len(pw) not in (1, len(given)):
                raise ValueError("PlaneBCE: pos_weight holds %d values for %d planes" % (len(pw), len(given)))
            if not all(v > 0.0 for v in pw):
                raise ValueError("PlaneBCE: pos_weight must be positive, got %r" % (pw,))
            pw = dict(zip(given, pw * (len(given) if len(pw) == 1 else 1)))
        self.pos_weight = pw

    def _as_kp_sum(self):
        return LossSum(None, None, (1.0, self))

    def extra_repr(self):
        return "planes=%r, pos_weight=%r" % (self.planes, self.pos_weight)


class LossSum(seglosses._Front, _KpAlgebra, nn.Module):
    """``seg`` (a ``vk.seglosses`` term or sum of mode binary or multilabel, or None) + ``w_heat`` * a ``HeatmapFocalLoss`` +
    ``w_bce`` * a ``PlaneBCE``: at most one of each, at least one of the two, on planes that do not overlap.  The module form runs
    ``vk_seg_loss`` and ``vk_kp_loss`` through one autograd function; ``Unet.loss_and_backward(loss=...)`` runs ``vk_unet_loss_kp``.
    ``last_components``: device tensor [total, pix, focal, dice, jaccard, tversky, mcc, heat, plane_bce] of the last call (unweighted
    term values; no host sync).  An ``ignore_index`` of the ``vk.seglosses`` part applies to that part alone."""

    def __init__(self, seg, heat, bce):
        super().__init__()
        for name, part, cls in (("heat", heat, HeatmapFocalLoss), ("bce", bce, PlaneBCE)):
            if part is None:
                continue
            if not (isinstance(part, tuple) and len(part) == 2 and isinstance(part[1], cls)):
                raise TypeError("vk.keypoints.LossSum: %s must be None or (weight, %s)" % (name, cls.__name__))
            if seglosses._weight(part[0]) is None:
                raise TypeError("vk.keypoints.LossSum: the weight must be a number")
        if heat is None and bce is None:
            raise ValueError("vk.keypoints.LossSum: neither a HeatmapFocalLoss nor a PlaneBCE")
        if heat is not None and bce is not None and set(heat[1].planes) & set(bce[1].planes):
            raise ValueError("LossSum: HeatmapFocalLoss and PlaneBCE overlap on plane(s) %r"
                             % (sorted(set(heat[1].planes) & set(bce[1].planes)),))
        if seg is not None:
            if isinstance(seg, lovasz._LovaszAlgebra):
                raise ValueError("a sum with a Lovasz term cannot join a vk.keypoints sum: the fused step runs one second part beside "
                                 "vk_seg_loss")
            if not isinstance(seg, seglosses._Algebra):
                raise TypeError("vk.keypoints.LossSum: seg must be a vk.seglosses term or sum, got %s" % type(seg).__name__)
            seg = seglosses.LossSum(seg._as_sum().terms)                 # a copy
            if seg.mode == "multiclass":
                raise ValueError("LossSum: the vk.seglosses part is of mode 'multiclass'; the keypoint terms are per-plane sigmoid losses "
                                 "and join a binary or multilabel sum only")
        self.seg = seg
        self.heat = None if heat is None else (float(heat[0]), heat[1])
        self.bce = None if bce is None else (float(bce[0]), bce[1])
        self._mods = nn.ModuleList([p[1] for p in (self.heat, self.bce) if p is not None])
        self.mode = None if seg is None else seg.mode
        self.ignore_index = None if seg is None else seg.ignore_index
        self.last_components: Optional[torch.Tensor] = None
        self._ws = {}

    def _as_kp_sum(self):
        return self

    def resolved_mode(self, C: int) -> str:
        if self.seg is not None:
            return self.seg.resolved_mode(C)
        return _lossfn.check_classes("binary" if C == 1 else "multilabel", C)

    def check_shapes(self, logits: torch.Tensor, target: torch.Tensor) -> str:
        mode = super().check_shapes(logits, target)
        self.kp_cfg(int(logits.shape[1]))                    # the planes against C, before anything is asked of the device
        return mode

    def kp_cfg(self, C: int) -> "L.vk_kp_loss_cfg":
        """The ``vk_kp_loss_cfg`` of this sum for logits with C planes."""
        self.resolved_mode(C)
        c = L.vk_kp_loss_cfg()
        c.struct_size = _sizeof(L.vk_kp_loss_cfg)
        c.alpha, c.beta, c.pos_threshold = 2, 4, 1.0
        for name, part in (("HeatmapFocalLoss", self.heat), ("PlaneBCE", self.bce)):
            if part is not None and max(part[1].planes) >= C:
                raise ValueError("%s(planes=%r) names a plane >= C = %d" % (name, part[1].planes, C))
        if self.heat is not None:
            w, t = self.heat
            c.heat_planes, c.w_heat, c.alpha, c.beta, c.pos_threshold = _mask(t.planes), w, t.alpha, t.beta, t.pos_threshold
        if self.bce is not None:
            w, t = self.bce
            c.bce_planes, c.w_bce = _mask(t.planes), w
            if t.pos_weight is not None:
                c.has_pos_weight = 1
                for i in range(16):
                    c.pos_weight[i] = t.pos_weight.get(i, 1.0)
        return c

    def seg_cfg(self, C: int):
        return None if self.seg is None else self.seg.cfg(C)

    def workspace(self, N: int, C: int, HW: int, device) -> torch.Tensor:
        """the device scratch of vk_kp_loss for this shape (cached per shape)"""
        if N * C * HW > MAX_ENTRIES:
            raise VkError("vk.keypoints.LossSum: %d logits in one call, at most 2^31 - 1" % (N * C * HW))
        key = (N, C, HW, str(device))
        ws = self._ws.get(key)
        if ws is None:
            nbytes = L.lib().vk_kp_loss_workspace_bytes(N, C, HW)
            if nbytes == 0:
                raise VkError("vk_kp_loss_workspace_bytes refuses N=%d C=%d HW=%d" % (N, C, HW))
            ws = self._ws[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
        return ws

    def _run(self, x, y, dl):
        N, Cc, H, W = x.shape
        HW = H * W
        kcfg = self.kp_cfg(Cc)
        lib = L.lib()
        st = L.current_stream()
        out = torch.zeros(16, dtype=torch.float32, device=x.device)
        if self.seg is not None:
            sws = torch.empty(lib.vk_seg_loss_workspace_bytes(N, Cc, HW), dtype=torch.uint8, device=x.device)
            L.check(lib.vk_seg_loss(self.seg.cfg(Cc), N, Cc, HW, x.data_ptr(), y.data_ptr(), sws.data_ptr(), sws.numel(), out.data_ptr(),
                                    L.ptr(dl), 1.0, st), "vk_seg_loss")
        ws = self.workspace(N, Cc, HW, x.device)
        L.check(lib.vk_kp_loss(kcfg, N, Cc, HW, x.data_ptr(), y.data_ptr(), ws.data_ptr(), ws.numel(), out[8:].data_ptr(), None, L.ptr(dl),
                               1.0, 1 if self.seg is not None else 0, st), "vk_kp_loss")
        total = out[0] + out[8]
        self.last_components = torch.cat([total.reshape(1), out[1:6], out[7:8], out[9:11]])
        return total, None

    def extra_repr(self):
        return "w_heat=%r, w_bce=%r" % (None if self.heat is None else self.heat[0], None if self.bce is None else self.bce[0])
