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

Coordinates are those of the geometry records: pixel (x, y) lies at the point (x, y).  ``vk.micrographs.truth()`` uses the same
convention (its vertices are the renderer's 1/16-pixel fixed point divided by 16), so its vertices go to ``targets`` unconverted.
CUDA tensors only: there is no CPU fallback."""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Iterable, List, Optional, Tuple

import numpy as np
import torch

from . import _lib as L
from . import geometry as G
from . import instances as I
from . import subpix as SP
from ._lib import VkError

__all__ = ["FLAGS", "PEAK_DTYPE", "Peaks", "gaussian_table", "make_targets", "params", "peaks", "postprocess", "refine", "table_radius16",
           "targets", "vertex_metrics", "with_targets"]

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
