"""Second-pass inference on one window per indentation (csrc/zoom.hip).

The letterboxed map of a 3072 x 2048 micrograph shows an indentation six times coarser than the camera recorded it, and sub-pixel
refinement cannot recover what the network never saw.  Here the first pass only finds the indentations; every one of them is then cut
from the uint8 source image into a window of its own, at the finest scale that still shows it whole, and segmented, fitted and
refined there::

    prob = torch.sigmoid(model(x))[:, 0]                                  # the letterboxed first pass, [B, S, S]
    dets = vk.geometry.detect(prob, fit="quad")
    aff = vk.subpix.letterbox_affine(h, w, 512, "centered")
    fine = vk.zoom.refine_detections(model, [img_u8], dets, prob, affine=aff)     # a RefinedDetections, in source pixels
    vk.instances.match(fine, refined_gt)                                  # plugs into the matching unchanged
    vk.Segmenter(model).measure(img_bgr)                                  # all of it, one image -> the detection list

Three kernels: ``vk_zoom_windows`` (the windows, on the device, from the records), ``vk_zoom_gather`` (an antialiased gather into
normalised network inputs: bilinear below scale 1, the area average above) and ``vk_zoom_merge`` (the second pass's record replaces
the first pass's only where it is found, refined without a failure flag and agrees with it; otherwise today's answer stays).  One
host synchronisation: the number of windows sizes the model batch.  What a trained model gains from the second pass is not measured
anywhere in this repository: this module is the mechanism and ``vk.instances.match`` the means to measure it.  CUDA tensors only."""
from __future__ import annotations

import ctypes as C
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from . import geometry as G
from . import subpix as SP
from ._lib import VkError

__all__ = ["STATUS", "WINDOW_DTYPE", "ZoomedDetections", "gather", "measure", "merge", "postprocess", "refine_detections", "window_affine",
           "windows"]

STATUS = dict(L.ZOOM_STATUS)
WINDOW_DTYPE = np.dtype(L.vk_zoom_window)


def _sizes_tensor(sizes, B: int, device) -> torch.Tensor:
    t = sizes if isinstance(sizes, torch.Tensor) else torch.as_tensor(np.asarray(sizes, np.int32))
    t = t.to(device=device, dtype=torch.int32).reshape(-1, 2)
    if t.shape[0] == 1 and B > 1:
        t = t.expand(B, 2)
    if tuple(t.shape) != (B, 2):
        raise ValueError("sizes must be (h, w) or one such row per map [%d, 2], got %s" % (B, tuple(t.shape)))
    return t.contiguous()


def windows(dets: G.Detections, sizes, affine=None, S: int = 512, margin: float = 1.5, s_min: float = 1.0, s_max: float = 32.0,
            max_windows: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """One window per valid record of ``dets`` -> (records uint8 [max_windows, 40] (``WINDOW_DTYPE``), count int32 [1]), both on the
    device, in ascending (map, slot) order; no host synchronisation.  ``sizes``: (h, w) of the source images, one row per map;
    ``affine``: the first pass's (ox, oy, inv_scale) as in ``vk.subpix.refine``.  The window shows the indentation's bounding square
    enlarged by ``margin`` on S output pixels, at a scale clamped to [s_min, s_max] source pixels per output pixel."""
    if not isinstance(dets, G.Detections) or isinstance(dets, SP.RefinedDetections):
        raise ValueError("expected the Detections of vk.geometry.detect")
    if not dets.raw.is_cuda:
        raise VkError("the detections are on %s: this package runs on an MI355X only and has no CPU fallback" % dets.raw.device)
    dev = dets.raw.device
    B, M = int(dets.raw.shape[0]), dets.max_components
    cap = min(B * M, 65535) if max_windows is None else int(max_windows)
    p = L.vk_zoom_params(int(S), cap, float(margin), float(s_min), float(s_max))
    aff = SP._affine_tensor(affine, B, dev)
    sz = _sizes_tensor(sizes, B, dev)
    out = G._record_buffer((max(min(cap, 65535), 1),), WINDOW_DTYPE.itemsize, dev, zero=True)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    L.check(L.lib().vk_zoom_windows(C.byref(p), B, dets.raw.data_ptr(), dets.record_bytes, dets.box_offset, dets.valid_offset,
                                    dets.counts.data_ptr(), M, L.ptr(aff), sz.data_ptr(), out.data_ptr(), count.data_ptr(),
                                    L.current_stream()), "vk_zoom_windows")
    return out, count


def window_affine(win: torch.Tensor) -> torch.Tensor:
    """The window records -> float64 [n, 3] = (ox, oy, inv_scale) rows for ``vk.subpix.refine``, on the device without a read-back:
    inv_scale = s, ox = -((X0 + 0.5 s) - 0.5) / s, oy alike."""
    f = win.reshape(-1).view(torch.float64).reshape(-1, 5)
    X0, Y0, s = f[:, 2], f[:, 3], f[:, 4]
    half = s * 0.5
    return torch.stack([-((X0 + half) - 0.5) / s, -((Y0 + half) - 0.5) / s, s], dim=1).contiguous()


def _image_table(images: Sequence[torch.Tensor]):
    tab = (L.vk_zoom_image * len(images))()
    for i, im in enumerate(images):
        if not isinstance(im, torch.Tensor) or im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3:
            raise ValueError("image %d: expected a uint8 BGR tensor [h, w, 3]" % i)
        if not im.is_cuda:
            raise VkError("image %d is on %s: this package runs on an MI355X only and has no CPU fallback" % (i, im.device))
        if im.stride(2) != 1 or im.stride(1) != 3:
            raise ValueError("image %d: pixels must be contiguous (only the row stride is free), got strides %s" % (i, tuple(im.stride())))
        tab[i] = L.vk_zoom_image(im.data_ptr(), int(im.shape[0]), int(im.shape[1]), int(im.stride(0)))
    return tab


def gather(images: Sequence[torch.Tensor], win: torch.Tensor, n: int, S: int = 512, pad_value: int = 0, flags: int = 0) -> torch.Tensor:
    """The first ``n`` windows cut from ``images`` (uint8 BGR tensors [h, w, 3] on the device, each its own tensor, rows may be padded)
    -> float32 [n, 3, S, S], normalised as ``vk.prepost.preprocess`` does.  ``flags``: ``VK_ZOOM_STAGED`` (diagnostic)."""
    images = list(images)
    tab = _image_table(images)
    dev = win.device
    x = torch.empty(int(n), 3, int(S), int(S), dtype=torch.float32, device=dev)
    tab_dev = torch.empty(max(len(images), 1) * 3, dtype=torch.int64, device=dev)
    L.check(L.lib().vk_zoom_gather(int(n), int(S), win.data_ptr(), len(images), tab, tab_dev.data_ptr(), int(pad_value), int(flags),
                                   x.data_ptr(), L.current_stream()), "vk_zoom_gather")
    return x


class ZoomedDetections(SP.RefinedDetections):
    """A ``RefinedDetections`` whose records are the second pass's where it was accepted and the first pass's coarse refinement
    elsewhere (``vs`` and the diagonals are source pixels either way; ``v`` is in the coordinates of the map the record was refined on).
    ``clean``, ``counts`` and ``slots`` are the first pass's.  ``status`` int32 [B, max_components]: one of ``STATUS`` zoomed /
    no_target / refine_failed / disagrees / no_window, or-ed with the window's clipped / scale_clamped_* bits; ``scale`` float64
    [B, max_components]: the window's source pixels per map pixel (0 without a window).  ``second``: the second pass's intermediate
    results (windows, count, inputs, probabilities, detections, refinement), for diagnosis."""

    def __init__(self, source: G.Detections, raw: torch.Tensor, method: str, status: torch.Tensor, scale: torch.Tensor,
                 coarse: SP.RefinedDetections, second: Dict):
        super().__init__(source, raw, method)
        self.status, self.scale, self.coarse, self.second = status, scale, coarse, second


def _segment_chunks(segment: Callable, x: torch.Tensor, batch: int) -> torch.Tensor:
    """logits [n, S, S] of channel 0: ``segment`` sees chunks of exactly ``batch`` inputs, the last one filled with zero tiles."""
    n, S = int(x.shape[0]), int(x.shape[-1])
    logits = torch.empty(n, S, S, dtype=torch.float32, device=x.device)
    for i in range(0, n, batch):
        chunk = x[i:i + batch]
        k = int(chunk.shape[0])
        if k < batch:
            chunk = torch.cat([chunk, x.new_zeros(batch - k, *x.shape[1:])])
        lg = segment(chunk)
        if lg.dim() != 4 or int(lg.shape[0]) != batch or tuple(lg.shape[2:]) != (S, S):
            raise ValueError("segment must map [%d, 3, %d, %d] to logits [%d, C, %d, %d], got %s" % (batch, S, S, batch, S, S, tuple(lg.shape)))
        logits[i:i + k] = lg[:k, 0].float()
    return logits


def merge(win: torch.Tensor, n: int, dets2: Optional[G.Detections], fine2: Optional[SP.RefinedDetections], coarse: SP.RefinedDetections,
          S: int, agree: float = 0.25) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``vk_zoom_merge`` -> (records uint8 [B, max_components, 200], status int32 [B, max_components], scale float64 alike)."""
    src = coarse.source
    B, M = int(coarse.raw.shape[0]), coarse.max_components
    dev = coarse.raw.device
    out = G._record_buffer((B, M), SP.RECORD_DTYPE.itemsize, dev, zero=True)
    status = torch.empty(B, M, dtype=torch.int32, device=dev)
    scale = torch.empty(B, M, dtype=torch.float64, device=dev)
    if n > 0:
        second = (dets2.raw.data_ptr(), dets2.record_bytes, dets2.box_offset, dets2.valid_offset, dets2.counts.data_ptr(),
                  dets2.max_components, fine2.raw.data_ptr())
    else:
        second = (0, 0, 0, -1, 0, 0, 0)
    L.check(L.lib().vk_zoom_merge(int(S), float(agree), int(n), win.data_ptr(), *second, B, M, src.counts.data_ptr(), coarse.raw.data_ptr(),
                                  out.data_ptr(), status.data_ptr(), scale.data_ptr(), L.current_stream()), "vk_zoom_merge")
    return out, status, scale


def refine_detections(segment: Callable, images: Sequence[torch.Tensor], dets: G.Detections, prob: torch.Tensor, affine=None,
                      S: int = 512, fit: Optional[str] = None, method: str = "corner", batch: int = 16, agree: float = 0.25,
                      max_components2: int = 8, pad_value: int = 0, window_args: Optional[Dict] = None,
                      detect_args: Optional[Dict] = None, refine_args: Optional[Dict] = None) -> ZoomedDetections:
    """The whole second pass.  ``segment``: a ``vk.Unet`` in eval mode or any callable [k, 3, S, S] -> logits [k, C, S, S] (channel 0 is
    used), called in chunks of exactly ``batch``.  ``images``: one uint8 BGR device tensor per map of ``dets``; ``prob``: the float32
    [B, h, w] map ``dets`` was detected on; ``affine``: its letterbox rows.  ``fit`` (default: the first pass's), ``detect_args`` and
    ``max_components2`` go to the second ``vk.geometry.detect``; ``method`` and ``refine_args`` to both ``vk.subpix.refine`` calls;
    ``window_args`` (margin, s_min, s_max, max_windows) to ``windows``."""
    images = list(images)
    B = int(dets.raw.shape[0])
    if len(images) != B:
        raise ValueError("%d images for %d maps" % (len(images), B))
    if batch < 1:
        raise ValueError("batch must be positive")
    fit = dets.fit if fit is None else fit
    G._fit(fit)
    rargs = dict(refine_args or {})
    with torch.no_grad():
        coarse = SP.refine(dets, prob, method=method, affine=affine, **rargs)
        _image_table(images)                                      # argument errors before anything is launched
        sizes = [[int(im.shape[0]), int(im.shape[1])] for im in images]
        win, count = windows(dets, sizes, affine, S, **(window_args or {}))
        n = int(count.item())                                     # the module's only synchronisation: it sizes the model batch
        second: Dict = dict(windows=win, count=count, n=n, x=None, prob=None, dets=None, fine=None)
        dets2 = fine2 = None
        if n > 0:
            x = gather(images, win, n, S, pad_value)
            prob2 = torch.sigmoid(_segment_chunks(segment, x, int(batch)))
            dets2 = G.detect(prob2, fit=fit, max_components=int(max_components2), **(detect_args or {}))
            fine2 = SP.refine(dets2, prob2, method=method, affine=window_affine(win)[:n], **rargs)
            second.update(x=x, prob=prob2, dets=dets2, fine=fine2)
        raw, status, scale = merge(win, n, dets2, fine2, coarse, S, agree)
    return ZoomedDetections(dets, raw, method, status, scale, coarse, second)


def _lists(dets: G.Detections, fine: SP.RefinedDetections, fit: str) -> List[List[Dict]]:
    """The detection lists of ``vk.subpix.postprocess`` from a first pass and its refined records (``zoom_status`` / ``zoom_scale``
    added when ``fine`` is a ``ZoomedDetections``)."""
    counts = dets.counts.cpu().numpy()
    zoomed = isinstance(fine, ZoomedDetections)
    status = fine.status.cpu().numpy() if zoomed else None
    scale = fine.scale.cpu().numpy() if zoomed else None
    out = []
    for b, (coarse, recs) in enumerate(zip(dets.records(counts), fine.records(counts))):
        by_label = {int(r["label"]): (s, r) for s, r in enumerate(recs)}
        rows = G._fit(fit).to_dicts(coarse)
        for d in rows:
            s, r = by_label[d["label"]]
            d.update(d1=float(r["d1"]), d2=float(r["d2"]), d_mean=float(r["d_mean"]), box_subpix=r["vs"].reshape(4, 2).copy(),
                     box_subpix_map=r["v"].reshape(4, 2).copy(), subpix_flags=r["flags"].copy())
            if zoomed:
                d.update(zoom_status=int(status[b, s]), zoom_scale=float(scale[b, s]))
        out.append(rows)
    return out


def postprocess(segment: Callable, images: Sequence[torch.Tensor], prob: torch.Tensor, fit: str = "rect", method: str = "corner",
                affine=None, S: int = 512, zoom_args: Optional[Dict] = None, **detect_args) -> Tuple[torch.Tensor, List[List[Dict]]]:
    """``vk.subpix.postprocess`` with the second pass: (clean uint8 [B, h, w] on the device, per map the detection list, sorted by
    area) with ``d1``, ``d2``, ``d_mean``, ``box_subpix`` in source pixels from the zoom pass where it was accepted, and
    ``zoom_status`` / ``zoom_scale`` added per row.  ``detect_args`` go to the first ``vk.geometry.detect``, ``zoom_args`` to
    ``refine_detections``."""
    dets = G.detect(prob, fit=fit, **detect_args)
    fine = refine_detections(segment, images, dets, prob, affine=affine, S=S, method=method, **(zoom_args or {}))
    return dets.clean, _lists(dets, fine, fit)


def _measure(seg, img_bgr, fit: str, zoom: bool, method: str, **kw):
    """The steps of ``measure`` -> (the image on the device, the letterbox metadata, the logits [S, S], the first pass's detections, the
    refined ones)."""
    from . import prepost as PP
    heatmap = method == "heatmap"         # vk.keypoints: the vertices from plane 1 of a two-plane model, in place of vk.subpix
    if heatmap:
        if zoom:
            raise ValueError("method='heatmap' needs zoom=False: the zoom pass with a heatmap read-out is not implemented")
        classes = getattr(seg.model, "classes", None)
        if isinstance(classes, int) and classes < 2:
            raise ValueError("method='heatmap' needs a model with a mask plane and a heatmap plane, this one has %d plane(s)" % classes)
    src = PP._as_device_u8(img_bgr, seg.device)
    h, w = int(src.shape[0]), int(src.shape[1])
    size = int(seg.img_size)
    with torch.no_grad():
        x, meta = PP.preprocess(src, size, "centered", seg.device)
        planes = seg.model(x)
        if heatmap and planes.shape[1] < 2:
            raise ValueError("method='heatmap' needs a model with a mask plane and a heatmap plane, this one has %d plane(s)"
                             % planes.shape[1])
        logits = planes[:, 0].float()
        prob = torch.sigmoid(logits)
    dets = G.detect(prob, fit=fit)
    aff = SP.letterbox_affine(h, w, size, "centered")
    if heatmap:
        from . import keypoints as KP
        fine = KP.refine(dets, torch.sigmoid(planes[:, 1].float()), affine=aff, **(kw.get("refine_args") or {}))
    elif zoom:
        fine = refine_detections(seg.model, [src], dets, prob, affine=aff, S=size, method=method, **kw)
    else:
        fine = SP.refine(dets, prob, method=method, affine=aff, **(kw.get("refine_args") or {}))
    return src, meta, logits[0], dets, fine


def measure(seg, img_bgr, fit: str = "quad", zoom: bool = True, method: str = "corner", **kw) -> List[Dict]:
    """``Segmenter.measure``: letterbox -> model -> detect -> coarse refinement with the letterbox's affine row (-> the zoom pass) -> the
    detection list of one image in source pixels.  ``kw`` go to ``refine_detections``."""
    _, _, _, dets, fine = _measure(seg, img_bgr, fit, zoom, method, **kw)
    return _lists(dets, fine, fit)[0]
