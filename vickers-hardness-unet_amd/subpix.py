"""Sub-pixel vertex refinement of the indentation fit (csrc/subpix.hip, ``vk_subpix_refine``).

The geometry records carry int32 corners, so a diagonal is quantised to one map pixel at either tip: on a letterboxed 512 x 512 map
of a 3072 x 2048 micrograph that is six source pixels, 0.5 - 1 % of a typical diagonal and twice that in HV.  The probability map the
fit was made from is still on the device and holds the edge to a fraction of a pixel::

    pred = vk.instances.detect(prob, fit="quad")
    fine = vk.subpix.refine(pred, prob, method="lines", affine=vk.subpix.letterbox_affine(h, w, 512, "centered"))
    fine.records()[0]["d_mean"]                                  # in source-image pixels, float64
    vk.instances.match(vk.subpix.refine(pred, prob), vk.subpix.refine(gt, mask.float()))       # plugs into the matching unchanged
    vk.ObjectMetrics(fit="quad", refine=dict(method="lines"))    # says whether it helped on a validation set

Two estimators, because they fail in opposite directions: ``"corner"``, the gradient-orthogonality iteration
(pulled inward as the edge ramp widens), and ``"lines"``, the intersection of the two sides fitted through their level crossings
(unbiased under blur, but assumes straight sides near the tip).  IEEE float64 in a fixed order: the same bytes on every run.  CUDA
tensors only: there is no CPU fallback."""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib as L
from . import geometry as G
from . import prepost as PP
from ._lib import VkError

__all__ = ["FLAGS", "RECORD_DTYPE", "RefinedDetections", "corner_weights", "letterbox_affine", "params", "postprocess", "refine"]

FLAGS = dict(L.SUBPIX_FLAGS)
RECORD_DTYPE = np.dtype(L.vk_subpix_quad)
_METHODS = {"corner": L.VK_SUBPIX_CORNER, "lines": L.VK_SUBPIX_LINES}
_CORNER_DEFAULTS = dict(win=5, zero_zone=-1, max_iter=40, eps=1e-3)
_LINES_DEFAULTS = dict(lo=0.1, hi=0.5, n_stations=12, reach=6, level=None, max_shift=None)


def corner_weights(win: int) -> List[float]:
    """wt[k] = exp(-((k - win) / win)^2), k = 0 .. 2 win, in float64: the method's only transcendental stays on the host."""
    return [math.exp(-(((k - win) / win) * ((k - win) / win))) for k in range(2 * win + 1)]


def params(method: str = "corner", default_level: float = G.BIN_THRESH, **kw) -> L.vk_subpix_params:
    """The parameter block of one call.  corner: ``win`` 2..15 (5), ``zero_zone`` -1..win-1 (-1 = none), ``max_iter`` 1..100 (40),
    ``eps`` (1e-3).  lines: ``lo``, ``hi`` (0.1, 0.5), ``n_stations`` 3..32 (12), ``reach`` 1..15 (6), ``level`` (the detection
    threshold), ``max_shift`` (reach).  The ranges themselves are checked by the library."""
    if method not in _METHODS:
        raise ValueError("method must be 'corner' or 'lines', got %r" % (method,))
    defaults = _CORNER_DEFAULTS if method == "corner" else _LINES_DEFAULTS
    unknown = set(kw) - set(defaults)
    if unknown:
        raise ValueError("unknown %s parameter(s) %s; known: %s" % (method, sorted(unknown), sorted(defaults)))
    v = dict(defaults, **kw)
    p = L.vk_subpix_params()
    p.method = _METHODS[method]
    if method == "corner":
        p.win, p.zero_zone, p.max_iter, p.eps = int(v["win"]), int(v["zero_zone"]), int(v["max_iter"]), float(v["eps"])
        if 2 <= p.win <= L.VK_SUBPIX_MAX_WIN:
            for k, wk in enumerate(corner_weights(p.win)):
                p.wt[k] = wk
    else:
        p.n_stations, p.reach, p.lo, p.hi = int(v["n_stations"]), int(v["reach"]), float(v["lo"]), float(v["hi"])
        p.level = float(default_level if v["level"] is None else v["level"])
        p.max_shift = float(p.reach if v["max_shift"] is None else v["max_shift"])
    return p


def letterbox_affine(h: int, w: int, size: int, geometry="centered") -> np.ndarray:
    """float64 [3] = (ox, oy, inv_scale) of an h x w image letterboxed into size x size: a map coordinate (x, y) is the source
    coordinate ((x - ox) * inv_scale, (y - oy) * inv_scale).  ``geometry``: a convention of ``prepost.letterbox_geometry`` or the tuple
    it returns (scale, nh, nw, top, left)."""
    geo = PP.letterbox_geometry(int(h), int(w), int(size), geometry) if isinstance(geometry, str) else tuple(geometry)
    scale, _, _, top, left = geo
    return np.array([float(left), float(top), 1.0 / float(scale)], np.float64)


class RefinedDetections(G.Detections):
    """``Detections`` whose ``raw`` holds ``vk_subpix_quad`` records [B, max_components, 200] (``RECORD_DTYPE``): the refined vertices
    ``v`` (map coordinates) and ``vs`` (source coordinates), per-vertex ``flags`` and ``iters``, and the diagonals in source pixels.
    ``clean``, ``counts`` and ``slots`` are the source's own tensors, so it goes to ``vk.instances.match`` as it is."""

    def __init__(self, source: G.Detections, raw: torch.Tensor, method: str):
        super().__init__(source.fit, source.clean, raw, source.counts, source.slots, source.max_components)
        self.source, self.method = source, method

    @property
    def record_dtype(self) -> np.dtype:
        return RECORD_DTYPE

    @property
    def diag_offset(self) -> int:
        return int(L.vk_subpix_quad.d_mean.offset)


def _affine_tensor(affine, B: int, device) -> Optional[torch.Tensor]:
    if affine is None:
        return None
    if isinstance(affine, torch.Tensor):
        a = affine.detach().to(device=device, dtype=torch.float64)
    else:
        a = torch.from_numpy(np.ascontiguousarray(np.asarray(affine, np.float64))).to(device)
    if a.dim() == 1 and a.numel() == 3:
        a = a.reshape(1, 3).expand(B, 3)
    if tuple(a.shape) != (B, 3):
        raise ValueError("affine must be (ox, oy, inv_scale) or one such row per map [%d, 3], got %s" % (B, tuple(a.shape)))
    return a.contiguous()


def refine(dets: G.Detections, prob: torch.Tensor, method: str = "corner", affine=None, **kw) -> RefinedDetections:
    """Refines the four corners of every record of ``dets`` on ``prob``, the float32 [B, h, w] map ``dets`` was detected on.  No host
    synchronisation.  ``affine``: None, (ox, oy, inv_scale) or one row per map (``letterbox_affine``); the diagonals and ``vs`` are then
    in source-image pixels.  Keyword parameters as in ``params``; ``level`` defaults to the fit's detection threshold."""
    if not isinstance(dets, G.Detections) or isinstance(dets, RefinedDetections):
        raise ValueError("expected the Detections of vk.instances.detect")
    if dets.slots is None:
        raise ValueError("refinement needs the slot map: these Detections were made with detect(slots=False)")
    if not isinstance(prob, torch.Tensor) or prob.dim() != 3:
        raise ValueError("expected a float32 tensor [B, h, w]")
    if not prob.is_cuda or not dets.raw.is_cuda:
        raise VkError("probability maps are on %s: this package runs on an MI355X only and has no CPU fallback" % prob.device)
    if tuple(prob.shape) != tuple(dets.slots.shape) or prob.device != dets.raw.device:
        raise ValueError("the map %s is not the one the detections %s were made from" % (tuple(prob.shape), tuple(dets.slots.shape)))
    p = params(method, G._fit(dets.fit).bin_thresh, **kw)
    prob = prob.detach().contiguous().float()
    B, h, w = (int(v) for v in prob.shape)
    aff = _affine_tensor(affine, B, prob.device)
    out = G._record_buffer((B, dets.max_components), RECORD_DTYPE.itemsize, prob.device, zero=True)
    L.check(L.lib().vk_subpix_refine(C.byref(p), B, h, w, prob.data_ptr(), dets.raw.data_ptr(), dets.record_bytes, dets.box_offset,
                                     dets.valid_offset, dets.counts.data_ptr(), dets.max_components, L.ptr(aff), out.data_ptr(),
                                     L.current_stream()), "vk_subpix_refine")
    return RefinedDetections(dets, out, method)


def postprocess(prob: torch.Tensor, fit: str = "rect", method: str = "corner", affine=None, refine_args: Optional[Dict] = None,
                **detect_args) -> Tuple[torch.Tensor, List[List[Dict]]]:
    """``prob`` float32 [B, h, w] on the device -> (clean uint8 [B, h, w] on the device, per map the detection list of
    ``postprocess_minarearect_multi`` / ``postprocess_quadrilateral_multi``, sorted by area) with ``d1``, ``d2``, ``d_mean`` refined
    (source pixels when ``affine`` is given), ``box_subpix`` float64 [4, 2] (``vs``), ``box_subpix_map`` (``v``) and ``subpix_flags``
    [4] added; ``box`` stays the int32 fit.  ``detect_args`` go to ``vk.instances.detect``, ``refine_args`` to ``refine``."""
    dets = G.detect(prob, fit=fit, **detect_args)
    fine = refine(dets, prob, method=method, affine=affine, **(refine_args or {}))
    counts = dets.counts.cpu().numpy()                    # synchronises; read once for both record lists
    out = []
    for coarse, recs in zip(dets.records(counts), fine.records(counts)):
        by_label = dict(zip(recs["label"].tolist(), recs))          # a refined record carries its source's label, unique within a map
        rows = G._fit(fit).to_dicts(coarse)               # sorted by area; without the quadrilateral records of valid == 0
        for d in rows:
            r = by_label[d["label"]]
            d.update(d1=float(r["d1"]), d2=float(r["d2"]), d_mean=float(r["d_mean"]), box_subpix=r["vs"].reshape(4, 2).copy(),
                     box_subpix_map=r["v"].reshape(4, 2).copy(), subpix_flags=r["flags"].copy())
        out.append(rows)
    return dets.clean, out
