"""Host-side mirror of the reference's geometry post-processing, running on the device
through libvkunet.so (``vk_geom_minarearect`` / ``vk_geom_quadrilateral`` / ``vk_geom_slot_map``, csrc/geometry.hip):

    reference                                                        here
    ui_infer_rectangle.postprocess_minarearect_multi (:291-381) .... postprocess_minarearect_multi (one map, same return value)
                                                                     postprocess_minarearect_batch (B maps of one size, one call)
    ui_infer_quadrilateral.postprocess_minarearect_multi (:423-530)
      + robust_quadrilateral_from_contour and helpers (:262-420) .... postprocess_quadrilateral_multi / postprocess_quadrilateral_batch
                                                                     (``vk_geom_quadrilateral``: the 4-vertex fit of the newer GUI)
    (none: everything stays on the device) ......................... detect -> Detections (what vk.instances and vk.subpix work on)

The reference thresholds the probability map with numpy and hands everything else to cv2 on the CPU, one image at a time on the
GUI thread; here threshold, 3x3 open/close, 8-connected labelling with the area filter, convex hull, minimum-area rectangle,
int32 corners and the two diagonals are device kernels over the whole batch, and only the few detection records travel back.

This module is the only place that launches the geometry kernels (``_run``) and the only one that knows what differs between the
two fits (``_FITS``).  Every record layout is the ctypes structure of ``_lib``; its numpy dtype is ``np.dtype`` of that structure.
No CPU fallback: without libvkunet.so or with a CPU tensor these raise."""
from __future__ import annotations

import ctypes as C
import math
from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from ._lib import VkError

BIN_THRESH = 0.50        # ui_infer_rectangle.py:45
BIN_THRESH_QUAD = 0.45   # ui_infer_quadrilateral.py:46
MIN_AREA_FRAC = 0.0008   # ui_infer_rectangle.py:46
MORPH_KERNEL = 3
OPEN_ITER = 1
CLOSE_ITER = 1
FIT_OUTSET_PX = 2        # ui_infer_quadrilateral.py:433

_BRANCH = {0: "none", 1: "bisection", 2: "subsample", 3: "extremes"}


# ------------------------------------------------------------------------------------------------ records -> the reference's dicts
def _columns(rows: np.ndarray, *names: str):
    """The named fields of structured ``rows`` as Python ints / floats, one tuple per record (``float(np.float32)`` is exact)."""
    return zip(*(rows[n].tolist() for n in names))


def _records(rows: np.ndarray) -> List[Dict]:
    """``vk_geom_det`` rows of one map (``Detections.records()``) -> the detection list of ui_infer_rectangle.py."""
    out = [{"label": label, "area": area, "box": box.reshape(4, 2).copy(), "center": (cx, cy), "d1": d1, "d2": d2, "d_mean": d_mean,
            "size": (rw, rh), "direction": (ux, uy), "hull_vertices": hull_n}
           for box, (label, area, cx, cy, d1, d2, d_mean, rw, rh, ux, uy, hull_n)
           in zip(rows["box"], _columns(rows, "label", "area", "cx", "cy", "d1", "d2", "d_mean", "rw", "rh", "ux", "uy", "hull_n"))]
    out.sort(key=lambda r: r["area"], reverse=True)          # ui_infer_rectangle.py:379 (stable: ties keep label order)
    return out


def _quad_records(rows: np.ndarray) -> List[Dict]:
    """``vk_geom_quad`` rows of one map -> the detection list of ui_infer_quadrilateral.py."""
    out = [{"label": label, "area": area, "box": box.reshape(4, 2).copy(), "center": (cx, cy), "d1": d1, "d2": d2, "d_mean": d_mean,
            "quality": quality, "branch": _BRANCH.get(branch, "?"), "n_candidates": n_candidates, "contour_points": contour_n,
            "hull_vertices": hull_n, "flags": flags}
           for box, (valid, label, area, cx, cy, d1, d2, d_mean, quality, branch, n_candidates, contour_n, hull_n, flags)
           in zip(rows["box"], _columns(rows, "valid", "label", "area", "cx", "cy", "d1", "d2", "d_mean", "quality", "branch",
                                        "n_candidates", "contour_n", "hull_n", "flags"))
           if valid]                                         # `if quad is None: continue` (ui_infer_quadrilateral.py:498-499)
    out.sort(key=lambda r: r["area"], reverse=True)          # ui_infer_quadrilateral.py:526
    return out


# ------------------------------------------------------------------------------------------------ what differs between the two fits
class _Fit(NamedTuple):
    record: type              # the ctypes structure of one record
    dtype: np.dtype           # the same layout for numpy
    entry: str                # entry point of libvkunet.so
    takes_outset: bool        # ... which takes fit_outset_px after the descriptor
    bin_thresh: float         # the GUI's default threshold
    to_dicts: Callable[[np.ndarray], List[Dict]]


_FITS = {"rect": _Fit(L.vk_geom_det, np.dtype(L.vk_geom_det), "vk_geom_minarearect", False, BIN_THRESH, _records),
         "quad": _Fit(L.vk_geom_quad, np.dtype(L.vk_geom_quad), "vk_geom_quadrilateral", True, BIN_THRESH_QUAD, _quad_records)}


def _fit(fit) -> _Fit:
    if fit not in _FITS:
        raise ValueError("fit must be 'rect' or 'quad', got %r" % (fit,))
    return _FITS[fit]


def _record_buffer(lead: Sequence[int], rec: int, device, zero: bool = False) -> torch.Tensor:
    """uint8 [*lead, rec] for records of ``rec`` bytes (a multiple of 8) holding int64 / float64 fields: allocated as int64, so the
    records are 8-byte aligned whatever the allocator does."""
    make = torch.zeros if zero else torch.empty
    return make(math.prod(lead) * rec // 8, dtype=torch.int64, device=device).view(torch.uint8).view(*lead, rec)


# ------------------------------------------------------------------------------------------------ the detection core
class Detections:
    """What one geometry call leaves, all on the device: ``clean`` uint8 [B, h, w] in {0, 255}; ``raw`` uint8 [B, max_components,
    record bytes] (``vk_geom_det`` or ``vk_geom_quad`` records, slots in label order); ``counts`` int32 [B] (kept components, also
    when they exceed ``max_components``); ``slots`` int32 [B, h, w]: the slot of every pixel's component, -1 for background and for
    components below ``min_area``, -2 for a kept component beyond ``max_components`` (None after ``detect(slots=False)``)."""

    def __init__(self, fit: str, clean: torch.Tensor, raw: torch.Tensor, counts: torch.Tensor, slots: Optional[torch.Tensor],
                 max_components: int):
        self.fit, self.clean, self.raw, self.counts, self.slots, self.max_components = fit, clean, raw, counts, slots, max_components

    @property
    def record_dtype(self) -> np.dtype:
        return _FITS[self.fit].dtype

    @property
    def record_bytes(self) -> int:
        return int(self.record_dtype.itemsize)

    @property
    def diag_offset(self) -> int:
        return int(_FITS[self.fit].record.d_mean.offset)

    @property
    def box_offset(self) -> int:
        return int(_FITS[self.fit].record.box.offset)

    @property
    def valid_offset(self) -> int:
        """Byte offset of the record's ``valid`` field; -1 where the fit has none (every rectangle is valid)."""
        field = getattr(_FITS[self.fit].record, "valid", None)
        return -1 if field is None else int(field.offset)

    def records(self, counts: Optional[np.ndarray] = None) -> List[np.ndarray]:
        """Per map the structured records of its min(count, max_components) slots, in slot order.  The only method that reads back:
        ``raw``, and ``counts`` unless the caller hands over the host copy it already has."""
        host = self.raw.cpu().numpy().reshape(-1).view(self.record_dtype).reshape(self.raw.shape[0], self.max_components)
        cnt = self.counts.cpu().numpy() if counts is None else counts
        return [host[b, :min(int(cnt[b]), self.max_components)].copy() for b in range(host.shape[0])]


def _device_maps(prob) -> torch.Tensor:
    if not isinstance(prob, torch.Tensor) or prob.dim() != 3:
        raise ValueError("expected a float32 tensor [B, h, w]")
    if not prob.is_cuda:
        raise VkError("probability maps are on %s: this package runs on an MI355X only and has no CPU fallback" % prob.device)
    return prob.detach().contiguous().float()


def _run(fit: str, prob: torch.Tensor, bin_thresh, min_area, min_area_frac, morph_kernel, open_iter, close_iter, fit_outset_px,
         max_components, slots: bool) -> Detections:
    """The launch sequence, once: descriptor, workspace, outputs, the fit's entry point and (``slots``) the slot map.  ``prob`` comes
    from ``_device_maps``.  The library checks the descriptor's ranges (``VkError``) before anything is allocated."""
    f = _FITS[fit]
    B, h, w = (int(v) for v in prob.shape)
    if bin_thresh is None:
        bin_thresh = f.bin_thresh
    if min_area is None:
        min_area = max(200, int(min_area_frac * h * w))      # ui_infer_rectangle.py:322, ui_infer_quadrilateral.py:457
    cap = int(max_components)
    desc = L.vk_geom_desc(h, w, float(bin_thresh), int(morph_kernel), int(open_iter), int(close_iter), int(min_area), cap)
    lib = L.lib()
    nbytes = lib.vk_geom_workspace_bytes(C.byref(desc), B)
    if nbytes < 0:
        L.check(-1, "vk_geom_workspace_bytes")
    dev = prob.device
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    clean = torch.empty(B, h, w, dtype=torch.uint8, device=dev)
    raw = torch.zeros(B, cap, C.sizeof(f.record), dtype=torch.uint8, device=dev)
    counts = torch.zeros(B, dtype=torch.int32, device=dev)
    st = L.current_stream()
    head = (C.byref(desc), int(fit_outset_px)) if f.takes_outset else (C.byref(desc),)
    L.check(getattr(lib, f.entry)(*head, B, prob.data_ptr(), clean.data_ptr(), raw.data_ptr(), counts.data_ptr(), ws.data_ptr(), nbytes, st),
            f.entry)
    slot_map = None
    if slots:
        slot_map = torch.empty(B, h, w, dtype=torch.int32, device=dev)
        L.check(lib.vk_geom_slot_map(C.byref(desc), B, ws.data_ptr(), nbytes, slot_map.data_ptr(), st), "vk_geom_slot_map")
    return Detections(fit, clean, raw, counts, slot_map, cap)


def detect(prob: torch.Tensor, fit: str = "rect", bin_thresh: Optional[float] = None, min_area: Optional[int] = None,
           morph_kernel: int = MORPH_KERNEL, open_iter: int = OPEN_ITER, close_iter: int = CLOSE_ITER,
           fit_outset_px: int = FIT_OUTSET_PX, max_components: int = 64, slots: bool = True) -> Detections:
    """``prob`` float32 [B, h, w] on the device -> ``Detections``; no host round trip.

    ``fit``: "rect" (``vk_geom_minarearect``, bin_thresh 0.5 by default) or "quad" (``vk_geom_quadrilateral``, 0.45).  ``min_area`` in
    pixels; None is the reference's max(200, int(0.0008 h w)).  ``slots=False`` leaves the slot map out (``Detections.slots`` is None):
    enough for the records, not for ``vk.instances.match`` or ``vk.subpix.refine``."""
    _fit(fit)
    prob = _device_maps(prob)
    if not 1 <= int(max_components) <= 4096:
        raise ValueError("max_components %r outside 1..4096" % (max_components,))
    return _run(fit, prob, bin_thresh, min_area, MIN_AREA_FRAC, morph_kernel, open_iter, close_iter, fit_outset_px, max_components, slots)


# ------------------------------------------------------------------------------------------------ the reference's entry points
def _batch(fit: str, prob, bin_thresh, min_area_frac, morph_kernel, open_iter, close_iter, fit_outset_px, max_components):
    dets = _run(fit, _device_maps(prob), bin_thresh, None, min_area_frac, morph_kernel, open_iter, close_iter, fit_outset_px,
                max_components, slots=False)
    return dets.clean, [_FITS[fit].to_dicts(rows) for rows in dets.records()]          # records() synchronises


def _multi(fit: str, prob01, device, *args):
    """One map, numpy (uploaded) or tensor, through ``_batch``; the clean mask comes back as numpy, as in the reference."""
    if isinstance(prob01, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(prob01, dtype=np.float32)).to(torch.device(device if device is not None else "cuda"))
    else:
        t = prob01
    clean, dets = _batch(fit, t.reshape(1, *t.shape[-2:]), *args, max_components=64)
    return clean[0].cpu().numpy(), dets[0]


def postprocess_minarearect_batch(prob: torch.Tensor, bin_thresh: float = BIN_THRESH, min_area_frac: float = MIN_AREA_FRAC,
                                  morph_kernel: int = MORPH_KERNEL, open_iter: int = OPEN_ITER, close_iter: int = CLOSE_ITER,
                                  max_components: int = 64) -> Tuple[torch.Tensor, List[List[Dict]]]:
    """``prob``: float32 [B, h, w] probability maps on the device.  Returns (clean uint8 [B, h, w] in {0, 255} on the device,
    per map the reference's detection list).  One host synchronisation at the end (the detection records are read back)."""
    return _batch("rect", prob, bin_thresh, min_area_frac, morph_kernel, open_iter, close_iter, 0, max_components)


def postprocess_minarearect_multi(img_bgr, prob01, bin_thresh: float = BIN_THRESH, min_area_frac: float = MIN_AREA_FRAC,
                                  morph_kernel: int = MORPH_KERNEL, open_iter: int = OPEN_ITER, close_iter: int = CLOSE_ITER,
                                  device=None):
    """Signature and return value of ui_infer_rectangle.postprocess_minarearect_multi (:291-381): ``(clean_bin uint8 [h, w],
    detections)`` with ``detections`` sorted by area, each ``{"label", "area", "box" int32 [4, 2], "center", "d1", "d2", "d_mean"}``
    (+ "size", "direction", "hull_vertices").  ``img_bgr`` is accepted and ignored, as in the reference.  ``prob01`` may be a numpy
    array (uploaded) or a device tensor (what ``vk.Segmenter.infer`` can hand over without a round trip)."""
    return _multi("rect", prob01, device, bin_thresh, min_area_frac, morph_kernel, open_iter, close_iter, 0)


def postprocess_quadrilateral_batch(prob: torch.Tensor, bin_thresh: float = BIN_THRESH_QUAD, min_area_frac: float = MIN_AREA_FRAC,
                                    morph_kernel: int = MORPH_KERNEL, open_iter: int = OPEN_ITER, close_iter: int = CLOSE_ITER,
                                    fit_outset_px: int = FIT_OUTSET_PX, max_components: int = 64) -> Tuple[torch.Tensor, List[List[Dict]]]:
    """``prob``: float32 [B, h, w] on the device -> (clean uint8 [B, h, w] on the device, per map the detection list of
    ui_infer_quadrilateral.postprocess_minarearect_multi).  One host synchronisation (the records are read back)."""
    return _batch("quad", prob, bin_thresh, min_area_frac, morph_kernel, open_iter, close_iter, fit_outset_px, max_components)


def postprocess_quadrilateral_multi(img_bgr, prob01, bin_thresh: float = BIN_THRESH_QUAD, min_area_frac: float = MIN_AREA_FRAC,
                                    morph_kernel: int = MORPH_KERNEL, open_iter: int = OPEN_ITER, close_iter: int = CLOSE_ITER,
                                    fit_outset_px: int = FIT_OUTSET_PX, device=None):
    """Signature and return value of ui_infer_quadrilateral.postprocess_minarearect_multi (:423-530): ``(clean_bin uint8 [h, w],
    detections)``, each detection ``{"label", "area", "box" int32 [4, 2] clockwise, "center", "d1", "d2", "d_mean"}`` (+ diagnostics).
    ``img_bgr`` is accepted and ignored, as in the reference."""
    return _multi("quad", prob01, device, bin_thresh, min_area_frac, morph_kernel, open_iter, close_iter, fit_outset_px)
