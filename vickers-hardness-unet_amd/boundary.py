"""Distance maps of masks on the device: how far the predicted outline lies from the labelled one, and a loss that
pulls the outline in particular.

Everything downstream of the mask reads the diagonal of an indentation off its outline; ``seg_metrics``, ``vk.sweep`` and every term of
``vk.seglosses`` / ``vk.lovasz`` score area.  This module adds

* ``edt_sq``: the exact squared Euclidean distance transform (``vk_edt_sq``), int32, to the foreground, the background or the inner
  boundary of a mask;
* ``signed_distance``: the map of the boundary loss of Kervadec et al. (MIDL 2019): the distance to the foreground outside it,
  ``1 - distance to the background`` inside it, 0 for an empty or a full mask (``vk_boundary_phi``);
* ``surface_stats`` / ``surface_metrics`` / ``BoundaryMetrics``: Hausdorff distance, its 95th percentile, the average symmetric
  surface distance, the normalised surface Dice at given tolerances and Boundary IoU, per image (``vk_boundary_stats``);
* ``BoundaryLoss``: ``mean(sigmoid(logits) * phi)`` with its gradient (``vk_boundary_loss``).

The percentile is the NEAREST RANK one: the k-th smallest of the n squared distances, k = (95 n + 99) // 100 — an element of the
sample, found exactly by a radix select; ``numpy.percentile`` interpolates between two elements and gives another number.  ``hd95`` is
the larger of the two directed percentiles.

``BoundaryLoss`` returns a tensor through an ``autograd.Function``; it adds to the value of any other loss as tensors do
(``vk.DiceLoss(mode="binary")(l, y) + 0.01 * vk.BoundaryLoss()(l, y)``).  It is NOT a member of the ``LossSum`` algebra of
``vk.seglosses`` and is not reachable from ``model.loss_and_backward``: it runs as a call of its own after the forward pass.  The
softmax form of the loss is not implemented.  Whether the loss improves the diagonal error of a trained model is unmeasured: no
trained weights exist.  No CPU fallback: without libvkunet.so and an MI355X the entry points raise."""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch
from torch import nn

from . import _lib as L
from ._lib import VkError

NONE = L.VK_EDT_NONE
MAX_SIDE = L.VK_EDT_MAX_SIDE
SITES = {"fg": L.VK_EDT_FG, "bg": L.VK_EDT_BG, "edge": L.VK_EDT_EDGE}
ROWS = {"auto": 0, "search": L.VK_EDT_ROWS_SEARCH, "envelope": L.VK_EDT_ROWS_ENVELOPE}
RECORD_DTYPE = np.dtype([("n_pred", "<i8"), ("n_gt", "<i8"), ("area_pred", "<i8"), ("area_gt", "<i8"), ("max2_pg", "<i4"), ("max2_gp", "<i4"),
                         ("q95_2_pg", "<i4"), ("q95_2_gp", "<i4"), ("sum_pg", "<f8"), ("sum_gp", "<f8"), ("within_pg", "<i8", (8,)),
                         ("within_gp", "<i8", (8,)), ("band_inter", "<i8"), ("band_union", "<i8"), ("flags", "<i4"), ("reserved", "<i4")])
assert RECORD_DTYPE.itemsize == C.sizeof(L.vk_boundary_rec)


def _maps(t: torch.Tensor, who: str):
    """A mask or probability tensor [..., h, w] as (contiguous tensor, kind, batch, h, w)."""
    if not isinstance(t, torch.Tensor) or t.dim() < 2:
        raise ValueError(f"{who}: expected a tensor [..., h, w]")
    if not t.is_cuda:
        raise VkError(f"{who}: input is on {t.device}: no CPU fallback in this package")
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    if t.dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"{who}: dtype {t.dtype} is neither uint8 / bool nor float32")
    h, w = int(t.shape[-2]), int(t.shape[-1])
    batch = int(t.numel() // max(h * w, 1))
    if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE) or batch < 1:
        raise ValueError(f"{who}: maps of {h} x {w} (batch {batch}) outside 1..{MAX_SIDE}")
    return t.contiguous(), (L.VK_EDT_SRC_U8 if t.dtype == torch.uint8 else L.VK_EDT_SRC_F32), batch, h, w


def _edt(t, kind, batch, h, w, threshold, sites, ws=None):
    d2 = torch.empty(t.shape, dtype=torch.int32, device=t.device)
    if ws is None:
        ws = torch.empty(int(L.lib().vk_edt_workspace_bytes(batch, h, w)) // 4, dtype=torch.int32, device=t.device)
    L.check(L.lib().vk_edt_sq(batch, h, w, t.data_ptr(), kind, float(threshold), sites, d2.data_ptr(), ws.data_ptr(), ws.numel() * 4,
                              L.current_stream()), "vk_edt_sq")
    return d2, ws


def edt_sq(mask: torch.Tensor, sites: str = "fg", threshold: float = 0.5, rows: str = "auto") -> torch.Tensor:
    """int32, the shape of ``mask`` ([..., h, w]; uint8 / bool: foreground != 0; float32: foreground > ``threshold``): the squared
    distance of every pixel to the nearest site of its own map — ``"fg"``, ``"bg"`` or ``"edge"`` (foreground pixels with a
    4-neighbour inside the image in the background).  ``NONE`` (2^31 - 1) everywhere in a map without a site.  ``rows``: ``"auto"``
    (the kernel chooses per row), ``"search"`` or ``"envelope"``: the two exact forms of the row pass give the same map
    (``profiles/boundary/README.md`` has their times)."""
    if sites not in SITES:
        raise ValueError(f"sites must be one of {sorted(SITES)}, not {sites!r}")
    if rows not in ROWS:
        raise ValueError(f"rows must be one of {sorted(ROWS)}, not {rows!r}")
    t, kind, batch, h, w = _maps(mask, "edt_sq")
    return _edt(t, kind, batch, h, w, threshold, SITES[sites] | ROWS[rows])[0]


def signed_distance(target: torch.Tensor, threshold: float = 0.5) -> torch.Tensor:
    """float32, the shape of ``target``: sqrt(d2 to the foreground) on the background, 1 - sqrt(d2 to the background) on the
    foreground (<= 0, 0 on the inner boundary), 0 everywhere for an empty or a full map."""
    t, kind, batch, h, w = _maps(target, "signed_distance")
    d_fg, ws = _edt(t, kind, batch, h, w, threshold, L.VK_EDT_FG)
    d_bg, _ = _edt(t, kind, batch, h, w, threshold, L.VK_EDT_BG, ws)
    phi = torch.empty(t.shape, dtype=torch.float32, device=t.device)
    L.check(L.lib().vk_boundary_phi(batch, h, w, d_fg.data_ptr(), d_bg.data_ptr(), phi.data_ptr(), L.current_stream()), "vk_boundary_phi")
    return phi


def radius_sq(tau: float) -> int:
    """floor(tau^2): for an integer d^2, d <= tau iff d^2 <= floor(tau^2)."""
    if not (tau >= 0 and math.isfinite(tau)):
        raise ValueError(f"radius {tau!r} must be finite and >= 0")
    return min(int(math.floor(float(tau) * float(tau))), NONE - 1)


def surface_stats(pred: torch.Tensor, target: torch.Tensor, threshold: float = 0.5, tolerances: Sequence[float] = (1, 2, 3), band: float = 2,
                  from_logits: bool = False, target_threshold: float = 0.5) -> torch.Tensor:
    """One ``vk_boundary_rec`` per map, as a uint8 tensor [batch, 216] that stays on the device (``records`` reads it back).  ``pred``
    and ``target``: [..., h, w] of the same shape, masks or probabilities; ``from_logits`` applies ``torch.sigmoid`` to ``pred`` first
    (the C ABI takes masks or probabilities only).  No host synchronisation."""
    if tuple(pred.shape) != tuple(target.shape):
        raise ValueError(f"pred {tuple(pred.shape)} and target {tuple(target.shape)} differ in shape")
    if len(tolerances) > 8:
        raise ValueError("at most 8 tolerances")
    tol2 = (C.c_int32 * 8)(*[radius_sq(t) for t in tolerances])
    if from_logits:
        pred = torch.sigmoid(pred.float())
    p, pk, batch, h, w = _maps(pred, "surface_stats")
    g, gk, _, _, _ = _maps(target, "surface_stats")
    lib = L.lib()
    ws = torch.empty(int(lib.vk_boundary_stats_workspace_bytes(batch, h, w)) // 8, dtype=torch.int64, device=p.device)
    out = torch.empty(batch, RECORD_DTYPE.itemsize // 8, dtype=torch.int64, device=p.device)
    L.check(lib.vk_boundary_stats(batch, h, w, p.data_ptr(), pk, float(threshold), g.data_ptr(), gk, float(target_threshold), len(tolerances),
                                  tol2, radius_sq(band), out.data_ptr(), ws.data_ptr(), ws.numel() * 8, L.current_stream()),
            "vk_boundary_stats")
    return out.view(torch.uint8)


def records(stats: torch.Tensor) -> np.ndarray:
    """The device records of ``surface_stats`` as a numpy structured array (``RECORD_DTYPE``): the one read-back."""
    return np.frombuffer(stats.cpu().numpy().tobytes(), dtype=RECORD_DTYPE).copy()


def metrics_from_records(recs: np.ndarray, tolerances: Sequence[float], scale=None) -> Dict[str, object]:
    """Per-image arrays and their means from host records: ``hd``, ``hd95``, ``assd`` (map pixels times ``scale``), ``nsd`` ({tau:
    array}), ``boundary_iou``; ``mean`` holds the batch means.  Both boundaries empty: distances 0, ratios 1; one empty: ``inf`` and 0."""
    n = len(recs)
    sc = np.ones(n) if scale is None else np.broadcast_to(np.asarray(scale, np.float64), (n,)).copy()
    n_p, n_g = recs["n_pred"].astype(np.float64), recs["n_gt"].astype(np.float64)
    both, none = (n_p > 0) & (n_g > 0), (n_p == 0) & (n_g == 0)
    fill = np.where(none, 0.0, np.inf)
    tot = np.where(both, n_p + n_g, 1.0)

    def dist(v):
        return np.where(both, sc * v, fill)

    out = {"hd": dist(np.sqrt(np.maximum(np.maximum(recs["max2_pg"], recs["max2_gp"]), 0).astype(np.float64))),
           "hd95": dist(np.sqrt(np.maximum(np.maximum(recs["q95_2_pg"], recs["q95_2_gp"]), 0).astype(np.float64))),
           "assd": dist((recs["sum_pg"] + recs["sum_gp"]) / tot)}
    ratio_fill = np.where(none, 1.0, 0.0)
    out["nsd"] = {t: np.where(both, (recs["within_pg"][:, k] + recs["within_gp"][:, k]) / tot, ratio_fill) for k, t in enumerate(tolerances)}
    bu = recs["band_union"].astype(np.float64)
    out["boundary_iou"] = np.where(both, np.where(bu > 0, recs["band_inter"] / np.where(bu > 0, bu, 1.0), 1.0), ratio_fill)
    with np.errstate(invalid="ignore"):
        mean = {k: float(np.mean(v)) for k, v in out.items() if k != "nsd"} if n else {}
        if n:
            mean["nsd"] = {t: float(np.mean(v)) for t, v in out["nsd"].items()}
    out["mean"] = mean
    out["n_images"] = n
    return out


def surface_metrics(pred: torch.Tensor, target: torch.Tensor, threshold: float = 0.5, tolerances: Sequence[float] = (1, 2, 3), band: float = 2,
                    scale=None, from_logits: bool = False) -> Dict[str, object]:
    """``surface_stats``, one read-back, ``metrics_from_records``.  ``scale``: per-image map-to-source factors (or one number), so the
    distances read in source pixels as ``vk.subpix`` reports diagonals; tolerances and the band stay in map pixels."""
    return metrics_from_records(records(surface_stats(pred, target, threshold, tolerances, band, from_logits)), tuple(tolerances), scale)


class BoundaryMetrics:
    """Surface metrics over an epoch, shaped like ``ThresholdSweep``: ``update`` per batch (device records, no synchronisation),
    ``compute()`` reads everything back once.  The result over several batches equals one call over their union."""

    def __init__(self, threshold: float = 0.5, tolerances: Sequence[float] = (1, 2, 3), band: float = 2, from_logits: bool = False):
        self.threshold, self.tolerances, self.band, self.from_logits = float(threshold), tuple(tolerances), band, bool(from_logits)
        [radius_sq(t) for t in self.tolerances + (band,)]
        self.reset()

    def reset(self) -> None:
        self._stats: List[torch.Tensor] = []
        self._scales: List[np.ndarray] = []

    @property
    def n_images(self) -> int:
        return sum(int(s.shape[0]) for s in self._stats)

    @property
    def n_batches(self) -> int:
        return len(self._stats)

    def update(self, pred: torch.Tensor, target: torch.Tensor, scale=None) -> None:
        s = surface_stats(pred, target, self.threshold, self.tolerances, self.band, self.from_logits)
        n = int(s.shape[0])
        self._stats.append(s)
        self._scales.append(np.ones(n) if scale is None else np.broadcast_to(np.asarray(scale, np.float64), (n,)).copy())

    def compute(self) -> Dict[str, object]:
        if not self._stats:
            raise ValueError("BoundaryMetrics.compute() before any update")
        return metrics_from_records(records(torch.cat(self._stats)), self.tolerances, np.concatenate(self._scales))


def _loss_call(logits: torch.Tensor, phi: torch.Tensor, grad_scale: float, want_grad: bool):
    n = int(logits.shape[0])
    c = int(logits.shape[1]) if logits.dim() >= 3 else 1
    hw = int(logits.numel() // max(n * c, 1))
    out = torch.empty(1, dtype=torch.float32, device=logits.device)
    ws = torch.empty(L.VK_BOUNDARY_LOSS_WS_BYTES // 8, dtype=torch.float64, device=logits.device)
    grad = torch.empty_like(logits) if want_grad else None
    L.check(L.lib().vk_boundary_loss(n, c, hw, logits.data_ptr(), phi.data_ptr(), float(grad_scale), L.ptr(grad), out.data_ptr(), ws.data_ptr(),
                                     ws.numel() * 8, L.current_stream()), "vk_boundary_loss")
    return out, grad


class _BoundaryLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, phi):
        out, grad = _loss_call(logits, phi, 1.0, ctx.needs_input_grad[0])
        ctx.save_for_backward(grad)
        return out.reshape(())

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return (grad * g if grad is not None else None), None


class BoundaryLoss(nn.Module):
    """``mean(sigmoid(logits) * phi)`` over logits [N, C, H, W] (or [N, H, W]), 1 <= C <= 16, float32.  ``forward(logits, target=None,
    dist=None)``: ``dist`` is ``phi`` (``signed_distance`` of the target, e.g. computed once per dataset); without it ``phi`` is built
    from ``target`` under ``no_grad``.  Returns a 0-d tensor; the gradient is written by the same kernel pass.  Not a ``LossSum`` term
    and not part of ``model.loss_and_backward`` (see the module text)."""

    def __init__(self, threshold: float = 0.5):
        super().__init__()
        self.threshold = float(threshold)

    def forward(self, logits: torch.Tensor, target: Optional[torch.Tensor] = None, dist: Optional[torch.Tensor] = None) -> torch.Tensor:
        if (target is None) == (dist is None):
            raise ValueError("BoundaryLoss takes either target or dist")
        if not isinstance(logits, torch.Tensor) or logits.dim() < 3:
            raise ValueError("logits must be [N, C, H, W] or [N, H, W]")
        if not logits.is_cuda:
            raise VkError(f"loss input is on {logits.device}: no CPU fallback in this package")
        if logits.dtype != torch.float32:
            raise ValueError(f"logits must be float32, not {logits.dtype}")
        if logits.dim() >= 4 and not 1 <= logits.shape[1] <= 16:
            raise ValueError(f"C = {logits.shape[1]} outside 1..16")
        if dist is None:
            if target.numel() != logits.numel():
                raise ValueError(f"target {tuple(target.shape)} does not match logits {tuple(logits.shape)}")
            with torch.no_grad():
                t = target.reshape(logits.shape)
                dist = signed_distance(t if t.dtype in (torch.uint8, torch.bool) else t.float(), self.threshold)
        if tuple(dist.shape) != tuple(logits.shape) or dist.dtype != torch.float32 or dist.device != logits.device:
            raise ValueError("dist must be a float32 tensor of the shape and device of logits")
        return _BoundaryLossFn.apply(logits.contiguous(), dist.contiguous())
