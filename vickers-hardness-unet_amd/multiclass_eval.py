"""Validation and inference for ``vk.multiclass.Unet(classes=C)`` on the device (re-exported by ``vk.multiclass``).

Validation (csrc/multiclass_eval.hip, ``vk_seg_metrics_multi``): the reference's thresholded ``dice_coef`` / ``iou_coef``
(train.py:230-281) per class, from one pass over the logits and the target::

    mean_dice, mean_iou, dice_c, iou_c = vk.multiclass.seg_metrics(logits, target, mode="multiclass")

    mode="multilabel"  logits [N,C,H,W], target [N,C,H,W] of 0/1; pred_c = sigmoid(x_c) > threshold (x_c > threshold with
                       from_logits=False).  Another target value is a bad label and skips that (pixel, class).
    mode="multiclass"  logits [N,C,H,W] (C >= 2), target int [N,H,W]; pred = argmax_c x_c (ties to the lowest index).  A label
                       outside [0, C) is a bad label and skips the pixel.

Per (image, class): tp, fp, fn, tn as exact int64 counts; dice = (2 tp + eps) / (2 tp + fp + fn + eps) and
iou = (tp + eps) / (tp + fp + fn + eps) in fp32 with the reference's operation order.  A class that is absent from both the
prediction and the target of an image scores 1 there, as in the reference.  A class's score is the mean over images, the overall
score the mean over classes.

Inference (csrc/multiclass_post.hip): the class-plane counterparts of ``prepost.postprocess_mask`` / ``postprocess_prob`` and of the
``predict_mask`` / ``Segmenter`` wrappers, reusing ``prepost.preprocess`` and ``letterbox_geometry`` unchanged.  One class plane
``probs[k:k+1]`` of ``Segmenter.infer`` output is a probability map that ``vk.geometry.postprocess_minarearect_batch`` /
``postprocess_quadrilateral_batch`` take as they are.  CUDA tensors only: there is no CPU fallback."""
from __future__ import annotations

import ctypes as C
from typing import List, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from . import prepost as _pp
from ._lib import VkError

__all__ = ["seg_stats", "seg_metrics_device", "seg_metrics", "postprocess_labels", "postprocess_masks", "postprocess_probs",
           "predict_mask", "Segmenter"]

MODES = {"multilabel": L.VK_LOSS_MULTILABEL, "multiclass": L.VK_LOSS_MULTICLASS}
MAX_CLASSES = 16


def _mode(mode: str, classes: int) -> int:
    if mode not in MODES:
        raise ValueError("mode must be 'multilabel' or 'multiclass', got %r" % (mode,))
    if not 1 <= classes <= MAX_CLASSES:
        raise ValueError("expected 1 <= C <= %d classes, got %d" % (MAX_CLASSES, classes))
    if mode == "multiclass" and classes < 2:
        raise ValueError("mode 'multiclass' needs C >= 2 classes (got %d); use 'multilabel' for one class" % classes)
    return MODES[mode]


def _run_metrics(logits: torch.Tensor, target: torch.Tensor, mode: str, threshold: float, from_logits: bool, eps: float):
    """-> (out fp32 [2 + 2C + 2NC], stats int64 [4, N, C], bad-label count int32 [1]), all on the device"""
    if logits.dim() < 3 or logits.shape[0] < 1:
        raise ValueError("expected logits [N, C, H, W], got %s" % (tuple(logits.shape),))
    n, c = int(logits.shape[0]), int(logits.shape[1])
    m = _mode(mode, c)
    if m == L.VK_LOSS_MULTICLASS:
        want = (n,) + tuple(logits.shape[2:])
        if tuple(target.shape) != want:
            raise ValueError("multiclass target must be [N, H, W] = %s, got %s" % (want, tuple(target.shape)))
        if target.is_floating_point() or target.dtype == torch.bool:
            raise ValueError("multiclass target must hold integer class indices, got %s" % target.dtype)
        t = target.detach().to(torch.int64).contiguous()
    else:
        if tuple(target.shape) != tuple(logits.shape):
            raise ValueError("multilabel target must have the logits' shape %s, got %s" % (tuple(logits.shape), tuple(target.shape)))
        t = target.detach().to(torch.float32).contiguous()
    if not (logits.is_cuda and target.is_cuda):
        raise VkError("seg metrics take CUDA tensors (%s / %s): no CPU fallback in this package" % (logits.device, target.device))
    x = logits.detach().to(torch.float32).contiguous()
    per_image = x.numel() // (n * c)
    lib = L.lib()
    ws_bytes = lib.vk_seg_metrics_multi_workspace_bytes(n, c)
    ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=x.device)
    out = torch.empty(2 + 2 * c + 2 * n * c, dtype=torch.float32, device=x.device)
    bad = torch.empty(1, dtype=torch.int32, device=x.device)
    stats = torch.empty(4, n, c, dtype=torch.int64, device=x.device)
    L.check(lib.vk_seg_metrics_multi(m, n, c, per_image, x.data_ptr(), t.data_ptr(), 1 if from_logits else 0, float(threshold),
                                     float(eps), ws.data_ptr(), ws_bytes, stats.data_ptr(), out.data_ptr(),
                                     bad.data_ptr(), L.current_stream()), "vk_seg_metrics_multi")
    return out, stats, bad


def seg_stats(logits: torch.Tensor, target: torch.Tensor, mode: str, threshold: float = 0.5,
              from_logits: bool = True) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(tp, fp, fn, tn): int64 [N, C] device tensors, smp ``get_stats``'s layout with the prediction rule of the module docstring.
    No host synchronisation; bad labels are skipped without a check (``seg_metrics`` raises on them)."""
    _, stats, _ = _run_metrics(logits, target, mode, threshold, from_logits, 1e-7)
    return stats[0], stats[1], stats[2], stats[3]


def seg_metrics_device(logits: torch.Tensor, target: torch.Tensor, mode: str, threshold: float = 0.5, from_logits: bool = True,
                       eps: float = 1e-7) -> torch.Tensor:
    """Device tensor of 2 + 2 C + 2 N C floats: [mean dice, mean iou, dice_c[C], iou_c[C], per image n and class c: dice, iou];
    no host synchronisation."""
    return _run_metrics(logits, target, mode, threshold, from_logits, eps)[0]


def seg_metrics(logits: torch.Tensor, target: torch.Tensor, mode: str, threshold: float = 0.5, from_logits: bool = True,
                eps: float = 1e-7) -> Tuple[float, float, List[float], List[float]]:
    """(mean dice, mean iou, dice per class, iou per class) as Python floats, from one synchronisation.  Raises VkError when the
    target holds bad labels (see the module docstring)."""
    out, _, bad_d = _run_metrics(logits, target, mode, threshold, from_logits, eps)
    v = out.to("cpu", non_blocking=True)
    bad = int(bad_d.item())             # synchronises the stream: both copies are complete
    c = int(logits.shape[1])
    if bad:
        what = "label(s) outside [0, %d)" % c if mode == "multiclass" else "target value(s) other than 0 or 1"
        raise VkError("%s target holds %d %s" % (mode, bad, what))
    v = v.tolist()
    return v[0], v[1], v[2:2 + c], v[2 + c:2 + 2 * c]


# ------------------------------------------------------------------------------------------------ inference post-processing
def _planes(logits_csq: torch.Tensor) -> torch.Tensor:
    """[C, S, S] (or [1, C, S, S]) logits -> contiguous fp32 [C, S, S] on the device."""
    lg = logits_csq.detach()
    if lg.dim() == 4 and lg.shape[0] == 1:
        lg = lg[0]
    if lg.dim() != 3 or lg.shape[1] != lg.shape[2]:
        raise ValueError("expected square class planes [C, S, S], got %s" % (tuple(logits_csq.shape),))
    if not 1 <= lg.shape[0] <= MAX_CLASSES:
        raise ValueError("expected 1 <= C <= %d class planes, got %d" % (MAX_CLASSES, lg.shape[0]))
    if not lg.is_cuda:
        raise VkError("post-processing takes CUDA tensors (%s): no CPU fallback in this package" % lg.device)
    return lg.to(torch.float32).contiguous()


def postprocess_labels(logits_csq: torch.Tensor, meta: Tuple) -> torch.Tensor:
    """logits [C, S, S] -> uint8 label map [h, w] on the device: argmax over the classes, crop, INTER_NEAREST."""
    lg = _planes(logits_csq)
    _, geo, (h, w) = meta
    out = torch.empty(h, w, dtype=torch.uint8, device=lg.device)
    d = _pp._desc(h, w, int(lg.shape[-1]), geo)
    L.check(L.lib().vk_letterbox_postprocess_labels(C.byref(d), int(lg.shape[0]), lg.data_ptr(), out.data_ptr(), L.current_stream()),
            "vk_letterbox_postprocess_labels")
    return out


def postprocess_masks(logits_csq: torch.Tensor, meta: Tuple, thresh: float = 0.5) -> torch.Tensor:
    """logits [C, S, S] -> uint8 {0,255} masks [C, h, w] on the device: per class sigmoid >= thresh, crop, INTER_NEAREST."""
    lg = _planes(logits_csq)
    _, geo, (h, w) = meta
    out = torch.empty(lg.shape[0], h, w, dtype=torch.uint8, device=lg.device)
    d = _pp._desc(h, w, int(lg.shape[-1]), geo)
    L.check(L.lib().vk_letterbox_postprocess_mask_multi(C.byref(d), int(lg.shape[0]), lg.data_ptr(), float(thresh), out.data_ptr(),
                                                         L.current_stream()), "vk_letterbox_postprocess_mask_multi")
    return out


def postprocess_probs(logits_csq: torch.Tensor, meta: Tuple, mode: str) -> torch.Tensor:
    """logits [C, S, S] -> probabilities fp32 [C, h, w] in [0, 1] on the device: per-class sigmoid ("multilabel") or softmax over the
    classes ("multiclass"), crop, INTER_LINEAR (a copy when the crop has the original size), clip."""
    lg = _planes(logits_csq)
    m = _mode(mode, int(lg.shape[0]))
    _, geo, (h, w) = meta
    out = torch.empty(lg.shape[0], h, w, dtype=torch.float32, device=lg.device)
    d = _pp._desc(h, w, int(lg.shape[-1]), geo)
    L.check(L.lib().vk_letterbox_postprocess_prob_multi(C.byref(d), int(lg.shape[0]), m, lg.data_ptr(), out.data_ptr(),
                                                         L.current_stream()), "vk_letterbox_postprocess_prob_multi")
    return out


def predict_mask(model, bgr: np.ndarray, mode: str, device=None, img_size: int = 512, thresh: float = 0.5) -> np.ndarray:
    """predict_mask (infer_pth_gui.py:45-53) for C classes, "pad_br" letterbox: the uint8 label map [h, w] for mode "multiclass",
    uint8 {0,255} masks [C, h, w] for mode "multilabel"."""
    device = torch.device(device if device is not None else "cuda")
    x, meta = _pp.preprocess(bgr, img_size, "pad_br", device)
    with torch.no_grad():
        logits = model(x)
    _mode(mode, int(logits.shape[1]))
    if mode == "multiclass":
        return postprocess_labels(logits[0], meta).cpu().numpy()
    return postprocess_masks(logits[0], meta, thresh).cpu().numpy()


class Segmenter(_pp.Segmenter):
    """``prepost.Segmenter`` ("centered" letterbox) for a C-class model: ``infer`` gives fp32 probabilities [C, h, w] (per-class sigmoid
    for mode "multilabel", softmax for "multiclass"), ``infer_labels`` the uint8 argmax label map [h, w]."""

    def __init__(self, model, mode: str, img_size: int = 512, device=None):
        if mode not in MODES:
            raise ValueError("mode must be 'multilabel' or 'multiclass', got %r" % (mode,))
        super().__init__(model, img_size, device)
        self.mode = mode

    def _logits(self, x):
        with torch.no_grad():
            return self.model(x)

    def infer(self, img_bgr: np.ndarray) -> np.ndarray:
        x, meta = self.preprocess(img_bgr)
        return postprocess_probs(self._logits(x)[0], meta, self.mode).cpu().numpy()

    def infer_labels(self, img_bgr: np.ndarray) -> np.ndarray:
        x, meta = self.preprocess(img_bgr)
        return postprocess_labels(self._logits(x)[0], meta).cpu().numpy()

    def infer_batch(self, images: Sequence[np.ndarray]) -> List[np.ndarray]:
        """Several images through ONE forward pass; [C, h, w] probabilities per image."""
        x, metas = _pp.preprocess_batch(images, self.img_size, "centered", self.device)
        logits = self._logits(x)
        return [postprocess_probs(logits[i], m, self.mode).cpu().numpy() for i, m in enumerate(metas)]
