"""Loss modules with the reference's call signatures (train.py:600-601, 438):

    loss_bce  = nn.BCEWithLogitsLoss()            (torch's own; works unchanged on our logits)
    loss_dice = vk.losses.DiceLoss(mode="binary") (this file; replaces smp.losses.DiceLoss)
    loss = loss_bce(logits, y) + loss_dice(logits, y)

``DiceLoss`` and ``BCEDiceLoss`` run the fused HIP reduction (vk_bce_dice_loss); both participate in
autograd.  smp defaults restated: from_logits=True, smooth=0, eps=1e-7, log_loss=False, batch-global
reduction.

``DiceLoss`` / ``BCEDiceLoss`` here are the reference's binary drop-ins and refuse other modes, as before.  More than one class
(``vk.multiclass.Unet(classes=C)``, logits [N,C,H,W]) uses the subclasses in ``vk.multiclass``, which take every mode:

    vk.multiclass.DiceLoss(mode="multilabel")  target fp32 [N,C,H,W]  sigmoid per channel      (vk_multilabel_loss)
    vk.multiclass.DiceLoss(mode="multiclass")  target int64 [N,H,W]   softmax over channels    (vk_multiclass_loss)
    vk.multiclass.BCEDiceLoss(mode="multilabel") = nn.BCEWithLogitsLoss() + DiceLoss("multilabel")
    CEDiceLoss()                                 = nn.CrossEntropyLoss() + DiceLoss("multiclass")   (also vk.multiclass.CEDiceLoss)

A multi-class label outside [0, C) raises VkError (the kernel reports it through a device flag that is read back)."""
from __future__ import annotations

from functools import partial

import torch
import torch.nn as nn

from . import _lib
from ._lib import VkError, check, lib
from ._lossfn import LossFn, check_target


def _binary_run(w_bce, x, y, dl):
    sums = torch.empty(8, dtype=torch.float64, device=x.device)
    out = torch.empty(4, dtype=torch.float32, device=x.device)
    check(lib().vk_bce_dice_loss(x.numel(), x.data_ptr(), y.data_ptr(), sums.data_ptr(), out.data_ptr(), _lib.ptr(dl), 1.0, w_bce, 1.0,
                                 _lib.current_stream()), "vk_bce_dice_loss")
    return out[0], None


def _multi_run(multiclass, w_pix, x, y, dl):
    """vk_multilabel_loss / vk_multiclass_loss on logits [N,C,H,W]: w_pix * (BCE or CE) + Dice."""
    N, Cc, H, W = x.shape
    L = lib()
    ws = torch.empty(L.vk_multi_loss_workspace_bytes(N, Cc, H * W), dtype=torch.uint8, device=x.device)
    out = torch.empty(4, dtype=torch.float32, device=x.device)
    fn = L.vk_multiclass_loss if multiclass else L.vk_multilabel_loss
    check(fn(N, Cc, H * W, x.data_ptr(), y.data_ptr(), ws.data_ptr(), ws.numel(), out.data_ptr(), _lib.ptr(dl), 1.0, w_pix, 1.0,
             _lib.current_stream()), "vk_multiclass_loss" if multiclass else "vk_multilabel_loss")
    return out[0], out[3] if multiclass else None          # out[3]: the device flag of out-of-range labels


def _apply(logits, target, mode, w_pix):
    """``w_pix * (BCE or CE) + Dice`` of ``mode`` through the fused reduction of that mode."""
    if not logits.is_cuda:
        raise VkError("loss input is on %s: no CPU fallback in this package" % logits.device)
    if mode == "binary":
        return LossFn.apply(logits, target, partial(_binary_run, w_pix), False, None)
    if logits.dim() != 4:
        raise ValueError("expected logits [N,C,H,W], got %s" % (tuple(logits.shape),))
    check_target(logits.shape, target, mode, "DiceLoss('multiclass')")
    return LossFn.apply(logits, target, partial(_multi_run, mode == "multiclass", w_pix), mode == "multiclass", None)


class DiceLoss(nn.Module):
    modes = ("binary",)            # the reference's DiceLoss; vk.multiclass.DiceLoss adds "multilabel" and "multiclass"

    def __init__(self, mode: str = "binary", classes=None, log_loss: bool = False, from_logits: bool = True,
                 smooth: float = 0.0, ignore_index=None, eps: float = 1e-7):
        super().__init__()
        if mode not in self.modes or classes is not None or log_loss or not from_logits or smooth != 0.0 \
                or ignore_index is not None or eps != 1e-7:
            raise NotImplementedError("only DiceLoss(mode=%s) with smp defaults is implemented (reference train.py:601)%s"
                                      % (" | ".join(repr(m) for m in self.modes),
                                         "" if len(self.modes) > 1 else "; more than one class: vk.multiclass.DiceLoss"))
        self.mode = mode

    def forward(self, y_pred, y_true):
        return _apply(y_pred, y_true, self.mode, 0.0)


class BCEDiceLoss(nn.Module):
    """``BCEWithLogitsLoss()(x, y) + DiceLoss(mode)(x, y)`` in one reduction pass; mode 'binary' here, also 'multilabel' in
    vk.multiclass.BCEDiceLoss."""
    modes = ("binary",)

    def __init__(self, mode: str = "binary"):
        super().__init__()
        if mode not in self.modes:
            raise NotImplementedError("BCEDiceLoss(mode=%r): %s" % (mode, " | ".join(repr(m) for m in self.modes)))
        self.mode = mode

    def forward(self, y_pred, y_true):
        return _apply(y_pred, y_true, self.mode, 1.0)


class CEDiceLoss(nn.Module):
    """``CrossEntropyLoss()(x, t) + DiceLoss('multiclass')(x, t)`` in one reduction pass; t int64 [N,H,W] in [0, C)."""

    def forward(self, y_pred, y_true):
        return _apply(y_pred, y_true, "multiclass", 1.0)
