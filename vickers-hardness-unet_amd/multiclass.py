"""More than one class: ``smp.Unet(..., classes=C)`` for 1 <= C <= 16 and the multi-label / multi-class losses smp pairs with it.

``vk.Unet`` and ``vk.DiceLoss`` are the reference's binary drop-ins (train.py:372-378, 601) and keep refusing ``classes != 1`` and the
other loss modes; the classes here are the same objects with the wider contract::

    model = vk.multiclass.Unet(encoder_weights=None, classes=3)       # logits [N,3,H,W]
    dice = vk.multiclass.DiceLoss(mode="multiclass")                  # or "multilabel" / "binary"
    loss = nn.CrossEntropyLoss()(logits, t) + dice(logits, t)         # t int64 [N,H,W]
    model.loss_and_backward(x, t, mode="multiclass")                  # the fused step

The kernels are in csrc/multiclass.hip (vk_head_fwd_multi, vk_head_bwd_multi, vk_multilabel_loss, vk_multiclass_loss).

Validation and inference (multiclass_eval.py: csrc/multiclass_eval.hip, csrc/multiclass_post.hip)::

    mean_dice, mean_iou, dice_c, iou_c = vk.multiclass.seg_metrics(logits, t, mode="multiclass")
    probs = vk.multiclass.Segmenter(model, mode="multiclass").infer(bgr)      # fp32 [C, h, w]"""
from __future__ import annotations

from . import losses as _losses
from . import unet as _unet
from .losses import CEDiceLoss  # noqa: F401
from .multiclass_eval import (Segmenter, postprocess_labels, postprocess_masks, postprocess_probs, predict_mask,  # noqa: F401
                              seg_metrics, seg_metrics_device, seg_stats)

__all__ = ["Unet", "DiceLoss", "BCEDiceLoss", "CEDiceLoss", "seg_stats", "seg_metrics_device", "seg_metrics", "postprocess_labels",
           "postprocess_masks", "postprocess_probs", "predict_mask", "Segmenter"]


class Unet(_unet.Unet):
    """``vk.Unet`` with ``1 <= classes <= 16``: segmentation_head.0 is [C,16,3,3] + bias [C], forward returns fp32 [N,C,H,W]."""
    max_classes = 16


class DiceLoss(_losses.DiceLoss):
    """smp ``DiceLoss`` for mode "binary", "multilabel" (target fp32 [N,C,H,W]) or "multiclass" (target int64 [N,H,W] in [0, C))."""
    modes = ("binary", "multilabel", "multiclass")


class BCEDiceLoss(_losses.BCEDiceLoss):
    """``BCEWithLogitsLoss()(x, y) + DiceLoss(mode)(x, y)`` in one reduction pass, mode "binary" or "multilabel"."""
    modes = ("binary", "multilabel")
