"""The other encoders of the reference's config: ``smp.Unet(encoder_name=...)`` for ``resnet18`` / ``resnet34`` / ``resnet50``.

The reference's ``build_model(encoder, weights)`` (train.py:357-379) passes ``cfg["encoder"]`` straight to ``smp.Unet``, and its
recommended config (train.py:747-749) lists ``'resnet18' / 'resnet34' / 'resnet50' / 'efficientnet-b0'``.  ``vk.Unet`` and
``vk.multiclass.Unet`` stay the resnet34 model; the class here is ``vk.multiclass.Unet`` with the wider encoder check::

    model = vk.encoders.Unet(encoder_name=cfg["encoder"], encoder_weights=None, in_channels=3, classes=1, activation=None)

resnet18 is the BasicBlock network with 2-2-2-2 blocks and runs on the resnet34 kernels; resnet50's Bottleneck blocks (1x1 -> 3x3 ->
1x1, expansion 4, the stride on the 3x3 as in torchvision v1.5) run their 36 pointwise convolutions on csrc/conv1x1.hip.  State-dict
keys, order and shapes are smp's; ``set_seed(s); vk.encoders.Unet(...)`` draws torchvision's and smp's initial weights in their order.
``efficientnet-b0`` is not implemented (NotImplementedError), nor are ImageNet weights (``encoder_weights`` other than None: VkError)."""
from __future__ import annotations

from typing import Optional

from . import multiclass as _multiclass

__all__ = ["Unet", "build_model", "ENCODERS"]

ENCODERS = ("resnet18", "resnet34", "resnet50")


class Unet(_multiclass.Unet):
    """``vk.multiclass.Unet`` (1 <= classes <= 16) with ``encoder_name`` in resnet18 / resnet34 / resnet50."""
    encoders = ENCODERS


def build_model(encoder: str = "resnet34", weights: Optional[str] = None) -> Unet:
    """Mirror of reference train.py:357-379 for any encoder of ``ENCODERS``."""
    return Unet(encoder_name=encoder, encoder_weights=weights, in_channels=3, classes=1, activation=None)
