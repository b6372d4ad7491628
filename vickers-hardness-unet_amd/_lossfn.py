"""What every loss front end of the package shares (``vk.losses``, ``vk.seglosses``, ``vk.lovasz`` and the fused step of ``Unet``): how a
target becomes what a kernel reads, how it is checked against the logits, and the one autograd function around a loss kernel."""
from __future__ import annotations

import torch

from ._lib import VkError

MAX_CLASSES = 16


def check_classes(mode: str, C: int) -> str:
    if mode == "binary" and C != 1:
        raise ValueError("mode 'binary' needs logits with one channel, got %d" % C)
    if mode == "multiclass" and C < 2:
        raise ValueError("mode 'multiclass' needs C >= 2 channels, got %d" % C)
    if not 1 <= C <= MAX_CLASSES:
        raise ValueError("expected 1 <= C <= %d classes, got %d" % (MAX_CLASSES, C))
    return mode


def check_target(shape, target: torch.Tensor, mode: str, who=None):
    """The target against logits of ``shape`` [N,C,H,W].  ``who`` is the message prefix of a caller that checks the multiclass target
    alone and leaves the sigmoid modes to ``marshal`` (the drop-ins of ``vk.losses``, the fused step)."""
    N, _, H, W = shape
    if mode == "multiclass":
        if tuple(target.shape) != (N, H, W) or target.dtype != torch.int64:
            raise ValueError("%s: target must be int64 [N,H,W]%s, got %s %s"
                             % (who or "mode 'multiclass'", "" if who else " = %s" % ((N, H, W),), target.dtype, tuple(target.shape)))
    elif who is None:
        try:
            ok = tuple(torch.broadcast_shapes(tuple(target.shape), tuple(shape))) == tuple(shape)
        except RuntimeError:
            ok = False
        if not ok:
            raise ValueError("mode %r: target must broadcast to the logits' shape %s, got %s" % (mode, tuple(shape), tuple(target.shape)))


def marshal(logits: torch.Tensor, target: torch.Tensor, multiclass: bool):
    """(contiguous fp32 logits, the target as the kernels read it): int64 [N,H,W] labels as they are, anything else as fp32 broadcast
    to the logits' shape."""
    x = logits.detach().contiguous().float()
    if multiclass:
        return x, target.detach().contiguous()
    return x, target.detach().float().expand_as(x).contiguous()


class LossFn(torch.autograd.Function):
    """``run(x, y, dl) -> (total, bad)`` launches the loss kernels on the marshalled inputs; they write d total / d logits into ``dl``
    (None: no gradient wanted).  ``total`` is a 0-dim device tensor, ``bad`` None or the 0-dim device count of multiclass labels that are
    neither a class nor ``ignore_index``: reading it back is the one host sync, and a count other than 0 raises VkError."""

    @staticmethod
    def forward(ctx, logits, target, run, multiclass, ignore_index):
        x, y = marshal(logits, target, multiclass)
        dl = torch.empty_like(x) if logits.requires_grad else None
        total, bad = run(x, y, dl)
        if bad is not None:
            bad = int(bad.item())
            if bad:
                raise VkError("multi-class target holds %d label(s) outside [0, %d)%s" % (
                    bad, x.shape[1], "" if ignore_index is None else " other than ignore_index=%d" % ignore_index))
        ctx.dl = dl
        ctx.in_dtype = logits.dtype
        return total.clone() if total._is_view() else total         # never a view into the kernels' result buffer

    @staticmethod
    def backward(ctx, g_total):
        return None if ctx.dl is None else (ctx.dl * g_total).to(ctx.in_dtype), None, None, None, None
