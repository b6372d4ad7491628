"""The two members of ``smp.losses`` that ``vk.seglosses`` leaves out: ``LovaszLoss`` on a stable device radix sort (csrc/lovasz.hip
behind ``vk_lovasz_loss``) and ``MCCLoss`` as a sixth kind of the fused ``vk_seg_loss`` reduction::

    from importlib import import_module
    vk = import_module("vickers-hardness-unet_amd")
    loss = vk.seglosses.BCEWithLogitsLoss() + vk.lovasz.LovaszLoss("binary")
    loss(logits, y).backward()                      # vk_seg_loss, then vk_lovasz_loss adding into the same gradient
    model.loss_and_backward(x, y, loss=loss)        # the fused step (vk_unet_loss_lovasz)

    LovaszLoss(mode, per_image=False, ignore_index=None, from_logits=True)
    MCCLoss(eps=1e-5)                               # binary; sums with the vk.seglosses terms in one pass

Lovasz hinge (binary, multilabel): e = 1 - x (2 y - 1), sorted descending (equal errors by ascending flat index: a stable sort, which
fixes the gradient among ties), loss = sum_k relu(e_(k)) dJ_k with the Jaccard increments dJ of the sorted labels, over the whole batch
or per image and averaged.  Lovasz softmax (multiclass): per class present among the valid labels, e = |[t == c] - softmax(x)_c|, the
same sum; mean over the present classes.  Entries equal to ``ignore_index`` are left out.  A segment without a valid entry is 0.

``MCCLoss`` deviates from smp in one point: smp's MCCLoss feeds its input through unchanged (it expects probabilities); this package's
kernels take logits, so p = sigmoid(x) here.

``w * lovasz``, ``lovasz + seg_term_or_sum`` and ``seg_term_or_sum + lovasz`` build a ``vk.lovasz.LossSum``: an optional
``vk.seglosses.LossSum`` and one weighted Lovasz term that agree on mode and ``ignore_index`` under the rules of ``vk.seglosses``.
Data-parallel training: the loss is batch-local per rank, like Dice.  Refused: ``from_logits=False``, MCC outside binary mode, more
than 2^31 - 1 logits in one call, CPU tensors (no CPU fallback)."""
from __future__ import annotations

import ctypes
import math
from typing import Optional

import torch
import torch.nn as nn

from . import _lib, _lossfn, seglosses
from ._lib import VkError, check, lib

__all__ = ["LovaszLoss", "MCCLoss", "LossSum"]

MAX_ENTRIES = 2 ** 31 - 1


class MCCLoss(seglosses._Term):
    """1 - Matthews correlation of sigmoid(logits) against a 0/1 target (mode 'binary'), from the sums of the fused reduction."""
    kind = "mcc"

    def __init__(self, eps: float = 1e-5):
        if not (isinstance(eps, (int, float)) and math.isfinite(eps) and eps > 0):
            raise ValueError("MCCLoss: eps must be > 0, got %r" % (eps,))
        super().__init__("binary", None, dict(eps=float(eps)))


class _LovaszAlgebra:
    def _as_lovasz_sum(self) -> "LossSum":
        raise NotImplementedError

    def __add__(self, other):
        if isinstance(other, (int, float)) and not isinstance(other, bool) and other == 0:
            return self._as_lovasz_sum()
        me = self._as_lovasz_sum()
        if isinstance(other, _LovaszAlgebra):
            raise ValueError("two Lovasz terms in one sum: a sum holds at most one")
        if not isinstance(other, seglosses._Algebra):
            return NotImplemented
        seg = other._as_sum() if me.seg is None else me.seg + other
        return LossSum(seg, me.w, me.term)

    __radd__ = __add__

    def __mul__(self, w):
        w = seglosses._weight(w)
        if w is None:
            return NotImplemented
        me = self._as_lovasz_sum()
        return LossSum(None if me.seg is None else w * me.seg, w * me.w, me.term)

    __rmul__ = __mul__


class LovaszLoss(_LovaszAlgebra, nn.Module):
    def __init__(self, mode: str, per_image: bool = False, ignore_index: Optional[int] = None, from_logits: bool = True):
        super().__init__()
        seglosses._check_mode(mode, "LovaszLoss")
        if not from_logits:
            raise NotImplementedError("LovaszLoss(from_logits=False): the kernels take logits")
        self.mode = mode
        self.per_image = bool(per_image)
        self.ignore_index = seglosses._check_ignore(ignore_index, "LovaszLoss")
        self._sum = None

    def _as_lovasz_sum(self):
        return LossSum(None, 1.0, self)

    def cfg(self, C: int):
        return self._as_lovasz_sum().lovasz_cfg(C)

    def forward(self, y_pred, y_true):
        if self._sum is None:
            object.__setattr__(self, "_sum", self._as_lovasz_sum())       # keeps the workspace cache; not a submodule (no cycle)
        return self._sum(y_pred, y_true)

    def extra_repr(self):
        return "mode=%r, per_image=%r, ignore_index=%r" % (self.mode, self.per_image, self.ignore_index)


class LossSum(seglosses._Front, _LovaszAlgebra, nn.Module):
    """``seg`` (a ``vk.seglosses.LossSum`` or None) + ``w`` * ``term`` (a ``LovaszLoss``).  ``last_components``: device tensor
    [total, pix, focal, dice, jaccard, tversky, mcc, lovasz] of the last call (unweighted term values; no host sync)."""

    def __init__(self, seg, w: float, term: LovaszLoss):
        super().__init__()
        if not isinstance(term, LovaszLoss):
            raise TypeError("vk.lovasz.LossSum: the Lovasz term must be a LovaszLoss, got %s" % type(term).__name__)
        w = seglosses._weight(w)
        if w is None:
            raise TypeError("vk.lovasz.LossSum: the weight must be a number")
        ign = term.ignore_index
        if seg is not None:
            if not isinstance(seg, seglosses._Algebra):
                raise TypeError("vk.lovasz.LossSum: seg must be a vk.seglosses term or sum, got %s" % type(seg).__name__)
            seg = seglosses.LossSum(seg._as_sum().terms)            # a copy: the mode and ignore_index of the whole sum go into it
            if seg.mode is not None and seg.mode != term.mode:
                raise ValueError("LossSum: terms disagree on mode: the vk.seglosses part is %r, LovaszLoss is %r" % (seg.mode, term.mode))
            if term.mode == "multiclass" and any(t.bce for _, t in seg.terms):
                raise ValueError("LossSum: a BCE term cannot join a sum of mode 'multiclass' (use CrossEntropyLoss / SoftCrossEntropyLoss)")
            if seg.ignore_index is not None and ign is not None and seg.ignore_index != ign:
                raise ValueError("LossSum: terms disagree on ignore_index: the vk.seglosses part has %r, LovaszLoss has %r"
                                 % (seg.ignore_index, ign))
            ign = ign if ign is not None else seg.ignore_index
            seg.mode = term.mode
            seg.ignore_index = ign
        self.seg = seg
        self.w = w
        self.term = term
        self.mode = term.mode
        self.ignore_index = ign
        self.last_components: Optional[torch.Tensor] = None
        self._ws = {}

    def _as_lovasz_sum(self):
        return self

    def resolved_mode(self, C: int) -> str:
        return _lossfn.check_classes(self.mode, C)

    def lovasz_cfg(self, C: int) -> "_lib.vk_lovasz_cfg":
        c = _lib.vk_lovasz_cfg()
        c.struct_size = ctypes.sizeof(_lib.vk_lovasz_cfg)
        c.mode = seglosses._MODE_CODE[self.resolved_mode(C)]
        c.per_image = 1 if self.term.per_image else 0
        c.has_ignore = 0 if self.ignore_index is None else 1
        c.ignore_index = 0 if self.ignore_index is None else self.ignore_index
        return c

    def seg_cfg(self, C: int):
        return None if self.seg is None else self.seg.cfg(C)

    def workspace(self, lcfg, N: int, C: int, HW: int, device) -> torch.Tensor:
        """the device scratch of vk_lovasz_loss for this shape (cached per shape)"""
        if N * C * HW > MAX_ENTRIES:
            raise VkError("LovaszLoss: %d logits in one call, at most 2^31 - 1" % (N * C * HW))
        key = (N, C, HW, str(device))
        ws = self._ws.get(key)
        if ws is None:
            nbytes = lib().vk_lovasz_workspace_bytes(lcfg, N, C, HW)
            if nbytes == 0:
                raise VkError("vk_lovasz_workspace_bytes refuses N=%d C=%d HW=%d" % (N, C, HW))
            ws = self._ws[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
        return ws

    def _run(self, x, y, dl):
        N, Cc, H, W = x.shape
        HW = H * W
        lcfg = self.lovasz_cfg(Cc)
        L = lib()
        st = _lib.current_stream()
        out = torch.zeros(12, dtype=torch.float32, device=x.device)
        if self.seg is not None:
            sws = torch.empty(L.vk_seg_loss_workspace_bytes(N, Cc, HW), dtype=torch.uint8, device=x.device)
            check(L.vk_seg_loss(self.seg.cfg(Cc), N, Cc, HW, x.data_ptr(), y.data_ptr(), sws.data_ptr(), sws.numel(), out.data_ptr(),
                                _lib.ptr(dl), 1.0, st), "vk_seg_loss")
        ws = self.workspace(lcfg, N, Cc, HW, x.device)
        check(L.vk_lovasz_loss(lcfg, N, Cc, HW, x.data_ptr(), y.data_ptr(), ws.data_ptr(), ws.numel(), out[8:].data_ptr(), _lib.ptr(dl),
                               self.w, 1 if self.seg is not None else 0, st), "vk_lovasz_loss")
        total = out[0] + self.w * out[8]
        self.last_components = torch.cat([total.reshape(1), out[1:6], out[7:9]])
        return total, out[9] if lcfg.mode == _lib.VK_LOSS_MULTICLASS else None

    def extra_repr(self):
        return "w_lovasz=%r, mode=%r, ignore_index=%r" % (self.w, self.mode, self.ignore_index)
