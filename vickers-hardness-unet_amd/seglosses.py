"""``smp.losses`` (minus Lovasz and MCC, which live in ``vk.lovasz``) on one fused, deterministic device reduction: csrc/seg_loss.hip behind ``vk_seg_loss``.

Constructor signatures are smp's (and torch.nn's for the last two), so a training script changes only the import::

    from importlib import import_module
    L = import_module("vickers-hardness-unet_amd").seglosses
    loss = 0.5 * L.FocalLoss("multiclass", ignore_index=255) + L.TverskyLoss("multiclass", alpha=0.3, beta=0.7, ignore_index=255)
    loss(logits, t).backward()                       # ONE vk_seg_loss call for the whole sum
    model.loss_and_backward(x, t, loss=loss)         # the fused step (vk_unet_loss_cfg)

    DiceLoss, JaccardLoss, TverskyLoss(mode, classes, log_loss, from_logits, smooth, ignore_index, eps[, alpha, beta, gamma])
    FocalLoss(mode, alpha, gamma, ignore_index, ...)
    SoftBCEWithLogitsLoss(..., ignore_index, smooth_factor, pos_weight)      mean over ALL entries, ignored ones zeroed (smp)
    SoftCrossEntropyLoss(..., smooth_factor, ignore_index)                   mean over ALL pixels, ignored ones zeroed (smp)
    CrossEntropyLoss(ignore_index, label_smoothing), BCEWithLogitsLoss(pos_weight)        torch.nn semantics (mean over VALID)

``w * term`` and ``a + b`` build a ``LossSum``; the terms of a sum agree on ``mode`` and on ``ignore_index`` (a term that has none
takes the sum's) and each kind (pixel-wise, focal, dice, jaccard, tversky) appears at most once.  The mode-less pixel terms fit
themselves in: a BCE term is binary or multilabel, a cross-entropy term multiclass.  A term whose denominator is empty because every
entry is ignored is 0 (torch and smp give NaN there).  A multiclass label that is neither a class nor ``ignore_index`` raises VkError
from the modules and makes the fused step's values NaN.  What smp has and this module does not raises NotImplementedError naming the
argument.  ``vk.DiceLoss``, ``vk.multiclass.*`` and ``vk.losses.*`` are unchanged."""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from . import _lib, _lossfn
from ._lib import VkError, check, lib
from ._lossfn import MAX_CLASSES
from . import multiclass_eval as _mce

__all__ = ["DiceLoss", "JaccardLoss", "TverskyLoss", "FocalLoss", "SoftBCEWithLogitsLoss", "SoftCrossEntropyLoss", "CrossEntropyLoss",
           "BCEWithLogitsLoss", "LovaszLoss", "MCCLoss", "LossSum", "seg_metrics"]

MODES = ("binary", "multilabel", "multiclass")
KINDS = ("pix", "focal", "dice", "jaccard", "tversky", "mcc")          # bit i of vk_seg_loss_cfg.terms; "mcc": vk.lovasz.MCCLoss
_MODE_CODE = {"binary": _lib.VK_LOSS_BINARY, "multilabel": _lib.VK_LOSS_MULTILABEL, "multiclass": _lib.VK_LOSS_MULTICLASS}


def _check_mode(mode, who):
    if mode not in MODES:
        raise ValueError("%s: mode must be one of %s, got %r" % (who, " | ".join(repr(m) for m in MODES), mode))


def _check_ignore(ignore_index, who):
    if ignore_index is None:
        return None
    if isinstance(ignore_index, bool) or int(ignore_index) != ignore_index or not -2 ** 31 <= int(ignore_index) < 2 ** 31:
        raise ValueError("%s: ignore_index must be an integer that fits 32 bits, got %r" % (who, ignore_index))
    return int(ignore_index)


def _weight(w):
    """a loss weight as a float; None for what is no number"""
    if isinstance(w, bool) or not isinstance(w, (int, float)):
        return None
    if not math.isfinite(w):
        raise ValueError("loss weight must be finite, got %r" % (w,))
    return float(w)


class _Algebra:
    """``w * loss`` and ``loss_a + loss_b``"""

    def _as_sum(self) -> "LossSum":
        raise NotImplementedError

    def __add__(self, other):
        if isinstance(other, (int, float)) and not isinstance(other, bool) and other == 0:
            return self._as_sum()                       # sum([...]) starts from 0
        if not isinstance(other, _Algebra):
            return NotImplemented
        return LossSum(self._as_sum().terms + other._as_sum().terms)

    __radd__ = __add__

    def __mul__(self, w):
        w = _weight(w)
        if w is None:
            return NotImplemented
        return LossSum([(w * a, t) for a, t in self._as_sum().terms])

    __rmul__ = __mul__


class _Term(_Algebra, nn.Module):
    kind = ""
    bce = False            # a pixel term that is BCE (binary / multilabel) rather than cross-entropy

    def __init__(self, mode: Optional[str], ignore_index: Optional[int], opts: dict):
        super().__init__()
        self.mode = mode
        self.ignore_index = ignore_index
        self.opts = opts

    def _as_sum(self):
        return LossSum([(1.0, self)])

    def forward(self, y_pred, y_true):
        return self._as_sum()(y_pred, y_true)

    def spec(self, C: int) -> dict:
        return self._as_sum().spec(C)

    def cfg(self, C: int):
        return self._as_sum().cfg(C)

    def extra_repr(self):
        return "mode=%r, ignore_index=%r, %s" % (self.mode, self.ignore_index, ", ".join("%s=%r" % kv for kv in self.opts.items()))


def _region_opts(who, mode, classes, log_loss, from_logits, smooth, ignore_index, eps):
    _check_mode(mode, who)
    if not from_logits:
        raise NotImplementedError("%s(from_logits=False): the kernels take logits" % who)
    if classes is not None:
        classes = [int(c) for c in (classes.tolist() if isinstance(classes, torch.Tensor) else classes)]
        if not classes or min(classes) < 0 or max(classes) >= MAX_CLASSES:
            raise ValueError("%s: classes must name classes in [0, %d), got %r" % (who, MAX_CLASSES, classes))
        classes = sorted(set(classes))
    if not (math.isfinite(smooth) and smooth >= 0):
        raise ValueError("%s: smooth must be finite and >= 0, got %r" % (who, smooth))
    if not (math.isfinite(eps) and eps > 0):
        raise ValueError("%s: eps must be > 0, got %r" % (who, eps))
    return dict(smooth=float(smooth), eps=float(eps), log_loss=bool(log_loss), classes=classes), _check_ignore(ignore_index, who)


class DiceLoss(_Term):
    kind = "dice"

    def __init__(self, mode: str, classes=None, log_loss: bool = False, from_logits: bool = True, smooth: float = 0.0,
                 ignore_index: Optional[int] = None, eps: float = 1e-7):
        o, ign = _region_opts("DiceLoss", mode, classes, log_loss, from_logits, smooth, ignore_index, eps)
        super().__init__(mode, ign, o)


class JaccardLoss(_Term):
    kind = "jaccard"

    def __init__(self, mode: str, classes=None, log_loss: bool = False, from_logits: bool = True, smooth: float = 0.0,
                 eps: float = 1e-7, ignore_index: Optional[int] = None):
        o, ign = _region_opts("JaccardLoss", mode, classes, log_loss, from_logits, smooth, ignore_index, eps)
        super().__init__(mode, ign, o)


class TverskyLoss(_Term):
    kind = "tversky"

    def __init__(self, mode: str, classes=None, log_loss: bool = False, from_logits: bool = True, smooth: float = 0.0,
                 ignore_index: Optional[int] = None, eps: float = 1e-7, alpha: float = 0.5, beta: float = 0.5, gamma: float = 1.0):
        o, ign = _region_opts("TverskyLoss", mode, classes, log_loss, from_logits, smooth, ignore_index, eps)
        if not (math.isfinite(gamma) and gamma >= 1.0):
            raise NotImplementedError("TverskyLoss(gamma=%r): gamma must be >= 1 (below, the derivative is unbounded at a zero mean)"
                                      % (gamma,))
        if not (math.isfinite(alpha) and math.isfinite(beta)):
            raise ValueError("TverskyLoss: alpha and beta must be finite")
        o.update(alpha=float(alpha), beta=float(beta), gamma=float(gamma))
        super().__init__(mode, ign, o)


class FocalLoss(_Term):
    kind = "focal"

    def __init__(self, mode: str, alpha: Optional[float] = None, gamma: Optional[float] = 2.0, ignore_index: Optional[int] = None,
                 reduction: Optional[str] = "mean", normalized: bool = False, reduced_threshold: Optional[float] = None):
        _check_mode(mode, "FocalLoss")
        if reduction != "mean":
            raise NotImplementedError("FocalLoss(reduction=%r): only 'mean'" % (reduction,))
        if normalized:
            raise NotImplementedError("FocalLoss(normalized=True) is not implemented")
        if reduced_threshold is not None:
            raise NotImplementedError("FocalLoss(reduced_threshold=%r) is not implemented" % (reduced_threshold,))
        if gamma is None or not math.isfinite(gamma) or not (gamma == 0 or gamma >= 1.0):
            raise NotImplementedError("FocalLoss(gamma=%r): gamma must be 0 or >= 1 (in between, the derivative is unbounded where the "
                                      "prediction is exact)" % (gamma,))
        if alpha is not None and not math.isfinite(alpha):
            raise ValueError("FocalLoss: alpha must be finite")
        super().__init__(mode, _check_ignore(ignore_index, "FocalLoss"),
                         dict(alpha=None if alpha is None else float(alpha), gamma=float(gamma)))


def _pos_weight_list(pos_weight, who):
    if pos_weight is None:
        return None
    if isinstance(pos_weight, torch.Tensor):
        if pos_weight.dim() == 4 and (pos_weight.shape[0] != 1 or pos_weight.shape[2] != 1 or pos_weight.shape[3] != 1):
            raise ValueError("%s: pos_weight must be a scalar, [C] or [1,C,1,1], got %s" % (who, tuple(pos_weight.shape)))
        if pos_weight.dim() not in (0, 1, 4):
            raise ValueError("%s: pos_weight must be a scalar, [C] or [1,C,1,1], got %s" % (who, tuple(pos_weight.shape)))
        v = [float(a) for a in pos_weight.detach().reshape(-1).tolist()]
    elif isinstance(pos_weight, (int, float)):
        v = [float(pos_weight)]
    else:
        v = [float(a) for a in pos_weight]
    if not v or len(v) > MAX_CLASSES or not all(math.isfinite(a) for a in v):
        raise ValueError("%s: pos_weight must hold 1 or C finite values, got %r" % (who, v))
    return v


def _smooth_factor(sf, who):
    sf = 0.0 if sf is None else float(sf)
    if not 0.0 <= sf <= 1.0:
        raise ValueError("%s: label smoothing must lie in [0, 1], got %r" % (who, sf))
    return sf


class SoftBCEWithLogitsLoss(_Term):
    kind = "pix"
    bce = True

    def __init__(self, weight=None, ignore_index: Optional[int] = -100, reduction: str = "mean", smooth_factor: Optional[float] = None,
                 pos_weight=None):
        if weight is not None:
            raise NotImplementedError("SoftBCEWithLogitsLoss(weight=...): per-class weights are not implemented")
        if reduction != "mean":
            raise NotImplementedError("SoftBCEWithLogitsLoss(reduction=%r): only 'mean'" % (reduction,))
        who = "SoftBCEWithLogitsLoss"
        super().__init__(None, _check_ignore(ignore_index, who),
                         dict(smooth_factor=_smooth_factor(smooth_factor, who), pos_weight=_pos_weight_list(pos_weight, who), denom="all"))


class BCEWithLogitsLoss(_Term):
    """torch.nn.BCEWithLogitsLoss(pos_weight=...)"""
    kind = "pix"
    bce = True

    def __init__(self, pos_weight=None):
        super().__init__(None, None, dict(smooth_factor=0.0, pos_weight=_pos_weight_list(pos_weight, "BCEWithLogitsLoss"), denom="valid"))


class SoftCrossEntropyLoss(_Term):
    kind = "pix"

    def __init__(self, reduction: str = "mean", smooth_factor: Optional[float] = None, ignore_index: Optional[int] = -100, dim: int = 1):
        if reduction != "mean":
            raise NotImplementedError("SoftCrossEntropyLoss(reduction=%r): only 'mean'" % (reduction,))
        if dim != 1:
            raise NotImplementedError("SoftCrossEntropyLoss(dim=%r): the class dimension is 1" % (dim,))
        who = "SoftCrossEntropyLoss"
        super().__init__("multiclass", _check_ignore(ignore_index, who),
                         dict(smooth_factor=_smooth_factor(smooth_factor, who), pos_weight=None, denom="all"))


class CrossEntropyLoss(_Term):
    """torch.nn.CrossEntropyLoss(ignore_index=..., label_smoothing=...): mean over the valid pixels"""
    kind = "pix"

    def __init__(self, ignore_index: int = -100, label_smoothing: float = 0.0):
        who = "CrossEntropyLoss"
        super().__init__("multiclass", _check_ignore(ignore_index, who),
                         dict(smooth_factor=_smooth_factor(label_smoothing, who), pos_weight=None, denom="valid"))


def LovaszLoss(*a, **k):
    raise NotImplementedError("LovaszLoss needs a device sort and is not implemented here: use vk.lovasz.LovaszLoss")


def MCCLoss(*a, **k):
    raise NotImplementedError("MCCLoss is not implemented here: use vk.lovasz.MCCLoss")


class _Front:
    """What ``LossSum`` and ``vk.lovasz.LossSum`` share: the checks of a call and the autograd function around ``_run``."""

    def check_shapes(self, logits: torch.Tensor, target: torch.Tensor) -> str:
        if logits.dim() != 4:
            raise ValueError("expected logits [N,C,H,W], got %s" % (tuple(logits.shape),))
        mode = self.resolved_mode(logits.shape[1])
        _lossfn.check_target(logits.shape, target, mode)
        return mode

    def forward(self, y_pred, y_true):
        mode = self.check_shapes(y_pred, y_true)
        if not y_pred.is_cuda or not y_true.is_cuda:
            raise VkError("loss input is on %s / %s: no CPU fallback in this package" % (y_pred.device, y_true.device))
        if y_pred.dtype not in (torch.float32, torch.bfloat16, torch.float16):
            raise ValueError("logits must be fp32, bf16 or fp16, got %s" % y_pred.dtype)
        return _lossfn.LossFn.apply(y_pred, y_true, self._run, mode == "multiclass", self.ignore_index)


class LossSum(_Front, _Algebra, nn.Module):
    """A weighted sum of terms, computed by one ``vk_seg_loss`` call.  ``last_components``: device tensor
    [total, pix, focal, dice, jaccard, tversky] of the last call (unweighted term values, 0 for absent kinds; no host sync)."""

    def __init__(self, terms: Sequence[Tuple[float, _Term]]):
        super().__init__()
        terms = [(float(w), t) for w, t in terms]
        if not terms:
            raise ValueError("LossSum: no terms")
        seen = {}
        for _, t in terms:
            if t.kind in seen:
                raise ValueError("LossSum: two terms of kind %r (%s and %s); each kind appears at most once"
                                 % (t.kind, type(seen[t.kind]).__name__, type(t).__name__))
            seen[t.kind] = t
        modes = {}
        for _, t in terms:
            if t.mode is not None:
                modes.setdefault(t.mode, t)
        if len(modes) > 1:
            raise ValueError("LossSum: terms disagree on mode: " + ", ".join("%s is %r" % (type(t).__name__, m) for m, t in modes.items()))
        mode = next(iter(modes), None)
        if mode != "binary" and "mcc" in seen and mode is not None:
            raise ValueError("LossSum: MCCLoss is a binary loss and cannot join a sum of mode %r" % (mode,))
        if mode == "multiclass" and any(t.bce for _, t in terms):
            raise ValueError("LossSum: a BCE term cannot join a sum of mode 'multiclass' (use CrossEntropyLoss / SoftCrossEntropyLoss)")
        igns = {}
        for _, t in terms:
            if t.ignore_index is not None:
                igns.setdefault(t.ignore_index, t)
        if len(igns) > 1:
            raise ValueError("LossSum: terms disagree on ignore_index: "
                             + ", ".join("%s has %r" % (type(t).__name__, i) for i, t in igns.items()))
        self.terms: List[Tuple[float, _Term]] = terms
        self._mods = nn.ModuleList([t for _, t in terms])
        self.mode = mode
        self.ignore_index = next(iter(igns), None)
        self.last_components: Optional[torch.Tensor] = None

    def _as_sum(self):
        return self

    def resolved_mode(self, C: int) -> str:
        mode = self.mode if self.mode is not None else ("binary" if C == 1 else "multilabel")     # a BCE term alone: by C
        return _lossfn.check_classes(mode, C)

    def spec(self, C: int) -> dict:
        """The sum as plain data: dict(mode, ignore_index, terms={kind: dict(w=weight, **options)}) with the options resolved for C
        channels (``pos_weight`` as C floats or None, ``classes`` as a sorted list or None)."""
        out = dict(mode=self.resolved_mode(C), ignore_index=self.ignore_index, terms={})
        for w, t in self.terms:
            o = dict(t.opts, w=w)
            if t.kind == "pix" and o["pos_weight"] is not None:
                pw = o["pos_weight"]
                if len(pw) not in (1, C):
                    raise ValueError("pos_weight holds %d values for %d channels" % (len(pw), C))
                o["pos_weight"] = list(pw) * (C if len(pw) == 1 else 1)
            if o.get("classes") is not None and max(o["classes"]) >= C:
                raise ValueError("%s(classes=%r) names a class >= C = %d" % (type(t).__name__, o["classes"], C))
            out["terms"][t.kind] = o
        return out

    def cfg(self, C: int) -> "_lib.vk_seg_loss_cfg":
        """The ``vk_seg_loss_cfg`` of this sum for logits with C channels."""
        import ctypes
        s = self.spec(C)
        c = _lib.vk_seg_loss_cfg()
        c.struct_size = ctypes.sizeof(_lib.vk_seg_loss_cfg)
        c.mode = _MODE_CODE[s["mode"]]
        c.has_ignore = 0 if s["ignore_index"] is None else 1
        c.ignore_index = 0 if s["ignore_index"] is None else s["ignore_index"]
        terms = 0
        for k, o in s["terms"].items():
            terms |= 1 << KINDS.index(k)
            setattr(c, "w_" + k, o["w"])
            if k == "pix":
                c.pix_smooth = o["smooth_factor"]
                c.pix_denom_valid = 1 if o["denom"] == "valid" else 0
                if o["pos_weight"] is not None:
                    c.has_pos_weight = 1
                    for i, v in enumerate(o["pos_weight"]):
                        c.pos_weight[i] = v
            elif k == "focal":
                c.focal_has_alpha = 0 if o["alpha"] is None else 1
                c.focal_alpha = 0.0 if o["alpha"] is None else o["alpha"]
                c.focal_gamma = o["gamma"]
            elif k == "mcc":
                c.mcc_eps = o["eps"]
            else:
                setattr(c, k + "_smooth", o["smooth"])
                setattr(c, k + "_eps", o["eps"])
                setattr(c, k + "_log", 1 if o["log_loss"] else 0)
                setattr(c, k + "_classes", 0 if o["classes"] is None else sum(1 << i for i in o["classes"]))
                if k == "tversky":
                    c.tversky_alpha, c.tversky_beta, c.tversky_gamma = o["alpha"], o["beta"], o["gamma"]
        c.terms = terms
        return c

    def _run(self, x, y, dl):
        N, Cc, H, W = x.shape
        cfg = self.cfg(Cc)
        L = lib()
        ws = torch.empty(L.vk_seg_loss_workspace_bytes(N, Cc, H * W), dtype=torch.uint8, device=x.device)
        out = torch.empty(8, dtype=torch.float32, device=x.device)
        check(L.vk_seg_loss(cfg, N, Cc, H * W, x.data_ptr(), y.data_ptr(), ws.data_ptr(), ws.numel(), out.data_ptr(), _lib.ptr(dl), 1.0,
                            _lib.current_stream()), "vk_seg_loss")
        self.last_components = out[:6]
        return out[0], out[6] if cfg.mode == _lib.VK_LOSS_MULTICLASS else None

    def extra_repr(self):
        return "weights=%r, mode=%r, ignore_index=%r" % ([w for w, _ in self.terms], self.mode, self.ignore_index)


def as_loss_sum(loss) -> LossSum:
    if not isinstance(loss, _Algebra):
        raise TypeError("loss= takes a vk.seglosses term or LossSum, got %s" % type(loss).__name__)
    return loss._as_sum()


def seg_metrics(logits: torch.Tensor, target: torch.Tensor, mode: str, ignore_index: Optional[int] = None, threshold: float = 0.5,
                from_logits: bool = True, eps: float = 1e-7):
    """``vk.multiclass.seg_metrics`` with the pixels labelled ``ignore_index`` left out: (mean dice, mean iou, dice per class, iou per
    class).  Multiclass with ``ignore_index`` outside [0, C): the metrics kernel skips such labels already; here its skipped count
    must equal the number of ``ignore_index`` labels, anything else skipped is a bad label (VkError with the count)."""
    if ignore_index is None:
        return _mce.seg_metrics(logits, target, mode, threshold, from_logits, eps)
    ignore_index = _check_ignore(ignore_index, "seg_metrics")
    if mode != "multiclass":
        raise NotImplementedError("seg_metrics(mode=%r, ignore_index=...): only mode 'multiclass' takes ignore_index" % (mode,))
    if logits.dim() == 4 and 0 <= ignore_index < logits.shape[1]:
        raise NotImplementedError("seg_metrics(ignore_index=%d) inside [0, C = %d) is not implemented" % (ignore_index, logits.shape[1]))
    out, _, bad_d = _mce._run_metrics(logits, target, mode, threshold, from_logits, eps)
    n_ign = (target == ignore_index).sum()
    v = out.to("cpu", non_blocking=True)
    bad = int(bad_d.item()) - int(n_ign.item())
    c = int(logits.shape[1])
    if bad:
        raise VkError("multiclass target holds %d label(s) outside [0, %d) other than ignore_index=%d" % (bad, c, ignore_index))
    v = v.tolist()
    return v[0], v[1], v[2:2 + c], v[2 + c:2 + 2 * c]
