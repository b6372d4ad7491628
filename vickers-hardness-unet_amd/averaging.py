"""Averaged weights: ``vk.ModelEMA`` (exponential moving average, timm's ``ModelEmaV2`` / torch's ``AveragedModel`` with
``get_ema_multi_avg_fn``) and ``vk.SWA`` (the equal-weight average of ``torch.optim.swa_utils.AveragedModel``) over the model's two flat
fp32 buffers: the parameters and the BatchNorm running statistics (torch's ``use_buffers=True``, timm's behaviour).

The average is two flat buffers and one element rule, ``a' = fma(p - a, w, a)`` (``w == 1``: a copy), whose weight ``w`` is resolved
on the device from a device counter::

    ema = vk.ModelEMA(model, decay=0.999, warmup=True)     # vk.SWA(model) for the equal-weight average
    opt = vk.adamw_for(model, lr); ema.attach(opt)         # opt.step() now also updates the average
    ...                                                    # or, unattached: opt.step(); ema.update()
    with ema.applied():                                    # the model holds the averaged weights
        val = validate(model)
    torch.save(ema.state_dict(), "best.pth")               # a plain model checkpoint, smp's keys

Attached, the whole-buffer AdamW step updates the average inside its own launch (``vk_adamw_step_amp_avg``: the updated parameter is
still in a register); the per-tensor / param-group / clipped step is followed by one ``vk_avg_update``.  Both give the bits of
``opt.step(); ema.update(found_inf)``.  ``applied()`` exchanges the model's buffers and the average in place (``vk_avg_swap``): no third
copy of the weights exists.

BatchNorm statistics are averaged with the parameters' rule; ``num_batches_tracked`` is left alone.  There is no ``update_bn`` pass:
the engine's BatchNorm momentum is fixed at 0.1 and torch's ``update_bn`` needs a cumulative average.  Data parallel: every rank holds
the same parameters after the all-reduced step, so every rank's average has the same bits; nothing is communicated.  No CPU fallback."""
from __future__ import annotations

import contextlib
from typing import Dict, Optional

import torch

from . import _lib
from ._lib import VkError, check, lib

_KINDS = {"ema": _lib.VK_AVG_EMA, "swa": _lib.VK_AVG_SWA}


class _Average:
    """The two flat buffers, the device counter and the rule; ``ModelEMA`` and ``SWA`` choose the rule."""

    kind = "ema"

    def __init__(self, model, decay: float, warmup: bool):
        decay = float(decay)
        if not 0.0 <= decay < 1.0:           # false for a NaN too
            raise ValueError("decay must be a number in [0, 1), got %r" % decay)
        flat = getattr(model, "_flat", None)
        if not isinstance(flat, dict) or "params" not in flat or "bufs" not in flat:
            raise VkError("an average is taken over the flat buffers of a vk.Unet, vk.multiclass.Unet or vk.encoders.Unet")
        if not model.flat_params.is_cuda:
            raise VkError("the model is on %s: no CPU fallback" % model.flat_params.device)
        self.model = model
        self.decay, self.warmup = decay, bool(warmup)
        self._params = flat["params"].detach().clone()
        self._bufs = flat["bufs"].detach().clone()
        dev = self._params.device
        self._count = torch.zeros(1, dtype=torch.int32, device=dev)      # updates taken (a skipped one does not count)
        self._scratch = torch.zeros(2, dtype=torch.float32, device=dev)
        self._optimizer = None
        self._applied = False

    # ------------------------------------------------------------------ state
    @property
    def device(self) -> torch.device:
        return self._params.device

    @property
    def updates(self) -> int:
        """Updates taken so far (reads the device counter: the one host sync of this class; for logging / checkpoints only)."""
        return int(self._count.item())

    def to(self, device) -> "_Average":
        """Move the average (after ``model.to(device)``: it does not follow the model by itself)."""
        self._params, self._bufs = self._params.to(device), self._bufs.to(device)
        self._count, self._scratch = self._count.to(device), self._scratch.to(device)
        return self

    def _rule(self) -> _lib.vk_avg_rule:
        return _lib.vk_avg_rule(_KINDS[self.kind], self.decay, 1 if self.warmup else 0)

    def _ranges(self):
        """The (average, model) ranges of both buffers, after checking that they still match."""
        f = self.model._flat
        p, b = f["params"], f["bufs"]
        if not p.is_cuda:
            raise VkError("the model is on %s: no CPU fallback" % p.device)
        if p.device != self._params.device:
            raise VkError("the model is on %s but its average is on %s: move it too (average.to(device))" % (p.device, self._params.device))
        if p.numel() != self._params.numel() or b.numel() != self._bufs.numel():
            raise VkError("the model's flat buffers hold %d + %d elements, the average %d + %d"
                          % (p.numel(), b.numel(), self._params.numel(), self._bufs.numel()))
        return (_lib.vk_avg_range * 2)(_lib.vk_avg_range(self._params.data_ptr(), p.data_ptr(), p.numel()),
                                       _lib.vk_avg_range(self._bufs.data_ptr(), b.data_ptr(), b.numel()))

    @staticmethod
    def _flag(found_inf, device) -> Optional[torch.Tensor]:
        if found_inf is None:
            return None
        if not isinstance(found_inf, torch.Tensor):
            raise VkError("found_inf must be a device tensor (a float here would have to come from a host sync)")
        return found_inf.reshape(-1)[:1].to(device=device, dtype=torch.float32)

    # ------------------------------------------------------------------ update
    def _update(self, found_inf: Optional[torch.Tensor]):
        """One vk_avg_update over both buffers (found_inf: None or float32[1] on the device)."""
        ranges = self._ranges()
        check(lib().vk_avg_update(2, ranges, self._rule(), self._count.data_ptr(), _lib.ptr(found_inf), self._scratch.data_ptr(),
                                  _lib.current_stream()), "vk_avg_update")

    @torch.no_grad()
    def update(self, found_inf: Optional[torch.Tensor] = None) -> None:
        """Move the average toward the model's current weights and statistics: one launch over both buffers, no host sync.
        ``found_inf`` (a GradScaler's device flag): a non-zero value skips the update and the counter, as it skips the step."""
        if self._optimizer is not None:
            raise VkError("this average is attached to an optimizer, whose step() updates it: update() would count the step twice")
        if self._applied:
            raise VkError("update() inside applied(): the model holds the average")
        self._update(self._flag(found_inf, self._params.device))

    def attach(self, optimizer) -> "_Average":
        """Make ``optimizer.step()`` (a ``FusedAdamW`` of this model) update the average as well, with the step's own ``found_inf``."""
        from .optim import FusedAdamW
        if not isinstance(optimizer, FusedAdamW):
            raise VkError("attach() takes a vk.FusedAdamW (vk.adamw_for(model, ...)); with another optimizer call update() after step()")
        if optimizer._model is not None and optimizer._model is not self.model:
            raise VkError("the optimizer is attached to another model")
        if self._optimizer is not None or optimizer._average is not None:
            raise VkError("already attached: detach() first (an optimizer carries one average)")
        optimizer._average = self
        self._optimizer = optimizer
        return self

    def detach(self) -> "_Average":
        if self._optimizer is not None:
            self._optimizer._average = None
            self._optimizer = None
        return self

    def _before_step(self, model):
        """FusedAdamW.step() with this average attached: refuse what would corrupt it, before anything is launched."""
        if model is not self.model:
            raise VkError("the optimizer is attached to another model than its average")
        if self._applied:
            raise VkError("optimizer.step() inside applied(): the model holds the average")
        self._ranges()

    # ------------------------------------------------------------------ evaluate with the average
    def _swap(self):
        check(lib().vk_avg_swap(2, self._ranges(), _lib.current_stream()), "vk_avg_swap")
        self.model.mark_weights_dirty()

    @contextlib.contextmanager
    def applied(self):
        """The model holds the averaged weights and statistics inside the block and its own again after it (also when the body
        raises): an in-place exchange on entry and on exit, and ``mark_weights_dirty()``.  Not re-entrant; no ``update()`` and no
        attached ``step()`` inside."""
        if self._applied:
            raise VkError("applied() is not re-entrant")
        self._swap()
        self._applied = True
        try:
            yield self.model
        finally:
            self._applied = False
            self._swap()

    @torch.no_grad()
    def copy_to(self, model=None) -> None:
        """Make the average the weights and statistics of ``model`` (default: the averaged model) for good."""
        if self._applied:
            raise VkError("copy_to() inside applied(): the model holds the average")
        model = self.model if model is None else model
        f = model._flat
        if f["params"].numel() != self._params.numel() or f["bufs"].numel() != self._bufs.numel():
            raise VkError("copy_to: the model's flat buffers do not have the average's sizes")
        f["params"].copy_(self._params)
        f["bufs"].copy_(self._bufs)
        model.mark_weights_dirty()

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """A plain model checkpoint of the averaged weights: the model's own keys and shapes (smp's), the averaged parameters and
        running statistics (views of the average, as ``nn.Module.state_dict`` returns views of the model) and a copy of the model's
        current ``num_batches_tracked``.  ``Unet.load_state_dict(strict=True)`` loads it."""
        m = self.model
        flat = {"params": self._params, "bufs": self._bufs}
        by_name = {}
        for name, kind, dims, off, numel in m._table:
            if kind == 0:
                K, Cc, R, S = dims
                by_name[name] = flat["params"][off:off + numel].view(K, R, S, Cc).permute(0, 3, 1, 2)
            elif kind == 1:
                by_name[name] = flat["params"][off:off + numel]
            elif kind == 2:
                by_name[name] = flat["bufs"][off:off + numel]
        out = {}
        for key, value in m.state_dict().items():
            out[key] = by_name[key].detach() if key in by_name else value.detach().clone()
        return out

    def averaging_state_dict(self) -> dict:
        """Everything needed to resume averaging: both flat buffers, the counter (a host sync), kind, decay and warmup."""
        return {"kind": self.kind, "decay": self.decay, "warmup": self.warmup, "updates": self.updates,
                "params": self._params, "bufs": self._bufs}

    def load_averaging_state_dict(self, sd: dict) -> None:
        if sd["kind"] != self.kind:
            raise VkError("this is a %s average, the state is of kind %r" % (self.kind, sd["kind"]))
        p, b = sd["params"], sd["bufs"]
        if p.numel() != self._params.numel() or b.numel() != self._bufs.numel() or p.dtype != torch.float32 or b.dtype != torch.float32:
            raise VkError("the state holds %d + %d elements, the model's flat buffers %d + %d (fp32)"
                          % (p.numel(), b.numel(), self._params.numel(), self._bufs.numel()))
        if self._applied:
            raise VkError("load_averaging_state_dict() inside applied(): the model holds the average")
        decay = float(sd["decay"])
        if not 0.0 <= decay < 1.0:
            raise ValueError("decay must be a number in [0, 1), got %r" % decay)
        self.decay, self.warmup = decay, bool(sd["warmup"])
        self._params.copy_(p.reshape(-1))
        self._bufs.copy_(b.reshape(-1))
        self._count.fill_(int(sd["updates"]))


class ModelEMA(_Average):
    """Exponential moving average of a model's weights and BatchNorm statistics: ``a' = a + (1 - decay_t)(p - a)``, with
    ``decay_t = decay``, or with ``warmup=True`` timm's ``min(decay, (1 + t) / (10 + t))`` at update ``t`` (1-based).  The average
    starts as a copy of the model."""

    kind = "ema"

    def __init__(self, model, decay: float = 0.999, warmup: bool = False):
        super().__init__(model, decay, warmup)


class SWA(_Average):
    """Stochastic weight averaging: the equal-weight mean of the model at every ``update()`` (``a' = a + (p - a) / t``; the first
    sample replaces the starting copy).  Usually updated once per epoch late in training, under ``torch.optim.swa_utils.SWALR``."""

    kind = "swa"

    def __init__(self, model):
        super().__init__(model, 0.0, False)
