"""``FusedAdamW`` — ``torch.optim.AdamW(model.parameters(), lr, weight_decay=1e-4)`` (reference
train.py:606) as ONE HIP launch over the model's flat fp32 parameter / gradient / moment buffers.

It is a real ``torch.optim.Optimizer``, so ``CosineAnnealingLR`` (train.py:607),
``optimizer.param_groups[0]["lr"]`` (train.py:656), ``zero_grad(set_to_none=True)`` (train.py:428) and
``GradScaler.step(optimizer)`` (train.py:444) work unchanged.  Arithmetic follows
torch/optim/adam.py's single-tensor path (decoupled decay, bias-corrected).

GradScaler (train.py:441-445, 610-611): the optimizer declares ``_step_supports_amp_scaling``, so
``scaler.step(optimizer)`` hands it the scale and the overflow flag as DEVICE tensors
(``optimizer.grad_scale`` / ``optimizer.found_inf``); ``vk_adamw_step_amp`` reads both on the device,
folds the unscale into the update, skips the whole step on an overflow and keeps its step counter on the
device — no ``.item()``, no host round trip.  ``vk.GradScaler`` (below) additionally replaces torch's
foreach inf check over the 140 gradient views by one pass over the flat buffer.

Fine-tuning (frozen tensors, or an optimizer over a subset of the model's parameters): like torch, a step updates only the owned
tensors that have a gradient, and each tensor keeps its own step count (torch's per-parameter ``state["step"]``), so a tensor that
is unfrozen later starts its bias correction at step 1.  That is the per-tensor step: one segment per tensor, its tables built once
per set of tensors.  As long as every step has covered every tensor, the whole-buffer kernel and its one counter run.

Param groups (``FusedAdamW([dict(params=..., lr=...), ...])``, at most ``VK_ADAMW_MAX_GROUPS``; ``vk.finetune_groups`` builds the usual
ones): every tensor takes ``lr``, ``betas``, ``eps`` and ``weight_decay`` from its group, in the same two launches
(``vk_adamw_step_groups``).  ``clip_grad_norm_`` computes the global norm of the owned gradients in one read of them and leaves the clip
coefficient on the device for the next ``step()``, which folds it into its gradient factor: **``p.grad`` is not rewritten** (torch
scales the gradients in place; here they keep their unclipped values), there is no second pass and no host sync.  Which kernel a
``step()`` launches: one group, no pending coefficient, every tensor active and no per-tensor counters yet -> ``vk_adamw_step_amp``
(what ``vk.adamw_for(model, lr, wd)`` has always launched); anything else -> ``vk_adamw_step_groups`` over the active tensors (with one
group its group table holds zeros).  Both run the same element function, so the same values give the same bits.

Averaged weights: a ``vk.ModelEMA`` / ``vk.SWA`` attached with ``average.attach(optimizer)`` is updated by every ``step()`` with the
step's own ``found_inf``: inside the whole-buffer launch (``vk_adamw_step_amp_avg``), or by one ``vk_avg_update`` after
``vk_adamw_step_groups``.  Without one, ``step()`` launches what it always has."""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional, Tuple

import torch

from . import _lib
from ._lib import VkError, check, lib


class FusedAdamW(torch.optim.Optimizer):
    # torch.amp.GradScaler: pass grad_scale / found_inf as attributes instead of unscaling + syncing on the host
    _step_supports_amp_scaling = True

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 amsgrad: bool = False):
        if amsgrad:
            raise NotImplementedError("amsgrad is not used by the reference")
        params = list(params)
        if not params:
            raise VkError("FusedAdamW takes model.parameters() of one vickers-hardness-unet_amd.Unet, a subset of them, or a list of "
                          "param-group dicts over them")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        self._model = None
        super().__init__(params, defaults)      # calls add_param_group once per group
        self._m = self._v = None
        self._step_dev = None           # int32[1] on the device: optimizer steps actually taken (skipped AMP steps do not count)
        self._scratch = None            # float32[4] device scratch of vk_adamw_step_amp
        self._pending_step = 0          # step count loaded from a state dict before the device buffers exist
        self.grad_inv_scale = 1.0       # extra factor applied to gradients inside the kernel (DP averaging)
        # per-tensor steps (fine-tuning): int32 [tensors] on the device, created from _step_dev by the first step that leaves a tensor
        # out; from then on every step runs the per-tensor kernel.  None while every step has covered every tensor.
        self._steps_dev: Optional[torch.Tensor] = None
        self._pending_steps: Optional[List[int]] = None     # per-tensor counts loaded from a state dict
        self._owned: List[Tuple[int, torch.nn.Parameter]] = []   # (tensor index in the model's table, parameter)
        self._seg_key = None            # (tensor indices, device) the segment / block tables below were built for
        self._seg = self._blocks = self._seg_scratch = None
        self._nblocks = 0
        # param groups: group index per tensor index, and the device table of it in the order of the active tensors
        self._group_of: Dict[int, int] = {}
        self._grouping = 0              # bumped whenever _group_of is rebuilt
        self._grp_key = None            # (tensor indices, device, _grouping) _seg_group was built for
        self._seg_group = None
        # clip_grad_norm_: float32[1] on the device, consumed (taken or skipped) by the next step(), dropped by zero_grad()
        self._clip_coef: Optional[torch.Tensor] = None
        self._norm_partials = None      # float64 [blocks] scratch of vk_grad_norm_segments
        self._average = None            # a vk.ModelEMA / vk.SWA that every step() updates (its attach()); None: steps as ever

    def add_param_group(self, param_group):
        if len(self.param_groups) >= _lib.VK_ADAMW_MAX_GROUPS:
            raise VkError("FusedAdamW supports at most VK_ADAMW_MAX_GROUPS = %d param groups" % _lib.VK_ADAMW_MAX_GROUPS)
        if isinstance(param_group, dict) and param_group.get("amsgrad"):
            raise NotImplementedError("amsgrad is not used by the reference")
        if self._model is not None:       # a group added after attach(): same model (checked before torch adds it), new grouping
            ps = param_group["params"]
            ps = [ps] if isinstance(ps, torch.Tensor) else list(ps)
            known = {id(p) for p in self._model._param_list}
            if not all(id(p) in known for p in ps):
                raise VkError("FusedAdamW must own parameters of the attached model: the new group holds a tensor of another model")
            param_group = dict(param_group, params=ps)
        super().add_param_group(param_group)
        if self._model is not None:
            self.attach(self._model)

    def attach(self, model) -> "FusedAdamW":
        """Bind to the Unet whose parameters were passed (all of them or a subset, in any number of groups; needed to reach its flat
        buffers)."""
        index = {id(p): i for i, p in enumerate(model._param_list)}
        owned, group_of = [], {}
        for gi, grp in enumerate(self.param_groups):
            for p in grp["params"]:
                if id(p) not in index:
                    raise VkError("FusedAdamW must own parameters of the attached model (all of them or a subset): group %d holds "
                                  "a tensor of another model" % gi)
                owned.append((index[id(p)], p))
                group_of[index[id(p)]] = gi
        self._model = model
        self._owned = sorted(owned, key=lambda o: o[0])
        self._group_of = group_of
        self._grouping += 1
        self._seg_key = self._grp_key = None
        return self

    def _find_model(self):
        if self._model is None:
            raise VkError("call FusedAdamW.attach(model) (or use vk.adamw_for(model, ...)) before step()")
        return self._model

    @property
    def step_count(self) -> int:
        """Optimizer steps taken so far — with per-tensor counts the largest of them (reads the device counter: a host sync; for
        logging / checkpoints only)."""
        if self._steps_dev is not None:
            return int(self._steps_dev.max().item())
        if self._pending_steps is not None:
            return max(self._pending_steps)
        return int(self._step_dev.item()) if self._step_dev is not None else int(self._pending_step)

    def tensor_steps(self) -> List[int]:
        """Steps taken per parameter tensor of the attached model (its table order = ``model.parameters()``; a host sync)."""
        n = len(self._find_model()._param_list)
        if self._steps_dev is not None:
            return [int(v) for v in self._steps_dev.cpu()]
        if self._pending_steps is not None:
            return list(self._pending_steps)
        return [self.step_count] * n

    def _ensure_state(self, p: torch.Tensor):
        dev = p.device
        if self._m is None:
            self._m = torch.zeros_like(p)
            self._v = torch.zeros_like(p)
        elif self._m.device != dev:
            # moments loaded from a checkpoint mapped elsewhere, or the model moved: move them, never re-zero them silently
            self._m = self._m.to(dev)
            self._v = self._v.to(dev)
        if self._m.shape != p.shape:
            raise VkError("optimizer state does not match the model's flat parameter buffer")
        if self._step_dev is None or self._step_dev.device != dev:
            start = self.step_count if self._steps_dev is None and self._pending_steps is None else 0
            self._step_dev = torch.full((1,), start, dtype=torch.int32, device=dev)
            self._scratch = torch.zeros(4, dtype=torch.float32, device=dev)
        if self._pending_steps is not None:
            if len(self._pending_steps) != len(self._find_model()._param_list):
                raise VkError("optimizer state holds %d per-tensor steps, the model has %d tensors"
                              % (len(self._pending_steps), len(self._find_model()._param_list)))
            self._steps_dev = torch.tensor(self._pending_steps, dtype=torch.int32, device=dev)
            self._pending_steps = None
        elif self._steps_dev is not None and self._steps_dev.device != dev:
            self._steps_dev = self._steps_dev.to(dev)

    @torch.no_grad()
    def zero_grad(self, set_to_none: bool = True):
        # p.grad = None for API fidelity; the flat buffer itself is zeroed lazily by the next backward
        super().zero_grad(set_to_none=True)
        self._clip_coef = None          # a coefficient belongs to the gradients it was computed from

    @torch.no_grad()
    def step(self, closure=None, found_inf: torch.Tensor | None = None, grad_scale: torch.Tensor | None = None):
        if closure is not None:
            raise NotImplementedError("closure is not used by the reference")
        m = self._find_model()
        p, g = m.flat_params, m.flat_grads
        if not p.is_cuda:
            raise VkError("parameters are on %s: no CPU fallback" % p.device)
        # torch updates the parameters that have a gradient (frozen ones have none after a backward)
        avg = self._average
        if avg is not None:
            avg._before_step(m)         # raises inside applied(), or when the average no longer matches the model
        # GradScaler support: torch sets these attributes around step() (device tensors; never read on the host here)
        fi = found_inf if found_inf is not None else getattr(self, "found_inf", None)
        gs = grad_scale if grad_scale is not None else getattr(self, "grad_scale", None)
        if gs is not None and not isinstance(gs, torch.Tensor):
            raise VkError("grad_scale must be a device tensor (a float here would have to come from a host sync)")
        if fi is not None:
            fi = fi.reshape(-1)[:1].to(device=p.device, dtype=torch.float32)
        if gs is not None:
            gs = gs.reshape(-1)[:1].to(device=p.device, dtype=torch.float32)
        active = tuple(t for t, q in self._owned if q.grad is not None)
        if not active:
            if any(q.requires_grad for _, q in self._owned):
                raise VkError("optimizer.step() before backward(): gradients are None (zero_grad(set_to_none=True) was the last call)")
            if avg is not None:         # every owned tensor is frozen: the step moves nothing, the average still takes its sample
                avg._update(fi)
            return None
        self._ensure_state(p)
        clip, self._clip_coef = self._clip_coef, None       # consumed by this step, whether found_inf lets it be taken or not
        if len(self.param_groups) > 1 or clip is not None or len(active) < len(m._param_list) or self._steps_dev is not None:
            self._step_groups(m, active, gs, fi, clip)
            if avg is not None:         # tensors without a gradient move toward their current value too: the table kernel skips them
                avg._update(fi)
        else:                                                 # one group, every tensor, one counter: the whole buffer
            grp = self.param_groups[0]
            hp = (float(grp["lr"]), float(grp["betas"][0]), float(grp["betas"][1]), float(grp["eps"]), float(grp["weight_decay"]))
            if avg is None:
                check(lib().vk_adamw_step_amp(p.numel(), p.data_ptr(), g.data_ptr(), self._m.data_ptr(), self._v.data_ptr(), *hp,
                                              self._step_dev.data_ptr(), float(self.grad_inv_scale), _lib.ptr(gs), _lib.ptr(fi),
                                              self._scratch.data_ptr(), 0, 0, _lib.current_stream()),
                      "vk_adamw_step_amp")
            else:                                             # the same step, the average updated by the same launch
                bufs = m._flat["bufs"]
                check(lib().vk_adamw_step_amp_avg(p.numel(), p.data_ptr(), g.data_ptr(), self._m.data_ptr(), self._v.data_ptr(), *hp,
                                                  self._step_dev.data_ptr(), float(self.grad_inv_scale), _lib.ptr(gs), _lib.ptr(fi),
                                                  self._scratch.data_ptr(), 0, 0, avg._params.data_ptr(), avg._count.data_ptr(),
                                                  avg._rule(), avg._scratch.data_ptr(), avg._bufs.data_ptr(), bufs.data_ptr(),
                                                  bufs.numel(), _lib.current_stream()),
                      "vk_adamw_step_amp_avg")
        m.mark_weights_dirty()
        return None

    def _tables(self, m, active: Tuple[int, ...]):
        """Segment and block tables of the tensors in `active` (one segment each), shared by the per-tensor step and the gradient
        norm."""
        dev = m.flat_params.device
        L = lib()
        if self._seg_key != (active, dev):    # the set of tensors changed: new tables (the only host -> device copies)
            seg = torch.tensor([[m._param_ranges[t][0], m._param_ranges[t][0] + m._param_ranges[t][1], t] for t in active],
                               dtype=torch.int64)
            seg_p = C.cast(seg.data_ptr(), C.POINTER(C.c_int64))
            nb = L.vk_adamw_segment_blocks(len(active), seg_p, None, 0)
            if nb < 0:
                check(nb, "vk_adamw_segment_blocks")
            blocks = torch.empty((nb, 2), dtype=torch.int32)
            rc = L.vk_adamw_segment_blocks(len(active), seg_p, C.cast(blocks.data_ptr(), C.POINTER(C.c_int32)), nb)
            if rc < 0:
                check(rc, "vk_adamw_segment_blocks")
            self._seg, self._blocks = seg.to(dev), blocks.to(dev)
            self._seg_scratch = torch.zeros(4 + 2 * len(active), dtype=torch.float32, device=dev)
            self._norm_partials = None
            self._nblocks = nb
            self._seg_key = (active, dev)

    def _step_groups(self, m, active: Tuple[int, ...], gs, fi, clip):
        """vk_adamw_step_groups over the tensors in `active`: each with its group's hyper-parameters, the gradient factor times the
        pending clip coefficient (read on the device)."""
        p, g = m.flat_params, m.flat_grads
        dev = p.device
        if self._steps_dev is None:        # first per-tensor step: every tensor has taken the steps of the shared counter so far
            self._steps_dev = self._step_dev.repeat(len(m._param_list))
        self._tables(m, active)
        if self._grp_key != (active, dev, self._grouping):     # the set of tensors or the grouping changed
            self._seg_group = torch.tensor([self._group_of[t] for t in active], dtype=torch.int32).to(dev)
            self._grp_key = (active, dev, self._grouping)
        groups = self.param_groups
        hp = (_lib.vk_adamw_group * len(groups))(*[
            _lib.vk_adamw_group(float(q["lr"]), float(q["betas"][0]), float(q["betas"][1]), float(q["eps"]), float(q["weight_decay"]))
            for q in groups])
        check(lib().vk_adamw_step_groups(len(active), self._seg.data_ptr(), self._seg_group.data_ptr(), self._nblocks,
                                         self._blocks.data_ptr(), p.data_ptr(), g.data_ptr(), self._m.data_ptr(), self._v.data_ptr(),
                                         len(groups), hp, self._steps_dev.data_ptr(), float(self.grad_inv_scale), _lib.ptr(gs),
                                         _lib.ptr(fi), _lib.ptr(clip), self._seg_scratch.data_ptr(), _lib.current_stream()),
              "vk_adamw_step_groups")

    @torch.no_grad()
    def clip_grad_norm_(self, max_norm: float, norm_type: float = 2.0, error_if_nonfinite: bool = False) -> torch.Tensor:
        """``torch.nn.utils.clip_grad_norm_`` over the owned tensors that have a gradient, in one read of them
        (``vk_grad_norm_segments``).  Returns the total norm of ``grad_inv_scale * grad`` as a 0-dim fp32 device tensor, without a
        host sync.  The clip coefficient ``min(max_norm / (total + 1e-6), 1)`` stays on the device and multiplies the gradients inside
        the next ``step()`` of this optimizer (taken or skipped); ``zero_grad()`` discards it.  **Unlike torch, ``p.grad`` is not
        rewritten**: it keeps the unclipped values.  With a GradScaler: ``scaler.unscale_(opt); opt.clip_grad_norm_(m);
        scaler.step(opt); scaler.update()``."""
        if error_if_nonfinite:
            raise NotImplementedError("error_if_nonfinite needs a host sync: test the returned tensor instead")
        norm_type = float(norm_type)
        if norm_type == 2.0:
            kind = _lib.VK_NORM_L2
        elif norm_type == math.inf:
            kind = _lib.VK_NORM_INF
        else:
            raise NotImplementedError("clip_grad_norm_: norm_type must be 2 or inf, got %r" % norm_type)
        max_norm = float(max_norm)
        if not max_norm >= 0.0:
            raise ValueError("clip_grad_norm_: max_norm must be a number >= 0, got %r" % max_norm)
        m = self._find_model()
        g = m.flat_grads
        if not g.is_cuda:
            raise VkError("gradients are on %s: no CPU fallback" % g.device)
        active = tuple(t for t, q in self._owned if q.grad is not None)
        if not active:                     # torch: the norm of no gradients is 0 and nothing is clipped
            self._clip_coef = None
            return torch.zeros((), dtype=torch.float32, device=g.device)
        self._tables(m, active)
        if self._norm_partials is None:
            self._norm_partials = torch.empty(self._nblocks, dtype=torch.float64, device=g.device)
        out = torch.empty(2, dtype=torch.float32, device=g.device)      # fresh: the caller keeps out[0], the next step reads out[1]
        check(lib().vk_grad_norm_segments(len(active), self._seg.data_ptr(), self._nblocks, self._blocks.data_ptr(), g.data_ptr(), kind,
                                          float(self.grad_inv_scale), max_norm, self._norm_partials.data_ptr(), out.data_ptr(),
                                          _lib.current_stream()),
              "vk_grad_norm_segments")
        self._clip_coef = out[1:2]
        return out[0]

    def state_dict(self):
        sd = super().state_dict()
        sd["fused"] = {"step": self.step_count, "exp_avg": self._m, "exp_avg_sq": self._v}
        if self._steps_dev is not None or self._pending_steps is not None:
            sd["fused"]["steps"] = self.tensor_steps()      # per tensor, in the model's parameter order
        return sd

    def load_state_dict(self, sd):
        sd = dict(sd)                       # never mutate the caller's dict
        fused = sd.pop("fused", None)
        super().load_state_dict(sd)
        if fused is not None:
            self._pending_step = int(fused["step"])
            steps = fused.get("steps")      # absent in the one-counter format: "step" is then every tensor's count
            self._pending_steps = [int(s) for s in steps] if steps is not None else None
            self._step_dev = None           # re-created on the parameters' device from _pending_step at the next step()
            self._steps_dev = None
            self._m, self._v = fused["exp_avg"], fused["exp_avg_sq"]


class GradScaler(torch.amp.GradScaler):
    """``torch.amp.GradScaler('cuda')`` (reference train.py:610-611) whose inf check / unscale of a ``FusedAdamW``'s gradients
    is ONE launch over the model's flat gradient buffer (``vk_amp_unscale_check``) instead of torch's foreach
    kernels over the 140 strided views.  Everything else — scale growth/backoff, ``scale()``, ``update()``, state dict — is
    torch's own code; the stock ``torch.amp.GradScaler`` also works with ``FusedAdamW`` (sync-free as well)."""

    def _unscale_grads_(self, optimizer, inv_scale, found_inf, allow_fp16):
        model = getattr(optimizer, "_model", None)
        if not isinstance(optimizer, FusedAdamW) or model is None or not model.flat_params.is_cuda:
            return super()._unscale_grads_(optimizer, inv_scale, found_inf, allow_fp16)
        g = model.flat_grads
        dev = g.device
        fi = found_inf.to(dev, non_blocking=True) if found_inf.device != dev else found_inf
        inv = inv_scale.to(dev, non_blocking=True) if inv_scale.device != dev else inv_scale
        check(lib().vk_amp_unscale_check(g.numel(), g.data_ptr(), inv.data_ptr(), fi.data_ptr(), _lib.current_stream()),
              "vk_amp_unscale_check")
        return {dev: fi}


def clip_grad_norm_(optimizer: FusedAdamW, max_norm: float, norm_type: float = 2.0, error_if_nonfinite: bool = False) -> torch.Tensor:
    """``optimizer.clip_grad_norm_(max_norm, norm_type, error_if_nonfinite)``: see FusedAdamW.clip_grad_norm_."""
    return optimizer.clip_grad_norm_(max_norm, norm_type=norm_type, error_if_nonfinite=error_if_nonfinite)


def finetune_groups(model, lr: float, encoder_lr_scale: float = 1.0, weight_decay: float = 1e-4,
                    decay_norm_and_bias: bool = True) -> List[dict]:
    """Param groups of the usual fine-tuning recipe, for ``FusedAdamW`` / ``adamw_for(groups=...)`` or ``torch.optim.AdamW``: the
    encoder at ``lr * encoder_lr_scale`` and the rest at ``lr``, each split, with ``decay_norm_and_bias=False``, into the tensors
    that keep ``weight_decay`` and the 1-D ones (BatchNorm weight and bias, head bias) at ``weight_decay=0``.  Up to four groups,
    empty ones dropped; every parameter of the model is in exactly one."""
    buckets = {(enc, nodecay): [] for enc in (True, False) for nodecay in (False, True)}
    for name, p in model.named_parameters():
        buckets[(name.startswith("encoder."), (not decay_norm_and_bias) and p.dim() <= 1)].append(p)
    return [dict(params=ps, lr=lr * encoder_lr_scale if enc else lr, weight_decay=0.0 if nodecay else weight_decay)
            for (enc, nodecay), ps in buckets.items() if ps]


def adamw_for(model, lr: float, weight_decay: float = 1e-4, groups=None, **kw) -> FusedAdamW:
    """``torch.optim.AdamW(model.parameters(), lr=lr, weight_decay=1e-4)`` of train.py:606, fused.  ``groups``: a list of param-group
    dicts over the model's parameters (``vk.finetune_groups``) in place of ``model.parameters()``; ``lr`` and ``weight_decay`` are
    then the defaults of the groups that do not set them."""
    return FusedAdamW(model.parameters() if groups is None else groups, lr=lr, weight_decay=weight_decay, **kw).attach(model)
