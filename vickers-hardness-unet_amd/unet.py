"""``Unet`` — drop-in for ``segmentation_models_pytorch.Unet("resnet34", in_channels=3, classes=1)``
as the reference builds it (train.py:357-379 ``build_model``; infer_pth_gui.py:31-33; ui_infer_*.py
``Segmenter``), executed by the HIP engine in libvkunet.so.

API surface kept: constructor arguments, ``forward(x[N,3,S,S] fp32) -> logits
[N,1,S,S] fp32`` (``vk.multiclass.Unet``: ``classes=C``, 1 <= C <= 16, logits [N,C,S,S]; ``vk.inputs.Unet``: ``in_channels=c``, 1 <= c <= 4, x [N,c,S,S]), ``train()/eval()``, ``.to(device)``, ``parameters()``, ``state_dict()`` /
``load_state_dict(strict=True)`` with smp's 278 keys (conv weights are logical OIHW tensors whose memory
is KRSC = torch channels_last, all living in one flat fp32 buffer), autograd participation
(``loss.backward()`` fills ``p.grad``), ``torch.autocast`` selects the 16-bit plan exactly where the
reference autocasts (train.py:431-435) while un-autocast calls (validate, train.py:510) run fp32.

There is no CPU execution path: a CPU tensor or a missing libvkunet.so raises.
"""
from __future__ import annotations

import os
import ctypes as C
import math
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn

from . import _lib, _lossfn
from ._lib import VkError, check, lib


class _Holder(nn.Module):
    """Attribute container so that parameter names reproduce smp's module tree."""

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError("structural container only; call the Unet")


class _Plan:
    """One engine handle + workspace for a fixed (N, size, dtype, training) — static shapes, static
    addresses (hipGraph-friendly)."""

    def __init__(self, model: "Unet", N: int, S, dtype: torch.dtype, training: bool):
        L = lib()
        H, W = (S, S) if isinstance(S, int) else S          # S: the side of a square input or (height, width)
        self.key = (N, S, dtype, training)
        self.N, self.S, self.H, self.W, self.dtype, self.training = N, S, H, W, dtype, training
        cfg = _lib.vk_unet_config(N, H, _lib.dtype_code(dtype), 1 if training else 0, W)
        h = C.c_void_p()
        self.classes = model.classes
        model._create_handle(cfg, h)
        self.h = h
        self.ws_bytes = L.vk_unet_workspace_bytes(h)
        dev = model._flat["params"].device
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=dev)
        self.loss_out = torch.zeros(4, dtype=torch.float32, device=dev)
        self._seg_out = self._lovasz_out = self._kp_out = None       # the result buffers of the loss= routes: made at a route's first step on this plan
        self.weights_version = None
        self.mask = None                    # trainable flags the engine holds (vk_unet_set_trainable); None: not pushed yet
        self.bn_frozen = None               # BatchNorm modes the engine holds (vk_unet_set_bn_frozen); None: not pushed (all train)
        self.in_channels = model.in_channels
        self.dx: Optional[torch.Tensor] = None     # fp32 [N,in_channels,H,W] input gradient the engine writes (vk_unet_set_input_grad)
        self.dx_on = False
        self.serial = 0                     # forwards this plan has run; a graph remembers the value its own forward left (_UnetFn)
        self.last_forward = ""              # what ran that forward, for the message of a displaced graph
        self.bucket_trainable: List[bool] = []
        self.nbuckets = L.vk_unet_num_buckets(h)
        self.buckets: List[Tuple[int, int]] = []
        for b in range(self.nbuckets):
            b0, b1 = C.c_int64(), C.c_int64()
            check(L.vk_unet_bucket_range(h, b, C.byref(b0), C.byref(b1)))
            self.buckets.append((b0.value, b1.value))
        self.bind(model)

    def bind(self, model: "Unet"):
        f = model._flat
        grads = model._ensure_grads() if self.training else None
        check(lib().vk_unet_bind(self.h, f["params"].data_ptr(), _lib.ptr(grads), f["bufs"].data_ptr(),
                                 f["nbt"].data_ptr(), self.ws.data_ptr(), self.ws_bytes), "vk_unet_bind")
        self.weights_version = None

    def set_trainable(self, model: "Unet", mask: Tuple[bool, ...]):
        """Hand the engine one requires_grad flag per parameter tensor (host only; done when the flags change)."""
        if mask == self.mask:
            return
        flags = (C.c_uint8 * len(mask))(*mask)
        check(lib().vk_unet_set_trainable(self.h, flags, len(mask)), "vk_unet_set_trainable")
        self.mask = mask
        ranges = [(off, off + numel) for (off, numel), t in zip(model._param_ranges, mask) if t]
        self.bucket_trainable = [any(a < b1 and b0 < b for a, b in ranges) for b0, b1 in self.buckets]

    def set_bn_frozen(self, flags: Tuple[bool, ...]):
        """Hand the engine one frozen-statistics flag per BatchNorm layer (host only; done when the flags change)."""
        if flags == self.bn_frozen or (self.bn_frozen is None and not any(flags)):
            return
        arr = (C.c_uint8 * len(flags))(*flags)
        check(lib().vk_unet_set_bn_frozen(self.h, arr, len(flags)), "vk_unet_set_bn_frozen")
        self.bn_frozen = flags

    def set_input_grad(self, on: bool, device):
        """Point the engine's input-gradient output at the plan's buffer, or at nothing (host only; done when it changes)."""
        if on == self.dx_on:
            return
        if on and self.dx is None:
            self.dx = torch.empty(self.N, self.in_channels, self.H, self.W, dtype=torch.float32, device=device)
        check(lib().vk_unet_set_input_grad(self.h, self.dx.data_ptr() if on else None), "vk_unet_set_input_grad")
        self.dx_on = on

    def seg_out(self) -> torch.Tensor:
        """The 8 floats vk_unet_loss_cfg writes (loss=<vk.seglosses>)."""
        if self._seg_out is None:
            self._seg_out = torch.zeros(8, dtype=torch.float32, device=self.ws.device)
        return self._seg_out

    def lovasz_out(self):
        """(the 16 floats vk_unet_loss_lovasz writes, the indices of the 8 that are reported, the 8 floats they are gathered into)."""
        if self._lovasz_out is None:
            dev = self.ws.device
            self._lovasz_out = (torch.zeros(16, dtype=torch.float32, device=dev),
                                torch.tensor([0, 1, 2, 3, 4, 5, 7, 8], dtype=torch.int64, device=dev),
                                torch.empty(8, dtype=torch.float32, device=dev))
        return self._lovasz_out

    def kp_out(self):
        """(the 16 floats vk_unet_loss_kp writes, the indices of the 9 that are reported, the 9 floats they are gathered into)."""
        if self._kp_out is None:
            dev = self.ws.device
            self._kp_out = (torch.zeros(16, dtype=torch.float32, device=dev),
                            torch.tensor([0, 1, 2, 3, 4, 5, 7, 8, 9], dtype=torch.int64, device=dev),
                            torch.empty(9, dtype=torch.float32, device=dev))
        return self._kp_out

    def debug_tensor(self, name: str) -> torch.Tensor:
        """Copy of a named intermediate (NHWC) — parity/debug only."""
        p = C.c_void_p()
        dims = (C.c_int * 4)()
        check(lib().vk_unet_debug_tensor(self.h, name.encode(), C.byref(p), C.byref(dims)), "vk_unet_debug_tensor")
        shape = [d for d in dims]
        is_f32 = name.startswith(("scale:", "shift:", "dlogits"))
        dt = torch.float32 if is_f32 else self.dtype
        off = p.value - self.ws.data_ptr()
        n = 1
        for d in shape:
            n *= d
        nbytes = n * torch.empty((), dtype=dt).element_size()
        return self.ws[off:off + nbytes].view(dt).view(shape).clone()

    def __del__(self):
        try:
            if getattr(self, "h", None):
                lib().vk_unet_destroy(self.h)
                self.h = None
        except Exception:
            pass


class _UnetFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, anchor, model, plan, mask):
        ctx.model, ctx.plan, ctx.mask = model, plan, mask      # requires_grad as it was when the forward ran (torch records it then)
        ctx.x_dtype, ctx.x_device = x.dtype, x.device
        logits = model._run_forward(plan, x, True, "a forward with a graph (model(x) in grad mode)")
        ctx.serial = plan.serial           # the plan's workspace holds THIS forward's activations while the two are equal
        return logits

    @staticmethod
    def backward(ctx, g):
        want_dx = bool(ctx.needs_input_grad[0])
        plan = ctx.plan
        if plan.serial != ctx.serial:      # before anything is written: the gradients and every .grad stay as they are
            raise VkError("backward() through a forward whose activations are gone: the plan (N=%d, %dx%d, %s) has since run %s, "
                          "which overwrote them (%d forward(s) later). One plan holds the activations of one forward: call backward() "
                          "before the next forward of that shape and dtype (model(x), a torch.no_grad() forward or loss_and_backward), "
                          "see INTEGRATION.md \"One forward per shape at a time\""
                          % (plan.N, plan.H, plan.W, str(plan.dtype).replace("torch.", ""), plan.last_forward,
                             plan.serial - ctx.serial))
        ctx.model._run_backward(ctx.plan, g.contiguous().float(), ctx.mask, want_dx)
        # the plan's buffer is rewritten by the next backward: hand autograd a copy in x's dtype
        dx = ctx.plan.dx.to(dtype=ctx.x_dtype, copy=True) if want_dx else None
        return dx, None, None, None, None


class Unet(nn.Module):
    max_classes = 1                # the reference's binary model; vk.multiclass.Unet takes 1 <= classes <= 16
    encoders = ("resnet34",)       # the reference's encoder; vk.encoders.Unet also builds resnet18 and resnet50
    in_channels_allowed = (3,)     # the reference's colour input; vk.inputs.Unet takes 1 <= in_channels <= 4

    def __init__(self, encoder_name: str = "resnet34", encoder_depth: int = 5, encoder_weights: Optional[str] = "imagenet",
                 decoder_use_batchnorm: bool = True, decoder_channels=(256, 128, 64, 32, 16),
                 decoder_attention_type: Optional[str] = None, in_channels: int = 3, classes: int = 1,
                 activation: Optional[str] = None, aux_params: Optional[dict] = None, *,
                 compute_dtype: torch.dtype = torch.float32):
        super().__init__()
        if encoder_name not in self.encoders:
            if self.encoders == ("resnet34",):
                raise NotImplementedError("only the reference's configuration encoder_name='resnet34' is implemented")
            raise NotImplementedError("encoder_name=%r: one of %s is implemented" % (encoder_name, ", ".join(self.encoders)))
        if encoder_weights is not None:
            raise VkError("encoder_weights=%r needs a checkpoint download; no network here — pass None and "
                          "load_state_dict() a checkpoint instead" % (encoder_weights,))
        if (encoder_depth != 5 or tuple(decoder_channels) != (256, 128, 64, 32, 16) or not decoder_use_batchnorm
                or decoder_attention_type is not None or in_channels not in self.in_channels_allowed or activation is not None
                or aux_params is not None):
            chans = "=3" if self.in_channels_allowed == (3,) else " in %s" % (self.in_channels_allowed,)
            raise NotImplementedError("only in_channels%s, activation=None, default decoder are implemented "
                                      "(reference train.py:372-378)" % chans)
        if not isinstance(classes, int) or not 1 <= classes <= self.max_classes:
            if self.max_classes == 1:
                raise NotImplementedError("classes=%r: vk.Unet is the reference's binary model (classes=1); more than one class: "
                                          "vk.multiclass.Unet(classes=C), 1 <= C <= 16" % (classes,))
            raise NotImplementedError("classes=%r: 1 <= classes <= %d is implemented (the head is one 16-wide tile of output "
                                      "channels)" % (classes, self.max_classes))
        self.classes = classes
        self.in_channels = int(in_channels)
        self.encoder_name = encoder_name
        self.compute_dtype = compute_dtype
        L = lib()
        cfg = _lib.vk_unet_config(1, 32, _lib.VK_F32, 0)
        h = C.c_void_p()
        self._create_handle(cfg, h)
        try:
            self._table = []
            for i in range(L.vk_unet_num_tensors(h)):
                ti = _lib.vk_tensor_info()
                check(L.vk_unet_tensor_info(h, i, C.byref(ti)))
                self._table.append((ti.name.decode(), ti.kind, [ti.dims[j] for j in range(ti.ndim)], ti.offset, ti.numel))
            n_params = L.vk_unet_param_numel(h)
            n_bufs = L.vk_unet_buffer_numel(h)
        finally:
            L.vk_unet_destroy(h)
        n_bn = sum(1 for t in self._table if t[1] == 3)
        self._flat: Dict[str, Optional[torch.Tensor]] = {
            "params": torch.zeros(n_params, dtype=torch.float32),
            "grads": None,
            "bufs": torch.zeros(n_bufs, dtype=torch.float32),
            "nbt": torch.zeros(n_bn, dtype=torch.int64),
        }
        self._leaves: Dict[str, Tuple[nn.Module, str]] = {}
        self._plans: Dict[tuple, _Plan] = {}
        self._dirty = 0
        self._reducer = None
        self._time_groups = None
        self._group_events = []
        self._anchor = torch.zeros((), requires_grad=True)
        self._build_tree()
        self._rebuild_views()
        self._default_init()

    # ------------------------------------------------------------------ structure
    def _create_handle(self, cfg, h):
        """Engine plan of this model's encoder, classes and input channels (vk_unet_create_ex: resnet34; vk_unet_create_enc: the other
        encoders; vk_unet_create_in: in_channels other than 3)."""
        codes = {"resnet18": _lib.VK_ENC_RESNET18, "resnet34": _lib.VK_ENC_RESNET34, "resnet50": _lib.VK_ENC_RESNET50}
        if self.in_channels != 3:
            check(lib().vk_unet_create_in(C.byref(cfg), self.classes, codes[self.encoder_name], self.in_channels, C.byref(h)),
                  "vk_unet_create_in")
        elif self.encoder_name == "resnet34":
            check(lib().vk_unet_create_ex(C.byref(cfg), self.classes, C.byref(h)), "vk_unet_create_ex")
        else:
            check(lib().vk_unet_create_enc(C.byref(cfg), self.classes, codes[self.encoder_name], C.byref(h)), "vk_unet_create_enc")

    def _view(self, kind: int, dims: List[int], off: int, numel: int, which: str = "params") -> torch.Tensor:
        if kind == 0:
            K, Cc, R, S = dims
            return self._flat[which][off:off + numel].view(K, R, S, Cc).permute(0, 3, 1, 2)
        if kind == 1:
            return self._flat[which][off:off + numel]
        if kind == 2:
            return self._flat["bufs"][off:off + numel]
        return self._flat["nbt"][off]

    def _build_tree(self):
        for name, kind, dims, off, numel in self._table:
            parts = name.split(".")
            mod: nn.Module = self
            for p in parts[:-1]:
                if p not in mod._modules:
                    mod.add_module(p, _Holder())
                mod = mod._modules[p]
            leaf = parts[-1]
            if kind in (0, 1):
                mod.register_parameter(leaf, nn.Parameter(torch.empty(0), requires_grad=True))
            else:
                mod.register_buffer(leaf, torch.empty(0))
            self._leaves[name] = (mod, leaf)

    def _rebuild_views(self):
        for name, kind, dims, off, numel in self._table:
            mod, leaf = self._leaves[name]
            v = self._view(kind, dims, off, numel)
            if kind in (0, 1):
                p = mod._parameters[leaf]
                p.data = v
                p.grad = None
            else:
                mod._buffers[leaf] = v
        self._anchor = torch.zeros((), requires_grad=True, device=self._flat["params"].device)
        self._param_list = [self._leaves[t[0]][0]._parameters[self._leaves[t[0]][1]] for t in self._table if t[1] in (0, 1)]
        self._param_ranges = [(t[3], t[4]) for t in self._table if t[1] in (0, 1)]
        self._bn_modules = [self._leaves[t[0]][0] for t in self._table if t[1] == 3]

    def _apply(self, fn, recurse=True):
        for k in ("params", "grads", "bufs", "nbt"):
            t = self._flat[k]
            if t is not None:
                nt = fn(t)
                want = torch.int64 if k == "nbt" else torch.float32
                if nt.dtype != want:
                    raise VkError("the fp32 master copy cannot be converted to %s; choose the compute type with "
                                  "torch.autocast or compute_dtype=" % nt.dtype)
                self._flat[k] = nt
        self._rebuild_views()
        self._plans.clear()
        self._dirty += 1
        return self

    def _default_init(self):
        """smp / torchvision default initialisation, drawing from torch's global RNG in the same order
        and with the same shapes as the constructors would ([upstream]), so that
        ``set_seed(42); Unet(...)`` reproduces the oracle's weights."""
        sd = {name: self._view(kind, dims, off, numel) for name, kind, dims, off, numel in self._table}

        def ctor_draw(shape, bias=False):   # nn.Conv2d / nn.Linear reset_parameters()
            w = torch.empty(shape)
            nn.init.kaiming_uniform_(w, a=math.sqrt(5))
            if bias:
                fan_in = w[0].numel()
                bound = 1 / math.sqrt(fan_in)
                nn.init.uniform_(torch.empty(shape[0]), -bound, bound)

        with torch.no_grad():
            for name, kind, dims, off, numel in self._table:
                if kind == 1 and name.endswith(".weight") and len(dims) == 1:
                    sd[name].fill_(1.0)                       # BN gamma
                elif kind == 2 and name.endswith("running_var"):
                    sd[name].fill_(1.0)
            enc = [t for t in self._table if t[1] == 0 and t[0].startswith("encoder.")]
            dec = [t for t in self._table if t[1] == 0 and t[0].startswith("decoder.")]
            head = [t for t in self._table if t[1] == 0 and t[0].startswith("segmentation_head.")][0]
            # torchvision constructs conv1, then per block conv1, conv2 (, conv3 in a Bottleneck), (downsample) — but the
            # downsample conv is built BEFORE the block in _make_layer
            def ctor_order(ts):
                out, block = [], []
                for t in ts + [("", 0, [], 0, 0)]:
                    parts = t[0].split(".")
                    prefix = ".".join(parts[:3]) if len(parts) > 3 and parts[1].startswith("layer") else t[0]
                    if block and (not t[0] or prefix != block[0][0]):
                        out += [b[1] for b in block if ".downsample." in b[1][0]] + [b[1] for b in block if ".downsample." not in b[1][0]]
                        block = []
                    if t[0]:
                        block.append((prefix, t))
                return out
            # torchvision builds its ResNet with 3 input channels whatever in_channels is (smp patches conv1 afterwards, below)
            def tv_shape(t):
                return [t[2][0], 3] + t[2][2:] if t[0] == "encoder.conv1.weight" else t[2]
            for t in ctor_order(enc):
                ctor_draw(tv_shape(t))
            ctor_draw([1000, enc[-1][2][0]], bias=True)        # the fc layer torchvision builds and smp deletes (512 x expansion inputs)
            for t in enc:                                      # ResNet.__init__ init loop (module order)
                w = torch.empty(tv_shape(t))
                nn.init.kaiming_normal_(w, mode="fan_out", nonlinearity="relu")
                if t[0] != "encoder.conv1.weight" or self.in_channels == 3:      # otherwise smp replaces this tensor, below
                    sd[t[0]].copy_(w)
            if self.in_channels != 3:
                # smp get_encoder -> set_in_channels(in_channels, pretrained=False) -> patch_first_conv: conv1.weight becomes a fresh
                # [64][in_channels][7][7] tensor and reset_parameters() draws it (kaiming_uniform_, a = sqrt(5)): one more draw, behind
                # the encoder's init loop and before the decoder exists.  Recalled from upstream source; no fixture pins it
                w = torch.empty(enc[0][2])
                nn.init.kaiming_uniform_(w, a=math.sqrt(5))
                sd[enc[0][0]].copy_(w)
            for t in dec:
                ctor_draw(t[2])
            ctor_draw(head[2], bias=True)
            for t in dec:                                      # smp initialize_decoder
                w = torch.empty(t[2])
                nn.init.kaiming_uniform_(w, mode="fan_in", nonlinearity="relu")
                sd[t[0]].copy_(w)
            w = torch.empty(head[2])                           # smp initialize_head
            nn.init.xavier_uniform_(w)
            sd[head[0]].copy_(w)
            sd["segmentation_head.0.bias"].zero_()
        self._dirty += 1

    # ------------------------------------------------------------------ flat-buffer access (optimizer / DP)
    @property
    def flat_params(self) -> torch.Tensor:
        return self._flat["params"]

    @property
    def flat_grads(self) -> torch.Tensor:
        return self._ensure_grads()

    def _ensure_grads(self) -> torch.Tensor:
        if self._flat["grads"] is None:
            self._flat["grads"] = torch.zeros_like(self._flat["params"])
        return self._flat["grads"]

    def _attach_grads(self, mask: Optional[Tuple[bool, ...]] = None, missing_only: bool = False):
        """Point ``.grad`` of the trainable parameters at their views of the flat gradient buffer; frozen ones get None (torch leaves the
        grad of a parameter that did not require it untouched: with ``missing_only`` they keep theirs, and a trainable tensor that had
        none starts from zero, as a fresh torch grad does)."""
        g = self._ensure_grads()
        i = 0
        for name, kind, dims, off, numel in self._table:
            if kind in (0, 1):
                mod, leaf = self._leaves[name]
                p = mod._parameters[leaf]
                if mask is None or mask[i]:
                    if not missing_only or p.grad is None:
                        view = self._view(kind, dims, off, numel, "grads")
                        if missing_only:
                            view.zero_()
                        p.grad = view
                elif not missing_only:
                    p.grad = None
                i += 1

    def _trainable_mask(self) -> Tuple[bool, ...]:
        return tuple(bool(p.requires_grad) for p in self._param_list)

    def _bn_frozen_flags(self) -> Tuple[bool, ...]:
        """One flag per BatchNorm layer, in the engine's order (the num_batches_tracked entries of the tensor table): the layer's mode
        is the ``training`` flag of the module that owns its weight / running stats (``encoder.bn1``, ...), as in torch."""
        return tuple(not m.training for m in self._bn_modules)

    def mark_weights_dirty(self):
        """Call after writing the flat parameter buffer through a raw pointer (FusedAdamW does)."""
        self._dirty += 1

    def _weights_version(self):
        # Parameter.data views carry their own version counters, so sum them (in-place edits by a stock
        # torch optimizer or load_state_dict bump them); raw-pointer writers call mark_weights_dirty().
        return (self._dirty, sum(p._version for p in self._param_list))

    # ------------------------------------------------------------------ plans
    def plan_for(self, N: int, S, dtype: torch.dtype, training: bool) -> _Plan:
        key = (N, S, dtype, training)
        p = self._plans.get(key)
        if p is None and not training:
            p = self._plans.get((N, S, dtype, True))    # a training plan can also run eval forwards
        if p is None:
            p = _Plan(self, N, S, dtype, training)
            self._plans[key] = p
        return p

    def _check_input(self, x: torch.Tensor):
        if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.shape[1] != self.in_channels:
            raise ValueError("expected input [N,%d,H,W], got %s" % (self.in_channels, tuple(x.shape)))
        h, w = x.shape[-2:]
        if h % 32 or w % 32:
            raise RuntimeError(f"Wrong input shape height={h}, width={w}. Expected image height and width divisible by 32.")
        if not x.is_cuda:
            raise VkError("input is on %s: this package runs on an MI355X only and has no CPU fallback" % x.device)
        if self._flat["params"].device != x.device:
            raise VkError("model is on %s but the input is on %s" % (self._flat["params"].device, x.device))

    def _run_forward(self, plan: _Plan, x: torch.Tensor, training: bool, who: str = "a forward without a graph") -> torch.Tensor:
        L = lib()
        plan.serial += 1                    # whatever graph an earlier forward of this plan left can no longer run its backward
        plan.last_forward = who
        st = _lib.current_stream()
        ver = self._weights_version()
        if plan.weights_version != ver:
            check(L.vk_unet_refresh_weights(plan.h, st), "vk_unet_refresh_weights")
            plan.weights_version = ver
        x = x.detach().contiguous().float()
        if training:
            plan.set_bn_frozen(self._bn_frozen_flags())      # per-layer BatchNorm modes; the engine keeps them for the backward
        logits = torch.empty(plan.N, self.classes, plan.H, plan.W, dtype=torch.float32, device=x.device)
        check(L.vk_unet_forward(plan.h, x.data_ptr(), logits.data_ptr(), 1 if training else 0, st), "vk_unet_forward")
        plan._last_x = x      # keep the input alive until backward has consumed the plan's x4 copy
        return logits

    def _run_backward(self, plan: _Plan, dlogits: Optional[torch.Tensor], mask: Tuple[bool, ...], want_dx: bool = False):
        L = lib()
        st = _lib.current_stream()
        plan.set_trainable(self, mask)
        plan.set_input_grad(want_dx, self._flat["params"].device)
        if all(mask):
            fresh = next(iter(self.parameters())).grad is None
        else:
            # fine-tuning: the buffer is zeroed when no trainable tensor holds a gradient (after zero_grad; not from a fixed tensor —
            # the stem weight, say, when it is frozen, or a tensor unfrozen between two accumulating backwards); frozen ranges stay 0
            fresh = all(p.grad is None for p, t in zip(self._param_list, mask) if t)
        if fresh:
            check(L.vk_unet_zero_grad(plan.h, st), "vk_unet_zero_grad")
            self._attach_grads(None if all(mask) else mask)
        else:
            # accumulating: a trainable tensor whose grad was set to None (an optimizer over a subset zeroes only its own) starts at 0
            self._attach_grads(mask, missing_only=True)
        red = self._reducer
        if red is not None and getattr(red, "enabled", True) and not getattr(plan, "_side_off", False):
            check(L.vk_unet_set_side_stream(plan.h, 0), "vk_unet_set_side_stream")    # see include/vk_unet.h
            plan._side_off = True
        capped = False
        # bench.py's overlap budget: `_time_groups` = [begin, end) stage ranges to run as separate calls with a HIP event pair around
        # each (the grouping of the "deferred" policy is [(0, 9), (9, 10)]); durations are read with group_times_ms()
        tg = getattr(self, "_time_groups", None)
        if red is None and tg is None and not os.environ.get("VK_BACKWARD_PER_STAGE"):
            # nobody needs a stage's gradients before the end: one call, so that the weight gradients of ALL stages run as one batch
            check(L.vk_unet_backward(plan.h, _lib.ptr(dlogits), 0, plan.nbuckets, st), "vk_unet_backward")
            return
        if os.environ.get("VK_BACKWARD_PER_STAGE"):
            groups = [(s, s + 1) for s in range(plan.nbuckets)]
        elif red is not None and hasattr(red, "stage_groups"):
            groups = red.stage_groups(plan.nbuckets)
        elif tg is not None:
            groups = [tuple(g) for g in tg]
        else:
            groups = [(s, s + 1) for s in range(plan.nbuckets)]
        timed = tg is not None or (red is not None and getattr(red, "timing", False))
        try:
            for s0, s1 in groups:
                if red is not None and getattr(red, "reserved_cus", 0) > 0 and getattr(red, "in_flight", False) and not capped:
                    L.vk_set_reserved_cus(red.reserved_cus)      # collectives share the chip from here on: see parallel.py
                    capped = True
                if timed:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                check(L.vk_unet_backward(plan.h, _lib.ptr(dlogits), s0, s1, st), "vk_unet_backward")
                if timed:
                    e1.record()
                    self._group_events.append((s0, s1, e0, e1))
                if red is not None:
                    for s in range(s0, s1):
                        if plan.bucket_trainable[s]:
                            red.bucket_ready(s, plan.buckets[s])
                        else:
                            red.bucket_ready(s, plan.buckets[s], trainable=False)    # frozen: no collective (parallel.py)
        finally:
            if capped:
                L.vk_set_reserved_cus(0)
        if red is not None:
            red.finish()

    def group_times_ms(self):
        """Durations of the timed backward groups since the last call: {(begin, end): [ms per step, ...]} (synchronises)."""
        out = {}
        for s0, s1, e0, e1 in self._group_events:
            e1.synchronize()
            out.setdefault((s0, s1), []).append(e0.elapsed_time(e1))
        self._group_events.clear()
        return out

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        self._check_input(x)
        N, _, H, W = x.shape
        S = H if H == W else (H, W)           # plans are keyed by the side of a square input or by (height, width)
        if torch.is_autocast_enabled():
            dtype = torch.get_autocast_dtype('cuda')
        else:
            dtype = self.compute_dtype
        mask = self._trainable_mask()
        # a graph iff grad mode is on and something needs a gradient (a parameter or the input), in either mode of the root; the
        # BatchNorm layers run in their own modules' modes (_bn_frozen_flags) on a training plan.  Without a graph and with every layer
        # in eval mode: the eval plan, as before.
        need_grad = torch.is_grad_enabled() and (any(mask) or x.requires_grad)
        all_frozen = all(self._bn_frozen_flags())
        plan = self.plan_for(N, S, dtype, need_grad or not all_frozen)
        if need_grad:
            return _UnetFn.apply(x, self._anchor, self, plan, mask)
        return self._run_forward(plan, x, not all_frozen, "a forward without a graph (torch.no_grad(), or nothing requires grad)")

    # ------------------------------------------------------------------ fused step (no autograd graph)
    def loss_and_backward(self, x: torch.Tensor, y: torch.Tensor, grad_scale: float = 1.0,
                          dtype: Optional[torch.dtype] = None, mode: Optional[str] = None, loss=None) -> torch.Tensor:
        """forward (BatchNorm layers in their modules' modes) + loss + backward in one call; the engine's loss kernel feeds the
        head gradient directly.  Returns a device tensor [total, bce or ce, dice] (no host sync).
        Equivalent to train.py:436-448 ``logits = model(x); loss = bce + dice; loss.backward()``; ``requires_grad`` of the parameters
        is read at this call (frozen ones get no gradient, see INTEGRATION.md "Fine-tuning").
        ``mode``: None / "binary" (classes == 1: BCEWithLogitsLoss + DiceLoss("binary")), "multilabel" (y fp32 [N,C,H,W]:
        BCEWithLogitsLoss + DiceLoss("multilabel")) or "multiclass" (y int64 [N,H,W] in [0, C): CrossEntropyLoss +
        DiceLoss("multiclass"); a label outside [0, C) makes the result NaN).  With classes > 1 the mode must be
        given.
        ``loss``: a ``vk.seglosses`` term or sum instead of ``mode`` (the two exclude each other): the same step with that loss
        (vk_unet_loss_cfg); returns a device tensor [total, pix, focal, dice, jaccard, tversky] of a buffer of its own.  A
        ``vk.lovasz.LovaszLoss`` or ``vk.lovasz.LossSum`` runs vk_unet_loss_lovasz instead and returns
        [total, pix, focal, dice, jaccard, tversky, mcc, lovasz].  A ``vk.keypoints`` term or ``vk.keypoints.LossSum`` runs
        vk_unet_loss_kp and returns [total, pix, focal, dice, jaccard, tversky, mcc, heat, plane_bce]."""
        if loss is not None:
            if mode is not None:
                raise ValueError("loss_and_backward: give mode= or loss=, not both")
            from . import lovasz, seglosses
            from . import keypoints
            if isinstance(loss, keypoints._KpAlgebra):
                S = loss._as_kp_sum()
                kcfg, scfg = S.kp_cfg(self.classes), S.seg_cfg(self.classes)

                def launch(plan, logits, y, st):
                    ws = S.workspace(plan.N, self.classes, plan.H * plan.W, logits.device)
                    check(lib().vk_unet_loss_kp(plan.h, scfg, kcfg, logits.data_ptr(), y.data_ptr(), ws.data_ptr(), ws.numel(),
                                                plan.kp_out()[0].data_ptr(), float(grad_scale), st), "vk_unet_loss_kp")

                plan = self._fused_step(x, y, dtype, False, "loss=<multiclass>", True, launch)
                out, pick, picked = plan.kp_out()
                S.last_components = torch.index_select(out, 0, pick, out=picked)
                return picked
            if isinstance(loss, lovasz._LovaszAlgebra):
                S = loss._as_lovasz_sum()
                lcfg, scfg = S.lovasz_cfg(self.classes), S.seg_cfg(self.classes)

                def launch(plan, logits, y, st):
                    ws = S.workspace(lcfg, plan.N, self.classes, plan.H * plan.W, logits.device)
                    check(lib().vk_unet_loss_lovasz(plan.h, scfg, lcfg, S.w, logits.data_ptr(), y.data_ptr(), ws.data_ptr(), ws.numel(),
                                                    plan.lovasz_out()[0].data_ptr(), float(grad_scale), st), "vk_unet_loss_lovasz")

                plan = self._fused_step(x, y, dtype, lcfg.mode == _lib.VK_LOSS_MULTICLASS, "loss=<multiclass>", True, launch)
                out, pick, picked = plan.lovasz_out()
                S.last_components = torch.index_select(out, 0, pick, out=picked)
                return picked
            S = seglosses.as_loss_sum(loss)
            cfg = S.cfg(self.classes)

            def launch(plan, logits, y, st):
                check(lib().vk_unet_loss_cfg(plan.h, cfg, logits.data_ptr(), y.data_ptr(), plan.seg_out().data_ptr(), float(grad_scale),
                                             st), "vk_unet_loss_cfg")

            plan = self._fused_step(x, y, dtype, cfg.mode == _lib.VK_LOSS_MULTICLASS, "loss=<multiclass>", True, launch)
            S.last_components = plan.seg_out()[:6]
            return S.last_components
        if mode is None:
            if self.classes != 1:
                raise ValueError("loss_and_backward: classes=%d needs mode='multilabel' or mode='multiclass'" % self.classes)
            mode = "binary"
        codes = {"binary": _lib.VK_LOSS_BINARY, "multilabel": _lib.VK_LOSS_MULTILABEL, "multiclass": _lib.VK_LOSS_MULTICLASS}
        if mode not in codes:
            raise ValueError("loss_and_backward: unknown mode %r" % (mode,))

        def launch(plan, logits, y, st):
            if mode == "binary":
                check(lib().vk_unet_loss(plan.h, logits.data_ptr(), y.data_ptr(), plan.loss_out.data_ptr(), float(grad_scale),
                                         1.0, 1.0, st), "vk_unet_loss")
            else:
                check(lib().vk_unet_loss_ex(plan.h, codes[mode], logits.data_ptr(), y.data_ptr(), plan.loss_out.data_ptr(),
                                            float(grad_scale), 1.0, 1.0, st), "vk_unet_loss_ex")

        return self._fused_step(x, y, dtype, mode == "multiclass", "mode='multiclass'", False, launch).loss_out[:3]

    def _fused_step(self, x, y, dtype, multiclass: bool, who: str, nchw: bool, launch) -> _Plan:
        """The step every route of ``loss_and_backward`` runs; returns the plan, whose buffer ``launch(plan, logits, y, stream)`` made
        the engine's loss kernel write.  ``who`` names the route in the message about a multiclass target; ``nchw``: the ``loss=``
        routes, which also refuse a sigmoid-mode target that is not [N, 1 or classes, H, W]."""
        self._check_input(x)
        mask = self._trainable_mask()
        if not any(mask):
            raise VkError("loss_and_backward: no parameter requires grad (every tensor is frozen)")
        N, _, H, W = x.shape
        shape = (N, self.classes, H, W)
        if multiclass:
            _lossfn.check_target(shape, y, "multiclass", "loss_and_backward(%s)" % who)
        elif nchw and (y.dim() != 4 or y.shape[0] != N or y.shape[1] not in (1, self.classes) or tuple(y.shape[2:]) != (H, W)):
            raise ValueError("loss_and_backward(loss=...): target must be [N,%d,H,W], got %s" % (self.classes, tuple(y.shape)))
        plan = self.plan_for(N, H if H == W else (H, W), dtype or self.compute_dtype, True)
        logits, y = _lossfn.marshal(self._run_forward(plan, x, True, "loss_and_backward"), y, multiclass)
        launch(plan, logits, y, _lib.current_stream())
        self._run_backward(plan, None, mask)
        self.last_logits = logits
        return plan


def build_model(encoder: str = "resnet34", weights: Optional[str] = "imagenet") -> Unet:
    """Mirror of reference train.py:357-379."""
    return Unet(encoder_name=encoder, encoder_weights=weights, in_channels=3, classes=1, activation=None)
