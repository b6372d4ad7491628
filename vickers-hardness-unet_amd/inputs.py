"""Grayscale and four-channel inputs: ``smp.Unet(in_channels=c)`` for 1 <= c <= 4, and the bridge from the 3-channel data path.

Vickers micrographs come off monochrome cameras; the reference replicates them to three channels only because it reads its files with
``IMREAD_COLOR``.  ``vk.Unet``, ``vk.multiclass.Unet`` and ``vk.encoders.Unet`` stay the reference's 3-channel model (they raise for any
other ``in_channels``); the class here is ``vk.encoders.Unet`` with the wider check::

    model = vk.inputs.Unet(encoder_name="resnet34", encoder_weights=None, in_channels=1, classes=1, activation=None).cuda()
    vk.inputs.load_pretrained(model, torch.load("best.pth"))     # a colour checkpoint: conv1.weight summed over its three channels

The stem's kernels read a 4-channel NHWC copy of the input whatever ``in_channels`` is (the channels past it are zero), so the forward
runs the same kernels; the stem's weight and data gradients take the channel count (csrc/conv_wgrad.hip).  ``encoder.conv1.weight`` is
``[64, c, 7, 7]``, every other key and shape is smp's, and ``x.grad`` is ``[N, c, H, W]``.

The package's device data path (``DeviceDataset.batch``, ``PatchDataset.batch``, ``CopyPaste.batch``, the letterbox, tile and zoom
preprocessing) emits normalised 3-channel fp32 NCHW everywhere.  ``ChannelAdapter`` puts one launch (``vk_input_mix``) between it and a
model of another channel count, so ``Segmenter(ChannelAdapter(m))``, ``predict_mask``, ``infer_tiled``, ``measure`` and a training loop
over a ``DeviceDataset`` work unchanged.

Not built: a single-channel uint8 store in the datasets, single-channel letterbox / augmentation kernels, and a packed
1-channel stem input.  Nothing here claims an accuracy for training on gray images."""
from __future__ import annotations

import ctypes as C
import math
from typing import Mapping, Optional, Sequence, Union

import torch
import torch.nn as nn

from . import _lib
from . import encoders as _encoders
from ._lib import VkError, check, lib

__all__ = ["Unet", "build_model", "adapt_first_conv", "load_pretrained", "ChannelAdapter", "luma_matrix", "IN_CHANNELS",
           "IMAGENET_MEAN", "IMAGENET_STD", "LUMA_WEIGHTS"]

IN_CHANNELS = (1, 2, 3, 4)
FIRST_CONV = "encoder.conv1.weight"
# the constants of the package's normalisation (prepost.hip, reference train.py) and of OpenCV's BGR -> gray conversion, in RGB order
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
LUMA_WEIGHTS = (0.299, 0.587, 0.114)


class Unet(_encoders.Unet):
    """``vk.encoders.Unet`` with ``in_channels`` in 1..4 (``in_channels=3`` is that very model, bit for bit)."""
    in_channels_allowed = IN_CHANNELS


def build_model(encoder: str = "resnet34", weights: Optional[str] = None, in_channels: int = 1) -> Unet:
    """The reference's ``build_model`` (train.py:357-379) with the one line that changes: ``in_channels``."""
    return Unet(encoder_name=encoder, encoder_weights=weights, in_channels=in_channels, classes=1, activation=None)


def adapt_first_conv(weight_or_state_dict: Union[torch.Tensor, Mapping[str, torch.Tensor]], in_channels: int):
    """smp's ``patch_first_conv(pretrained=True)`` for a 3-channel first convolution ``[K, 3, R, S]``: one channel is the sum over the
    three; otherwise ``new[:, i] = w[:, i % 3]`` and all of it times ``3 / in_channels``.  A tensor gives a tensor; a state dict gives a
    copy of the dict with ``encoder.conv1.weight`` replaced (the other entries are the same tensors)."""
    if isinstance(in_channels, bool) or not isinstance(in_channels, int) or in_channels < 1:
        raise ValueError("in_channels=%r: a positive integer" % (in_channels,))
    if isinstance(weight_or_state_dict, Mapping):
        if FIRST_CONV not in weight_or_state_dict:
            raise KeyError("the state dict has no %s" % FIRST_CONV)
        out = dict(weight_or_state_dict)
        out[FIRST_CONV] = adapt_first_conv(out[FIRST_CONV], in_channels)
        return out
    w = weight_or_state_dict.detach()
    if w.dim() != 4 or w.shape[1] != 3:
        raise ValueError("expected a 3-channel first convolution [K,3,R,S], got %s" % (tuple(w.shape),))
    if in_channels == 3:
        return w.clone()
    if in_channels == 1:
        return w.sum(1, keepdim=True)
    new = torch.empty(w.shape[0], in_channels, w.shape[2], w.shape[3], dtype=w.dtype, device=w.device)
    for i in range(in_channels):
        new[:, i] = w[:, i % 3]
    return new * (3 / in_channels)


def load_pretrained(model: Unet, state_dict: Mapping[str, torch.Tensor], strict: bool = True):
    """Load a 3-channel checkpoint (the reference's ``best.pth`` layout: the state dict of ``smp.Unet(in_channels=3)`` / ``vk.Unet``)
    into a model of another ``in_channels`` through ``adapt_first_conv``.  Returns what ``load_state_dict`` returns."""
    if not isinstance(getattr(model, "in_channels", None), int):
        raise VkError("load_pretrained takes a vk.inputs.Unet")
    return model.load_state_dict(adapt_first_conv(state_dict, model.in_channels), strict=strict)


def luma_matrix():
    """(M [1][3], b [1]) of ``ChannelAdapter(mode="luma")`` as Python floats: with w = LUMA_WEIGHTS, mean_g = sum w_j mean_j and
    std_g = sum w_j std_j over the ImageNet constants, M[0][j] = w_j std_j / std_g and b = 0.  A gray value v replicated to three
    channels and normalised per channel, x_j = (v/255 - mean_j) / std_j, then maps to sum_j w_j (v/255 - mean_j) / std_g =
    (v/255 - mean_g) / std_g: the image normalised with the gray constants."""
    std_g = sum(w * s for w, s in zip(LUMA_WEIGHTS, IMAGENET_STD))
    return [[w * s / std_g for w, s in zip(LUMA_WEIGHTS, IMAGENET_STD)]], [0.0]


class ChannelAdapter(nn.Module):
    """``model`` behind one ``vk_input_mix`` launch: ``forward(x3)`` and ``loss_and_backward(x3, y, **kw)`` take the normalised 3-channel
    fp32 NCHW batch of the device data path, form ``out[:, o] = b[o] + sum_j M[o][j] x3[:, j]`` (``cout = len(M)`` planes, which must be
    the model's ``in_channels``) and run the model on it.  ``mode="luma"``: ``luma_matrix()``, one plane; or give ``matrix`` ([cout][3])
    and optionally ``bias`` ([cout]).  It is a data step: no gradient flows to ``x3`` (``x.grad`` is for inputs handed to the model
    itself)."""

    def __init__(self, model: nn.Module, mode: Optional[str] = None, matrix: Optional[Sequence[Sequence[float]]] = None,
                 bias: Optional[Sequence[float]] = None):
        super().__init__()
        if (mode is None) == (matrix is None):
            raise ValueError('ChannelAdapter: give mode="luma" or matrix=, not both and not neither')
        if mode is not None:
            if mode != "luma":
                raise ValueError("ChannelAdapter: unknown mode %r (\"luma\" is implemented)" % (mode,))
            if bias is not None:
                raise ValueError("ChannelAdapter: bias= goes with matrix=")
            matrix, bias = luma_matrix()
        M = torch.as_tensor(matrix, dtype=torch.float32).cpu()
        if M.dim() != 2 or M.shape[1] != 3 or not 1 <= M.shape[0] <= 4:
            raise ValueError("ChannelAdapter: matrix must be [cout][3] with 1 <= cout <= 4, got %s" % (tuple(M.shape),))
        b = torch.zeros(M.shape[0]) if bias is None else torch.as_tensor(bias, dtype=torch.float32).cpu()
        if tuple(b.shape) != (M.shape[0],):
            raise ValueError("ChannelAdapter: bias must be [%d], got %s" % (M.shape[0], tuple(b.shape)))
        if not (torch.isfinite(M).all() and torch.isfinite(b).all()):
            raise ValueError("ChannelAdapter: matrix and bias must be finite")
        want = getattr(model, "in_channels", None)
        if want is not None and want != M.shape[0]:
            raise ValueError("ChannelAdapter: the matrix makes %d channel(s) but the model takes in_channels=%d" % (M.shape[0], want))
        self.model = model
        self.cout = int(M.shape[0])
        self.matrix, self.bias = M.contiguous(), b.contiguous()      # host tensors: the kernel takes them by value
        self._M = (C.c_float * (3 * self.cout))(*self.matrix.flatten().tolist())
        self._b = (C.c_float * self.cout)(*self.bias.tolist())

    def mix(self, x3: torch.Tensor) -> torch.Tensor:
        """The mixed planes [N, cout, H, W] (fp32, a new tensor)."""
        if not isinstance(x3, torch.Tensor) or x3.dim() != 4 or x3.shape[1] != 3:
            raise ValueError("expected input [N,3,H,W], got %s" % (tuple(getattr(x3, "shape", ())),))
        if not x3.is_cuda:
            raise VkError("input is on %s: this package runs on an MI355X only and has no CPU fallback" % x3.device)
        x3 = x3.detach().contiguous().float()
        N, _, H, W = x3.shape
        out = torch.empty(N, self.cout, H, W, dtype=torch.float32, device=x3.device)
        check(lib().vk_input_mix(N, self.cout, H * W, x3.data_ptr(), self._M, self._b, out.data_ptr(), _lib.current_stream()),
              "vk_input_mix")
        return out

    def forward(self, x3: torch.Tensor) -> torch.Tensor:
        return self.model(self.mix(x3))

    def loss_and_backward(self, x3: torch.Tensor, y: torch.Tensor, **kw) -> torch.Tensor:
        return self.model.loss_and_backward(self.mix(x3), y, **kw)
