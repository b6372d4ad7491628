"""CPU restatement of ``smp.Unet(encoder_name, encoder_weights=None, in_channels=c, classes=C)`` for 1 <= c <= 4, on top of
tests/encoders_ref.py, and of smp's ``patch_first_conv(pretrained=True)``.

What smp does for ``in_channels != 3`` (recalled from upstream source; smp is not installed, so no fixture pins it): ``get_encoder``
builds the torchvision ResNet — with its 3-channel ``conv1`` and its kaiming_normal_ loop — and then calls
``encoder.set_in_channels(in_channels, pretrained=False)``, whose ``patch_first_conv`` replaces ``conv1.weight`` by a fresh
``[64][c][7][7]`` tensor and calls ``reset_parameters()``: one more RNG draw (kaiming_uniform_, a = sqrt(5)), placed after the encoder's
init loop and before the decoder is constructed.  For 3 channels nothing is drawn.  So the encoder below is ``ResNetEncoder(name)`` — the
3-channel constructor, for its draws — with ``conv1`` patched afterwards, which is what upstream executes."""
from typing import Optional

import torch
import torch.nn as nn

import encoders_ref as R
from oracle import unet_oracle as O


def patch_first_conv_fresh(conv: nn.Conv2d, in_channels: int) -> None:
    """patch_first_conv(pretrained=False)."""
    conv.in_channels = in_channels
    conv.weight = nn.parameter.Parameter(torch.Tensor(conv.out_channels, in_channels, *conv.kernel_size))
    conv.reset_parameters()


def adapt_first_conv(w: torch.Tensor, in_channels: int) -> torch.Tensor:
    """patch_first_conv(pretrained=True) on a 3-channel weight."""
    w = w.detach()
    if in_channels == 1:
        return w.sum(1, keepdim=True)
    new = torch.Tensor(w.shape[0], in_channels, *w.shape[2:]).to(w.dtype)
    for i in range(in_channels):
        new[:, i] = w[:, i % 3]
    return new * (3 / in_channels)


class InputsUnet(nn.Module):
    def __init__(self, name: str, in_channels: int = 3, classes: int = 1):
        super().__init__()
        self.encoder = R.ResNetEncoder(name)
        if in_channels != 3:
            patch_first_conv_fresh(self.encoder.conv1, in_channels)
            self.encoder.out_channels = (in_channels,) + tuple(self.encoder.out_channels[1:])
        self.decoder = O.UnetDecoder(self.encoder.out_channels)
        self.segmentation_head = O.SegmentationHead(16, classes)
        O._initialize_decoder(self.decoder)
        O._initialize_head(self.segmentation_head)

    def forward(self, x):
        return self.segmentation_head(self.decoder(*self.encoder(x)))


def build(name: str, in_channels: int = 3, classes: int = 1, seed: Optional[int] = None) -> InputsUnet:
    if seed is not None:
        O.set_seed(seed)
    return InputsUnet(name, in_channels, classes)
