"""CPU restatement of ``smp.Unet(encoder_name="resnet18" | "resnet34" | "resnet50", encoder_weights=None, classes=C)``, composed from
the oracle's ``BasicBlock`` / ``UnetDecoder`` / ``SegmentationHead`` / initialisers plus a torchvision-layout Bottleneck (v1.5: the
stride on the 3x3 convolution, expansion 4).  Module names, construction order and the RNG draws (the fc layer torchvision builds and smp
deletes, the encoder's kaiming_normal_ loop, smp's decoder / head initialisation) follow the upstream constructors."""
from typing import List, Optional

import torch
import torch.nn as nn

from oracle import unet_oracle as O

# encoder -> (block, blocks per layer); the known answers of the table in the issue that asked for the encoders
LAYOUTS = {"resnet18": ("basic", (2, 2, 2, 2)), "resnet34": ("basic", (3, 4, 6, 3)), "resnet50": ("bottleneck", (3, 4, 6, 3))}
EXPECTED = {"resnet18": (14_328_209, 182), "resnet34": (24_436_369, 278), "resnet50": (32_521_105, 380)}


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes: int, planes: int, stride: int = 1, downsample: Optional[nn.Module] = None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, 1, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        identity = x
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        if self.downsample is not None:
            identity = self.downsample(x)
        return self.relu(out + identity)


class ResNetEncoder(nn.Module):
    def __init__(self, name: str, in_channels: int = 3):
        super().__init__()
        kind, layers = LAYOUTS[name]
        block = O.BasicBlock if kind == "basic" else Bottleneck
        self.inplanes = 64
        self.conv1 = nn.Conv2d(in_channels, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        self.layer1 = self._make_layer(block, 64, layers[0])
        self.layer2 = self._make_layer(block, 128, layers[1], stride=2)
        self.layer3 = self._make_layer(block, 256, layers[2], stride=2)
        self.layer4 = self._make_layer(block, 512, layers[3], stride=2)
        e = block.expansion
        self.out_channels = (in_channels, 64, 64 * e, 128 * e, 256 * e, 512 * e)
        fc = nn.Linear(512 * e, 1000)          # torchvision builds it (RNG draws), smp deletes it
        del fc
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)

    def _make_layer(self, block, planes: int, blocks: int, stride: int = 1) -> nn.Sequential:
        downsample = None
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(nn.Conv2d(self.inplanes, planes * block.expansion, 1, stride, bias=False),
                                       nn.BatchNorm2d(planes * block.expansion))
        layers = [block(self.inplanes, planes, stride, downsample)]
        self.inplanes = planes * block.expansion
        for _ in range(1, blocks):
            layers.append(block(self.inplanes, planes))
        return nn.Sequential(*layers)

    def forward(self, x) -> List[torch.Tensor]:
        feats = [x]
        x = self.relu(self.bn1(self.conv1(x)))
        feats.append(x)
        x = self.layer1(self.maxpool(x))
        feats.append(x)
        x = self.layer2(x)
        feats.append(x)
        x = self.layer3(x)
        feats.append(x)
        x = self.layer4(x)
        feats.append(x)
        return feats


class EncoderUnet(nn.Module):
    """Restatement of ``smp.Unet(name, encoder_weights=None, in_channels=3, classes=classes)``."""

    def __init__(self, name: str, classes: int = 1):
        super().__init__()
        self.encoder = ResNetEncoder(name)
        self.decoder = O.UnetDecoder(self.encoder.out_channels)
        self.segmentation_head = O.SegmentationHead(16, classes)
        O._initialize_decoder(self.decoder)
        O._initialize_head(self.segmentation_head)

    def forward(self, x):
        return self.segmentation_head(self.decoder(*self.encoder(x)))


def build(name: str, classes: int = 1, seed: Optional[int] = None) -> EncoderUnet:
    if seed is not None:
        O.set_seed(seed)
    return EncoderUnet(name, classes)
