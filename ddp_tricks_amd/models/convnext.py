"""ConvNeXt-T (Liu et al., 2022; torchvision's ``convnext_tiny``) on the
framework's HIP-backed modules.

A block is depthwise 7x7 (pad 3, bias) -> LayerNorm over C -> 1x1 conv C -> 4C
-> GELU -> 1x1 conv 4C -> C -> layer scale, added to the block input.  The
depthwise conv runs on the LDS-tile kernels of ops/hip/dwconvk.hip, the
pointwise layers are 1x1 convs on the MFMA implicit GEMM (not ``Linear``: the
activations never leave channels_last), and LayerNorm, GELU and the layer
scale with the residual add are the kernels of ops/hip/ln.hip.  There is no
BatchNorm anywhere; every conv carries a bias.  The 4x4 stride-4 stem and the
2x2 stride-2 downsampling convs run on the dense conv as well.  Stochastic
depth is not implemented.

``cifar_stem=True`` makes the stem a 2x2 stride-2 conv for 32x32 inputs.

State-dict layout (S = 0..3 the stage of width d = 96, 192, 384, 768 and depth
3, 3, 9, 3; B the block within it):

    stem.conv.{weight,bias}            [96, 3, 4, 4]    ([96, 3, 2, 2] cifar)
    stem.norm.{weight,bias}            [96]
    downsample.S.norm.{weight,bias}    [d_S]            S = 0..2
    downsample.S.conv.{weight,bias}    [d_S+1, d_S, 2, 2]
    stages.S.B.dw.{weight,bias}        [d, 1, 7, 7]     depthwise
    stages.S.B.norm.{weight,bias}      [d]
    stages.S.B.pw1.{weight,bias}       [4d, d, 1, 1]
    stages.S.B.pw2.{weight,bias}       [d, 4d, 1, 1]
    stages.S.B.scale.gamma             [d]
    norm.{weight,bias}                 [768]
    fc.{weight,bias}                   [num_classes, 768]
"""
from __future__ import annotations

import torch
import torch.nn as nn

from ..ops.modules import (GELU, AdaptiveAvgPool2d, Conv2d, LayerNorm2d,
                           LayerScale, Linear)

_DEPTHS = (3, 3, 9, 3)
_DIMS = (96, 192, 384, 768)


class Block(nn.Module):
    def __init__(self, dim: int):
        super().__init__()
        self.dw = Conv2d(dim, dim, 7, padding=3, groups=dim)
        self.norm = LayerNorm2d(dim)
        self.pw1 = Conv2d(dim, 4 * dim, 1)
        self.act = GELU()
        self.pw2 = Conv2d(4 * dim, dim, 1)
        self.scale = LayerScale(dim)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        u = self.pw2(self.act(self.pw1(self.norm(self.dw(x)))))
        return self.scale(u, x)


class _Stem(nn.Module):
    def __init__(self, dim: int, patch: int):
        super().__init__()
        self.conv = Conv2d(3, dim, patch, stride=patch)
        self.norm = LayerNorm2d(dim)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.norm(self.conv(x))


class _Downsample(nn.Module):
    def __init__(self, cin: int, cout: int):
        super().__init__()
        self.norm = LayerNorm2d(cin)
        self.conv = Conv2d(cin, cout, 2, stride=2)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.conv(self.norm(x))


class ConvNeXt(nn.Module):
    def __init__(self, num_classes: int = 1000, cifar_stem: bool = False):
        super().__init__()
        self.stem = _Stem(_DIMS[0], 2 if cifar_stem else 4)
        self.stages = nn.ModuleList(
            nn.Sequential(*[Block(d) for _ in range(n)])
            for n, d in zip(_DEPTHS, _DIMS))
        self.downsample = nn.ModuleList(
            _Downsample(a, b) for a, b in zip(_DIMS[:-1], _DIMS[1:]))
        self.avgpool = AdaptiveAvgPool2d((1, 1))
        self.norm = LayerNorm2d(_DIMS[-1])
        self.fc = Linear(_DIMS[-1], num_classes)

        for m in self.modules():
            if isinstance(m, (Conv2d, Linear)):
                nn.init.trunc_normal_(m.weight, std=0.02)
                nn.init.zeros_(m.bias)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = self.stem(x)
        for s, stage in enumerate(self.stages):
            if s:
                x = self.downsample[s - 1](x)
            x = stage(x)
        x = self.norm(self.avgpool(x))
        return self.fc(torch.flatten(x, 1))


def convnext_tiny(num_classes=1000, cifar_stem=False):
    return ConvNeXt(num_classes, cifar_stem)
