"""MobileNetV1 (Howard et al., 2017) on the framework's HIP-backed modules.

The depthwise-separable family: every block is a depthwise 3x3 conv (the
direct VALU kernels of ops/hip/dwconv.hip) and a pointwise 1x1 conv (the MFMA
implicit GEMM; all channel counts are multiples of 8), each followed by
BatchNorm with the ReLU fused into its epilogue.  Both convs go through
``conv_bn``, so the BN statistics come out of the conv kernels and neither BN
runs a statistics pass.  Convs carry no bias.

``width_mult`` scales every channel count (rounded to a multiple of 8, at
least 8); ``cifar_stem=True`` gives the stem stride 1 for 32x32 inputs.

State-dict layout (N = 0..12, the block index):

    conv1.weight                       [32, 3, 3, 3]    stem
    bn1.{weight,bias,running_mean,running_var,num_batches_tracked}
    blocks.N.dw.weight                 [Cin, 1, 3, 3]   depthwise
    blocks.N.bn_dw.{weight,bias,running_mean,running_var,num_batches_tracked}
    blocks.N.pw.weight                 [Cout, Cin, 1, 1] pointwise
    blocks.N.bn_pw.{weight,bias,running_mean,running_var,num_batches_tracked}
    fc.{weight,bias}                   [num_classes, 1024]
"""
from __future__ import annotations

import torch
import torch.nn as nn

from ..ops.functional import conv_bn
from ..ops.modules import AdaptiveAvgPool2d, BatchNorm2d, Conv2d, Linear

# (in, out, stride) of the 13 depthwise-separable blocks at width 1.0
_BLOCKS = ([(32, 64, 1), (64, 128, 2), (128, 128, 1), (128, 256, 2),
            (256, 256, 1), (256, 512, 2)]
           + [(512, 512, 1)] * 5
           + [(512, 1024, 2), (1024, 1024, 1)])


def _width(c: int, mult: float) -> int:
    return max(8, int(round(c * mult / 8.0)) * 8)


class DWSeparable(nn.Module):
    def __init__(self, cin: int, cout: int, stride: int):
        super().__init__()
        self.dw = Conv2d(cin, cin, 3, stride=stride, padding=1, groups=cin,
                         bias=False)
        self.bn_dw = BatchNorm2d(cin, fuse_relu=True)
        self.pw = Conv2d(cin, cout, 1, bias=False)
        self.bn_pw = BatchNorm2d(cout, fuse_relu=True)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = conv_bn(self.dw, self.bn_dw, x)
        return conv_bn(self.pw, self.bn_pw, x)


class MobileNetV1(nn.Module):
    def __init__(self, num_classes: int = 1000, width_mult: float = 1.0,
                 cifar_stem: bool = False):
        super().__init__()
        c = _width(32, width_mult)
        self.conv1 = Conv2d(3, c, 3, stride=1 if cifar_stem else 2, padding=1,
                            bias=False)
        self.bn1 = BatchNorm2d(c, fuse_relu=True)
        self.blocks = nn.Sequential(*[
            DWSeparable(_width(i, width_mult), _width(o, width_mult), s)
            for i, o, s in _BLOCKS])
        self.avgpool = AdaptiveAvgPool2d((1, 1))
        self.fc = Linear(_width(1024, width_mult), num_classes)

        for m in self.modules():
            if isinstance(m, Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out",
                                        nonlinearity="relu")
            elif isinstance(m, BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = conv_bn(self.conv1, self.bn1, x)
        x = self.blocks(x)
        x = self.avgpool(x)
        return self.fc(torch.flatten(x, 1))


def mobilenet_v1(num_classes=1000, width_mult=1.0, cifar_stem=False):
    return MobileNetV1(num_classes, width_mult, cifar_stem)
