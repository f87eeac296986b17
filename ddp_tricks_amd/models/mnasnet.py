"""MnasNet-B1 (Tan et al., 2019; torchvision's ``mnasnet1_0``) on the
framework's HIP-backed modules.

Inverted residuals with depthwise 3x3 and 5x5 convs: the 3x3 run on the direct
kernels of ops/hip/dwconv.hip, the 5x5 on the LDS-tile kernels of
ops/hip/dwconvk.hip, the 1x1 expand / project convs on the MFMA implicit GEMM
(all channel counts are multiples of 8).  Every conv goes through ``conv_bn``,
so the BN statistics come out of the conv kernels.  The block's last BN has no
ReLU and, when stride is 1 and in == out, takes the block input as its
``residual``.  Convs carry no bias.

``cifar_stem=True`` gives the stem stride 1 for 32x32 inputs.

State-dict layout (S = 0..5 the stack, B the block within it):

    stem.conv1.weight                  [32, 3, 3, 3]
    stem.bn1.{weight,bias,running_mean,running_var,num_batches_tracked}
    stem.dw.weight                     [32, 1, 3, 3]    depthwise
    stem.bn_dw.{...}
    stem.pw.weight                     [16, 32, 1, 1]
    stem.bn_pw.{...}
    stacks.S.B.expand.weight           [Cin*e, Cin, 1, 1]
    stacks.S.B.bn_expand.{...}
    stacks.S.B.dw.weight               [Cin*e, 1, k, k] depthwise
    stacks.S.B.bn_dw.{...}
    stacks.S.B.project.weight          [Cout, Cin*e, 1, 1]
    stacks.S.B.bn_project.{...}
    head.weight                        [1280, 320, 1, 1]
    bn_head.{...}
    fc.{weight,bias}                   [num_classes, 1280]
"""
from __future__ import annotations

import torch
import torch.nn as nn

from ..ops.functional import conv_bn
from ..ops.modules import AdaptiveAvgPool2d, BatchNorm2d, Conv2d, Linear

# (out, kernel, stride, expansion, repeats) of the six stacks
_STACKS = [(24, 3, 2, 3, 3), (40, 5, 2, 3, 3), (80, 5, 2, 6, 3),
           (96, 3, 1, 6, 2), (192, 5, 2, 6, 4), (320, 3, 1, 6, 1)]


class InvertedResidual(nn.Module):
    def __init__(self, cin: int, cout: int, k: int, stride: int, expand: int):
        super().__init__()
        mid = cin * expand
        self.skip = stride == 1 and cin == cout
        self.expand = Conv2d(cin, mid, 1, bias=False)
        self.bn_expand = BatchNorm2d(mid, fuse_relu=True)
        self.dw = Conv2d(mid, mid, k, stride=stride, padding=k // 2,
                         groups=mid, bias=False)
        self.bn_dw = BatchNorm2d(mid, fuse_relu=True)
        self.project = Conv2d(mid, cout, 1, bias=False)
        self.bn_project = BatchNorm2d(cout)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        out = conv_bn(self.expand, self.bn_expand, x)
        out = conv_bn(self.dw, self.bn_dw, out)
        return conv_bn(self.project, self.bn_project, out,
                       residual=x if self.skip else None)


class _Stem(nn.Module):
    def __init__(self, stride: int):
        super().__init__()
        self.conv1 = Conv2d(3, 32, 3, stride=stride, padding=1, bias=False)
        self.bn1 = BatchNorm2d(32, fuse_relu=True)
        self.dw = Conv2d(32, 32, 3, padding=1, groups=32, bias=False)
        self.bn_dw = BatchNorm2d(32, fuse_relu=True)
        self.pw = Conv2d(32, 16, 1, bias=False)
        self.bn_pw = BatchNorm2d(16)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = conv_bn(self.conv1, self.bn1, x)
        x = conv_bn(self.dw, self.bn_dw, x)
        return conv_bn(self.pw, self.bn_pw, x)


class MnasNet(nn.Module):
    def __init__(self, num_classes: int = 1000, cifar_stem: bool = False):
        super().__init__()
        self.stem = _Stem(1 if cifar_stem else 2)
        stacks, cin = [], 16
        for cout, k, stride, expand, repeats in _STACKS:
            blocks = []
            for b in range(repeats):
                blocks.append(InvertedResidual(cin, cout, k,
                                               stride if b == 0 else 1,
                                               expand))
                cin = cout
            stacks.append(nn.Sequential(*blocks))
        self.stacks = nn.Sequential(*stacks)
        self.head = Conv2d(cin, 1280, 1, bias=False)
        self.bn_head = BatchNorm2d(1280, fuse_relu=True)
        self.avgpool = AdaptiveAvgPool2d((1, 1))
        self.fc = Linear(1280, num_classes)

        for m in self.modules():
            if isinstance(m, Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out",
                                        nonlinearity="relu")
            elif isinstance(m, BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = self.stacks(self.stem(x))
        x = conv_bn(self.head, self.bn_head, x)
        x = self.avgpool(x)
        return self.fc(torch.flatten(x, 1))


def mnasnet1_0(num_classes=1000, cifar_stem=False):
    return MnasNet(num_classes, cifar_stem)
