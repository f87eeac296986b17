"""Plain Vision Transformers (Dosovitskiy et al., 2021, in the form of Beyer
et al., "Better plain ViT baselines for ImageNet-1k", 2022) on the
framework's HIP-backed modules: global-average-pool head, no class token,
fixed 2-D sin-cos positions.

The token grid stays a 4-D channels_last activation [N, D, H, W] from the
patch conv to the pool: channels_last memory is the token-major [N, L, D]
matrix, so the pointwise layers are 1x1 convs on the MFMA implicit GEMM (not
``Linear``), the qkv conv's output is the packed matrix the attention kernels
of ops/hip/attn.hip read, and LayerNorm, GELU and the layer scale with the
residual add are the kernels of ops/hip/ln.hip.  The head dimension is 64.

A block is pre-norm:  x = ls1(attn(norm1(x)), x);  x = ls2(pw2(gelu(pw1(
norm2(x)))), x), the layer scale starting at 1e-4 (DeiT-III) and doing the
residual add.  No dropout, no stochastic depth.

``cifar_stem=True`` makes the patch 4 instead of 16, for 32x32 inputs (an 8x8
grid, L = 64).

State-dict layout (D the width, B = 0..depth-1 the block, p the patch):

    patch.{weight,bias}                  [D, 3, p, p]
    blocks.B.norm1.{weight,bias}         [D]
    blocks.B.attn.qkv.{weight,bias}      [3D, D, 1, 1]   rows: q | k | v,
                                                         head h at 64h of each
    blocks.B.attn.proj.{weight,bias}     [D, D, 1, 1]
    blocks.B.ls1.gamma                   [D]
    blocks.B.norm2.{weight,bias}         [D]
    blocks.B.pw1.{weight,bias}           [4D, D, 1, 1]
    blocks.B.pw2.{weight,bias}           [D, 4D, 1, 1]
    blocks.B.ls2.gamma                   [D]
    norm.{weight,bias}                   [D]
    fc.{weight,bias}                     [num_classes, D]

The position table (``pos.pos``) is a non-persistent buffer and is not in the
state dict.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from ..ops.modules import (GELU, AdaptiveAvgPool2d, Attention2d, Conv2d,
                           LayerNorm2d, LayerScale, Linear, PosEmbed2d)


class Block(nn.Module):
    def __init__(self, dim: int, num_heads: int):
        super().__init__()
        self.norm1 = LayerNorm2d(dim)
        self.attn = Attention2d(dim, num_heads)
        self.ls1 = LayerScale(dim, init=1e-4)
        self.norm2 = LayerNorm2d(dim)
        self.pw1 = Conv2d(dim, 4 * dim, 1)
        self.act = GELU()
        self.pw2 = Conv2d(4 * dim, dim, 1)
        self.ls2 = LayerScale(dim, init=1e-4)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = self.ls1(self.attn(self.norm1(x)), x)
        return self.ls2(self.pw2(self.act(self.pw1(self.norm2(x)))), x)


class ViT(nn.Module):
    def __init__(self, dim: int, num_heads: int, depth: int,
                 num_classes: int = 1000, cifar_stem: bool = False):
        super().__init__()
        patch = 4 if cifar_stem else 16
        grid = 8 if cifar_stem else 14
        self.patch = Conv2d(3, dim, patch, stride=patch)
        self.pos = PosEmbed2d(dim, grid, grid)
        self.blocks = nn.Sequential(
            *[Block(dim, num_heads) for _ in range(depth)])
        self.norm = LayerNorm2d(dim)
        self.avgpool = AdaptiveAvgPool2d((1, 1))
        self.fc = Linear(dim, num_classes)

        for m in self.modules():
            if isinstance(m, (Conv2d, Linear)):
                nn.init.trunc_normal_(m.weight, std=0.02)
                nn.init.zeros_(m.bias)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = self.blocks(self.pos(self.patch(x)))
        x = self.avgpool(self.norm(x))
        return self.fc(torch.flatten(x, 1))


def vit_tiny(num_classes=1000, cifar_stem=False):
    return ViT(192, 3, 12, num_classes, cifar_stem)


def vit_small(num_classes=1000, cifar_stem=False):
    return ViT(384, 6, 12, num_classes, cifar_stem)
