"""Yardsticks for the native TransNetV2 trunk, all torch on the CPU.

``trunk_f32`` is the ``nn.Module`` trunk as it stands.  ``trunk_bf16`` is
the same trunk with the roundings a bf16 implementation cannot avoid: conv
weights, every conv input and every BatchNorm output are rounded to bf16,
everything between stays f32.  Its error against ``trunk_f32`` is what bf16
storage costs on this net, and the native trunk is held to a multiple of it
(test_gpu_transnet_native.py); nothing here looks at the code under test.

``conv_bound`` is the single-kernel tolerance: one bf16 ulp of the wanted
value plus the f32 accumulation bound on both sides.
"""

from __future__ import annotations

import torch
from torch.nn import functional as F


def rb(x: torch.Tensor) -> torch.Tensor:
    """Round to bf16, keep f32."""
    return x.to(torch.bfloat16).float()


def _prep(frames_u8: torch.Tensor) -> torch.Tensor:
    return frames_u8.permute(0, 4, 1, 2, 3).float() / 255.0


@torch.no_grad()
def trunk_f32(net, frames_u8: torch.Tensor) -> list[torch.Tensor]:
    """The three pooled stack outputs (B,C,T,h,w) of ``net.SDDCNN``, f32."""
    x = _prep(frames_u8)
    feats = []
    for stack in net.SDDCNN:
        x = stack(x)
        feats.append(x)
    return feats


@torch.no_grad()
def trunk_bf16(net, frames_u8: torch.Tensor) -> list[torch.Tensor]:
    """``trunk_f32`` with bf16 conv weights, conv inputs and BatchNorm
    outputs."""
    x = _prep(frames_u8)
    feats = []
    for stack in net.SDDCNN:
        shortcut = None
        for block in stack.DDCNN:
            ys = []
            for conv in (block.Conv3D_1, block.Conv3D_2, block.Conv3D_4, block.Conv3D_8):
                spatial, temporal = conv.layers
                s = F.conv3d(rb(x), rb(spatial.weight), padding=spatial.padding)
                ys.append(F.conv3d(rb(s), rb(temporal.weight), dilation=temporal.dilation,
                                   padding=temporal.padding))
            x = rb(block.bn(torch.cat(ys, dim=1)))
            if block._activation:
                x = F.relu(x)
            if shortcut is None:
                shortcut = x
        x = stack.pool(F.relu(x) + shortcut)
        feats.append(x)
    return feats


def rel_l2(got: torch.Tensor, want: torch.Tensor) -> float:
    got, want = got.double(), want.double()
    return float((got - want).norm() / want.norm())


def conv_bound(want: torch.Tensor, abs_sum: torch.Tensor, k: int) -> torch.Tensor:
    """Allowed |got - want| of one conv: 2^-7 |want| + 2 K 2^-24 S, with S
    the same conv of |x| and |w|."""
    return 2.0 ** -7 * want.abs() + 2.0 * k * 2.0 ** -24 * abs_sum
