"""TransNetV2 conv trunk on the hand-written bf16 kernels (csrc/cc_conv.hip).

The three ``StackedDDCNNV2`` stacks of ``models/transnetv2.py`` (reference
transnetv2.py:152-347), repacked for channels-last bf16:

* a DDCNN block's four spatial convs share their input, so their weights
  are one ``[8F][3][3][Cin]`` tensor and one ``cc_conv3x3_bf16`` launch
  (branch b = output channels ``[b*2F, (b+1)*2F)``);
* its four dilated temporal convs are one ``cc_tconv3_bf16`` launch with
  weights ``[4][F][3][2F]``; the block's eval BatchNorm is folded into them
  in f32 (scale into the weights before their one bf16 rounding, offset into
  an f32 bias), and the kernel's epilogue is ``relu(acc + bias)`` plus, on
  the stack's last block, the dense shortcut;
* ``cc_avgpool2x2_bf16`` closes the stack.

``pack_trunk`` works from any state dict of ``_TransNetV2`` on the CPU and
knows nothing of where the weights came from; ``NativeTrunk`` uploads the
packed tensors and runs ``(B, T, 27, 48, 3)`` u8 windows to the three pooled
stack outputs, channels-last ``(B, T, h, w, 4F)`` bf16.  The heads stay on
torch (``_TransNetV2.heads``).  No fallback: a missing library or kernel
raises.
"""

from __future__ import annotations

from dataclasses import dataclass

import torch

from cosmos_curate_amd import hotpath

_DILATIONS = (1, 2, 4, 8)
_BN_EPS = 1e-3  # DilatedDCNNV2.bn


@dataclass
class PackedBlock:
    """One DDCNN block, f32 on the CPU, in the kernels' layouts."""

    spatial: torch.Tensor   # [8F, 3, 3, Cin]
    temporal: torch.Tensor  # [4, F, 3, 2F], BatchNorm scale folded in
    bias: torch.Tensor      # [4F], the BatchNorm offset

    @property
    def filters(self) -> int:
        return self.temporal.shape[1]

    @property
    def in_filters(self) -> int:
        return self.spatial.shape[3]


def pack_trunk(state_dict: dict[str, torch.Tensor]) -> list[list[PackedBlock]]:
    """The ``SDDCNN.*`` entries of a ``_TransNetV2`` state dict as stacks of
    ``PackedBlock`` (f32; the caller rounds to bf16 once, on upload)."""
    sd = {k: v.detach().float().cpu() for k, v in state_dict.items()
          if k.startswith("SDDCNN.")}
    stacks: list[list[PackedBlock]] = []
    s = 0
    while f"SDDCNN.{s}.DDCNN.0.bn.weight" in sd:
        blocks = []
        k = 0
        while f"SDDCNN.{s}.DDCNN.{k}.bn.weight" in sd:
            p = f"SDDCNN.{s}.DDCNN.{k}."
            scale = sd[p + "bn.weight"] / torch.sqrt(sd[p + "bn.running_var"] + _BN_EPS)
            bias = sd[p + "bn.bias"] - sd[p + "bn.running_mean"] * scale
            spatial, temporal = [], []
            for d in _DILATIONS:
                ws = sd[p + f"Conv3D_{d}.layers.0.weight"]  # [2F, Cin, 1, 3, 3]
                wt = sd[p + f"Conv3D_{d}.layers.1.weight"]  # [F, 2F, 3, 1, 1]
                if p + f"Conv3D_{d}.layers.1.bias" in sd:
                    raise ValueError("temporal conv bias is not part of the packed trunk")
                spatial.append(ws[:, :, 0].permute(0, 2, 3, 1))
                temporal.append(wt[:, :, :, 0, 0].permute(0, 2, 1))
            f = temporal[0].shape[0]
            tw = torch.stack(temporal) * scale.view(4, f, 1, 1)
            blocks.append(PackedBlock(torch.cat(spatial).contiguous(),
                                      tw.contiguous(), bias.contiguous()))
            k += 1
        if len(blocks) < 2:
            # a one-block stack's shortcut is taken before the relu, which
            # the temporal kernel's epilogue does not express
            raise ValueError("a stack needs at least two DDCNN blocks")
        stacks.append(blocks)
        s += 1
    if not stacks:
        raise ValueError("state dict holds no SDDCNN trunk")
    return stacks


def window_indices(total: int) -> list[torch.Tensor]:
    """Source-frame indices of every window of an ``total``-frame video: the
    rule of ``_get_batches`` (transnetv2_extraction_stages.py; 50-frame
    stride, frames i-25 .. i+74 clipped to the video, the first window
    padded in front with frame 0; tail windows are shorter than 100, as
    there) as gather indices, so the windows can be built on the device."""
    out = []
    for i in range(0, total + (-total % 50), 50):
        lo, hi = max(i - 25, 0), min(i + 75, total)
        idx = torch.arange(lo, hi, dtype=torch.int64)
        if i < 25:
            idx = torch.cat([torch.zeros(25 - i, dtype=torch.int64), idx])
        out.append(idx)
    return out


class NativeTrunk:
    """The packed trunk on one device."""

    def __init__(self, state_dict: dict[str, torch.Tensor],
                 device: torch.device | str = "cuda") -> None:
        hotpath.require_gpu()
        self.device = torch.device(device)
        self.stacks = []
        for blocks in pack_trunk(state_dict):
            self.stacks.append([
                (b.spatial.to(self.device, torch.bfloat16),
                 b.temporal.to(self.device, torch.bfloat16),
                 b.bias.to(self.device), b.in_filters, b.filters)
                for b in blocks
            ])
        if self.stacks[0][0][3] != 3:
            raise ValueError("the first spatial conv must read 3 channels")

    @torch.no_grad()
    def __call__(self, frames_u8: torch.Tensor) -> list[torch.Tensor]:
        if (frames_u8.dtype != torch.uint8 or frames_u8.ndim != 5
                or frames_u8.shape[-1] != 3 or not frames_u8.is_cuda):
            raise ValueError("frames must be a (B, T, H, W, 3) uint8 device tensor")
        b, t, h, w, _ = frames_u8.shape
        n = b * t
        feats = []
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream

            def new(*shape):
                return torch.empty(shape, dtype=torch.bfloat16, device=self.device)

            x = frames_u8.contiguous()
            for blocks in self.stacks:
                first = None
                for i, (ws, wt, bias, cin, f) in enumerate(blocks):
                    s = new(n, h, w, 8 * f)
                    if cin == 3:
                        hotpath.conv3x3_u8(x.data_ptr(), ws.data_ptr(), s.data_ptr(),
                                           n, h, w, 8 * f, stream)
                    else:
                        hotpath.conv3x3_bf16(x.data_ptr(), ws.data_ptr(), s.data_ptr(),
                                             n, h, w, cin, 8 * f, stream)
                    y = new(n, h, w, 4 * f)
                    # the stack tail relu(x) + shortcut rides on the last block
                    last = i == len(blocks) - 1 and first is not None
                    hotpath.tconv3_bf16(s.data_ptr(), wt.data_ptr(), bias.data_ptr(),
                                        first.data_ptr() if last else 0,
                                        y.data_ptr(), b, t, h * w, f, stream)
                    if first is None:
                        first = y
                    x = y
                p = new(n, h // 2, w // 2, x.shape[-1])
                hotpath.avgpool2x2_bf16(x.data_ptr(), p.data_ptr(), n, h, w,
                                        x.shape[-1], stream)
                h, w = h // 2, w // 2
                feats.append(p.view(b, t, h, w, -1))
                x = p
        return feats
