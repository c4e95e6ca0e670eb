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
stack outputs, channels-last ``(B, T, h, w, 4F)`` bf16.  No fallback: a
missing library or kernel raises.

The heads stay on torch (``_TransNetV2.heads``) unless asked for:
``pack_heads`` / ``NativeHeads`` are the same pair for everything after the
trunk, on the kernels of csrc/cc_tnheads.hip (DESIGN.md "TransNetV2 native
heads"): colour histograms, the frame-similarity embedding, the two
101-frame similarity bands with their ``Linear(101, 128)``, ``fc1`` with its
weight split into a bf16 hi and lo part, and the classifier.  They sum in a
fixed order, so all windows of a forward go through them in one pass.
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


_LOOKUP = 101  # lookup window of both similarity heads


@dataclass
class PackedHeads:
    """Everything after the trunk, on the CPU, in the kernels' layouts (f32
    unless noted)."""

    proj_wt: torch.Tensor     # [sum 4F, 128], frame_sim_layer.projection.weight^T
    proj_b: torch.Tensor      # [128]
    sim_fc_wt: torch.Tensor   # [101, 128], frame_sim_layer.fc.weight^T
    sim_fc_b: torch.Tensor    # [128]
    hist_fc_wt: torch.Tensor  # [101, 128], color_hist_layer.fc.weight^T
    hist_fc_b: torch.Tensor   # [128]
    fc1_hi: torch.Tensor      # bf16 [N, 256 + KF]: bf16(w)
    fc1_lo: torch.Tensor      # bf16 [N, 256 + KF]: bf16(w - float(fc1_hi))
    fc1_b: torch.Tensor       # [N]
    cls_w: torch.Tensor       # [N]
    cls_b: float


def pack_heads(state_dict: dict[str, torch.Tensor]) -> PackedHeads:
    """The head entries of a ``_TransNetV2`` state dict as ``PackedHeads``.
    ``fc1.weight``'s columns are already in the kernels' order: colour head
    (128), frame-similarity head (128), then stack 3's pooled output
    flattened ``(h, w, C)``."""
    names = ("frame_sim_layer.projection.weight", "frame_sim_layer.projection.bias",
             "frame_sim_layer.fc.weight", "frame_sim_layer.fc.bias",
             "color_hist_layer.fc.weight", "color_hist_layer.fc.bias",
             "fc1.weight", "fc1.bias", "cls_layer1.weight", "cls_layer1.bias")
    missing = [n for n in names if n not in state_dict]
    if missing:
        raise ValueError(f"state dict holds no heads: {', '.join(missing)} missing")
    proj_w, proj_b, sim_w, sim_b, hist_w, hist_b, fc1_w, fc1_b, cls_w, cls_b = (
        state_dict[n].detach().float().cpu() for n in names)

    def want(name: str, t: torch.Tensor, *shape: int | None) -> None:
        if t.ndim != len(shape) or any(s is not None and s != d
                                       for s, d in zip(shape, t.shape)):
            raise ValueError(f"{name} has shape {tuple(t.shape)}, expected "
                             f"{tuple('any' if s is None else s for s in shape)}")

    want("frame_sim_layer.projection.weight", proj_w, 128, None)
    want("frame_sim_layer.projection.bias", proj_b, 128)
    for n, w, b in (("frame_sim_layer", sim_w, sim_b), ("color_hist_layer", hist_w, hist_b)):
        want(n + ".fc.weight", w, 128, _LOOKUP)
        want(n + ".fc.bias", b, 128)
    want("fc1.weight", fc1_w, None, None)
    n_out, k = fc1_w.shape
    want("fc1.bias", fc1_b, n_out)
    want("cls_layer1.weight", cls_w, 1, n_out)
    want("cls_layer1.bias", cls_b, 1)
    if proj_w.shape[1] > 512:
        raise ValueError("the projection reads at most 512 channel means")
    if n_out % 16 != 0 or k <= 256 or (k - 256) % 32 != 0:
        raise ValueError(f"fc1.weight {tuple(fc1_w.shape)}: outputs must be a multiple "
                         "of 16, inputs 256 plus a multiple of 32")
    hi = fc1_w.to(torch.bfloat16)
    lo = (fc1_w - hi.float()).to(torch.bfloat16)
    return PackedHeads(
        proj_w.t().contiguous(), proj_b.contiguous(),
        sim_w.t().contiguous(), sim_b.contiguous(),
        hist_w.t().contiguous(), hist_b.contiguous(),
        hi.contiguous(), lo.contiguous(), fc1_b.contiguous(),
        cls_w[0].contiguous(), float(cls_b[0]))


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


class NativeHeads:
    """The packed heads on one device: ``(frames_u8 (B,T,H,W,3), feats from
    NativeTrunk) -> (B,T,1)`` f32 probabilities, six launches and no torch
    arithmetic between them."""

    def __init__(self, state_dict: dict[str, torch.Tensor],
                 device: torch.device | str = "cuda") -> None:
        hotpath.require_gpu()
        self.device = torch.device(device)
        p = pack_heads(state_dict)
        self.cls_b = p.cls_b
        (self.proj_wt, self.proj_b, self.sim_fc_wt, self.sim_fc_b, self.hist_fc_wt,
         self.hist_fc_b, self.fc1_hi, self.fc1_lo, self.fc1_b, self.cls_w) = (
            t.to(self.device) for t in (
                p.proj_wt, p.proj_b, p.sim_fc_wt, p.sim_fc_b, p.hist_fc_wt,
                p.hist_fc_b, p.fc1_hi, p.fc1_lo, p.fc1_b, p.cls_w))

    @torch.no_grad()
    def __call__(self, frames_u8: torch.Tensor, feats: list[torch.Tensor]) -> torch.Tensor:
        if (frames_u8.dtype != torch.uint8 or frames_u8.ndim != 5
                or frames_u8.shape[-1] != 3 or not frames_u8.is_cuda):
            raise ValueError("frames must be a (B, T, H, W, 3) uint8 device tensor")
        b, t, h, w, _ = frames_u8.shape
        n = b * t
        for f in feats:
            if (f.dtype != torch.bfloat16 or f.ndim != 5 or tuple(f.shape[:2]) != (b, t)
                    or not f.is_cuda or not f.is_contiguous()):
                raise ValueError("features must be contiguous (B, T, h, w, C) bf16 "
                                 "device tensors of the frames' windows")
        if sum(f.shape[-1] for f in feats) != self.proj_wt.shape[0]:
            raise ValueError("the features' channels do not match the projection")
        n_out, k = self.fc1_hi.shape
        kf = feats[-1][0, 0].numel()
        if k != 256 + kf:
            raise ValueError(f"fc1 reads {k} inputs, the heads give 256 + {kf}")
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream

            def new(*shape):
                return torch.empty(shape, dtype=torch.float32, device=self.device)

            x = frames_u8.contiguous()
            hist, emb, hd, y, prob = new(n, 512), new(n, 128), new(n, 256), new(n, n_out), new(n)
            hotpath.tn_hist512_u8(x.data_ptr(), hist.data_ptr(), n, h * w, stream)
            hotpath.tn_framesim_embed(
                [(f.data_ptr(), f.shape[2] * f.shape[3], f.shape[4]) for f in feats],
                self.proj_wt.data_ptr(), self.proj_b.data_ptr(), emb.data_ptr(), n, 128,
                stream)
            # _TransNetV2.heads' concatenation: colour head, similarity head, features
            hotpath.tn_simband_fc(hist.data_ptr(), self.hist_fc_wt.data_ptr(),
                                  self.hist_fc_b.data_ptr(), hd.data_ptr(), b, t, 512,
                                  256, 0, stream)
            hotpath.tn_simband_fc(emb.data_ptr(), self.sim_fc_wt.data_ptr(),
                                  self.sim_fc_b.data_ptr(), hd.data_ptr(), b, t, 128,
                                  256, 128, stream)
            # stack 3's pooled output is (h, w, C)-contiguous per frame: the
            # flatten order of the heads, read in place
            hotpath.tn_fc1_relu(hd.data_ptr(), feats[-1].data_ptr(), self.fc1_hi.data_ptr(),
                                self.fc1_lo.data_ptr(), self.fc1_b.data_ptr(), y.data_ptr(),
                                n, 256, kf, n_out, stream)
            hotpath.tn_cls_sigmoid(y.data_ptr(), self.cls_w.data_ptr(), self.cls_b,
                                   prob.data_ptr(), n, n_out, stream)
        return prob.view(b, t, 1)
