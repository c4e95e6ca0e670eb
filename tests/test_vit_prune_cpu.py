"""Last-layer CLS pruning of ClipVisionTowerAMD, pinned on the CPU.

The pruned tower (default) computes the last encoder layer's Q, attention,
out-proj, LN2 and MLP for the CLS rows only; the full tower computes them
for every token and then keeps row 0.  Both must give the same embedding.
_linear is patched to torch, so this pins the Python control flow (weight
slices, row selection, residual rows) without a GPU; the HIP kernels are
pinned in tests/test_gpu_vit_prune.py.
"""

import pytest
import torch

from cosmos_curate_amd.models import clip_weights as cw
from cosmos_curate_amd.models.clip_vit import ClipVisionTowerAMD


def _torch_linear(self, x, w, b, act=0, residual=None):
    y = torch.nn.functional.linear(x.float(), w.float(), b.float() if b is not None else None)
    if act == 1:
        y = y * torch.sigmoid(1.702 * y)
    if residual is not None:
        y = y + residual.float()
    return y.to(torch.bfloat16)


@pytest.mark.parametrize("layers", [2, 1])
def test_pruned_matches_full(monkeypatch, layers):
    # head dim 64 (the GPU route's contract), 2x2 patches + CLS = 5 tokens
    cfg = cw.VitConfig("tiny_prune", hidden=128, layers=layers, heads=2,
                       intermediate=256, patch=32, proj=64, image=64)
    weights = cw.make_clip_vit_weights(cfg)
    monkeypatch.setattr(ClipVisionTowerAMD, "_linear", _torch_linear)
    tower = ClipVisionTowerAMD(weights, cfg)
    assert tower.prune_last_layer  # pruned is the default

    # count GEMM rows to prove the pruned route really is taken
    rows = []
    inner = ClipVisionTowerAMD._linear

    def counting(self, x, w, b, act=0, residual=None):
        rows.append(x.shape[0])
        return inner(self, x, w, b, act, residual)

    monkeypatch.setattr(ClipVisionTowerAMD, "_linear", counting)

    torch.manual_seed(layers)
    n, seq = 3, 5
    pixels = torch.randn(n, 3, 64, 64)
    pruned = tower(pixels)
    pruned_rows, rows = rows, []
    tower.prune_last_layer = False
    full = tower(pixels)
    full_rows = rows

    assert pruned.shape == full.shape == (n, 64)
    cos = torch.sum(pruned * full, dim=1)  # both unit-norm
    print("per-frame cosine pruned vs full:", cos.tolist())
    assert torch.all(cos >= 0.9999), cos

    # full: patch + 4 GEMMs/layer on n*seq rows + projection on n rows;
    # pruned: the last layer is K/V on n*seq rows, then Q, out, fc1, fc2
    # on n rows
    assert full_rows == [n * 4] + [n * seq] * (4 * layers) + [n]
    assert pruned_rows == (
        [n * 4] + [n * seq] * (4 * (layers - 1)) + [n * seq] + [n] * 4 + [n]
    )
