"""Native TransNetV2 trunk: everything that needs no GPU.

Weight packing (BatchNorm folding, weight order, branch-to-channel mapping,
pooling floor) evaluated with plain torch f32, the library's host-side
argument checks, the device-windowing index table against ``_get_batches``,
and the bf16 rounding emulation that the GPU tests use as their yardstick.
The kernels themselves are pinned in test_gpu_transnet_native.py.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch
from torch.nn import functional as F

import transnet_bf16_ref as ref
from cosmos_curate_amd import hotpath
from cosmos_curate_amd.models.transnetv2 import (
    TransNetV2,
    _TransNetV2,
    make_transnetv2_weights,
)
from cosmos_curate_amd.models.transnetv2_native import pack_trunk, window_indices
from cosmos_curate_amd.pipelines.video.clipping.transnetv2_extraction_stages import (
    TransNetV2ClipExtractionStage,
    _get_batches,
)

CC_ERR_INVALID, CC_ERR_UNSUPPORTED = -1, -6


@pytest.fixture(scope="module")
def net():
    n = _TransNetV2()
    n.load_state_dict(make_transnetv2_weights(), strict=True)
    return n.eval()


@pytest.fixture(scope="module")
def golden_input(golden_dir):
    return torch.from_numpy(np.load(golden_dir / "transnetv2_golden.npz")["input"])


@pytest.fixture(scope="module")
def f32_feats(net, golden_input):
    return ref.trunk_f32(net, golden_input)


# ---- 1. weight packing -------------------------------------------------------

def eval_packed_f32(stacks, frames_u8: torch.Tensor) -> list[torch.Tensor]:
    """The packed trunk in plain torch f32, channels-last, wired as the
    kernels are: one 3x3 conv for the four branches, branch b's temporal conv
    on channels [b*2F, (b+1)*2F) with dilation 2^b, relu(acc + bias), the
    shortcut added on the stack's last block, floor pooling."""
    b, t, h, w, _ = frames_u8.shape
    x = frames_u8.float() / 255.0
    feats = []
    for blocks in stacks:
        first = None
        for i, blk in enumerate(blocks):
            f = blk.filters
            s = F.conv2d(x.reshape(b * t, h, w, -1).permute(0, 3, 1, 2),
                         blk.spatial.permute(0, 3, 1, 2), padding=1)
            s = s.permute(0, 2, 3, 1).reshape(b, t, h, w, 8 * f)
            ys = []
            for br in range(4):
                xi = s[..., br * 2 * f:(br + 1) * 2 * f].permute(0, 4, 1, 2, 3)
                wt = blk.temporal[br].permute(0, 2, 1)[..., None, None]  # [F, 2F, 3, 1, 1]
                y = F.conv3d(xi, wt, bias=blk.bias[br * f:(br + 1) * f],
                             dilation=(2 ** br, 1, 1), padding=(2 ** br, 0, 0))
                ys.append(y.permute(0, 2, 3, 4, 1))
            y = F.relu(torch.cat(ys, dim=-1))
            if i == len(blocks) - 1:
                y = y + first
            if first is None:
                first = y
            x = y
        h2, w2 = h // 2, w // 2
        x = x[:, :, :2 * h2, :2 * w2].reshape(b, t, h2, 2, w2, 2, -1).mean(dim=(3, 5))
        h, w = h2, w2
        feats.append(x)
    return feats


def test_packed_trunk_reproduces_the_module(net, golden_input, f32_feats):
    stacks = pack_trunk(net.state_dict())
    assert [[(b.in_filters, b.filters) for b in s] for s in stacks] == [
        [(3, 16), (64, 16)], [(64, 32), (128, 32)], [(128, 64), (256, 64)]]
    got = eval_packed_f32(stacks, golden_input)
    assert [tuple(g.shape[2:]) for g in got] == [(13, 24, 64), (6, 12, 128), (3, 6, 256)]
    # rtol 1e-5 per element, with the floor an elementwise relative bound
    # needs: a feature is an f32 sum that cancels (relu clips about half of
    # them at zero), and folding BatchNorm reassociates that sum, so the
    # difference scales with the terms, not with where the sum lands.  The
    # floor is the same 1e-5 of the stack's rms (about 0.02, so 2e-7) —
    # a swapped branch or tap is wrong by the rms itself.
    for g, want in zip(got, f32_feats):
        np.testing.assert_allclose(g.permute(0, 4, 1, 2, 3).numpy(), want.numpy(),
                                   rtol=1e-5, atol=1e-5 * float(want.pow(2).mean().sqrt()))


def test_pack_rejects_a_state_dict_without_trunk():
    with pytest.raises(ValueError):
        pack_trunk({"fc1.weight": torch.zeros(1)})


# ---- 2. host validation, no device -------------------------------------------

P = 0x10000  # an aligned address nothing dereferences: every call below is rejected first


def _rejected(rc: int, code: int, word: str) -> None:
    assert rc == code
    assert word in hotpath.load().cc_last_error().decode()


@pytest.mark.parametrize(("cin", "cout"), [(3, 128), (32, 128), (96, 128), (512, 128),
                                            (64, 0), (64, 24), (64, 528)])
def test_conv3x3_rejects_unsupported_channels(cin, cout):
    lib = hotpath.load()
    _rejected(lib.cc_conv3x3_bf16(P, P, P, 3, 27, 48, cin, cout, 0),
              CC_ERR_UNSUPPORTED, "conv3x3")
    if cin == 64:
        _rejected(lib.cc_conv3x3_u8(P, P, P, 3, 27, 48, cout, 0),
                  CC_ERR_UNSUPPORTED, "conv3x3_u8")


def test_conv3x3_rejects_bad_pointers_and_sizes():
    lib = hotpath.load()
    for args in [(None, P, P, 3, 27, 48), (P, None, P, 3, 27, 48), (P, P, None, 3, 27, 48),
                 (P + 8, P, P, 3, 27, 48), (P, P + 2, P, 3, 27, 48), (P, P, P + 8, 3, 27, 48),
                 (P, P, P, 0, 27, 48), (P, P, P, 3, 0, 48), (P, P, P, 3, 27, -1)]:
        _rejected(lib.cc_conv3x3_bf16(*args, 64, 128, 0), CC_ERR_INVALID, "conv3x3")
    for args in [(None, P, P, 3, 27, 48), (P, P + 8, P, 3, 27, 48), (P, P, P + 4, 3, 27, 48),
                 (P, P, P, 0, 27, 48)]:
        _rejected(lib.cc_conv3x3_u8(*args, 128, 0), CC_ERR_INVALID, "conv3x3_u8")


def test_tconv3_rejects_bad_arguments():
    lib = hotpath.load()
    for f in (0, 8, 48, 128):
        _rejected(lib.cc_tconv3_bf16(P, P, P, None, P, 2, 20, 72, f, 0),
                  CC_ERR_UNSUPPORTED, "tconv3")
    for t in (0, -5):
        _rejected(lib.cc_tconv3_bf16(P, P, P, None, P, 2, t, 72, 16, 0),
                  CC_ERR_INVALID, "tconv3")
    for args in [(None, P, P, None, P), (P, None, P, None, P), (P, P, None, None, P),
                 (P, P, P, None, None), (P + 8, P, P, None, P), (P, P, P + 4, None, P),
                 (P, P, P, P + 8, P), (P, P, P, None, P + 2)]:
        _rejected(lib.cc_tconv3_bf16(*args, 2, 20, 72, 16, 0), CC_ERR_INVALID, "tconv3")
    _rejected(lib.cc_tconv3_bf16(P, P, P, None, P, 0, 20, 72, 16, 0),
              CC_ERR_INVALID, "tconv3")


def test_avgpool_rejects_bad_arguments():
    lib = hotpath.load()
    _rejected(lib.cc_avgpool2x2_bf16(P, P, 3, 6, 12, 12, 0), CC_ERR_UNSUPPORTED, "avgpool")
    for args in [(None, P, 3, 6, 12, 64), (P, P + 8, 3, 6, 12, 64), (P, P, 0, 6, 12, 64),
                 (P, P, 3, 1, 12, 64), (P, P, 3, 6, 1, 64), (P, P, 3, 6, 12, 0)]:
        _rejected(lib.cc_avgpool2x2_bf16(*args, 0), CC_ERR_INVALID, "avgpool")


# ---- 3. windowing ------------------------------------------------------------

@pytest.mark.parametrize("total", [1, 24, 25, 50, 51, 100, 149])
def test_window_indices_equal_get_batches(total):
    frames = np.arange(total, dtype=np.uint8).reshape(total, 1, 1, 1) * np.ones(
        (1, 2, 2, 3), dtype=np.uint8)
    want = list(_get_batches(frames))
    got = window_indices(total)
    assert len(got) == len(want)
    for idx, batch in zip(got, want):
        np.testing.assert_array_equal(frames[idx.numpy()], batch)


def test_backend_option_defaults_to_torch():
    assert TransNetV2().backend == "torch"
    assert TransNetV2ClipExtractionStage().backend == "torch"
    assert TransNetV2ClipExtractionStage(backend="native").model.backend == "native"
    with pytest.raises(ValueError):
        TransNetV2(backend="miopen")


# ---- 4. the yardstick itself -------------------------------------------------

def test_bf16_emulation_stays_close_to_f32(net, golden_input, f32_feats):
    """Conv weights, conv inputs and BatchNorm outputs in bf16 cost about
    1e-3 relative L2 per stack; an emulation that drifts past 2e-3 would be
    a lax yardstick for the native trunk."""
    for i, (emu, want) in enumerate(zip(ref.trunk_bf16(net, golden_input), f32_feats)):
        err = ref.rel_l2(emu, want)
        print(f"stack {i + 1}: emulation rel L2 {err:.3e}, rms {float(want.pow(2).mean().sqrt()):.3e}")
        assert 0 < err <= 2e-3
