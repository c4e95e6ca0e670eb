"""Native TransNetV2 trunk on the MI355X: kernels, trunk, model, stage.

Every yardstick is torch f32 on the CPU (tests/transnet_bf16_ref.py):
single kernels against the f32 conv of the same bf16 operands, the trunk
against three times the error of a bf16 emulation of the module, the model
against the committed golden predictions, the stage against the torch route.
"""

from __future__ import annotations

import pathlib

import numpy as np
import pytest
import torch
from torch.nn import functional as F

import transnet_bf16_ref as ref
from cosmos_curate_amd import hotpath
from cosmos_curate_amd.core.interfaces import SequentialRunner, run_pipeline
from cosmos_curate_amd.models.transnetv2 import (
    TransNetV2,
    _TransNetV2,
    make_transnetv2_weights,
)
from cosmos_curate_amd.models.transnetv2_native import NativeTrunk
from cosmos_curate_amd.pipelines.video.clipping import transnetv2_extraction_stages as tstages
from cosmos_curate_amd.pipelines.video.utils import raw_backend
from cosmos_curate_amd.pipelines.video.utils.data_model import (
    SplitPipeTask,
    Video,
    VideoMetadata,
)

pytestmark = pytest.mark.gpu

STACK_HW = {16: (27, 48), 32: (13, 24), 64: (6, 12)}


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _bf16_randn(gen: torch.Generator, *shape: int, scale: float = 1.0) -> torch.Tensor:
    """f32 values that bf16 holds exactly."""
    return ref.rb(torch.randn(shape, generator=gen) * scale)


def _dev(x: torch.Tensor) -> torch.Tensor:
    return x.to("cuda", torch.bfloat16)


def _assert_within(got: torch.Tensor, want: torch.Tensor, bound: torch.Tensor, what: str) -> None:
    got = got.float().cpu()
    want = ref.rb(want)
    excess = (got - want).abs() - bound
    worst = int(excess.argmax())
    print(f"{what}: max |got-want| {float((got - want).abs().max()):.3e}, "
          f"largest share of the bound {float(((got - want).abs() / bound.clamp_min(1e-30)).max()):.3f}")
    assert torch.isfinite(got).all()
    assert float(excess.max()) <= 0, (
        f"{what}: element {worst} off by {float((got - want).abs().flatten()[worst]):.3e}, "
        f"allowed {float(bound.flatten()[worst]):.3e}")


def _conv2d_cl(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """[N,H,W,Cin] x [Cout,3,3,Cin] -> [N,H,W,Cout], f32, zero padding 1."""
    return F.conv2d(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), padding=1).permute(0, 2, 3, 1)


# ---- cc_conv3x3_bf16 / cc_conv3x3_u8 -----------------------------------------

@pytest.mark.parametrize(("cin", "cout", "h", "w"), [
    (64, 128, 27, 48), (64, 256, 13, 24), (128, 256, 13, 24),
    (128, 512, 6, 12), (256, 512, 6, 12)])
def test_conv3x3_bf16(cin, cout, h, w):
    gen = torch.Generator().manual_seed(cin * 1000 + cout)
    x = _bf16_randn(gen, 3, h, w, cin)
    wt = _bf16_randn(gen, cout, 3, 3, cin, scale=0.05)
    want = _conv2d_cl(x, wt)
    bound = ref.conv_bound(ref.rb(want), _conv2d_cl(x.abs(), wt.abs()), 9 * cin)
    xd, wd = _dev(x), _dev(wt)
    y = torch.full((3, h, w, cout), float("nan"), dtype=torch.bfloat16, device="cuda")
    hotpath.conv3x3_bf16(xd.data_ptr(), wd.data_ptr(), y.data_ptr(), 3, h, w, cin, cout, _stream())
    _assert_within(y, want, bound, f"conv3x3 {cin}->{cout} {h}x{w}")


def test_conv3x3_u8_first_layer():
    gen = torch.Generator().manual_seed(3)
    xu = torch.randint(0, 256, (3, 27, 48, 3), generator=gen, dtype=torch.uint8)
    wt = _bf16_randn(gen, 128, 3, 3, 3, scale=0.05)
    x = ref.rb(xu.float() / 255.0)
    want = _conv2d_cl(x, wt)
    bound = ref.conv_bound(ref.rb(want), _conv2d_cl(x, wt.abs()), 27)
    xd, wd = xu.cuda(), _dev(wt)
    y = torch.full((3, 27, 48, 128), float("nan"), dtype=torch.bfloat16, device="cuda")
    hotpath.conv3x3_u8(xd.data_ptr(), wd.data_ptr(), y.data_ptr(), 3, 27, 48, 128, _stream())
    _assert_within(y, want, bound, "conv3x3_u8 3->128 27x48")


# ---- cc_tconv3_bf16 ----------------------------------------------------------

def _tconv_ref(x, wt, bias, shortcut, f):
    """(want, S): x [B,T,HW,8F], wt [4,F,3,2F] -> [B,T,HW,4F] f32; S is the
    same sum over magnitudes (taps, bias and shortcut)."""
    def run(x, wt, bias, shortcut, relu):
        ys = []
        for br in range(4):
            xi = x[..., br * 2 * f:(br + 1) * 2 * f].permute(0, 3, 1, 2)[..., None]  # [B,2F,T,HW,1]
            w5 = wt[br].permute(0, 2, 1)[..., None, None]
            y = F.conv3d(xi, w5, bias=bias[br * f:(br + 1) * f],
                         dilation=(2 ** br, 1, 1), padding=(2 ** br, 0, 0))
            ys.append(y[..., 0].permute(0, 2, 3, 1))
        y = torch.cat(ys, dim=-1)
        if relu:
            y = F.relu(y)
        return y if shortcut is None else y + shortcut
    return (run(x, wt, bias, shortcut, True),
            run(x.abs(), wt.abs(), bias.abs(), None if shortcut is None else shortcut.abs(), False))


def _tconv_gpu(xd, wd, bd, sd, b, t, hw, f):
    y = torch.full((b, t, hw, 4 * f), float("nan"), dtype=torch.bfloat16, device="cuda")
    hotpath.tconv3_bf16(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(),
                        sd.data_ptr() if sd is not None else 0, y.data_ptr(),
                        b, t, hw, f, _stream())
    return y


@pytest.mark.parametrize("f", [16, 32, 64])
@pytest.mark.parametrize(("t", "with_shortcut"), [(20, False), (20, True), (5, True)])
def test_tconv3_bf16(f, t, with_shortcut):
    """T = 20 > 2*8: the dilation-8 taps meet both pads and a valid
    interior; T = 5: the outer taps of dilations 4 and 8 are all padding."""
    b, hw = 2, STACK_HW[f][0] * STACK_HW[f][1]
    gen = torch.Generator().manual_seed(f * 100 + t + int(with_shortcut))
    x = _bf16_randn(gen, b, t, hw, 8 * f)
    wt = _bf16_randn(gen, 4, f, 3, 2 * f, scale=0.05)
    bias = torch.randn(4 * f, generator=gen) * 0.5
    sc = _bf16_randn(gen, b, t, hw, 4 * f) if with_shortcut else None
    want, s = _tconv_ref(x, wt, bias, sc, f)
    bound = ref.conv_bound(ref.rb(want), s, 3 * 2 * f + 2)
    xd, wd, bd = _dev(x), _dev(wt), bias.cuda()
    sd = _dev(sc) if with_shortcut else None
    y = _tconv_gpu(xd, wd, bd, sd, b, t, hw, f)
    _assert_within(y, want, bound, f"tconv3 F={f} T={t} shortcut={with_shortcut}")

    # windows are independent: other content in window 1 leaves window 0 alone
    xd2 = xd.clone()
    xd2[1] = _dev(_bf16_randn(gen, t, hw, 8 * f))
    y2 = _tconv_gpu(xd2, wd, bd, sd, b, t, hw, f)
    assert torch.equal(y2[0], y[0])
    assert not torch.equal(y2[1], y[1])


# ---- cc_avgpool2x2_bf16 ------------------------------------------------------

@pytest.mark.parametrize(("h", "w", "c"), [(27, 48, 64), (13, 24, 128), (6, 12, 256)])
def test_avgpool2x2_bf16(h, w, c):
    gen = torch.Generator().manual_seed(h)
    x = _bf16_randn(gen, 3, h, w, c)
    want = F.avg_pool2d(x.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
    assert want.shape == (3, h // 2, w // 2, c)
    xd = _dev(x)
    y = torch.full(want.shape, float("nan"), dtype=torch.bfloat16, device="cuda")
    hotpath.avgpool2x2_bf16(xd.data_ptr(), y.data_ptr(), 3, h, w, c, _stream())
    _assert_within(y, want, 2.0 ** -7 * ref.rb(want).abs(), f"avgpool {h}x{w}x{c}")


# ---- trunk features ----------------------------------------------------------

@pytest.fixture(scope="module")
def net():
    n = _TransNetV2()
    n.load_state_dict(make_transnetv2_weights(), strict=True)
    return n.eval()


@pytest.fixture(scope="module")
def trunk(net):
    return NativeTrunk(net.state_dict())


@pytest.fixture(scope="module")
def golden(golden_dir):
    g = np.load(golden_dir / "transnetv2_golden.npz")
    return torch.from_numpy(g["input"]), g["output"]


def _check_trunk(net, trunk, frames_u8: torch.Tensor, what: str) -> None:
    want = ref.trunk_f32(net, frames_u8)
    emu = ref.trunk_bf16(net, frames_u8)
    got = [f.float().cpu().permute(0, 4, 1, 2, 3) for f in trunk(frames_u8.cuda())]
    for i, (g, e, w) in enumerate(zip(got, emu, want)):
        assert g.shape == w.shape
        err, yard = ref.rel_l2(g, w), ref.rel_l2(e, w)
        cos = F.cosine_similarity(g.transpose(1, 2).flatten(2), w.transpose(1, 2).flatten(2), dim=2)
        print(f"{what} stack {i + 1}: native rel L2 {err:.3e}, emulation {yard:.3e}, "
              f"min per-frame cosine {float(cos.min()):.7f}")
        assert err <= 3 * yard


def test_trunk_features_golden_input(net, trunk, golden):
    _check_trunk(net, trunk, golden[0], "golden")


def test_trunk_features_random_batch(net, trunk):
    gen = torch.Generator().manual_seed(11)
    frames = torch.randint(0, 256, (2, 30, 27, 48, 3), generator=gen, dtype=torch.uint8)
    _check_trunk(net, trunk, frames, "random B=2 T=30")


# ---- full model --------------------------------------------------------------

@pytest.fixture(scope="module")
def native_model():
    m = TransNetV2(backend="native")
    m.setup()
    return m


def test_native_model_matches_golden(native_model, golden):
    x, want = golden
    got = native_model(x.cuda())[0, :, 0].cpu().numpy()
    print(f"native vs golden: max |diff| {np.abs(got - want).max():.3e}")
    np.testing.assert_allclose(got, want, atol=5e-4)


def test_native_model_batch_and_rerun_are_bit_identical(native_model):
    gen = torch.Generator().manual_seed(5)
    x = torch.randint(0, 256, (16, 100, 27, 48, 3), generator=gen, dtype=torch.uint8).cuda()
    batched = native_model(x)
    assert batched.shape == (16, 100, 1)
    assert torch.equal(native_model(x), batched)
    singles = torch.cat([native_model(x[i:i + 1]) for i in range(16)])
    assert torch.equal(singles, batched)


# ---- stage -------------------------------------------------------------------

FPS, SECONDS, H, W = 30, 5, 128, 192


def _video_task() -> SplitPipeTask:
    raw = raw_backend.make_synthetic_clip(FPS * SECONDS, H, W, FPS, seed=42)
    v = Video(
        input_video=pathlib.Path("/synthetic/tnv2.mp4"),
        metadata=VideoMetadata(size=1, height=H, width=W, framerate=float(FPS),
                               num_frames=FPS * SECONDS, duration=float(SECONDS),
                               video_codec="raw"),
        encoded_data=np.frombuffer(raw, dtype=np.uint8),
    )
    return SplitPipeTask(videos=[v])


def test_stage_native_gives_the_same_clips_as_torch(native_model):
    threshold = 0.4
    clips = {}
    for backend in ("torch", "native"):
        out = run_pipeline([_video_task()], [tstages.VideoFrameExtractionStage()],
                           runner=SequentialRunner())
        frames = out[0].video.frame_array.resolve().copy()
        stage = tstages.TransNetV2ClipExtractionStage(
            threshold=threshold, min_length_s=0.5, min_length_frames=8, crop_s=None,
            backend=backend)
        out = run_pipeline(out, [stage], runner=SequentialRunner())
        assert not out[0].video.errors
        clips[backend] = [(c.uuid, c.span) for c in out[0].video.clips]
    assert frames.shape == (FPS * SECONDS, 27, 48, 3)

    # the comparison means something only if no f32 prediction sits on the
    # threshold, where a bf16 trunk may legitimately fall on the other side
    torch_model = TransNetV2()
    torch_model.setup()
    probs = torch.cat([
        torch_model(torch.from_numpy(np.ascontiguousarray(b)).cuda().unsqueeze(0))[0, 25:75]
        for b in tstages._get_batches(frames)])[: len(frames), 0].cpu().numpy()
    gap = float(np.abs(probs - threshold).min())
    print(f"closest torch f32 prediction to the threshold: {gap:.4f}")
    assert gap > 1e-3, (
        f"a torch f32 prediction lies {gap:.2e} from the threshold {threshold}: "
        "choose another seed for the synthetic video")

    flags_torch = tstages._get_predictions(torch_model, frames, threshold)
    flags_native = tstages._get_predictions_native(native_model, frames, threshold)
    np.testing.assert_array_equal(flags_native, flags_torch)
    assert clips["native"] == clips["torch"]
    assert len(clips["torch"]) >= 1
