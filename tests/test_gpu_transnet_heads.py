"""Native TransNetV2 heads on the MI355X: kernels, model, stage.

Every yardstick is the CPU restatement of tests/transnet_heads_ref.py in
f64 (the histogram: in f32, bit for bit), the module's own f32 heads, the
committed golden predictions, and the torch route of the stage.
"""

from __future__ import annotations

import pathlib

import numpy as np
import pytest
import torch

import transnet_heads_ref as ref
from cosmos_curate_amd import hotpath
from cosmos_curate_amd.core.interfaces import SequentialRunner, run_pipeline
from cosmos_curate_amd.models.transnetv2 import (
    TransNetV2,
    _TransNetV2,
    make_transnetv2_weights,
)
from cosmos_curate_amd.models.transnetv2_native import NativeHeads, NativeTrunk, pack_heads
from cosmos_curate_amd.pipelines.video.clipping import transnetv2_extraction_stages as tstages
from cosmos_curate_amd.pipelines.video.utils import raw_backend
from cosmos_curate_amd.pipelines.video.utils.data_model import (
    SplitPipeTask,
    Video,
    VideoMetadata,
)

pytestmark = pytest.mark.gpu


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _nan(*shape: int) -> torch.Tensor:
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def _assert_within(got: torch.Tensor, want: torch.Tensor, bound: torch.Tensor, what: str) -> None:
    got, want, bound = got.double().cpu(), want.double(), bound.double()
    diff = (got - want).abs()
    excess = diff - bound
    worst = int(excess.argmax())
    print(f"{what}: max |got-want| {float(diff.max()):.3e}, largest share of the bound "
          f"{float((diff / bound.clamp_min(1e-300)).max()):.3f}")
    assert torch.isfinite(got).all()
    assert float(excess.max()) <= 0, (
        f"{what}: element {worst} off by {float(diff.flatten()[worst]):.3e}, "
        f"allowed {float(bound.flatten()[worst]):.3e}")


# ---- cc_tn_hist512_u8 ----------------------------------------------------------

def _hist_gpu(frames: torch.Tensor) -> np.ndarray:
    n, pixels, _ = frames.shape
    out = _nan(n, 512)
    hotpath.tn_hist512_u8(frames.cuda().data_ptr(), out.data_ptr(), n, pixels, _stream())
    return out.cpu().numpy()


def test_hist512_random_frames():
    gen = torch.Generator().manual_seed(1)
    frames = torch.randint(0, 256, (5, 27 * 48, 3), generator=gen, dtype=torch.uint8)
    np.testing.assert_array_equal(_hist_gpu(frames), ref.hist512(frames))


def test_hist512_constant_frame():
    frames = torch.tensor([200, 17, 99], dtype=torch.uint8).expand(1, 27 * 48, 3).contiguous()
    got = _hist_gpu(frames)
    np.testing.assert_array_equal(got, ref.hist512(frames))
    assert got[0, (6 << 6) | (0 << 3) | 3] == 1.0 and np.count_nonzero(got) == 1


def test_hist512_4096_pixels():
    """The largest frame: one bin holding all 4096 pixels has c^2 = 2^24."""
    gen = torch.Generator().manual_seed(2)
    frames = torch.randint(0, 256, (2, 4096, 3), generator=gen, dtype=torch.uint8)
    frames[1] = 255
    got = _hist_gpu(frames)
    np.testing.assert_array_equal(got, ref.hist512(frames))
    assert got[1, 511] == 1.0


# ---- cc_tn_framesim_embed --------------------------------------------------------

def test_framesim_embed_real_shapes():
    gen = torch.Generator().manual_seed(3)
    shapes = [(312, 64), (72, 128), (18, 256)]
    # pooled stack outputs are relu(x) + shortcut: mostly positive, bf16 values
    maps = [ref.rb(torch.randn(3, hw, c, generator=gen).abs() * 0.5) for hw, c in shapes]
    wt = torch.randn(448, 128, generator=gen) * 0.05
    b = torch.randn(128, generator=gen) * 0.02
    e64 = ref.framesim_project([m.double() for m in maps], wt.double(), b.double())
    want = ref.framesim_embed([m.double() for m in maps], wt.double(), b.double())
    bound = ref.normalized_bound(e64, ref.framesim_project_bound(
        [m.double() for m in maps], wt.double(), b.double()))
    dev = [m.to("cuda", torch.bfloat16) for m in maps]
    wd, bd = wt.cuda(), b.cuda()
    out = _nan(3, 128)
    hotpath.tn_framesim_embed([(d.data_ptr(), hw, c) for d, (hw, c) in zip(dev, shapes)],
                              wd.data_ptr(), bd.data_ptr(), out.data_ptr(), 3, 128, _stream())
    _assert_within(out, want, bound, "framesim_embed")
    torch.testing.assert_close(out.cpu().norm(dim=1), torch.ones(3), rtol=1e-6, atol=0)


# ---- cc_tn_simband_fc --------------------------------------------------------------

def _simband_gpu(xd, wd, bd, b, t, d, ldo=256, col=0):
    out = _nan(b * t, ldo)
    hotpath.tn_simband_fc(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), out.data_ptr(),
                          b, t, d, ldo, col, _stream())
    return out


@pytest.mark.parametrize(("b", "t", "d"), [(2, 1, 128), (2, 51, 128), (2, 100, 512),
                                           (1, 130, 512)])
def test_simband_fc(b, t, d):
    """T = 1: every partner but the frame itself is outside; 51: the band's
    far end is reached by one frame only; 100: a full window; 130: frames
    whose whole band lies inside, and a T no multiple of the frame group."""
    gen = torch.Generator().manual_seed(t * 1000 + d)
    x = torch.randn(b, t, d, generator=gen)
    x = x / x.norm(dim=-1, keepdim=True)
    wt = torch.randn(101, 128, generator=gen) * 0.1
    bias = torch.randn(128, generator=gen) * 0.05
    want = ref.simband_fc(x.double(), wt.double(), bias.double()).reshape(b * t, 128)
    bound = ref.simband_fc_bound(x.double(), wt.double(), bias.double()).reshape(b * t, 128)
    xd, wd, bd = x.cuda(), wt.cuda(), bias.cuda()
    col = 128 if d == 128 else 0  # where the model puts this head
    out = _simband_gpu(xd, wd, bd, b, t, d, col=col)
    _assert_within(out[:, col:col + 128], want, bound, f"simband_fc B={b} T={t} D={d}")
    other = out[:, :128] if col else out[:, 128:]
    assert torch.isnan(other).all(), "columns outside [col, col+128) were written"
    assert float(want.max()) > 0

    # windows are independent: each window alone gives the same bits
    for i in range(b):
        single = _simband_gpu(xd[i:i + 1].contiguous(), wd, bd, 1, t, d, col=col)
        assert torch.equal(single[:, col:col + 128], out[i * t:(i + 1) * t, col:col + 128])


# ---- cc_tn_fc1_relu ------------------------------------------------------------------

def _fc1_gpu(hd, feat, hi, lo, bias, m, kh, kf, n):
    y = _nan(m, n)
    hotpath.tn_fc1_relu(hd.data_ptr(), feat.data_ptr(), hi.data_ptr(), lo.data_ptr(),
                        bias.data_ptr(), y.data_ptr(), m, kh, kf, n, _stream())
    return y


@pytest.mark.parametrize(("m", "kh", "kf", "n"), [(1, 256, 4608, 1024), (70, 64, 96, 48),
                                                  (130, 256, 4608, 1024)])
def test_fc1_relu(m, kh, kf, n):
    """M = 1: one live column in a tile; (70, 64, 96, 48): row and output
    tails, K below one unrolled block; M = 130: five row tiles, a tail of 2."""
    gen = torch.Generator().manual_seed(m * 7 + n)
    hd = torch.randn(m, kh, generator=gen).abs() * 0.3   # relu outputs
    feat = ref.rb(torch.randn(m, kf, generator=gen).abs() * 0.1)
    w = torch.randn(n, kh + kf, generator=gen) * 0.05
    bias = torch.randn(n, generator=gen) * 0.02
    w_hi, w_lo = ref.split(w)
    d = torch.float64
    pre_split = ref.fc1_split(hd.to(d), feat.to(d), w_hi.to(d), w_lo.to(d), bias.to(d))
    s = ref.fc1_abs_sum(hd.to(d), feat.to(d), w_hi.to(d), w_lo.to(d), bias.to(d))
    bound = ref.sum_bound(3 * kh + 2 * kf, s)
    pre_exact = torch.cat([hd, feat], dim=1).to(d) @ w.to(d).T + bias.to(d)

    hdd, fd = hd.cuda(), feat.to("cuda", torch.bfloat16)
    hid, lod = w_hi.to("cuda", torch.bfloat16), w_lo.to("cuda", torch.bfloat16)
    bd = bias.cuda()
    y = _fc1_gpu(hdd, fd, hid, lod, bd, m, kh, kf, n)
    what = f"fc1_relu M={m} KH={kh} KF={kf} N={n}"
    _assert_within(y, torch.relu(pre_split), bound, what + " vs split operands")
    _assert_within(y, torch.relu(pre_exact), bound + 2.0 ** -16 * s, what + " vs f32 operands")
    assert float((y > 0).float().mean()) > 0.2

    if m == 130:
        for row in (0, 31, 32, 127, 128, 129):
            one = _fc1_gpu(hdd[row:row + 1].contiguous(), fd[row:row + 1].contiguous(),
                           hid, lod, bd, 1, kh, kf, n)
            assert torch.equal(one[0], y[row]), f"row {row} alone differs from row {row} of 130"


# ---- cc_tn_cls_sigmoid ------------------------------------------------------------------

def test_cls_sigmoid():
    gen = torch.Generator().manual_seed(9)
    y = torch.randn(70, 1024, generator=gen).abs() * 0.5
    w = torch.randn(1024, generator=gen) * 0.05
    b = -0.3
    want = ref.cls_sigmoid(y.double(), w.double(), b)
    bound = ref.cls_sigmoid_bound(y.double(), w.double(), b, want)
    yd, wd = y.cuda(), w.cuda()
    p = _nan(70)
    hotpath.tn_cls_sigmoid(yd.data_ptr(), wd.data_ptr(), b, p.data_ptr(), 70, 1024, _stream())
    _assert_within(p, want, bound, "cls_sigmoid")
    assert 0.01 < float(want.min()) and float(want.max()) < 0.99 and float(want.std()) > 0.05


# ---- full model -----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def net():
    n = _TransNetV2()
    n.load_state_dict(make_transnetv2_weights(), strict=True)
    return n.eval()


@pytest.fixture(scope="module")
def golden(golden_dir):
    g = np.load(golden_dir / "transnetv2_golden.npz")
    return torch.from_numpy(g["input"]), g["output"]


@pytest.fixture(scope="module")
def model():
    m = TransNetV2(backend="native", heads="native")
    m.setup()
    return m


def test_model_matches_golden(model, golden):
    x, want = golden
    got = model(x.cuda())
    assert got.shape == (1, x.shape[1], 1) and got.dtype == torch.float32
    got = got[0, :, 0].cpu().numpy()
    print(f"native trunk + native heads vs golden: max |diff| {np.abs(got - want).max():.3e}")
    np.testing.assert_allclose(got, want, atol=5e-4)


@pytest.mark.parametrize("which", ["golden", "random B=2 T=30"])
def test_heads_match_the_module_on_native_features(net, golden, which):
    """The module's f32 heads, fed the native trunk's features, are the
    yardstick; the allowance is three times what the CPU restatement itself
    differs from them on this input (never under 1e-6)."""
    if which == "golden":
        frames = golden[0]
    else:
        gen = torch.Generator().manual_seed(11)
        frames = torch.randint(0, 256, (2, 30, 27, 48, 3), generator=gen, dtype=torch.uint8)
    sd = net.state_dict()
    feats = NativeTrunk(sd)(frames.cuda())
    got = NativeHeads(sd)(frames.cuda(), feats).cpu()
    cl = [f.float().cpu() for f in feats]
    want = net.heads(frames, [f.permute(0, 4, 1, 2, 3) for f in cl])
    err = float((ref.heads(pack_heads(sd), frames, cl) - want).abs().max())
    diff = float((got - want).abs().max())
    print(f"{which}: native heads vs module heads {diff:.3e}; restatement vs module {err:.3e}")
    assert got.shape == want.shape
    assert diff <= max(3 * err, 1e-6)


def test_model_batch_and_rerun_are_bit_identical(model):
    gen = torch.Generator().manual_seed(5)
    x = torch.randint(0, 256, (16, 100, 27, 48, 3), generator=gen, dtype=torch.uint8).cuda()
    batched = model(x)
    assert batched.shape == (16, 100, 1)
    assert torch.equal(model(x), batched)
    singles = torch.cat([model(x[i:i + 1]) for i in range(16)])
    assert torch.equal(singles, batched)
    assert float(batched.std()) > 0


def test_model_runs_a_tail_window(model):
    gen = torch.Generator().manual_seed(6)
    x = torch.randint(0, 256, (2, 37, 27, 48, 3), generator=gen, dtype=torch.uint8).cuda()
    torch_heads = TransNetV2(backend="native")
    torch_heads.setup()
    got, want = model(x), torch_heads(x)
    assert got.shape == want.shape == (2, 37, 1)
    assert torch.isfinite(got).all()
    print(f"T=37: native heads vs torch heads {float((got - want).abs().max()):.3e}")
    torch.testing.assert_close(got, want, rtol=0, atol=5e-6)


# ---- stage --------------------------------------------------------------------------------------

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


def test_stage_native_heads_give_the_same_clips(model):
    threshold = 0.4
    clips = {}
    routes = {"torch": {}, "native": {"backend": "native"},
              "native heads": {"backend": "native", "heads": "native"}}
    for name, kw in routes.items():
        out = run_pipeline([_video_task()], [tstages.VideoFrameExtractionStage()],
                           runner=SequentialRunner())
        frames = out[0].video.frame_array.resolve().copy()
        stage = tstages.TransNetV2ClipExtractionStage(
            threshold=threshold, min_length_s=0.5, min_length_frames=8, crop_s=None, **kw)
        out = run_pipeline(out, [stage], runner=SequentialRunner())
        assert not out[0].video.errors
        clips[name] = [(c.uuid, c.span) for c in out[0].video.clips]
    assert frames.shape == (FPS * SECONDS, 27, 48, 3)

    torch_model = TransNetV2()
    torch_model.setup()
    native_model = TransNetV2(backend="native")
    native_model.setup()
    flags_torch = tstages._get_predictions(torch_model, frames, threshold)
    flags_native = tstages._get_predictions_native(native_model, frames, threshold)
    flags_heads = tstages._get_predictions_native(model, frames, threshold)
    np.testing.assert_array_equal(flags_heads, flags_torch)
    np.testing.assert_array_equal(flags_heads, flags_native)
    assert clips["native heads"] == clips["torch"] == clips["native"]
    assert len(clips["torch"]) >= 1
