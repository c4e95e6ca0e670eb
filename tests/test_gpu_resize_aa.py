"""cc_resize_aa_u8 on the MI355X: bit-exact against tests/resize_aa_ref.py fed
the library's own tables, at the smallest shapes where the kernel changes
path (band and block edges, unaligned rows, crop along either axis, upscale,
identity, several chunks of source rows per band), plus the tower that takes
it under ``resize="antialias"`` and the default chain, which must not move.

Every resize below runs on guarded buffers: the input frames sit between
rows of 0xFF and the output between rows of 7, so a stray read changes the
result and a stray write shows in a guard, without a fault.  Every call runs
twice and must give the same bytes.  Every rejected call returns before any
launch; nothing here hands a kernel a bad pointer or size.
"""

from __future__ import annotations

import numpy as np
import pytest
import torch

import resize_aa_ref as ref
from cosmos_curate_amd import hotpath

pytestmark = pytest.mark.gpu

N = 3  # frames per call, so that a frame-stride error shows


@pytest.fixture(scope="module")
def lib():
    return hotpath.require_gpu()


def frames(n: int, h: int, w: int, seed: int) -> np.ndarray:
    """Frame 0 textured, the others uniform noise."""
    rng = np.random.default_rng(seed)
    out = rng.integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)
    out[0] = ref.textured_frame(h, w, seed)
    return out


def host_tables(tabs: hotpath.ResizeAATables):
    """The device tables read back, as resize_aa_ref's (first, count, w)."""
    ty = ref.split_table(tabs.table_y.cpu().numpy(), tabs.size, tabs.taps_y)
    tx = ref.split_table(tabs.table_x.cpu().numpy(), tabs.size, tabs.taps_x)
    return ty, tx


def run_guarded(lib, src: np.ndarray, tabs: hotpath.ResizeAATables) -> np.ndarray:
    """cc_resize_aa_u8 twice on guarded buffers -> the output as numpy, after
    checking the guards and that both launches agree."""
    n, h, w, _ = src.shape
    size = tabs.size
    ibuf = np.full((n * h + 2, w * 3), 0xFF, dtype=np.uint8)
    ibuf[1:-1] = src.reshape(n * h, w * 3)
    idev = torch.from_numpy(ibuf).cuda()
    row = size * 3
    outs = []
    for _ in range(2):
        obuf = torch.full((n * size + 2, row), 7, dtype=torch.uint8, device="cuda")
        hotpath.check(lib.cc_resize_aa_u8(
            idev.data_ptr() + w * 3, n, h, w, obuf.data_ptr() + row, size, size,
            tabs.table_y.data_ptr(), tabs.taps_y, tabs.table_x.data_ptr(),
            tabs.taps_x, 0))
        torch.cuda.synchronize()
        got = obuf.cpu().numpy()
        assert (got[0] == 7).all() and (got[-1] == 7).all(), "output guard row written"
        outs.append(got[1:-1].reshape(n, size, size, 3))
    np.testing.assert_array_equal(outs[0], outs[1], err_msg="two launches differ")
    np.testing.assert_array_equal(idev.cpu().numpy(), ibuf)  # inputs are read-only
    return outs[0]


def check_case(lib, h, w, size, filt, n=N, geometry=None, taps=None):
    tabs = hotpath.resize_aa_tables(filt, h, w, size)
    assert hotpath.resize_aa_tables(filt, h, w, size) is tabs  # uploaded once
    if geometry is not None:
        assert (tabs.resized_h, tabs.resized_w, tabs.top, tabs.left) == geometry
    if taps is not None:
        assert (tabs.taps_y, tabs.taps_x) == taps
    ty, tx = host_tables(tabs)
    fid = ref.FILTERS[filt]
    for got_t, want_t in ((ty, ref.table(fid, h, tabs.resized_h, tabs.top, size)),
                          (tx, ref.table(fid, w, tabs.resized_w, tabs.left, size))):
        for a, b in zip(got_t, want_t[:3]):
            np.testing.assert_array_equal(a, b)
    src = frames(n, h, w, seed=h * 1000 + w)
    got = run_guarded(lib, src, tabs)
    want = np.stack([ref.resize(f, ty, tx) for f in src])
    np.testing.assert_array_equal(got, want)
    return src, got


# (h, w, size, (rh, rw, top, left), (taps_y, taps_x))
CASES = {
    "band-edges-crop6": (70, 100, 32, (32, 45, 0, 6), (11, 11)),
    "odd-width-unaligned-rows": (37, 53, 16, (16, 22, 0, 3), (11, 11)),
    "portrait-crop-y": (100, 64, 32, (50, 32, 9, 0), (9, 9)),
    "upscale-taps5": (20, 30, 32, (32, 48, 0, 8), (5, 5)),
    "identity": (32, 32, 32, (32, 32, 0, 0), (5, 5)),
    "ragged-224": (240, 320, 224, (224, 298, 0, 37), (7, 7)),
    "43-taps-many-chunks": (330, 517, 32, (32, 50, 0, 9), (43, 43)),
}


@pytest.mark.parametrize("case", CASES.values(), ids=CASES.keys())
def test_bitexact_bicubic(lib, case):
    h, w, size, geometry, taps = case
    src, got = check_case(lib, h, w, size, "bicubic", geometry=geometry, taps=taps)
    if (h, w) == (size, size):
        np.testing.assert_array_equal(got, src)  # identity table: weight 1
    # the same through the public call
    out = hotpath.resize_aa_center_crop(torch.from_numpy(src).cuda(), size, "bicubic")
    assert out.shape == (N, size, size, 3) and out.dtype == torch.uint8
    np.testing.assert_array_equal(out.cpu().numpy(), got)


@pytest.mark.parametrize("shape", [(70, 100, 32), (37, 53, 16)])
def test_bitexact_bilinear(lib, shape):
    h, w, size = shape
    _, got = check_case(lib, h, w, size, "bilinear")
    _, cubic = check_case(lib, h, w, size, "bicubic")
    assert not np.array_equal(got, cubic)  # the filter is a matter of the table


def test_bitexact_1080p_pair(lib):
    """Two 1080x1920 frames -> 224: 21 taps, crop offset 87, two chunks of
    source rows per band."""
    src, got = check_case(lib, 1080, 1920, 224, "bicubic", n=2,
                          geometry=(224, 398, 0, 87), taps=(21, 21))
    # the restatement's own tables give the same bytes as the library's
    want = ref.resize_center_crop(src[0], 224)
    np.testing.assert_array_equal(got[0], want)


def test_timing_name(lib):
    tabs = hotpath.resize_aa_tables("bicubic", 37, 53, 16)
    src = frames(N, 37, 53, seed=5)
    hotpath.timing_enable(True)
    try:
        run_guarded(lib, src, tabs)
        assert hotpath.timing_report("resize_aa_u8")[1] == 2
        assert hotpath.timing_report("resize_bicubic_u8")[1] == 0
    finally:
        hotpath.timing_enable(False)


def test_rejections_leave_the_output_untouched(lib):
    h, w, size = 37, 53, 16
    tabs = hotpath.resize_aa_tables("bicubic", h, w, size)
    src = torch.zeros((1, h, w, 3), dtype=torch.uint8, device="cuda")
    out = torch.full((1, size, size, 3), 0x5A, dtype=torch.uint8, device="cuda")
    good = dict(src=src.data_ptr(), n=1, h=h, w=w, out=out.data_ptr(), oh=size, ow=size,
                ty=tabs.table_y.data_ptr(), tapsy=tabs.taps_y,
                tx=tabs.table_x.data_ptr(), tapsx=tabs.taps_x)

    def call(a):
        return lib.cc_resize_aa_u8(a["src"], a["n"], a["h"], a["w"], a["out"], a["oh"],
                                   a["ow"], a["ty"], a["tapsy"], a["tx"], a["tapsx"], 0)

    invalid = {
        "null in": dict(src=None), "null out": dict(out=None),
        "null table y": dict(ty=None), "null table x": dict(tx=None),
        "table y misaligned": dict(ty=tabs.table_y.data_ptr() + 2),
        "n 0": dict(n=0), "h 0": dict(h=0), "w -1": dict(w=-1),
        "out_h 0": dict(oh=0), "out_w 0": dict(ow=0),
        "taps_y 0": dict(tapsy=0), "taps_x -3": dict(tapsx=-3),
    }
    for name, change in invalid.items():
        assert call(dict(good, **change)) == -1, name  # CC_ERR_INVALID
        assert lib.cc_last_error().decode(), name
    unsupported = {
        "taps_y above the bound": dict(tapsy=hotpath.RESIZE_AA_MAX_TAPS + 2),
        "taps_x above the bound": dict(tapsx=hotpath.RESIZE_AA_MAX_TAPS + 2),
    }
    for name, change in unsupported.items():
        assert call(dict(good, **change)) == -6, name  # CC_ERR_UNSUPPORTED
        assert lib.cc_last_error().decode(), name
    with pytest.raises(ValueError):
        hotpath.resize_aa_tables("bicubic", 8000, 8000, 32)  # 501 taps
    with pytest.raises(ValueError):
        hotpath.resize_aa_center_crop(src.float(), size)
    torch.cuda.synchronize()
    assert bool((out == 0x5A).all())
    assert call(good) == 0  # the unchanged arguments are accepted
    torch.cuda.synchronize()
    assert not bool((out == 0x5A).all())


# ---- the tower -------------------------------------------------------------------

@pytest.fixture(scope="module")
def tower_frames():
    return frames(2, 240, 320, seed=11)


def test_tower_antialias_matches_oracle(lib, tower_frames):
    from cosmos_curate_amd.models.clip import CLIPImageEmbeddings
    from cosmos_curate_amd.models.clip_weights import make_clip_vit_b32_weights
    from oracle import vit as oracle_vit
    from oracle.color import clip_preprocess

    model = CLIPImageEmbeddings(resize="antialias")
    model.setup()
    emb = model(tower_frames)
    assert emb.shape == (2, 512)
    norms = torch.linalg.vector_norm(emb, dim=-1).cpu()
    torch.testing.assert_close(norms, torch.ones(2), rtol=1e-3, atol=1e-3)
    crop = np.stack([ref.resize_center_crop(f, 224) for f in tower_frames])
    oracle = oracle_vit.build_reference_clip_vision(make_clip_vit_b32_weights())
    want = oracle_vit.embed_frames_fp32(oracle, clip_preprocess(crop))
    cos = np.sum(want * emb.cpu().numpy(), axis=1)
    print("cosine", cos.tolist())
    assert np.all(cos >= 0.999), cos


def test_default_chain_keeps_todays_bytes(lib, tower_frames):
    """resize="cubic" (and no keyword) still is cc_resize_bicubic_u8 + crop
    with the present size arithmetic, and not the antialiased chain."""
    from cosmos_curate_amd.models.clip import CLIPImageEmbeddings, _CLIPImageEmbeddings

    dev = torch.from_numpy(tower_frames).cuda()
    n, h, w, _ = dev.shape
    size = 224
    scale = size / min(h, w)
    rh, rw = max(size, round(h * scale)), max(size, round(w * scale))
    full = torch.empty((n, rh, rw, 3), dtype=torch.uint8, device="cuda")
    hotpath.check(lib.cc_resize_bicubic_u8(dev.data_ptr(), n, h, w, full.data_ptr(),
                                           rh, rw, 0))
    top, left = (rh - size) // 2, (rw - size) // 2
    today = full[:, top:top + size, left:left + size, :].contiguous()

    default = CLIPImageEmbeddings()
    cubic = CLIPImageEmbeddings(resize="cubic")
    default.setup()
    cubic.setup()
    for m in (default, cubic):
        assert m._model._resize == "cubic"
        assert torch.equal(m._model._resize_center_crop_u8(dev), today)
    seen = []
    orig = _CLIPImageEmbeddings.preprocess_patches_u8

    def spy(self, frames_u8):
        seen.append(frames_u8.clone())
        return orig(self, frames_u8)

    _CLIPImageEmbeddings.preprocess_patches_u8 = spy
    try:
        e_default = default(dev)
        e_cubic = cubic(dev)
        aa = CLIPImageEmbeddings(resize="antialias")
        aa.setup()
        aa(dev)
    finally:
        _CLIPImageEmbeddings.preprocess_patches_u8 = orig
    assert torch.equal(seen[0], today) and torch.equal(seen[1], today)
    assert torch.equal(e_default, e_cubic)
    want_aa = np.stack([ref.resize_center_crop(f, 224) for f in tower_frames])
    np.testing.assert_array_equal(seen[2].cpu().numpy(), want_aa)
    assert not torch.equal(seen[2], today)
    with pytest.raises(ValueError):
        CLIPImageEmbeddings(resize="lanczos")
