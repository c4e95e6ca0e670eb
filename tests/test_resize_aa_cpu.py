"""The antialiased resize + center crop without a GPU: the written definition
(tests/resize_aa_ref.py) against the arithmetic it restates (torch CPU
F.interpolate(antialias=True), clamp, round), cc_resize_aa_table_build
against the definition's tables, the size and crop arithmetic against
hand-worked cases, and the keyword's way through the models, stages and CLI.
"""

from __future__ import annotations

import argparse
import ctypes
import inspect

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resize_aa_ref as ref
from cosmos_curate_amd import hotpath

# (h, w) -> (oh, ow)
SHAPES = [
    ((240, 320), (224, 298)),
    ((70, 100), (32, 45)),
    ((37, 53), (16, 22)),
    ((20, 30), (32, 48)),  # upscale
    ((100, 64), (50, 32)),
    ((65, 129), (7, 14)),
    ((224, 224), (224, 224)),
    ((1080, 1920), (224, 398)),
]
MODES = {ref.BICUBIC: "bicubic", ref.BILINEAR: "bilinear"}


def torch_reference(src: np.ndarray, oh: int, ow: int, filt: int) -> np.ndarray:
    x = torch.from_numpy(src).permute(2, 0, 1)[None].float()
    y = F.interpolate(x, size=(oh, ow), mode=MODES[filt], antialias=True,
                      align_corners=False)
    return y.clamp(0, 255).round()[0].permute(1, 2, 0).numpy().astype(np.uint8)


@pytest.fixture(scope="module")
def lib():
    return hotpath.load()


# ---- 1. the restatement against torch's arithmetic ------------------------------

@pytest.mark.parametrize("filt", [ref.BICUBIC, ref.BILINEAR], ids=["bicubic", "bilinear"])
@pytest.mark.parametrize(("src_hw", "out_hw"), SHAPES,
                         ids=[f"{h}x{w}" for (h, w), _ in SHAPES])
def test_restatement_matches_torch(src_hw, out_hw, filt):
    """The two differ only in f32 weight rounding and summation order: no
    value off by more than 1 code, at most 2e-3 of the values off at all."""
    (h, w), (oh, ow) = src_hw, out_hw
    rng = np.random.default_rng(20260 + h)
    contents = {"noise": rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8),
                "textured": ref.textured_frame(h, w, seed=h + w)}
    for name, src in contents.items():
        got = ref.resize_full(src, oh, ow, filt)
        want = torch_reference(src, oh, ow, filt)
        diff = np.abs(got.astype(np.int16) - want.astype(np.int16))
        share = float((diff > 0).mean())
        print(f"{h}x{w} {MODES[filt]} {name}: max {int(diff.max())} share {share:.2e}")
        if (h, w) == (oh, ow):
            np.testing.assert_array_equal(got, src)  # identity is exact
            np.testing.assert_array_equal(want, src)
        assert int(diff.max()) <= 1, name
        assert share <= 2e-3, (name, share)


def test_antialias_matters_on_a_downscale():
    """What the keyword is for: on a real downscale (the 1080p -> 224 ratio)
    the four-tap, no-antialias result is far from the antialiased one."""
    src = ref.textured_frame(270, 480, seed=3)
    x = torch.from_numpy(src).permute(2, 0, 1)[None].float()
    plain = F.interpolate(x, size=(56, 99), mode="bicubic", antialias=False,
                          align_corners=False).clamp(0, 255).round()
    plain = plain[0].permute(1, 2, 0).numpy()
    aa = ref.resize_full(src, 56, 99).astype(np.float32)
    assert float(np.abs(aa - plain).mean()) > 8.0


def test_crop_only_computes_the_crop():
    """resize_center_crop == the crop of the full resize, bit for bit."""
    for (h, w), size in (((70, 100), 32), ((100, 64), 32), ((37, 53), 16)):
        src = ref.textured_frame(h, w, seed=h)
        rh, rw, top, left = ref.geometry(h, w, size)
        full = ref.resize_full(src, rh, rw)
        np.testing.assert_array_equal(ref.resize_center_crop(src, size),
                                      full[top:top + size, left:left + size])


# ---- 2. cc_resize_aa_table_build ----------------------------------------------------

AXES = sorted({(i, o) for (h, w), (oh, ow) in SHAPES for i, o in ((h, oh), (w, ow))})


@pytest.mark.parametrize("filt", [ref.BICUBIC, ref.BILINEAR], ids=["bicubic", "bilinear"])
def test_table_build_equals_the_restatement(lib, filt):
    for in_size, out_size in AXES:
        first, count, w, taps = ref.table(filt, in_size, out_size)
        got_taps = ctypes.c_int()
        nbytes = lib.cc_resize_aa_table_build(filt, in_size, out_size, 0, out_size,
                                              None, 0, ctypes.byref(got_taps))
        assert got_taps.value == taps
        assert nbytes == out_size * (2 + taps) * 4  # the size query
        img, taps2 = hotpath.resize_aa_table_build(filt, in_size, out_size)
        assert taps2 == taps and img.nbytes == nbytes
        f2, c2, w2 = ref.split_table(img, out_size, taps)
        np.testing.assert_array_equal(f2, first)
        np.testing.assert_array_equal(c2, count)
        np.testing.assert_array_equal(w2, w)
        assert (c2 >= 1).all() and (c2 <= taps).all() and (f2 >= 0).all()
        assert int((f2 + c2).max()) <= in_size
        sums = w2.astype(np.float64).sum(axis=1)
        # each of <= taps weights is rounded to f32 once (relative 2^-24 of a
        # value below ~1.2): the sum stays within 2^-22 of 1
        assert float(np.abs(sums - 1.0).max()) <= 2.0 ** -22
        for j in range(out_size):
            assert not w2[j, c2[j]:].any()  # padding weights are zero
        # a crop is the same rows of the same table
        if out_size > 5:
            off, length = out_size // 3, out_size - out_size // 3 - 1
            part, ptaps = hotpath.resize_aa_table_build(filt, in_size, out_size, off, length)
            pf, pc, pw = ref.split_table(part, length, ptaps)
            np.testing.assert_array_equal(pf, first[off:off + length])
            np.testing.assert_array_equal(pc, count[off:off + length])
            np.testing.assert_array_equal(pw, w[off:off + length])


def test_table_build_upscale_is_the_plain_filter():
    """scale < 1: the four-tap (two-tap) filter with edge truncation."""
    first, count, w, taps = ref.table(ref.BICUBIC, 20, 32)
    assert taps == 5 and int(count.max()) <= 5 and int(count.min()) >= 2
    first, count, w, taps = ref.table(ref.BILINEAR, 20, 32)
    assert taps == 3 and int(count.max()) <= 3
    first, count, w, taps = ref.table(ref.BICUBIC, 224, 224)
    assert (w.max(axis=1) == 1.0).all() and (np.abs(w).sum(axis=1) == 1.0).all()
    np.testing.assert_array_equal(first + np.argmax(w, axis=1), np.arange(224))


def test_table_build_rejections(lib):
    taps = ctypes.c_int(-7)
    buf = np.zeros(4096, dtype=np.uint8)
    ptr = buf.ctypes.data_as(ctypes.c_void_p)

    def build(filt=1, i=100, o=45, off=6, length=32, out=ptr, nbytes=buf.nbytes):
        return lib.cc_resize_aa_table_build(filt, i, o, off, length, out, nbytes,
                                            ctypes.byref(taps))

    need = 32 * (2 + 11) * 4
    assert build() == need and taps.value == 11
    assert build(out=None, nbytes=0) == need
    bad = {
        "unknown filter": dict(filt=2), "negative filter": dict(filt=-1),
        "in_size 0": dict(i=0), "out_size 0": dict(o=0), "out_size -4": dict(o=-4),
        "crop_off -1": dict(off=-1), "crop_len 0": dict(length=0),
        "crop past the output": dict(off=14, length=32),
        "crop_off past the output": dict(off=46, length=1),
        "buffer too small": dict(nbytes=need - 1),
    }
    for name, change in bad.items():
        assert build(**change) == -1, name  # CC_ERR_INVALID
        assert lib.cc_last_error().decode(), name
    with pytest.raises(RuntimeError):
        hotpath.resize_aa_table_build("bicubic", 100, 45, 14, 32)
    with pytest.raises(ValueError):
        hotpath.resize_aa_table_build("lanczos", 100, 45)


# ---- 3. size and crop arithmetic ------------------------------------------------------

def test_geometry_follows_torchvision():
    cases = {
        # (h, w, size): (rh, rw, top, left)
        (70, 100, 32): (32, 45, 0, 6),        # 45 - 32 = 13 -> 6.5 -> 6 (half to even)
        (100, 70, 32): (45, 32, 6, 0),        # portrait, the same half
        (37, 53, 16): (16, 22, 0, 3),         # 16*53/37 = 22.9 truncates to 22
        (100, 64, 32): (50, 32, 9, 0),        # portrait, crop along y
        (240, 320, 224): (224, 298, 0, 37),   # 298.67 truncates (round gives 299)
        (1080, 1920, 224): (224, 398, 0, 87),
        (20, 30, 32): (32, 48, 0, 8),         # upscale
        (224, 224, 224): (224, 224, 0, 0),
        (50, 53, 50): (50, 53, 0, 2),         # 3 -> 1.5 -> 2 (half to even, up)
        (50, 55, 50): (50, 55, 0, 2),         # 5 -> 2.5 -> 2 (half to even, down)
    }
    for (h, w, size), want in cases.items():
        assert ref.geometry(h, w, size) == want, (h, w, size)
        assert hotpath.resize_aa_geometry(h, w, size) == want, (h, w, size)
    with pytest.raises(ValueError):
        hotpath.resize_aa_geometry(0, 10, 4)


# ---- 4. the keyword through models, stages and CLI ---------------------------------------

def test_keyword_defaults_and_checks():
    from cosmos_curate_amd.models.clip import CLIPImageEmbeddings, _CLIPImageEmbeddings
    from cosmos_curate_amd.models.clip_aesthetics import CLIPAestheticScorer
    from cosmos_curate_amd.pipelines.video.embedding.clip_stages import ClipEmbeddingStage
    from cosmos_curate_amd.pipelines.video.filtering.aesthetics.aesthetic_filter_stages import (
        AestheticFilterStage,
    )

    for cls in (CLIPImageEmbeddings, _CLIPImageEmbeddings, CLIPAestheticScorer,
                ClipEmbeddingStage, AestheticFilterStage):
        assert inspect.signature(cls.__init__).parameters["resize"].default == "cubic", cls
    assert inspect.signature(hotpath.resize_aa_center_crop).parameters[
        "filter"].default == "bicubic"
    assert CLIPImageEmbeddings()._resize == "cubic"
    assert CLIPImageEmbeddings("siglip_l16_256", resize="antialias")._resize == "antialias"
    assert CLIPAestheticScorer(resize="antialias")._resize == "antialias"
    stage = ClipEmbeddingStage(variant="vit_l14", resize="antialias")
    assert stage.model._resize == "antialias" and stage._resize == "antialias"
    assert ClipEmbeddingStage().model._resize == "cubic"
    stage = AestheticFilterStage(resize="antialias")
    assert stage.model._resize == "antialias"
    assert AestheticFilterStage().model._resize == "cubic"
    for make in (CLIPImageEmbeddings, CLIPAestheticScorer, ClipEmbeddingStage,
                 AestheticFilterStage):
        with pytest.raises(ValueError):
            make(resize="lanczos")


def _split_args(tmp_path, *extra):
    from cosmos_curate_amd.pipelines.video.splitting_pipeline import _setup_parser

    (tmp_path / "in").mkdir(exist_ok=True)
    p = argparse.ArgumentParser()
    _setup_parser(p)
    return p.parse_args(["--input-video-path", str(tmp_path / "in"),
                         "--output-clip-path", str(tmp_path / "out"), *extra])


def _inner(stages):
    return [st.stage if hasattr(st, "stage") else st for st in stages]


def test_cli_default_builds_todays_objects(tmp_path, monkeypatch):
    from cosmos_curate_amd.pipelines.video import splitting_pipeline as sp

    assert _split_args(tmp_path).embedding_resize == "cubic"
    with pytest.raises(SystemExit):
        _split_args(tmp_path, "--embedding-resize", "lanczos")
    # at the default the stages are constructed with exactly today's keywords
    seen = []
    real = sp.ClipEmbeddingStage

    def spy(*a, **kw):
        seen.append(kw)
        return real(*a, **kw)

    monkeypatch.setattr(sp, "ClipEmbeddingStage", spy)
    for extra in ((), ("--embedding-resize", "cubic")):
        stages = _inner(sp._assemble_stages(
            _split_args(tmp_path, "--aesthetic-threshold", "3.5", *extra)))
        assert [type(s).__name__ for s in stages] == [
            "VideoDownloader", "FixedStrideExtractorStage", "ClipTranscodingStage",
            "ClipFrameExtractionStage", "AestheticFilterStage", "ClipFrameCreationStage",
            "ClipEmbeddingStage", "ClipWriterStage"]
        assert seen.pop() == {"log_stats": True, "variant": "vit_b32"}
        assert stages[4].model._resize == "cubic" and stages[6].model._resize == "cubic"
    stages = _inner(sp._assemble_stages(_split_args(
        tmp_path, "--aesthetic-threshold", "3.5", "--embedding-resize", "antialias",
        "--embedding-model", "siglip_l16_256")))
    assert seen.pop() == {"log_stats": True, "variant": "siglip_l16_256",
                          "resize": "antialias"}
    assert stages[4].model._resize == "antialias" and stages[6].model._resize == "antialias"
    # ignored under internvideo2: the same stages with and without it
    iv2 = [type(s).__name__ for s in _inner(sp._assemble_stages(_split_args(
        tmp_path, "--embedding-algorithm", "internvideo2")))]
    iv2_aa = _inner(sp._assemble_stages(_split_args(
        tmp_path, "--embedding-algorithm", "internvideo2", "--embedding-resize",
        "antialias")))
    assert [type(s).__name__ for s in iv2_aa] == iv2
    assert not any(hasattr(s, "_resize") for s in iv2_aa)


def test_cli_dry_run_shows_the_option(tmp_path, capsys):
    from cosmos_curate_amd.pipelines.video.splitting_pipeline import split

    summary = split(_split_args(tmp_path, "--dry-run", "--aesthetic-threshold", "3.5"))
    assert summary["dry_run"] and summary["num_stages"] == 8
    quiet = capsys.readouterr().out.splitlines()
    assert "ClipEmbeddingStage" in quiet and "AestheticFilterStage" in quiet
    assert not any("resize" in line for line in quiet)
    split(_split_args(tmp_path, "--dry-run", "--aesthetic-threshold", "3.5",
                      "--embedding-resize", "antialias"))
    shown = capsys.readouterr().out.splitlines()
    assert "ClipEmbeddingStage resize=antialias" in shown
    assert "AestheticFilterStage resize=antialias" in shown
    assert len(shown) == len(quiet) == 8
    assert sum("resize" in line for line in shown) == 2
