"""ctypes binding to libcchot.so — the product side of the C ABI.

Declarations mirror include/cc_hotpath.h one-to-one.  Host entry points
(demux) work anywhere; device entry points require a GPU and FAIL LOUDLY
when the extension or the device is missing — there is no CPU fallback in
the product path (tier contract; see also csrc/cc_decode.cpp for the
rocDecode seam).
"""

from __future__ import annotations

import ctypes
import functools
import pathlib

import numpy as np
import numpy.typing as npt

_LIB_PATH = pathlib.Path(__file__).resolve().parent / "lib" / "libcchot.so"
_lib: ctypes.CDLL | None = None


class HotpathUnavailableError(RuntimeError):
    """libcchot.so missing or unusable — the product GPU path must not run."""


class GemmPlan(ctypes.Structure):
    """cc_gemm_plan_info: how a GEMM call would be launched."""

    _fields_ = [
        ("body", ctypes.c_int32),
        ("tiles_x", ctypes.c_int32),
        ("tiles_y", ctypes.c_int32),
        ("grid", ctypes.c_int32),
        ("block", ctypes.c_int32),
        ("xcd_remap", ctypes.c_int32),
        ("epi_staged", ctypes.c_int32),
    ]


class AttnPlan(ctypes.Structure):
    """cc_attn_plan_info: how a cc_attn call would be launched."""

    _fields_ = [
        ("rung", ctypes.c_int32),
        ("grid", ctypes.c_int32),
        ("block", ctypes.c_int32),
    ]


ATTN_RUNGS = ("small", "mid", "flash")  # cc_attn_plan_info.rung values


def _declare(lib: ctypes.CDLL) -> None:
    c = ctypes
    lib.cc_last_error.restype = c.c_char_p
    lib.cc_hip_available.restype = c.c_int
    lib.cc_rocdecode_available.restype = c.c_int

    lib.cc_demux_open.argtypes = [c.c_char_p, c.c_size_t, c.POINTER(c.c_void_p)]
    lib.cc_demux_probe.argtypes = [c.c_void_p, c.c_void_p]
    lib.cc_demux_timestamps.argtypes = [
        c.c_void_p, c.c_void_p, c.c_size_t, c.POINTER(c.c_size_t)]
    lib.cc_demux_packet.argtypes = [
        c.c_void_p, c.c_size_t, c.POINTER(c.c_void_p), c.POINTER(c.c_size_t),
        c.POINTER(c.c_int64), c.POINTER(c.c_int32)]
    lib.cc_demux_close.argtypes = [c.c_void_p]
    lib.cc_demux_remux_clip.argtypes = [
        c.c_void_p, c.c_double, c.c_double, c.POINTER(c.c_void_p),
        c.POINTER(c.c_size_t)]
    lib.cc_buffer_free.argtypes = [c.c_void_p]

    lib.cc_decode_session_create.argtypes = [
        c.c_int, c.c_int32, c.POINTER(c.c_void_p)]
    lib.cc_decode_submit.argtypes = [
        c.c_void_p, c.c_char_p, c.c_size_t, c.c_int64]
    lib.cc_decode_map_frames.argtypes = [
        c.c_void_p, c.c_void_p, c.c_size_t, c.POINTER(c.c_size_t)]
    lib.cc_decode_stream_format.argtypes = [c.c_void_p, c.c_void_p]
    lib.cc_decode_stream_transfer.argtypes = [
        c.c_void_p, c.POINTER(c.c_int32), c.POINTER(c.c_int32)]
    lib.cc_decode_recycle.argtypes = [c.c_void_p]
    lib.cc_decode_destroy.argtypes = [c.c_void_p]

    lib.cc_malloc.argtypes = [c.POINTER(c.c_void_p), c.c_size_t]
    lib.cc_free.argtypes = [c.c_void_p]
    lib.cc_memcpy_h2d.argtypes = [c.c_void_p, c.c_void_p, c.c_size_t, c.c_uint64]
    lib.cc_memcpy_d2h.argtypes = [c.c_void_p, c.c_void_p, c.c_size_t, c.c_uint64]
    lib.cc_stream_sync.argtypes = [c.c_uint64]

    lib.cc_nv12_to_rgb.argtypes = [
        c.c_void_p, c.c_void_p, c.c_int, c.c_int, c.c_int, c.c_size_t,
        c.c_void_p, c.c_uint64]
    lib.cc_nv12_to_rgb_resize.argtypes = [
        c.c_void_p, c.c_void_p, c.c_int, c.c_int, c.c_int, c.c_size_t,
        c.c_void_p, c.c_int, c.c_int, c.c_uint64]
    lib.cc_yuv420sp_to_rgb.argtypes = [
        c.c_void_p, c.c_void_p, c.c_int, c.c_int, c.c_int, c.c_size_t,
        c.c_int, c.c_int, c.c_int, c.c_void_p, c.c_uint64]
    lib.cc_yuv420sp_to_rgb_resize.argtypes = [
        c.c_void_p, c.c_void_p, c.c_int, c.c_int, c.c_int, c.c_size_t,
        c.c_int, c.c_int, c.c_int, c.c_void_p, c.c_int, c.c_int, c.c_uint64]
    lib.cc_hdr_tables_build.argtypes = [c.c_int, c.c_float, c.c_void_p]
    lib.cc_yuv420sp_hdr_to_rgb.argtypes = [
        c.c_void_p, c.c_void_p, c.c_int, c.c_int, c.c_int, c.c_size_t,
        c.c_int, c.c_int, c.c_int, c.c_void_p, c.c_float, c.c_void_p,
        c.c_uint64]
    lib.cc_yuv420sp_hdr_to_rgb_resize.argtypes = [
        c.c_void_p, c.c_void_p, c.c_int, c.c_int, c.c_int, c.c_size_t,
        c.c_int, c.c_int, c.c_int, c.c_void_p, c.c_float, c.c_void_p,
        c.c_int, c.c_int, c.c_uint64]
    lib.cc_resize_bilinear_u8.argtypes = [
        c.c_void_p, c.c_int, c.c_int, c.c_int, c.c_void_p, c.c_int, c.c_int,
        c.c_uint64]
    lib.cc_resize_bicubic_u8.argtypes = lib.cc_resize_bilinear_u8.argtypes
    lib.cc_resize_aa_table_build.argtypes = [
        c.c_int, c.c_int, c.c_int, c.c_int, c.c_int, c.c_void_p, c.c_size_t,
        c.POINTER(c.c_int)]
    lib.cc_resize_aa_u8.argtypes = [
        c.c_void_p, c.c_int, c.c_int, c.c_int, c.c_void_p, c.c_int, c.c_int,
        c.c_void_p, c.c_int, c.c_void_p, c.c_int, c.c_uint64]
    lib.cc_clip_preprocess.argtypes = [
        c.c_void_p, c.c_int, c.c_int, c.c_int, c.POINTER(c.c_float),
        c.POINTER(c.c_float), c.c_void_p, c.c_int, c.c_uint64]
    lib.cc_clip_preprocess_patches.argtypes = [
        c.c_void_p, c.c_int, c.c_int, c.c_int, c.c_int, c.c_int,
        c.POINTER(c.c_float), c.POINTER(c.c_float), c.c_void_p, c.c_uint64]
    lib.cc_gather_frames_u8.argtypes = [
        c.c_void_p, c.c_int, c.c_size_t, c.c_void_p, c.c_void_p, c.c_int,
        c.c_int, c.c_void_p, c.c_uint64]
    lib.cc_motion_estimate.argtypes = [
        c.c_void_p, c.c_void_p, c.c_int, c.c_int, c.c_int, c.c_size_t,
        c.c_size_t, c.c_int, c.c_int, c.c_int, c.c_void_p, c.c_void_p,
        c.c_uint64]
    lib.cc_gemm_bf16.argtypes = [
        c.c_void_p, c.c_void_p, c.c_void_p, c.c_int64, c.c_int64, c.c_int64,
        c.c_void_p, c.c_int, c.c_uint64]
    lib.cc_gemm_bf16_ex.argtypes = [
        c.c_void_p, c.c_void_p, c.c_void_p, c.c_int64, c.c_int64, c.c_int64,
        c.c_void_p, c.c_int, c.c_int, c.c_void_p, c.c_uint64]
    lib.cc_gemm_bf16_strided.argtypes = [
        c.c_void_p, c.c_int64, c.c_void_p, c.c_void_p, c.c_int64, c.c_int64,
        c.c_int64, c.c_void_p, c.c_int, c.c_int, c.c_void_p, c.c_int64,
        c.c_uint64]
    lib.cc_gemm_plan.argtypes = [
        c.c_int64, c.c_int64, c.c_int64, c.c_int64, c.c_int64, c.c_int,
        c.c_int, c.c_int, c.POINTER(GemmPlan)]

    lib.cc_attn_cls.argtypes = [
        c.c_void_p, c.c_void_p, c.c_void_p, c.c_int64, c.c_void_p, c.c_int64,
        c.c_int, c.c_int, c.c_int, c.c_float, c.c_uint64]
    lib.cc_attn.argtypes = [
        c.c_void_p, c.c_void_p, c.c_int64, c.c_int, c.c_int, c.c_int,
        c.c_float, c.c_uint64]
    lib.cc_attn_plan.argtypes = [
        c.c_int64, c.c_int, c.c_int, c.c_int, c.POINTER(AttnPlan)]
    lib.cc_attn_small.argtypes = lib.cc_attn.argtypes
    lib.cc_attn_mid.argtypes = lib.cc_attn.argtypes
    lib.cc_attn_flash.argtypes = lib.cc_attn.argtypes
    lib.cc_attn_rung.argtypes = [c.c_int, *lib.cc_attn.argtypes]
    lib.cc_layernorm_bf16.argtypes = [
        c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_int64, c.c_int64,
        c.c_float, c.c_uint64]
    lib.cc_ln_stats_bf16.argtypes = [
        c.c_void_p, c.c_int64, c.c_int64, c.c_void_p, c.c_uint64]
    lib.cc_ln_finalize.argtypes = [
        c.c_void_p, c.c_int64, c.c_int64, c.c_int64, c.c_float, c.c_void_p,
        c.c_uint64]
    lib.cc_gemm_bf16_res_stats.argtypes = [
        c.c_void_p, c.c_void_p, c.c_void_p, c.c_int64, c.c_int64, c.c_int64,
        c.c_void_p, c.c_void_p, c.c_void_p, c.c_uint64]
    lib.cc_gemm_bf16_ln.argtypes = [
        c.c_void_p, c.c_int64, c.c_void_p, c.c_void_p, c.c_void_p,
        c.c_void_p, c.c_void_p, c.c_void_p, c.c_int64, c.c_int64, c.c_int64,
        c.c_int, c.c_float, c.c_uint64]
    lib.cc_rms_finalize.argtypes = lib.cc_ln_finalize.argtypes
    lib.cc_gemm_bf16_rms.argtypes = lib.cc_gemm_bf16_ln.argtypes
    lib.cc_rmsnorm_bf16.argtypes = [
        c.c_void_p, c.c_void_p, c.c_void_p, c.c_int64, c.c_int64, c.c_float,
        c.c_uint64]
    lib.cc_qk_rmsnorm_bf16.argtypes = [
        c.c_void_p, c.c_int64, c.c_int64, c.c_int64, c.c_void_p, c.c_void_p,
        c.c_float, c.c_uint64]
    lib.cc_embed_assemble_ln.argtypes = [
        c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p,
        c.c_void_p, c.c_int64, c.c_int64, c.c_int64, c.c_float, c.c_uint64]
    lib.cc_pairwise_max_earlier.argtypes = [
        c.c_void_p, c.c_int64, c.c_int64, c.c_void_p, c.c_void_p, c.c_uint64]
    lib.cc_conv3x3_bf16.argtypes = [
        c.c_void_p, c.c_void_p, c.c_void_p, c.c_int64, c.c_int, c.c_int,
        c.c_int, c.c_int, c.c_uint64]
    lib.cc_conv3x3_u8.argtypes = [
        c.c_void_p, c.c_void_p, c.c_void_p, c.c_int64, c.c_int, c.c_int,
        c.c_int, c.c_uint64]
    lib.cc_tconv3_bf16.argtypes = [
        c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_int64,
        c.c_int, c.c_int, c.c_int, c.c_uint64]
    lib.cc_avgpool2x2_bf16.argtypes = [
        c.c_void_p, c.c_void_p, c.c_int64, c.c_int, c.c_int, c.c_int,
        c.c_uint64]
    lib.cc_tn_hist512_u8.argtypes = [
        c.c_void_p, c.c_void_p, c.c_int64, c.c_int, c.c_uint64]
    lib.cc_tn_framesim_embed.argtypes = [
        c.c_void_p, c.c_void_p, c.c_void_p, c.c_int, c.c_int, c.c_int,
        c.c_int, c.c_int, c.c_int, c.c_int, c.c_void_p, c.c_void_p,
        c.c_void_p, c.c_int64, c.c_int, c.c_uint64]
    lib.cc_tn_simband_fc.argtypes = [
        c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_int64, c.c_int,
        c.c_int, c.c_int, c.c_int, c.c_uint64]
    lib.cc_tn_fc1_relu.argtypes = [
        c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p,
        c.c_void_p, c.c_int64, c.c_int, c.c_int, c.c_int, c.c_uint64]
    lib.cc_tn_cls_sigmoid.argtypes = [
        c.c_void_p, c.c_void_p, c.c_float, c.c_void_p, c.c_int64, c.c_int,
        c.c_uint64]

    lib.cc_timing_enable.argtypes = [c.c_int]
    lib.cc_timing_report.argtypes = [
        c.c_char_p, c.POINTER(c.c_double), c.POINTER(c.c_int64)]


def load() -> ctypes.CDLL:
    """dlopen libcchot.so (idempotent)."""
    global _lib
    if _lib is None:
        if not _LIB_PATH.exists():
            raise HotpathUnavailableError(
                f"{_LIB_PATH} not built — run python -m cosmos_curate_amd.build"
            )
        _lib = ctypes.CDLL(str(_LIB_PATH))
        _declare(_lib)
    return _lib


def available() -> bool:
    try:
        load()
    except HotpathUnavailableError:
        return False
    return True


def require_gpu() -> ctypes.CDLL:
    """The product GPU path gate: extension present AND a HIP device visible."""
    lib = load()
    rc = lib.cc_hip_available()
    if rc != 0:
        raise HotpathUnavailableError(
            f"HIP device unavailable: {lib.cc_last_error().decode()}"
        )
    return lib


def check(rc: int) -> None:
    if rc != 0:
        lib = load()
        raise RuntimeError(f"cc error {rc}: {lib.cc_last_error().decode()}")


def yuv_to_rgb_resize(
    y: int, uv: int, n: int, src_h: int, src_w: int, pitch_bytes: int,
    out_rgb: int, out_h: int, out_w: int, stream: int, *,
    bit_depth: int = 8, matrix: int = 0, full_range: bool = False,
) -> None:
    """Fused 4:2:0 semi-planar -> RGB + bilinear resize on device pointers.

    Always cc_yuv420sp_to_rgb_resize: the library's one YUV launcher picks
    the kernel, and at (8, bt601, limited) that is the kernel and the bits
    of cc_nv12_to_rgb_resize.  No fallback: a failing call raises.
    """
    check(load().cc_yuv420sp_to_rgb_resize(
        y, uv, n, src_h, src_w, pitch_bytes, bit_depth, matrix,
        int(bool(full_range)), out_rgb, out_h, out_w, stream))


HDR_TRANSFER_PQ = 1  # CC_HDR_TRANSFER_PQ
HDR_TABLE_BYTES = 20480  # CC_HDR_TABLE_BYTES: f32 tin[4096] then u8 tout[4096]


def hdr_tables_build(
    transfer: int = HDR_TRANSFER_PQ, reference_white_nits: float = 203.0,
) -> npt.NDArray[np.uint8]:
    """The table image of cc_hdr_tables_build as host bytes (host-only, no
    GPU needed): ``img[:16384].view(np.float32)`` is ``tin``,
    ``img[16384:]`` is ``tout``.  Raises on a transfer without tables or a
    reference white that is not positive and finite."""
    img = np.empty(HDR_TABLE_BYTES, dtype=np.uint8)
    check(load().cc_hdr_tables_build(
        transfer, reference_white_nits, img.ctypes.data_as(ctypes.c_void_p)))
    return img


_hdr_tables_dev: dict[tuple[int, int, float], object] = {}


def hdr_tables(
    transfer: int = HDR_TRANSFER_PQ, reference_white_nits: float = 203.0,
):
    """The same image as a uint8 device tensor on the current device, built
    and uploaded once per (device, transfer, reference white); pass its
    ``data_ptr()`` as ``tables``."""
    import torch

    key = (torch.cuda.current_device(), int(transfer), float(reference_white_nits))
    dev = _hdr_tables_dev.get(key)
    if dev is None:
        img = hdr_tables_build(transfer, reference_white_nits)
        dev = torch.from_numpy(img).to(torch.device("cuda", key[0]))
        _hdr_tables_dev[key] = dev
    return dev


def hdr_inv_w2(peak_nits: float, reference_white_nits: float = 203.0) -> float:
    """The tone-mapping constant 1/(peak/white)^2, rounded to f32 once."""
    if not (peak_nits > 0 and reference_white_nits > 0):
        raise ValueError("peak and reference white must be positive")
    ratio = float(peak_nits) / float(reference_white_nits)
    return float(np.float32(1.0 / (ratio * ratio)))


def yuv_hdr_to_rgb(
    y: int, uv: int, n: int, h: int, w: int, pitch_bytes: int, out_rgb: int,
    stream: int, *, tables: int, inv_w2: float,
    bit_depth: int = 10, matrix: int = 2, full_range: bool = False,
) -> None:
    """PQ 4:2:0 semi-planar -> tone-mapped SDR RGB at full resolution on
    device pointers (cc_yuv420sp_hdr_to_rgb).  No fallback: a failing call
    raises."""
    check(load().cc_yuv420sp_hdr_to_rgb(
        y, uv, n, h, w, pitch_bytes, bit_depth, matrix, int(bool(full_range)),
        tables, inv_w2, out_rgb, stream))


def yuv_hdr_to_rgb_resize(
    y: int, uv: int, n: int, src_h: int, src_w: int, pitch_bytes: int,
    out_rgb: int, out_h: int, out_w: int, stream: int, *, tables: int,
    inv_w2: float, bit_depth: int = 10, matrix: int = 2,
    full_range: bool = False,
) -> None:
    """yuv_to_rgb_resize for PQ content: every tap tone-mapped to SDR before
    the blend (cc_yuv420sp_hdr_to_rgb_resize).  No fallback: a failing call
    raises."""
    check(load().cc_yuv420sp_hdr_to_rgb_resize(
        y, uv, n, src_h, src_w, pitch_bytes, bit_depth, matrix,
        int(bool(full_range)), tables, inv_w2, out_rgb, out_h, out_w, stream))


RESIZE_AA_FILTERS = {"bilinear": 0, "bicubic": 1}  # CC_RESIZE_AA_*
RESIZE_AA_MAX_TAPS = 129  # CC_RESIZE_AA_MAX_TAPS


def _resize_aa_filter(filter: str | int) -> int:
    if isinstance(filter, str):
        if filter not in RESIZE_AA_FILTERS:
            raise ValueError(
                f"filter must be one of {sorted(RESIZE_AA_FILTERS)}, got {filter!r}")
        return RESIZE_AA_FILTERS[filter]
    return int(filter)


def resize_aa_table_build(
    filter: str | int, in_size: int, out_size: int, crop_off: int = 0,
    crop_len: int | None = None,
) -> tuple[npt.NDArray[np.uint8], int]:
    """One axis' table image of cc_resize_aa_table_build as host bytes, and
    its tap count (host-only, no GPU needed).  The image holds int32
    first[crop_len], int32 count[crop_len], f32 w[crop_len][taps] for the
    outputs [crop_off, crop_off + crop_len) of an in_size -> out_size
    antialiased resize; ``crop_len=None`` means up to out_size.  Raises on
    arguments the library rejects."""
    lib = load()
    if crop_len is None:
        crop_len = out_size - crop_off
    f = _resize_aa_filter(filter)
    taps = ctypes.c_int()
    nbytes = lib.cc_resize_aa_table_build(
        f, in_size, out_size, crop_off, crop_len, None, 0, ctypes.byref(taps))
    if nbytes < 0:
        check(nbytes)
    img = np.empty(nbytes, dtype=np.uint8)
    rc = lib.cc_resize_aa_table_build(
        f, in_size, out_size, crop_off, crop_len,
        img.ctypes.data_as(ctypes.c_void_p), nbytes, ctypes.byref(taps))
    if rc != nbytes:
        check(rc if rc < 0 else -1)
    return img, taps.value


def resize_aa_geometry(src_h: int, src_w: int, size: int) -> tuple[int, int, int, int]:
    """(rh, rw, top, left) of torchvision's Resize(size) + CenterCrop(size):
    the short side becomes ``size``, the long side ``int(size*long/short)``
    (truncating), the crop sits at ``int(round((resized - size) / 2.0))``
    with Python's round (half to even)."""
    if src_h <= 0 or src_w <= 0 or size <= 0:
        raise ValueError(f"non-positive size {src_h}x{src_w} -> {size}")
    if src_h <= src_w:
        rh, rw = size, int(size * src_w / src_h)
    else:
        rh, rw = int(size * src_h / src_w), size
    return rh, rw, int(round((rh - size) / 2.0)), int(round((rw - size) / 2.0))


class ResizeAATables:
    """Both axes' device tables of one (filter, src_h, src_w, size) resize +
    center crop: ``table_y`` / ``table_x`` (uint8 device tensors), their tap
    counts and the crop geometry."""

    __slots__ = ("table_y", "table_x", "taps_y", "taps_x", "size",
                 "resized_h", "resized_w", "top", "left")

    def __init__(self, table_y, table_x, taps_y, taps_x, size, resized_h,
                 resized_w, top, left) -> None:
        self.table_y, self.table_x = table_y, table_x
        self.taps_y, self.taps_x = taps_y, taps_x
        self.size = size
        self.resized_h, self.resized_w = resized_h, resized_w
        self.top, self.left = top, left


_resize_aa_tables_dev: dict[tuple[int, int, int, int, int], ResizeAATables] = {}


def resize_aa_tables(filter: str | int, src_h: int, src_w: int, size: int) -> ResizeAATables:
    """The tables of Resize(size, antialias=True) + CenterCrop(size) for
    (src_h, src_w) frames on the current device, built and uploaded once per
    (device, filter, src_h, src_w, size).  Raises when an axis needs more
    taps than the kernel takes (a downscale past 1/32 for bicubic)."""
    import torch

    f = _resize_aa_filter(filter)
    key = (torch.cuda.current_device(), f, int(src_h), int(src_w), int(size))
    tabs = _resize_aa_tables_dev.get(key)
    if tabs is None:
        rh, rw, top, left = resize_aa_geometry(src_h, src_w, size)
        img_y, taps_y = resize_aa_table_build(f, src_h, rh, top, size)
        img_x, taps_x = resize_aa_table_build(f, src_w, rw, left, size)
        if max(taps_y, taps_x) > RESIZE_AA_MAX_TAPS:
            raise ValueError(
                f"resize {src_h}x{src_w} -> {size} needs {max(taps_y, taps_x)} "
                f"taps, the kernel takes {RESIZE_AA_MAX_TAPS}")
        dev = torch.device("cuda", key[0])
        tabs = ResizeAATables(
            torch.from_numpy(img_y).to(dev), torch.from_numpy(img_x).to(dev),
            taps_y, taps_x, int(size), rh, rw, top, left)
        _resize_aa_tables_dev[key] = tabs
    return tabs


def resize_aa_center_crop(frames_dev_u8, size: int, filter: str | int = "bicubic"):
    """(n, h, w, 3) u8 on the device -> (n, size, size, 3) u8 on the device:
    torchvision's Resize(size, antialias=True) + CenterCrop(size) in one
    kernel that computes only the cropped region (cc_resize_aa_u8).  No
    fallback: a failing call raises."""
    import torch

    lib = require_gpu()
    if (frames_dev_u8.dtype != torch.uint8 or frames_dev_u8.ndim != 4
            or frames_dev_u8.shape[-1] != 3 or not frames_dev_u8.is_cuda):
        raise ValueError("frames must be a (n, h, w, 3) uint8 device tensor")
    n, h, w, _ = frames_dev_u8.shape
    with torch.cuda.device(frames_dev_u8.device):
        tabs = resize_aa_tables(filter, h, w, size)
        src = frames_dev_u8.contiguous()
        out = torch.empty((n, size, size, 3), dtype=torch.uint8, device=src.device)
        stream = torch.cuda.current_stream(src.device).cuda_stream
        check(lib.cc_resize_aa_u8(
            src.data_ptr(), n, h, w, out.data_ptr(), size, size,
            tabs.table_y.data_ptr(), tabs.taps_y, tabs.table_x.data_ptr(),
            tabs.taps_x, stream))
    return out


def estimate_motion(
    cur_ptr: int, ref_ptr: int, n: int, h: int, w: int, pitch_bytes: int,
    mv_out_ptr: int, stream: int, *,
    frame_stride_bytes: int | None = None, bit_depth: int = 8,
    search_range: int = 16, mv_lambda: int = 4, cost_out_ptr: int = 0,
) -> None:
    """Block-matching motion estimation of ``n`` (cur, ref) luma pairs on
    device pointers (cc_motion_estimate): int16 (dx, dy) per 16x16 block
    into ``mv_out_ptr`` [n, ceil(h/16), ceil(w/16), 2], optionally the
    winning cost as uint32 into ``cost_out_ptr``.

    ``frame_stride_bytes=None`` means densely stacked planes
    (``pitch_bytes*h``).  ``bit_depth`` 8 reads one byte per sample, 10 and
    12 two (P016).  No fallback: a failing call raises.
    """
    if bit_depth not in (8, 10, 12):
        raise ValueError(f"bit_depth must be 8, 10 or 12, got {bit_depth}")
    if frame_stride_bytes is None:
        frame_stride_bytes = pitch_bytes * h
    check(load().cc_motion_estimate(
        cur_ptr, ref_ptr, n, h, w, pitch_bytes, frame_stride_bytes,
        1 if bit_depth == 8 else 2, search_range, mv_lambda, mv_out_ptr,
        cost_out_ptr or None, stream))


def conv3x3_bf16(x_ptr: int, w_ptr: int, y_ptr: int, frames: int, h: int,
                 w: int, cin: int, cout: int, stream: int) -> None:
    """3x3 spatial conv, zero padding 1, on bf16 channels-last device
    pointers (cc_conv3x3_bf16): x [frames,h,w,cin], weights
    [cout][3][3][cin], y [frames,h,w,cout].  No fallback: a failing call
    raises."""
    check(load().cc_conv3x3_bf16(x_ptr, w_ptr, y_ptr, frames, h, w, cin, cout,
                                 stream))


def conv3x3_u8(x_ptr: int, w_ptr: int, y_ptr: int, frames: int, h: int,
               w: int, cout: int, stream: int) -> None:
    """The same conv for a 3-channel u8 input taken as bf16(x/255)
    (cc_conv3x3_u8): x u8 [frames,h,w,3], weights bf16 [cout][3][3][3]."""
    check(load().cc_conv3x3_u8(x_ptr, w_ptr, y_ptr, frames, h, w, cout, stream))


def tconv3_bf16(x_ptr: int, w_ptr: int, bias_ptr: int, shortcut_ptr: int,
                y_ptr: int, b: int, t: int, hw: int, f: int,
                stream: int) -> None:
    """Four-branch dilated temporal conv + bias + relu (+ shortcut) on
    device pointers (cc_tconv3_bf16): x [b,t,hw,8f], weights [4][f][3][2f],
    bias f32 [4f], y [b,t,hw,4f]; ``shortcut_ptr`` 0 for none."""
    check(load().cc_tconv3_bf16(x_ptr, w_ptr, bias_ptr, shortcut_ptr or None,
                                y_ptr, b, t, hw, f, stream))


def avgpool2x2_bf16(x_ptr: int, y_ptr: int, frames: int, h: int, w: int,
                    c: int, stream: int) -> None:
    """2x2 average pool of bf16 channels-last frames, odd sizes floored
    (cc_avgpool2x2_bf16): [frames,h,w,c] -> [frames,h//2,w//2,c]."""
    check(load().cc_avgpool2x2_bf16(x_ptr, y_ptr, frames, h, w, c, stream))


def tn_hist512_u8(frames_ptr: int, out_ptr: int, frames: int, pixels: int,
                  stream: int) -> None:
    """L2-normalised 512-bin RGB histograms (cc_tn_hist512_u8): u8
    [frames,pixels,3] -> f32 [frames,512]; at most 4096 pixels a frame."""
    check(load().cc_tn_hist512_u8(frames_ptr or None, out_ptr or None, frames,
                                  pixels, stream))


def tn_framesim_embed(maps: list[tuple[int, int, int]], proj_wt_ptr: int,
                      proj_b_ptr: int, out_ptr: int, frames: int, out_dim: int,
                      stream: int) -> None:
    """Spatial means of up to three bf16 channels-last maps, projection and
    L2 normalisation (cc_tn_framesim_embed).  ``maps`` holds (pointer, hw,
    channels) per map [frames,hw,channels]; weights f32 [sum channels][128]
    (transposed), out f32 [frames,128]."""
    n = len(maps)
    ptrs, hws, cs = ([m[i] for m in maps] + [0] * (3 - n) for i in range(3))
    check(load().cc_tn_framesim_embed(
        *(p or None for p in ptrs[:3]), *hws[:3], *cs[:3], n, proj_wt_ptr or None,
        proj_b_ptr or None, out_ptr or None, frames, out_dim, stream))


def tn_simband_fc(x_ptr: int, fc_wt_ptr: int, fc_b_ptr: int, out_ptr: int,
                  b: int, t: int, d: int, ldo: int, col: int, stream: int) -> None:
    """The 101-wide similarity band of every frame of x f32 [b,t,d] (d 128 or
    512), Linear(101,128) with weights f32 [101][128] (transposed) and relu
    (cc_tn_simband_fc), into columns [col, col+128) of out f32 [b*t,ldo]."""
    check(load().cc_tn_simband_fc(x_ptr or None, fc_wt_ptr or None,
                                  fc_b_ptr or None, out_ptr or None, b, t, d,
                                  ldo, col, stream))


def tn_fc1_relu(hd_ptr: int, feat_ptr: int, w_hi_ptr: int, w_lo_ptr: int,
                bias_ptr: int, y_ptr: int, m: int, kh: int, kf: int, n: int,
                stream: int) -> None:
    """relu(bias + [hd | feat] . w^T) with split-bf16 operands
    (cc_tn_fc1_relu): hd f32 [m,kh], feat bf16 [m,kf], w_hi and w_lo bf16
    [n][kh+kf], bias f32 [n], y f32 [m,n]."""
    check(load().cc_tn_fc1_relu(hd_ptr or None, feat_ptr or None,
                                w_hi_ptr or None, w_lo_ptr or None,
                                bias_ptr or None, y_ptr or None, m, kh, kf, n,
                                stream))


def tn_cls_sigmoid(y_ptr: int, w_ptr: int, b: float, p_ptr: int, m: int, n: int,
                   stream: int) -> None:
    """sigmoid(b + y . w) per row (cc_tn_cls_sigmoid): y f32 [m,n], w f32
    [n], p f32 [m]."""
    check(load().cc_tn_cls_sigmoid(y_ptr or None, w_ptr or None, b,
                                   p_ptr or None, m, n, stream))


def gemm_plan(
    M: int, N: int, K: int, *, lda: int | None = None, ldr: int | None = None,
    has_bias: bool = False, act: int = 0, has_residual: bool = False,
) -> GemmPlan:
    """The launch plan of a cc_gemm_bf16* call with these arguments
    (cc_gemm_plan; default knobs, host-only).  ``lda`` / ``ldr`` default to
    dense rows.  Raises on arguments the GEMM itself would reject."""
    plan = GemmPlan()
    check(load().cc_gemm_plan(
        M, N, K, K if lda is None else lda, N if ldr is None else ldr,
        int(has_bias), act, int(has_residual), ctypes.byref(plan)))
    return plan


def attn_plan(n_frames: int, seq: int, heads: int, hidden: int) -> AttnPlan:
    """The launch plan of a cc_attn call with these arguments (cc_attn_plan;
    host-only): ``ATTN_RUNGS[plan.rung]`` names the kernel.  Raises on
    arguments cc_attn itself would reject."""
    plan = AttnPlan()
    check(load().cc_attn_plan(n_frames, seq, heads, hidden, ctypes.byref(plan)))
    return plan


@functools.lru_cache(maxsize=None)
def attn_supported(heads: int, hidden: int) -> bool:
    """Whether cc_attn takes this head geometry — the library's own answer
    (cc_attn_plan accepts it), so the set of head dims is stated once, in
    csrc/cc_attn_plan.hpp.  Asked once per geometry."""
    plan = AttnPlan()
    return load().cc_attn_plan(1, 1, heads, hidden, ctypes.byref(plan)) == 0


class VideoInfo(ctypes.Structure):
    _fields_ = [
        ("width", ctypes.c_uint32),
        ("height", ctypes.c_uint32),
        ("timescale", ctypes.c_uint32),
        ("num_samples", ctypes.c_uint32),
        ("num_sync_samples", ctypes.c_uint32),
        ("codec", ctypes.c_int32),
        ("duration_s", ctypes.c_double),
        ("avg_fps", ctypes.c_double),
    ]


class Nv12Frame(ctypes.Structure):
    """cc_nv12_frame: a mapped VCN NV12 or P016 surface (device pointers;
    pitch in bytes)."""

    _fields_ = [
        ("y", ctypes.c_void_p),
        ("uv", ctypes.c_void_p),
        ("pitch", ctypes.c_size_t),
        ("pts", ctypes.c_int64),
        ("width", ctypes.c_uint32),
        ("height", ctypes.c_uint32),
    ]


class StreamFormat(ctypes.Structure):
    """cc_stream_format: what the stream's sequence header signalled."""

    _fields_ = [
        ("bit_depth", ctypes.c_int32),
        ("chroma_format", ctypes.c_int32),
        ("matrix_coefficients", ctypes.c_int32),
        ("full_range", ctypes.c_int32),
        ("bytes_per_sample", ctypes.c_int32),
    ]


class DecodeSession:
    """RAII wrapper over cc_decode_* (the VCN/rocDecode seam,
    nvcodec_utils.py:199-313 NvVideoDecoder counterpart).

    Raises on construction with CC_ERR_NO_ROCDECODE when librocdecode is
    absent — loud, no CPU fallback.  Mapped surfaces stay valid until
    ``recycle()``; consume (launch + synchronize) first.
    """

    def __init__(self, device: int = 0, codec: int = 0) -> None:
        lib = load()
        h = ctypes.c_void_p()
        check(lib.cc_decode_session_create(device, codec, ctypes.byref(h)))
        self._lib = lib
        self._h: ctypes.c_void_p | None = h

    def submit(self, packet: bytes | None, pts: int = 0) -> None:
        """One AnnexB access unit; None flushes (end of stream)."""
        if packet is None:
            check(self._lib.cc_decode_submit(self._h, None, 0, 0))
        else:
            check(self._lib.cc_decode_submit(self._h, packet, len(packet), pts))

    def map_frames(self, cap: int = 32) -> list[Nv12Frame]:
        arr = (Nv12Frame * cap)()
        n = ctypes.c_size_t()
        check(self._lib.cc_decode_map_frames(
            self._h, ctypes.byref(arr), cap, ctypes.byref(n)))
        return [arr[i] for i in range(n.value)]

    def stream_format(self) -> StreamFormat:
        """Bit depth, chroma format and colour signalling of the stream;
        raises before the first sequence header has been parsed."""
        fmt = StreamFormat()
        check(self._lib.cc_decode_stream_format(self._h, ctypes.byref(fmt)))
        return fmt

    def stream_transfer(self) -> tuple[int, int]:
        """(transfer_characteristics, colour_primaries), the H.273 codes of
        the stream (16 = PQ, 9 = BT.2020); raises when stream_format does."""
        tc, cp = ctypes.c_int32(), ctypes.c_int32()
        check(self._lib.cc_decode_stream_transfer(
            self._h, ctypes.byref(tc), ctypes.byref(cp)))
        return tc.value, cp.value

    def recycle(self) -> None:
        check(self._lib.cc_decode_recycle(self._h))

    def close(self) -> None:
        if self._h is not None:
            self._lib.cc_decode_destroy(self._h)
            self._h = None

    def __del__(self) -> None:  # pragma: no cover - GC timing
        try:
            self.close()
        except Exception:
            pass


class Demuxer:
    """RAII wrapper over cc_demux_* (host-only, no GPU needed)."""

    def __init__(self, data: bytes) -> None:
        lib = load()
        h = ctypes.c_void_p()
        check(lib.cc_demux_open(data, len(data), ctypes.byref(h)))
        self._lib = lib
        self._h: ctypes.c_void_p | None = h

    def probe(self) -> VideoInfo:
        info = VideoInfo()
        check(self._lib.cc_demux_probe(self._h, ctypes.byref(info)))
        return info

    def timestamps(self) -> npt.NDArray[np.float32]:
        n = ctypes.c_size_t()
        check(self._lib.cc_demux_timestamps(self._h, None, 0, ctypes.byref(n)))
        out = np.empty(n.value, dtype=np.float32)
        check(
            self._lib.cc_demux_timestamps(
                self._h, out.ctypes.data_as(ctypes.c_void_p), n.value, ctypes.byref(n)
            )
        )
        return out

    def packet(self, index: int) -> tuple[bytes, int, bool]:
        p = ctypes.c_void_p()
        sz = ctypes.c_size_t()
        pts = ctypes.c_int64()
        kf = ctypes.c_int32()
        check(
            self._lib.cc_demux_packet(
                self._h, index, ctypes.byref(p), ctypes.byref(sz),
                ctypes.byref(pts), ctypes.byref(kf),
            )
        )
        return ctypes.string_at(p, sz.value), pts.value, bool(kf.value)

    def remux_clip(self, start_s: float, end_s: float) -> bytes:
        """Sample-exact stream-copy of the span into a standalone MP4."""
        buf = ctypes.c_void_p()
        sz = ctypes.c_size_t()
        check(
            self._lib.cc_demux_remux_clip(
                self._h, start_s, end_s, ctypes.byref(buf), ctypes.byref(sz)
            )
        )
        try:
            return ctypes.string_at(buf, sz.value)
        finally:
            self._lib.cc_buffer_free(buf)

    def close(self) -> None:
        if self._h is not None:
            self._lib.cc_demux_close(self._h)
            self._h = None

    def __enter__(self) -> "Demuxer":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def __del__(self) -> None:
        try:
            self.close()
        except Exception:
            pass


def timing_enable(on: bool = True) -> None:
    lib = load()
    check(lib.cc_timing_enable(1 if on else 0))
    if on:
        check(lib.cc_timing_reset())


def timing_report(kernel: str) -> tuple[float, int]:
    """(total device ms, launch count) accumulated for `kernel`."""
    lib = load()
    ms = ctypes.c_double()
    cnt = ctypes.c_int64()
    check(lib.cc_timing_report(kernel.encode(), ctypes.byref(ms), ctypes.byref(cnt)))
    return ms.value, cnt.value
