"""Raw-NV12 / raw-P016 clip payload — the pluggable codec backend's null codec.

The hot path downstream of hardware decode consumes NV12 surfaces in HBM
(SURVEY.md §8 row a5).  This ROCm image ships no librocdecode (see
csrc/cc_decode.cpp), so kernel-path tests and the bench feed the pipeline
clips whose ``encoded_data`` is a raw NV12 payload instead of H.264
(SURVEY.md §7 hard part (d): "design the ABI so the codec is a pluggable
backend (rocDecode | null-raw) and carry raw-frame fixtures").

Payload layout (little-endian), version 1 — 8-bit NV12:
    magic  b"CCNV12RAW\\0"  (10 bytes)
    u16 version=1
    u32 n_frames, height, width, fps_num, fps_den
    then per frame: Y plane (h*w bytes) + interleaved UV plane (h/2*w bytes)

Version 2 — 10/12-bit P016 (what a VCN session maps for Main10/Main12
streams).  Same magic, same 32-byte header, so routing on the magic and
``HEADER_SIZE`` byte slicing keep working:
    magic, u16 version=2
    u32 n_frames, height, width, fps_num
    u16 fps_den, u8 bit_depth (10 | 12), u8 matrix | full_range << 7
    then per frame: Y plane (h*w u16) + interleaved UV plane (h/2*w u16),
    samples little-endian and MSB-aligned (value << (16 - bit_depth))
``matrix`` is the conversion-kernel code (0 BT.601, 1 BT.709, 2 BT.2020-NCL),
the colour standard the clip signals.

Version 3 — version 2 whose colour byte also carries the transfer function
in bits 2..3: ``matrix | transfer << 2 | full_range << 7`` with ``transfer``
0 = unspecified / SDR, 1 = PQ (SMPTE ST 2084; cc_hdr_tables_build's code).
Only written for a nonzero transfer, so every version-2 payload keeps its
bytes.
"""

from __future__ import annotations

import struct

import numpy as np
import numpy.typing as npt

MAGIC = b"CCNV12RAW\x00"
_HDR = struct.Struct("<10sHIIIII")
_HDR2 = struct.Struct("<10sHIIIIHBB")
HEADER_SIZE = _HDR.size
assert _HDR2.size == HEADER_SIZE
TRANSFER_SDR, TRANSFER_PQ = 0, 1
TRANSFERS = (TRANSFER_SDR, TRANSFER_PQ)


def pack_header(
    n: int, h: int, w: int, fps_num: int, fps_den: int = 1, *,
    bit_depth: int = 8, matrix: int = 0, full_range: bool = False,
    transfer: int = 0,
) -> bytes:
    """The 32-byte payload header alone (for zero-copy body slicing).

    The defaults give a version-1 (8-bit NV12) header; ``bit_depth`` 10 or
    12 gives version 2, and version 3 with a nonzero ``transfer``.  Version
    1 has no room for colour signalling, so an 8-bit header takes none.
    """
    if transfer not in TRANSFERS:
        raise ValueError(f"transfer must be 0 (SDR) or 1 (PQ), got {transfer}")
    if bit_depth == 8:
        if matrix != 0 or full_range or transfer:
            raise ValueError("version-1 (8-bit) headers carry no colour signalling")
        return _HDR.pack(MAGIC, 1, n, h, w, fps_num, fps_den)
    if bit_depth not in (10, 12):
        raise ValueError(f"bit_depth must be 8, 10 or 12, got {bit_depth}")
    if matrix not in (0, 1, 2):
        raise ValueError(f"matrix must be 0, 1 or 2, got {matrix}")
    return _HDR2.pack(MAGIC, 3 if transfer else 2, n, h, w, fps_num, fps_den,
                      bit_depth,
                      matrix | (transfer << 2) | (int(bool(full_range)) << 7))


def encode_raw_nv12(
    y: npt.NDArray[np.uint8], uv: npt.NDArray[np.uint8], fps_num: int, fps_den: int = 1
) -> bytes:
    """Pack (N,H,W) Y + (N,H/2,W) interleaved-UV planes into a payload."""
    n, h, w = y.shape
    assert uv.shape == (n, h // 2, w), (y.shape, uv.shape)
    hdr = _HDR.pack(MAGIC, 1, n, h, w, fps_num, fps_den)
    frames = np.concatenate(
        [np.concatenate([y[i].reshape(-1), uv[i].reshape(-1)]) for i in range(n)]
    )
    return hdr + frames.tobytes()


def encode_raw_p016(
    y: npt.NDArray[np.uint16], uv: npt.NDArray[np.uint16], fps_num: int,
    fps_den: int = 1, *, bit_depth: int, matrix: int = 0, full_range: bool = False,
    transfer: int = 0,
) -> bytes:
    """Pack (N,H,W) Y + (N,H/2,W) interleaved-UV u16 planes (MSB-aligned
    samples) into a version-2 payload (version 3 with a nonzero
    ``transfer``)."""
    n, h, w = y.shape
    assert y.dtype == np.uint16 and uv.dtype == np.uint16, (y.dtype, uv.dtype)
    assert uv.shape == (n, h // 2, w), (y.shape, uv.shape)
    hdr = pack_header(n, h, w, fps_num, fps_den, bit_depth=bit_depth,
                      matrix=matrix, full_range=full_range, transfer=transfer)
    frames = np.concatenate(
        [np.concatenate([y[i].reshape(-1), uv[i].reshape(-1)]) for i in range(n)]
    )
    return hdr + frames.astype("<u2", copy=False).tobytes()


def is_raw_nv12(data: bytes | npt.NDArray[np.uint8]) -> bool:
    """True for a raw payload of either version (NV12 or P016)."""
    b = bytes(data[: len(MAGIC)])
    return b == MAGIC


def _unpack(data: bytes) -> tuple[int, int, int, int, int, int, int, bool]:
    """(n, h, w, fps_num, fps_den, bit_depth, matrix, full_range)."""
    head = bytes(data[:HEADER_SIZE])
    magic, ver, n, h, w, num, den = _HDR.unpack_from(head)
    assert magic == MAGIC and ver in (1, 2, 3), (magic, ver)
    if ver == 1:
        return n, h, w, num, den, 8, 0, False
    _, _, n, h, w, num, den, depth, flags = _HDR2.unpack_from(head)
    if ver == 3:
        # bits 2..3 are the transfer (parse_transfer); the rest as version 2
        assert (flags >> 2) & 3 in TRANSFERS and not flags & 0x70, flags
        flags &= ~0x0C
    assert depth in (10, 12) and (flags & 0x7F) in (0, 1, 2), (depth, flags)
    return n, h, w, num, den, depth, flags & 0x7F, bool(flags >> 7)


def parse_transfer(data: bytes) -> int:
    """The transfer function the payload signals: 0 unspecified / SDR (every
    version-1 and version-2 payload), 1 PQ."""
    _unpack(data)  # the header checks
    head = bytes(data[:HEADER_SIZE])
    ver = _HDR.unpack_from(head)[1]
    return (_HDR2.unpack_from(head)[8] >> 2) & 3 if ver == 3 else TRANSFER_SDR


def parse_header(data: bytes) -> tuple[int, int, int, float]:
    """Returns (n_frames, height, width, fps) for either version."""
    n, h, w, num, den, *_ = _unpack(data)
    return n, h, w, num / den


def parse_format(data: bytes) -> tuple[int, int, bool, int]:
    """Returns (bit_depth, matrix, full_range, bytes_per_sample);
    (8, 0, False, 1) for a version-1 payload."""
    *_, depth, matrix, full_range = _unpack(data)
    return depth, matrix, full_range, 1 if depth == 8 else 2


def frame_nbytes(data: bytes) -> int:
    """Bytes one frame (Y + UV planes) occupies in the payload body."""
    _, h, w, _ = parse_header(data)
    return (h * w + (h // 2) * w) * parse_format(data)[3]


def frame_planes(
    data: bytes, indices: npt.NDArray[np.int32]
) -> tuple[npt.NDArray, npt.NDArray]:
    """Host gather of selected frames' (Y, UV) planes from the payload:
    uint8 arrays for version 1, uint16 (MSB-aligned samples) for version 2."""
    n, h, w, _ = parse_header(data)
    dtype = np.dtype(np.uint8) if parse_format(data)[3] == 1 else np.dtype("<u2")
    fsz = h * w + (h // 2) * w  # samples per frame
    body = np.frombuffer(data, dtype=dtype, offset=_HDR.size)
    ys = np.empty((len(indices), h, w), dtype=dtype)
    uvs = np.empty((len(indices), h // 2, w), dtype=dtype)
    for j, i in enumerate(indices.tolist()):
        base = i * fsz
        ys[j] = body[base : base + h * w].reshape(h, w)
        uvs[j] = body[base + h * w : base + fsz].reshape(h // 2, w)
    return ys, uvs


def timestamps(data: bytes) -> npt.NDArray[np.float32]:
    """Synthesized PTS grid i/fps, float32 (the null codec's demux)."""
    n, _, _, fps = parse_header(data)
    return (np.arange(n, dtype=np.float32) / np.float32(fps)).astype(np.float32)


def make_synthetic_clip(
    n_frames: int, height: int, width: int, fps: int, seed: int
) -> bytes:
    """Seeded moving-gradient + noise NV12 clip (BASELINE.md corpus recipe)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:height, 0:width]
    t = np.arange(n_frames)[:, None, None]
    y = ((xx[None] * 255 // max(width, 1) + yy[None] // 2 + t * 7) % 256).astype(np.uint8)
    y = np.clip(
        y.astype(np.int16) + rng.integers(-12, 13, size=y.shape, dtype=np.int16), 0, 255
    ).astype(np.uint8)
    uv = rng.integers(96, 160, size=(n_frames, height // 2, width), dtype=np.uint8).astype(
        np.uint8
    )
    return encode_raw_nv12(y, uv, fps)


def make_synthetic_clip_p016(
    n_frames: int, height: int, width: int, fps: int, seed: int, *,
    bit_depth: int = 10, matrix: int = 0, full_range: bool = False,
    transfer: int = 0,
) -> bytes:
    """Seeded moving-gradient + noise P016 clip with TRUE ``bit_depth``-bit
    content: the gradient and the noise live on the full 2^bit_depth code
    range (the low bits below 8-bit precision are populated), then samples
    are MSB-aligned as a decoder surface would hold them.  ``transfer`` only
    labels the payload (version 3 when nonzero); the samples are the same."""
    rng = np.random.default_rng(seed)
    top = 1 << bit_depth
    step = top // 256
    yy, xx = np.mgrid[0:height, 0:width]
    t = np.arange(n_frames)[:, None, None]
    y = (xx[None] * (top - 1) // max(width, 1) + yy[None] * step // 2
         + t * (7 * step + 1)) % top
    y = np.clip(y + rng.integers(-12 * step, 12 * step + 1, size=y.shape), 0, top - 1)
    uv = rng.integers(96 * step, 160 * step, size=(n_frames, height // 2, width))
    shift = 16 - bit_depth
    return encode_raw_p016(
        (y << shift).astype(np.uint16), (uv << shift).astype(np.uint16), fps,
        bit_depth=bit_depth, matrix=matrix, full_range=full_range,
        transfer=transfer,
    )
