"""External pin of the demuxer's PTS contract against the H.264
BITSTREAM — the independent authority inside the same files.

VERDICT r01 ("What's weak" #3): the sintel_pts golden was produced by
the oracle's own parser, so an elst/ctts bug would propagate into
"expected".  This suite re-derives the facts from the video elementary
stream instead (oracle/h264_bitstream.py — SPS geometry, VUI timing,
slice-header picture order counts per ISO/IEC 14496-10 §8.2.1), which
the container tables never touch:

  * display order from POC  ==  presentation order from ctts-derived PTS
  * SPS crop-adjusted WxH   ==  demux probe WxH
  * VUI fps (when present)  ==  stts-derived average fps
  * frame_num continuity sanity on the decode-order walk

Runs on the committed real-AVC fixtures (tests/golden_videos.py: the
reference's test_clip_10s / test_video_30s and the ffmpeg samples
cockatoo / realshort, slice payload blanked past the headers).
"""

from __future__ import annotations

import numpy as np
import pytest

from golden_videos import NAMES, video_bytes
from oracle import h264_bitstream as bs
from oracle import mp4_demux

# real AVC elementary streams only (synth_bframes.mp4 carries fake
# payloads for container-level tests and has no parsable slices).
# cockatoo is the load-bearing case: a real ffmpeg B-frame stream
# (275/280 nonzero ctts entries, 59 reordered positions) — exactly the
# reordering the VERDICT asked to pin externally.
FIXTURES = list(NAMES)


def _segment_order_check(ticks, pocs_idr, name):
    """Per coded-video-sequence (IDR-delimited): POC display order must
    equal the ctts-derived PTS order.  POC resets at IDRs, so the
    comparison is segment-local by construction (§8.2.1)."""
    starts = [i for i, (_, idr) in enumerate(pocs_idr) if idr] or [0]
    bounds = [*starts, len(pocs_idr)]
    reordered_total = 0
    for a, b in zip(bounds[:-1], bounds[1:]):
        seg_pts = np.array(ticks[a:b], dtype=np.int64)
        seg_poc = np.array([p for p, _ in pocs_idr[a:b]], dtype=np.int64)
        o1 = np.argsort(seg_pts, kind="stable")
        o2 = np.argsort(seg_poc, kind="stable")
        assert np.array_equal(o1, o2), (
            f"{name}: display order diverges in segment [{a}:{b}]")
        reordered_total += int((o1 != np.arange(b - a)).sum())
    return reordered_total


@pytest.mark.parametrize("name", FIXTURES)
def test_poc_display_order_matches_ctts_pts(name):
    data = video_bytes(name)
    trk = mp4_demux.parse_mp4(data)[0]
    pkts = mp4_demux.annexb_packets(data, trk)
    ticks = trk.pts
    pocs_idr = bs.access_unit_pocs_idr(pkts)
    assert len(pocs_idr) == len(ticks)
    reordered = _segment_order_check(ticks, pocs_idr, name)
    if name == "cockatoo":
        # the B-frame case must actually exercise reordering
        assert reordered >= 50, reordered


@pytest.mark.parametrize("name", FIXTURES)
def test_sps_geometry_and_fps_match_container(name):
    data = video_bytes(name)
    trk = mp4_demux.parse_mp4(data)[0]
    pkts = mp4_demux.annexb_packets(data, trk)[:4]
    sps = bs.sps_of_packets(pkts)
    assert (sps.width, sps.height) == (trk.width, trk.height)
    if sps.fps is not None:
        ts = trk.pts_seconds_sorted()
        stts_fps = (len(ts) - 1) / float(ts[-1] - ts[0])
        assert sps.fps == pytest.approx(stts_fps, rel=0.02)


def test_bitstream_parser_on_c_abi_packets():
    """The C demuxer's packets (the PRODUCT path) carry the same POC
    order — the pin holds through the C ABI, not just the oracle."""
    from cosmos_curate_amd import hotpath

    data = video_bytes("cockatoo")
    with hotpath.Demuxer(data) as d:
        info = d.probe()
        pkts, ticks = [], []
        for i in range(info.num_samples):
            pkt, pts, _ = d.packet(i)
            pkts.append(pkt)
            ticks.append(pts)
    _segment_order_check(ticks, bs.access_unit_pocs_idr(pkts),
                         "c-abi:cockatoo")


def test_pin_catches_ctts_corruption():
    """Negative control: corrupt one ctts entry of the real B-frame
    stream and the POC pin must DETECT the divergence — evidence the
    cross-check has teeth, not just vacuous agreement."""
    data = bytearray(video_bytes("cockatoo"))
    i = bytes(data).find(b"ctts")
    assert i > 0, "fixture has no ctts box"
    # ctts box: size(4) type(4) ver/flags(4) entry_count(4) then
    # (sample_count, sample_offset) pairs — swap the offsets of the
    # first two entries if distinct, else scale one up
    import struct

    entry0 = i + 12
    _, off0 = struct.unpack_from(">II", data, entry0)
    _, off1 = struct.unpack_from(">II", data, entry0 + 8)
    if off0 != off1:
        struct.pack_into(">I", data, entry0 + 4, off1)
        struct.pack_into(">I", data, entry0 + 8 + 4, off0)
    else:
        struct.pack_into(">I", data, entry0 + 4, off0 + 1024)
    trk = mp4_demux.parse_mp4(bytes(data))[0]
    pkts = mp4_demux.annexb_packets(bytes(data), trk)
    pocs_idr = bs.access_unit_pocs_idr(pkts)
    with pytest.raises(AssertionError):
        _segment_order_check(trk.pts, pocs_idr, "corrupted-ctts")
