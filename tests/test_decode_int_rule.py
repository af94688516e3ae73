"""CPU: the rule of alac_hip_decode_int as tests/decode_int_ref.py restates it.  It is the inverse of the source rule of
alac_hip_pcm_requantize: for every legal (D, container_bytes, S, left_justified) and both families of layouts, requantizing
(tests/pcm_requant_ref.py) what the reference wrote, with the same descriptor at depth D, returns the packed bytes it started
from with zero samples clipped; the identity descriptor reproduces the bytes; and the layout check accepts and refuses what
include/alac_hip.h lists."""
import numpy as np
import pytest

import decode_int_ref as ref
import pcm_requant_ref as rq

FRAME = 64
PACKETS = 3
SENTINEL = 0xC3


def samples(depth, channels, seed):
    """random samples with both extremes, zero and +-1 among them, int64 [channels, frames]"""
    rng = np.random.default_rng(seed)
    lo, hi = -(1 << (depth - 1)), (1 << (depth - 1)) - 1
    s = rng.integers(lo, hi + 1, (channels, FRAME * PACKETS), dtype=np.int64)
    edge = np.array([lo, hi, 0, -1, 1, lo + 1, hi - 1], np.int64)
    for c in range(channels):
        s[c, c:c + edge.size] = edge
        s[c, -edge.size:] = edge[::-1]
    return s


def layouts(channels, frames):
    """(name, channel_stride, frame_stride): planar, padded planar with strided frames, interleaved, padded channels-inner"""
    out = [("planar", frames, 1), ("frames inner, padded", 3 * frames + 5, 3), ("interleaved", 1, channels),
           ("channels inner, padded", 2, 2 * channels + 3)]
    return out


@pytest.mark.parametrize("channels", [1, 2, 3])
@pytest.mark.parametrize("depth,cb,S,lj", ref.LEGAL)
def test_requantizing_the_output_returns_the_bytes(depth, cb, S, lj, channels):
    frames = FRAME * PACKETS
    s = samples(depth, channels, depth * 7 + cb + S + lj + channels)
    raw = rq.pack(s, depth)
    assert np.array_equal(ref.samples_of(raw, depth, channels), s)
    for name, cs, fs in layouts(channels, frames):
        size = ref.span_bytes(channels, frames, cb, cs, fs) + 7
        out = np.full(size, SENTINEL, np.uint8)
        ref.decode_int(raw, depth, channels, cb, S, lj, cs, fs, out)
        v = ref.load(out, channels, frames, cb, cs, fs)
        got, clipped = rq.convert(v, S, cb, lj, depth, FRAME)
        assert not clipped.any(), (name, "clipped")
        assert np.array_equal(rq.pack(got, depth), raw), name
        # no byte outside the addressed containers moved
        touched = np.zeros(size, bool)
        at = ref.index_of(channels, frames, cs, fs) * cb
        for k in range(cb):
            touched[at + k] = True
        assert (out[~touched] == SENTINEL).all(), name
        assert touched.sum() == channels * frames * cb, name  # no two samples share a byte


@pytest.mark.parametrize("channels", [1, 2, 6])
@pytest.mark.parametrize("depth", ref.DEPTHS)
def test_identity_descriptor_reproduces_the_bytes(depth, channels):
    s = samples(depth, channels, depth + channels)
    raw = rq.pack(s, depth)
    d = ref.identity(depth, channels)
    out = np.full(raw.size, SENTINEL, np.uint8)
    ref.decode_int(raw, depth, channels, d["container_bytes"], d["bits"], d["left_justified"], d["channel_stride"],
                   d["frame_stride"], out)
    assert np.array_equal(out, raw)


def test_written_mask_leaves_the_rest_alone():
    s = samples(24, 2, 5)
    raw = rq.pack(s, 24)
    frames = s.shape[1]
    written = np.ones(s.shape, bool)
    written[:, FRAME * 2 + 10:] = False  # a short last packet
    out = np.full(2 * frames * 4, SENTINEL, np.uint8)
    ref.decode_int(raw, 24, 2, 4, 32, 1, frames, 1, out, written)
    v = out.view("<i4").reshape(2, frames)
    assert np.array_equal(v[written], (s[written] << 8).astype(np.int32))
    assert (out.reshape(2, frames, 4)[~written] == SENTINEL).all()


def test_full_scale_values_in_every_container():
    for depth, cb, S, lj in ref.LEGAL:
        lo, hi = -(1 << (depth - 1)), (1 << (depth - 1)) - 1
        v = ref.containers_of(np.array([lo, hi, -1, 0]), depth, cb, S, lj)
        width = 8 * cb if lj else S
        assert v[0] == -(1 << (width - 1)) and v[1] == (hi << (width - depth)) and v[3] == 0
        assert v[2] == -(1 << (width - depth))


def test_descriptor_check():
    for depth in ref.DEPTHS:
        for cb in (0, 1, 2, 3, 4, 5, 8):
            for S in (0, 8, 16, 20, 24, 28, 32, 64):
                for lj in (0, 1, 2):
                    legal = (depth, cb, S, lj) in ref.LEGAL
                    assert (ref.descriptor_refusal(depth, cb, S, lj) is None) == legal, (depth, cb, S, lj)
    assert ref.descriptor_refusal(16, 4, 32, 1, reserved=1) == "reserved"
    assert ref.descriptor_refusal(24, 4, 20, 0) == "bits below D"
    assert ref.descriptor_refusal(24, 2, 16, 1) == "bits below D"
    assert ref.descriptor_refusal(16, 2, 24, 1) == "bits"


def test_layout_check():
    T, C = 10 * 4096, 2
    ok = lambda cs, fs, ch=C: ref.layout_refusal(ch, T, 4, cs, fs) is None
    # frames inner: frame_stride >= 1 and channel_stride >= T * frame_stride
    assert ok(T, 1) and ok(T + 37, 1) and ok(3 * T, 3) and ok(3 * T + 1, 3)
    assert not ok(T - 1, 1) and not ok(3 * T - 1, 3)
    # channels inner: channel_stride >= 1 and frame_stride >= C * channel_stride
    assert ok(1, 2) and ok(1, 5) and ok(3, 6) and ok(3, 7)
    assert not ok(1, 1) and not ok(3, 5) and not ok(2, 3)
    assert ok(1, 6, ch=6) and not ok(1, 5, ch=6) and ok(2, 12, ch=6) and not ok(2, 11, ch=6)
    # zero strides
    assert not ok(T, 0) and not ok(0, 2) and not ok(0, 1)
    # one channel: only frame_stride >= 1
    assert ok(0, 1, ch=1) and ok(0, 7, ch=1) and ok(12345, 2, ch=1) and not ok(5, 0, ch=1)
    # a largest index whose byte offset overflows 64 bits
    assert not ok(1 << 62, 1) and not ok(1, 1 << 50) and not ok(0, 1 << 50, ch=1)
    # in every accepted layout the containers are distinct; in the refused ones above two of them coincide
    for cs, fs in ((40, 1), (45, 1), (120, 3), (1, 2), (1, 5), (3, 6), (3, 7)):
        assert ref.layout_refusal(2, 40, 4, cs, fs) is None
        at = ref.index_of(2, 40, cs, fs)
        assert np.unique(at).size == at.size, (cs, fs)
    for cs, fs in ((39, 1), (1, 1), (3, 3)):
        assert ref.layout_refusal(2, 40, 4, cs, fs) is not None
        at = ref.index_of(2, 40, cs, fs)
        assert np.unique(at).size < at.size, (cs, fs)
