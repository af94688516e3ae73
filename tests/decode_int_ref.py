"""The rule of alac_hip_decode_int (include/alac_hip.h) restated in numpy, from the header's text alone: the bytes
alac_hip_decode writes plus a destination descriptor give the containers, each at its index, and nothing else is touched;
and the checks of the descriptor and of the layout.  No library and no GPU needed."""
import numpy as np

DEPTHS = (16, 20, 24, 32)
BPS = {16: 2, 20: 3, 24: 3, 32: 4}
# every legal (D, container_bytes, S, left_justified): D <= S <= 8 * container_bytes
LEGAL = [(D, cb, S, lj) for D in DEPTHS for cb in (2, 3, 4) for S in DEPTHS for lj in (1, 0) if D <= S <= 8 * cb]


def samples_of(raw, depth, channels):
    """alac_hip_decode's bytes -> the decoded samples s, int64 [channels, frames]: the low D bits, sign-extended (a 20-bit
    sample sits left-justified in its 3-byte container)"""
    raw = np.ascontiguousarray(raw, np.uint8)
    if depth == 16:
        s = raw.view("<i2").astype(np.int64)
    elif depth == 32:
        s = raw.view("<i4").astype(np.int64)
    else:
        b = raw.reshape(-1, 3).astype(np.int64)
        s = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        s = (s ^ 0x800000) - 0x800000
        if depth == 20:
            s = s >> 4
    return np.ascontiguousarray(s.reshape(-1, channels).T)


def shift_of(depth, container_bytes, bits, left_justified):
    return (8 * container_bytes if left_justified else bits) - depth


def containers_of(s, depth, container_bytes, bits, left_justified):
    """samples -> the sign-extended values of their containers (int64; they fit the container as signed numbers)"""
    v = np.asarray(s, np.int64) << shift_of(depth, container_bytes, bits, left_justified)
    top = 1 << (8 * container_bytes - 1)
    assert ((v >= -top) & (v < top)).all()
    return v


def descriptor_refusal(depth, container_bytes, bits, left_justified, reserved=0):
    """what the header refuses in the descriptor's first four words (None: nothing)"""
    if container_bytes not in (2, 3, 4):
        return "container_bytes"
    if bits not in DEPTHS or bits > 8 * container_bytes:
        return "bits"
    if bits < depth:
        return "bits below D"
    if left_justified > 1:
        return "left_justified"
    if reserved != 0:
        return "reserved"
    return None


def layout_refusal(channels, total_frames, container_bytes, channel_stride, frame_stride):
    """the layout check: T = num_packets * frame_size frames of C channels (None: accepted)"""
    C, T, cs, fs = channels, total_frames, channel_stride, frame_stride
    if fs < 1 or (C > 1 and cs < 1):
        return "zero stride"
    last = (C - 1) * cs + (T - 1) * fs
    if (last + 1) * container_bytes >= 1 << 64 or cs >= 1 << 64 or fs >= 1 << 64:
        return "overflow"
    if C == 1:
        return None
    if cs >= T * fs:      # frames inner
        return None
    if fs >= C * cs:      # channels inner
        return None
    return "two samples can share a container"


def index_of(channels, total_frames, channel_stride, frame_stride):
    """container index of every (channel, frame), int64 [channels, frames]"""
    c = np.arange(channels, dtype=np.int64)[:, None]
    t = np.arange(total_frames, dtype=np.int64)[None, :]
    return c * channel_stride + t * frame_stride


def span_bytes(channels, total_frames, container_bytes, channel_stride, frame_stride):
    """bytes from the first container to the end of the last one"""
    return int(((channels - 1) * channel_stride + (total_frames - 1) * frame_stride + 1) * container_bytes)


def store(out, values, container_bytes, channel_stride, frame_stride, written=None):
    """out: uint8 array, changed in place: the containers `values` ([channels, frames], sign-extended) little-endian at their
    indices, only where `written` (bool [channels, frames], None: everywhere); no other byte changes"""
    v = np.asarray(values, np.int64)
    ch, frames = v.shape
    at = index_of(ch, frames, channel_stride, frame_stride) * container_bytes
    if written is None:
        written = np.ones(v.shape, bool)
    at, v = at[written], v[written]
    for k in range(container_bytes):
        out[at + k] = ((v >> (8 * k)) & 0xFF).astype(np.uint8)
    return out


def load(buf, channels, total_frames, container_bytes, channel_stride, frame_stride):
    """the sign-extended containers of a buffer, int64 [channels, frames] (what a reader of the layout sees)"""
    buf = np.asarray(buf, np.uint8)
    at = index_of(channels, total_frames, channel_stride, frame_stride) * container_bytes
    v = np.zeros(at.shape, np.int64)
    for k in range(container_bytes):
        v |= buf[at + k].astype(np.int64) << (8 * k)
    top = 1 << (8 * container_bytes - 1)
    return (v ^ top) - top


def decode_int(raw, depth, channels, container_bytes, bits, left_justified, channel_stride, frame_stride, out, written=None):
    """alac_hip_decode's bytes `raw` + a (legal) descriptor -> `out` (uint8, in place) as alac_hip_decode_int leaves it"""
    assert descriptor_refusal(depth, container_bytes, bits, left_justified) is None
    s = samples_of(raw, depth, channels)
    assert layout_refusal(channels, s.shape[1], container_bytes, channel_stride, frame_stride) is None
    v = containers_of(s, depth, container_bytes, bits, left_justified)
    return store(out, v, container_bytes, channel_stride, frame_stride, written)


def identity(depth, channels):
    """the descriptor that reproduces alac_hip_decode's bytes"""
    return dict(container_bytes=BPS[depth], bits=depth, left_justified=1, channel_stride=1, frame_stride=channels)
