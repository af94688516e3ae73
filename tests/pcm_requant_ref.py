"""The integer rule of include/alac_hip.h (alac_hip_pcm_requantize / alac_hip_encode_int) restated in numpy, from the header's
text alone: the sample out of its container, exact widening, reduction by round half to even of (s * 2^(24 - D) + k) / 2^24
in 64-bit integers with the k of the dither rule (dither_ref.dither_k), the clamp and the clipped flag; and the packing of
the result into the PCM alac_hip_encode reads.  No library and no GPU needed."""
import numpy as np

from dither_ref import dither_k

DEPTHS = (16, 20, 24, 32)
REDUCING = [(S, b) for S in DEPTHS for b in DEPTHS if b < S]  # six pairs
WIDENING = [(S, b) for S in DEPTHS for b in DEPTHS if b > S]  # six pairs


def sample_of(container, bits, container_bytes, left_justified):
    """the sign-extended containers (any int array) -> (int64 samples s, mask of containers that were out of range)"""
    v = np.asarray(container, np.int64)
    if left_justified:
        return v >> (8 * container_bytes - bits), np.zeros(v.shape, bool)
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    return np.clip(v, lo, hi), (v < lo) | (v > hi)


def requantize(s, bits, depth, k=None):
    """samples s of `bits` significant bits -> (int64 samples at `depth` bits, clipped mask); k: the dither integers or None"""
    s = np.asarray(s, np.int64)
    if depth >= bits:
        assert k is None, "nothing is rounded: dither is refused"
        return s << (depth - bits), np.zeros(s.shape, bool)
    D = bits - depth
    acc = s * (1 << (24 - D)) + (0 if k is None else np.asarray(k, np.int64))
    q, rem = acc >> 24, acc & ((1 << 24) - 1)
    r = q + ((rem > (1 << 23)) | ((rem == (1 << 23)) & ((q & 1) == 1)))
    lo, hi = -(1 << (depth - 1)), (1 << (depth - 1)) - 1
    return np.clip(r, lo, hi), (r < lo) | (r > hi)


def convert(containers, bits, container_bytes, left_justified, depth, frame_size, num_samples=None, seed=None, origin=None):
    """containers: int array [C, frames] of sign-extended containers, frames = num_packets * frame_size.  num_samples: the
    frames of every packet (None: all); frames behind them are staged as zero with no dither and are not clipped.  seed: TPDF
    dither with that seed (None: none), origin: every packet's first stream frame (None: p * frame_size).
    -> (int64 samples [C, frames], clipped mask [C, frames])"""
    v = np.asarray(containers, np.int64)
    ch, frames = v.shape
    npk = frames // frame_size
    assert npk * frame_size == frames
    live = np.ones(frames, bool)
    if num_samples is not None:
        i = np.arange(frames) % frame_size
        live = i < np.repeat(np.minimum(np.asarray(num_samples, np.int64), frame_size), frame_size)
    v = np.where(live[None, :], v, 0)
    s, bad = sample_of(v, bits, container_bytes, left_justified)
    k = None
    if seed is not None:
        first = np.arange(npk, dtype=np.uint64) * np.uint64(frame_size) if origin is None else np.asarray(origin, np.uint64)
        t = (first[:, None] + np.arange(frame_size, dtype=np.uint64)[None, :]).reshape(-1)
        k = np.where(live[None, :], dither_k(seed, np.arange(ch)[:, None], t[None, :]), 0)
    out, clipped = requantize(s, bits, depth, k)
    return out, (bad | clipped) & live[None, :]


def pack(s, depth):
    """int samples [C, frames] -> the packed little-endian interleaved PCM (20 bits: left-justified in 3 bytes)"""
    v = np.ascontiguousarray(np.asarray(s, np.int64).T).reshape(-1)
    if depth == 16:
        return v.astype("<i2").view(np.uint8).copy()
    if depth == 32:
        return v.astype("<i4").view(np.uint8).copy()
    c = (v << 4 if depth == 20 else v) & 0xFFFFFF
    out = np.empty((v.size, 3), np.uint8)
    out[:, 0], out[:, 1], out[:, 2] = c & 0xFF, (c >> 8) & 0xFF, (c >> 16) & 0xFF
    return out.reshape(-1)


def pack3(v):
    """sign-extended containers (flat int array) -> packed little-endian 3-byte containers, uint8"""
    c = np.asarray(v, np.int64).reshape(-1) & 0xFFFFFF
    out = np.empty((c.size, 3), np.uint8)
    out[:, 0], out[:, 1], out[:, 2] = c & 0xFF, (c >> 8) & 0xFF, (c >> 16) & 0xFF
    return out.reshape(-1)


def edge_samples(bits, depth):
    """what a test input must hold besides random samples: both extremes and, where the depth is reduced, ties (odd
    multiples of 2^(D-1)) around zero and at both ends, the top one of which clips"""
    top = 1 << (bits - 1)
    v = [top - 1, -top, 0, -1, 1]
    if depth < bits:
        h = 1 << (bits - depth - 1)
        v += [m * h for m in range(-9, 10)] + [top - m * h for m in range(1, 6)] + [-top + m * h for m in range(0, 6)]
        v += [m * h + d for m in (-3, 3, 5) for d in (-1, 1)]
    return np.array(v, np.int64)
