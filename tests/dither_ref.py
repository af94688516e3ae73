"""The TPDF dither rule of include/alac_hip.h (alac_hip_encode_float_dither) restated in numpy, from the header's text alone:
Philox4x32-10 keyed by the seed, counted by (frame index >> 1, channel); the triangular integer k; the one float32 rounding
of x * 2^(b-1) + d; then the quantization rule of alac_hip_encode_float.  No library and no GPU needed."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57  # Philox4x32 multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85  # key increments (golden ratio, sqrt(3) - 1)
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: four uint64 arrays (or ints) holding 32-bit words, key: two 32-bit ints -> four uint64 arrays of 32-bit words"""
    c = [np.asarray(v, np.uint64) & MASK for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]  # 32 x 32 -> 64 bits: exact in uint64
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def dither_k(seed, channel, t):
    """the integer k of the rule (int64, -(2^24 - 1) .. 2^24 - 1) for seed, channel (broadcastable) and frame indices t"""
    t = np.asarray(t, np.uint64)
    ch = np.asarray(channel, np.uint64)
    t, ch = np.broadcast_arrays(t, ch)
    big = t >> np.uint64(1)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w = philox4x32_10((big & MASK, big >> np.uint64(32), ch, 0), (seed & 0xFFFFFFFF, seed >> 32))
    odd = (t & np.uint64(1)) == 1
    wa = np.where(odd, w[2], w[0])
    wb = np.where(odd, w[3], w[1])
    return (wa >> np.uint64(8)).astype(np.int64) - (wb >> np.uint64(8)).astype(np.int64)


def dither(seed, channel, t):
    """d of the rule as float32: k * 2^-24, exact"""
    return (dither_k(seed, channel, t).astype(np.float64) * 2.0 ** -24).astype(np.float32)


def quantize_dithered(x, depth, seed, origin=0, channels=None):
    """x: float32 [C, frames], frame i of the array being stream frame origin + i (origin an int, or a uint64 array [frames]
    of every frame's own index); channels: the channel index of every row (default 0 .. C-1).
    -> (int64 samples, clipped mask), by the rule: v = float32(float64(x) * 2^(b-1) + d), r = rint(v), saturate, NaN -> 0"""
    assert depth in (16, 20, 24)
    x = np.asarray(x, np.float32)
    ch, frames = x.shape
    t = np.asarray(origin, np.uint64) + np.arange(frames, dtype=np.uint64) if np.ndim(origin) == 0 else np.asarray(origin, np.uint64)
    rows = np.arange(ch) if channels is None else np.asarray(channels)
    d = dither(seed, rows[:, None], t[None, :])
    top = 2 ** (depth - 1)
    with np.errstate(invalid="ignore", over="ignore"):
        v = (x.astype(np.float64) * float(top) + d.astype(np.float64)).astype(np.float32)
        r = np.rint(v.astype(np.float64))
        nan = np.isnan(x)
        hi, lo = r > top - 1, r < -top
        s = np.where(nan, 0, np.clip(np.nan_to_num(r, nan=0.0, posinf=top, neginf=-top - 1), -top, top - 1))
    return s.astype(np.int64), nan | hi | lo


def packet_frames(num_packets, frame_size, origin=None):
    """stream frame index of every staged frame of a call: origin[p] + i (origin None: p * frame_size) -> uint64 [frames]"""
    first = (np.arange(num_packets, dtype=np.uint64) * np.uint64(frame_size) if origin is None
             else np.asarray(origin, np.uint64))
    return (first[:, None] + np.arange(frame_size, dtype=np.uint64)[None, :]).reshape(-1)
