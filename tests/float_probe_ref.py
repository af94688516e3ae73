"""numpy restatement of the probe rule of include/alac_hip.h (alac_hip_float_probe) and of alac_hip_float_report_depth.

A report is 8 uint32 words, the memory of an alac_hip_float_report: over_range (0-1, low word first), nan (2-3), need_bits
(4), peak_bits (5), reserved (6-7)."""
import numpy as np


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def need(x):
    """need(x) per element of a float32 array (int64); 0 for the zeros, and for NaN and the infinities (which are no
    finite samples)"""
    u = bits(x).astype(np.int64)
    E, M = (u >> 23) & 0xFF, u & 0x7FFFFF
    sig = np.where(E == 0, M, M | 0x800000)
    lsb = np.where(E == 0, -149, E - 150)
    low = sig & -sig  # lowest set bit: a power of two, its log2 is exact
    ctz = np.log2(np.maximum(low, 1)).astype(np.int64)
    return np.where((sig == 0) | (E == 255), 0, np.maximum(0, 1 - (lsb + ctz)))


def report(x):
    """the report of one segment: x holds its samples, every channel, in any shape"""
    u = bits(np.asarray(x, dtype=np.float32).ravel())
    mag = u & np.uint32(0x7FFFFFFF)
    nan = mag > 0x7F800000
    over = ~nan & ((mag > 0x3F800000) | (u == 0x3F800000))  # x >= 1.0 or x < -1.0, infinities included
    finite = mag < 0x7F800000
    r = np.zeros(8, dtype=np.uint32)
    r[0], r[1] = int(over.sum()) & 0xFFFFFFFF, int(over.sum()) >> 32
    r[2], r[3] = int(nan.sum()) & 0xFFFFFFFF, int(nan.sum()) >> 32
    r[4] = need(u.view(np.float32))[finite].max(initial=0)
    r[5] = mag[~nan].max(initial=0)
    return r


def reports(x, seg_first_frame=None):
    """[num_segments, 8] uint32: x is [channels, frames]; segment s = frames [first[s], first[s + 1]) (None: all of x)"""
    x = np.asarray(x)
    first = [0, x.shape[1]] if seg_first_frame is None else [int(f) for f in seg_first_frame]
    return np.stack([report(x[:, a:b]) for a, b in zip(first[:-1], first[1:])])


def report_depth(r):
    """alac_hip_float_report_depth on the 8 words of a report"""
    r = np.asarray(r).view(np.uint32) if np.asarray(r).dtype == np.int32 else np.asarray(r, dtype=np.uint32)
    if r[0] or r[1] or r[2] or r[3] or r[4] > 32:
        return 0
    return 16 if r[4] <= 16 else 20 if r[4] <= 20 else 24 if r[4] <= 24 else 32
