"""numpy restatement of the integer probe rule of include/alac_hip.h (alac_hip_int_probe) and of alac_hip_int_report_depth,
from the header's text alone.

The source is (container_bytes, bits, left_justified), as in an alac_hip_int_source; the containers are sign-extended integers
[channels, frames].  A report is 8 uint32 words, the memory of an alac_hip_int_report: out_of_range (0-1, low word first),
differing_frames (2-3), need_bits (4), peak (5), pad_bits (6), reserved (7)."""
import numpy as np


def split(v, container_bytes, bits, left_justified):
    """sign-extended containers -> (samples s, pad bits, out-of-range mask), int64"""
    v = np.asarray(v, np.int64)
    P = 8 * container_bytes - bits
    if left_justified:
        return v >> P, v & ((1 << P) - 1), np.zeros(v.shape, bool)
    s = np.clip(v, -(1 << (bits - 1)), (1 << (bits - 1)) - 1)
    return s, np.zeros(v.shape, np.int64), v != s


def need(s, bits):
    """need(s) per element: 0 for 0, else bits - ctz(s)"""
    s = np.asarray(s, np.int64)
    low = s & -s  # lowest set bit: a power of two, its log2 is exact
    ctz = np.log2(np.maximum(low, 1)).astype(np.int64)
    return np.where(s == 0, 0, bits - ctz)


def report(v, src):
    """the report of one segment: v [channels, frames] holds its containers"""
    container_bytes, bits, left_justified = src
    v = np.asarray(v, np.int64)
    s, pad, bad = split(v, container_bytes, bits, left_justified)
    differing = int((s != s[:1]).any(axis=0).sum())
    r = np.zeros(8, dtype=np.uint32)
    r[0], r[1] = int(bad.sum()) & 0xFFFFFFFF, int(bad.sum()) >> 32
    r[2], r[3] = differing & 0xFFFFFFFF, differing >> 32
    r[4] = need(s, bits).max(initial=0)
    r[5] = np.abs(s).max(initial=0)
    r[6] = np.bitwise_or.reduce(pad.ravel()) if pad.size else 0
    return r


def reports(v, src, seg_first_frame=None):
    """[num_segments, 8] uint32: v is [channels, frames]; segment s = frames [first[s], first[s + 1]) (None: all of v)"""
    v = np.asarray(v)
    first = [0, v.shape[1]] if seg_first_frame is None else [int(f) for f in seg_first_frame]
    return np.stack([report(v[:, a:b], src) for a, b in zip(first[:-1], first[1:])])


def report_depth(r):
    """alac_hip_int_report_depth on the 8 words of a report"""
    r = np.asarray(r).view(np.uint32) if np.asarray(r).dtype == np.int32 else np.asarray(r, dtype=np.uint32)
    if r[0] or r[1] or r[6]:
        return 0
    return 16 if r[4] <= 16 else 20 if r[4] <= 20 else 24 if r[4] <= 24 else 32
