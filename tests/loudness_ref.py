"""The loudness rule of include/alac_hip.h restated in numpy, from the header's text alone: the K-weighting coefficients, the
sequential filter (one pass over time from zero state, no chunks), the 100 ms rows, the sample peak, the gate and the channel
weights.  What tests/test_loudness_rule.py, tests/test_gpu_loudness.py and tools/loudness_timing.py compare the library with."""
import math

import numpy as np

SHELF = (1681.974450955533, 3.999843853973347, 0.7071752369554196)
HIGHPASS = (38.13547087602444, 0.5003270373238773)
# ITU-R BS.1770-4, table 1 and table 2 (48 kHz): b0, b1, b2, a1, a2
BS1770_48K = (1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
              1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621)
WEIGHTS = {1: [1], 2: [1, 1], 3: [1, 1, 1], 4: [1, 1, 1, 1], 5: [1, 1, 1, 1.41, 1.41], 6: [1, 1, 1, 1.41, 1.41, 0],
           7: [1, 1, 1, 1.41, 1.41, 1, 0], 8: [1, 1, 1, 1, 1, 1.41, 1.41, 0]}


# Not part of the rule: how alac_loudness.hip cuts a segment (loud_chunk_frames, kLoudGroup in alac_kernels.hpp), restated
# only so that the GPU tests can put their frame counts around what a wave and a scan group cover.  The results do not depend
# on it: test_row_count_equals_the_restatement pins the values the shapes were chosen for.
GROUP_CHUNKS = 256


def chunk_frames(fs):
    """the largest divisor of hop = fs // 10 that is <= 64, or where that is below 16 the smallest one >= 16"""
    hop = fs // 10
    best = max(d for d in range(1, 65) if hop % d == 0)
    return best if best >= 16 else next(d for d in range(16, hop + 1) if hop % d == 0)


def rate_ok(fs):
    return 8000 <= fs <= 384000 and fs % 10 == 0


def coefficients(fs):
    """{b0, b1, b2, a1, a2} of the shelf, then of the high-pass"""
    f0, G, Q = SHELF
    K = math.tan(math.pi * f0 / fs)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    shelf = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0,
             2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    f0, Q = HIGHPASS
    K = math.tan(math.pi * f0 / fs)
    a0 = 1.0 + K / Q + K * K
    return np.array(shelf + [1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])


def _biquad_scalar(c, x):
    b0, b1, b2, a1, a2 = c
    s1 = s2 = 0.0
    out = []
    for v in x:
        y = b0 * v + s1
        s1 = b1 * v - a1 * y + s2
        s2 = b2 * v - a2 * y
        out.append(y)
    return out


def _biquad_vector(c, x):
    b0, b1, b2, a1, a2 = c
    s1 = np.zeros(x.shape[1])
    s2 = np.zeros(x.shape[1])
    out = np.empty_like(x)
    for i in range(x.shape[0]):
        v = x[i]
        y = b0 * v + s1
        s1 = b1 * v - a1 * y + s2
        s2 = b2 * v - a2 * y
        out[i] = y
    return out


def kweight(x, fs):
    """x float64 [frames, channels] -> the filtered signal, each channel from zero state: transposed direct form II, a loop
    over time (vectorised over the channels where there are many, one Python float at a time where there are few: the same
    IEEE operations in the same order either way)"""
    x = np.asarray(x, dtype=np.float64)
    c = [float(v) for v in coefficients(fs)]
    if x.shape[1] > 4:
        return _biquad_vector(c[5:], _biquad_vector(c[:5], x))
    out = np.empty_like(x)
    for ch in range(x.shape[1]):
        out[:, ch] = _biquad_scalar(c[5:], _biquad_scalar(c[:5], x[:, ch].tolist()))
    return out


def int_samples(containers, bits, left_justified, container_bits):
    """sign-extended containers (int64 array) -> the samples s after justification and saturation"""
    v = np.asarray(containers, dtype=np.int64)
    if left_justified:
        return v >> (container_bits - bits)
    return np.clip(v, -(1 << (bits - 1)), (1 << (bits - 1)) - 1)


def int_values(containers, bits, left_justified, container_bits):
    return int_samples(containers, bits, left_justified, container_bits).astype(np.float64) * 2.0 ** -(bits - 1)


def float_values(f):
    """float32 array -> (x as float64 with the non-finite samples read as 0.0, the mask of the non-finite ones)"""
    f = np.asarray(f, dtype=np.float32)
    bad = ~np.isfinite(f)
    return np.where(bad, np.float32(0.0), f).astype(np.float64), bad


def segment_rows(x, fs):
    """x float64 [frames, channels] of ONE segment -> its rows [floor(frames / hop), channels]"""
    hop = fs // 10
    n = x.shape[0] // hop
    if n == 0:
        return np.zeros((0, x.shape[1]))
    y = kweight(x[:n * hop], fs)
    return (y * y).reshape(n, hop, x.shape[1]).sum(axis=1)


def measure(x, fs, table=None, nonfinite=None):
    """x float64 [frames, channels]; table: ascending frame indices [segments + 1] or None (all frames); nonfinite: the mask
    float_values() gave, or None.  -> (rows of all segments back to back [rows, channels], [(first_block, num_blocks, peak,
    nonfinite count)] per segment)"""
    table = [0, x.shape[0]] if table is None else [int(t) for t in table]
    rows, reports = [], []
    first = 0
    for s in range(len(table) - 1):
        seg = x[table[s]:table[s + 1]]
        e = segment_rows(seg, fs)
        bad = 0 if nonfinite is None else int(nonfinite[table[s]:table[s + 1]].sum())
        reports.append((first, e.shape[0], float(np.abs(seg).max()) if seg.size else 0.0, bad))
        rows.append(e)
        first += e.shape[0]
    return np.concatenate(rows, axis=0), reports


def loudness(p):
    return -0.691 + 10.0 * math.log10(p) if p > 0 else -math.inf


def integrated(energy, hop, weights=None):
    """energy [blocks, channels] of one segment -> LUFS, -inf where no block passes the gates or there are fewer than 4 rows"""
    e = np.asarray(energy, dtype=np.float64)
    if e.shape[0] < 4:
        return -math.inf
    G = np.asarray(WEIGHTS[e.shape[1]] if weights is None else weights, dtype=np.float64)
    power = []
    for j in range(e.shape[0] - 3):
        z = (e[j] + e[j + 1] + e[j + 2] + e[j + 3]) / (4.0 * hop)
        p = 0.0
        for c in range(e.shape[1]):
            p += G[c] * z[c]
        power.append(float(p))
    l = [loudness(p) for p in power]
    first = [p for p, v in zip(power, l) if v > -70.0]
    if not first:
        return -math.inf
    gate = loudness(math.fsum(first) / len(first)) - 10.0
    second = [p for p, v in zip(power, l) if v > -70.0 and v > gate]
    if not second:
        return -math.inf
    return loudness(math.fsum(second) / len(second))
