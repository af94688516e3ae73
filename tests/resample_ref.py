"""The sample-rate conversion rule of include/alac_hip.h restated in numpy, from the header's text alone: the plan of a rate pair,
the closed form of the Kaiser-windowed sinc with np.i0, and the segment loop (both ends zero-extended, no delay).  What
tests/test_resample_rule.py, tests/test_gpu_resample.py and tools/resample_timing.py compare the library with."""
import math

import numpy as np

Z, BETA = 40, 10.0


def plan(in_rate, out_rate):
    """(L, M, K) of a rate pair, or None where the calls refuse it"""
    for r in (in_rate, out_rate):
        if r % 10 or not 8000 <= r <= 384000:
            return None
    if in_rate == out_rate:
        return None
    g = math.gcd(in_rate, out_rate)
    L, M = out_rate // g, in_rate // g
    if L > 640 or M > 640:
        return None
    return L, M, 2 * -(-Z * max(L, M) // L)


def closed_form(L, M, K):
    """h_p[k] = c sinc(c t) I0(beta sqrt(max(0, 1 - (2 t / K)^2))) / I0(beta), t = p / L + k - K / 2, c = min(L, M) / M: [L, K]"""
    c = min(L, M) / M
    t = np.arange(L, dtype=np.float64)[:, None] / L + np.arange(K, dtype=np.float64)[None, :] - K // 2
    w = np.i0(BETA * np.sqrt(np.maximum(0.0, 1.0 - (2.0 * t / K) ** 2))) / np.i0(BETA)
    return c * np.sinc(c * t) * w  # np.sinc(u) = sin(pi u) / (pi u), 1 at 0


def out_frames(n, L, M):
    return -(-n * L // M)


def out_table(table, L, M):
    """every segment's first output frame and the total: [segments + 1]"""
    out = [0]
    for s in range(len(table) - 1):
        out.append(out[-1] + out_frames(int(table[s + 1]) - int(table[s]), L, M))
    return out


def segment(x, L, M, coefs):
    """x float64 [frames, channels] of ONE segment -> the sums in double, before the rounding to float32: [ceil(N L / M),
    channels].  y[m] = sum_k h_p[k] x[n0 + K/2 - k], n0 = m M div L, p = m M mod L, x = 0 outside the segment."""
    coefs = np.asarray(coefs, dtype=np.float64)
    K, n = coefs.shape[1], x.shape[0]
    outs = out_frames(n, L, M)
    y = np.zeros((outs, x.shape[1]), dtype=np.float64)
    if outs == 0:
        return y
    half = K // 2
    # position i of xp is frame i - half of the segment: frames [-half, n + half] exist, zeros outside [0, n)
    xp = np.zeros((n + 2 * half + 1, x.shape[1]), dtype=np.float64)
    xp[half:half + n] = x
    k = np.arange(K, dtype=np.int64)
    for a in range(0, outs, 4096):
        m = np.arange(a, min(outs, a + 4096), dtype=np.int64)
        n0, p = m * M // L, m * M % L
        idx = n0[:, None] + half - k[None, :] + half  # [outputs, K]
        y[m] = np.einsum("ok,okc->oc", coefs[p], xp[idx])
    return y


def resample(x, L, M, coefs, table=None):
    """x float64 [frames, channels]; table: ascending frame indices [segments + 1] or None (all frames) -> the sums of all
    segments back to back, float64 [out_total, channels]"""
    table = [0, x.shape[0]] if table is None else [int(t) for t in table]
    parts = [segment(x[table[s]:table[s + 1]], L, M, coefs) for s in range(len(table) - 1)]
    return np.concatenate(parts, axis=0) if parts else np.zeros((0, x.shape[1]))


def bound(coefs, peak):
    """what fusing and the order of the sums may move a double sum by: K * 2^-52 * max_p sum_k |h_p[k]| * peak"""
    coefs = np.asarray(coefs, dtype=np.float64)
    return coefs.shape[1] * 2.0 ** -52 * float(np.abs(coefs).sum(axis=1).max()) * float(peak)


def float32_spacing(v):
    """the distance between neighbouring float32 values at the magnitude v (float64 array)"""
    _, e = np.frexp(np.asarray(v, dtype=np.float64))  # |v| = f * 2^e, f in [0.5, 1)
    return np.ldexp(1.0, np.maximum(e - 24, -149))


def accepted(ref, bnd):
    """the accepted distance of a device float32 from the reference's double: a correctly rounded float of a sum inside the
    bound, and nothing looser: bound + half the float32 spacing at |ref| + bound"""
    ref = np.asarray(ref, dtype=np.float64)
    return bnd + 0.5 * float32_spacing(np.abs(ref) + bnd)


def response(coefs, L, M, nfft=1 << 21):
    """the prototype proto[p + k L] = h_p[k] at the rate L * in_rate, its gain relative to L on nfft / 2 + 1 frequencies from
    0 to half that rate -> (frequencies in units of the LOWER of the two rates' Nyquist, gain)"""
    coefs = np.asarray(coefs, dtype=np.float64)
    proto = coefs.T.reshape(-1)  # [K, L] flattened: index k L + p
    gain = np.abs(np.fft.rfft(proto, nfft)) / L
    f = np.arange(nfft // 2 + 1, dtype=np.float64) / nfft  # cycles per prototype sample; the input rate is 1 / L, the output 1 / M
    nyq = 0.5 / max(L, M)
    return f / nyq, gain


def measure_response(coefs, L, M, edge=0.907):
    """(largest passband deviation in dB up to `edge` of the lower Nyquist, largest gain in dB among the frequencies whose
    alias at the output rate lies at or below `edge` of it, the passband itself left out, gain in dB at the lower Nyquist,
    largest |sum_k h_p[k] - 1| over the phases)"""
    f, gain = response(coefs, L, M)
    passband = f <= edge
    dev = float(np.abs(20.0 * np.log10(gain[passband])).max())
    # the output rate in units of the lower Nyquist: 2 max(L, M) / M; the alias of f there
    fs_out = 2.0 * max(L, M) / M
    alias = np.abs(f - np.round(f / fs_out) * fs_out)
    stop = (alias <= edge) & ~passband
    # going up, the images of the input's band around multiples of the input rate must go as well
    fs_in = 2.0 * max(L, M) / L
    image = np.abs(f - np.round(f / fs_in) * fs_in)
    stop |= (image <= edge) & ~passband
    worst = float(20.0 * np.log10(max(gain[stop].max(), 1e-300))) if stop.any() else -math.inf
    at_nyquist = float(20.0 * np.log10(gain[np.argmin(np.abs(f - 1.0))]))
    phase = float(np.abs(np.asarray(coefs).sum(axis=1) - 1.0).max())
    return dev, worst, at_nyquist, phase


def quantize(y, depth):
    """the quantization rule of alac_hip_encode_float (include/alac_hip.h) on float32 values: rint(x * 2^(depth - 1)) with ties
    to even, saturated to the depth's range"""
    v = np.rint(np.asarray(y, dtype=np.float32).astype(np.float64) * 2.0 ** (depth - 1))
    return np.clip(v, -(2.0 ** (depth - 1)), 2.0 ** (depth - 1) - 1).astype(np.int64)


def near_boundary(ref, bnd, depth):
    """the samples of the reference's sums that lie within the accepted distance of a rounding boundary of the quantization
    to `depth` bits (a half-integer of x * 2^(depth - 1)): where a device float inside the accepted distance may quantize to
    the neighbouring value"""
    ref = np.asarray(ref, dtype=np.float64)
    scaled = ref * 2.0 ** (depth - 1)
    dist = np.abs(scaled - np.floor(scaled) - 0.5)  # to the nearest half-integer
    return dist <= accepted(ref, bnd) * 2.0 ** (depth - 1)
