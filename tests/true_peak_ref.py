"""The true-peak rule of include/alac_hip.h restated in numpy, from the header's text alone: the oversampling factor, the closed
form of the 49-tap Hann-windowed sinc cut into phases, one full-mode np.convolve per phase (both ends zero-extended) and the
maxima.  What tests/test_true_peak_rule.py, tests/test_gpu_true_peak.py, tests/test_gpu_alacconvert_true_peak.py and
tools/true_peak_timing.py compare the library with."""
import math

import numpy as np


def factor(fs):
    return 4 if fs < 96000 else 2 if fs < 192000 else 1


def closed_form(F):
    """phases 1 .. F-1 of h[j] = sinc(m pi / F) * hann(j), j = 0..48, m = j - 24: [F - 1, taps]; tap j is index j div F of
    phase j mod F, and taps below 1e-6 are dropped (all of them lie in phase 0, whose one tap 1.0 is the sample itself)"""
    h = []
    for j in range(49):
        m = j - 24
        s = 1.0 if m == 0 else math.sin(m * math.pi / F) / (m * math.pi / F)
        h.append(s * 0.5 * (1.0 - math.cos(2.0 * math.pi * j / 48)))
    phases = []
    for p in range(F):
        taps = [(j // F, h[j]) for j in range(p, 49, F) if abs(h[j]) >= 1e-6]
        if p == 0:
            assert taps == [(24 // F, 1.0)], taps
            continue
        assert [k for k, _ in taps] == list(range(len(taps))), (F, p)
        phases.append([v for _, v in taps])
    return np.array(phases, dtype=np.float64).reshape(F - 1, -1 if F > 1 else 0)


def segment_peaks(x, coefs):
    """x float64 [frames, channels] of ONE segment; coefs [F - 1, taps] -> (true peak per channel, sample peak per channel)"""
    channels = x.shape[1]
    sample = np.abs(x).max(axis=0) if x.shape[0] else np.zeros(channels)
    true = sample.copy()
    if x.shape[0]:
        for c in range(channels):
            for h in coefs:
                true[c] = max(true[c], float(np.abs(np.convolve(x[:, c], h, mode="full")).max()))
    return true, sample


def measure(x, fs, table=None, nonfinite=None, coefs=None):
    """x float64 [frames, channels]; table: ascending frame indices [segments + 1] or None (all frames); nonfinite: the mask
    loudness_ref.float_values() gave, or None; coefs: the filter to use (None: the closed form).
    -> (true peak [segments, channels], [(true peak, sample peak, nonfinite count)] per segment)"""
    coefs = closed_form(factor(fs)) if coefs is None else np.asarray(coefs, dtype=np.float64)
    table = [0, x.shape[0]] if table is None else [int(t) for t in table]
    peaks, reports = [], []
    for s in range(len(table) - 1):
        true, sample = segment_peaks(x[table[s]:table[s + 1]], coefs)
        bad = 0 if nonfinite is None else int(nonfinite[table[s]:table[s + 1]].sum())
        peaks.append(true)
        reports.append((float(true.max()), float(sample.max()), bad))
    return np.array(peaks).reshape(len(table) - 1, x.shape[1]), reports


def bound(coefs, sample_peak):
    """what fusing and the order of the sums may move an output by: taps * 2^-52 * sum |h_p[k]| * sample peak, of the phase
    where that is largest (0 where nothing is filtered)"""
    coefs = np.asarray(coefs, dtype=np.float64)
    if coefs.size == 0:
        return 0.0 * np.asarray(sample_peak, dtype=np.float64)
    return coefs.shape[1] * 2.0 ** -52 * float(np.abs(coefs).sum(axis=1).max()) * np.asarray(sample_peak, dtype=np.float64)


def dbtp(v):
    return 20.0 * math.log10(v) if v > 0 else -math.inf
