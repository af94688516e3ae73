"""CPU: the true-peak rule of include/alac_hip.h.  alac_hip_true_peak_filter gives the factors, tap counts and coefficients of
the restatement (tests/true_peak_ref.py); the restatement with the library's coefficients measures the true-peak signals of
EBU Tech 3341 (cases 15-19) inside the document's tolerance; the surface exists and refuses what it must without a context."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import alac_amd
import true_peak_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["alac_hip_true_peak_workspace_bytes", "alac_hip_true_peak_int", "alac_hip_true_peak_float",
         "alac_hip_true_peak_int_host", "alac_hip_true_peak_float_host", "alac_hip_true_peak_filter"]


# ---- the filter ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs,factor,taps", [(44100, 4, 12), (48000, 4, 12), (95990, 4, 12), (96000, 2, 24), (191990, 2, 24),
                                            (192000, 1, 0), (384000, 1, 0)])
def test_filter_shapes_and_coefficients(fs, factor, taps):
    f, coefs = alac_amd.true_peak_filter(fs)
    assert f == factor == tr.factor(fs)
    assert coefs.shape == (factor - 1, taps)
    want = tr.closed_form(factor)
    assert want.shape == coefs.shape
    if coefs.size:
        print(fs, "max |h - closed form|", float(np.abs(coefs - want).max()), "sum |h| per phase", np.abs(coefs).sum(axis=1))
        assert np.abs(coefs - want).max() <= 1e-15


def test_the_shapes_the_header_names():
    four, two = tr.closed_form(4), tr.closed_form(2)
    assert four.shape == (3, 12) and two.shape == (1, 24)
    assert np.allclose(np.abs(four).sum(axis=1), [1.631, 1.864, 1.631], atol=5e-4)
    assert np.allclose(np.abs(two).sum(axis=1), [2.307], atol=5e-4)
    assert np.allclose(four[0], four[2][::-1], rtol=0, atol=1e-15)  # phases 1 and 3 mirror each other


@pytest.mark.parametrize("fs", [7990, 44101])
def test_filter_refuses_other_rates(fs):
    lib = alac_amd.load_library()
    f, k = C.c_uint32(9), C.c_uint32(9)
    out = np.full(36, 7.0)
    assert lib.alac_hip_true_peak_filter(fs, C.byref(f), C.byref(k), out.ctypes.data) == -50
    assert (f.value, k.value) == (9, 9) and (out == 7.0).all()
    with pytest.raises(ValueError):
        alac_amd.true_peak_filter(fs)


def test_filter_refuses_null_pointers():
    lib = alac_amd.load_library()
    f, k = C.c_uint32(9), C.c_uint32(9)
    out = np.full(36, 7.0)
    assert lib.alac_hip_true_peak_filter(48000, None, C.byref(k), out.ctypes.data) == -50
    assert lib.alac_hip_true_peak_filter(48000, C.byref(f), None, out.ctypes.data) == -50
    assert lib.alac_hip_true_peak_filter(48000, C.byref(f), C.byref(k), None) == -50
    assert (f.value, k.value) == (9, 9) and (out == 7.0).all()


# ---- EBU Tech 3341, the true-peak signals ------------------------------------------------------------------------------------
def faded_sine(divisor, level, degrees, fs=48000):
    """one second of a sine at fs / divisor with a 0.1 s linear fade in and out (a sine switched on at full level has a real
    onset overshoot of up to 0.65 dB, which is not what the cases mean)"""
    n = np.arange(fs, dtype=np.float64)
    x = level * np.sin(2.0 * math.pi * n / divisor + math.radians(degrees))
    ramp = np.minimum(1.0, np.minimum(n, fs - 1 - n) / (0.1 * fs))
    return (x * ramp)[:, None]


TECH_3341 = {15: (4, 0.50, 0.0, -6.0), 16: (4, 0.50, 45.0, -6.0), 17: (6, 0.50, 60.0, -6.0), 18: (8, 0.50, 67.5, -6.0),
             19: (4, 1.41, 45.0, 3.0)}


@pytest.mark.parametrize("case", sorted(TECH_3341))
def test_tech_3341_true_peak_signals(case):
    divisor, level, degrees, want = TECH_3341[case]
    _, coefs = alac_amd.true_peak_filter(48000)
    x = faded_sine(divisor, level, degrees)
    peaks, reports = tr.measure(x, 48000, coefs=coefs)
    got, sample = tr.dbtp(reports[0][0]), tr.dbtp(reports[0][1])
    print("case %d: %.3f dBTP (sample peak %.2f dBFS), expected %.1f" % (case, got, sample, want))
    assert want - 0.4 <= got <= want + 0.2
    assert reports[0][0] >= reports[0][1] and peaks[0, 0] == reports[0][0]
    if case == 16:
        assert abs(sample - (-9.03)) <= 0.01  # the samples fall 45 degrees off the crests: 3 dB under the true peak


def test_the_tail_is_flushed():
    """a peak in the last frame: the largest filtered outputs lie behind the segment's end, and the true peak is never below
    the sample peak"""
    x = np.zeros((40, 1))
    x[-1, 0] = 0.125
    peaks, reports = tr.measure(x, 48000)
    assert reports[0][0] == reports[0][1] == 0.125
    x[-1, 0], x[-2, 0] = 0.5, 0.5  # two equal samples: the crest lies between them, half a frame behind the last but one
    peaks, reports = tr.measure(x, 48000)
    assert reports[0][0] > 0.6 and reports[0][1] == 0.5


# ---- the surface -------------------------------------------------------------------------------------------------------------
def test_library_exports_and_binds_the_symbols():
    lib = C.CDLL(alac_amd.LIB_PATH)
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in alac_amd.SIGNATURES, n
    alac_amd.load_library()
    for m in ("true_peak_int", "true_peak_float", "true_peak_reports"):
        assert callable(getattr(alac_amd.Context, m, None)), m
    assert callable(alac_amd.true_peak_filter)


def test_header_declares_the_calls_the_struct_and_the_rule():
    with open(os.path.join(ROOT, "include", "alac_hip.h")) as f:
        text = f.read()
    for n in NAMES:
        assert re.search(r"\b" + n + r"\s*\(", text), n
    struct = text[text.index("typedef struct alac_hip_true_peak_report {"):text.index("} alac_hip_true_peak_report;")]
    fields = re.findall(r"^\s+(uint\d+_t|double) (\w+);", struct, re.M)
    assert fields == [("double", "true_peak"), ("double", "peak"), ("uint64_t", "nonfinite"), ("uint64_t", "reserved")]
    assert C.sizeof(alac_amd.TruePeakReport) == 32
    assert [n for n, _ in alac_amd.TruePeakReport._fields_] == [n for _, n in fields]
    for line in ("F = 4 for fs < 96 000, F = 2 for 96 000 <= fs < 192 000, F = 1 from 192 000 up",
                 "h[j] = (m == 0 ? 1 : sin(m pi / F) / (m pi / F)) * 0.5 * (1 - cos(2 pi j / 48))",
                 "p = j mod F at index k = j div F", "|h[j]| < 1e-6 are dropped",
                 "y_p[n] = sum_k h_p[k] x[n - k]     for n in [0, N + K - 1)", "every step one fused multiply-add",
                 "libebur128 does not flush it", "true_peak = max(sample peak, max over p >= 1 and n of |y_p[n]|)"):
        assert line in text, line


def test_refusal_without_a_context_and_the_workspace_query():
    lib = alac_amd.load_library()
    sig = alac_amd.SIGNATURES
    assert len(sig["alac_hip_true_peak_int"][1]) == 12 and len(sig["alac_hip_true_peak_float"][1]) == 13
    assert len(sig["alac_hip_true_peak_int_host"][1]) == 10 and len(sig["alac_hip_true_peak_float_host"][1]) == 11
    src = alac_amd.IntSource(4, 24, 1, 0, 4096, 1)
    for s in (None, C.byref(src)):
        assert lib.alac_hip_true_peak_int(None, None, s, 2, 48000, 10, None, 1, None, 0, None, None) == -50
        assert lib.alac_hip_true_peak_int_host(None, None, s, 2, 48000, 10, None, 1, None, None) == -50
    assert lib.alac_hip_true_peak_float(None, None, 2, 4096, 1, 48000, 10, None, 1, None, 0, None, None) == -50
    assert lib.alac_hip_true_peak_float_host(None, None, 2, 4096, 1, 48000, 10, None, 1, None, None) == -50
    ws = lib.alac_hip_true_peak_workspace_bytes
    assert 0 < ws(2, 1) == ws(8, 1) < ws(2, 1000) and ws(2, 1000) % 256 == 0
    assert ws(2, 1000) <= 2 * 1001 * 8 + 256  # the two tables; nothing that grows with the frames
    for bad in ((0, 1), (9, 1), (2, 0)):
        assert ws(*bad) == 0, bad


def test_class_declares_loudness_true_peak_batch():
    with open(os.path.join(ROOT, "include", "alac", "ALACDecoder.h")) as f:
        text = f.read()
    assert re.search(r"LoudnessTruePeakBatch\(const uint8_t \*stream, const uint32_t \*packetBytes, uint32_t numPackets,\s+"
                     r"const uint32_t \*fileFirstPacket, uint32_t numFiles, double \*outLufs, double \*outPeak,\s+"
                     r"double \*outTruePeak, uint32_t \*outFrames, int32_t \*outStatus\)", text)
