"""CPU: the sample-rate conversion rule of include/alac_hip.h.  alac_hip_resample_filter gives the plan and the coefficients of
the restatement (tests/resample_ref.py); alac_hip_resample_frames gives ceil(N L / M) per segment; the restatement agrees with
scipy.signal.resample_poly where scipy is present; the library's coefficients have the response DESIGN.md section 27 records;
the surface exists and refuses what it must without a context."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import alac_amd
import resample_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["alac_hip_resample_filter", "alac_hip_resample_frames", "alac_hip_resample_workspace_bytes", "alac_hip_resample_int",
         "alac_hip_resample_float", "alac_hip_resample_int_host", "alac_hip_resample_float_host"]

# (in_rate, out_rate): L / M = 160/147, 147/160, 2/1, 1/2, 1/4, 147/320, 147/640, 441/80, 640/147
PAIRS = [(44100, 48000), (48000, 44100), (48000, 96000), (96000, 48000), (192000, 48000), (96000, 44100), (192000, 44100),
         (8000, 44100), (44100, 192000)]
RATIOS = [(160, 147), (147, 160), (2, 1), (1, 2), (1, 4), (147, 320), (147, 640), (441, 80), (640, 147)]
TAPS = {(160, 147): 80, (2, 1): 80, (441, 80): 80, (640, 147): 80, (147, 160): 88, (1, 2): 160, (1, 4): 320, (147, 320): 176,
        (147, 640): 350}


# ---- the plan and the filter ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair,ratio", list(zip(PAIRS, RATIOS)))
def test_filter_plan_and_coefficients(pair, ratio):
    L, M, coefs = alac_amd.resample_filter(*pair)
    assert (L, M) == ratio
    assert rr.plan(*pair) == (L, M, coefs.shape[1]) and coefs.shape == (L, TAPS[ratio])
    want = rr.closed_form(L, M, coefs.shape[1])
    print(pair, "max |h - closed form|", float(np.abs(coefs - want).max()), "max_p sum |h|", float(np.abs(coefs).sum(axis=1).max()))
    assert np.abs(coefs - want).max() <= 2.0 ** -40
    assert coefs[0, 0] != 0.0  # the tap at t = -K/2: the window is not zero there, and the tap is kept


def test_filter_size_query():
    lib = alac_amd.load_library()
    L, M, K = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    assert lib.alac_hip_resample_filter(96000, 44100, C.byref(L), C.byref(M), C.byref(K), None) == 0
    assert (L.value, M.value, K.value) == (147, 320, 176)
    assert lib.alac_hip_resample_filter(192000, 44100, C.byref(L), C.byref(M), C.byref(K), None) == 0
    assert (L.value, M.value, K.value) == (147, 640, 350)
    out = np.full(147 * 350 + 1, 7.0)
    assert lib.alac_hip_resample_filter(192000, 44100, C.byref(L), C.byref(M), C.byref(K), out.ctypes.data) == 0
    assert out[-1] == 7.0 and (out[:-1] != 7.0).all()
    for null in range(3):
        ptrs = [C.byref(L), C.byref(M), C.byref(K)]
        ptrs[null] = None
        assert lib.alac_hip_resample_filter(192000, 44100, *ptrs, None) == -50


BAD_PAIRS = [(44101, 48000), (48000, 44105), (7990, 48000), (48000, 384010), (48000, 48000), (22050, 384000), (384000, 11030),
             (0, 48000)]


@pytest.mark.parametrize("pair", BAD_PAIRS)
def test_every_refusal_of_the_rate_pair(pair):
    """not a multiple of 10, out of range, equal rates, L or M above 640"""
    lib = alac_amd.load_library()
    assert rr.plan(*pair) is None
    L, M, K = C.c_uint32(9), C.c_uint32(9), C.c_uint32(9)
    out = np.full(64, 7.0)
    assert lib.alac_hip_resample_filter(pair[0], pair[1], C.byref(L), C.byref(M), C.byref(K), out.ctypes.data) == -50
    assert (L.value, M.value, K.value) == (9, 9, 9) and (out == 7.0).all()
    with pytest.raises(ValueError):
        alac_amd.resample_filter(*pair)
    first = np.full(2, 7, dtype=np.uint64)
    assert lib.alac_hip_resample_frames(pair[0], pair[1], 1000, None, 1, first.ctypes.data) == 0
    assert (first == 7).all()
    assert lib.alac_hip_resample_workspace_bytes(pair[0], pair[1], 2, 1) == 0


# ---- the frame counts --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", [(44100, 48000), (48000, 44100), (192000, 44100), (8000, 44100)])
def test_frames_are_ceil_n_l_over_m(pair):
    L, M, _ = rr.plan(*pair)
    for n in (0, 1, 146, 147, 148, 10 ** 12 + 7):
        total, first = alac_amd.resample_frames(pair[0], pair[1], n)
        assert total == -(-n * L // M) == rr.out_frames(n, L, M) and list(first) == [0, total]
    table = [5, 5, 6, 152, 299, 299, 447, 1000]
    total, first = alac_amd.resample_frames(pair[0], pair[1], 1000, table)
    want = rr.out_table(table, L, M)
    assert list(first) == want and total == want[-1]
    assert want[1] == 0 and want[2] == -(-L // M)  # an empty segment, and one of 1 frame


def test_frames_refuses_bad_tables():
    lib = alac_amd.load_library()
    first = np.full(4, 7, dtype=np.uint64)
    for table, total, nseg in (([0, 10, 5, 20], 20, 3), ([0, 10, 20, 30], 29, 3), ([0, 10], 20, 0)):
        t = np.array(table, dtype=np.uint64)
        assert lib.alac_hip_resample_frames(44100, 48000, total, t.ctypes.data, nseg, first.ctypes.data) == 0
        assert (first == 7).all()
    assert lib.alac_hip_resample_frames(44100, 48000, 20, None, 2, first.ctypes.data) == 0 and (first == 7).all()
    assert lib.alac_hip_resample_frames(44100, 48000, 147, None, 1, None) == 160


# ---- the restatement against scipy -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair,ratio", list(zip(PAIRS, RATIOS)))
def test_restatement_agrees_with_resample_poly(pair, ratio):
    signal = pytest.importorskip("scipy.signal")
    L, M, K = rr.plan(*pair)
    coefs = rr.closed_form(L, M, K)
    # the prototype proto[p + k L] = h_p[k], divided by L (resample_poly scales its window by L), one zero appended: odd
    # length, centred at (K/2) L
    window = np.concatenate([coefs.T.reshape(-1) / L, [0.0]])
    x = np.random.default_rng(20 + L + M).standard_normal(3001)
    want = signal.resample_poly(x, L, M, window=window)
    got = rr.segment(x[:, None], L, M, coefs)[:, 0]
    assert got.shape == want.shape
    err = float(np.abs(got - want).max())
    print(ratio, "max |restatement - resample_poly|", err)
    assert err <= 1e-12 * float(np.abs(x).max())


# ---- the response of the library's coefficients ----------------------------------------------------------------------------
@pytest.mark.parametrize("pair,ratio", list(zip(PAIRS, RATIOS)))
def test_response_of_the_coefficients(pair, ratio):
    L, M, coefs = alac_amd.resample_filter(*pair)
    dev, worst, nyq, phase = rr.measure_response(coefs, L, M)
    print("%d/%d: passband %.6f dB, folding %.2f dB, at Nyquist %.2f dB, phase sums within %.2e, max_p sum |h| %.3f"
          % (L, M, dev, worst, nyq, phase, float(np.abs(coefs).sum(axis=1).max())))
    assert dev <= 0.001
    assert worst <= -99.0
    assert phase <= 1e-5
    assert abs(nyq + 6.0) <= 0.1


# ---- the surface -------------------------------------------------------------------------------------------------------------
def test_library_exports_and_binds_the_symbols():
    lib = C.CDLL(alac_amd.LIB_PATH)
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in alac_amd.SIGNATURES, n
    alac_amd.load_library()
    for m in ("resample_int", "resample_float", "resample_reports"):
        assert callable(getattr(alac_amd.Context, m, None)), m
    assert callable(alac_amd.resample_filter) and callable(alac_amd.resample_frames)


def test_header_declares_the_calls_the_struct_and_the_rule():
    with open(os.path.join(ROOT, "include", "alac_hip.h")) as f:
        text = f.read()
    for n in NAMES:
        assert re.search(r"\b" + n + r"\s*\(", text), n
    struct = text[text.index("typedef struct alac_hip_resample_report {"):text.index("} alac_hip_resample_report;")]
    fields = re.findall(r"^\s+(uint\d+_t|double) (\w+);", struct, re.M)
    assert fields == [("uint64_t", "out_first"), ("uint64_t", "out_frames"), ("double", "peak"), ("uint64_t", "nonfinite")]
    assert C.sizeof(alac_amd.ResampleReport) == 32
    assert [n for n, _ in alac_amd.ResampleReport._fields_] == [n for _, n in fields]
    for line in ("L = out_rate / g and M = in_rate / g; both must be at most 640", "K = 2 * ceil(Z * max(L, M) / L)",
                 "h_p[k] = c * sinc(c t) * I0(beta * sqrt(max(0, 1 - (2 t / K)^2))) / I0(beta)",
                 "n0 = (m * M) div L and p = (m * M) mod L", "y[m] = (float)( sum_{k = 0}^{K - 1} h_p[k] * x[n0 + K/2 - k] )",
                 "every step one fused multiply-add", "that tap is kept"):
        assert line in text, line


def test_refusal_without_a_context_and_the_workspace_query():
    lib = alac_amd.load_library()
    sig = alac_amd.SIGNATURES
    assert len(sig["alac_hip_resample_int"][1]) == 15 and len(sig["alac_hip_resample_float"][1]) == 16
    assert len(sig["alac_hip_resample_int_host"][1]) == 13 and len(sig["alac_hip_resample_float_host"][1]) == 14
    src = alac_amd.IntSource(4, 24, 1, 0, 4096, 1)
    for s in (None, C.byref(src)):
        assert lib.alac_hip_resample_int(None, None, s, 2, 44100, 48000, 10, None, 1, None, 0, None, 0, 0, None) == -50
        assert lib.alac_hip_resample_int_host(None, None, s, 2, 44100, 48000, 10, None, 1, None, 0, 0, None) == -50
    assert lib.alac_hip_resample_float(None, None, 2, 4096, 1, 44100, 48000, 10, None, 1, None, 0, None, 0, 0, None) == -50
    assert lib.alac_hip_resample_float_host(None, None, 2, 4096, 1, 44100, 48000, 10, None, 1, None, 0, 0, None) == -50
    ws = lib.alac_hip_resample_workspace_bytes
    assert 0 < ws(44100, 48000, 2, 1) == ws(44100, 48000, 8, 1) < ws(44100, 48000, 2, 1000)
    assert ws(44100, 48000, 2, 1000) % 256 == 0
    # the coefficient table and the segment tables; nothing that grows with the frames
    assert 160 * 80 * 8 <= ws(44100, 48000, 2, 1) <= 160 * 80 * 8 + 512
    assert ws(44100, 48000, 2, 1000) <= 160 * 80 * 8 + 3 * 1001 * 8 + 512
    for bad in ((44100, 48000, 0, 1), (44100, 48000, 9, 1), (44100, 48000, 2, 0), (44100, 44100, 2, 1)):
        assert ws(*bad) == 0, bad
