"""CPU: the float probe's rule and surface.  The numpy restatement (float_probe_ref.py) against exact rational arithmetic
and through the quantization rule of alac_hip_encode_float; alac_hip_float_report_depth against a table of hand-made
reports; the symbols are exported, bound and declared with the rule stated; a call without a context is refused; alacconvert
names --float-bits auto."""
import ctypes
import inspect
import os
import re
import subprocess
from fractions import Fraction

import numpy as np

import alac_amd
import float_probe_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CU = os.path.join(ROOT, "convert-utility")
NAMES = ["alac_hip_float_probe_workspace_bytes", "alac_hip_float_probe", "alac_hip_float_probe_host",
         "alac_hip_float_report_depth"]
DEPTHS = (16, 20, 24, 32)


def f32(v):
    return np.float32(v)


def edge_values():
    one = f32(1.0)
    vals = [f32(0.0), f32(-0.0), one, -one, np.nextafter(one, f32(0)), -np.nextafter(one, f32(0)), np.nextafter(one, f32(2)),
            -np.nextafter(one, f32(2)), f32(0.5), f32(-0.5), f32(1.5), f32(2.0), f32(-2.0), f32(3.0), f32(1e30),
            f32(3 * 2.0 ** -20), f32(2.0 ** -126), f32(2.0 ** -127), f32(2.0 ** -149), f32(-2.0 ** -149),
            f32(3 * 2.0 ** -149), np.finfo(np.float32).max]
    vals += [f32(2.0 ** -k) for k in range(0, 33)] + [f32(-(2.0 ** -k)) for k in range(0, 33)]
    rng = np.random.default_rng(20)
    vals += list((rng.integers(-32768, 32768, 200) / 32768.0).astype(np.float32))
    vals += list((rng.integers(-(1 << 23), 1 << 23, 200) / float(1 << 23)).astype(np.float32))
    vals += list(rng.uniform(-1.0, 1.0, 200).astype(np.float32))  # off-grid
    vals += list(rng.integers(0, 1 << 32, 400, dtype=np.uint64).astype(np.uint32).view(np.float32))  # any bit pattern
    return np.array(vals, dtype=np.float32)


def test_need_against_exact_rationals():
    x = edge_values()
    x = x[np.isfinite(x)]
    n = fr.need(x)
    assert n.min() >= 0 and n.max() == 150
    for v, nb in zip(x, n):
        q = Fraction(float(v))
        for b in {0, 1, 2, 15, 16, 17, 20, 24, 32, 33, 149, 150, 151, int(nb) - 1, int(nb), int(nb) + 1}:
            if b < 0:
                continue
            whole = (q * Fraction(2) ** (b - 1)).denominator == 1
            assert whole == (nb <= b), (v, nb, b)
    known = {-1.0: 1, 1.0: 1, 0.5: 2, 2.0 ** -15: 16, 2.0 ** -16: 17, 3 * 2.0 ** -20: 21, 2.0 ** -23: 24, 2.0 ** -31: 32,
             2.0 ** -32: 33, 2.0 ** -149: 150, 0.0: 0, -0.0: 0, 2.0: 0, 1.5: 2}
    for v, nb in known.items():
        assert int(fr.need(np.array([v], dtype=np.float32))[0]) == nb, v
    assert list(fr.need(np.array([np.nan, np.inf, -np.inf], dtype=np.float32))) == [0, 0, 0]


def quantize_back(x, b):
    """alac_hip_decode_float(alac_hip_encode_float(x)) by the rules of include/alac_hip.h, in float64 (exact here)"""
    with np.errstate(invalid="ignore"):
        r = np.rint(x.astype(np.float64) * 2.0 ** (b - 1))
    s = np.where(np.isnan(r), 0.0, np.clip(r, -(2.0 ** (b - 1)), 2.0 ** (b - 1) - 1))
    return (s * 2.0 ** -(b - 1)).astype(np.float32)


def test_a_named_depth_is_lossless_and_the_smallest():
    x = edge_values()
    for v in x:
        d = fr.report_depth(fr.report([v]))
        for b in DEPTHS:
            same = bool(quantize_back(np.array([v]), b)[0] == v)  # -0.0 == +0.0: it comes back as +0.0
            if d and b >= d:
                assert same, (v, d, b)
            if -1.0 <= v < 1.0 and (d == 0 or b < d):
                assert not same, (v, d, b)  # the smallest: every depth below loses this sample
    assert fr.report_depth(fr.report(np.array([np.nan], dtype=np.float32))) == 0


def test_report_fields():
    x = np.array([[0.25, -1.0, np.nan, np.inf], [1.0, -1.5, 2.0 ** -20, -0.0]], dtype=np.float32)
    r = fr.report(x)
    assert list(r) == [3, 0, 1, 0, 21, 0x7F800000, 0, 0]  # over: inf, 1.0, -1.5
    assert list(fr.report(np.zeros((2, 0), dtype=np.float32))) == [0] * 8
    rs = fr.reports(x, [0, 1, 1, 3, 4])
    assert rs.shape == (4, 8) and list(rs[1]) == [0] * 8
    assert list(rs[0]) == [1, 0, 0, 0, 3, 0x3F800000, 0, 0]
    assert list(rs[2]) == [1, 0, 1, 0, 21, 0x3FC00000, 0, 0]


def hand_made(need=0, nan=0, over=0):
    return alac_amd.FloatReport(over, nan, need, 0, (ctypes.c_uint32 * 2)(0, 0))


def test_report_depth_table():
    lib = alac_amd.load_library()
    assert ctypes.sizeof(alac_amd.FloatReport) == 32
    table = {0: 16, 1: 16, 16: 16, 17: 20, 20: 20, 21: 24, 24: 24, 25: 32, 32: 32, 33: 0, 150: 0}
    for need, depth in table.items():
        r = hand_made(need=need)
        assert lib.alac_hip_float_report_depth(ctypes.byref(r)) == depth, need
        words = np.frombuffer(bytes(r), dtype=np.uint32)
        assert fr.report_depth(words) == depth, need
    for r in (hand_made(need=16, nan=1), hand_made(need=16, over=1), hand_made(nan=1 << 40), hand_made(over=1 << 40)):
        assert lib.alac_hip_float_report_depth(ctypes.byref(r)) == 0
        assert fr.report_depth(np.frombuffer(bytes(r), dtype=np.uint32)) == 0
    assert lib.alac_hip_float_report_depth(None) == 0


def test_library_exports_and_binds_the_probe():
    lib = ctypes.CDLL(alac_amd.LIB_PATH)
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in alac_amd.SIGNATURES, n
    assert len(alac_amd.SIGNATURES["alac_hip_float_probe"][1]) == 11
    assert len(alac_amd.SIGNATURES["alac_hip_float_probe_host"][1]) == 9
    alac_amd.load_library()
    lib = alac_amd.load_library()
    assert lib.alac_hip_float_probe_workspace_bytes(0) == 0
    for n in (1, 31, 32, 1024):
        assert lib.alac_hip_float_probe_workspace_bytes(n) >= (n + 1) * 8


def test_header_declares_the_probe_and_states_the_rule():
    with open(os.path.join(ROOT, "include", "alac_hip.h")) as f:
        text = f.read()
    for n in NAMES:
        assert re.search(r"\b" + n + r"\s*\(", text), n
    flat = " ".join(text.split()).replace(" * ", " ")
    for phrase in ("typedef struct alac_hip_float_report", "sig = M | 0x800000, lsb = E - 150", "lsb = -149",
                   "max(0, 1 - (lsb + ctz(sig)))", "x * 2^(b-1) is an integer exactly when need(x) <= b",
                   "-0.0 comes back as +0.0", "Frames outside every segment are not read",
                   "Every word is written by every call", "Read and validated before the call returns",
                   "frame_stride 0", "channel_stride 0 with more than one channel", "overflows 64 bits", "num_segments 0",
                   "not ascending or ends behind total_frames", "a workspace too small"):
        assert phrase.replace(" * ", " ") in flat, phrase  # (the comment's line starts went the same way)
    decl = flat[flat.index("int32_t alac_hip_float_probe("):]
    decl = decl[:decl.index(";")]
    order = ["ctx", "d_in", "num_channels", "channel_stride", "frame_stride", "total_frames", "h_seg_first_frame",
             "num_segments", "d_workspace", "workspace_bytes", "d_reports"]
    pos = [decl.index(a) for a in order]
    assert pos == sorted(pos)


def test_probe_without_a_context_is_a_parameter_error():
    lib = alac_amd.load_library()
    u64 = ctypes.c_uint64
    assert lib.alac_hip_float_probe(None, None, 2, u64(1), u64(1), u64(0), None, 1, None, u64(0), None) == -50
    assert lib.alac_hip_float_probe_host(None, None, 2, u64(1), u64(1), u64(0), None, 1, None) == -50


def test_context_methods():
    sig = inspect.signature(alac_amd.Context.probe_float)
    assert list(sig.parameters) == ["self", "x", "seg_first_frame"] and sig.parameters["seg_first_frame"].default is None
    sig = inspect.signature(alac_amd.Context.lossless_depth)
    assert list(sig.parameters) == ["self", "x", "seg_first_frame"] and sig.parameters["seg_first_frame"].default is None


def test_alacconvert_names_float_bits_auto():
    subprocess.check_call(["make", "-C", CU, "alacconvert"], stdout=subprocess.DEVNULL)
    binary = os.path.join(CU, "alacconvert")
    p = subprocess.run([binary, "-h"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and "--float-bits auto" in p.stdout
    # auto promises lossless: with --dither it is malformed usage, before any file is opened
    p = subprocess.run([binary, "--float-bits", "auto", "--dither", "none.wav", "none.caf"], capture_output=True, text=True,
                       timeout=60)
    assert p.returncode == 1 and "Usage" in p.stdout and "--dither needs --float-bits 16, 20 or 24" in p.stderr
    assert not os.path.exists("none.caf")
