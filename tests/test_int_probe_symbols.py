"""CPU: the integer probe surface exists — libalac_hip.so exports alac_hip_int_probe, its host form, the workspace query and
alac_hip_int_report_depth, all bound in SIGNATURES; include/alac_hip.h declares them, the report struct and the rule's lines;
the calls refuse a null context with -50 (every other refusal needs a context, hence a GPU: tests/test_gpu_int_probe.py);
alac_hip_int_report_depth is host only and equals its restatement; ALACEncoder declares ProbeInt."""
import ctypes as C
import os
import re

import numpy as np

import alac_amd
import int_probe_ref as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["alac_hip_int_probe_workspace_bytes", "alac_hip_int_probe", "alac_hip_int_probe_host", "alac_hip_int_report_depth"]


def header():
    with open(os.path.join(ROOT, "include", "alac_hip.h")) as f:
        return f.read()


def test_library_exports_and_binds_the_four_symbols():
    lib = C.CDLL(alac_amd.LIB_PATH)
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in alac_amd.SIGNATURES, n
    alac_amd.load_library()
    for m in ("probe_int", "lossless_depth_int"):
        assert callable(getattr(alac_amd.Context, m, None)), m


def test_header_declares_the_calls_the_struct_and_the_rule():
    text = header()
    for n in NAMES:
        assert re.search(r"\b" + n + r"\s*\(", text), n
    struct = text[text.index("typedef struct alac_hip_int_report {"):text.index("} alac_hip_int_report;")]
    fields = re.findall(r"^\s+(uint\d+_t) (\w+);", struct, re.M)
    assert fields == [("uint64_t", "out_of_range"), ("uint64_t", "differing_frames"), ("uint32_t", "need_bits"),
                      ("uint32_t", "peak"), ("uint32_t", "pad_bits"), ("uint32_t", "reserved")]
    assert C.sizeof(alac_amd.IntReport) == 32
    assert [(n, C.sizeof(t)) for n, t in alac_amd.IntReport._fields_] == [(n, int(t[4:-2]) // 8) for t, n in fields]
    decl = text[text.index("int32_t alac_hip_int_probe("):]
    decl = decl[:decl.index(";")]
    for arg in ("const void *d_in", "const alac_hip_int_source *src", "uint32_t num_channels", "uint64_t total_frames",
                "const uint64_t *h_seg_first_frame", "uint32_t num_segments", "void *d_workspace", "uint64_t workspace_bytes",
                "alac_hip_int_report *d_reports"):
        assert arg in decl, arg
    for line in ("c * channel_stride + t * frame_stride", "s = v >> P (arithmetic),  pad = v & (2^P - 1)",
                 "s = clamp(v, -2^(S-1), 2^(S-1) - 1),  pad = 0", "the container is out of range when v != s",
                 "S - ctz(s)", "exactly when need(s) <= b", "x = s * 2^-(S-1); s = -2^(S-1) gives 1, as -1.0 does"):
        assert line in text, line


def test_signatures_and_refusal_without_a_context():
    sig = alac_amd.SIGNATURES
    assert len(sig["alac_hip_int_probe"][1]) == 10 and len(sig["alac_hip_int_probe_host"][1]) == 8
    # alac_hip_float_probe's list with (d_in, src) for (d_in, channel_stride, frame_stride), the channel count behind them
    assert sig["alac_hip_int_probe"][1][4:] == sig["alac_hip_float_probe"][1][5:]
    assert sig["alac_hip_int_probe_host"][1][4:] == sig["alac_hip_float_probe_host"][1][5:]
    lib = alac_amd.load_library()
    src = alac_amd.IntSource(4, 24, 1, 0, 4096, 1)
    for s in (None, C.byref(src)):
        assert lib.alac_hip_int_probe(None, None, s, 2, 10, None, 1, None, 0, None) == -50
        assert lib.alac_hip_int_probe_host(None, None, s, 2, 10, None, 1, None) == -50
    for n in (0, 1, 7, 31, 32, 1000):
        assert lib.alac_hip_int_probe_workspace_bytes(n) == lib.alac_hip_float_probe_workspace_bytes(n)


def test_report_depth_is_host_only_and_equals_the_restatement():
    lib = alac_amd.load_library()
    assert lib.alac_hip_int_report_depth(None) == 0
    cases = [(0, 0, n, 0) for n in range(0, 33)] + [(1, 0, 3, 0), (1 << 32, 0, 3, 0), (0, 0, 3, 1), (0, 0, 3, 0x8000),
                                                    (0, 5, 17, 0), (0, 1 << 40, 24, 0)]
    for oor, diff, need, pad in cases:
        r = alac_amd.IntReport(oor, diff, need, 123, pad, 0)
        words = np.frombuffer(bytes(r), dtype=np.uint32)
        assert lib.alac_hip_int_report_depth(C.byref(r)) == ir.report_depth(words), (oor, diff, need, pad)
    assert lib.alac_hip_int_report_depth(C.byref(alac_amd.IntReport(0, 9, 17, 5, 0, 0))) == 20


def test_class_declares_probe_int():
    with open(os.path.join(ROOT, "include", "alac", "ALACEncoder.h")) as f:
        text = f.read()
    assert "ProbeInt(const void *pcm, const alac_hip_int_source &src, uint32_t numChannels, uint64_t totalFrames," in text
    assert "const uint64_t *segFirstFrame, uint32_t numSegments, alac_hip_int_report *reports)" in text
