"""CPU: the loudness surface exists — libalac_hip.so exports alac_hip_loudness_int, alac_hip_loudness_float, their host forms,
the workspace query and the three host-only helpers, all bound in SIGNATURES; include/alac_hip.h declares them, the report
struct and the rule's lines; the calls refuse a null context with -50 (every other refusal needs a context, hence a GPU:
tests/test_gpu_loudness.py); the workspace grows with the frames and is 0 for what the calls refuse; ALACDecoder declares
LoudnessBatch."""
import ctypes as C
import os
import re

import alac_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["alac_hip_loudness_workspace_bytes", "alac_hip_loudness_int", "alac_hip_loudness_float", "alac_hip_loudness_int_host",
         "alac_hip_loudness_float_host", "alac_hip_loudness_filter", "alac_hip_loudness_rows", "alac_hip_loudness_integrated"]


def header():
    with open(os.path.join(ROOT, "include", "alac_hip.h")) as f:
        return f.read()


def test_library_exports_and_binds_the_symbols():
    lib = C.CDLL(alac_amd.LIB_PATH)
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in alac_amd.SIGNATURES, n
    alac_amd.load_library()
    for m in ("loudness_int", "loudness_float", "loudness_reports"):
        assert callable(getattr(alac_amd.Context, m, None)), m
    for f in ("integrated_loudness", "loudness_filter", "loudness_rows"):
        assert callable(getattr(alac_amd, f, None)), f


def test_header_declares_the_calls_the_struct_and_the_rule():
    text = header()
    for n in NAMES:
        assert re.search(r"\b" + n + r"\s*\(", text), n
    struct = text[text.index("typedef struct alac_hip_loudness_report {"):text.index("} alac_hip_loudness_report;")]
    fields = re.findall(r"^\s+(uint\d+_t|double) (\w+);", struct, re.M)
    assert fields == [("uint32_t", "first_block"), ("uint32_t", "num_blocks"), ("double", "peak"), ("uint64_t", "nonfinite"),
                      ("uint64_t", "reserved")]
    assert C.sizeof(alac_amd.LoudnessReport) == 32
    assert [n for n, _ in alac_amd.LoudnessReport._fields_] == [n for _, n in fields]
    assert [C.sizeof(t) for _, t in alac_amd.LoudnessReport._fields_] == [4, 4, 8, 8, 8]
    assert alac_amd.LoudnessReport.peak.offset == 8 and alac_amd.LoudnessReport.nonfinite.offset == 16
    decl = text[text.index("int32_t alac_hip_loudness_int("):]
    decl = decl[:decl.index(";")]
    for arg in ("const void *d_in", "const alac_hip_int_source *src", "uint32_t num_channels", "uint32_t sample_rate",
                "uint64_t total_frames", "const uint64_t *h_seg_first_frame", "uint32_t num_segments", "void *d_workspace",
                "uint64_t workspace_bytes", "double *d_energy", "uint64_t energy_rows", "alac_hip_loudness_report *d_reports"):
        assert arg in decl, arg
    decl = text[text.index("int32_t alac_hip_loudness_float("):]
    decl = decl[:decl.index(";")]
    for arg in ("const float *d_in", "uint64_t channel_stride", "uint64_t frame_stride", "uint32_t sample_rate",
                "double *d_energy", "uint64_t energy_rows"):
        assert arg in decl, arg
    for line in ("x = s * 2^-(S-1) in double", "x = (double)f", "is read as 0.0 and counted",
                 "y = b0 x + s1;   s1 = b1 x - a1 y + s2;   s2 = b2 x - a2 y",
                 "f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196",
                 "K = tan(pi f0 / fs), Vh = 10^(G/20), Vb = Vh^0.4996667741545416, a0 = 1 + K/Q + K^2",
                 "b = [(Vh + Vb K/Q + K^2), 2 (K^2 - Vh), (Vh - Vb K/Q + K^2)] / a0",
                 "a1 = 2 (K^2 - 1) / a0, a2 = (1 - K/Q + K^2) / a0", "f0 = 38.13547087602444, Q = 0.5003270373238773",
                 "b = [1, -2, 1]", "fs must be a multiple of 10 in [8 000, 384 000]", "hop = fs / 10 frames (100 ms)",
                 "floor(n / hop) rows", "d_energy[(first_block[s] + k) * num_channels + c]",
                 "gating block j covers rows j .. j+3, z_c = sum / (4 * hop);  l_j = -0.691 + 10 log10 sum_c G_c z_cj",
                 "the absolute gate is -70", "10 LU under", "-HUGE_VAL when no block passes or there are fewer than 4 rows",
                 "8  C Lc Rc L R Ls Rs LFE        1 1 1 1 1 1.41 1.41 0"):
        assert line in text, line


def test_signatures_and_refusal_without_a_context():
    sig = alac_amd.SIGNATURES
    assert len(sig["alac_hip_loudness_int"][1]) == 13 and len(sig["alac_hip_loudness_float"][1]) == 14
    assert len(sig["alac_hip_loudness_int_host"][1]) == 11 and len(sig["alac_hip_loudness_float_host"][1]) == 12
    lib = alac_amd.load_library()
    src = alac_amd.IntSource(4, 24, 1, 0, 4096, 1)
    for s in (None, C.byref(src)):
        assert lib.alac_hip_loudness_int(None, None, s, 2, 48000, 10, None, 1, None, 0, None, 0, None) == -50
        assert lib.alac_hip_loudness_int_host(None, None, s, 2, 48000, 10, None, 1, None, 0, None) == -50
    assert lib.alac_hip_loudness_float(None, None, 2, 4096, 1, 48000, 10, None, 1, None, 0, None, 0, None) == -50
    assert lib.alac_hip_loudness_float_host(None, None, 2, 4096, 1, 48000, 10, None, 1, None, 0, None) == -50


def test_workspace_query():
    lib = alac_amd.load_library()
    ws = lib.alac_hip_loudness_workspace_bytes
    assert ws(48000, 2, 0, 1) > 0 and ws(48000, 2, 0, 1) % 256 == 0
    assert ws(48000, 2, 1 << 20, 1) < ws(48000, 2, 1 << 21, 1) < ws(48000, 8, 1 << 21, 1) < ws(48000, 8, 1 << 21, 1000)
    # a chunk of L frames keeps 4 state words and a sum per channel: 40 bytes per channel and chunk, and a little per segment
    L = 64  # the chunk at 48 kHz
    assert ws(48000, 2, 1 << 24, 1) < 1.01 * 2 * 40 * (1 << 24) / L + 4096
    for bad in ((44101, 2, 100, 1), (48000, 0, 100, 1), (48000, 9, 100, 1), (48000, 2, 100, 0)):
        assert ws(*bad) == 0, bad


def test_class_declares_loudness_batch():
    with open(os.path.join(ROOT, "include", "alac", "ALACDecoder.h")) as f:
        text = f.read()
    assert "LoudnessBatch(const uint8_t *stream, const uint32_t *packetBytes, uint32_t numPackets, const uint32_t *fileFirstPacket," in text
    assert "uint32_t numFiles, double *outLufs, double *outPeak, uint32_t *outFrames, int32_t *outStatus)" in text
