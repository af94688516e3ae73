"""CPU: the integer encode surface exists — libalac_hip.so exports alac_hip_pcm_requantize, alac_hip_encode_int, their host
forms and the workspace query, all bound in SIGNATURES; include/alac_hip.h declares them, the source struct and the rule's
lines; the calls refuse a null context with -50 (every other refusal needs a context, hence a GPU: tests/test_gpu_encode_int.py);
the workspace query equals the float one's; ALACEncoder declares EncodeSegmentsInt."""
import ctypes as C
import os
import re

import alac_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["alac_hip_pcm_requantize", "alac_hip_pcm_requantize_host", "alac_hip_encode_int_workspace_bytes", "alac_hip_encode_int",
         "alac_hip_encode_int_host"]


def header():
    with open(os.path.join(ROOT, "include", "alac_hip.h")) as f:
        return f.read()


def test_library_exports_and_binds_the_five_symbols():
    lib = C.CDLL(alac_amd.LIB_PATH)
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in alac_amd.SIGNATURES, n
    alac_amd.load_library()
    for m in ("requantize", "encode_int"):
        assert callable(getattr(alac_amd.Context, m, None)), m


def test_header_declares_the_calls_the_struct_and_the_rule():
    text = header()
    for n in NAMES:
        assert re.search(r"\b" + n + r"\s*\(", text), n
    struct = text[text.index("typedef struct alac_hip_int_source {"):text.index("} alac_hip_int_source;")]
    fields = re.findall(r"^\s+(uint\d+_t) (\w+);", struct, re.M)
    assert fields == [("uint32_t", "container_bytes"), ("uint32_t", "bits"), ("uint32_t", "left_justified"),
                      ("uint32_t", "reserved"), ("uint64_t", "channel_stride"), ("uint64_t", "frame_stride")]
    assert C.sizeof(alac_amd.capi.IntSource) == 32
    assert [(n, C.sizeof(t)) for n, t in alac_amd.capi.IntSource._fields_] == [(n, int(t[4:-2]) // 8) for t, n in fields]
    decl = text[text.index("int32_t alac_hip_encode_int("):]
    decl = decl[:decl.index(";")]
    for arg in ("const void *d_in", "const alac_hip_int_source *src", "uint32_t max_segment_packets", "uint32_t *d_clipped",
                "const alac_hip_dither *dither", "const uint64_t *d_packet_origin"):
        assert arg in decl, arg
    decl = text[text.index("int32_t alac_hip_pcm_requantize("):]
    decl = decl[:decl.index(";")]
    for arg in ("uint8_t *d_pcm_out", "uint64_t pcm_capacity", "uint32_t *d_clipped", "const uint32_t *d_num_samples"):
        assert arg in decl, arg
    for line in ("c * channel_stride + (p * frame_size + i) * frame_stride", "r = s << (b - S)",
                 "acc = s * 2^(24 - D) + k", "q   = acc >> 24 (floor),  rem = acc & (2^24 - 1)",
                 "r   = q + (rem > 2^23  or  (rem == 2^23 and q is odd))", "out = clamp(r, -2^(b-1), 2^(b-1) - 1)",
                 "clipped = the container was out of range, or r was outside that interval",
                 "s = container >> (8 * container_bytes - S), arithmetic", "(out << 4)", "staged as zero, with no dither",
                 "EQUALS that of alac_hip_encode_float on x = s * 2^-(S-1)", "rules DIFFER in some samples",
                 "mean 0 and variance 1/4 LSB^2"):
        assert line in text, line


def test_signatures_and_refusal_without_a_context():
    sig = alac_amd.SIGNATURES
    assert sig["alac_hip_pcm_requantize"] == sig["alac_hip_pcm_requantize_host"] and len(sig["alac_hip_pcm_requantize"][1]) == 11
    # alac_hip_encode_float_dither's list with (d_in, src) for (d_in, channel_stride, frame_stride)
    assert len(sig["alac_hip_encode_int"][1]) == len(sig["alac_hip_encode_float_dither"][1]) - 1 == 20
    assert len(sig["alac_hip_encode_int_host"][1]) == len(sig["alac_hip_encode_float_dither_host"][1]) - 1 == 17
    assert sig["alac_hip_encode_int"][1][4:] == sig["alac_hip_encode_float_dither"][1][5:]
    assert sig["alac_hip_encode_int_host"][1][4:] == sig["alac_hip_encode_float_dither_host"][1][5:]
    lib = alac_amd.load_library()
    fmt = alac_amd.make_format(4096, 16, 2, 44100)
    src = alac_amd.capi.IntSource(4, 24, 1, 0, 4096, 1)
    for f, s in ((None, None), (C.byref(fmt), C.byref(src))):
        assert lib.alac_hip_pcm_requantize(None, f, None, s, None, 1, None, 0, None, None, None) == -50
        assert lib.alac_hip_pcm_requantize_host(None, f, None, s, None, 1, None, 0, None, None, None) == -50
        assert lib.alac_hip_encode_int(None, f, None, s, None, 1, None, 0, 0, None, 0, None, 0, None, 0, None, None, None, None,
                                       None) == -50
        assert lib.alac_hip_encode_int_host(None, f, None, s, None, 1, None, 0, None, 0, None, 0, None, None, None, None,
                                            None) == -50


def test_workspace_query_equals_the_float_one():
    lib = alac_amd.load_library()
    for fs, depth, ch, n, nseg in ((4096, 16, 2, 10, 10), (4096, 24, 2, 100, 3), (17, 20, 6, 3, 3), (1028, 32, 1, 7, 1)):
        fmt = alac_amd.make_format(fs, depth, ch, 44100)
        ws = lib.alac_hip_encode_int_workspace_bytes(C.byref(fmt), n, nseg)
        assert ws == lib.alac_hip_encode_float_workspace_bytes(C.byref(fmt), n, nseg) and ws > 0 and ws % 256 == 0
    assert lib.alac_hip_encode_int_workspace_bytes(C.byref(alac_amd.make_format(4096, 18, 2, 44100)), 10, 10) == 0
    assert lib.alac_hip_encode_int_workspace_bytes(None, 10, 10) == 0


def test_class_declares_encode_segments_int():
    with open(os.path.join(ROOT, "include", "alac", "ALACEncoder.h")) as f:
        text = f.read()
    assert "EncodeSegmentsInt(const void *pcm, const alac_hip_int_source &src, const uint32_t *numSamples" in text
    assert "except EncodeSegmentsInt" in text[text.index("TPDF dither for the float encode methods"):text.index("void SetDither")]
