"""CPU: the float decode surface exists — libalac_hip.so exports alac_hip_decode_float and its host form, both are bound in
SIGNATURES, include/alac_hip.h documents the layout, the channel stride and the scale, and a call without a context is a
parameter error."""
import ctypes
import os
import re

import alac_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["alac_hip_decode_float", "alac_hip_decode_float_host"]


def test_library_exports_decode_float():
    lib = ctypes.CDLL(alac_amd.LIB_PATH)
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in alac_amd.SIGNATURES, n
    alac_amd.load_library()  # every bound symbol resolves


def test_header_documents_decode_float():
    with open(os.path.join(ROOT, "include", "alac_hip.h")) as f:
        text = f.read()
    for n in NAMES:
        assert re.search(r"\b" + n + r"\s*\(", text), n
    decl = text[text.index("int32_t alac_hip_decode_float("):]
    decl = decl[:decl.index(";")]
    for arg in ("float *d_out", "uint64_t channel_stride", "d_num_samples_out", "d_status"):
        assert arg in decl, arg
    # the layout, the stride's lower bound and the scale
    assert "d_out[c * channel_stride + p * frame_size + i]" in text
    assert "num_packets * frame_size" in text
    assert "2^-(bit_depth - 1)" in text
    assert "alac_hip_decode_workspace_bytes_stream" in text


def test_signatures_match_the_header():
    """twelve arguments for the device form (pointer, u64 stride), ten for the host form"""
    res, args = alac_amd.SIGNATURES["alac_hip_decode_float"]
    assert res is ctypes.c_int32 and len(args) == 12 and args[9] is ctypes.c_uint64 and args[7] is ctypes.c_uint64
    res, args = alac_amd.SIGNATURES["alac_hip_decode_float_host"]
    assert res is ctypes.c_int32 and len(args) == 10 and args[7] is ctypes.c_uint64


def test_decode_float_without_a_context_is_a_parameter_error():
    lib = alac_amd.load_library()
    assert lib.alac_hip_decode_float(None, None, 0, None, None, 0, None, 0, None, 0, None, None) == -50
    assert lib.alac_hip_decode_float_host(None, None, 0, None, None, 0, None, 0, None, None) == -50


def test_context_has_decode_float():
    assert callable(getattr(alac_amd.Context, "decode_float", None))
