"""CPU: the integer decode surface exists — libalac_hip.so exports alac_hip_decode_int and its host form, both are bound in
SIGNATURES, include/alac_hip.h declares them and states the rule (the index, the two shifts, the refusal of a reduction, the
two families of layouts), and a call without a context is a parameter error."""
import ctypes
import os
import re

import alac_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["alac_hip_decode_int", "alac_hip_decode_int_host"]


def header():
    with open(os.path.join(ROOT, "include", "alac_hip.h")) as f:
        return f.read()


def test_library_exports_decode_int():
    lib = ctypes.CDLL(alac_amd.LIB_PATH)
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in alac_amd.SIGNATURES, n
    alac_amd.load_library()  # every bound symbol resolves


def test_header_declares_decode_int():
    text = header()
    for n in NAMES:
        assert re.search(r"\b" + n + r"\s*\(", text), n
    decl = text[text.index("int32_t alac_hip_decode_int("):]
    decl = decl[:decl.index(";")]
    for arg in ("void *d_out", "const alac_hip_int_dest *dst", "d_workspace", "d_num_samples_out", "d_status"):
        assert arg in decl, arg
    decl = text[text.index("int32_t alac_hip_decode_int_host("):]
    decl = decl[:decl.index(";")]
    for arg in ("void *h_out", "const alac_hip_int_dest *dst", "h_packet_bytes", "h_num_samples_out", "h_status"):
        assert arg in decl, arg
    # the destination is the existing struct under another name, not a new one
    assert re.search(r"typedef\s+alac_hip_int_source\s+alac_hip_int_dest\s*;", text)
    assert len(re.findall(r"typedef struct alac_hip_int_", text)) == 2  # alac_hip_int_source and alac_hip_int_report


def test_header_states_the_rule():
    text = header()
    sec = text[text.index("batch decode to integer PCM"):text.index("typedef alac_hip_int_source alac_hip_int_dest")]
    flat = " ".join(sec.replace("*", " ").split())
    for phrase in ("c channel_stride + (p frame_size + i) frame_stride",
                   "s << (8 container_bytes - D)",
                   "s << (S - D)",
                   "D <= S <= 8 container_bytes",
                   "S < D is refused",
                   "alac_hip_pcm_requantize",
                   "channel_stride >= T frame_stride",
                   "frame_stride >= C channel_stride",
                   "alac_hip_decode_workspace_bytes_stream",
                   "reproduces alac_hip_decode's output byte for byte"):
        assert phrase in flat, phrase


def test_signatures_match_the_header():
    """twelve arguments for the device form (the u64 workspace size the only integer wider than 32 bits), ten for the host
    form"""
    res, args = alac_amd.SIGNATURES["alac_hip_decode_int"]
    assert res is ctypes.c_int32 and len(args) == 12 and args[7] is ctypes.c_uint64
    assert args[2] is ctypes.c_uint32 and args[5] is ctypes.c_uint32
    assert all(a is ctypes.c_void_p for i, a in enumerate(args) if i not in (2, 5, 7))
    res, args = alac_amd.SIGNATURES["alac_hip_decode_int_host"]
    assert res is ctypes.c_int32 and len(args) == 10
    assert all(a is ctypes.c_void_p for i, a in enumerate(args) if i not in (2, 5))


def test_decode_int_without_a_context_is_a_parameter_error():
    lib = alac_amd.load_library()
    dst = alac_amd.capi.IntSource(4, 32, 1, 0, 4096, 1)
    assert lib.alac_hip_decode_int(None, None, 0, None, None, 0, None, 0, None, ctypes.byref(dst), None, None) == -50
    assert lib.alac_hip_decode_int_host(None, None, 0, None, None, 0, None, ctypes.byref(dst), None, None) == -50


def test_context_has_decode_int():
    assert callable(getattr(alac_amd.Context, "decode_int", None))
