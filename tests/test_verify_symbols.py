"""CPU: the verify surface exists — libalac_hip.so exports alac_hip_verify*, include/alac_hip.h documents them, the host-only
sizing call answers without a GPU, and alacconvert lists --verify and --compare."""
import ctypes
import os
import re
import subprocess

import alac_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["alac_hip_verify", "alac_hip_verify_host", "alac_hip_verify_workspace_bytes_stream"]


def test_library_exports_verify():
    lib = ctypes.CDLL(alac_amd.LIB_PATH)
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in alac_amd.SIGNATURES, n


def test_header_documents_verify():
    with open(os.path.join(ROOT, "include", "alac_hip.h")) as f:
        text = f.read()
    for n in NAMES:
        assert re.search(r"\b" + n + r"\s*\(", text), n
    for arg in ("d_pcm_expected", "d_num_samples_expected", "d_first_mismatch", "d_bad_packets", "0xFFFFFFFF",
                "codec/ALACDecoder.cu"):
        assert arg in text, arg


def test_verify_workspace_is_the_decode_workspace_plus_the_frame_counts():
    """host only: no PCM plane — one uint32 per packet (rounded to 256 bytes) on top of what decode needs"""
    alac_amd.load_library()
    lib = ctypes.CDLL(alac_amd.LIB_PATH)
    lib.alac_hip_verify_workspace_bytes_stream.restype = ctypes.c_uint64
    lib.alac_hip_verify_workspace_bytes_stream.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64]
    lib.alac_hip_decode_workspace_bytes_stream.restype = ctypes.c_uint64
    lib.alac_hip_decode_workspace_bytes_stream.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64]
    for depth, ch, n, sb in ((16, 2, 10000, 0), (24, 6, 77, 123456), (32, 1, 1, 0)):
        fmt = alac_amd.make_format(4096, depth, ch)
        v = lib.alac_hip_verify_workspace_bytes_stream(ctypes.byref(fmt), n, sb)
        d = lib.alac_hip_decode_workspace_bytes_stream(ctypes.byref(fmt), n, sb)
        assert v == d + (n * 4 + 255) // 256 * 256
        assert v < d + n * fmt.packet_bytes
    bad = alac_amd.make_format(4096, 17, 2)
    assert lib.alac_hip_verify_workspace_bytes_stream(ctypes.byref(bad), 10, 0) == 0


def test_verify_without_a_context_is_a_parameter_error():
    lib = ctypes.CDLL(alac_amd.LIB_PATH)
    lib.alac_hip_verify.restype = ctypes.c_int32
    lib.alac_hip_verify_host.restype = ctypes.c_int32
    assert lib.alac_hip_verify(None, None, 0, None, None, 0, None, None, None, ctypes.c_uint64(0), None, None, None) == -50
    assert lib.alac_hip_verify_host(None, None, 0, None, None, 0, None, None, None, None) == -50


def test_alacconvert_usage_lists_verify_and_compare():
    cu = os.path.join(ROOT, "convert-utility")
    subprocess.check_call(["make", "-C", cu, "alacconvert"], stdout=subprocess.DEVNULL)
    p = subprocess.run([os.path.join(cu, "alacconvert"), "-h"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1
    assert "--verify" in p.stdout and "--compare" in p.stdout
    # --compare takes exactly two files and no other option
    p = subprocess.run([os.path.join(cu, "alacconvert"), "--compare", "--batch", "a.caf", "b.wav"], capture_output=True,
                       text=True, timeout=60)
    assert p.returncode == 1 and "Usage" in p.stdout
