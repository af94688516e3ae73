"""CPU: the verify-float surface exists — libalac_hip.so exports alac_hip_verify_float and its host form, SIGNATURES binds
them, include/alac_hip.h declares them and states what they promise, a call without a context is refused,
Context.verify_float has its defaults, and alacconvert lists --verify-source and refuses it without --float-bits."""
import ctypes
import inspect
import os
import re
import subprocess

import alac_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CU = os.path.join(ROOT, "convert-utility")
NAMES = ["alac_hip_verify_float", "alac_hip_verify_float_host"]


def test_library_exports_verify_float():
    lib = ctypes.CDLL(alac_amd.LIB_PATH)
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in alac_amd.SIGNATURES, n
    assert len(alac_amd.SIGNATURES["alac_hip_verify_float"][1]) == 17
    assert len(alac_amd.SIGNATURES["alac_hip_verify_float_host"][1]) == 14
    alac_amd.load_library()  # every bound name resolves


def test_header_declares_and_documents_verify_float():
    with open(os.path.join(ROOT, "include", "alac_hip.h")) as f:
        text = f.read()
    for n in NAMES:
        assert re.search(r"\b" + n + r"\s*\(", text), n
    flat = " ".join(text.split())
    flat = flat.replace(" * ", " ")
    # property 1: what may be loaded from the source
    assert "Only frames i < min(expected[p], frame_size) of packet p are ever loaded from d_in" in flat
    assert "clamps by the expected count before it forms an address" in flat
    # the refusal list
    for phrase in ("everything alac_hip_verify refuses", "d_in null or not 4-byte aligned", "frame_stride 0",
                   "channel_stride 0 with more than one channel", "the largest index overflowing 64 bits",
                   "a dither mode above ALAC_HIP_DITHER_TPDF", "reserved != 0", "mode TPDF on a 32-bit stream",
                   "a d_packet_origin that is not 8-byte aligned", "A mismatch is data, not an error"):
        assert phrase in flat, phrase
    # the argument order: alac_hip_verify's, with alac_hip_encode_float_dither's source and dither arguments in theirs
    decl = flat[flat.index("int32_t alac_hip_verify_float("):]
    decl = decl[:decl.index(";")]
    order = ["h_cookie", "cookie_size", "d_stream", "d_packet_offsets", "num_packets", "d_in", "channel_stride", "frame_stride",
             "d_num_samples_expected", "dither", "d_packet_origin", "d_workspace", "workspace_bytes", "d_first_mismatch",
             "d_status", "d_bad_packets"]
    pos = [decl.index(a) for a in order]
    assert pos == sorted(pos)


def test_verify_float_without_a_context_is_a_parameter_error():
    lib = alac_amd.load_library()
    u64 = ctypes.c_uint64
    assert lib.alac_hip_verify_float(None, None, 0, None, None, 0, None, u64(0), u64(0), None, None, None, None, u64(0), None,
                                     None, None) == -50
    assert lib.alac_hip_verify_float_host(None, None, 0, None, None, 0, None, u64(0), u64(0), None, None, None, None, None) == -50


def test_context_verify_float_signature():
    sig = inspect.signature(alac_amd.Context.verify_float)
    assert list(sig.parameters) == ["self", "cookie", "stream", "offsets", "num_packets", "x", "num_samples", "dither", "seed",
                                    "packet_origin"]
    defaults = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert defaults == {"num_samples": None, "dither": None, "seed": 0, "packet_origin": None}


def test_alacconvert_lists_and_refuses_verify_source(tmp_path):
    subprocess.check_call(["make", "-C", CU, "alacconvert"], stdout=subprocess.DEVNULL)
    binary = os.path.join(CU, "alacconvert")
    p = subprocess.run([binary, "-h"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and "--verify-source" in p.stdout
    assert "--verify" in p.stdout and "--compare" in p.stdout
    # --verify-source is "against the float file": without --float-bits there is none — one line on stderr, nothing written
    src, dst = tmp_path / "in.wav", tmp_path / "out.caf"
    import sys
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import caf_oracle as co
    src.write_bytes(co.make_wav(bytes(4096 * 4), 2, 44100, 16))
    for flags in (["--verify-source"], ["--verify-source", "--batch"], ["--verify", "--verify-source"]):
        p = subprocess.run([binary] + flags + [str(src), str(dst)], capture_output=True, text=True, timeout=60)
        assert p.returncode == 1, flags
        lines = [l for l in p.stderr.splitlines() if l.strip()]
        assert len(lines) == 1 and "--verify-source" in lines[0] and "--float-bits" in lines[0], (flags, p.stderr)
        assert not dst.exists()
    # --compare still stands alone
    p = subprocess.run([binary, "--compare", "--verify-source", "a.caf", "b.wav"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and "Usage" in p.stdout
