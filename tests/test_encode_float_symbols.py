"""CPU: the float encode surface exists — libalac_hip.so exports alac_hip_encode_float, its host form and its workspace
query, all bound in SIGNATURES; include/alac_hip.h declares them and states the quantization rule; alacconvert's usage
names --float-bits; and the container code sniffs float WAVE / CAF files only when asked to (alacconvert --float-bits),
every file sniffing as before otherwise."""
import ctypes as C
import os
import re
import struct
import subprocess
import sys

import numpy as np

import alac_amd
from container_lib import SO, Container, Info, _u8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import caf_oracle as co  # noqa: E402

NAMES = ["alac_hip_encode_float_workspace_bytes", "alac_hip_encode_float", "alac_hip_encode_float_host"]
FLOAT_GUID = bytes([3, 0, 0, 0, 0, 0, 0x10, 0, 0x80, 0, 0, 0xAA, 0, 0x38, 0x9B, 0x71])
PCM_GUID = bytes([1]) + FLOAT_GUID[1:]


def make_float_wav(x, rate=44100, extensible=False, bits=32, guid=FLOAT_GUID):
    """x: float32 [channels, frames] -> a WAVE file of format tag 3 (or EXTENSIBLE with the given subformat)"""
    ch = x.shape[0]
    data = np.ascontiguousarray(x.T).astype("<f4" if bits == 32 else "<f8").tobytes()
    bpf = ch * bits // 8
    if extensible:
        fmt = struct.pack("<HHIIHHHHI", 0xFFFE, ch, rate, rate * bpf, bpf, bits, 22, bits, (1 << ch) - 1) + guid
    else:
        fmt = struct.pack("<HHIIHH", 3, ch, rate, rate * bpf, bpf, bits)
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", len(data)) + data
    return b"RIFF" + struct.pack("<I", len(body)) + body


def make_float_caf(x, rate=44100, little_endian=True):
    """x: float32 [channels, frames] -> a CAF lpcm file with the float flag, in either byte order"""
    ch = x.shape[0]
    data = np.ascontiguousarray(x.T).astype("<f4" if little_endian else ">f4").tobytes()
    out = b"caff\x00\x01\x00\x00"
    out += b"desc" + struct.pack(">q", 32) + struct.pack(">d4sIIIII", float(rate), b"lpcm", 1 | (2 if little_endian else 0),
                                                         4 * ch, 1, ch, 32)
    out += b"data" + struct.pack(">q", len(data) + 4) + b"\x00\x00\x00\x00" + data
    return out


def test_library_exports_encode_float():
    lib = C.CDLL(alac_amd.LIB_PATH)
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in alac_amd.SIGNATURES, n
    alac_amd.load_library()
    assert callable(getattr(alac_amd.Context, "encode_float", None))


def test_header_declares_and_states_the_rule():
    with open(os.path.join(ROOT, "include", "alac_hip.h")) as f:
        text = f.read()
    for n in NAMES:
        assert re.search(r"\b" + n + r"\s*\(", text), n
    decl = text[text.index("int32_t alac_hip_encode_float("):]
    decl = decl[:decl.index(";")]
    for arg in ("const float *d_in", "uint64_t channel_stride", "uint64_t frame_stride", "uint32_t *d_clipped",
                "uint32_t max_segment_packets"):
        assert arg in decl, arg
    for line in ("r = rint(x * 2^(b-1))", "round half to even", "0                 if x is NaN",
                 "2^(b-1) - 1       if r >  2^(b-1) - 1", "-2^(b-1)          if r < -2^(b-1)",
                 "clipped(x) = x is NaN or r was outside [-2^(b-1), 2^(b-1) - 1]", "(s << 4)",
                 "d_in[c * channel_stride + (p * frame_size + i) * frame_stride]"):
        assert line in text, line
    with open(os.path.join(ROOT, "include", "alac", "ALACEncoder.h")) as f:
        assert "EncodeSegmentsFloat(const float *pcm, uint64_t channelStride, uint64_t frameStride" in f.read()


def test_signatures_and_refusal_without_a_context():
    res, args = alac_amd.SIGNATURES["alac_hip_encode_float"]
    assert res is C.c_int32 and len(args) == 19 and args[3] is C.c_uint64 and args[4] is C.c_uint64
    res, args = alac_amd.SIGNATURES["alac_hip_encode_float_host"]
    assert res is C.c_int32 and len(args) == 16
    lib = alac_amd.load_library()
    assert lib.alac_hip_encode_float(None, None, None, 0, 1, None, 1, None, 0, 0, None, 0, None, 0, None, 0, None, None,
                                     None) == -50
    fmt = alac_amd.make_format(4096, 16, 2, 44100)
    # the encode workspace, then the staged PCM of every packet
    ws = lib.alac_hip_encode_float_workspace_bytes(C.byref(fmt), 10, 10)
    assert ws >= lib.alac_hip_encode_workspace_bytes(C.byref(fmt), 10, 10) + 10 * fmt.packet_bytes and ws % 256 == 0
    assert lib.alac_hip_encode_float_workspace_bytes(C.byref(alac_amd.make_format(4096, 18, 2, 44100)), 10, 10) == 0


def test_alacconvert_usage_names_float_bits():
    binary = os.path.join(ROOT, "convert-utility", "alacconvert")
    p = subprocess.run([binary], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and "--float-bits" in p.stdout


def sniff_float(data):
    lib = C.CDLL(SO)
    info, err, is_float = Info(), C.create_string_buffer(128), C.c_int32(-1)
    rc = lib.alacfile_sniff_float(_u8(data), C.c_uint64(len(data)), C.byref(info), C.byref(is_float), err, 128)
    return rc, info, is_float.value, err.value.decode()


def test_float_sniffing_only_when_asked():
    Container()  # (re)builds libcontainer.so from the current sources
    x = np.linspace(-1, 1, 2 * 100, dtype=np.float32).reshape(2, 100)
    for name, f in (("tag 3", make_float_wav(x)), ("extensible", make_float_wav(x, extensible=True))):
        rc, info, err = Container().sniff(f)
        assert rc == -1 and err == "Cannot determine what format file is", name  # unchanged: refused
        rc, info, is_float, err = sniff_float(f)
        assert rc == 0 and is_float == 1 and info.channels == 2 and info.bits_per_channel == 32, (name, err)
        assert info.data_size == 800 and f[info.data_pos:info.data_pos + 800] == x.T.astype("<f4").tobytes(), name
    rc, info, is_float, err = sniff_float(make_float_wav(x[:1], bits=64))
    assert rc == 0 and is_float == 1 and info.bits_per_channel == 64  # alacconvert refuses it by its width
    rc, _, _, err = sniff_float(make_float_wav(x, extensible=True, guid=PCM_GUID))
    assert rc == -1 and err == "Cannot determine what format file is"
    for le in (True, False):
        f = make_float_caf(x, little_endian=le)
        rc, info, _ = Container().sniff(f)
        assert rc == 0 and info.bits_per_channel == 32 and info.big_endian_pcm == (not le)  # as before: lpcm
        rc, info, is_float, err = sniff_float(f)
        assert rc == 0 and is_float == 1 and info.big_endian_pcm == (not le) and info.data_size == 800
    # integer PCM sniffs as integer either way
    pcm = (np.arange(200, dtype=np.int16) * 7).tobytes()
    for f in (co.make_wav(pcm, 2, 44100, 16), co.make_pcm_caf(pcm, 2, 44100, 16)):
        rc, info, is_float, err = sniff_float(f)
        assert rc == 0 and is_float == 0 and info.bits_per_channel == 16
        rc2, info2, _ = Container().sniff(f)
        assert rc2 == 0 and bytes(info2) == bytes(info)
