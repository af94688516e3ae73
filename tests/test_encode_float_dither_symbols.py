"""CPU: the dithered float encode surface exists — libalac_hip.so exports alac_hip_encode_float_dither and its host form, both
bound in SIGNATURES with the arguments of the calls they extend plus (dither, packet origin); include/alac_hip.h declares
them and carries the rule line for line; a call without a context is refused; alacconvert's usage names --dither and the flag
is refused without a bit depth it can dither to."""
import ctypes as C
import os
import re
import subprocess

import alac_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["alac_hip_encode_float_dither", "alac_hip_encode_float_dither_host"]
BIN = os.path.join(ROOT, "convert-utility", "alacconvert")

RULE = """
T  = t >> 1
w  = Philox4x32-10( counter = (T & 0xffffffff, T >> 32, c, 0),  key = (S & 0xffffffff, S >> 32) )   # 4 words
(wa, wb) = (w[0], w[1]) if t is even, (w[2], w[3]) if t is odd       # one Philox call serves two frames
k  = (int)(wa >> 8) - (int)(wb >> 8)                                  # -(2^24 - 1) .. 2^24 - 1, triangular
d  = (float)k * 2^-24                                                 # exact; strictly inside (-1, 1) LSB
v  = x * 2^(b-1) + d        rounded ONCE to float32  (the product is exact, so fmaf and mul-then-add agree)
r  = rint(v)                                                          # then exactly the existing rule:
s, clipped(x)  as alac_hip_encode_float defines them from r           # saturation, NaN -> 0 and clipped
"""


def test_library_exports_and_binds_both():
    lib = C.CDLL(alac_amd.LIB_PATH)
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in alac_amd.SIGNATURES, n
    alac_amd.load_library()
    res, args = alac_amd.SIGNATURES["alac_hip_encode_float_dither"]
    base = alac_amd.SIGNATURES["alac_hip_encode_float"][1]
    assert res is C.c_int32 and len(args) == 21 and args[:19] == base and args[19:] == [C.c_void_p] * 2
    res, args = alac_amd.SIGNATURES["alac_hip_encode_float_dither_host"]
    base = alac_amd.SIGNATURES["alac_hip_encode_float_host"][1]
    assert res is C.c_int32 and len(args) == 18 and args[:16] == base and args[16:] == [C.c_void_p] * 2
    assert C.sizeof(alac_amd.Dither) == 16 and alac_amd.Dither.seed.offset == 8 and alac_amd.Dither.reserved.offset == 4


def test_header_declares_them_and_carries_the_rule():
    with open(os.path.join(ROOT, "include", "alac_hip.h")) as f:
        text = f.read()
    for n in NAMES:
        assert re.search(r"\b" + n + r"\s*\(", text), n
    for n, own in (("alac_hip_encode_float_dither", "d_packet_origin"), ("alac_hip_encode_float_dither_host", "h_packet_origin")):
        decl = text[text.index("int32_t " + n + "("):]
        decl = decl[:decl.index(";")]
        assert decl.count(",") + 1 == (21 if own[0] == "d" else 18), n
        assert "const alac_hip_dither *dither" in decl and "const uint64_t *" + own in decl, n
    assert "enum { ALAC_HIP_DITHER_NONE = 0, ALAC_HIP_DITHER_TPDF = 1 };" in text
    struct = re.search(r"typedef struct alac_hip_dither \{(.*?)\} alac_hip_dither;", text, re.S).group(1)
    assert re.findall(r"(uint\d+_t) (\w+);", struct) == [("uint32_t", "mode"), ("uint32_t", "reserved"), ("uint64_t", "seed")]
    for line in RULE.strip().split("\n"):
        assert line in text, line
    for words in ("0xD2511F53 / 0xCD9E8D57", "0x9E3779B9 / 0xBB67AE85", "ten rounds", "t = origin[p] + i",
                  "p * frame_size when it is NULL", "no dither there", "== x no longer holds on the grid"):
        assert words in text, words
    with open(os.path.join(ROOT, "include", "alac", "ALACEncoder.h")) as f:
        enc = f.read()
    assert "void SetDither(uint32_t mode, uint64_t seed)" in enc and "const uint64_t *packetOrigin" in enc


def test_refusal_without_a_context():
    lib = alac_amd.load_library()
    dz = alac_amd.Dither(1, 0, 7)
    assert lib.alac_hip_encode_float_dither(None, None, None, 0, 1, None, 1, None, 0, 0, None, 0, None, 0, None, 0, None, None,
                                            None, C.byref(dz), None) == -50
    total = C.c_uint64(5)
    assert lib.alac_hip_encode_float_dither_host(None, None, None, 0, 1, None, 1, None, 0, None, 0, None, 0, None,
                                                 C.byref(total), None, C.byref(dz), None) == -50
    import inspect
    sig = inspect.signature(alac_amd.Context.encode_float)
    assert [sig.parameters[k].default for k in ("dither", "seed", "packet_origin")] == [None, 0, None]


def run(*args):
    p = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
    return p.returncode, p.stdout, p.stderr


def test_alacconvert_names_and_refuses_the_flag(tmp_path):
    rc, out, _ = run()
    assert rc == 1 and "--dither" in out and "--dither-seed" in out
    src = tmp_path / "in.wav"
    src.write_bytes(b"")
    for flags in ([], ["--float-bits", 32]):
        rc, out, err = run("--dither", *flags, src, tmp_path / "out.caf")
        assert rc == 1 and "--dither" in err, (flags, err)
        assert not (tmp_path / "out.caf").exists()
    rc, out, err = run("--float-bits", 16, "--dither", "--dither-seed", "12x", src, tmp_path / "out.caf")
    assert rc == 1 and "Usage" in out  # a seed that is not a number
