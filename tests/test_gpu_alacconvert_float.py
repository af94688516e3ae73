"""alacconvert --float-bits N on the GPU: a 32-bit float WAVE (tag 3 or EXTENSIBLE) or CAF (either byte order) file gives,
byte for byte, the CAF / M4A that alacconvert writes for the integer WAVE holding the numpy-quantized samples at N bits
(the rule of include/alac_hip.h); --batch, the clip warning, the refusals, and a float WAVE without the flag still
refused as before."""
import os
import subprocess
import sys

import numpy as np
import pytest

from container_lib import music_like
from test_encode_float_symbols import make_float_caf, make_float_wav
from test_gpu_encode_float import quantize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import caf_oracle as co  # noqa: E402

pytestmark = pytest.mark.gpu
CU = os.path.join(ROOT, "convert-utility")
BIN = os.path.join(CU, "alacconvert")


@pytest.fixture(scope="module")
def binary(gpu_ctx):
    subprocess.check_call(["make", "-C", CU, "alacconvert"], stdout=subprocess.DEVNULL)
    return BIN


def run(binary, *args):
    p = subprocess.run([binary] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    return p.returncode, p.stdout, p.stderr


def floats(ch, frames, seed, gain=0.9):
    """music-like float32 [ch, frames], off the integer grid"""
    s = np.frombuffer(music_like(frames, ch, 16, seed), "<i2").reshape(frames, ch).T.astype(np.float64)
    rng = np.random.default_rng(seed)
    return (s / 32768.0 * gain + rng.normal(0, 3e-6, s.shape)).astype(np.float32)


def int_wav(x, bits):
    """the integer WAVE of x quantized at `bits` by numpy"""
    s, _ = quantize(x, bits)
    v = s.T.reshape(-1)
    if bits == 16:
        pcm = v.astype("<i2").tobytes()
    else:
        c = v & 0xFFFFFF
        pcm = np.stack([c & 0xFF, (c >> 8) & 0xFF, (c >> 16) & 0xFF], axis=1).astype(np.uint8).tobytes()
    return co.make_wav(pcm, x.shape[0], 44100, bits)


def convert(binary, tmp_path, name, data, out_ext, *flags):
    src, dst = tmp_path / f"{name}.in", tmp_path / f"{name}.{out_ext}"
    src.write_bytes(data)
    rc, out, err = run(binary, *flags, src, dst)
    return rc, out, err, (dst.read_bytes() if dst.exists() else None)


@pytest.mark.parametrize("bits,ch,kind,ext", [(16, 2, "tag3", "caf"), (24, 2, "tag3", "caf"), (16, 1, "tag3", "caf"),
                                              (24, 1, "extensible", "caf"), (16, 2, "extensible", "caf"),
                                              (24, 2, "caf_le", "caf"), (16, 1, "caf_be", "caf"), (24, 2, "caf_be", "caf"),
                                              (16, 2, "tag3", "m4a"), (24, 1, "caf_le", "m4a")])
def test_float_file_equals_integer_file(binary, tmp_path, bits, ch, kind, ext):
    x = floats(ch, 3 * 4096 + 123, bits + ch)
    data = {"tag3": lambda: make_float_wav(x), "extensible": lambda: make_float_wav(x, extensible=True),
            "caf_le": lambda: make_float_caf(x), "caf_be": lambda: make_float_caf(x, little_endian=False)}[kind]()
    rc, _, err, got = convert(binary, tmp_path, "f", data, ext, "--float-bits", bits)
    assert rc == 0 and "clipped" not in err, err
    rc, _, err, want = convert(binary, tmp_path, "i", int_wav(x, bits), ext)
    assert rc == 0, err
    assert got == want


def test_batch_of_two_float_files(binary, tmp_path):
    xs = [floats(2, 2 * 4096 + 7, 1), floats(2, 4096 * 3, 2)]
    args = []
    for k, x in enumerate(xs):
        (tmp_path / f"f{k}.wav").write_bytes(make_float_wav(x))
        args += [tmp_path / f"f{k}.wav", tmp_path / f"f{k}.caf"]
    rc, _, err = run(binary, "--batch", "--float-bits", 24, *args)
    assert rc == 0, err
    for k, x in enumerate(xs):
        rc, _, err, want = convert(binary, tmp_path, f"i{k}", int_wav(x, 24), "caf")
        assert rc == 0 and (tmp_path / f"f{k}.caf").read_bytes() == want


def test_clip_warning(binary, tmp_path):
    x = floats(2, 4096 + 50, 9, gain=6.0)  # music_like peaks near full scale / 4
    _, clip = quantize(x, 16)
    assert clip.sum() > 0
    rc, _, err, got = convert(binary, tmp_path, "loud", make_float_wav(x), "caf", "--float-bits", 16)
    assert rc == 0 and got is not None
    assert f"Warning: {int(clip.sum())} samples clipped to 16 bits" in err and "loud.in" in err
    rc, _, err, want = convert(binary, tmp_path, "i", int_wav(x, 16), "caf")
    assert got == want


def test_refusals(binary, tmp_path):
    x = floats(2, 5000, 4)
    cases = {
        "f64": (make_float_wav(x, bits=64), ["--float-bits", 16], "64-bit"),
        "int": (int_wav(x, 16), ["--float-bits", 16], "not integer PCM"),
        "verify": (make_float_wav(x), ["--float-bits", 16, "--verify"], "--verify"),
    }
    for name, (data, flags, words) in cases.items():
        rc, _, err, got = convert(binary, tmp_path, name, data, "caf", *flags)
        lines = [ln for ln in err.splitlines() if ln.strip()]
        assert rc == 1 and got is None and len(lines) == 1, (name, err)
        assert words in lines[0] and f"{name}.in" in lines[0], (name, err)


def test_float_wav_without_the_flag_is_still_refused(binary, tmp_path):
    for name, data in (("tag3", make_float_wav(floats(2, 4000, 5))),
                       ("ext", make_float_wav(floats(1, 4000, 6), extensible=True))):
        rc, _, err, got = convert(binary, tmp_path, name, data, "caf")
        assert rc == 1 and got is None and "Cannot determine what format file is" in err, err
