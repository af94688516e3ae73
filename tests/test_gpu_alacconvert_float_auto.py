"""alacconvert --float-bits auto on the GPU: one --batch of mixed float material comes out at every file's own lossless depth
(16, 24, 16 and 20 bits side by side), each output decodes to its source floats, the 16-bit ones are the bytes of
--float-bits 16; a file without a lossless depth is refused with nothing written; --dither is refused; --verify-source,
--segment-packets, --lpc and --devices work as with a number."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import float_probe_ref as fr
from test_encode_float_symbols import make_float_caf, make_float_wav

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import caf_oracle as co  # noqa: E402

pytestmark = pytest.mark.gpu
CU = os.path.join(ROOT, "convert-utility")
BIN = os.path.join(CU, "alacconvert")


def run(*args):
    p = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    return p.returncode, p.stdout, p.stderr


def on_grid(bits, ch, frames, seed):
    """float32 [ch, frames] on the grid of `bits` bits, using its lowest bit"""
    top = 2 ** (bits - 1)
    s = np.random.default_rng(seed).integers(-top, top, (ch, frames), dtype=np.int64)
    s[0, 0], s[ch - 1, frames - 1] = 1, -top
    return (s.astype(np.float64) / top).astype(np.float32)


def wav_samples(data):
    """an integer WAVE -> (bits, float64 [ch, frames] of sample / 2^(bits - 1)); 20 bits sit left-justified in 3 bytes"""
    assert data[:4] == b"RIFF" and data[8:12] == b"WAVE"
    pos, fmt, pcm = 12, None, None
    while pos + 8 <= len(data):
        tag, size = data[pos:pos + 4], struct.unpack("<I", data[pos + 4:pos + 8])[0]
        if tag == b"fmt ":
            fmt = struct.unpack("<HHIIHH", data[pos + 8:pos + 24])
        elif tag == b"data":
            pcm = data[pos + 8:pos + 8 + size]
        pos += 8 + size + (size & 1)
    ch, bits = fmt[1], fmt[5]
    if bits == 16:
        v = np.frombuffer(pcm, "<i2").astype(np.float64) / 2.0 ** 15
    else:
        assert bits in (20, 24)
        b = np.frombuffer(pcm, np.uint8).reshape(-1, 3).astype(np.int64)
        s = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        v = (s - ((s & 0x800000) << 1)).astype(np.float64) / 2.0 ** 23
    return bits, v.reshape(-1, ch).T


FILES = [  # name, depth, floats -> the file's bytes, the floats
    ("mono16.wav", 16, lambda x: make_float_wav(x), lambda: on_grid(16, 1, 2 * 4096 + 77, 1)),
    ("stereo24.wav", 24, lambda x: make_float_wav(x), lambda: on_grid(24, 2, 3 * 4096 + 5, 2)),
    ("stereo16.wav", 16, lambda x: make_float_wav(x, extensible=True), lambda: on_grid(16, 2, 4096 + 1, 3)),
    ("stereo20be.caf", 20, lambda x: make_float_caf(x, little_endian=False), lambda: on_grid(20, 2, 2 * 4096, 4)),
]


@pytest.fixture(scope="module")
def batch(gpu_ctx, tmp_path_factory):
    subprocess.check_call(["make", "-C", CU, "alacconvert"], stdout=subprocess.DEVNULL)
    d = tmp_path_factory.mktemp("auto")
    items, args = [], []
    for name, depth, write, make in FILES:
        x = make()
        (d / name).write_bytes(write(x))
        items.append((name, depth, x, d / name, d / (name + ".caf")))
        args += [d / name, d / (name + ".caf")]
    rc, out, err = run("--batch", "--float-bits", "auto", *args)
    assert rc == 0, err
    return d, items, out


def test_every_file_at_its_own_depth(batch):
    d, items, out = batch
    for name, depth, x, src, dst in items:
        assert co.get_cookie(dst.read_bytes())[5] == depth, name
        assert f"lossless at {depth} bits: {src}" in out, (name, out)


def test_outputs_decode_to_the_source_floats(batch):
    d, items, _ = batch
    args = []
    for name, depth, x, src, dst in items:
        args += [dst, d / (name + ".back.wav")]
    rc, _, err = run("--batch", *args)
    assert rc == 0, err
    for name, depth, x, src, dst in items:
        bits, v = wav_samples((d / (name + ".back.wav")).read_bytes())
        assert bits == depth and v.shape == x.shape, name
        assert np.array_equal(v.astype(np.float32).view(np.uint32), x.view(np.uint32)), name


def test_sixteen_bit_outputs_are_those_of_float_bits_16(batch):
    d, items, _ = batch
    sixteen = [it for it in items if it[1] == 16]
    args = []
    for name, depth, x, src, dst in sixteen:
        args += [src, d / (name + ".n16.caf")]
    rc, _, err = run("--batch", "--float-bits", 16, *args)
    assert rc == 0 and len(sixteen) == 2, err
    for name, depth, x, src, dst in sixteen:
        assert dst.read_bytes() == (d / (name + ".n16.caf")).read_bytes(), name


def test_a_file_without_a_lossless_depth_is_refused(batch, tmp_path):
    d, items, _ = batch
    t = np.arange(5000, dtype=np.float64)
    x = np.stack([np.sin(t * 0.01), np.cos(t * 0.013)]).astype(np.float32) * np.float32(0.7)
    assert fr.report_depth(fr.report(x)) == 0 and fr.report(x)[4] > 32  # the small samples beside the zero crossings
    (tmp_path / "sine.wav").write_bytes(make_float_wav(x))
    rc, _, err = run("--float-bits", "auto", tmp_path / "sine.wav", tmp_path / "sine.caf")
    assert rc == 1 and not (tmp_path / "sine.caf").exists()
    assert "no lossless bit depth" in err and "need_bits" in err and "over_range 0" in err and "nan 0" in err and "sine.wav" in err
    # beside a good file: the bad one is named, nothing is written
    loud = on_grid(16, 2, 4096, 8)
    loud[1, 100] = 1.0
    (tmp_path / "loud.wav").write_bytes(make_float_wav(loud))
    rc, _, err = run("--batch", "--float-bits", "auto", items[0][3], tmp_path / "good.caf", tmp_path / "loud.wav", tmp_path / "loud.caf")
    assert rc == 1 and "over_range 1" in err and "loud.wav" in err and "mono16" not in err
    assert not (tmp_path / "loud.caf").exists() and not (tmp_path / "good.caf").exists()


def test_auto_with_dither_is_refused(batch, tmp_path):
    d, items, _ = batch
    rc, out, err = run("--float-bits", "auto", "--dither", items[0][3], tmp_path / "o.caf")
    assert rc == 1 and "Usage" in out and "--dither" in err and not (tmp_path / "o.caf").exists()


@pytest.mark.parametrize("flags", [["--verify-source"], ["--segment-packets", 2, "--devices", 1], ["--lpc"]])
def test_auto_takes_the_options_of_a_number(batch, tmp_path, flags):
    d, items, _ = batch
    (name, depth, x, src, dst), (name2, depth2, x2, src2, dst2) = items[1], items[2]  # 24-bit and 16-bit stereo
    rc, _, err = run("--batch", "--float-bits", "auto", *flags, src, tmp_path / "a.caf", src2, tmp_path / "a2.caf")
    assert rc == 0, err
    for s, n, o in ((src, depth, "a.caf"), (src2, depth2, "a2.caf")):
        rc, _, err = run("--batch", "--float-bits", n, *flags, s, tmp_path / ("n" + o))
        assert rc == 0, err
        assert (tmp_path / o).read_bytes() == (tmp_path / ("n" + o)).read_bytes(), (flags, o)
