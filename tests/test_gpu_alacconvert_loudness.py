"""alacconvert --loudness and ALACDecoder::LoudnessBatch on the GPU: a WAV, its CAF and its M4A print the same line but for the
path, and the line holds the restatement's values (tests/loudness_ref.py) to the printed digits; a float WAV is accepted; a
silent file prints -inf; --loudness with any other option exits 1, and so does a damaged file while the other files still get
their lines; --devices 2 prints the same lines; the class measures files whose frames lie back to back and files with a short
packet in their middle alike."""
import math
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import alac_amd
import loudness_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import caf_oracle as co  # noqa: E402

pytestmark = pytest.mark.gpu
CU = os.path.join(ROOT, "convert-utility")
CPP = os.path.join(ROOT, "tests", "cpp")
BIN = os.path.join(CU, "alacconvert")


def run(*args, env=None):
    p = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, **(env or {})))
    return p.returncode, p.stdout, p.stderr


def samples(frames, ch, bits, rate, seed, level=0.4):
    """int64 [frames, ch]: tones and noise at `level` of full scale"""
    rng = np.random.default_rng(seed)
    t = np.arange(frames)[:, None]
    x = level * (0.7 * np.sin(2 * np.pi * (440.0 + 110 * np.arange(ch)[None, :]) * t / rate) + 0.1 * rng.standard_normal((frames, ch)))
    return np.round(x * ((1 << (bits - 1)) - 1)).astype(np.int64)


def pack(s, bits):
    """samples [frames, ch] -> the little-endian bytes of a WAVE's data chunk (16 or 24 bits)"""
    if bits == 16:
        return s.astype("<i2").tobytes()
    return (s & 0xffffff).astype("<u4").view(np.uint8).reshape(-1, 4)[:, :3].tobytes()


def float_wav(x, rate):
    """float32 [frames, ch] -> a WAVE of format tag 3"""
    ch, pcm = x.shape[1], x.astype("<f4").tobytes()
    body = b"WAVE" + b"fmt " + struct.pack("<IHHIIHH", 16, 3, ch, rate, rate * 4 * ch, 4 * ch, 32) + b"data" + struct.pack("<I", len(pcm)) + pcm
    return b"RIFF" + struct.pack("<I", len(body)) + body


def line(x, rate, path):
    """the line alacconvert prints for the values x float64 [frames, ch]"""
    rows, reports = lr.measure(x, rate)
    lufs, peak = lr.integrated(rows, rate // 10), reports[0][2]
    return "%.2f LUFS  %.2f dBFS  %d  %s\n" % (lufs, 20.0 * math.log10(peak) if peak > 0 else -math.inf, x.shape[0], path)


@pytest.fixture(scope="module")
def library(gpu_ctx, tmp_path_factory):
    """sources and their encodes: name -> (path, values float64 [frames, ch], rate)"""
    subprocess.check_call(["make", "-C", CU, "alacconvert"], stdout=subprocess.DEVNULL)
    d = tmp_path_factory.mktemp("loudness")
    files, batch = {}, ["--batch"]
    for name, bits, ch, frames, rate in (("s16", 16, 2, 4096 * 12 + 321, 44100), ("s24", 24, 2, 4096 * 11 + 7, 48000),
                                         ("six", 16, 6, 4096 * 6 + 5, 48000), ("silent", 16, 1, 4096 * 11, 44100),
                                         ("short", 16, 2, 4096 * 3 + 9, 44100)):
        s = samples(frames, ch, bits, rate, bits + ch, 0.0 if name == "silent" else 0.4)
        value = (s.astype(np.float64) * 2.0 ** -(bits - 1), rate)
        wav = d / f"{name}.wav"
        wav.write_bytes(co.make_wav(pack(s, bits), ch, rate, bits))
        files[f"{name}.wav"] = (wav, *value)
        for ext in ("caf", "m4a"):
            batch += [wav, d / f"{name}.{ext}"]
            files[f"{name}.{ext}"] = (d / f"{name}.{ext}", *value)
    rc, _, err = run(*batch)
    assert rc == 0, err
    f = (samples(44100, 2, 24, 44100, 99).astype(np.float32) / np.float32(1 << 23)) * np.float32(1.5)  # floats are not clipped
    f[100, 1] = np.nan  # read as 0.0
    (d / "float.wav").write_bytes(float_wav(f, 44100))
    files["float.wav"] = (d / "float.wav", lr.float_values(f)[0], 44100)
    be = samples(44100, 2, 16, 44100, 7)
    (d / "be.caf").write_bytes(co.make_pcm_caf(be.astype(">i2").tobytes(), 2, 44100, 16, little_endian=False))
    files["be.caf"] = (d / "be.caf", be.astype(np.float64) * 2.0 ** -15, 44100)
    return files


def lines_of(files, names):
    return "".join(line(files[n][1], files[n][2], files[n][0]) for n in names)


def test_source_and_every_encode_print_the_restatements_line(library):
    names = sorted(library)  # files of different cookies, depths, rates and channel counts, WAV, CAF, M4A, float, in one call
    rc, out, err = run("--loudness", *[library[n][0] for n in names])
    assert rc == 0, err
    print(out)
    assert out == lines_of(library, names)
    got = {n: ln.rsplit("  ", 1)[0] for n, ln in zip(names, out.splitlines())}
    for stem in ("s16", "s24", "six", "silent", "short"):
        assert got[f"{stem}.wav"] == got[f"{stem}.caf"] == got[f"{stem}.m4a"], stem
    assert got["silent.wav"].startswith("-inf LUFS  -inf dBFS  ")
    assert got["short.wav"].startswith("-inf LUFS  ") and "-inf dBFS" not in got["short.wav"]  # under 400 ms: a peak, no loudness
    assert not got["float.wav"].startswith("-inf") and not got["six.m4a"].startswith("-inf")


def test_devices(library):
    names = sorted(library)
    rc, out, err = run("--loudness", library["s24.m4a"][0])
    assert rc == 0 and out == lines_of(library, ["s24.m4a"]), err
    rc, out, err = run("--loudness", "--devices", 2, *[library[n][0] for n in names], env={"ALACCONVERT_SHARE_DEVICES": "1"})
    assert rc == 0, err
    assert out == lines_of(library, names)


def test_no_other_option_and_the_usage_text_unchanged(library):
    f = library["s16.wav"][0]
    usage = run()[1]
    assert "--loudness" not in usage
    for extra in (["--batch"], ["--lpc"], ["--verify"], ["--verify-source"], ["--crc"], ["--compare"], ["--dither"],
                  ["--segment-packets", 4], ["--float-bits", 16], ["--bits", 16], ["--crc-check", f]):
        rc, out, err = run("--loudness", *extra, f)
        assert rc == 1 and "LUFS" not in out, extra
    rc, out, err = run("--loudness")
    assert rc == 1 and out == usage


def test_a_damaged_file_is_named_and_the_others_still_print(library, tmp_path):
    raw = bytearray(library["s16.caf"][0].read_bytes())
    at = raw.rindex(b"data") + 4 + 8 + 4  # chunk size and edit count, then the first packet
    raw[at] = 0x40  # a coupling channel element: not decodable
    bad = tmp_path / "damaged.caf"
    bad.write_bytes(bytes(raw))
    cut = tmp_path / "cut.caf"
    cut.write_bytes(bytes(raw[:40]))
    rc, out, err = run("--loudness", library["s16.wav"][0], bad, cut, tmp_path / "missing.caf", library["s24.m4a"][0])
    assert rc == 1
    assert out == lines_of(library, ["s16.wav", "s24.m4a"])
    assert str(bad) in err and str(cut) in err


@pytest.fixture(scope="module")
def harness(gpu_ctx):
    subprocess.check_call(["make", "-C", CPP, "-f", "loudness.mk", "loudness"], stdout=subprocess.DEVNULL)
    return os.path.join(CPP, "loudness")


def test_class_level_loudness_batch(gpu_ctx, harness, tmp_path):
    """ALACDecoder::LoudnessBatch over 14 packets of 16-bit stereo, the last one short: as one file, as three files of which the
    middle one is empty, and with the short packet moved into the middle of a file (its frames are copied together first)."""
    fmt = alac_amd.make_format(4096, 16, 2, 44100)
    total = 13 * 4096 + 1234
    s = samples(total, 2, 16, 44100, 3)
    pcm = np.frombuffer(pack(s, 16), np.uint8)
    stream, sizes, _ = gpu_ctx.encode_host(fmt, pcm, total, segment_packets=0)
    npk = len(sizes)
    assert npk == 14
    offs = np.concatenate([[0], np.cumsum(sizes.astype(np.int64))])
    (tmp_path / "cookie").write_bytes(gpu_ctx.magic_cookie(fmt).tobytes())
    x = s.astype(np.float64) * 2.0 ** -15

    def run_harness(order, first):
        (tmp_path / "stream").write_bytes(b"".join(stream[offs[p]:offs[p + 1]].tobytes() for p in order))
        (tmp_path / "sizes").write_bytes(np.array([sizes[p] for p in order], dtype=np.uint32).tobytes())
        (tmp_path / "first").write_bytes(np.array(first, dtype=np.uint32).tobytes())
        p = subprocess.run([harness] + [str(tmp_path / n) for n in ("cookie", "stream", "sizes", "first")], capture_output=True,
                           text=True, timeout=120)
        assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
        lines = p.stdout.split("\n")
        return [tuple(float(v) for v in ln.split()) for ln in lines[:len(first) - 1]], lines[len(first) - 1:len(first) + 1]

    def frames_of(packets):
        return np.concatenate([x[p * 4096:(p + 1) * 4096] for p in packets]) if len(packets) else x[:0]

    def want(packets):
        v = frames_of(packets)
        rows, reports = lr.measure(v, 44100)
        return lr.integrated(rows, 4410), reports[0][2]

    def same(got, packets):
        lufs, peak = want(packets)
        assert got[1] == peak and (got[0] == lufs if math.isinf(lufs) else abs(got[0] - lufs) <= 1e-6), (got, lufs, peak)

    whole = list(range(npk))
    got, tail = run_harness(whole, [0, npk])
    same(got[0], whole)
    assert tail == [f"frames {total}", "bad 0"]
    got, tail = run_harness(whole, [0, 8, 8, npk])
    same(got[0], whole[:8]), same(got[1], []), same(got[2], whole[8:])
    got, tail = run_harness([], [0, 0, 0])  # files without packets: nothing to decode, nothing to measure
    assert got == [(-math.inf, 0.0), (-math.inf, 0.0)] and tail == ["frames 0", "bad 0"]
    order = whole[8:] + whole[:8]  # the short packet in the middle of the one file
    got, tail = run_harness(order, [0, npk])
    same(got[0], order)
    assert tail == [f"frames {total}", "bad 0"]
