"""alacconvert --crc and --crc-check on the GPU: a WAV, its CAF and M4A encodes and an --lpc encode print the CRC-32 Python
computes over the WAV's data chunk; files of different cookies in one call; --devices; the check flow (OK, FAILED after one
flipped payload byte, FAILED open); the usage errors; and a plain encode and decode that write what they always wrote."""
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import caf_oracle as co  # noqa: E402
from container_lib import Container, music_like  # noqa: E402
from test_container import oracle_codec  # noqa: E402

pytestmark = pytest.mark.gpu
CU = os.path.join(ROOT, "convert-utility")
BIN = os.path.join(CU, "alacconvert")


def run(*args, env=None):
    p = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, **(env or {})))
    return p.returncode, p.stdout, p.stderr


def pcm20(frames, ch, seed):
    """20-bit samples left-justified in 3-byte containers"""
    rng = np.random.default_rng(seed)
    t = np.arange(frames)
    v = np.stack([np.round((0.3 * np.sin(2 * np.pi * (300.0 + 90 * c) * t / 44100.0) + 0.02 * rng.standard_normal(frames)) * ((1 << 19) - 1))
                  for c in range(ch)], axis=1).astype(np.int64)
    return ((v << 4) & 0xffffff).astype("<u4").view(np.uint8).reshape(-1, 4)[:, :3].tobytes()


def wav_of(pcm, ch, rate, bits):
    bpf = ch * ((bits + 7) // 8)  # 20 bits: 3-byte containers
    body = b"WAVE" + b"fmt " + struct.pack("<IHHIIHH", 16, 1, ch, rate, rate * bpf, bpf, bits) + b"data" + struct.pack("<I", len(pcm)) + pcm
    return b"RIFF" + struct.pack("<I", len(body)) + body


@pytest.fixture(scope="module")
def library(gpu_ctx, tmp_path_factory):
    """three sources and their encodes, made with two conversions: name -> (path, crc32 of the PCM, frames)"""
    subprocess.check_call(["make", "-C", CU, "alacconvert"], stdout=subprocess.DEVNULL)
    d = tmp_path_factory.mktemp("crc")
    files, plain, lpc = {}, ["--batch"], ["--lpc", "--batch"]
    for name, bits, ch, frames, rate in (("s16", 16, 2, 4096 * 3 + 321, 44100), ("s24", 24, 2, 4096 * 2 + 7, 48000), ("m20", 20, 1, 4096 + 40, 44100)):
        pcm = pcm20(frames, ch, 5) if bits == 20 else music_like(frames, ch, bits, bits + ch)
        wav = d / f"{name}.wav"
        wav.write_bytes(wav_of(pcm, ch, rate, bits))
        value = (zlib.crc32(pcm), frames)
        files[f"{name}.wav"] = (wav, *value)
        for ext in ("caf", "m4a"):
            plain += [wav, d / f"{name}.{ext}"]
            files[f"{name}.{ext}"] = (d / f"{name}.{ext}", *value)
        lpc += [wav, d / f"{name}_lpc.caf"]
        files[f"{name}_lpc.caf"] = (d / f"{name}_lpc.caf", *value)
        if bits == 16:  # big-endian PCM in CAF: swapped on the way in, as the encode path does
            be = d / f"{name}_be.caf"
            be.write_bytes(co.make_pcm_caf(np.frombuffer(pcm, "<i2").astype(">i2").tobytes(), ch, rate, bits, little_endian=False))
            files[f"{name}_be.caf"] = (be, *value)
    for cmd in (plain, lpc):
        rc, _, err = run(*cmd)
        assert rc == 0, err
    return files


def lines_of(files, names):
    return "".join(f"{files[n][1]:08x}  {files[n][2]}  {files[n][0]}\n" for n in names)


def test_source_and_every_encode_print_the_crc_of_the_data_chunk(library):
    names = sorted(library)  # 16-, 24- and 20-bit files of different cookies and sample rates, WAV, CAF, M4A, in one call
    rc, out, err = run("--crc", *[library[n][0] for n in names])
    assert rc == 0, err
    assert out == lines_of(library, names)
    # one file alone, and the files dealt to two workers: the same lines in the same order
    rc, out, err = run("--crc", library["s24.m4a"][0])
    assert rc == 0 and out == lines_of(library, ["s24.m4a"]), err
    rc, out, err = run("--crc", "--devices", 2, *[library[n][0] for n in names], env={"ALACCONVERT_SHARE_DEVICES": "1"})
    assert rc == 0, err
    assert out == lines_of(library, names)


def test_crc_check_round_trip_and_failures(library, tmp_path):
    names = sorted(library)
    listing = tmp_path / "library.crc"
    listing.write_text(lines_of(library, names))
    rc, out, err = run("--crc-check", listing)
    assert rc == 0, err
    assert out == "".join(f"{library[n][0]}: OK\n" for n in names)
    # one flipped byte in the middle of a packet's payload
    good = library["s16.caf"][0].read_bytes()
    _, sizes, dpos = Container().parse_alac_caf(good)
    at = dpos + int(sizes[0]) + int(sizes[1]) // 2
    bad = tmp_path / "flipped.caf"
    bad.write_bytes(good[:at] + bytes([good[at] ^ 0x10]) + good[at + 1:])
    listing.write_text(lines_of(library, ["s24.wav"]) + f"{library['s16.caf'][1]:08x}  {library['s16.caf'][2]}  {bad}\n"
                       + f"00000000  1  {tmp_path / 'missing.caf'}\n" + lines_of(library, ["m20.m4a"]))
    rc, out, err = run("--crc-check", listing)
    assert rc == 1
    assert out == f"{library['s24.wav'][0]}: OK\n{bad}: FAILED\n{tmp_path / 'missing.caf'}: FAILED open\n{library['m20.m4a'][0]}: OK\n"
    # --crc itself on the two: the good lines, the bad ones named on stderr, exit 1
    rc, out, err = run("--crc", library["s24.wav"][0], tmp_path / "missing.caf")
    assert rc == 1 and out == lines_of(library, ["s24.wav"]) and "missing.caf" in err
    # a wrong frame count fails as a wrong value does
    listing.write_text(f"{library['s24.wav'][1]:08x}  {library['s24.wav'][2] + 1}  {library['s24.wav'][0]}\n")
    rc, out, _ = run("--crc-check", listing)
    assert rc == 1 and out == f"{library['s24.wav'][0]}: FAILED\n"


def test_float_input_is_refused(library, tmp_path):
    from test_encode_float_symbols import make_float_wav
    src = tmp_path / "f.wav"
    src.write_bytes(make_float_wav(np.zeros((2, 100), dtype=np.float32)))
    rc, out, err = run("--crc", src)
    assert rc == 1 and out == "" and "float" in err


@pytest.mark.parametrize("extra", [["--batch"], ["--lpc"], ["--verify"], ["--verify-source"], ["--compare"], ["--float-bits", "16"],
                                   ["--float-bits", "auto"], ["--dither"], ["--segment-packets", "2"]],
                         ids=lambda v: v[0])
def test_both_options_stand_alone(library, tmp_path, extra):
    listing = tmp_path / "l.crc"
    listing.write_text(lines_of(library, ["s16.wav"]))
    for mode in (["--crc", library["s16.wav"][0]], ["--crc-check", listing]):
        rc, out, _ = run(*extra, *mode)
        assert rc == 1 and out.startswith("Usage:"), (extra, mode)
    rc, out, _ = run("--crc", library["s16.wav"][0], "--crc-check", listing)
    assert rc == 1 and out.startswith("Usage:")
    assert run("--crc")[0] == 1 and run("--crc-check", listing, library["s16.wav"][0])[0] == 1


def test_plain_conversions_write_what_they_wrote(library, oracle, tmp_path):
    pcm = music_like(4096 * 2 + 77, 2, 16, 3)
    wav = co.make_wav(pcm, 2, 44100, 16)
    src, caf, back = tmp_path / "in.wav", tmp_path / "out.caf", tmp_path / "back.wav"
    src.write_bytes(wav)
    rc, out, err = run(src, caf)
    assert rc == 0 and out == f"Input file: {src}\nOutput file: {caf}\n", err
    cookie, enc, dec = oracle_codec(oracle, 16, 2, 44100)
    want = co.encode_file(wav, cookie, enc)
    assert caf.read_bytes() == want
    assert run(caf, back)[0] == 0
    assert back.read_bytes() == co.decode_file(want, True, dec)
