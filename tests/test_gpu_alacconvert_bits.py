"""alacconvert --bits N / --bits auto on the GPU: a 24-bit file of 16-bit samples comes out as the 16-bit file, with a number
and with auto; a genuine 24-bit file is left alone by auto; widening decodes to the shifted samples; a mixed --batch under
auto gives 16- and 24-bit streams side by side; --dither is reproducible alone and in --batch, passes --verify and decodes to
the integer rule's samples (pcm_requant_ref.py); a dual-mono file is noted."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import pcm_requant_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import caf_oracle as co  # noqa: E402

pytestmark = pytest.mark.gpu
CU = os.path.join(ROOT, "convert-utility")
BIN = os.path.join(CU, "alacconvert")
FRAME = 4096
N = FRAME + 77  # one full packet and 77 frames


def run(*args):
    p = subprocess.run([BIN] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    return p.returncode, p.stdout, p.stderr


def wav(s, bits, rate=44100):
    """int samples [ch, frames] -> an integer WAVE of `bits` bits"""
    return co.make_wav(pr.pack(s, bits).tobytes(), s.shape[0], rate, bits)


def wav_samples(data):
    """an integer WAVE -> (bits, int64 [ch, frames]); 20 bits sit left-justified in 3 bytes"""
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
        v = np.frombuffer(pcm, "<i2").astype(np.int64)
    else:
        assert bits in (20, 24)
        b = np.frombuffer(pcm, np.uint8).reshape(-1, 3).astype(np.int64)
        s = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        v = (s - ((s & 0x800000) << 1)) >> (24 - bits)
    return bits, v.reshape(-1, ch).T


def music(ch, bits, seed):
    """[ch, N] samples of `bits` bits that use the lowest one: a slow wave plus noise, so that the predictor has work"""
    rng = np.random.default_rng(seed)
    t = np.arange(N)
    top = 1 << (bits - 1)
    s = np.stack([np.sin(t * (0.01 + 0.003 * c)) * 0.4 * top for c in range(ch)]) + rng.integers(-top // 64, top // 64, (ch, N))
    s = np.clip(np.rint(s), -top, top - 1).astype(np.int64)
    s[0, 0], s[ch - 1, N - 1] = 1, -top
    return s


@pytest.fixture(scope="module")
def files(gpu_ctx, tmp_path_factory):
    subprocess.check_call(["make", "-C", CU, "alacconvert"], stdout=subprocess.DEVNULL)
    d = tmp_path_factory.mktemp("bits")
    s16, s24 = music(2, 16, 1), music(2, 24, 2)
    mono = music(1, 16, 3)
    content = {
        "s16.wav": wav(s16, 16), "s16in24.wav": wav(s16 << 8, 24), "s24.wav": wav(s24, 24),
        "dual.wav": wav(np.stack([s24[0] >> 4 << 4, s24[0] >> 4 << 4]), 24),  # dual mono, and 20-bit material
        "mono16in24.wav": wav(mono << 8, 24),
    }
    for name, data in content.items():
        (d / name).write_bytes(data)
    rc, _, err = run(d / "s16.wav", d / "s16.plain.caf")
    assert rc == 0, err
    rc, _, err = run(d / "s24.wav", d / "s24.plain.caf")
    assert rc == 0, err
    return d, {"s16": s16, "s24": s24, "mono": mono}


def decoded(d, name):
    rc, _, err = run(d / name, d / (name + ".back.wav"))
    assert rc == 0, err
    return wav_samples((d / (name + ".back.wav")).read_bytes())


def test_sixteen_bits_in_24_bit_containers_come_out_as_the_16_bit_file(files):
    d, _ = files
    rc, out, err = run("--bits", 16, d / "s16in24.wav", d / "n16.caf")
    assert rc == 0 and err == "", err
    assert (d / "n16.caf").read_bytes() == (d / "s16.plain.caf").read_bytes()
    assert len((d / "n16.caf").read_bytes()) < len((d / "s24.plain.caf").read_bytes())


def test_auto_names_16_bits_and_writes_the_same_file(files):
    d, _ = files
    rc, out, err = run("--bits", "auto", d / "s16in24.wav", d / "a16.caf")
    assert rc == 0, err
    assert f"lossless at 16 bits: {d / 's16in24.wav'}" in out and "channels identical" not in out, out
    assert (d / "a16.caf").read_bytes() == (d / "s16.plain.caf").read_bytes()
    # an M4A output too
    rc, _, err = run("--bits", "auto", d / "s16in24.wav", d / "a16.m4a")
    assert rc == 0, err
    rc, _, err = run(d / "s16.wav", d / "p16.m4a")
    assert rc == 0 and (d / "a16.m4a").read_bytes() == (d / "p16.m4a").read_bytes()


def test_auto_leaves_a_genuine_24_bit_file_alone(files):
    d, _ = files
    rc, out, err = run("--bits", "auto", d / "s24.wav", d / "a24.caf")
    assert rc == 0 and f"lossless at 24 bits: {d / 's24.wav'}" in out, (out, err)
    assert (d / "a24.caf").read_bytes() == (d / "s24.plain.caf").read_bytes()
    rc, _, err = run("--bits", 24, d / "s24.wav", d / "n24.caf")  # ... as does its own depth as a number
    assert rc == 0 and (d / "n24.caf").read_bytes() == (d / "s24.plain.caf").read_bytes()


def test_widening_decodes_to_the_shifted_samples(files):
    d, s = files
    rc, _, err = run("--bits", 24, "--verify", d / "s16.wav", d / "w24.caf")
    assert rc == 0, err
    bits, v = decoded(d, "w24.caf")
    assert bits == 24 and np.array_equal(v, s["s16"] << 8)


def test_a_mixed_batch_under_auto(files):
    d, s = files
    names = ["s16in24.wav", "s24.wav", "mono16in24.wav", "dual.wav", "s16.wav"]
    args = []
    for n in names:
        args += [d / n, d / (n + ".auto.caf")]
    rc, out, err = run("--batch", "--bits", "auto", "--verify", *args)
    assert rc == 0, err
    depths = [co.get_cookie((d / (n + ".auto.caf")).read_bytes())[5] for n in names]
    assert depths == [16, 24, 16, 20, 16]
    for n, depth in zip(names, depths):
        assert f"lossless at {depth} bits" in [line for line in out.splitlines() if line.endswith(str(d / n))][-1]
    assert (d / "s16in24.wav.auto.caf").read_bytes() == (d / "s16.plain.caf").read_bytes()
    assert (d / "s16.wav.auto.caf").read_bytes() == (d / "s16.plain.caf").read_bytes()
    assert (d / "s24.wav.auto.caf").read_bytes() == (d / "s24.plain.caf").read_bytes()
    bits, v = decoded(d, "mono16in24.wav.auto.caf")
    assert bits == 16 and np.array_equal(v, s["mono"])
    bits, v = decoded(d, "dual.wav.auto.caf")
    assert bits == 20 and np.array_equal(v[0], s["s24"][0] >> 4) and np.array_equal(v[0], v[1])


def test_a_dual_mono_file_is_noted(files):
    d, _ = files
    rc, out, err = run("--bits", "auto", d / "dual.wav", d / "dual.caf")
    assert rc == 0, err
    assert f"lossless at 20 bits, channels identical: {d / 'dual.wav'}" in out, out
    # the encode does not change for it
    rc, _, err = run("--bits", 20, d / "dual.wav", d / "dual20.caf")
    assert rc == 0 and (d / "dual.caf").read_bytes() == (d / "dual20.caf").read_bytes()


def test_dither_is_reproducible_verifies_and_follows_the_rule(files):
    d, s = files
    flags = ["--bits", 16, "--dither", "--dither-seed", 7]
    for out in ("d1.caf", "d2.caf"):
        rc, _, err = run(*flags, "--verify", d / "s24.wav", d / out)
        assert rc == 0, err
    rc, _, err = run("--batch", *flags, d / "s16in24.wav", d / "b0.caf", d / "s24.wav", d / "b1.caf", d / "dual.wav", d / "b2.caf")
    assert rc == 0, err
    one = (d / "d1.caf").read_bytes()
    assert one == (d / "d2.caf").read_bytes() == (d / "b1.caf").read_bytes()
    rc, _, err = run("--bits", 16, d / "s24.wav", d / "plain16.caf")
    assert rc == 0 and (d / "plain16.caf").read_bytes() != one
    rc, _, err = run("--bits", 16, "--dither", "--dither-seed", 8, d / "s24.wav", d / "d8.caf")
    assert rc == 0 and (d / "d8.caf").read_bytes() != one
    # the decoded samples are the integer rule's with that seed, the file's frames counted from 0
    padded = np.zeros((2, 2 * FRAME), np.int64)
    padded[:, :N] = s["s24"]
    want, _ = pr.convert(padded, 24, 3, True, 16, FRAME, num_samples=[FRAME, N - FRAME], seed=7)
    bits, v = decoded(d, "d1.caf")
    assert bits == 16 and np.array_equal(v, want[:, :N])
    plain, _ = pr.convert(padded, 24, 3, True, 16, FRAME, num_samples=[FRAME, N - FRAME])
    bits, v = decoded(d, "plain16.caf")
    assert bits == 16 and np.array_equal(v, plain[:, :N])


def test_a_reduction_that_clips_warns_and_succeeds(files, tmp_path):
    d, s = files
    loud = s["s24"].copy()
    loud[1, 100] = (1 << 23) - 1  # rounds up to 2^15: clipped
    (tmp_path / "loud.wav").write_bytes(wav(loud, 24))
    rc, _, err = run("--bits", 16, "--verify", tmp_path / "loud.wav", tmp_path / "loud.caf")
    assert rc == 0 and "Warning: 1 samples clipped to 16 bits" in err and "loud.wav" in err, err
    assert (tmp_path / "loud.caf").exists()


@pytest.mark.parametrize("flags", [["--lpc"], ["--segment-packets", 1, "--devices", 1], ["--verify", "--lpc"]])
def test_bits_takes_the_other_encode_options(files, tmp_path, flags):
    """under --lpc, --segment-packets and --devices the converted file is still the one the 16-bit file gives, and auto is N"""
    d, _ = files
    rc, _, err = run("--batch", *flags, d / "s16.wav", tmp_path / "plain.caf", d / "s24.wav", tmp_path / "plain24.caf")
    assert rc == 0, err
    rc, _, err = run("--batch", "--bits", "auto", *flags, d / "s16in24.wav", tmp_path / "auto.caf", d / "s24.wav", tmp_path / "auto24.caf")
    assert rc == 0, err
    rc, _, err = run("--batch", "--bits", 16, *flags, d / "s16in24.wav", tmp_path / "n16.caf")
    assert rc == 0, err
    assert (tmp_path / "auto.caf").read_bytes() == (tmp_path / "n16.caf").read_bytes() == (tmp_path / "plain.caf").read_bytes()
    assert (tmp_path / "auto24.caf").read_bytes() == (tmp_path / "plain24.caf").read_bytes()
