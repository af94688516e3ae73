"""alacconvert --rate R on the GPU: a 16-bit stereo WAV at 44.1 kHz through --rate 48000 and a 24-bit one at 96 kHz through
--rate 44100 --float-bits 24 give files whose header carries R, whose frame count is ceil(N L / M) and which decode to the
restatement of the resampling rule (tests/resample_ref.py, with the library's coefficients) pushed through the quantization
rule of alac_hip_encode_float — but for the samples the restatement itself flags as within the accepted distance of a rounding
boundary, at most one per file.  A file gives the same bytes alone and in --batch; a file already at R gives the bytes of the
run without --rate; the refused combinations exit with the usage text and write nothing; --dither --dither-seed 7 gives what
encode_float(dither="tpdf", seed=7) gives on the resampled floats."""
import io
import os
import subprocess
import wave

import numpy as np
import pytest
import torch

import alac_amd
import resample_ref as rr
from test_gpu_alacconvert_loudness import CU, co, float_wav, pack, run

pytestmark = pytest.mark.gpu

# (name, bits, in rate, out rate, options, seed, amplitude): 0.25 s of stereo noise; the seeds are those for which at most
# one sample of the restatement lies within the accepted distance of a rounding boundary (counted on the CPU; the test
# asserts it; the accepted distance is 2^-10 of a 16-bit step at -30 dBFS and 2^-10 of a 24-bit step at -80 dBFS, so louder
# signals have more of them)
CASES = [("cd", 16, 44100, 48000, [], 1, 0.03), ("master", 24, 96000, 44100, ["--float-bits", 24], 0, 0.0001)]


def source(bits, rate, seed, scale):
    """int64 [frames, 2]: 0.25 s"""
    frames = rate // 4
    return np.rint(np.random.default_rng(seed).uniform(-scale, scale, (frames, 2)) * 2.0 ** (bits - 1)).astype(np.int64)


def decoded(path, tmp):
    """an ALAC file through alacconvert's decode -> (rate, int64 [frames, ch])"""
    out = tmp / (os.path.basename(str(path)) + ".decoded.wav")
    rc, _, err = run(path, out)
    assert rc == 0, err
    with wave.open(io.BytesIO(out.read_bytes())) as w:
        rate, ch, width, n = w.getframerate(), w.getnchannels(), w.getsampwidth(), w.getnframes()
        raw = np.frombuffer(w.readframes(n), np.uint8)
    if width == 2:
        v = raw.view("<i2").astype(np.int64)
    else:
        b = raw.reshape(-1, 3).astype(np.int64)
        v = ((b[:, 0] | b[:, 1] << 8 | b[:, 2] << 16) ^ 0x800000) - 0x800000
    return rate, v.reshape(n, ch)


@pytest.fixture(scope="module")
def files(gpu_ctx, tmp_path_factory):
    subprocess.check_call(["make", "-C", CU, "alacconvert"], stdout=subprocess.DEVNULL)
    d = tmp_path_factory.mktemp("rate")
    out = {}
    for name, bits, rate, _, _, seed, scale in CASES:
        s = source(bits, rate, seed, scale)
        (d / f"{name}.wav").write_bytes(co.make_wav(pack(s, bits), 2, rate, bits))
        out[name] = (d / f"{name}.wav", s)
    return d, out


@pytest.mark.parametrize("name,bits,in_rate,out_rate,options,seed,scale", CASES)
def test_rate_gives_the_restatement_quantized(files, tmp_path, name, bits, in_rate, out_rate, options, seed, scale):
    d, srcs = files
    wav, s = srcs[name]
    L, M, coefs = alac_amd.resample_filter(in_rate, out_rate)
    rc, _, err = run("--rate", out_rate, *options, wav, tmp_path / "out.caf")
    assert rc == 0 and "Warning" not in err, err
    rate, got = decoded(tmp_path / "out.caf", tmp_path)
    assert rate == out_rate  # the header carries R
    assert got.shape == (rr.out_frames(s.shape[0], L, M), 2)
    x = s.astype(np.float64) * 2.0 ** -(bits - 1)
    ref = rr.segment(x, L, M, coefs)
    excused = rr.near_boundary(ref, rr.bound(coefs, np.abs(x).max()), bits)
    print(name, "samples near a rounding boundary:", int(excused.sum()), "of", excused.size)
    assert int(excused.sum()) <= 1
    want = rr.quantize(ref.astype(np.float32), bits)
    assert np.array_equal(got[~excused], want[~excused]) and np.abs(got - want).max() <= 1
    # the same bytes alone and in --batch: next to itself, and (without --float-bits) next to a file of another rate and depth
    extra = [srcs["master"][0], tmp_path / "b2.caf"] if name == "cd" else []
    rc, _, err = run("--batch", "--rate", out_rate, *options, wav, tmp_path / "b1.caf", *extra, wav, tmp_path / "b3.m4a")
    assert rc == 0, err
    assert (tmp_path / "b1.caf").read_bytes() == (tmp_path / "out.caf").read_bytes()
    rate, again = decoded(tmp_path / "b3.m4a", tmp_path)
    assert rate == out_rate and np.array_equal(again, got)
    if extra:
        rate, other = decoded(tmp_path / "b2.caf", tmp_path)
        assert rate == out_rate and other.shape == (srcs["master"][1].shape[0] // 2, 2) and int(np.abs(other).max()) < 1 << 23


def test_a_file_already_at_the_rate_is_encoded_as_without_rate(files, tmp_path):
    d, srcs = files
    wav = srcs["cd"][0]
    rc, _, err = run("--rate", 44100, wav, tmp_path / "same.caf")
    assert rc == 0 and str(wav) in err and "44100" in err
    rc, _, _ = run(wav, tmp_path / "plain.caf")
    assert rc == 0
    assert (tmp_path / "same.caf").read_bytes() == (tmp_path / "plain.caf").read_bytes()
    # next to a file that is resampled, in one batch
    rc, _, err = run("--batch", "--rate", 44100, wav, tmp_path / "s.caf", srcs["master"][0], tmp_path / "m.caf")
    assert rc == 0, err
    assert (tmp_path / "s.caf").read_bytes() == (tmp_path / "plain.caf").read_bytes()
    assert decoded(tmp_path / "m.caf", tmp_path)[0] == 44100


def test_refused_combinations_print_the_usage_text_and_write_nothing(files, tmp_path):
    d, srcs = files
    wav = srcs["cd"][0]
    usage = run()[1]
    assert "--rate" not in usage
    rc, _, _ = run(wav, tmp_path / "alac.caf")
    assert rc == 0
    out = tmp_path / "never.caf"
    fl = tmp_path / "float.wav"
    fl.write_bytes(float_wav((srcs["cd"][1][:3000] / 32768.0).astype(np.float32), 44100))
    for args in (["--rate", 48000, "--bits", 24, wav, out], ["--rate", 48000, "--float-bits", "auto", fl, out],
                 ["--rate", 48000, "--verify", wav, out], ["--rate", 48000, "--float-bits", 16, "--verify-source", fl, out],
                 ["--rate", 48000, "--compare", tmp_path / "alac.caf", wav], ["--rate", 48000, "--crc", wav],
                 ["--rate", 48000, "--loudness", wav], ["--rate", 48000, tmp_path / "alac.caf", tmp_path / "never.wav"],
                 ["--rate", 48001, wav, out], ["--rate", 7990, wav, out], ["--rate", 384000, wav, out], ["--rate", wav, out],
                 ["--rate", 0, wav, out]):
        rc, text, err = run(*args)
        assert rc == 1 and text.replace("Input file: %s\nOutput file: %s\n" % (args[-2], args[-1]), "").startswith(usage), (args, text, err)
        assert not out.exists() and not (tmp_path / "never.wav").exists(), args
    # a float input needs --float-bits N
    rc, _, err = run("--rate", 48000, fl, out)
    assert rc == 1 and "--float-bits" in err and not out.exists()
    rc, _, err = run("--rate", 48000, "--float-bits", 16, fl, out)
    assert rc == 0 and decoded(out, tmp_path)[0] == 48000


def test_dither_gives_what_encode_float_gives_on_the_resampled_floats(gpu_ctx, files, tmp_path):
    d, srcs = files
    wav, s = srcs["master"]
    rc, _, err = run("--rate", 48000, "--float-bits", 16, "--dither", "--dither-seed", 7, wav, tmp_path / "d.caf")
    assert rc == 0, err
    rate, got = decoded(tmp_path / "d.caf", tmp_path)
    x = torch.from_numpy((s << 8).astype(np.int32)).to(gpu_ctx.device).t()  # the file's 24 bits, left-justified
    y, _ = gpu_ctx.resample_int(x, 96000, 48000, bits=24)
    fmt = alac_amd.make_format(4096, 16, 2, 48000)
    frames = y.shape[1]
    packets = -(-frames // 4096)
    seg = torch.tensor([0, packets], dtype=torch.int32, device=gpu_ctx.device)
    bufs = gpu_ctx.encode_float(fmt, y, seg_first=seg, max_segment_packets=packets, dither="tpdf", seed=7)
    gpu_ctx.synchronize()
    total = int(bufs["offsets"][-1].item())
    f, ns, st, _ = gpu_ctx.decode_float(gpu_ctx.magic_cookie(fmt), bufs["out"][:total], bufs["offsets"], packets)
    gpu_ctx.synchronize()
    assert int(st.abs().sum()) == 0
    want = np.rint(f.cpu().numpy()[:, :frames].astype(np.float64) * 32768.0).astype(np.int64).T
    assert rate == 48000 and np.array_equal(got, want)
    # ... and the stream inside the file is that stream, byte for byte
    assert bufs["out"][:total].cpu().numpy().tobytes() in (tmp_path / "d.caf").read_bytes()
    plain = tmp_path / "p.caf"
    assert run("--rate", 48000, "--float-bits", 16, wav, plain)[0] == 0
    assert not np.array_equal(decoded(plain, tmp_path)[1], got)  # the dither did something
