"""alacconvert --loudness --true-peak and ALACDecoder::LoudnessTruePeakBatch on the GPU: a 16-bit WAV, a float WAV and two ALAC
files of one cookie print the restatement's true peak (tests/true_peak_ref.py) to the printed digits in a dBTP column of its
own, and the other columns are what --loudness alone prints; a damaged ALAC file in the same call is named and does not stop the
others; --true-peak alone is refused with the usage text; the class gives the values LoudnessBatch gives plus the restatement's
true peak, for a batch without packets and a file with a short packet in its middle too."""
import math
import os
import subprocess

import numpy as np
import pytest

import alac_amd
import loudness_ref as lr
import true_peak_ref as tr
from test_gpu_alacconvert_loudness import CPP, CU, co, float_wav, pack, run, samples

pytestmark = pytest.mark.gpu


def true_peak_of(x, rate):
    """x float64 [frames, ch] -> the true peak over the channels, with the library's coefficients"""
    return tr.measure(x, rate, coefs=alac_amd.true_peak_filter(rate)[1])[1][0][0]


@pytest.fixture(scope="module")
def library(gpu_ctx, tmp_path_factory):
    """name -> (path, values float64 [frames, ch], rate): a 16-bit WAV, a float WAV, two ALAC files of one cookie"""
    subprocess.check_call(["make", "-C", CU, "alacconvert"], stdout=subprocess.DEVNULL)
    d = tmp_path_factory.mktemp("true_peak")
    files, batch = {}, ["--batch"]
    for name, frames, seed in (("a", 4096 * 5 + 321, 5), ("b", 4096 * 3 + 7, 6)):
        s = samples(frames, 2, 16, 44100, seed)
        # the case-16 signal in front: fs/4 sampled 45 degrees off its crests, so that the two peaks differ by 3 dB
        n = np.arange(2000)
        s[:2000, 0] = np.round(0.9 * 32767 * np.sin(2 * np.pi * n / 4 + np.pi / 4))
        wav = d / f"{name}.wav"
        wav.write_bytes(co.make_wav(pack(s, 16), 2, 44100, 16))
        files[f"{name}.wav"] = (wav, s.astype(np.float64) * 2.0 ** -15, 44100)
        batch += [wav, d / f"{name}.caf"]
        files[f"{name}.caf"] = (d / f"{name}.caf", s.astype(np.float64) * 2.0 ** -15, 44100)
    rc, _, err = run(*batch)
    assert rc == 0, err
    f = (samples(30000, 2, 24, 48000, 99).astype(np.float32) / np.float32(1 << 23)) * np.float32(1.5)  # floats are not clipped
    f[100, 1] = np.nan  # read as 0.0
    (d / "float.wav").write_bytes(float_wav(f, 48000))
    files["float.wav"] = (d / "float.wav", lr.float_values(f)[0], 48000)
    return files


def test_the_true_peak_column_and_the_other_columns(library, tmp_path):
    raw = bytearray(library["a.caf"][0].read_bytes())
    at = raw.rindex(b"data") + 4 + 8 + 4  # chunk size and edit count, then the first packet
    raw[at] = 0x40  # a coupling channel element: not decodable
    bad = tmp_path / "damaged.caf"
    bad.write_bytes(bytes(raw))
    names = ["a.wav", "float.wav", "a.caf", "b.caf"]
    paths = [library[n][0] for n in names]
    rc, plain, err = run("--loudness", *paths)
    assert rc == 0, err
    rc, out, err = run("--loudness", "--true-peak", paths[0], paths[1], paths[2], bad, paths[3])
    print(out)
    assert rc == 1 and str(bad) in err  # the damaged file is named, the others still print
    got, base = out.splitlines(), plain.splitlines()
    assert len(got) == len(base) == 4
    for n, g, b in zip(names, got, base):
        lufs, dbfs, dbtp, frames, path = g.split("  ")
        assert "  ".join([lufs, dbfs, frames, path]) == b, n
        _, x, rate = library[n]
        assert dbtp == "%.2f dBTP" % tr.dbtp(true_peak_of(x, rate)), n
    # the case-16 signal in a.wav and a.caf: 3 dB between the two peaks
    assert float(got[0].split("  ")[2].split()[0]) - float(got[0].split("  ")[1].split()[0]) > 2.0
    assert got[0].rsplit("  ", 1)[0] == got[2].rsplit("  ", 1)[0]
    rc, two, err = run("--loudness", "--true-peak", "--devices", 2, *paths, env={"ALACCONVERT_SHARE_DEVICES": "1"})
    assert rc == 0 and two.splitlines() == got, err


def test_true_peak_alone_is_refused_and_the_usage_text_is_unchanged(library):
    f = library["a.wav"][0]
    usage = run()[1]
    assert "--true-peak" not in usage and "--loudness" not in usage
    rc, out, err = run("--true-peak", f)
    assert rc == 1 and out == usage
    rc, out, err = run("--true-peak", "--crc", f)
    assert rc == 1 and out == usage
    rc, out, err = run("--loudness", "--true-peak")
    assert rc == 1 and out == usage
    rc, out, err = run("--loudness", "--true-peak", "--batch", f)
    assert rc == 1 and "LUFS" not in out


@pytest.fixture(scope="module")
def harness(gpu_ctx):
    subprocess.check_call(["make", "-C", CPP, "-f", "true_peak.mk", "true_peak"], stdout=subprocess.DEVNULL)
    return os.path.join(CPP, "true_peak")


def test_class_level_loudness_true_peak_batch(gpu_ctx, harness, tmp_path):
    """14 packets of 16-bit stereo, the last one short: as one file, as three files of which the middle one is empty, without
    packets, and with the short packet moved into the middle of a file"""
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
    _, coefs = alac_amd.true_peak_filter(44100)

    def run_harness(order, first):
        (tmp_path / "stream").write_bytes(b"".join(stream[offs[p]:offs[p + 1]].tobytes() for p in order))
        (tmp_path / "sizes").write_bytes(np.array([sizes[p] for p in order], dtype=np.uint32).tobytes())
        (tmp_path / "first").write_bytes(np.array(first, dtype=np.uint32).tobytes())
        p = subprocess.run([harness] + [str(tmp_path / n) for n in ("cookie", "stream", "sizes", "first")], capture_output=True,
                           text=True, timeout=120)
        assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
        lines = p.stdout.split("\n")
        return [tuple(float(v) for v in ln.split()) for ln in lines[:len(first) - 1]], lines[len(first) - 1:len(first) + 1]

    def same(got, packets):
        lufs, peak, true, lufs2, peak2 = got
        assert peak == peak2 and (lufs == lufs2 or (math.isnan(lufs) and math.isnan(lufs2))), got  # what LoudnessBatch gives
        v = np.concatenate([x[p * 4096:(p + 1) * 4096] for p in packets]) if len(packets) else x[:0]
        want, reports = tr.measure(v, 44100, coefs=coefs)
        assert peak == reports[0][1]
        assert abs(true - reports[0][0]) <= float(tr.bound(coefs, reports[0][1])) and true >= peak, (got, reports)

    whole = list(range(npk))
    got, tail = run_harness(whole, [0, npk])
    same(got[0], whole)
    assert tail == [f"frames {total}", "bad 0"]
    got, tail = run_harness(whole, [0, 8, 8, npk])
    same(got[0], whole[:8]), same(got[1], []), same(got[2], whole[8:])
    assert got[1][2] == 0.0
    got, tail = run_harness([], [0, 0, 0])  # files without packets: nothing to decode, nothing to measure
    assert got == [(-math.inf, 0.0, 0.0, -math.inf, 0.0)] * 2 and tail == ["frames 0", "bad 0"]
    order = whole[8:] + whole[:8]  # the short packet in the middle of the one file
    got, tail = run_harness(order, [0, npk])
    same(got[0], order)
    assert tail == [f"frames {total}", "bad 0"]
