"""alacconvert --verify-source and --compare with a float reference on the GPU: --float-bits N [--dither --dither-seed S]
--verify-source writes the bytes of the same command without the flag (alone, in --batch, with --devices 2); --compare
out.caf in_float.wav [--dither --dither-seed S] matches, names packet and frame of one changed float, and fails with the
wrong seed; an integer reference prints what it always printed."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_encode_float_symbols import make_float_caf, make_float_wav
from test_gpu_alacconvert_float import floats, int_wav, run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

pytestmark = pytest.mark.gpu
CU = os.path.join(ROOT, "convert-utility")
BIN = os.path.join(CU, "alacconvert")
KEYS = [(16, []), (24, []), (16, ["--dither", "--dither-seed", "0x1234"]), (24, ["--dither", "--dither-seed", "77"])]


@pytest.fixture(scope="module")
def binary(gpu_ctx):
    subprocess.check_call(["make", "-C", CU, "alacconvert"], stdout=subprocess.DEVNULL)
    return BIN


def write_inputs(tmp_path, specs):
    """float files of (channels, frames, seed, kind) -> [in0, out0, in1, out1, ...], the outputs, the floats"""
    args, outs, xs = [], [], []
    for k, (ch, frames, seed, kind) in enumerate(specs):
        x = floats(ch, frames, seed)
        data = {"wav": lambda: make_float_wav(x), "caf_be": lambda: make_float_caf(x, little_endian=False)}[kind]()
        src, dst = tmp_path / f"in{k}.{kind[:3]}", tmp_path / f"out{k}.{'m4a' if k % 2 else 'caf'}"
        src.write_bytes(data)
        args += [src, dst]
        outs.append(dst)
        xs.append(x)
    return args, outs, xs


@pytest.mark.parametrize("bits,key", KEYS, ids=lambda v: "-".join(map(str, v)) if isinstance(v, list) else str(v))
@pytest.mark.parametrize("mode", ["single", "batch", "devices", "lpc", "segments"])
def test_verify_source_writes_the_same_bytes(binary, tmp_path, mode, bits, key):
    if mode == "single":
        flags, specs = [], [(2, 3 * 4096 + 5, 11, "wav")]
    elif mode == "lpc":
        flags, specs = ["--lpc"], [(2, 2 * 4096 + 100, 12, "wav")]
    elif mode == "segments":
        flags, specs = ["--segment-packets", 2], [(1, 5 * 4096 + 1, 13, "caf_be")]
    else:
        flags = ["--batch"] + (["--devices", 2] if mode == "devices" else [])
        specs = [(2, 2 * 4096 + 9, 14, "wav"), (2, 5000, 15, "caf_be"), (1, 777, 16, "wav"), (2, 4096 * 4, 17, "wav"), (1, 9000, 18, "wav")]
    env = dict(os.environ, ALACCONVERT_SHARE_DEVICES="1")
    args, outs, _ = write_inputs(tmp_path, specs)
    cmd = [binary] + [str(a) for a in flags + ["--float-bits", bits] + key]
    p = subprocess.run(cmd + [str(a) for a in args], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stderr
    plain = [o.read_bytes() for o in outs]
    for o in outs:
        o.unlink()
    p = subprocess.run(cmd + ["--verify-source"] + [str(a) for a in args], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stderr
    assert [o.read_bytes() for o in outs] == plain
    # and every output compares equal to its float source with the same key
    for src, o in zip(args[0::2], outs):
        rc, out, err = run(binary, "--compare", *key, o, src)
        assert rc == 0 and "matches" in out, (out, err)


@pytest.mark.parametrize("bits,key", KEYS, ids=lambda v: "-".join(map(str, v)) if isinstance(v, list) else str(v))
def test_compare_with_a_float_reference(binary, tmp_path, bits, key):
    x = floats(2, 3 * 4096 + 500, 21 + bits)
    src, caf = tmp_path / "in.wav", tmp_path / "out.caf"
    src.write_bytes(make_float_wav(x))
    rc, _, err = run(binary, "--float-bits", bits, *key, src, caf)
    assert rc == 0, err
    rc, out, err = run(binary, "--compare", *key, caf, src)
    assert rc == 0 and "matches" in out and "(4 packets)" in out, (out, err)
    # the big-endian CAF of the same floats is the same reference
    be = tmp_path / "in_be.caf"
    be.write_bytes(make_float_caf(x, little_endian=False))
    assert run(binary, "--compare", *key, caf, be)[0] == 0
    # one float changed by 3 LSB: the right channel of sample-frame 8513 = packet 2, frame 321
    y = x.copy()
    y[1, 2 * 4096 + 321] += np.float32(3.0 / 2 ** (bits - 1))
    bad = tmp_path / "changed.wav"
    bad.write_bytes(make_float_wav(y))
    rc, out, err = run(binary, "--compare", *key, caf, bad)
    assert rc == 1 and "packet 2, frame 321" in out, (out, err)
    # a reference of another length is no match either
    short = tmp_path / "short.wav"
    short.write_bytes(make_float_wav(x[:, :4096 * 2]))
    assert run(binary, "--compare", *key, caf, short)[0] == 1
    if key:
        # the wrong seed, and no dither at all
        rc, out, _ = run(binary, "--compare", "--dither", "--dither-seed", "5", caf, src)
        assert rc == 1 and "differs" in out, out
        rc, out, _ = run(binary, "--compare", caf, src)
        assert rc == 1 and "differs" in out, out
    else:
        rc, out, _ = run(binary, "--compare", "--dither", caf, src)
        assert rc == 1 and "differs" in out, out


def test_compare_with_an_integer_reference_is_unchanged(binary, tmp_path):
    x = floats(2, 2 * 4096 + 50, 31)
    src, ref, caf = tmp_path / "in.wav", tmp_path / "int.wav", tmp_path / "out.caf"
    src.write_bytes(make_float_wav(x))
    ref.write_bytes(int_wav(x, 16))
    rc, _, err = run(binary, "--float-bits", 16, src, caf)
    assert rc == 0, err
    rc, out, err = run(binary, "--compare", caf, ref)
    assert rc == 0 and out.strip() == f'Compare: "{caf}" matches "{ref}" (3 packets)', (out, err)
    # an integer reference of another depth: different, as before; --dither wants a float reference
    ref24 = tmp_path / "int24.wav"
    ref24.write_bytes(int_wav(x, 24))
    rc, out, _ = run(binary, "--compare", caf, ref24)
    assert rc == 1 and "16-bit 2-channel" in out and "24-bit 2-channel" in out
    rc, _, err = run(binary, "--compare", "--dither", caf, ref)
    assert rc == 1 and "float reference" in err
    # --compare still takes no other option
    rc, out, _ = run(binary, "--compare", "--batch", caf, ref)
    assert rc == 1 and "Usage" in out


def test_verify_source_refusals(binary, tmp_path):
    x = floats(2, 5000, 4)
    src, dst = tmp_path / "in.wav", tmp_path / "out.caf"
    src.write_bytes(int_wav(x, 16))
    rc, _, err = run(binary, "--verify-source", src, dst)
    lines = [ln for ln in err.splitlines() if ln.strip()]
    assert rc == 1 and len(lines) == 1 and "--float-bits" in lines[0] and not dst.exists()
    # --float-bits N --verify keeps its refusal
    src.write_bytes(make_float_wav(x))
    rc, _, err = run(binary, "--float-bits", 16, "--verify", src, dst)
    assert rc == 1 and "--verify does not take float input" in err and not dst.exists()
