"""alacconvert --float-bits N --dither [--dither-seed S] on the GPU: a float WAVE or CAF file gives, byte for byte, the file
that alacconvert writes without the flags for the integer WAVE holding the samples of the numpy restatement of the dither
rule (tests/dither_ref.py, every file's frames counted from 0); the same file alone, in --batch beside others and with
--devices 2; and two seeds give two files."""
import numpy as np
import pytest

import dither_ref as dr
from test_encode_float_symbols import make_float_caf, make_float_wav
from test_gpu_alacconvert_float import binary, co, convert, floats, run  # noqa: F401  (binary: the fixture)

pytestmark = pytest.mark.gpu


def int_wav(x, bits, seed):
    """the integer WAVE of x quantized at `bits` with the restatement's dither"""
    s, clip = dr.quantize_dithered(x, bits, seed)
    assert not clip.any()
    v = s.T.reshape(-1)
    if bits == 16:
        pcm = v.astype("<i2").tobytes()
    else:
        c = (v << 4 if bits == 20 else v) & 0xFFFFFF
        pcm = np.stack([c & 0xFF, (c >> 8) & 0xFF, (c >> 16) & 0xFF], axis=1).astype(np.uint8).tobytes()
    return co.make_wav(pcm, x.shape[0], 44100, bits)


@pytest.mark.parametrize("bits,ch,kind,ext,seed", [(16, 2, "tag3", "caf", None), (16, 2, "tag3", "caf", "12345"),
                                                   (16, 1, "caf_be", "caf", "0x0123456789ABCDEF"), (24, 2, "caf_le", "caf", "7"),
                                                   (24, 1, "extensible", "m4a", "0xffffffffffffffff"), (24, 2, "caf_be", "caf", "3")])
def test_dithered_float_file_equals_integer_file(binary, tmp_path, bits, ch, kind, ext, seed):
    x = floats(ch, 3 * 4096 + 123, bits + ch)
    data = {"tag3": lambda: make_float_wav(x), "extensible": lambda: make_float_wav(x, extensible=True),
            "caf_le": lambda: make_float_caf(x), "caf_be": lambda: make_float_caf(x, little_endian=False)}[kind]()
    flags = ["--float-bits", bits, "--dither"] + ([] if seed is None else ["--dither-seed", seed])
    rc, _, err, got = convert(binary, tmp_path, "f", data, ext, *flags)
    assert rc == 0 and "clipped" not in err, err
    rc, _, err, want = convert(binary, tmp_path, "i", int_wav(x, bits, int(seed or "0", 0)), ext)
    assert rc == 0, err
    assert got == want
    rc, _, err, plain = convert(binary, tmp_path, "p", data, ext, "--float-bits", bits)
    assert rc == 0 and plain != got


def test_alone_in_a_batch_and_over_two_devices(binary, tmp_path, monkeypatch):
    xs = [floats(2, 2 * 4096 + 7, 1), floats(2, 4096 * 3, 2), floats(2, 4096 + 1, 3), floats(1, 5000, 4)]
    args, alone = [], []
    for k, x in enumerate(xs):
        (tmp_path / f"f{k}.wav").write_bytes(make_float_wav(x))
        args += [tmp_path / f"f{k}.wav", tmp_path / f"f{k}.caf"]
        rc, _, err = run(binary, "--float-bits", 16, "--dither", "--dither-seed", 99, tmp_path / f"f{k}.wav", tmp_path / f"a{k}.caf")
        assert rc == 0, err
        alone.append((tmp_path / f"a{k}.caf").read_bytes())
        rc, _, err, want = convert(binary, tmp_path, f"i{k}", int_wav(x, 16, 99), "caf")
        assert rc == 0 and alone[k] == want, k
    monkeypatch.setenv("ALACCONVERT_SHARE_DEVICES", "1")
    for extra in ([], ["--devices", 2]):
        for k in range(len(xs)):
            (tmp_path / f"f{k}.caf").unlink(missing_ok=True)
        rc, _, err = run(binary, "--batch", *extra, "--float-bits", 16, "--dither", "--dither-seed", 99, *args)
        assert rc == 0, err
        for k in range(len(xs)):
            assert (tmp_path / f"f{k}.caf").read_bytes() == alone[k], (extra, k)


def test_two_seeds_give_two_files(binary, tmp_path):
    data = make_float_wav(floats(2, 4096 * 2, 5))
    outs = [convert(binary, tmp_path, f"s{s}{k}", data, "caf", "--float-bits", 20, "--dither", "--dither-seed", s)[3]
            for k, s in enumerate((1, 2, 1))]
    assert outs[0] is not None and outs[0] != outs[1] and outs[0] == outs[2]
