"""CPU, no library: the numpy restatement of the TPDF dither rule (tests/dither_ref.py) against things that are not this
project's code: Philox4x32-10 known answers from Random123's kat_vectors, values of k that follow from them by hand, the
statistics a TPDF dither must have (error mean 0 and variance 1/4 LSB^2 whatever the input, no correlation between
channels or along time) and the signal-dependence of the error of plain rounding that dither removes."""
import numpy as np
import pytest

import dither_ref as dr

SEEDS = [0, 1, 0x0123456789ABCDEF]
N = 1 << 20


@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(counter, key, want):
    got = dr.philox4x32_10(counter, key)
    assert tuple(int(w) for w in got) == want


def test_k_known_values():
    assert dr.dither_k(0, 0, np.arange(4)).tolist() == [-8077789, 2184913, 10236620, 11019893]
    # the first two by hand from the first known answer
    assert 0x6627e8 - 0xe169c5 == -8077789 and 0xbc57ac - 0x9b00db == 2184913
    assert dr.dither_k(0, 1, np.arange(2)).tolist() == [-7096409, -7659189]
    assert dr.dither_k(0x0123456789ABCDEF, 5, np.array([2 ** 32 + 1, 2 ** 33], np.uint64)).tolist() == [10515490, 8965496]
    assert dr.dither_k(1, 0, np.array([4095, 4096])).tolist() == [-4954558, 3214424]


def test_d_is_exact_and_inside_one_lsb():
    k = dr.dither_k(7, 3, np.arange(1 << 16))
    d = dr.dither(7, 3, np.arange(1 << 16))
    assert np.array_equal(d.astype(np.float64) * 2.0 ** 24, k.astype(np.float64))
    assert np.abs(k).max() <= 2 ** 24 - 1 and float(np.abs(d).max()) < 1.0


@pytest.mark.parametrize("seed", SEEDS)
def test_dither_is_uncorrelated(seed):
    t = np.arange(N, dtype=np.uint64)
    d0 = dr.dither(seed, 0, t).astype(np.float64)
    d1 = dr.dither(seed, 1, t).astype(np.float64)
    bound = 6.0 / 1024

    def corr(a, b):
        return float(np.corrcoef(a, b)[0, 1])

    figures = {"channels": corr(d0, d1)}
    for lag in (1, 2, 3):
        figures[f"lag{lag}"] = corr(d0[:-lag], d0[lag:])
    print(hex(seed), figures)
    for what, c in figures.items():
        assert abs(c) < bound, (hex(seed), what, c)
    # a TPDF of two uniforms on [0, 1): variance 1/6
    assert abs(d0.var() - 1.0 / 6) < 0.005 and abs(d0.mean()) < 3.0 / 1024


@pytest.mark.parametrize("depth", [16, 20, 24])
@pytest.mark.parametrize("seed", SEEDS)
def test_error_mean_and_variance_do_not_depend_on_the_input(seed, depth):
    top = 2.0 ** (depth - 1)
    for f in (0, 0.125, 0.25, 0.3, 0.5, 0.75):
        x = np.full((1, N), (100 + f) / top, np.float32)
        s, clip = dr.quantize_dithered(x, depth, seed)
        assert not clip.any()
        e = s[0].astype(np.float64) - x[0].astype(np.float64) * top  # in LSB
        print(hex(seed), depth, f, "mean", e.mean(), "variance", e.var())
        assert abs(e.mean()) < 3.0 / 1024, (hex(seed), depth, f, e.mean())
        assert abs(e.var() - 0.25) < 0.005, (hex(seed), depth, f, e.var())


def test_sine_error_follows_the_signal_only_without_dither():
    t = np.arange(N)
    x = (0.3 * np.sin(2 * np.pi * 440.0 * t / 44100.0)).astype(np.float32)[None, :]
    x64 = x[0].astype(np.float64) * 32768.0

    def corr(s):
        e = s.astype(np.float64) - x64
        return float(np.corrcoef(e * e, x64 * x64)[0, 1])

    plain = corr(np.rint(x64))
    dithered = corr(dr.quantize_dithered(x, 16, 0)[0][0])
    print("corr(e^2, x^2): plain", plain, "dithered", dithered)
    assert plain > 0.02
    assert abs(dithered) < 6.0 / 1024


def test_quantization_without_dither_bits_is_the_plain_rule():
    """where d happens to be 0 the rule is alac_hip_encode_float's; and the specials saturate and count as there"""
    x = np.array([[np.inf, -np.inf, np.nan, 1.0, -1.0, 0.0, 3e38, -3e38, 0.5, -0.5]], np.float32)
    s, clip = dr.quantize_dithered(x, 16, 5)
    assert s[0, :3].tolist() == [32767, -32768, 0] and clip[0, :3].all()
    assert s[0, 6:8].tolist() == [32767, -32768] and clip[0, 6:8].all()
    assert abs(s[0, 8] - 16384) <= 1 and abs(s[0, 9] + 16384) <= 1 and not clip[0, 8:].any()
    assert s[0, 3] in (32767,) and s[0, 4] in (-32768, -32767) and abs(s[0, 5]) <= 1
