"""CPU: the integer rule of include/alac_hip.h as tests/pcm_requant_ref.py restates it.  Against exact rational rounding
(Python's round on s / 2^D, which is exact for these sizes and rounds half to even) at all six reducing pairs, every tie,
both extremes; widening is exact; undithered and S <= 24 the result equals the float rule's on x = s * 2^-(S-1); right-
justified containers saturate and count, the low bits of left-justified ones are ignored; and the dithered error has mean 0
and variance 1/4 LSB^2 within a sampling bound."""
import numpy as np
import pytest

import pcm_requant_ref as R
from dither_ref import dither_k


def exact(s, bits, depth):
    """round half to even of s / 2^D by Python's round (s / 2^D is an exact float64: |s| < 2^53) -> (clamped, clipped)"""
    D = bits - depth
    r = np.array([round(int(v) / 2 ** D) for v in s], np.int64)
    lo, hi = -(1 << (depth - 1)), (1 << (depth - 1)) - 1
    return np.clip(r, lo, hi), (r < lo) | (r > hi)


def float_rule(x, depth):
    """the rule of alac_hip_encode_float for finite x (float32): rint of the exact product, saturated"""
    top = 2 ** (depth - 1)
    r = np.rint(x.astype(np.float64) * float(top))
    return np.clip(r, -top, top - 1).astype(np.int64), (r > top - 1) | (r < -top)


@pytest.mark.parametrize("bits,depth", R.REDUCING)
def test_reduction_equals_exact_rational_rounding(bits, depth):
    rng = np.random.default_rng(bits * 100 + depth)
    top = 1 << (bits - 1)
    s = np.concatenate([rng.integers(-top, top, 20000), R.edge_samples(bits, depth)])
    got, gclip = R.requantize(s, bits, depth)
    want, wclip = exact(s, bits, depth)
    assert np.array_equal(got, want) and np.array_equal(gclip, wclip)


@pytest.mark.parametrize("bits,depth", R.REDUCING)
def test_ties_at_every_multiple_of_half_an_lsb(bits, depth):
    """s = m * 2^(D-1): m even is exact (m / 2); m odd lies half way and goes to the even one of (m - 1) / 2, (m + 1) / 2"""
    D = bits - depth
    count = 1 << (bits - D + 1)  # the multiples inside the source range
    if count <= 1 << 17:
        m = np.arange(-(count // 2), count // 2, dtype=np.int64)
    else:  # (24 -> 20, 32 -> 20, 32 -> 24: both ends and a sample of the rest)
        rng = np.random.default_rng(D)
        ends = np.arange(2000, dtype=np.int64)
        m = np.concatenate([ends - count // 2, rng.integers(-(count // 2), count // 2, 1 << 17), count // 2 - 2000 + ends])
    s = m << (D - 1)
    lower = (m - 1) // 2
    want = np.where(m % 2 == 0, m // 2, np.where(lower % 2 == 0, lower, lower + 1))
    lo, hi = -(1 << (depth - 1)), (1 << (depth - 1)) - 1
    got, clip = R.requantize(s, bits, depth)
    assert np.array_equal(got, np.clip(want, lo, hi)) and np.array_equal(clip, want > hi)
    sub = np.concatenate([np.arange(0, 2000), np.arange(m.size - 2000, m.size)])
    assert np.array_equal(got[sub], exact(s[sub], bits, depth)[0])


@pytest.mark.parametrize("bits,depth", R.REDUCING)
def test_extremes(bits, depth):
    top, out_top = 1 << (bits - 1), 1 << (depth - 1)
    got, clip = R.requantize(np.array([top - 1, -top]), bits, depth)
    assert got.tolist() == [out_top - 1, -out_top] and clip.tolist() == [True, False]


@pytest.mark.parametrize("bits,depth", R.WIDENING + [(d, d) for d in R.DEPTHS])
def test_widening_is_exact(bits, depth):
    rng = np.random.default_rng(bits + depth)
    top = 1 << (bits - 1)
    s = np.concatenate([rng.integers(-top, top, 20000), [top - 1, -top, 0, -1]])
    got, clip = R.requantize(s, bits, depth)
    assert np.array_equal(got, s * (1 << (depth - bits))) and not clip.any()
    assert got.max() == (1 << (depth - 1)) - (1 << (depth - bits)) and got.min() == -(1 << (depth - 1))
    with pytest.raises(AssertionError):
        R.requantize(s, bits, depth, k=np.zeros(s.size, np.int64))


@pytest.mark.parametrize("bits,depth", [(20, 16), (24, 16), (24, 20)])
def test_undithered_equals_the_float_rule(bits, depth):
    rng = np.random.default_rng(bits * 7 + depth)
    top = 1 << (bits - 1)
    D = bits - depth
    ties = (np.arange(-(1 << (bits - D)), 1 << (bits - D), dtype=np.int64) << (D - 1))  # every multiple of half an LSB
    s = np.concatenate([rng.integers(-top, top, 200000), ties, [top - 1, -top]])
    x = (s.astype(np.float64) * 2.0 ** -(bits - 1)).astype(np.float32)
    assert np.array_equal(x.astype(np.float64) * top, s)  # x is exact
    got, gclip = R.requantize(s, bits, depth)
    want, wclip = float_rule(x, depth)
    assert np.array_equal(got, want) and np.array_equal(gclip, wclip) and gclip.any()


@pytest.mark.parametrize("container_bytes,bits", [(3, 16), (3, 20), (4, 16), (4, 20), (4, 24)])
def test_right_justified_containers_saturate_and_count(container_bytes, bits):
    top = 1 << (bits - 1)
    full = 1 << (8 * container_bytes - 1)
    v = np.array([top - 1, top, top + 1, full - 1, -top, -top - 1, -full, 0, 5])
    s, bad = R.sample_of(v, bits, container_bytes, False)
    assert s.tolist() == [top - 1, top - 1, top - 1, top - 1, -top, -top, -top, 0, 5]
    assert bad.tolist() == [False, True, True, True, False, True, True, False, False]
    out, clip = R.convert(v.reshape(1, -1), bits, container_bytes, False, 16, v.size)
    # a saturated container counts even where the rounding that follows does not clip (the bottom one)
    assert clip[0].tolist() == [bits > 16, True, True, True, False, True, True, False, False]
    assert out[0, 5] == -32768 and out[0, 1] == 32767


@pytest.mark.parametrize("container_bytes,bits", [(3, 16), (3, 20), (4, 16), (4, 20), (4, 24)])
def test_left_justified_low_bits_are_ignored(container_bytes, bits):
    rng = np.random.default_rng(container_bytes * 40 + bits)
    top = 1 << (bits - 1)
    low = 8 * container_bytes - bits
    s = np.concatenate([rng.integers(-top, top, 5000), [top - 1, -top]])
    junk = rng.integers(0, 1 << low, s.size)
    got, bad = R.sample_of((s << low) | junk, bits, container_bytes, True)
    assert np.array_equal(got, s) and not bad.any()


def test_frames_behind_a_packet_are_zero_undithered_and_unclipped():
    v = np.full((2, 8), 0x7FFFFFFF, np.int64)
    out, clip = R.convert(v, 32, 4, True, 16, 4, num_samples=[3, 0], seed=9)
    assert out[:, 3:].tolist() == [[0] * 5] * 2 and not clip[:, 3:].any() and clip[:, :3].all()


@pytest.mark.parametrize("bits,depth", R.REDUCING)
def test_dithered_error_has_mean_0_and_variance_a_quarter(bits, depth):
    """N independent errors e = out - s / 2^D in LSB, E e = 0 and E e^2 = 1/4 whatever s is (TPDF of +-1 LSB; k's grid of
    2^-24 LSB moves either by less than 2^-23).  |e| < 1.5, so Var e^2 <= E e^4 <= 2.25 * E e^2 = 0.5625.  The bound is five
    standard deviations of the sample mean: 5 * 0.5 / sqrt(N) for e and 5 * 0.75 / sqrt(N) for e^2."""
    N = 200000
    rng = np.random.default_rng(bits * 31 + depth)
    D = bits - depth
    top = 1 << (bits - 1)
    s = rng.integers(-top + (4 << D), top - (4 << D), N)  # nothing clips
    k = dither_k(0xC0FFEE + bits, depth & 7, np.arange(N, dtype=np.uint64))
    out, clip = R.requantize(s, bits, depth, k)
    assert not clip.any()
    e = out - s / 2.0 ** D
    assert abs(e.mean()) < 5 * 0.5 / np.sqrt(N), e.mean()
    assert abs((e * e).mean() - 0.25) < 5 * 0.75 / np.sqrt(N), (e * e).mean()
    # and the dither does something: the undithered error's second moment is 1/12 at most
    e0 = R.requantize(s, bits, depth)[0] - s / 2.0 ** D
    assert (e0 * e0).mean() < 0.1
