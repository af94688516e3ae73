"""CPU: the integer probe rule of include/alac_hip.h as int_probe_ref.py restates it — against hand-made cases, against the
float probe's need(x) on x = s * 2^-(S-1) for S <= 24, and against the integer conversion rule (pcm_requant_ref.py): a
reduction to b bits is exact exactly when need_bits <= b."""
import numpy as np
import pytest

import float_probe_ref as fr
import int_probe_ref as ir
import pcm_requant_ref as pr

SOURCES = [(2, 16), (3, 16), (3, 20), (3, 24), (4, 16), (4, 20), (4, 24), (4, 32)]  # (container bytes, S)


def words(**kw):
    r = np.zeros(8, np.uint32)
    for k, v in kw.items():
        r[{"out_of_range": 0, "differing_frames": 2, "need_bits": 4, "peak": 5, "pad_bits": 6}[k]] = v
    return r


@pytest.mark.parametrize("cb,S", SOURCES)
def test_hand_made_cases(cb, S):
    top, P = 1 << (S - 1), 8 * cb - S
    for lj in (0, 1):
        put = (lambda s: s << P) if lj else (lambda s: s)
        src = (cb, S, lj)
        one = lambda *s: np.array([[put(x) for x in s]], np.int64)  # noqa: E731
        assert np.array_equal(ir.report(one(0, 0, 0), src), words())
        assert np.array_equal(ir.report(np.zeros((2, 0), np.int64), src), words())
        assert np.array_equal(ir.report(one(-top), src), words(need_bits=1, peak=top))  # as -1.0 in the float rule
        assert np.array_equal(ir.report(one(top - 1), src), words(need_bits=S, peak=top - 1))
        assert np.array_equal(ir.report(one(1, -1), src), words(need_bits=S, peak=1))
        assert np.array_equal(ir.report(one(top >> 1), src), words(need_bits=2, peak=top >> 1))  # 0.5
        assert np.array_equal(ir.report(one(3 << (S - 16), -(5 << (S - 16))), src), words(need_bits=16, peak=5 << (S - 16)))
    if P:  # right-justified in a wider container: one step out of range on each side saturates and is counted
        src = (cb, S, 0)
        assert np.array_equal(ir.report([[top]], src), words(out_of_range=1, need_bits=S, peak=top - 1))
        assert np.array_equal(ir.report([[-top - 1]], src), words(out_of_range=1, need_bits=1, peak=top))
        assert np.array_equal(ir.report([[top - 1, -top]], src), words(need_bits=S, peak=top))
        assert ir.report_depth(ir.report([[top]], src)) == 0
        # left-justified: the bits under the sample are pad bits, OR-ed
        src = (cb, S, 1)
        assert np.array_equal(ir.report([[(2 << P) | 1, (4 << P) | (1 << (P - 1))]], src),
                              words(need_bits=S - 1, peak=4, pad_bits=1 | (1 << (P - 1))))
        assert ir.report_depth(ir.report([[(2 << P) | 1]], src)) == 0
        assert np.array_equal(ir.report([[-1]], src), words(need_bits=S, peak=1, pad_bits=(1 << P) - 1))  # s = -1


def test_dual_mono_and_differing_frames():
    src = (2, 16, 1)
    a = np.array([5, -7, 0, 300, 2], np.int64)
    assert ir.report(np.stack([a, a]), src)[2] == 0
    b = a.copy()
    b[3] += 1
    assert ir.report(np.stack([a, b]), src)[2] == 1
    assert ir.report(np.stack([a, b, a, b]), src)[2] == 1  # a frame counts once, however many channels differ
    assert ir.report(np.stack([b, a, a]), src)[2] == 1     # against channel 0
    assert ir.report(a[None, :], src)[2] == 0
    # pad bits are no part of the sample: channels that differ only there are identical
    src = (4, 24, 1)
    assert ir.report(np.stack([a << 8, (a << 8) | 3]), src)[2] == 0
    # segments
    got = ir.reports(np.stack([a, b]), (2, 16, 1), [0, 3, 3, 5])
    assert got.shape == (3, 8) and got[:, 2].tolist() == [0, 0, 1] and not got[1].any()


def test_report_depth():
    for n, d in ((0, 16), (1, 16), (16, 16), (17, 20), (20, 20), (21, 24), (24, 24), (25, 32), (32, 32)):
        assert ir.report_depth(words(need_bits=n)) == d
    assert ir.report_depth(words(need_bits=3, out_of_range=1)) == 0
    assert ir.report_depth(words(need_bits=3, pad_bits=8)) == 0
    r = words(need_bits=3)
    r[1] = 1  # the high word of out_of_range
    assert ir.report_depth(r) == 0
    assert ir.report_depth(words(need_bits=3, differing_frames=9, peak=4)) == 16


@pytest.mark.parametrize("S", [16, 20, 24])
def test_need_is_the_float_rule_on_the_scaled_sample(S):
    rng = np.random.default_rng(S)
    top = 1 << (S - 1)
    s = rng.integers(-top, top, 5000, dtype=np.int64) << rng.integers(0, S, 5000)
    s = np.concatenate([np.clip(s, -top, top - 1), [-top, top - 1, 0, 1, -1]])
    x = (s.astype(np.float64) / top).astype(np.float32)
    assert np.array_equal(x.astype(np.float64) * top, s)  # exact floats
    assert np.array_equal(ir.need(s, S), fr.need(x))
    assert ir.report(s[None, :], (4, S, 0))[4] == fr.report(x)[4]


@pytest.mark.parametrize("S,b", pr.REDUCING)
def test_a_reduction_is_exact_exactly_when_need_fits(S, b):
    rng = np.random.default_rng(100 * S + b)
    top = 1 << (S - 1)
    s = np.clip(rng.integers(-top, top, 4000, dtype=np.int64) >> rng.integers(0, S, 4000) << rng.integers(0, S, 4000), -top, top - 1)
    s = np.concatenate([s, pr.edge_samples(S, b), [1 << (S - b), 1 << (S - b - 1), -(1 << (S - b)), 3 << (S - b - 1)]])
    out, clipped = pr.requantize(s, S, b)
    exact = ~clipped & ((out << (S - b)) == s)
    fits = ir.need(s, S) <= b
    assert np.array_equal(exact, fits)
    assert exact.any() and (~exact).any()
    # ... and the set as a whole: its report names a depth at which every sample is exact
    for keep in (fits, np.ones(s.size, bool)):
        d = ir.report_depth(ir.report(s[keep][None, :], (4, S, 0)))
        back, clip = pr.requantize(s[keep], S, d)
        assert not clip.any() and np.array_equal(back << (S - d) if d < S else back >> (d - S), s[keep])
