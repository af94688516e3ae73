"""The host reference of the LPC mode's search (oracle/lpc_ref.py), on its own: its fma, its Levinson recursion against an
exact one, the legality of what it forges, the known LPC totals of the reference audio, and the edge-signal set that
tests/test_gpu_lpc_reference.py runs on the GPU reaching every path of the search.  No GPU needed."""
import json
import lzma
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
import forge  # noqa: E402
import lpc_ref  # noqa: E402
from oracle_lib import REFERENCE_WAVS  # noqa: E402


def golden(name):
    with open(os.path.join(HERE, "golden", REFERENCE_WAVS[name]), "rb") as f:
        return np.frombuffer(lzma.decompress(f.read()), np.uint8)


def known(name):
    with open(os.path.join(HERE, "golden", "known_answers.json")) as f:
        return json.load(f)["wav"][name]


def test_fma_rounds_once():
    e = 2.0 ** -30
    a, b = 1.0 + e, 1.0 - e  # a * b = 1 - 2^-60: the product alone rounds to 1
    assert a * b - 1.0 == 0.0 and lpc_ref.fma(a, b, -1.0) == -2.0 ** -60
    rng = np.random.default_rng(1)
    for _ in range(2000):
        a, b, c = (float(v) for v in rng.standard_normal(3) * 2.0 ** rng.integers(-40, 40, 3))
        exact = Fraction(a) * Fraction(b) + Fraction(c)
        assert lpc_ref.fma(a, b, c) == float(exact)
    # a tie of the final rounding goes to even: 1 + 2^-53 (exactly halfway) -> 1, 1 + 3 * 2^-53 -> 1 + 2^-51
    assert lpc_ref.fma(2.0 ** -27, 2.0 ** -26, 1.0) == 1.0
    assert lpc_ref.fma(3 * 2.0 ** -27, 2.0 ** -26, 1.0) == 1.0 + 2.0 ** -51


def exact_levinson(r, order):
    a, err = [Fraction(0)] * (order + 1), Fraction(r[0])
    for m in range(1, order + 1):
        k = (r[m] - sum(a[i] * r[m - i] for i in range(1, m))) / err
        a = [Fraction(0)] + [a[i] - k * a[m - i] for i in range(1, m)] + [k] + a[m + 1:]
        err *= 1 - k * k
    return a


def test_levinson_mirror_matches_exact_recursion():
    rng = np.random.default_rng(2)
    for trial in range(6):
        x = np.round(rng.standard_normal(4096) * 3000).astype(np.int64)
        x = np.convolve(x, [1.0, 0.6, 0.2], "same").astype(np.int64)  # well conditioned, not white
        r = lpc_ref.autocorr(x, x.size)
        trace = lpc_ref.levinson(r, x.size)
        for cd in trace:
            assert cd.drop is None
            a = exact_levinson(r, cd.order)
            want = [round(float(v) * (1 << cd.den)) for v in a[1:]]
            assert max(abs(g - w) for g, w in zip(cd.coefs, want)) <= 1  # within a rounding step of the exact value
            amax = max(abs(float(v)) for v in a[1:])
            assert round(amax * (1 << cd.den)) <= 32767 and (cd.den == 15 or round(amax * (2 << cd.den)) > 32767)
        # the float coefficients themselves, before quantisation, to ~1e-12 relative
        a30 = exact_levinson(r, 30)
        r_f = [float(v) for v in r]
        mirror = mirror_coefs(r_f, 30)
        for m, e in zip(mirror[1:], a30[1:]):
            assert abs(m - float(e)) <= 1e-12 * max(abs(float(v)) for v in a30[1:])


def mirror_coefs(r, order):
    """lpc_ref.levinson's float recursion, without the candidate logic, for the comparison above"""
    a, err = [0.0] * (order + 1), r[0]
    for m in range(1, order + 1):
        acc = r[m]
        for i in range(1, m):
            acc = lpc_ref.fma(-a[i], r[m - i], acc)
        km = acc / err
        a[1:m] = [lpc_ref.fma(-km, a[m - i], a[i]) for i in range(1, m)]
        a[m] = km
        err *= lpc_ref.fma(-km, km, 1.0)
    return a


def test_autocorrelation_bound():
    x = np.full(8192, -(1 << 20) + 1, np.int64)  # |v| of full-scale 20-bit stereo: the worst case of the format
    assert lpc_ref.autocorr(x, x.size)[0] <= lpc_ref.EXACT
    with pytest.raises(AssertionError):
        lpc_ref.autocorr(np.full(8192, 1 << 21, np.int64), 8192)


def check_stream(oracle, pcm, total, depth, channels, frame):
    """every packet the reference forges decodes to its input and is never larger than Apple's independent packet"""
    stream, sizes, decisions = lpc_ref.stream(oracle, pcm, total, depth, channels, frame)
    enc = oracle.encoder(frame, depth, channels, 44100)
    _, ind = enc.encode_stream(pcm, total, segment_packets=1)
    assert bool((sizes <= ind).all())
    dec = oracle.decoder(enc.cookie())
    bpf = channels * forge.BPS[depth]
    ends = np.cumsum(sizes.astype(np.int64))
    for p, (s, e) in enumerate(zip(sizes.astype(np.int64), ends)):
        n = min(frame, total - p * frame)
        st, out, ns = dec.decode_packet(stream[e - s:e], bpf)
        assert st == 0 and ns == n and np.array_equal(out, pcm[p * frame * bpf:(p * frame + n) * bpf]), f"packet {p}"
    return stream, decisions


@pytest.mark.parametrize("name", ["05.wav", "50.wav", "70.wav"])
def test_known_totals(oracle, name):
    """the LPC streams the GPU wrote for the reference audio (444 858, 1 146 100 and 7 268 B)"""
    ka = known(name)
    stream, decisions = check_stream(oracle, golden(name), ka["sample_frames"], ka["bits"], ka["channels"], 4096)
    assert stream.size == ka["lpc_bytes"] and f"{oracle.fnv(stream):016x}" == ka["lpc_fnv"]
    assert stream.size == {"05.wav": 444858, "50.wav": 1146100, "70.wav": 7268}[name]


def test_edge_signals_reach_every_path(oracle):
    seen = set()
    for depth in (16, 20, 24, 32):
        for channels in (1, 2):
            pcm, total = lpc_ref.edge_signal(depth, channels)
            _, decisions = check_stream(oracle, pcm, total, depth, channels, 4096)
            seen |= lpc_ref.paths(decisions)
    want = {"r0", "den", "short", "den15", "den5..14", "win_apple", "mix0", "mix!=0", "escape"}
    want |= {f"win{o}" for o in lpc_ref.ORDERS}
    assert want <= seen, sorted(want - seen)
    assert seen & {"k", "err"}, "no unstable recursion"
