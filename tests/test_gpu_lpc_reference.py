"""Option "lpc" against its bit-exact host reference (oracle/lpc_ref.py): every packet's header (shift, mix, escape flag,
and per channel num, den and every coefficient) must equal the reference's decision, and the whole stream its forged
stream, byte for byte.  tests/test_gpu_lpc.py checks that the packets are legal; this file checks that the search chose
right: the autocorrelation, the Levinson recursion, the drop rules, the trial counts and the tie-break."""
import os
import sys

import numpy as np
import pytest

import alac_amd
from alac_amd.capi import AlacError

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
import forge  # noqa: E402
import lpc_ref  # noqa: E402
from container_lib import music_like  # noqa: E402
from test_gpu_lpc import check_packets, golden, known, lpc_encode, never_larger, split  # noqa: E402

pytestmark = pytest.mark.gpu


def against_reference(ctx, oracle, depth, channels, frame, pcm, total):
    """encode in the LPC mode on the GPU; every header equal to the reference's decision, the stream equal to its forged
    stream, and test_gpu_lpc's checks on top.  Returns the stream and the reference's decisions."""
    fmt = alac_amd.make_format(frame, depth, channels, 44100)
    stream, sizes = lpc_encode(ctx, fmt, pcm, total)
    ref_stream, ref_sizes, decisions = lpc_ref.stream(oracle, pcm, total, depth, channels, frame)
    assert len(sizes) == len(decisions)
    for p, (pkt, d) in enumerate(zip(split(stream, sizes), decisions)):
        esc, _, shifted, mix_bits, mix_res, params = forge.parse_header(pkt, channels)
        assert esc == d.escape, f"packet {p}: escape flag"
        if esc:
            continue
        assert (shifted, mix_bits, mix_res) == (d.shifted, d.mix_bits, d.mix_res), f"packet {p}: shift / mix"
        for c, (got, want) in enumerate(zip(params, d.params)):
            hdr = lambda cp: (cp.mode, cp.pb_factor, cp.num, cp.den_shift, [int(v) for v in cp.coefs[:cp.num]])  # noqa: E731
            assert hdr(got) == hdr(want), (f"packet {p} channel {c}: GPU {hdr(got)}, reference winner {d.winner[c]} "
                                           f"{hdr(want)}; trace {d.trace[c]}, Apple's channel {d.apple_cost[c]}")
    assert np.array_equal(sizes, ref_sizes) and np.array_equal(stream, ref_stream)
    check_packets(ctx, oracle, fmt, pcm, total, stream, sizes, frame=frame)
    never_larger(oracle, fmt, pcm, total, sizes, frame=frame)
    return stream, decisions


@pytest.mark.parametrize("name", ["05.wav", "50.wav", "70.wav"])
def test_reference_audio(gpu_ctx, oracle, name):
    ka = known(name)
    stream, _ = against_reference(gpu_ctx, oracle, ka["bits"], ka["channels"], 4096, golden(name), ka["sample_frames"])
    assert stream.size == ka["lpc_bytes"] and f"{oracle.fnv(stream):016x}" == ka["lpc_fnv"]


@pytest.mark.parametrize("depth", [16, 20, 24, 32])
@pytest.mark.parametrize("channels", [1, 2])
def test_edge_signals(gpu_ctx, oracle, depth, channels):
    """the edge-signal set of tests/test_lpc_reference.py, whose union reaches every path of the search"""
    pcm, total = lpc_ref.edge_signal(depth, channels)
    against_reference(gpu_ctx, oracle, depth, channels, 4096, pcm, total)


def test_full_scale_20bit_stereo_8192(gpu_ctx, oracle):
    """the worst case of the exact autocorrelation: |v| = 2^20 - 1 over 8192 samples, r[0] just under 2^53"""
    frames = 3 * 8192
    j = np.arange(frames)
    top, bottom = (1 << 19) - 1, -(1 << 19)
    left = np.where(j % 2 == 0, top, bottom)  # alternating, then a square wave of period 64, then a sine, all full scale
    left[8192:] = np.where((j[8192:] // 32) % 2 == 0, top, bottom)
    left[16384:] = np.round(np.sin(j[16384:] * 0.01) * (top + 0.5) - 0.5)
    x = np.stack([left, -left - 1])  # v = L - R = 2 L + 1 spans all 21 bits
    _, decisions = against_reference(gpu_ctx, oracle, 20, 2, 8192, forge.channels_to_pcm(x, 20), frames)
    assert any(not d.escape and d.mix_res != 0 for d in decisions)


@pytest.mark.parametrize("frame,channels", [(16, 2), (333, 2), (1152, 2), (4096, 2), (8192, 2), (16384, 1)])
def test_frame_sizes(gpu_ctx, oracle, frame, channels):
    """8192 stereo and 16 384 mono are the edge of the LDS planes (frame_size x channels <= 16 384)"""
    pcm, total = lpc_ref.edge_signal(16, channels, frame_size=frame, tail=frame // 2 + 1, seed=frame)
    against_reference(gpu_ctx, oracle, 16, channels, frame, pcm, total)
    music = np.frombuffer(music_like(2 * frame + 5, channels, 16, frame), np.uint8)
    against_reference(gpu_ctx, oracle, 16, channels, frame, music, 2 * frame + 5)


@pytest.mark.parametrize("n", [1, 2, 8, 9, 16, 17, 60, 61, 62, 1234])
def test_partial_last_packet(gpu_ctx, oracle, n):
    """short last packets: the 2 * order >= N stop and the predictor's warm-up"""
    channels, depth = (2, 16) if n % 2 == 0 else (1, 24)
    pcm, total = lpc_ref.edge_signal(depth, channels, tail=n, seed=n)
    against_reference(gpu_ctx, oracle, depth, channels, 4096, pcm, total)


@pytest.mark.parametrize("frame,channels", [(8193, 2), (16385, 1)])
def test_frame_size_limit_is_refused(gpu_ctx, frame, channels):
    fmt = alac_amd.make_format(frame, 16, channels, 44100)
    with gpu_ctx.options(lpc=1):
        with pytest.raises(AlacError) as e:
            gpu_ctx.encode_host(fmt, np.zeros(frame * fmt.bytes_per_frame, np.uint8), frame, segment_packets=1)
    assert e.value.code == -50
