"""Option "lpc": independent packets whose channels may carry predictor coefficients computed from the packet's own PCM
(alac_lpc.hip).  Every packet must decode to its input (oracle decoder, GPU decoder, the reference's compiled stages when
built), be rebuilt byte for byte by oracle/forge.py from the parameters in its own header, never be larger than the oracle's
independent packet (segment_packets = 1), and not depend on the batch around it."""
import lzma
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import alac_amd
from alac_amd.capi import AlacError

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import caf_oracle as co  # noqa: E402
import forge  # noqa: E402
from container_lib import music_like  # noqa: E402
from oracle_lib import have_ref, Ref, REFERENCE_WAVS  # noqa: E402

pytestmark = pytest.mark.gpu
FRAME = 4096


def golden(name):
    with open(os.path.join(HERE, "golden", REFERENCE_WAVS[name]), "rb") as f:
        return np.frombuffer(lzma.decompress(f.read()), np.uint8)


def known(name):
    with open(os.path.join(HERE, "golden", "known_answers.json")) as f:
        return json.load(f)["wav"][name]


def lpc_encode(ctx, fmt, pcm, total):
    with ctx.options(lpc=1):
        stream, sizes, _ = ctx.encode_host(fmt, pcm, total, segment_packets=1)
    return stream, sizes


def split(stream, sizes):
    ends = np.cumsum(sizes.astype(np.int64))
    return [stream[e - s:e] for s, e in zip(sizes.astype(np.int64), ends)]


def check_packets(ctx, oracle, fmt, pcm, total, stream, sizes, ref=None, frame=FRAME):
    """round trip through the oracle / reference / GPU decoders and the byte-for-byte re-forge; returns the LPC channels"""
    ch, depth, bpf = fmt.num_channels, fmt.bit_depth, fmt.bytes_per_frame
    pcm = np.concatenate([pcm, np.zeros(len(sizes) * frame * bpf - pcm.size, np.uint8)])
    cookie = ctx.magic_cookie(fmt)
    dec = oracle.decoder(cookie)
    rdec = oracle.decoder(cookie, hooks=ref.hooks()) if ref is not None else None
    forger = forge.Forger(oracle)
    lpc_channels = 0
    for p, pkt in enumerate(split(stream, sizes)):
        n = min(frame, total - p * frame)
        src = pcm[p * frame * bpf:(p * frame + n) * bpf]
        for d in (dec, rdec):
            if d is None:
                continue
            st, out, ns = d.decode_packet(pkt, bpf)
            assert st == 0 and ns == n and np.array_equal(out, src), f"packet {p}"
        esc, hn, shifted, mix_bits, mix_res, params = forge.parse_header(pkt, ch)
        assert hn == (None if n == frame else n)
        if esc:
            continue
        for cp in params:
            assert cp.mode == 0 and cp.pb_factor == 4 and cp.num <= 30 and cp.num != 31
            lpc_channels += cp.den_shift != 9 or cp.num not in (4, 8)
        again = forger.element(src, n, depth, ch, frame, params, mix_bits=mix_bits, mix_res=mix_res,
                               bytes_shifted=shifted)
        assert np.array_equal(again, pkt), f"re-forged packet {p} differs"
    offs = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes.astype(np.int64))])).cuda()
    out, ns, st, _ = ctx.decode(cookie, torch.from_numpy(stream).cuda(), offs, len(sizes))
    ctx.synchronize()
    assert int(st.abs().sum()) == 0 and int(ns.sum()) == total
    assert np.array_equal(out.cpu().numpy()[:total * bpf], pcm[:total * bpf])
    return lpc_channels


def never_larger(oracle, fmt, pcm, total, sizes, frame=FRAME):
    enc = oracle.encoder(frame, fmt.bit_depth, fmt.num_channels, 44100)
    _, ind = enc.encode_stream(pcm, total, segment_packets=1)
    assert len(ind) == len(sizes) and bool((sizes <= ind).all()), np.flatnonzero(sizes > ind)[:8]
    return int(ind.sum())


@pytest.mark.parametrize("name", ["05.wav", "50.wav", "70.wav"])
def test_reference_audio_round_trip_reforge_never_larger(gpu_ctx, oracle, name):
    ka = known(name)
    pcm = golden(name)
    fmt = alac_amd.make_format(FRAME, ka["bits"], ka["channels"], ka["rate"])
    total = ka["sample_frames"]
    stream, sizes = lpc_encode(gpu_ctx, fmt, pcm, total)
    ref = Ref() if have_ref() else None
    lpc_channels = check_packets(gpu_ctx, oracle, fmt, pcm, total, stream, sizes, ref)
    indep = never_larger(oracle, fmt, pcm, total, sizes)
    print(f"{name}: lpc {stream.size} B ({lpc_channels} LPC channels), independent {indep} B, chained "
          f"{ka['chained_bytes']} B ({100.0 * (stream.size / ka['chained_bytes'] - 1):+.2f} %)")
    if name != "70.wav":  # 70.wav is near silence: Apple's packets are already minimal
        assert lpc_channels > 0 and stream.size < indep


def encode_dev(ctx, fmt, d_pcm, n, **kw):
    stream, sizes = ctx.encode_to_host(fmt, d_pcm, n, **kw)
    return split(stream, sizes)


def test_batch_independence(gpu_ctx):
    fmt = alac_amd.make_format(FRAME, 16, 2, 44100)
    music = golden("50.wav")[:40 * FRAME * fmt.bytes_per_frame]
    n = 10000
    big = alac_amd.synth_pcm(0, n, fmt).copy()
    at = [0, 4321, n - 40]
    for a in at:
        big[a * FRAME * 4:(a + 40) * FRAME * 4] = music
    d_big = torch.from_numpy(big).cuda()
    d_music = torch.from_numpy(music.copy()).cuda()
    with gpu_ctx.options(lpc=1):
        alone = [encode_dev(gpu_ctx, fmt, d_music[p * FRAME * 4:(p + 1) * FRAME * 4].clone(), 1)[0] for p in range(0, 40, 13)]
        small = encode_dev(gpu_ctx, fmt, d_music, 40)
        assert all(np.array_equal(alone[i], small[13 * i]) for i in range(len(alone)))
        for thru in (0, 1):
            with gpu_ctx.options(thru=thru):
                pk = encode_dev(gpu_ctx, fmt, d_big, n)
            for a in at:
                assert all(np.array_equal(pk[a + p], small[p]) for p in range(40)), (thru, a)
        seg = torch.tensor([0, 7, 4000, 4321, n], dtype=torch.int32).cuda()
        pk = encode_dev(gpu_ctx, fmt, d_big, n, seg_first=seg)
        for a in at:
            assert all(np.array_equal(pk[a + p], small[p]) for p in range(40))
        pk = encode_dev(gpu_ctx, fmt, d_big, n, seg_first=seg, max_segment_packets=4000)
        assert all(np.array_equal(pk[4321 + p], small[p]) for p in range(40))


def wrap32_stereo(frames):
    x = np.empty((frames, 2), np.int32)
    x[:, 0] = np.where(np.arange(frames) % 2 == 0, 2 ** 31 - 1, -2 ** 31)
    x[:, 1] = -x[:, 0] - 1
    return x.astype("<i4").view(np.uint8).ravel()


@pytest.mark.parametrize("depth", [16, 20, 24, 32])
@pytest.mark.parametrize("channels", [1, 2])
def test_depths_partial_last_packet(gpu_ctx, oracle, depth, channels):
    frames = 3 * FRAME + 1234
    pcm = np.frombuffer(music_like(frames, channels, depth, 11 + depth + channels), np.uint8).copy()
    if depth == 20:
        pcm[0::3] &= 0xF0  # the 4 padding bits of each 3-byte container carry nothing
    fmt = alac_amd.make_format(FRAME, depth, channels, 44100)
    stream, sizes = lpc_encode(gpu_ctx, fmt, pcm, frames)
    check_packets(gpu_ctx, oracle, fmt, pcm, frames, stream, sizes)
    never_larger(oracle, fmt, pcm, frames, sizes)


@pytest.mark.parametrize("kind", ["silence", "noise", "wrap32"])
def test_silence_noise_wrap(gpu_ctx, oracle, kind):
    depth = 32 if kind == "wrap32" else 16
    fmt = alac_amd.make_format(FRAME, depth, 2, 44100)
    frames = 2 * FRAME
    if kind == "silence":
        pcm = np.zeros(frames * fmt.bytes_per_frame, np.uint8)
    elif kind == "noise":
        pcm = np.random.default_rng(5).integers(0, 256, frames * fmt.bytes_per_frame, dtype=np.uint8)
    else:
        pcm = wrap32_stereo(frames)
    stream, sizes = lpc_encode(gpu_ctx, fmt, pcm, frames)
    check_packets(gpu_ctx, oracle, fmt, pcm, frames, stream, sizes)
    never_larger(oracle, fmt, pcm, frames, sizes)
    if kind == "noise":
        assert all(forge.parse_header(p, 2)[0] for p in split(stream, sizes))


def test_lpc_with_fast_mode_is_refused(gpu_ctx):
    fmt = alac_amd.make_format(FRAME, 16, 2, 44100)
    pcm = alac_amd.synth_pcm(0, 2, fmt)
    with gpu_ctx.options(lpc=1, fast_mode=1):
        with pytest.raises(AlacError) as e:
            gpu_ctx.encode_host(fmt, pcm, 2 * FRAME, segment_packets=1)
    assert e.value.code == -50
    with gpu_ctx.options(lpc=1):
        with pytest.raises(AlacError) as e:
            gpu_ctx.encode_host(alac_amd.make_format(FRAME, 16, 6, 44100), np.zeros(FRAME * 12, np.uint8), FRAME)
    assert e.value.code == -50


def test_default_unchanged(gpu_ctx, oracle):
    """lpc back at 0 after an LPC encode: the chained stream is the reference's again"""
    ka = known("50.wav")
    pcm = golden("50.wav")
    fmt = alac_amd.make_format(FRAME, 16, 2, 44100)
    lpc_encode(gpu_ctx, fmt, pcm, ka["sample_frames"])
    assert gpu_ctx.get_option("lpc") == 0
    stream, sizes, _ = gpu_ctx.encode_host(fmt, pcm, ka["sample_frames"], segment_packets=0)
    assert stream.size == ka["chained_bytes"] and f"{oracle.fnv(stream):016x}" == ka["chained_fnv"]
    stream, sizes, _ = gpu_ctx.encode_host(fmt, pcm, ka["sample_frames"], segment_packets=1)
    assert stream.size == ka["indep_bytes"] and f"{oracle.fnv(stream):016x}" == ka["indep_fnv"]


@pytest.mark.parametrize("ext", ["caf", "m4a"])
def test_alacconvert_lpc(gpu_ctx, tmp_path, ext):
    ka = known("50.wav")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "convert-utility"), "alacconvert"], stdout=subprocess.DEVNULL)
    binary = os.path.join(ROOT, "convert-utility", "alacconvert")
    pcm = golden("50.wav")
    src, enc, back = tmp_path / "in.wav", tmp_path / f"out.{ext}", tmp_path / "back.wav"
    src.write_bytes(co.make_wav(pcm.tobytes(), 2, ka["rate"], 16))
    for args in (["--lpc", src, enc], [enc, back]):
        p = subprocess.run([binary] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
    from oracle_lib import parse_wav
    ch, rate, bits, data = parse_wav(back.read_bytes())
    assert (ch, rate, bits) == (2, ka["rate"], 16) and np.array_equal(data, pcm)
