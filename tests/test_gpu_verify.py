"""GPU: alac_hip_verify (Context.verify) and `alacconvert --verify / --compare`.  A verify pass must give exactly what
"alac_hip_decode, then compare on the host" gives — first differing frame per packet, 0 for an undecodable packet,
min(decoded, expected) for a frame count that differs — on every decoder path (fused and separate launches, pair lanes,
direct reads, uncompressed packets, the element rounds of 3..8 channels, the lane decoder)."""
import json
import lzma
import os
import subprocess
import sys

import numpy as np
import pytest

import alac_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import caf_oracle as co  # noqa: E402
from container_lib import music_like  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden")
BIN = os.path.join(ROOT, "convert-utility", "alacconvert")
CLEAN = 0xFFFFFFFF

# decoder paths: automatic, fused launch, separate launches with / without pair lanes, direct reads always / never, lane decoder
VARIANTS = [{}, {"dec_fused": 1}, {"dec_fused": 0}, {"dec_fused": 0, "dec_pair": 0}, {"dec_fused": 0, "dec_direct": 2},
            {"dec_fused": 0, "dec_direct": 0}, {"decoder_lane": 1}]


class Case:
    """one stream + the PCM it must decode to, laid out as alac_hip_decode writes it"""

    def __init__(self, cookie, packets, fmt, expected, counts):
        self.cookie = np.ascontiguousarray(cookie, np.uint8)
        self.sizes = np.array([len(p) for p in packets], np.int64)
        self.stream = np.concatenate(packets).astype(np.uint8)
        self.fmt = fmt
        self.expected = expected  # uint8 [n * packet_bytes]
        self.counts = np.asarray(counts, np.int32)

    @property
    def n(self):
        return len(self.sizes)


def packed_case(ctx, cookie, fmt, stream, sizes, pcm, frames):
    """expected PCM of a stream encoded from `pcm` (frames sample-frames, packets back to back)"""
    n = len(sizes)
    exp = np.zeros(n * fmt.packet_bytes, np.uint8)
    exp[:frames * fmt.bytes_per_frame] = pcm[:frames * fmt.bytes_per_frame]
    counts = [min(fmt.frame_size, frames - p * fmt.frame_size) for p in range(n)]
    ends = np.cumsum(sizes.astype(np.int64))
    packets = [stream[e - s:e] for s, e in zip(sizes.astype(np.int64), ends)]
    return Case(cookie, packets, fmt, exp, counts)


def encode_case(ctx, depth, channels, frames, pcm=None, seed=1, segment_packets=1, frame_size=4096, **options):
    fmt = alac_amd.make_format(frame_size, depth, channels, 44100)
    if pcm is None:
        pcm = np.frombuffer(music_like(frames, channels, depth, seed), np.uint8).copy()
        if depth == 20:
            pcm[0::3] &= 0xF0  # the 4 padding bits of a 3-byte container carry nothing
    with ctx.options(**options):
        stream, sizes, _ = ctx.encode_host(fmt, pcm, frames, segment_packets=segment_packets)
    return packed_case(ctx, ctx.magic_cookie(fmt), fmt, stream, sizes, pcm, frames)


def golden_wav(name):
    with open(os.path.join(GOLD, "known_answers.json")) as f:
        ka = json.load(f)["wav"][name]
    with open(os.path.join(GOLD, {"50.wav": "wav50_pcm.xz", "05.wav": "wav05_pcm.xz"}[name]), "rb") as f:
        pcm = np.frombuffer(lzma.decompress(f.read()), np.uint8)
    return ka, pcm


def verify(ctx, c, expected=None, counts="case", stream=None):
    import torch
    expected = c.expected if expected is None else expected
    stream = c.stream if stream is None else stream
    offs = np.concatenate([[0], np.cumsum(c.sizes)]).astype(np.int64)
    ns = None
    if counts is not None:
        ns = torch.from_numpy(np.ascontiguousarray(c.counts if isinstance(counts, str) else counts, np.int32)).cuda()
    fm, st, bad = ctx.verify(c.cookie, torch.from_numpy(stream).cuda(), torch.from_numpy(offs).cuda(), c.n,
                             torch.from_numpy(expected).cuda(), ns)
    ctx.synchronize()
    return fm.cpu().numpy().view(np.uint32), st.cpu().numpy(), int(bad.item())


def host_reference(ctx, c, expected=None, counts=None, stream=None):
    """alac_hip_decode, then the comparison on the host"""
    import torch
    expected = c.expected if expected is None else expected
    counts = c.counts if counts is None else np.asarray(counts)
    stream = c.stream if stream is None else stream
    offs = np.concatenate([[0], np.cumsum(c.sizes)]).astype(np.int64)
    out, ns, st, fmt = ctx.decode(c.cookie, torch.from_numpy(stream).cuda(), torch.from_numpy(offs).cuda(), c.n)
    ctx.synchronize()
    out, ns, st = out.cpu().numpy(), ns.cpu().numpy(), st.cpu().numpy()
    bpf, pb = fmt.bytes_per_frame, fmt.packet_bytes
    fm = np.full(c.n, CLEAN, np.uint32)
    for p in range(c.n):
        if st[p] != 0:
            fm[p] = 0
            continue
        m = min(int(ns[p]), int(counts[p]))
        a = out[p * pb:p * pb + m * bpf].reshape(m, bpf)
        b = expected[p * pb:p * pb + m * bpf].reshape(m, bpf)
        diff = np.nonzero((a != b).any(axis=1))[0]
        if diff.size:
            fm[p] = diff[0]
        elif int(ns[p]) != int(counts[p]):
            fm[p] = m
    return fm, st


def assert_clean(ctx, c, what):
    for v in VARIANTS:
        with ctx.options(**v):
            fm, st, bad = verify(ctx, c)
        assert bad == 0 and st.tolist() == [0] * c.n and (fm == CLEAN).all(), (what, v, np.nonzero(fm != CLEAN)[0][:8])


# ---- clean streams report nothing ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["independent", "lpc", "fast_mode", "segments"])
def test_clean_streams_of_this_library(gpu_ctx, kind):
    frames = 9 * 4096 + 1234  # a partial last packet
    if kind == "independent":
        c = encode_case(gpu_ctx, 16, 2, frames, seed=3)
    elif kind == "lpc":
        c = encode_case(gpu_ctx, 16, 2, frames, seed=4, lpc=1)
    elif kind == "fast_mode":
        c = encode_case(gpu_ctx, 16, 2, frames, seed=5, fast_mode=1)
    else:
        c = encode_case(gpu_ctx, 24, 2, frames, seed=6, segment_packets=4)
    assert_clean(gpu_ctx, c, kind)


@pytest.mark.parametrize("name", ["50.wav", "05.wav"])
def test_clean_chained_reference_audio(gpu_ctx, name):
    ka, pcm = golden_wav(name)
    fmt = alac_amd.make_format(4096, ka["bits"], ka["channels"], ka["rate"])
    frames = pcm.size // fmt.bytes_per_frame
    stream, sizes, _ = gpu_ctx.encode_host(fmt, pcm, frames, segment_packets=0)
    c = packed_case(gpu_ctx, gpu_ctx.magic_cookie(fmt), fmt, stream, sizes, pcm, frames)
    assert_clean(gpu_ctx, c, name)


@pytest.mark.parametrize("depth", [16, 20, 24, 32])
@pytest.mark.parametrize("channels", [1, 2, 6, 8])
def test_clean_depths_and_channels(gpu_ctx, depth, channels):
    c = encode_case(gpu_ctx, depth, channels, 3 * 4096 + 777, seed=depth + channels)
    assert_clean(gpu_ctx, c, (depth, channels))


@pytest.mark.parametrize("kind", ["noise", "wrap32", "noise24"])
def test_clean_escaped_and_wrapping_packets(gpu_ctx, kind):
    frames = 3 * 4096 + 100
    if kind == "wrap32":
        x = np.empty((frames, 2), np.int32)
        x[:, 0] = np.where(np.arange(frames) % 2 == 0, 2 ** 31 - 1, -2 ** 31)
        x[:, 1] = -x[:, 0] - 1
        c = encode_case(gpu_ctx, 32, 2, frames, pcm=x.astype("<i4").view(np.uint8).ravel())
    else:
        depth = 24 if kind == "noise24" else 16
        pcm = np.random.default_rng(9).integers(0, 256, frames * 2 * depth // 8, dtype=np.uint8)
        c = encode_case(gpu_ctx, depth, 2, frames, pcm=pcm)
    assert_clean(gpu_ctx, c, kind)


@pytest.mark.parametrize("fixture", ["forged.npz", "forged_mc.npz"])
def test_clean_forged_foreign_packets(gpu_ctx, fixture):
    """the committed foreign packets against the reference objects' own PCM (tests/golden/forged.npz; forged_mc.npz:
    several elements per packet of 3..8 channels, so the store sites write behind outFirst > 0)"""
    import torch
    z = np.load(os.path.join(GOLD, fixture))
    meta = json.loads(bytes(z["meta"]).decode())
    for m in meta:
        si = m["id"]
        sizes = z[f"s{si}_sizes"].astype(np.int64)
        stream = z[f"s{si}_stream"]
        cookie = z[f"s{si}_cookie"]
        ends = np.cumsum(sizes)
        offs = torch.from_numpy(np.concatenate([[0], ends]).astype(np.int64)).cuda()
        _, ns, _, fmt = gpu_ctx.decode(cookie, torch.from_numpy(stream).cuda(), offs, len(sizes))  # the frame counts only
        ns = ns.cpu().numpy()
        packets = [stream[e - s:e] for s, e in zip(sizes, ends)]
        c = Case(cookie, packets, fmt, np.zeros(len(packets) * fmt.packet_bytes, np.uint8), ns)
        want, woff = z[f"s{si}_pcm"], 0
        for p in range(c.n):
            nb = int(ns[p]) * fmt.bytes_per_frame
            c.expected[p * fmt.packet_bytes:p * fmt.packet_bytes + nb] = want[woff:woff + nb]
            woff += nb
        assert woff == len(want)
        assert_clean(gpu_ctx, c, m)


# ---- seeded differences are found exactly ---------------------------------------------------------------------------------

def seeded(c, packet, frame, channel, byte):
    bps = alac_amd.capi.BPS[c.fmt.bit_depth]
    e = c.expected.copy()
    e[packet * c.fmt.packet_bytes + frame * c.fmt.bytes_per_frame + channel * bps + byte] ^= 0x01
    return e


@pytest.mark.parametrize("depth,channels,channel,byte", [
    (16, 2, 1, 1), (16, 1, 0, 0), (20, 2, 0, 0), (24, 2, 1, 0),  # (24, 2, 1, 0): the shifted-off low byte of a 24-bit sample
    (24, 6, 4, 2), (16, 6, 3, 0), (32, 2, 0, 3), (32, 8, 7, 0)])  # channels 3 / 4 of 5.1: the third element (a CPE)
def test_one_seeded_difference(gpu_ctx, depth, channels, channel, byte):
    c = encode_case(gpu_ctx, depth, channels, 5 * 4096, seed=21)
    for packet, frame in ((0, 0), (2, 1234), (4, 4095)):
        e = seeded(c, packet, frame, channel, byte)
        for v in VARIANTS:
            with gpu_ctx.options(**v):
                fm, st, bad = verify(gpu_ctx, c, expected=e)
            want = np.full(c.n, CLEAN, np.uint32)
            want[packet] = frame
            assert bad == 1 and (st == 0).all() and np.array_equal(fm, want), (v, packet, frame, fm.tolist())


@pytest.mark.parametrize("depth,channels", [(16, 2), (24, 2), (20, 1), (24, 6), (32, 2)])
def test_random_seeded_differences_equal_decode_then_compare(gpu_ctx, depth, channels):
    """a few hundred random byte changes in all: verify == decode + numpy compare"""
    c = encode_case(gpu_ctx, depth, channels, 12 * 4096 + 999, seed=31)
    rng = np.random.default_rng(depth * 10 + channels)
    for rnd in range(6):
        e = c.expected.copy()
        for _ in range(12):
            p = int(rng.integers(0, c.n))
            f = int(rng.integers(0, c.counts[p]))
            i = p * c.fmt.packet_bytes + f * c.fmt.bytes_per_frame + int(rng.integers(0, c.fmt.bytes_per_frame))
            e[i] ^= int(rng.integers(1, 256))
        want_fm, want_st = host_reference(gpu_ctx, c, expected=e)
        for v in ({}, {"dec_fused": 0}, {"decoder_lane": 1}):
            with gpu_ctx.options(**v):
                fm, st, bad = verify(gpu_ctx, c, expected=e)
            assert np.array_equal(fm, want_fm) and np.array_equal(st, want_st), (v, rnd)
            assert bad == int((want_fm != CLEAN).sum())


# ---- damaged streams, frame counts ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("depth,channels", [(16, 2), (24, 2), (16, 6)])
def test_damaged_packets_equal_decode_then_compare(gpu_ctx, depth, channels):
    c = encode_case(gpu_ctx, depth, channels, 10 * 4096, seed=41)
    rng = np.random.default_rng(depth + channels)
    hit = [1, 4, 7]
    s = c.stream.copy()
    starts = np.concatenate([[0], np.cumsum(c.sizes)])
    for p in hit:
        for _ in range(3):
            i = int(starts[p] + rng.integers(0, c.sizes[p]))
            s[i] ^= np.uint8(1 << int(rng.integers(0, 8)))
    want_fm, want_st = host_reference(gpu_ctx, c, stream=s)
    for v in VARIANTS:
        with gpu_ctx.options(**v):
            fm, st, bad = verify(gpu_ctx, c, stream=s)
        assert np.array_equal(fm, want_fm) and np.array_equal(st, want_st), v
        assert bad == int((fm != CLEAN).sum())
        untouched = [p for p in range(c.n) if p not in hit]
        assert (fm[untouched] == CLEAN).all() and (st[untouched] == 0).all()


def test_frame_counts_that_differ(gpu_ctx):
    c = encode_case(gpu_ctx, 16, 2, 4 * 4096 + 1234, seed=51)
    counts = c.counts.copy()
    counts[0] = 100           # expected fewer than decoded
    counts[4] = 4096          # the partial packet decodes 1234
    counts[2] = 0
    for v in VARIANTS:
        with gpu_ctx.options(**v):
            fm, st, bad = verify(gpu_ctx, c, counts=counts)
        assert fm.tolist() == [100, CLEAN, 0, CLEAN, 1234] and bad == 3, v
    # an earlier differing frame wins; one behind the shorter count is not compared
    e = seeded(c, 0, 50, 0, 0)
    e = e.copy()
    e[1 * c.fmt.packet_bytes + 200 * c.fmt.bytes_per_frame] ^= 1
    counts[1] = 150
    fm, _, bad = verify(gpu_ctx, c, expected=e, counts=counts)
    assert fm.tolist()[:2] == [50, 150] and bad == 4
    # NULL counts: every packet full, so the partial last packet reports its decoded count
    fm, _, bad = verify(gpu_ctx, c, counts=None)
    assert fm.tolist() == [CLEAN] * 4 + [1234] and bad == 1


def test_host_form_and_class_agree(gpu_ctx):
    """alac_hip_verify_host returns the count and the same arrays"""
    c = encode_case(gpu_ctx, 24, 2, 6 * 4096, seed=61)
    e = seeded(c, 3, 77, 1, 0)
    lib = gpu_ctx.lib
    fm = np.zeros(c.n, np.uint32)
    st = np.zeros(c.n, np.int32)
    sizes = c.sizes.astype(np.uint32)
    counts = c.counts.astype(np.uint32)
    rc = lib.alac_hip_verify_host(gpu_ctx.h, c.cookie.ctypes.data, c.cookie.size, c.stream.ctypes.data, sizes.ctypes.data,
                                  c.n, e.ctypes.data, counts.ctypes.data, fm.ctypes.data, st.ctypes.data)
    assert rc == 1
    assert fm.tolist() == [CLEAN] * 3 + [77] + [CLEAN] * 2 and (st == 0).all()
    assert lib.alac_hip_verify_host(gpu_ctx.h, c.cookie.ctypes.data, c.cookie.size, c.stream.ctypes.data, sizes.ctypes.data,
                                    c.n, c.expected.ctypes.data, None, None, None) == 0


# ---- alacconvert ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def binary(gpu_ctx):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "convert-utility"), "alacconvert"], stdout=subprocess.DEVNULL)
    return BIN


def run(binary, *args):
    p = subprocess.run([binary] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    return p.returncode, p.stdout, p.stderr


def write_wavs(tmp_path, specs, ext):
    args = []
    for i, (bits, ch, frames, seed) in enumerate(specs):
        src, dst = tmp_path / f"in{i}.wav", tmp_path / f"out{i}{ext[i % len(ext)]}"
        src.write_bytes(co.make_wav(music_like(frames, ch, bits, seed), ch, 44100, bits))
        args += [src, dst]
    return args


@pytest.mark.parametrize("mode", ["single", "batch", "lpc"])
def test_cli_verify_writes_the_same_bytes(binary, tmp_path, mode):
    if mode == "single":
        args = write_wavs(tmp_path, [(16, 2, 4096 * 3 + 5, 71)], [".caf"])
    elif mode == "batch":
        args = ["--batch"] + write_wavs(tmp_path, [(16, 2, 4096 * 2 + 9, 72), (24, 2, 5000, 73), (16, 1, 777, 74),
                                                   (24, 1, 4096 * 4, 75), (16, 2, 33, 76)], [".caf", ".m4a"])
    else:
        args = ["--lpc", "--batch"] + write_wavs(tmp_path, [(16, 2, 4096 * 3 + 11, 77), (24, 1, 9000, 78)], [".m4a", ".caf"])
    outs = [args[i] for i in range(len(args)) if str(args[i]).endswith((".caf", ".m4a"))]
    rc, _, err = run(binary, *args)
    assert rc == 0, err
    plain = [o.read_bytes() for o in outs]
    for o in outs:
        o.unlink()
    rc, _, err = run(binary, "--verify", *args)
    assert rc == 0, err
    assert [o.read_bytes() for o in outs] == plain
    # and every output compares equal to its source
    ins = [args[i - 1] for i in range(len(args)) if str(args[i]).endswith((".caf", ".m4a"))]
    for src, o in zip(ins, outs):
        rc, out, err = run(binary, "--compare", o, src)
        assert rc == 0 and "matches" in out, (out, err)


def test_cli_compare_names_the_packet_and_frame(binary, tmp_path):
    pcm = bytearray(music_like(4096 * 3 + 500, 2, 16, 81))
    src, caf = tmp_path / "in.wav", tmp_path / "out.caf"
    src.write_bytes(co.make_wav(bytes(pcm), 2, 44100, 16))
    rc, _, err = run(binary, src, caf)
    assert rc == 0, err
    assert run(binary, "--compare", caf, src)[0] == 0
    frame = 2 * 4096 + 321
    pcm[frame * 4 + 2] ^= 0x40  # the right channel of sample-frame 8513 = packet 2, frame 321
    bad = tmp_path / "changed.wav"
    bad.write_bytes(co.make_wav(bytes(pcm), 2, 44100, 16))
    rc, out, err = run(binary, "--compare", caf, bad)
    assert rc == 1 and "packet 2, frame 321" in out, (out, err)
    # a reference of another length is no match either
    short = tmp_path / "short.wav"
    short.write_bytes(co.make_wav(bytes(pcm[:4096 * 4]), 2, 44100, 16))
    assert run(binary, "--compare", caf, short)[0] == 1
