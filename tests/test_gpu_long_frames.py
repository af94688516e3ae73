"""Frames above 65 536 samples.  `format_ok` admits frame sizes up to 1 048 576; the rest of the suite stops at 65 536 (one
shape of tests/test_gpu_fuzz.py).  Three things first happen above that:

  * the 65 535-zero cap of the adaptive Golomb run code (ag_enc.c:333-349; golf_sym and the plain coder on the encode side,
    the wide entropy decoder and the lane decoder on the other) — fed here through the stage entry points (the fixture of
    tests/test_long_runs.py), through silent packets whose lengths bracket the first and second firing, and through a sweep
    of silent gaps inside music, where the coder arrives at the run with an adapted mean;
  * the search switch of v1_plan at frame_size / 8 = 65 536 (frames 524 287 / 524 288 / 524 295): stagewise search launches
    in front of the fused final launch of the tiny and latency regimes;
  * everything that scales with the frame: slot capacity, residual planes, the 32-bit sample count of a partial packet,
    blocks per packet, row counters of the in-launch hand-offs, and, with 400 packets of 1 048 576 frames, a residual plane
    above 4 GiB outside the throughput regime.

Every comparison is bit-exact against the CPU oracle (packet bytes, sizes, PCM bytes, coefficient state); the float decode
too, its scale being a power of two.  The tests are ordered from the smallest shape to the largest, so `-x` stops at the
cheapest failure."""
import os
import sys

import numpy as np
import pytest

import alac_amd
from alac_amd.capi import AlacError
from oracle_lib import channel_elements, coded_zero_runs, expand_recipe, interleave_channels, load_long_runs

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import forge  # noqa: E402

pytestmark = pytest.mark.gpu

BPS = {16: 2, 20: 3, 24: 3, 32: 4}


# ---- signals (deterministic; modelled on noisy_music of tests/test_gpu_fuzz.py) -------------------------------------

def pack(a, depth):
    """int64 [frames][channels] -> packed little-endian interleaved PCM"""
    a = np.clip(a, -(1 << (depth - 1)), (1 << (depth - 1)) - 1).astype(np.int64)
    if depth == 16:
        return a.astype("<i2").view(np.uint8).reshape(-1)
    if depth == 32:
        return a.astype("<i4").view(np.uint8).reshape(-1)
    if depth == 20:
        a = a << 4                       # 20-bit samples sit in the top of 3 bytes
    return (a & 0xffffff).astype("<u4").view(np.uint8).reshape(-1, 4)[:, :3].reshape(-1).copy()


def music_samples(seed, frames, channels, depth):
    """a tone per channel with a little noise on it: compresses, never escapes -> int64 [frames][channels]"""
    rng = np.random.default_rng(seed)
    t = np.arange(frames)
    amp = float(1 << (depth - 3))
    cols = []
    for c in range(channels):
        x = amp * 0.5 * np.sin(2 * np.pi * rng.uniform(50, 3000) * t / 44100.0 + rng.uniform(0, 6))
        cols.append(x + rng.standard_normal(frames) * amp * 0.002)
    return np.round(np.stack(cols, axis=1)).astype(np.int64)


def music(seed, frames, channels, depth):
    return pack(music_samples(seed, frames, channels, depth), depth)


def gap_music(seed, frames, channels, depth, gaps):
    """music with silent stretches: gaps = [(first frame, length)]"""
    a = music_samples(seed, frames, channels, depth)
    for at, n in gaps:
        a[at:at + n] = 0
    return pack(a, depth)


def silence(frames, channels, depth):
    return np.zeros(frames * channels * BPS[depth], np.uint8)


def noise(seed, frames, channels, depth):
    """full-scale white noise: an escape packet"""
    rng = np.random.default_rng(seed)
    lim = 1 << (depth - 1)
    return pack(rng.integers(-lim, lim, size=(frames, channels)), depth)


class Batch:
    """packets of one format side by side: pcm [n * packet_bytes] (zeros behind a partial packet's samples), ns [n]"""

    def __init__(self, fmt, parts):
        self.fmt, self.n = fmt, len(parts)
        bpf = fmt.bytes_per_frame
        self.ns = np.array([len(p) // bpf for p in parts], np.int32)
        self.pcm = np.zeros(self.n * fmt.packet_bytes, np.uint8)
        for i, p in enumerate(parts):
            assert len(p) % bpf == 0 and len(p) <= fmt.packet_bytes
            self.pcm[i * fmt.packet_bytes:i * fmt.packet_bytes + len(p)] = p

    def src(self, p):
        a = p * self.fmt.packet_bytes
        return self.pcm[a:a + int(self.ns[p]) * self.fmt.bytes_per_frame]


def oracle_packets(oracle, b, seg_first=None, fast=False, info=None):
    """the oracle's packet for every packet of the batch (segments chain; None: every packet alone) and the final
    coefficient state of every segment; info: a list that receives last_info() of every packet"""
    fmt = b.fmt
    enc = oracle.encoder(fmt.frame_size, fmt.bit_depth, fmt.num_channels, fast=fast)
    seg_first = list(range(b.n + 1)) if seg_first is None else list(seg_first)
    pk, states = [], []
    for s in range(len(seg_first) - 1):
        enc.reset()
        for p in range(seg_first[s], seg_first[s + 1]):
            pk.append(enc.encode_packet(b.src(p), int(b.ns[p])))
            if info is not None:
                info.append(enc.last_info())
        states.append(enc.get_state())
    return pk, states


def gpu_encode(ctx, b, seg_first=None, state=None):
    import torch
    kw = {}
    if (b.ns != b.fmt.frame_size).any():
        kw["num_samples"] = torch.from_numpy(b.ns).cuda()
    if seg_first is not None:
        kw["seg_first"] = torch.tensor(list(seg_first), dtype=torch.int32).cuda()
    if state is not None:
        kw["state"] = state
    return ctx.encode_to_host(b.fmt, torch.from_numpy(b.pcm).cuda(), b.n, **kw)


def assert_packets(stream, sizes, want, what=()):
    assert [int(z) for z in sizes] == [len(w) for w in want], what
    off = 0
    for p, w in enumerate(want):
        assert np.array_equal(stream[off:off + len(w)], w), what + (p,)
        off += len(w)
    assert off == len(stream), what


def gpu_decode(ctx, cookie, packets):
    import torch
    stream = np.concatenate(packets)
    offs = np.concatenate([[0], np.cumsum([len(x) for x in packets])]).astype(np.int64)
    out, ns, st, fmt = ctx.decode(cookie, torch.from_numpy(stream).cuda(), torch.from_numpy(offs).cuda(), len(packets))
    ctx.synchronize()
    return out.cpu().numpy(), ns.cpu().numpy(), st.cpu().numpy()


def assert_round_trip(ctx, b, packets, what=()):
    out, ns, st = gpu_decode(ctx, ctx.magic_cookie(b.fmt), packets)
    assert not st.any(), what + (st.tolist(),)
    assert np.array_equal(ns, b.ns), what
    for p in range(b.n):
        a = p * b.fmt.packet_bytes
        assert np.array_equal(out[a:a + len(b.src(p))], b.src(p)), what + (p,)


def check_parity_and_round_trip(ctx, oracle, b, seg_first=None, what=()):
    want, _ = oracle_packets(oracle, b, seg_first)
    stream, sizes = gpu_encode(ctx, b, seg_first)
    assert_packets(stream, sizes, want, what)
    assert_round_trip(ctx, b, want, what)
    return want


# ---- 1. the stage entry points on the long-run fixture -----------------------------------------------------------------

def test_stage_coders_on_long_zero_runs(gpu_ctx):
    """alac_hip_dyn_comp / alac_hip_dyn_decomp (the plain coder of alac_dev.hpp and the lane decoder's dyn_decomp) on every
    vector of tests/golden/long_runs.npz: the reference's bits and bit counts, and the residuals back"""
    import torch
    fix = load_long_runs()
    assert len(fix) >= 150
    for f in fix:
        pc = expand_recipe(f["recipe"])
        n, bits, kw = len(pc), f["bits"], dict(mb0=f["mb"], pb=f["pb"], kb=f["kb"])
        dpc = torch.from_numpy(np.tile(pc, (2, 1))).cuda()  # two rows: lanes must not interfere
        # the fixture was coded at a start bit offset; the GPU entry point codes from bit 0: compare bits
        stride = (len(f["data"]) + 64 + 3) // 4 * 4
        out, nb = gpu_ctx.dyn_comp(dpc, n, bits, stride, **kw)
        gpu_ctx.synchronize()
        assert nb.cpu().tolist() == [f["nbits"]] * 2, f["id"]
        want = np.unpackbits(f["data"])[f["start_bit"]:f["start_bit"] + f["nbits"]]
        for r in range(2):
            assert np.array_equal(np.unpackbits(out[r].cpu().numpy())[:f["nbits"]], want), (f["id"], r)
        back, nb2, st = gpu_ctx.dyn_decomp(out, n, bits, **kw)
        gpu_ctx.synchronize()
        assert st.cpu().tolist() == [0, 0] and nb2.cpu().tolist() == [f["nbits"]] * 2, f["id"]
        assert torch.equal(back[:, :n], dpc), f["id"]


# ---- 2. the cap through the production encoder and decoder: silence -----------------------------------------------------

SILENT_LENGTHS = [65535, 65536, 65537, 65538, 131071, 131072, 131073, 131074, 140000]


@pytest.mark.parametrize("depth,channels", [(16, 2), (16, 1), (24, 2), (20, 1), (32, 1)])
def test_silent_packets_bracket_the_cap(gpu_ctx, oracle, depth, channels):
    """an all-zero packet of N samples per channel codes one ordinary symbol, then a run of N - 1 zeros: N = 65 535..65 538
    bracket the first firing of the cap, 131 071..131 074 the second.  Partial packets of one 140 000-sample format."""
    fmt = alac_amd.make_format(140000, depth, channels)
    b = Batch(fmt, [silence(n, channels, depth) for n in SILENT_LENGTHS])
    info = []
    want, _ = oracle_packets(oracle, b, info=info)
    # the inputs straddle the cap: a run of 65 534 and one of 65 535 zeros take the same 25 bits behind the first symbol's one,
    # the zero behind a capped run is a symbol of its own
    assert [i["bitsU"] for i in info[:3]] == [26, 26, 27]
    if channels == 2:
        assert [i["bitsV"] for i in info[:3]] == [26, 26, 27]
    assert not any(i["escape"] for i in info)
    stream, sizes = gpu_encode(gpu_ctx, b)
    assert_packets(stream, sizes, want, (depth, channels))
    assert_round_trip(gpu_ctx, b, want, (depth, channels))


# ---- 3. the cap with a warmed-up coder: a gap sweep --------------------------------------------------------------------

GAP_FRAME, GAP_AT = 70001, 2000
GAPS = list(range(65525, 65566))


def longest_zero_stretch(r):
    """(first index, length) of the longest stretch of zeros"""
    z = np.flatnonzero(np.concatenate([[1], r != 0, [1]]))
    k = int(np.argmax(np.diff(z)))
    return int(z[k]), int(z[k + 1] - z[k]) - 1


def channel_residuals(oracle, b, packets):
    """the residuals of every channel of every packet, from the oracle's packets alone: the header's mix and predictor
    parameters re-applied to the source (as tests/test_gpu_lpc.py re-forges packets); no packet may be an escape"""
    f, fmt = forge.Forger(oracle), b.fmt
    out = []
    for p, pkt in enumerate(packets):
        esc, hn, shifted, mix_bits, mix_res, params = forge.parse_header(pkt, fmt.num_channels)
        assert not esc, p
        n = int(b.ns[p])
        planes, _, chan_bits = f.planes(b.src(p), n, fmt.bit_depth, fmt.num_channels, mix_bits, mix_res, shifted)
        out.append([f._residuals(planes[c].astype(np.int32), n, cp, chan_bits) for c, cp in enumerate(params)])
    return out


def gap_batch(depth, channels, gaps):
    """one packet per gap length: 2 000 samples of music, the silent gap, music to the end (the same music in every packet)"""
    fmt = alac_amd.make_format(GAP_FRAME, depth, channels)
    return Batch(fmt, [gap_music(300 + depth + channels, GAP_FRAME, channels, depth, [(GAP_AT, g)]) for g in gaps])


GAP_SHAPES = [(16, 1), (16, 2), (24, 2)]


@pytest.mark.parametrize("depth,channels", GAP_SHAPES)
def test_gap_sweep_across_the_cap(gpu_ctx, oracle, depth, channels):
    """2 000 samples of music, G silent samples, music to the end, for every G of 65 525..65 565: the stretch of zero residuals
    walks across 65 535 one sample at a time, behind a coder the music has warmed up"""
    b = gap_batch(depth, channels, GAPS)
    want, _ = oracle_packets(oracle, b)
    seen = {longest_zero_stretch(r)[1] for per_packet in channel_residuals(oracle, b, want) for r in per_packet}
    assert set(range(65530, 65551)) <= seen, sorted(seen)
    stream, sizes = gpu_encode(gpu_ctx, b)
    assert_packets(stream, sizes, want, (depth, channels))
    assert_round_trip(gpu_ctx, b, want, (depth, channels))


def gap_run(r):
    """(index of its first zero, zeros swallowed) of the longest coded zero run of a channel"""
    return max(coded_zero_runs(r), key=lambda run: run[1])


@pytest.mark.parametrize("depth,channels", GAP_SHAPES)
def test_gap_sweep_with_coded_runs_across_the_cap(gpu_ctx, oracle, depth, channels):
    """A stretch of zero residuals of 65 535 is not a RUN of 65 535: behind music the first zeros (60 to 130 here) are ordinary
    symbols until the coder's mean has decayed, so the sweep above stays below the cap in the coder's own terms (a build with
    the cap moved to 65 534 in golf_sym or in the entropy decoder passes it).  This sweep is placed by the oracle: a probe
    packet gives, per channel, the gap length at which the coded run is 65 535, and the gaps run from 12 below the lower of
    them to 6 above the higher.  From the oracle's packets alone: every channel's coded run takes every length of
    65 525..65 535 — among them 65 534 followed by a non-zero symbol, which decodes differently if zero mode is left one zero
    early — and is capped in the packets beyond."""
    probe = gap_batch(depth, channels, [65000])
    at = []  # per channel: the gap whose run is exactly 65 535
    for r in channel_residuals(oracle, probe, oracle_packets(oracle, probe)[0])[0]:
        first, stretch = longest_zero_stretch(r)
        run_first, run = gap_run(r)
        assert first <= run_first and run_first + run == first + stretch  # the run ends the stretch
        at.append(65000 + 65535 - run)
    gaps = list(range(min(at) - 12, max(at) + 7))
    assert len(gaps) <= 80 and GAP_AT + gaps[-1] + 1000 < GAP_FRAME
    b = gap_batch(depth, channels, gaps)
    want, _ = oracle_packets(oracle, b)
    res = channel_residuals(oracle, b, want)
    for c in range(channels):
        runs = [gap_run(per_packet[c])[1] for per_packet in res]
        assert set(range(65525, 65536)) <= set(runs), (c, sorted(set(runs)))
        assert runs.count(65535) >= 5 and max(runs) == 65535, (c, runs)  # longer gaps: capped
    stream, sizes = gpu_encode(gpu_ctx, b)
    assert_packets(stream, sizes, want, (depth, channels))
    assert_round_trip(gpu_ctx, b, want, (depth, channels))


# ---- 4. every code path at the smallest long frame ----------------------------------------------------------------------

PATH_FRAME = 70001  # odd: no multiple of any tile
ENCODE_OPTIONS = [{}, {"narrow": 0}, {"narrow": 0, "fold": 0}, {"thru": 1}, {"fused": 0}, {"split_coder": 0}, {"encoder_lane": 1},
                  {"fast_mode": 1}]
DECODE_OPTIONS = [{}, {"dec_fused": 0}, {"dec_fused": 0, "dec_pair": 0}, {"dec_fused": 0, "dec_direct": 2},
                  {"dec_fused": 0, "dec_direct": 0}, {"decoder_lane": 1}]
_cache = {}


def path_batch(oracle, depth, channels):
    """music, a gap packet of the sweep, silence, full-scale noise (an escape), a partial packet of 65 537 samples and one of
    3, with the oracle's packets — built once per shape"""
    key = ("path", depth, channels)
    if key not in _cache:
        fmt = alac_amd.make_format(PATH_FRAME, depth, channels)
        b = Batch(fmt, [music(11, PATH_FRAME, channels, depth),
                        gap_music(12, PATH_FRAME, channels, depth, [(GAP_AT, 65545)]),
                        silence(PATH_FRAME, channels, depth),
                        noise(13, PATH_FRAME, channels, depth),
                        music(14, 65537, channels, depth),
                        music(15, 3, channels, depth)])
        info = []
        want, _ = oracle_packets(oracle, b, info=info)
        assert [i["escape"] for i in info] == [0, 0, 0, 1, 0, 1]  # three samples cost less raw than their header: a partial escape
        _cache[key] = (b, want)
    return _cache[key]


def opt_id(o):
    return ",".join(f"{k}={v}" for k, v in o.items()) or "default"


PATH_SHAPES = [(16, 2), (24, 2), (16, 1)]
# SetFastMode has no mono form: fast_mode runs with the stereo shapes only
ENCODE_CASES = [(d, c, o) for d, c in PATH_SHAPES for o in ENCODE_OPTIONS if c == 2 or not o.get("fast_mode")]


def case_id(v):
    return opt_id(v) if isinstance(v, dict) else str(v)


@pytest.mark.parametrize("depth,channels,opts", ENCODE_CASES, ids=case_id)
def test_encode_paths_at_70001(gpu_ctx, oracle, depth, channels, opts):
    b, want = path_batch(oracle, depth, channels)
    if opts.get("fast_mode"):
        want, _ = oracle_packets(oracle, b, fast=True)
    with gpu_ctx.options(**opts):
        stream, sizes = gpu_encode(gpu_ctx, b)
    assert_packets(stream, sizes, want, (depth, channels, opts))


@pytest.mark.parametrize("opts", DECODE_OPTIONS, ids=opt_id)
@pytest.mark.parametrize("depth,channels", PATH_SHAPES)
def test_decode_paths_at_70001(gpu_ctx, oracle, depth, channels, opts):
    b, want = path_batch(oracle, depth, channels)
    with gpu_ctx.options(**opts):
        assert_round_trip(gpu_ctx, b, want, (depth, channels, opts))


# ---- 5. the other entry points ------------------------------------------------------------------------------------------

def stream_tensors(packets):
    import torch
    offs = np.concatenate([[0], np.cumsum([len(x) for x in packets])]).astype(np.int64)
    return torch.from_numpy(np.concatenate(packets)).cuda(), torch.from_numpy(offs).cuda()


def float_planes(b):
    """the batch as float32 [channels][n * frame]: sample / 2^(depth - 1), exact"""
    fmt = b.fmt
    x = forge.pcm_to_channels(b.pcm, fmt.bit_depth, fmt.num_channels, b.n * fmt.frame_size)
    return (x.astype(np.float64) / float(1 << (fmt.bit_depth - 1))).astype(np.float32)


@pytest.mark.parametrize("depth", [16, 24])
def test_float_entry_points_at_70001(gpu_ctx, oracle, depth):
    import torch
    b, want = path_batch(oracle, depth, 2)
    fmt, cookie = b.fmt, gpu_ctx.magic_cookie(b.fmt)
    stream, offs = stream_tensors(want)
    x, ns, st, _ = gpu_ctx.decode_float(cookie, stream, offs, b.n)
    gpu_ctx.synchronize()
    assert not st.cpu().numpy().any() and np.array_equal(ns.cpu().numpy(), b.ns)
    assert np.array_equal(x.cpu().numpy(), float_planes(b))  # zeros behind the samples of a partial packet on both sides
    bufs = gpu_ctx.encode_float(fmt, x, num_samples=torch.from_numpy(b.ns).cuda())
    gpu_ctx.synchronize()
    total = int(bufs["offsets"][-1].item())
    assert_packets(bufs["out"][:total].cpu().numpy(), bufs["sizes"].cpu().numpy(), want, (depth,))


# (packet, frame index, channel) of the one corrupted sample: 65 536 is the last sample of the 65 537-sample partial packet,
# 70 000 the last sample of a full one
CORRUPTIONS = [(4, 65536, 1), (1, 65537, 0), (0, 70000, 1)]


@pytest.mark.parametrize("depth", [16, 24])
def test_verify_reports_mismatches_above_65535(gpu_ctx, oracle, depth):
    """alac_hip_verify / alac_hip_verify_float on the clean stream, then with exactly one sample of one packet changed in the
    source: the packet and the frame index of the first mismatch (an index that needs more than 16 bits)"""
    import torch
    b, want = path_batch(oracle, depth, 2)
    fmt, cookie = b.fmt, gpu_ctx.magic_cookie(b.fmt)
    stream, offs = stream_tensors(want)
    d_ns = torch.from_numpy(b.ns).cuda()
    d_pcm = torch.from_numpy(b.pcm).cuda()
    d_x = torch.from_numpy(float_planes(b)).cuda()
    clean = np.full(b.n, -1, np.int32)

    def report(r):
        fm, st, bad = r
        gpu_ctx.synchronize()
        assert not st.cpu().numpy().any()
        return fm.cpu().numpy(), int(bad.item())

    def assert_same(got, fm, nbad, what):
        assert np.array_equal(got[0], fm) and got[1] == nbad, (what, got)

    assert_same(report(gpu_ctx.verify(cookie, stream, offs, b.n, d_pcm, d_ns)), clean, 0, "verify, clean")
    assert_same(report(gpu_ctx.verify_float(cookie, stream, offs, b.n, d_x, d_ns)), clean, 0, "verify_float, clean")
    bps = BPS[depth]
    for p, j, c in CORRUPTIONS:
        assert j < b.ns[p]
        expect = clean.copy()
        expect[p] = j
        at = p * fmt.packet_bytes + (j * 2 + c) * bps + (bps - 2)  # a byte every depth keeps (20 / 24 bits: not the padding)
        d_bad = d_pcm.clone()
        d_bad[at] ^= 0x10
        assert_same(report(gpu_ctx.verify(cookie, stream, offs, b.n, d_bad, d_ns)), expect, 1, ("verify", p, j))
        d_badx = d_x.clone()
        lsb = 2.0 ** -(depth - 1)
        v = float(d_badx[c, p * fmt.frame_size + j].item())
        d_badx[c, p * fmt.frame_size + j] = v + lsb if v + lsb < 1.0 else v - lsb
        assert_same(report(gpu_ctx.verify_float(cookie, stream, offs, b.n, d_badx, d_ns)), expect, 1, ("verify_float", p, j))


@pytest.mark.parametrize("depth", [16, 24])
def test_host_forms_at_70001(gpu_ctx, oracle, depth):
    """alac_hip_encode_host / alac_hip_decode_host once: two full packets and the 65 537-sample partial one as a file of
    independent packets"""
    b, want = path_batch(oracle, depth, 2)
    fmt = b.fmt
    idx = [0, 1, 4]
    total = 2 * PATH_FRAME + 65537
    pcm = np.concatenate([b.src(p) for p in idx])
    stream, sizes, _ = gpu_ctx.encode_host(fmt, pcm, total, segment_packets=1)
    assert_packets(stream, sizes, [want[p] for p in idx], (depth,))
    cookie = gpu_ctx.magic_cookie(fmt)
    out = np.zeros(3 * fmt.packet_bytes, np.uint8)
    ns, st = np.zeros(3, np.uint32), np.zeros(3, np.int32)
    sizes = np.ascontiguousarray(sizes, np.uint32)
    gpu_ctx._check(gpu_ctx.lib.alac_hip_decode_host(gpu_ctx.h, cookie.ctypes.data, cookie.size, stream.ctypes.data,
                                                    sizes.ctypes.data, 3, out.ctypes.data, ns.ctypes.data, st.ctypes.data))
    assert not st.any() and ns.tolist() == [PATH_FRAME, PATH_FRAME, 65537]
    for k, p in enumerate(idx):
        assert np.array_equal(out[k * fmt.packet_bytes:k * fmt.packet_bytes + len(b.src(p))], b.src(p)), (depth, p)


# ---- 6. chained segments of long frames ---------------------------------------------------------------------------------

@pytest.mark.parametrize("opts", [{}, {"overlap_pos": 0}], ids=opt_id)
@pytest.mark.parametrize("depth", [16, 24])
def test_chained_segments_at_70001(gpu_ctx, oracle, depth, opts):
    """segments of 3, 1 and 3 packets: bytes and final coefficient state against the oracle's chains (as
    tests/test_gpu_chained.py::_check), with the positions of a chain overlapped and one after the other"""
    import torch
    key = ("chain", depth)
    seg_first = [0, 3, 4, 7]
    if key not in _cache:
        fmt = alac_amd.make_format(PATH_FRAME, depth, 2)
        parts = [music(20 + p, PATH_FRAME, 2, depth) if p % 3 else gap_music(20 + p, PATH_FRAME, 2, depth, [(GAP_AT, 65530 + 5 * p)])
                 for p in range(7)]
        b = Batch(fmt, parts)
        _cache[key] = (b,) + oracle_packets(oracle, b, seg_first)
    b, want, states = _cache[key]
    state = torch.zeros((3, 64), dtype=torch.int16).cuda()
    with gpu_ctx.options(**opts):
        stream, sizes = gpu_encode(gpu_ctx, b, seg_first, state)
    assert_packets(stream, sizes, want, (depth, opts))
    for s in range(3):
        assert np.array_equal(state[s].cpu().numpy(), states[s]), (depth, opts, s)


# ---- 7. multichannel ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("channels,depth", [(3, 16), (6, 24), (8, 16)])
def test_multichannel_at_66000(gpu_ctx, oracle, channels, depth):
    """the element loop (gather, one mono / stereo batch per element type, splice) with elements of 66 000 samples; the PCM of
    tests/test_gpu_multichannel.py: every element its own stretch of the synthetic workload"""
    frame, n = 66000, 3
    fmt = alac_amd.make_format(frame, depth, channels)
    parts = [(alac_amd.synth_pcm(16 * k, n, alac_amd.make_format(frame, depth, c)), c)
             for k, (ci, c) in enumerate(channel_elements(oracle, channels))]
    pcm = interleave_channels(parts, depth)
    lengths = [frame, 65537, frame]
    b = Batch(fmt, [pcm[p * fmt.packet_bytes:p * fmt.packet_bytes + lengths[p] * fmt.bytes_per_frame] for p in range(n)])
    check_parity_and_round_trip(gpu_ctx, oracle, b, what=(channels, depth))


# ---- 8. foreign streams -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("depth,channels,frame", [(16, 2, 70001), (24, 2, 131075), (32, 1, 70001)])
def test_foreign_streams_with_long_frames(gpu_ctx, oracle, depth, channels, frame):
    """packets another encoder could emit (oracle/forge.py: any order up to 31, any denominator shift, first-order mode,
    shifted-off bytes, partial frames) with rows above 65 536: GPU decode == oracle decode, through the fused launch, the
    separate launches and the lane decoder"""
    rng = np.random.default_rng(9000 + depth + frame)
    pk, pcm, ok = forge.forge_batch(forge.Forger(oracle), rng, 6, depth, channels, frame)
    ck = forge.cookie(frame, depth, channels)
    dec = oracle.decoder(ck)
    bpf = channels * BPS[depth]
    wants = []
    for p, (a, src, k) in enumerate(zip(pk, pcm, ok)):
        ost, want, n = dec.decode_packet(a, bpf)
        assert ost == 0 and n * bpf == len(src)
        if k:
            assert np.array_equal(want, src), ("forger / oracle round trip", p)
        wants.append((want, n))
    assert max(n for _, n in wants) == frame
    for opts in ({}, {"dec_fused": 0}, {"decoder_lane": 1}):
        with gpu_ctx.options(**opts):
            out, ns, st = gpu_decode(gpu_ctx, ck, pk)
        for p, (want, n) in enumerate(wants):
            assert st[p] == 0 and ns[p] == n, (opts, p, ok.info[p], int(st[p]))
            assert np.array_equal(out[p * frame * bpf:p * frame * bpf + n * bpf], want), (opts, p, ok.info[p])


# ---- 9. the search switch -------------------------------------------------------------------------------------------------

def switch_batch(oracle, frame, depth):
    """two chained packets: music, and music with two silent gaps of 70 000"""
    key = ("switch", frame, depth)
    if key not in _cache:
        fmt = alac_amd.make_format(frame, depth, 2)
        b = Batch(fmt, [music(40, frame, 2, depth), gap_music(41, frame, 2, depth, [(5000, 70000), (300000, 70000)])])
        _cache[key] = (b,) + oracle_packets(oracle, b, [0, 2])
    return _cache[key]


# 16-bit stereo on both sides of the boundary under three regimes; one 24-bit case at the boundary, default options
SWITCH_CASES = [(f, 16, o) for f in (524287, 524288, 524295) for o in ({}, {"narrow": 0}, {"fused": 0})] + [(524288, 24, {})]


@pytest.mark.parametrize("frame,depth,opts", SWITCH_CASES, ids=case_id)
def test_search_switch_at_524288(gpu_ctx, oracle, frame, depth, opts):
    """v1_plan turns the fused search off at frame_size / 8 = 65 536 (its progress word is (pass << 16) + rows): from 524 288
    on the tiny and latency regimes run the stagewise search launches in front of their fused final launch, with the overlap
    of packet positions off.  Both sides of the boundary, chained, bytes and state.  (The stage timing of
    alac_hip_profile_end marks the same stages under either search, so which one ran is not visible there.)"""
    import torch
    b, want, states = switch_batch(oracle, frame, depth)
    assert gpu_ctx.regime(b.fmt, 1) == "tiny"  # the regime stays; only the search in front of the final launch changes
    state = torch.zeros((1, 64), dtype=torch.int16).cuda()
    with gpu_ctx.options(**opts):
        stream, sizes = gpu_encode(gpu_ctx, b, [0, 2], state)
    assert_packets(stream, sizes, want, (frame, depth, opts))
    assert np.array_equal(state[0].cpu().numpy(), states[0]), (frame, depth, opts)
    if not opts:
        assert_round_trip(gpu_ctx, b, want, (frame, depth))


# ---- 10. the admitted maximum ---------------------------------------------------------------------------------------------

MAX_FRAME = 1 << 20


@pytest.mark.parametrize("depth,channels", [(16, 2), (32, 1)])
def test_frame_1048576(gpu_ctx, oracle, depth, channels):
    """two independent packets of the largest admitted frame: music, and silence (the cap fires 16 times)"""
    fmt = alac_amd.make_format(MAX_FRAME, depth, channels)
    b = Batch(fmt, [music(50, MAX_FRAME, channels, depth), silence(MAX_FRAME, channels, depth)])
    check_parity_and_round_trip(gpu_ctx, oracle, b, what=(depth, channels))


def test_frame_1048577_is_refused():
    """one sample more than format_ok admits: encode and a decode cookie fail with kALAC_ParamError, nothing is written, and
    the context works afterwards"""
    import ctypes as C
    import torch
    ctx = alac_amd.Context(0)
    bad = alac_amd.make_format(MAX_FRAME + 1, 16, 2)
    assert ctx.lib.alac_hip_encode_workspace_bytes(C.byref(bad), 1, 1) == 0
    pcm = torch.zeros(bad.packet_bytes, dtype=torch.uint8).cuda()
    ws = torch.full((1 << 20,), 0xA5, dtype=torch.uint8).cuda()
    out = torch.full((bad.packet_bytes + 64,), 0x5A, dtype=torch.uint8).cuda()
    sizes = torch.full((1,), 0x7fff0000, dtype=torch.int32).cuda()
    offs = torch.full((2,), 0x7fff000000000000, dtype=torch.int64).cuda()
    torch.cuda.synchronize()
    rc = ctx.lib.alac_hip_encode_segmented(ctx.h, C.byref(bad), pcm.data_ptr(), None, 1, None, 1, 0, None, 0, ws.data_ptr(),
                                           ws.numel(), out.data_ptr(), out.numel(), sizes.data_ptr(), offs.data_ptr())
    assert rc == -50
    ctx.synchronize()
    torch.cuda.synchronize()
    assert bool((out == 0x5A).all()) and bool((ws == 0xA5).all())
    assert int(sizes[0].item()) == 0x7fff0000 and int(offs[1].item()) == 0x7fff000000000000
    ck = forge.cookie(MAX_FRAME + 1, 16, 2)
    stream = torch.zeros(64, dtype=torch.uint8).cuda()
    with pytest.raises(AlacError) as ei:
        ctx.decode(ck, stream, torch.tensor([0, 32], dtype=torch.int64).cuda(), 1)
    assert ei.value.code == -50
    fm = alac_amd.make_format(0, 0, 0, 0)  # ... while the cookie of the admitted maximum is read
    assert ctx.lib.alac_hip_format_from_cookie(forge.cookie(MAX_FRAME, 16, 2).ctypes.data, 24, C.byref(fm)) == 0
    assert fm.frame_size == MAX_FRAME
    # the context is usable afterwards
    fmt = alac_amd.make_format(4096, 16, 2)
    src = alac_amd.synth_pcm(0, 4, fmt)
    s, z = ctx.encode_to_host(fmt, torch.from_numpy(src).cuda(), 4)
    out2, ns, st = gpu_decode(ctx, ctx.magic_cookie(fmt), [s[a:a + int(n)] for a, n in zip(np.cumsum(z) - z, z)])
    assert not st.any() and np.array_equal(out2, src)
    ctx.close()


# ---- 11. a plane above 4 GiB outside the throughput regime ---------------------------------------------------------------

@pytest.mark.parametrize("opts", [{}, {"narrow": 0}], ids=opt_id)
def test_residual_plane_above_4gib(gpu_ctx, oracle, opts):
    """400 independent 16-bit stereo packets of 1 048 576 frames: 832 padded chains, 1088 columns, so the final residual plane
    is (1 048 576 + 16) x 1088 x 4 = 4.56 GB — past 2^32 from 384 packets on — in the tiny regime (default) and the latency
    regime (narrow = 0); so far only the throughput regime had met such a plane (tests/test_gpu_shard125k.py).  Sampled
    packets against the oracle (the highest columns carry the highest offsets), the whole stream decoded back."""
    import torch
    n = 400
    fmt = alac_amd.make_format(MAX_FRAME, 16, 2)
    cols = (2 * n + 63) // 64 * 64 + 256  # enc_layout: chains padded to whole waves + the class regions' padding
    assert cols == 1088 and (MAX_FRAME + 16) * cols * 4 > 1 << 32
    with gpu_ctx.options(**opts):
        assert gpu_ctx.regime(fmt, n) == ("latency" if opts else "tiny")
        d_pcm = gpu_ctx.synth_pcm(0, n, fmt)
        b = gpu_ctx.encode(fmt, d_pcm, n)
        gpu_ctx.synchronize()
    offs = b["offsets"].cpu().numpy()
    sizes = b["sizes"].cpu().numpy().astype(np.int64)
    assert offs[0] == 0 and np.array_equal(np.diff(offs), sizes)
    enc = oracle.encoder(MAX_FRAME, 16, 2)
    for p in (0, 1, 7, 199, 392, 397, 398, 399):
        src = d_pcm[p * fmt.packet_bytes:(p + 1) * fmt.packet_bytes].cpu().numpy()
        enc.reset()
        want = enc.encode_packet(src, MAX_FRAME)
        got = b["out"][int(offs[p]):int(offs[p + 1])].cpu().numpy()
        assert sizes[p] == len(want) and np.array_equal(got, want), (opts, p)
    out, ns, st, _ = gpu_ctx.decode(gpu_ctx.magic_cookie(fmt), b["out"], b["offsets"], n, zero_fill=False)
    gpu_ctx.synchronize()
    assert int(st.abs().sum()) == 0 and bool((ns == MAX_FRAME).all())
    assert torch.equal(out, d_pcm)
    del out, d_pcm, b
    torch.cuda.empty_cache()
    gpu_ctx._ws = None  # ~15 GB of workspace: give it back to the other tests of the session
    torch.cuda.empty_cache()
