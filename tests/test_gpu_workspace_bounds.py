"""Every device call inside exactly the workspace its size query reports ("Confined to the reported workspace").

The session's context keeps one grow-only workspace and passes its whole size, so everywhere else in the suite a call runs in
a workspace as large as the largest any earlier test asked for.  Here every call runs through tests/workspace_guard.py: a
workspace of exactly the reported size with guard bytes on both sides, and each case asserts
  (a) both guards are untouched;
  (b) the outputs are byte-identical with the workspace pre-filled with 0x00, with 0xFF (which reads as "all done" in
      progress words, "ready" in hand-off flags and NaN in the loudness states) and, once per family, in the same buffer
      directly behind a call of another shape (real leftovers);
  (c) they are byte-identical to the same call through the ordinary oversize workspace of the unpatched binding, which the
      rest of the suite pins to the oracle;
  (d) they are not vacuous: encodes decode back to their input, decodes equal the source PCM or the fixture's.
The shapes are the smallest that reach each term of the layouts in alac_capi.hip; the table in DESIGN.md names the case of
every term."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import alac_amd
from alac_amd.capi import AlacError
from workspace_guard import FRONT_GUARD, Fence, GuardDamage, guarded

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BPS = {16: 2, 20: 3, 24: 3, 32: 4}


@pytest.fixture(scope="module")
def pair():
    """(ctx, plain): the context whose workspace requests the tests fence, and an unpatched one with the ordinary oversize
    workspace (64 MiB of 0xA5 before the first call; it grows like any other).  Contexts of this module's own: the session's
    gpu_ctx is never patched."""
    import torch
    ctx, plain = alac_amd.Context(0), alac_amd.Context(0)
    plain._workspace(64 << 20).fill_(0xA5)
    torch.cuda.synchronize()
    yield ctx, plain
    assert "_workspace" not in ctx.__dict__ and "_workspace" not in plain.__dict__
    ctx.close()
    plain.close()


@pytest.fixture
def opts(pair):
    """set the same options on both contexts for one test"""
    import contextlib
    ctx, plain = pair

    @contextlib.contextmanager
    def both(**kw):
        with ctx.options(**kw), plain.options(**kw):
            yield
    return both


# ---- the harness ------------------------------------------------------------------------------------------------------------------
def same(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, "output %d differs" % i)


def confined(pair, call, other=None, offset=0):
    """call(context) -> list of host arrays.  (a), (b), (c) of the module docstring; `other`: a call of another shape for the
    leftovers run.  Returns the outputs."""
    ctx, plain = pair
    want = call(plain)
    for fill in (0x00, 0xFF):
        with guarded(ctx, fill, offset=offset) as g:
            got = call(ctx)
            g.check()
        same(got, want, "workspace pre-filled with 0x%02X" % fill)
    if other is not None:
        with guarded(ctx, 0x00, offset=offset, stale=True) as g:
            other(ctx)
            g.check()
            first = len(g.allocs)
            got = call(ctx)
            g.check()
            assert all(f.reused for f in g.allocs[first:]), "the leftovers run did not re-use the buffer"
        same(got, want, "workspace holding another call's leftovers")
    return want


def refused(ctx, call, pristine=()):
    """the call with one byte less than the reported size: ParamError, and nothing touched — the workspace still holds its
    fill, the guards their pattern, and every tensor of `pristine` (tensor, fill byte) its fill"""
    import torch
    with guarded(ctx, 0x3C, shrink=1) as g:
        with pytest.raises(AlacError) as ei:
            call(ctx)
        assert ei.value.code == -50 and "workspace too small" in str(ei.value), str(ei.value)
        ctx.synchronize()
        assert len(g.allocs) == 1 and g.allocs[0].nbytes == g.allocs[0].asked - 1
        g.check()
        assert bool((g.allocs[0].raw[g.allocs[0].start:g.allocs[0].guard_at] == 0x3C).all()), "the refused call wrote the workspace"
    torch.cuda.synchronize()
    for t, fill in pristine:
        assert bool((t.view(torch.uint8) == fill).all()), "the refused call wrote an output"


# ---- PCM -------------------------------------------------------------------------------------------------------------------------
def pack(v, depth):
    """int64 samples [frames, channels] -> packed interleaved little-endian PCM bytes (20 bits: in the top of 3 bytes)"""
    v = np.asarray(v, np.int64)
    if depth == 20:
        v = v << 4
    b = BPS[depth]
    le = (v.reshape(-1, 1) >> (8 * np.arange(b))) & 0xFF
    return le.astype(np.uint8).reshape(-1)


def tone(frames, channels, depth, k=0):
    t = np.arange(frames, dtype=np.float64)[:, None]
    f = 0.011 * (1 + np.arange(channels))[None, :] + 0.003 * k
    return np.rint(0.3 * (1 << (depth - 1)) * np.sin(2 * np.pi * f * t + k)).astype(np.int64)


def noise(frames, channels, depth, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(-(1 << (depth - 1)), 1 << (depth - 1), (frames, channels), dtype=np.int64)


def packets_pcm(fmt, kinds, seed=1):
    """kinds: list of (signal, frames) -> (PCM bytes of len(kinds) whole packets, zero behind a partial one's frames; the
    frame counts).  signal: "tone", "silence", "noise"."""
    F, ch, d = fmt.frame_size, fmt.num_channels, fmt.bit_depth
    out = np.zeros((len(kinds), F, ch), np.int64)
    for p, (kind, n) in enumerate(kinds):
        if kind == "tone":
            out[p, :n] = tone(n, ch, d, p)
        elif kind == "noise":
            out[p, :n] = noise(n, ch, d, seed + p)
        elif kind == "mixed":  # channel 0 full-scale noise, the others a tone: in 3..8 channels an escaped element beside coded ones
            out[p, :n] = tone(n, ch, d, p)
            out[p, :n, 0] = noise(n, 1, d, seed + p)[:, 0]
    return pack(out.reshape(-1, ch), d), [n for _, n in kinds]


def independent_kinds(F):
    return [("tone", F), ("silence", F), ("noise", F), ("tone", 1), ("noise", min(7, F)), ("tone", F - 1)]


def cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def enc_out(c, b):
    c.synchronize()
    total = int(b["offsets"][-1].item())
    out = [b["out"][:total].cpu().numpy(), b["sizes"].cpu().numpy(), b["offsets"].cpu().numpy()]
    if "clipped" in b:
        out.append(b["clipped"].cpu().numpy())
    return out


def encode_call(fmt, pcm, ns, seg=None, chain=False, bound=0):
    """-> call(context) -> [stream, sizes, offsets (, state after, stream 2, sizes 2, offsets 2, state after 2)].  chain: the
    table's segments with state out, then the same packets again with that state in.  bound: the caller's bound on the longest
    segment (alac_hip_encode_segmented: the table is checked on the device, k_check_segments and its word of the workspace)."""
    import torch
    n = len(ns)
    full = all(x == fmt.frame_size for x in ns)

    def call(c):
        d = cuda(pcm)
        kw = {} if full else {"num_samples": torch.tensor(ns, dtype=torch.int32).cuda()}
        if seg is None:
            return enc_out(c, c.encode(fmt, d, n, **kw))
        sf = torch.tensor(seg, dtype=torch.int32).cuda()
        n16 = int(c.lib.alac_hip_state_int16(C.byref(fmt)))
        state = torch.zeros((len(seg) - 1, n16), dtype=torch.int16).cuda()
        out = enc_out(c, c.encode(fmt, d, n, seg_first=sf, state=state, max_segment_packets=bound, **kw)) + [state.cpu().numpy()]
        if chain:
            out += enc_out(c, c.encode(fmt, d, n, seg_first=sf, state=state, state_in=True, max_segment_packets=bound, **kw))
            out.append(state.cpu().numpy())
        return out
    return call


def decode_host(c, fmt, stream, sizes):
    """-> (pcm bytes, frame counts, status) of a stream, through context c"""
    offs = np.concatenate([[0], np.cumsum(np.asarray(sizes, np.int64))])
    pcm, ns, st, _ = c.decode(c.magic_cookie(fmt), cuda(stream), cuda(offs), len(sizes))
    c.synchronize()
    return pcm.cpu().numpy(), ns.cpu().numpy(), st.cpu().numpy()


def decodes_back(plain, fmt, stream, sizes, pcm, ns):
    """(d) for an encode: the stream decodes to its input"""
    assert len(stream) == int(np.sum(sizes)) and len(stream) > 0
    got, gns, st = decode_host(plain, fmt, stream, sizes)
    assert not st.any() and gns.tolist() == list(ns)
    assert got.tobytes() == np.ascontiguousarray(pcm).tobytes(), "the encode does not decode back to its input"


# ---- the detector itself ----------------------------------------------------------------------------------------------------------
def probe_call(nseg, per=10, channels=2, int_source=False):
    import torch

    def call(c):
        rng = np.random.default_rng(nseg)
        table = np.arange(nseg + 1, dtype=np.uint64) * per
        if int_source:
            x = cuda(rng.integers(-30000, 30000, (channels, nseg * per)).astype(np.int32) << 8)
            rep = c.probe_int(x, seg_first_frame=table)
        else:
            x = cuda((rng.integers(-30000, 30000, (channels, nseg * per)) / 32768.0).astype(np.float32))
            rep = c.probe_float(x, seg_first_frame=table)
        c.synchronize()
        return [rep.cpu().numpy()]
    return call


def test_the_detector_reports_damage_at_the_planted_offset(pair):
    """The probes' segment table of 31 segments is (31 + 1) x 8 = 256 bytes, the whole reported size, and the upload writes all
    of it (probe_table_to_device -> upload_segment_table: num_segments + 1 entries).  With the back guard begun 8 bytes inside
    the workspace the last entry (310 = 0x136: no byte of it is a pattern byte) lands on it: check() must name exactly those
    bytes.  The library writes only memory it was given."""
    ctx, _ = pair
    assert int(ctx.lib.alac_hip_float_probe_workspace_bytes(31)) == 256
    with guarded(ctx, 0x00, back_inset=8) as g:
        probe_call(31)(ctx)
        with pytest.raises(GuardDamage) as ei:
            g.check()
    msg = str(ei.value)
    assert "workspace of 256 bytes (the size reported)" in msg, msg
    assert "back guard damaged: 8 bytes, first at -8, last at -1 relative to the workspace's end" in msg, msg
    assert "front guard" not in msg, msg
    # and one entry less leaves the same guard alone: 30 segments are 248 bytes of table in the same 256
    with guarded(ctx, 0x00, back_inset=8) as g:
        probe_call(30)(ctx)
        g.check()
    assert "_workspace" not in ctx.__dict__  # restored


def test_a_fence_is_laid_out_as_documented(pair):
    import torch
    ctx, _ = pair
    f = Fence(torch, ctx.device, 1000, 0x11, offset=8)
    assert f.view.numel() == 1000 and f.view.data_ptr() % 256 == 8 and f.start == FRONT_GUARD + 8
    assert f.raw.numel() - (f.start + 1000) >= 1 << 20 and bool((f.view == 0x11).all())
    f.check()
    f.raw[f.start - 3] = 0
    f.raw[f.start + 1000 + 5] = 0
    with pytest.raises(GuardDamage) as ei:
        f.check()
    assert "first at -3, last at -3 relative to the workspace's start" in str(ei.value)
    assert "first at +5, last at +5 relative to the workspace's end" in str(ei.value)
    big = Fence(torch, ctx.device, 3 << 20, 0)
    assert big.raw.numel() - (big.start + (3 << 20)) >= 3 << 20  # back guard: at least the fenced size


# ---- encode: enc_layout -----------------------------------------------------------------------------------------------------------
def encode_scenarios(pair, fmt, leftovers=False):
    """six independent packets, then the chained table [0, 1, 4, 9] with state out and state in"""
    _, plain = pair
    F = fmt.frame_size
    pcm, ns = packets_pcm(fmt, independent_kinds(F))
    other = None
    if leftovers:
        ofmt = alac_amd.make_format(2 * F + 3, fmt.bit_depth, fmt.num_channels)
        opcm, ons = packets_pcm(ofmt, [("noise", 2 * F + 3), ("tone", 5), ("noise", 2 * F + 3)], seed=9)
        other = encode_call(ofmt, opcm, ons)
    out = confined(pair, encode_call(fmt, pcm, ns), other)
    decodes_back(plain, fmt, out[0], out[1], pcm, ns)
    kinds = [("tone", F), ("noise", F), ("tone", F), ("silence", F), ("tone", F), ("tone", F), ("noise", F), ("tone", F), ("tone", F - 1)]
    pcm, ns = packets_pcm(fmt, kinds, seed=5)
    out = confined(pair, encode_call(fmt, pcm, ns, seg=[0, 1, 4, 9], chain=True))
    decodes_back(plain, fmt, out[0], out[1], pcm, ns)
    decodes_back(plain, fmt, out[4], out[5], pcm, ns)
    same(confined(pair, encode_call(fmt, pcm, ns, seg=[0, 1, 4, 9], bound=5)), out[:4], "the table with the caller's bound")
    return out


@pytest.mark.parametrize("frame", [8, 17, 333, 4096])
@pytest.mark.parametrize("depth,channels", [(16, 2), (24, 2), (32, 2), (16, 1), (20, 1), (32, 1)])
def test_encode_formats(pair, depth, channels, frame):
    encode_scenarios(pair, alac_amd.make_format(frame, depth, channels), leftovers=(depth, channels, frame) == (16, 2, 333))


ENCODE_OPTIONS = [{}, {"split_coder": 0}, {"narrow": 0}, {"narrow": 0, "fold": 0}, {"thru": 1}, {"fused": 0}, {"overlap_pos": 0},
                  {"encoder_lane": 1}, {"fast_mode": 1}, {"stage_taps": 1}, {"lpc": 1}]


@pytest.mark.parametrize("depth,channels", [(16, 2), (24, 1)])
@pytest.mark.parametrize("options", ENCODE_OPTIONS, ids=lambda o: ",".join("%s=%d" % kv for kv in o.items()) or "default")
def test_encode_options(pair, opts, options, depth, channels):
    """every option set that changes which arrays of the layout are used (fast_mode has no mono form: it leaves mono alone)"""
    with opts(**options):
        encode_scenarios(pair, alac_amd.make_format(333, depth, channels))


def bulk_encode(pair, fmt, nseg, first=3):
    """nseg independent packets of the synthetic PCM (every signal class), confined and decoded back"""
    ctx, plain = pair
    pcm = alac_amd.synth_pcm(first, nseg, fmt)
    out = confined(pair, encode_call(fmt, pcm, [fmt.frame_size] * nseg))
    decodes_back(plain, fmt, out[0], out[1], pcm, [fmt.frame_size] * nseg)


@pytest.mark.parametrize("channels,nseg", [(1, 64), (1, 65), (2, 32), (2, 33)])
def test_encode_segment_counts_at_the_lane_padding(pair, channels, nseg):
    """lanes = align_up(segments x channels, 64): the last full wave, and one chain into the next"""
    bulk_encode(pair, alac_amd.make_format(32, 16, channels), nseg)


@pytest.mark.parametrize("frame", [64, 72])
@pytest.mark.parametrize("nseg", [2016, 2017, 2048, 2049])
def test_encode_at_the_split_coder_edge(pair, frame, nseg):
    """bitWordsB / bitsB exist iff the padded lanes are <= kSplitCoderMaxChains = 4096 (4032, 4096, 4096, 4160 lanes here), and
    the launcher's predicate (v1_plan: tiny && split_coder && padded chains <= 4096 && v1_split_at(frame) >= 48) must agree on
    both sides.  v1_split_at(64) = (64 * 2 / 3) / 48 * 48 = 0: at frame 64 the second coder wave never runs, so the layout's
    extra arrays are only reached from frame 72 on (v1_split_at(72) = 48), the smallest such frame."""
    ctx, _ = pair
    fmt = alac_amd.make_format(frame, 16, 2)
    assert ctx.regime(fmt, nseg) == "tiny"
    bulk_encode(pair, fmt, nseg)


@pytest.mark.parametrize("nseg", [1024, 1025])
def test_encode_compaction_counts(pair, opts, nseg):
    """cls: 256 + (numSegments / 1024 + 2) x 8 bytes of per-1024-packet class counts under thru = 1"""
    with opts(thru=1):
        assert pair[0].regime(alac_amd.make_format(16, 16, 2), nseg) == "throughput"
        bulk_encode(pair, alac_amd.make_format(16, 16, 2), nseg)


def test_encode_one_long_frame(pair):
    """65 537 samples: frame / 8 + 1 rows beyond 2^13, the stagewise search (rows of a pass >= 2^16 / 8 ...), wcap above 2^16 words"""
    _, plain = pair
    fmt = alac_amd.make_format(65537, 16, 2)
    pcm, ns = packets_pcm(fmt, [("tone", 65537), ("noise", 40001)])
    out = confined(pair, encode_call(fmt, pcm, ns))
    decodes_back(plain, fmt, out[0], out[1], pcm, ns)


# ---- encode: mc_layout ------------------------------------------------------------------------------------------------------------
MC_KINDS = [("tone", 512), ("mixed", 512), ("tone", 200), ("silence", 512)]


@pytest.mark.parametrize("channels,depth", [(3, 16), (6, 16), (8, 24)])
def test_encode_multichannel(pair, channels, depth):
    _, plain = pair
    fmt = alac_amd.make_format(512, depth, channels)
    pcm, ns = packets_pcm(fmt, MC_KINDS)
    ofmt = alac_amd.make_format(1100, depth, channels)
    opcm, ons = packets_pcm(ofmt, [("noise", 1100)] * 5, seed=4)
    out = confined(pair, encode_call(fmt, pcm, ns), encode_call(ofmt, opcm, ons) if channels == 6 else None)
    decodes_back(plain, fmt, out[0], out[1], pcm, ns)
    # the mixed packet: its first element (channel 0, a mono element in these layouts) is an escape — the escape flag is bit 22
    # of an element that is not partial: tag 3, instance 4, unused 12, partial 1, shift 2 — the tone packet's is not, and the
    # packet is shorter than its raw samples, so a coded element stands beside the escaped one
    first_escape = [int(out[0][int(out[2][p]) + 2] >> 1) & 1 for p in (0, 1)]
    assert first_escape == [0, 1] and out[1][1] < 512 * depth // 8 * channels
    # chained, with state out and in
    seg_out = confined(pair, encode_call(fmt, pcm, ns, seg=[0, 1, 4], chain=True))
    decodes_back(plain, fmt, seg_out[0], seg_out[1], pcm, ns)


# ---- encode_float / encode_int: the stage behind the workspace ----------------------------------------------------------------------
def test_encode_float_dithered_strided_with_clipped_counters(pair):
    """16-bit stereo from the transposed view of a [frames, channels + 1] tensor, TPDF dither, samples beyond full scale"""
    import torch
    ctx, plain = pair
    fmt = alac_amd.make_format(333, 16, 2)
    frames = 2 * 333 + 100
    rng = np.random.default_rng(7)
    x = (0.6 * np.sin(np.arange(frames * 3) * 0.013)).reshape(frames, 3).astype(np.float32)
    x[rng.integers(0, frames, 40), rng.integers(0, 2, 40)] = 1.5
    x[5, 1] = np.nan

    def call(c):
        xt = cuda(x).t()[:2]
        b = c.encode_float(fmt, xt, clipped=True, dither="tpdf", seed=11)
        return enc_out(c, b)

    def other(c):
        c.encode_float(alac_amd.make_format(700, 24, 2), cuda(np.full((2, 2000), 0.25, np.float32)))
    out = confined(pair, call, other)
    assert out[1].size == 3 and out[3].sum() >= 30  # three packets; the clipped samples were counted
    offs = cuda(out[2].astype(np.int64))
    fm, st, bad = plain.verify_float(plain.magic_cookie(fmt), cuda(out[0]), offs, 3, cuda(x).t()[:2], dither="tpdf", seed=11)
    plain.synchronize()
    assert int(bad.item()) == 0 and not st.cpu().numpy().any()  # (d): the stream holds the dithered source


def test_encode_float_24_bit_mono(pair):
    import torch
    _, plain = pair
    fmt = alac_amd.make_format(333, 24, 1)
    v = tone(2 * 333 + 332, 1, 24)
    x = (v[:, 0] / float(1 << 23)).astype(np.float32)[None, :]  # on the 24-bit grid: the quantizer gives v back

    def call(c):
        return enc_out(c, c.encode_float(fmt, cuda(x), clipped=True))
    out = confined(pair, call)
    assert not out[3].any()
    pcm = np.zeros(3 * 333, np.int64)
    pcm[:v.shape[0]] = v[:, 0]
    decodes_back(plain, fmt, out[0], out[1], pack(pcm[:, None], 24), [333, 333, 332])


def test_encode_int_packed_3_byte_containers(pair):
    """24-bit stereo from packed 3-byte containers (interleaved): exact"""
    _, plain = pair
    fmt = alac_amd.make_format(333, 24, 2)
    frames = 2 * 333 + 17
    v = np.concatenate([tone(333, 2, 24), noise(333, 2, 24, 3), tone(17, 2, 24, 2)])
    src = pack(v, 24)

    def call(c):
        return enc_out(c, c.encode_int(fmt, cuda(src), container_bytes=3, channel_stride=1, frame_stride=2, clipped=True))
    out = confined(pair, call)
    pcm = np.zeros((3 * 333, 2), np.int64)
    pcm[:frames] = v
    decodes_back(plain, fmt, out[0], out[1], pack(pcm, 24), [333, 333, 17])


def test_encode_int_reduced_with_dither_from_a_strided_source(pair):
    """int32 left-justified -> 16-bit stereo with TPDF dither, every second frame of the tensor"""
    ctx, plain = pair
    fmt = alac_amd.make_format(333, 16, 2)
    frames = 2 * 333 + 1
    big = (tone(2 * frames, 2, 32).T).astype(np.int32)

    def call(c):
        return enc_out(c, c.encode_int(fmt, cuda(big)[:, ::2], clipped=True, dither="tpdf", seed=5))
    out = confined(pair, call)
    want = plain.requantize(fmt, cuda(big)[:, ::2], dither="tpdf", seed=5)
    plain.synchronize()
    got, gns, st = decode_host(plain, fmt, out[0], out[1])
    assert not st.any() and gns.tolist() == [333, 333, 1]
    w = want.cpu().numpy()
    assert w.any() and got[:frames * 4].tobytes() == w[:frames * 4].tobytes()


# ---- the encoder's output at exactly alac_hip_encode_max_output_bytes --------------------------------------------------------------
@pytest.mark.parametrize("frame", [8, 17, 333])
@pytest.mark.parametrize("depth,channels", [(16, 2), (24, 2), (32, 2), (16, 1), (20, 1), (32, 1), (16, 3), (24, 8)])
def test_encode_output_of_escapes_only_at_its_reported_capacity(pair, depth, channels, frame):
    """Every packet full-scale noise: every element an escape of maximal size.  d_out is fenced at exactly
    alac_hip_encode_max_output_bytes ("+8 so word stores may overhang")."""
    import torch
    ctx, plain = pair
    fmt = alac_amd.make_format(frame, depth, channels)
    n = 5
    pcm, ns = packets_pcm(fmt, [("noise", frame)] * n, seed=depth + channels)
    cap = int(ctx.lib.alac_hip_encode_max_output_bytes(C.byref(fmt), n))
    want = encode_call(fmt, pcm, ns)(plain)
    for fill in (0x00, 0xFF):
        fence = Fence(torch, ctx.device, cap, fill, what="d_out")
        bufs = dict(out=fence.view, sizes=torch.empty(n, dtype=torch.int32, device=ctx.device),
                    offsets=torch.empty(n + 1, dtype=torch.int64, device=ctx.device))
        with guarded(ctx, fill) as g:
            got = enc_out(ctx, ctx.encode(fmt, cuda(pcm), n, bufs=bufs))
            g.check()
        fence.check()
        same(got, want, "d_out at its reported capacity, pre-filled with 0x%02X" % fill)
    raw = frame * channels * depth  # bits
    assert all(8 * int(s) > raw for s in want[1]), "a packet is shorter than its raw samples: not an escape"
    assert len(want[0]) <= cap
    decodes_back(plain, fmt, want[0], want[1], pcm, ns)


# ---- decode family: dec_layout, verify_ns_bytes --------------------------------------------------------------------------------------
class Stream:
    def __init__(self, name, cookie, fmt, stream, sizes, pcm=None, ns=None):
        self.name, self.cookie, self.fmt, self.stream = name, np.ascontiguousarray(cookie, np.uint8), fmt, np.ascontiguousarray(stream)
        self.sizes = np.asarray(sizes, np.int64)
        self.offsets = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        self.n = len(self.sizes)
        self.pcm, self.ns = pcm, ns  # the source PCM by packet (own streams) / back to back (fixtures, with ns None)


@pytest.fixture(scope="module")
def own_streams(pair):
    """what the guarded encodes above produce (they are byte-identical to the plain context's, which makes these)"""
    _, plain = pair
    out = []
    for name, fmt, kinds in (("mono", alac_amd.make_format(333, 16, 1), independent_kinds(333)),
                             ("stereo", alac_amd.make_format(333, 24, 2), independent_kinds(333)),
                             ("six", alac_amd.make_format(512, 16, 6), MC_KINDS)):
        pcm, ns = packets_pcm(fmt, kinds)
        r = encode_call(fmt, pcm, ns)(plain)
        out.append(Stream(name, plain.magic_cookie(fmt), fmt, r[0], r[1], pcm, ns))
    return out


def fixture_streams(name):
    z = np.load(os.path.join(GOLD, name))
    out = []
    for m in json.loads(bytes(z["meta"]).decode()):
        si = m["id"]
        cookie = z[f"s{si}_cookie"]
        fmt = alac_amd.Format()
        assert alac_amd.load_library().alac_hip_format_from_cookie(np.ascontiguousarray(cookie).ctypes.data, cookie.size,
                                                                   C.byref(fmt)) == 0
        out.append(Stream("%s:%d" % (name, si), cookie, fmt, z[f"s{si}_stream"], z[f"s{si}_sizes"], z[f"s{si}_pcm"]))
    return out


def decode_call(s):
    def decode(c):
        pcm, ns, st, _ = c.decode(s.cookie, cuda(s.stream), cuda(s.offsets), s.n)
        c.synchronize()
        return [pcm.cpu().numpy(), ns.cpu().numpy(), st.cpu().numpy()]
    return decode


def decode_family_calls(s, expected):
    """the four modes besides decode over one stream -> {mode: call}.  expected: (pcm bytes, frame counts) the verify calls compare with — the
    decode's own output, one sample of packet 0 changed so that the first-mismatch table is not all -1."""
    import torch
    fmt, n = s.fmt, s.n
    frames = n * fmt.frame_size
    exp_pcm, exp_ns = expected
    wrong = exp_pcm.copy()
    if exp_ns[0] > 0:
        wrong[(int(exp_ns[0]) - 1) * fmt.bytes_per_frame] ^= 0x10  # (bit 4: a 20-bit sample's lowest)
    scale = float(1 << (fmt.bit_depth - 1))
    width = BPS[fmt.bit_depth]
    v = np.zeros((frames * fmt.num_channels, 4), np.uint8)
    v[:, 4 - width:] = exp_pcm.reshape(-1, width)
    xs = (v.view("<i4").reshape(frames, fmt.num_channels) >> (32 - 8 * width + (4 if fmt.bit_depth == 20 else 0)))
    xf = np.ascontiguousarray((xs / scale).T.astype(np.float32))  # exact: at most 24 significant bits, or a 32-bit stream's
    exact_float = fmt.bit_depth <= 24

    def args(c):
        return s.cookie, cuda(s.stream), cuda(s.offsets), n

    def decode_float(c):
        pcm, ns, st, _ = c.decode_float(*args(c), channel_stride=frames + 7)
        c.synchronize()
        return [pcm.cpu().numpy(), ns.cpu().numpy(), st.cpu().numpy()]

    def decode_int(c):  # packed 3-byte containers, planar rows 5 containers further apart than they need be
        pcm, ns, st, _ = c.decode_int(*args(c), dtype=torch.uint8, layout="planar", left_justified=fmt.bit_depth <= 24,
                                      bits=24, channel_stride=frames + 5)
        c.synchronize()
        return [pcm.cpu().numpy(), ns.cpu().numpy(), st.cpu().numpy()]

    def verify(c):
        out = []
        for e in (exp_pcm, wrong):
            fm, st, bad = c.verify(*args(c), cuda(e), num_samples=cuda(exp_ns.astype(np.int32)))
            c.synchronize()
            out += [fm.cpu().numpy(), st.cpu().numpy(), bad.cpu().numpy()]
        return out

    def verify_float(c):
        fm, st, bad = c.verify_float(*args(c), cuda(xf), num_samples=cuda(exp_ns.astype(np.int32)))
        c.synchronize()
        return [fm.cpu().numpy(), st.cpu().numpy(), bad.cpu().numpy()]
    calls = dict(decode_float=decode_float, verify=verify, verify_float=verify_float)
    if fmt.bit_depth <= 24:
        calls["decode_int"] = decode_int  # (a 32-bit stream does not fit 3-byte containers)
    return calls, exact_float


def check_stream(pair, s, leftovers=None):
    """all modes of one stream, confined; (d): the decode equals the stream's source"""
    ctx, plain = pair
    fmt = s.fmt
    pcm, ns, st = confined(pair, decode_call(s), leftovers)
    assert not st.any(), (s.name, st.tolist())
    if s.ns is not None:  # own stream: the source by packet, zero behind a partial packet
        assert ns.tolist() == list(s.ns) and pcm.tobytes() == s.pcm.tobytes(), s.name
    else:  # fixture: the reference decoder's PCM, back to back
        at = 0
        for p in range(s.n):
            nb = int(ns[p]) * fmt.bytes_per_frame
            assert pcm[p * fmt.packet_bytes:p * fmt.packet_bytes + nb].tobytes() == s.pcm[at:at + nb].tobytes(), (s.name, p)
            at += nb
        assert at == len(s.pcm) and at > 0, s.name
    calls, exact_float = decode_family_calls(s, (pcm, ns.astype(np.int64)))
    for mode, call in calls.items():
        out = confined(pair, call)
        assert not out[2 if mode.startswith("decode") else 1].any(), (s.name, mode)  # status
        if mode == "verify":
            assert int(out[2][0]) == 0 and (out[0] == -1).all(), (s.name, "the decode's own PCM must verify")
            if ns[0] > 0:
                assert int(out[5][0]) == 1 and int(out[3][0]) == int(ns[0]) - 1, (s.name, "the changed sample must be found")
        elif mode == "verify_float" and exact_float:
            assert int(out[2][0]) == 0, (s.name, "the decode's own samples as floats must verify")
        elif mode == "decode_float":
            assert out[0].any(), s.name
        elif mode == "decode_int":
            assert out[0].any(), s.name


DECODE_OPTIONS = [{}, {"dec_fused": 0}, {"dec_fused": 0, "dec_pair": 0}, {"dec_fused": 0, "dec_direct": 0},
                  {"dec_fused": 0, "dec_direct": 2}, {"decoder_lane": 1}]
DECODE_IDS = [",".join("%s=%d" % kv for kv in o.items()) or "default" for o in DECODE_OPTIONS]


@pytest.mark.parametrize("options", DECODE_OPTIONS, ids=DECODE_IDS)
def test_decode_own_streams(pair, opts, own_streams, options):
    with opts(**options):
        for i, s in enumerate(own_streams):
            # leftovers: the six-channel stream's decode (a larger workspace) in the same buffer first
            check_stream(pair, s, decode_call(own_streams[2]) if i == 1 else None)


@pytest.mark.parametrize("options", DECODE_OPTIONS, ids=DECODE_IDS)
@pytest.mark.parametrize("fixture", ["forged.npz", "forged_mc.npz"])
def test_decode_foreign_fixtures(pair, opts, fixture, options):
    """the committed foreign packets: the generic predictor and the fall-back to the lane decoder.  The workspace is sized from
    the stream's length (alac_hip_decode_workspace_bytes_stream), which is what the binding asks for."""
    with opts(**options):
        for s in fixture_streams(fixture):
            check_stream(pair, s)


@pytest.mark.parametrize("options", DECODE_OPTIONS, ids=DECODE_IDS)
@pytest.mark.parametrize("depth,channels,frame", [(16, 2, 333), (24, 1, 17), (32, 2, 64), (20, 6, 40)])
def test_decode_of_escapes_only_fills_the_stage(pair, opts, options, depth, channels, frame):
    """a batch of maximal packets: the stream is as long as alac_hip_decode_workspace_bytes (the variant without a stream
    length) provides for, so the staged words reach the reported capacity"""
    ctx, plain = pair
    fmt = alac_amd.make_format(frame, depth, channels)
    n = 9
    pcm, ns = packets_pcm(fmt, [("noise", frame)] * n, seed=frame)
    r = encode_call(fmt, pcm, ns)(plain)
    s = Stream("escapes", plain.magic_cookie(fmt), fmt, r[0], r[1], pcm, ns)
    assert all(8 * int(z) > frame * channels * depth for z in s.sizes)
    lib = ctx.lib
    assert int(lib.alac_hip_decode_workspace_bytes(C.byref(fmt), n)) == \
        int(lib.alac_hip_decode_workspace_bytes_stream(C.byref(fmt), n, len(s.stream)))
    with opts(**options):
        check_stream(pair, s)


def fil(count):
    """the bits of an ID_FIL element with `count` payload bytes: tag 6, a 4-bit count or 15 and 8 bits more, the payload"""
    head = [1, 1, 0] + ([int(b) for b in format(count, "04b")] if count < 15 else [1, 1, 1, 1] + [int(b) for b in format(count - 14, "08b")])
    return head + [1, 0] * (4 * count)


def padded_stream(plain, fmt, n, fills):
    """n packets of this library's encoder, `fills` fill elements of 269 bytes in front of each one's element: a legal
    stream longer than n regular packets"""
    pcm = alac_amd.synth_pcm(1, n, fmt)
    r = encode_call(fmt, pcm, [fmt.frame_size] * n)(plain)
    pks = []
    for p in range(n):
        b = np.unpackbits(r[0][int(r[2][p]):int(r[2][p + 1])])
        element = list(b[:int(np.nonzero(b)[0][-1]) - 2])  # without ID_END and the padding
        pks.append(np.packbits(np.array(fil(269) * fills + element + [1, 1, 1], np.uint8)))
    return Stream("padded", plain.magic_cookie(fmt), fmt, np.concatenate(pks), [len(q) for q in pks], pcm, [fmt.frame_size] * n)


@pytest.mark.parametrize("options", DECODE_OPTIONS, ids=DECODE_IDS)
@pytest.mark.parametrize("channels", [1, 2])
def test_decode_of_a_padded_stream_at_the_size_its_length_reports(pair, opts, options, channels):
    """A stream padded with fill elements is longer than the regular bound, and the staging area is sized from the bytes the
    call is given: at the size alac_hip_decode_workspace_bytes_stream reports for the stream's length every packet decodes,
    as it does in the oversize workspace."""
    ctx, plain = pair
    fmt = alac_amd.make_format(256, 16, channels)
    s = padded_stream(plain, fmt, 8, 4)
    lib = ctx.lib
    assert int(lib.alac_hip_decode_workspace_bytes_stream(C.byref(fmt), s.n, len(s.stream))) > \
        int(lib.alac_hip_decode_workspace_bytes(C.byref(fmt), s.n))
    with opts(**options):
        check_stream(pair, s)


@pytest.mark.parametrize("options", DECODE_OPTIONS, ids=DECODE_IDS)
def test_decode_of_a_padded_stream_in_the_regular_workspace(pair, opts, options):
    """The same stream in exactly alac_hip_decode_workspace_bytes (the variant without a stream length), fenced: here the
    result legitimately depends on the bytes given — the packets that do not fit the staged words get status -50 (the
    `capWords - 2` / `- 3` clamps of alac_decode_v1.hip at the capacity a real caller has) — but the guards stay intact, the
    result is the same for every fill, and the packets that fit decode."""
    import torch
    ctx, plain = pair
    fmt = alac_amd.make_format(256, 16, 2)
    s = padded_stream(plain, fmt, 8, 4)
    n, lib = s.n, ctx.lib
    wsb = int(lib.alac_hip_decode_workspace_bytes(C.byref(fmt), n))
    stream, offs = cuda(s.stream), cuda(s.offsets)
    results = []
    with opts(**options):
        for fill in (0x00, 0xFF):
            fence = Fence(torch, ctx.device, wsb, fill)
            out, ns, st = filled(ctx, n * fmt.packet_bytes, torch.uint8, 0), filled(ctx, n, torch.int32, 0), filled(ctx, n, torch.int32, 0)
            torch.cuda.synchronize()
            assert lib.alac_hip_decode(ctx.h, s.cookie.ctypes.data, s.cookie.size, stream.data_ptr(), offs.data_ptr(), n,
                                       fence.view.data_ptr(), wsb, out.data_ptr(), ns.data_ptr(), st.data_ptr()) == 0
            ctx.synchronize()
            fence.check()
            results.append([out.cpu().numpy(), ns.cpu().numpy(), st.cpu().numpy()])
    same(results[1], results[0], "workspace pre-filled with 0xFF")
    out, ns, st = results[0]
    st = st.tolist()
    if options.get("decoder_lane") or options.get("dec_direct") == 2:
        # the first-generation decoder, and the separate launches of a 16-bit stream under dec_direct = 2, read the packets
        # where they lie (no staged copy): everything decodes
        assert st == [0] * n and out.tobytes() == s.pcm.tobytes()
        return
    assert st[0] == 0 and st[-1] == -50 and all(x in (0, -50) for x in st) and st == sorted(st, reverse=True), st
    k = st.index(-50)
    assert out[:k * fmt.packet_bytes].tobytes() == s.pcm[:k * fmt.packet_bytes].tobytes()
    assert not out[k * fmt.packet_bytes:].any()  # failed packets are zeroed


# ---- table-only workspaces: probes, CRC, true peak ----------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 8, 248])
@pytest.mark.parametrize("nseg", [1, 31, 32, 33])
@pytest.mark.parametrize("int_source", [False, True], ids=["float", "int"])
def test_probe_tables(pair, nseg, offset, int_source):
    """(n + 1) x 8 bytes: 31 segments fill 256 bytes to the last, 32 need 8 of the next block.  The probes ask for 8-byte
    alignment only (probe_table_to_device)."""
    out = confined(pair, probe_call(nseg, int_source=int_source), probe_call(40) if nseg == 33 else None, offset=offset)
    assert out[0].shape == (nseg, 8) and out[0][:, 4].all()  # need_bits of every segment


def crc_call(n):
    def call(c):
        data = np.random.default_rng(n).integers(0, 256, n * 100 + 50, dtype=np.uint8)
        ranges = [(100 * i + 3, 90 + (i % 7)) for i in range(n)]
        return [np.asarray(c.pcm_crc32(cuda(data), ranges), np.uint64)]
    return call


@pytest.mark.parametrize("offset", [0, 8, 248])
@pytest.mark.parametrize("n", [1, 16, 17])
def test_crc_tables(pair, n, offset):
    """n x 16 bytes: 16 ranges fill 256 bytes to the last"""
    import zlib
    out = confined(pair, crc_call(n), crc_call(20) if n == 17 else None, offset=offset)
    data = np.random.default_rng(n).integers(0, 256, n * 100 + 50, dtype=np.uint8).tobytes()
    for i, (crc, nb) in enumerate(out[0].tolist()):
        assert nb == 90 + (i % 7) and crc == zlib.crc32(data[100 * i + 3:100 * i + 3 + nb])


def true_peak_call(nseg, channels=2, rate=48000, per=130):
    def call(c):
        rng = np.random.default_rng(nseg)
        x = cuda((rng.integers(-30000, 30000, (channels, nseg * per)) / 32768.0).astype(np.float32))
        peaks, rep = c.true_peak_float(x, rate, seg_first_frame=np.arange(nseg + 1, dtype=np.uint64) * per)
        c.synchronize()
        return [peaks.cpu().numpy(), rep.cpu().numpy()]
    return call


@pytest.mark.parametrize("offset", [0, 8, 248])
@pytest.mark.parametrize("nseg", [1, 15, 16, 17])
def test_true_peak_tables(pair, nseg, offset):
    """2 (n + 1) x 8 bytes: 15 segments fill 256 bytes to the last.  per = 130 frames: two runs of the 4x interpolator and a
    short one in every segment."""
    out = confined(pair, true_peak_call(nseg), true_peak_call(21, channels=3) if nseg == 17 else None, offset=offset)
    assert out[0].shape == (nseg, 2) and (out[0] > 0.5).all()


# ---- loudness: loudness_layout, loudness_bounds ------------------------------------------------------------------------------------
def chunk_frames(rate):
    hop = rate // 10
    L = max(d for d in range(1, 65) if hop % d == 0)
    return L if L >= 16 else min(d for d in range(16, hop + 1) if hop % d == 0)


def loudness_call(rate, channels, table, int_source=False):
    def call(c):
        frames = int(table[-1])
        t = np.arange(frames)[None, :] * (0.05 + 0.01 * np.arange(channels))[:, None]
        x = 0.4 * np.sin(t)
        if int_source:
            e, rep = c.loudness_int(cuda(np.rint(x * 32767).astype(np.int16)), rate, seg_first_frame=np.asarray(table, np.uint64))
        else:
            e, rep = c.loudness_float(cuda(x.astype(np.float32)), rate, seg_first_frame=np.asarray(table, np.uint64))
        c.synchronize()
        return [e.cpu().numpy(), rep.cpu().numpy()]
    return call


def loudness_tables(rate):
    """name -> segment table (first frames)"""
    L, hop = chunk_frames(rate), rate // 10
    k = (2 * hop + L - 1) // L + 3  # chunks of a little more than two rows
    ragged = [1, k, 1, 1, 2 * k, 3, 1]  # chunks per segment; every segment one frame more: a short chunk and a short group each
    return {"k_chunks": [0, k * L], "k_chunks_and_a_frame": [0, k * L + 1],
            "every_segment_a_frame_over": np.concatenate([[0], np.cumsum([m * L + 1 for m in ragged])]).tolist(),
            "257_chunks": [0, 257 * L], "257_chunks_and_a_frame_then_one_chunk": [0, 257 * L + 1, 258 * L + 2]}


@pytest.mark.parametrize("offset", [0, 8])
@pytest.mark.parametrize("channels", [1, 2, 3])
@pytest.mark.parametrize("rate", [8000, 8010, 48000])
def test_loudness(pair, rate, channels, offset):
    """rates of chunks of 50, 89 (the only class above 64) and 64 frames.  Base offset 8 (mod 32): the arrays start 24 bytes
    further on, inside the layout's "+ 256"."""
    ctx, _ = pair
    L = chunk_frames(rate)
    assert L == {8000: 50, 8010: 89, 48000: 64}[rate]
    lib = ctx.lib
    for name, table in loudness_tables(rate).items():
        nseg, frames = len(table) - 1, table[-1]
        if name == "every_segment_a_frame_over":
            # total_frames / L + num_segments is met with equality: every segment ends in a short chunk (and a short group)
            chunks = sum((b - a + L - 1) // L for a, b in zip(table[:-1], table[1:]))
            assert chunks == frames // L + nseg
        other = loudness_call(rate, channels, [0, 300 * L + 5], int_source=True) if name == "k_chunks_and_a_frame" else None
        out = confined(pair, loudness_call(rate, channels, table), other, offset=offset)
        rows = int(lib.alac_hip_loudness_rows(rate, frames, np.asarray(table, np.uint64).ctypes.data, nseg))
        assert out[0].shape == (rows, channels) and rows >= 2 and np.isfinite(out[0]).all() and (out[0] > 0).all(), name
        assert out[1].shape == (nseg, 8), name


# ---- reported size - 1: refused, nothing touched -----------------------------------------------------------------------------------
def filled(ctx, shape, dtype, byte):
    import torch
    t = torch.empty(shape, dtype=dtype, device=ctx.device)
    t.view(torch.uint8).fill_(byte)
    return t


def test_one_byte_less_is_refused_encode(pair, opts):
    """alac_hip_encode_workspace_bytes always counts the LPC table behind the layout, and the call asks for it only under
    option lpc: there the reported size is exactly what the call needs.  3..8 channels have no LPC table."""
    import torch
    ctx, _ = pair
    for fmt, options in ((alac_amd.make_format(333, 16, 2), {"lpc": 1}), (alac_amd.make_format(512, 16, 6), {})):
        n = 4
        pcm, ns = packets_pcm(fmt, [("tone", fmt.frame_size)] * n)
        bufs = dict(out=filled(ctx, int(ctx.lib.alac_hip_encode_max_output_bytes(C.byref(fmt), n)), torch.uint8, 0x5A),
                    sizes=filled(ctx, n, torch.int32, 0x5A), offsets=filled(ctx, n + 1, torch.int64, 0x5A))
        with opts(**options):
            refused(ctx, lambda c: c.encode(fmt, cuda(pcm), n, bufs=bufs), [(t, 0x5A) for t in bufs.values()])


def test_one_byte_less_is_refused_encode_float_and_int(pair, opts):
    import torch
    ctx, _ = pair
    fmt = alac_amd.make_format(333, 16, 2)
    n = 3
    bufs = dict(out=filled(ctx, int(ctx.lib.alac_hip_encode_max_output_bytes(C.byref(fmt), n)), torch.uint8, 0x5A),
                sizes=filled(ctx, n, torch.int32, 0x5A), offsets=filled(ctx, n + 1, torch.int64, 0x5A),
                clipped=filled(ctx, n, torch.int32, 0x5A))
    x = np.zeros((2, 999), np.float32)
    with opts(lpc=1):
        refused(ctx, lambda c: c.encode_float(fmt, cuda(x), bufs=bufs, clipped=True), [(t, 0x5A) for t in bufs.values()])
        refused(ctx, lambda c: c.encode_int(fmt, cuda(x.astype(np.int32)), bufs=bufs, clipped=True), [(t, 0x5A) for t in bufs.values()])


def test_one_byte_less_is_refused_decode_family(pair, own_streams):
    import torch
    ctx, _ = pair
    s = own_streams[1]
    fmt, n = s.fmt, s.n
    frames = n * fmt.frame_size
    ns, st = filled(ctx, n, torch.int32, 0x5A), filled(ctx, n, torch.int32, 0x5A)
    a = lambda: (s.cookie, cuda(s.stream), cuda(s.offsets), n)  # noqa: E731
    pcm = filled(ctx, n * fmt.packet_bytes, torch.uint8, 0x5A)
    refused(ctx, lambda c: c.decode(*a(), out=(pcm, ns, st)), [(pcm, 0x5A), (ns, 0x5A), (st, 0x5A)])
    buf = filled(ctx, fmt.num_channels * frames, torch.float32, 0x5A)
    refused(ctx, lambda c: c.decode_float(*a(), out=(buf, ns, st)), [(buf, 0x5A), (ns, 0x5A), (st, 0x5A)])
    ints = filled(ctx, (fmt.num_channels, frames), torch.int32, 0x5A)
    refused(ctx, lambda c: c.decode_int(*a(), out=(ints, ns, st)), [(ints, 0x5A), (ns, 0x5A), (st, 0x5A)])
    # the verify calls allocate their tables inside the binding: the workspace and the guards only
    refused(ctx, lambda c: c.verify(*a(), cuda(s.pcm)))
    refused(ctx, lambda c: c.verify_float(*a(), cuda(np.zeros((fmt.num_channels, frames), np.float32))))


def test_one_byte_less_is_refused_table_only_calls_and_loudness(pair):
    """these bindings allocate their outputs inside the call: the library is called directly, with outputs the test filled"""
    import torch
    ctx, _ = pair
    lib, h = ctx.lib, ctx.h
    x = cuda(np.zeros((2, 4000), np.float32))
    table = np.arange(18, dtype=np.uint64) * 200
    nseg = 17
    rep = filled(ctx, (nseg, 8), torch.int32, 0x5A)
    energy = filled(ctx, (64, 2), torch.float64, 0x5A)
    peaks = filled(ctx, (nseg, 2), torch.float64, 0x5A)
    dig = filled(ctx, (nseg, 4), torch.int32, 0x5A)
    src = alac_amd.capi.IntSource(4, 32, 1, 0, 4000, 1)
    ranges = np.stack([np.arange(nseg, dtype=np.uint64) * 100, np.full(nseg, 50, np.uint64)], axis=1).copy()
    fs = 8010
    calls = {
        "float_probe": (int(lib.alac_hip_float_probe_workspace_bytes(nseg)), lambda ws, nb: lib.alac_hip_float_probe(
            h, x.data_ptr(), 2, 4000, 1, 4000, table.ctypes.data, nseg, ws, nb, rep.data_ptr())),
        "int_probe": (int(lib.alac_hip_int_probe_workspace_bytes(nseg)), lambda ws, nb: lib.alac_hip_int_probe(
            h, x.data_ptr(), C.byref(src), 2, 4000, table.ctypes.data, nseg, ws, nb, rep.data_ptr())),
        "pcm_crc32": (int(lib.alac_hip_pcm_crc32_workspace_bytes(nseg)), lambda ws, nb: lib.alac_hip_pcm_crc32(
            h, x.data_ptr(), 32000, ranges.ctypes.data, nseg, ws, nb, dig.data_ptr())),
        "true_peak_float": (int(lib.alac_hip_true_peak_workspace_bytes(2, nseg)), lambda ws, nb: lib.alac_hip_true_peak_float(
            h, x.data_ptr(), 2, 4000, 1, fs, 4000, table.ctypes.data, nseg, ws, nb, peaks.data_ptr(), rep.data_ptr())),
        "true_peak_int": (int(lib.alac_hip_true_peak_workspace_bytes(2, nseg)), lambda ws, nb: lib.alac_hip_true_peak_int(
            h, x.data_ptr(), C.byref(src), 2, fs, 4000, table.ctypes.data, nseg, ws, nb, peaks.data_ptr(), rep.data_ptr())),
        "loudness_float": (int(lib.alac_hip_loudness_workspace_bytes(fs, 2, 4000, nseg)), lambda ws, nb: lib.alac_hip_loudness_float(
            h, x.data_ptr(), 2, 4000, 1, fs, 4000, table.ctypes.data, nseg, ws, nb, energy.data_ptr(), 64, rep.data_ptr())),
        "loudness_int": (int(lib.alac_hip_loudness_workspace_bytes(fs, 2, 4000, nseg)), lambda ws, nb: lib.alac_hip_loudness_int(
            h, x.data_ptr(), C.byref(src), 2, fs, 4000, table.ctypes.data, nseg, ws, nb, energy.data_ptr(), 64, rep.data_ptr())),
    }
    for name, (reported, call) in calls.items():
        assert reported > 0 and reported % 256 == 0, name
        for offset in (0, 8):
            fence = Fence(torch, ctx.device, reported - 1, 0x3C, offset=offset)
            torch.cuda.synchronize()
            assert call(fence.view.data_ptr(), reported - 1) == -50, name
            assert "workspace too small" in lib.alac_hip_last_error(h).decode(), name
            ctx.synchronize()
            fence.check()
            assert (fence.contents() == 0x3C).all(), name
            for t in (rep, energy, peaks, dig):
                assert bool((t.view(torch.uint8) == 0x5A).all()), name
            # and the reported size itself is taken (the same buffer, one byte more of it)
            whole = Fence(torch, ctx.device, reported, 0x3C, offset=offset)
            torch.cuda.synchronize()
            assert call(whole.view.data_ptr(), reported) == 0, (name, lib.alac_hip_last_error(h).decode())
            ctx.synchronize()
            whole.check()
            for t in (rep, energy, peaks, dig):
                t.view(torch.uint8).fill_(0x5A)
