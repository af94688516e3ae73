"""GPU: alac_hip_decode_int (Context.decode_int) and its host form, bit for bit and byte for byte.  alac_hip_decode's bytes
plus the destination descriptor give, by the numpy restatement of the rule (tests/decode_int_ref.py), the containers the
call must write — at exactly the samples decode writes: the output is filled with a sentinel byte in front of the call, every
container decode writes must equal the reference, and every other byte must still be the sentinel (the gaps between rows, the
pad containers between strided frames, the bytes behind the last container).  Frame counts and statuses equal decode's."""
import json
import os

import numpy as np
import pytest
import torch

import alac_amd
import decode_int_ref as ref
from test_gpu_verify import GOLD, VARIANTS, Case, encode_case

pytestmark = pytest.mark.gpu
C = alac_amd.capi.C
SENT = 0xC3   # sentinel byte
PAD = 37      # containers of gap behind each planar row: the second row starts off every vector alignment
TAIL = 29     # bytes behind the last container
LAYOUT_VARIANTS = [{}, {"dec_fused": 0}, {"decoder_lane": 1}]
DTYPES = {4: torch.int32, 2: torch.int16, 3: torch.uint8}


def offsets_of(c):
    return torch.from_numpy(np.concatenate([[0], np.cumsum(c.sizes)]).astype(np.int64)).cuda()


def decode_reference(ctx, c, stream=None):
    """decode twice into buffers pre-filled with two different bytes: a sample decode wrote is equal in both.
    -> (decode's bytes, written mask [channels, frames], num_samples, status)"""
    stream = c.stream if stream is None else stream
    fmt = c.fmt
    d_stream, offs = torch.from_numpy(stream).cuda(), offsets_of(c)
    runs = []
    for fill in (0x5A, 0xA5):
        pcm = torch.full((c.n * fmt.packet_bytes,), fill, dtype=torch.uint8, device="cuda")
        ns = torch.zeros(c.n, dtype=torch.int32, device="cuda")
        st = torch.zeros(c.n, dtype=torch.int32, device="cuda")
        ctx.decode(c.cookie, d_stream, offs, c.n, out=(pcm, ns, st))
        ctx.synchronize()
        runs.append((pcm.cpu().numpy(), ns.cpu().numpy(), st.cpu().numpy()))
    (a, ns, st), (b, ns2, st2) = runs
    assert np.array_equal(ns, ns2) and np.array_equal(st, st2)
    bps = alac_amd.capi.BPS[fmt.bit_depth]
    written = (a == b).reshape(-1, fmt.num_channels, bps).all(axis=2).T  # [channels, frames]
    return a, np.ascontiguousarray(written), ns, st


class Layout:
    """a destination: container, justification, strides (in containers), the byte offset of container 0 in its buffer"""

    def __init__(self, name, cb, lj=1, bits=None, planar=True, cs=None, fs=None, base=0):
        self.name, self.cb, self.lj, self.bits, self.planar, self.cs, self.fs, self.base = name, cb, lj, bits, planar, cs, fs, base

    def resolve(self, fmt, frames):
        """-> (bits, channel_stride, frame_stride) with the defaults of the compact layouts filled in"""
        bits = (8 * self.cb if self.lj else fmt.bit_depth) if self.bits is None else self.bits
        if self.planar:
            cs, fs = (frames + PAD if self.cs is None else self.cs), (1 if self.fs is None else self.fs)
        else:
            cs, fs = (1 if self.cs is None else self.cs), (fmt.num_channels if self.fs is None else self.fs)
        return bits, cs, fs


PLANAR32 = Layout("planar int32", 4)


def decode_int(ctx, c, lay, stream=None):
    """decode_int into a sentinel-filled byte buffer, through a tensor view of the layout's strides
    -> (the whole buffer's bytes, num_samples, status, the view)"""
    stream = c.stream if stream is None else stream
    fmt = c.fmt
    ch, frames = fmt.num_channels, c.n * fmt.frame_size
    bits, cs, fs = lay.resolve(fmt, frames)
    span = ref.span_bytes(ch, frames, lay.cb, cs, fs)
    buf = torch.full((lay.base + span + TAIL,), SENT, dtype=torch.uint8, device="cuda")
    unit = 3 if lay.cb == 3 else 1
    typed = buf[lay.base:lay.base + span]
    if lay.cb != 3:
        typed = typed.view(DTYPES[lay.cb])
    shape, strides = ((ch, frames), (cs, fs)) if lay.planar else ((frames, ch), (fs, cs))
    view = typed.as_strided(shape + ((3,) if lay.cb == 3 else ()), tuple(s * unit for s in strides) + ((1,) if lay.cb == 3 else ()))
    ns = torch.zeros(c.n, dtype=torch.int32, device="cuda")
    st = torch.zeros(c.n, dtype=torch.int32, device="cuda")
    pcm, ns, st, _ = ctx.decode_int(c.cookie, torch.from_numpy(stream).cuda(), offsets_of(c), c.n, dtype=DTYPES[lay.cb],
                                    layout="planar" if lay.planar else "interleaved", bits=bits,
                                    left_justified=bool(lay.lj), out=(view, ns, st))
    ctx.synchronize()
    assert pcm.data_ptr() == view.data_ptr() and pcm.shape == view.shape and pcm.stride() == view.stride()
    return buf.cpu().numpy(), ns.cpu().numpy(), st.cpu().numpy(), view


def expected_bytes(c, lay, raw, written):
    fmt = c.fmt
    ch, frames = fmt.num_channels, c.n * fmt.frame_size
    bits, cs, fs = lay.resolve(fmt, frames)
    want = np.full(lay.base + ref.span_bytes(ch, frames, lay.cb, cs, fs) + TAIL, SENT, np.uint8)
    ref.decode_int(raw, fmt.bit_depth, ch, lay.cb, bits, lay.lj, cs, fs, want[lay.base:], written)
    return want


def assert_int_equals_decode(ctx, c, what, stream=None, variants=VARIANTS, layouts=(PLANAR32,)):
    for v in variants:
        with ctx.options(**v):
            raw, written, wns, wst = decode_reference(ctx, c, stream)
            results = [(lay, decode_int(ctx, c, lay, stream)) for lay in layouts]
        for lay, (got, ns, st, _) in results:
            assert np.array_equal(ns, wns) and np.array_equal(st, wst), (what, v, lay.name)
            want = expected_bytes(c, lay, raw, written)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (what, v, lay.name, bad[:4].tolist(), got[bad[:4]].tolist(), want[bad[:4]].tolist())


# ---- planar int32, left-justified: every decoder path -----------------------------------------------------------------------

@pytest.mark.parametrize("depth", [16, 20, 24, 32])
@pytest.mark.parametrize("channels", [1, 2])
def test_mono_stereo_depths(gpu_ctx, depth, channels):
    c = encode_case(gpu_ctx, depth, channels, 3 * 4096 + 777, seed=depth + channels)  # a short last packet
    assert_int_equals_decode(gpu_ctx, c, (depth, channels))


@pytest.mark.parametrize("depth,channels", [(16, 3), (24, 6), (20, 6), (32, 8), (16, 8)])
def test_multichannel(gpu_ctx, depth, channels):
    c = encode_case(gpu_ctx, depth, channels, 2 * 4096 + 555, seed=depth * channels)
    assert_int_equals_decode(gpu_ctx, c, (depth, channels))


@pytest.mark.parametrize("depth,channels", [(16, 2), (24, 2), (24, 1)])
def test_odd_frame_size(gpu_ctx, depth, channels):
    c = encode_case(gpu_ctx, depth, channels, 7 * 333 + 100, seed=7, frame_size=333)
    assert_int_equals_decode(gpu_ctx, c, ("frame 333", depth, channels))


@pytest.mark.parametrize("kind", ["noise16", "noise24", "noise20_mono"])
def test_escaped_packets(gpu_ctx, kind):
    depth, channels = {"noise16": (16, 2), "noise24": (24, 2), "noise20_mono": (20, 1)}[kind]
    frames = 3 * 4096 + 100
    pcm = np.random.default_rng(9).integers(0, 256, frames * channels * alac_amd.capi.BPS[depth], dtype=np.uint8)
    if depth == 20:
        pcm[0::3] &= 0xF0
    c = encode_case(gpu_ctx, depth, channels, frames, pcm=pcm)
    assert_int_equals_decode(gpu_ctx, c, kind)


@pytest.mark.parametrize("kind", ["lpc", "fast_mode", "segments"])
def test_encode_modes(gpu_ctx, kind):
    frames = 3 * 4096 + 777
    if kind == "lpc":
        c = encode_case(gpu_ctx, 16, 2, frames, seed=4, lpc=1)
    elif kind == "fast_mode":
        c = encode_case(gpu_ctx, 16, 2, frames, seed=5, fast_mode=1)
    else:
        c = encode_case(gpu_ctx, 24, 2, frames, seed=6, segment_packets=2)
    assert_int_equals_decode(gpu_ctx, c, kind)


@pytest.mark.parametrize("fixture", ["forged.npz", "forged_mc.npz"])
def test_forged_foreign_packets(gpu_ctx, fixture):
    z = np.load(os.path.join(GOLD, fixture))
    meta = json.loads(bytes(z["meta"]).decode())
    for m in meta:
        si = m["id"]
        sizes = z[f"s{si}_sizes"].astype(np.int64)
        stream = z[f"s{si}_stream"]
        cookie = z[f"s{si}_cookie"]
        fmt = alac_amd.Format()
        assert gpu_ctx.lib.alac_hip_format_from_cookie(np.ascontiguousarray(cookie).ctypes.data, cookie.size, C.byref(fmt)) == 0
        ends = np.cumsum(sizes)
        packets = [stream[e - s:e] for s, e in zip(sizes, ends)]
        c = Case(cookie, packets, fmt, np.zeros(0, np.uint8), np.zeros(len(packets), np.int32))
        assert_int_equals_decode(gpu_ctx, c, m)


@pytest.mark.parametrize("depth,channels", [(16, 2), (24, 2), (16, 6), (20, 1)])
def test_damaged_packets(gpu_ctx, depth, channels):
    c = encode_case(gpu_ctx, depth, channels, 10 * 4096, seed=41)
    rng = np.random.default_rng(depth + channels)
    s = c.stream.copy()
    starts = np.concatenate([[0], np.cumsum(c.sizes)])
    for p in (1, 4, 7):
        for _ in range(3):
            i = int(starts[p] + rng.integers(0, c.sizes[p]))
            s[i] ^= np.uint8(1 << int(rng.integers(0, 8)))
    assert_int_equals_decode(gpu_ctx, c, (depth, channels), stream=s)


# ---- the other layouts -----------------------------------------------------------------------------------------------------

def other_layouts(depth, channels, frames):
    """what the call offers besides compact planar int32: right-justified, int16, interleaved, packed 3-byte, transposed views
    with padded strides from both accepted families, row bases off the vector alignment"""
    T, ch = frames, channels
    lays = [Layout("planar int32 right-justified at D", 4, lj=0, bits=depth),
            Layout("interleaved int32", 4, planar=False),
            Layout("frames inner, padded int32", 4, cs=3 * T + 5, fs=3),
            Layout("channels inner, padded int32", 4, planar=False, cs=2, fs=2 * ch + 3),
            Layout("channels inner seen as planar", 4, planar=True, cs=1, fs=ch),
            Layout("planar int32, base 4 mod 16", 4, cs=T + 4, base=4)]
    if depth == 20:
        lays.append(Layout("planar int32 right-justified at 24", 4, lj=0, bits=24))
    if depth == 16:
        lays += [Layout("planar int16", 2), Layout("interleaved int16", 2, planar=False),
                 Layout("planar int16, base 2 mod 8", 2, cs=T + 4, base=2),
                 Layout("planar int16 right-justified", 2, lj=0, bits=16),
                 Layout("frames inner, padded int16", 2, cs=2 * T + 1, fs=2)]
    if depth in (20, 24):
        lays += [Layout("interleaved packed 3-byte", 3, planar=False),
                 Layout("planar packed 3-byte", 3, cs=T + 1),
                 Layout("interleaved packed 3-byte right-justified", 3, lj=0, bits=24, planar=False, base=1)]
    return lays


@pytest.mark.parametrize("depth,channels,frames,frame_size", [(16, 2, 3 * 4096 + 777, 4096), (24, 2, 3 * 4096 + 777, 4096),
                                                              (20, 6, 2 * 4096 + 555, 4096), (16, 2, 7 * 333 + 100, 333),
                                                              (24, 2, 7 * 333 + 100, 333)])
def test_other_layouts(gpu_ctx, depth, channels, frames, frame_size):
    c = encode_case(gpu_ctx, depth, channels, frames, seed=depth + channels + 3, frame_size=frame_size)
    assert_int_equals_decode(gpu_ctx, c, (depth, channels, frame_size), variants=LAYOUT_VARIANTS,
                             layouts=other_layouts(depth, channels, c.n * frame_size))


def test_escaped_packets_in_other_layouts(gpu_ctx):
    """the direct 16-bit stereo escapes have store sites of their own"""
    frames = 3 * 4096 + 100
    pcm = np.random.default_rng(19).integers(0, 256, frames * 4, dtype=np.uint8)
    c = encode_case(gpu_ctx, 16, 2, frames, pcm=pcm)
    assert_int_equals_decode(gpu_ctx, c, "noise16", variants=LAYOUT_VARIANTS, layouts=other_layouts(16, 2, c.n * 4096))


# ---- identity, round trip --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("depth,channels", [(16, 2), (20, 2), (24, 2), (32, 2), (24, 1), (20, 6)])
def test_identity_descriptor_gives_decodes_bytes(gpu_ctx, depth, channels):
    c = encode_case(gpu_ctx, depth, channels, 3 * 4096 + 777, seed=depth)
    d = ref.identity(depth, channels)
    lay = Layout("identity", d["container_bytes"], lj=1, bits=d["bits"], planar=False, cs=d["channel_stride"], fs=d["frame_stride"])
    for v in LAYOUT_VARIANTS:
        with gpu_ctx.options(**v):
            raw, written, wns, wst = decode_reference(gpu_ctx, c)
            got, ns, st, _ = decode_int(gpu_ctx, c, lay)
        assert np.array_equal(ns, wns) and np.array_equal(st, wst)
        bps = alac_amd.capi.BPS[depth]
        wbytes = np.repeat(np.ascontiguousarray(written.T).reshape(-1), bps)
        assert np.array_equal(got[:raw.size], np.where(wbytes, raw, SENT)), v
        assert (got[raw.size:] == SENT).all(), v


@pytest.mark.parametrize("depth", [16, 24, 32])
def test_round_trip_with_encode_int(gpu_ctx, depth):
    """encode_int of a random planar int32 tensor, then decode_int with the same descriptor (right-justified at S = D)"""
    frames = 3 * 4096
    fmt = alac_amd.make_format(4096, depth, 2, 44100)
    lo, hi = -(1 << (depth - 1)), (1 << (depth - 1)) - 1
    walk = np.cumsum(np.random.default_rng(depth).integers(-300, 301, (2, frames)), axis=1) * (1 << (depth - 16))
    x = np.clip(walk, lo, hi).astype(np.int32)
    x[:, :4] = [[lo, hi, 0, -1], [hi, lo, 1, 0]]
    dx = torch.from_numpy(x).cuda()
    bufs = gpu_ctx.encode_int(fmt, dx, bits=depth, left_justified=False)
    gpu_ctx.synchronize()
    total = int(bufs["offsets"][-1])
    n = frames // 4096
    got, ns, st, _ = gpu_ctx.decode_int(gpu_ctx.magic_cookie(fmt), bufs["out"][:total], bufs["offsets"], n, dtype=torch.int32,
                                        bits=depth, left_justified=False)
    gpu_ctx.synchronize()
    assert (st.cpu().numpy() == 0).all() and (ns.cpu().numpy() == 4096).all()
    assert got.shape == dx.shape and torch.equal(got, dx)


# ---- the Python surface, the host form, bad parameters ---------------------------------------------------------------------

def test_default_call_returns_a_compact_zero_filled_tensor(gpu_ctx):
    c = encode_case(gpu_ctx, 24, 2, 3 * 4096 + 5, seed=12)
    frames = c.n * 4096
    pcm, ns, st, fmt = gpu_ctx.decode_int(c.cookie, torch.from_numpy(c.stream).cuda(), offsets_of(c), c.n)
    gpu_ctx.synchronize()
    assert pcm.dtype == torch.int32 and pcm.is_cuda and pcm.is_contiguous() and tuple(pcm.shape) == (2, frames)
    src = ref.samples_of(c.expected, 24, 2)  # zero behind the short packet's frames
    assert np.array_equal(pcm.cpu().numpy(), (src << 8).astype(np.int32))
    # interleaved int32 right-justified: the containers of a 24-in-32 file
    pcm, _, _, _ = gpu_ctx.decode_int(c.cookie, torch.from_numpy(c.stream).cuda(), offsets_of(c), c.n, layout="interleaved",
                                      left_justified=False)
    gpu_ctx.synchronize()
    assert tuple(pcm.shape) == (frames, 2) and pcm.is_contiguous()
    assert np.array_equal(pcm.cpu().numpy(), src.T.astype(np.int32))
    # packed 3-byte containers: decode's own bytes
    pcm, _, _, _ = gpu_ctx.decode_int(c.cookie, torch.from_numpy(c.stream).cuda(), offsets_of(c), c.n, dtype=torch.uint8,
                                      layout="interleaved")
    gpu_ctx.synchronize()
    assert tuple(pcm.shape) == (frames, 2, 3) and np.array_equal(pcm.cpu().numpy().reshape(-1), c.expected)
    # a view into a larger batch tensor
    batch = torch.full((3, 2, frames + 8), 7, dtype=torch.int32, device="cuda")
    ns = torch.zeros(c.n, dtype=torch.int32, device="cuda")
    st = torch.zeros(c.n, dtype=torch.int32, device="cuda")
    view = batch[1, :, 4:4 + frames]
    gpu_ctx.decode_int(c.cookie, torch.from_numpy(c.stream).cuda(), offsets_of(c), c.n, out=(view, ns, st))
    gpu_ctx.synchronize()
    b = batch.cpu().numpy()
    live = np.arange(frames) < c.counts.sum()
    assert np.array_equal(b[1, :, 4:4 + frames][:, live], (src << 8).astype(np.int32)[:, live])
    b[1, :, 4:4 + frames][:, live] = 7
    assert (b == 7).all()
    with pytest.raises(ValueError):
        gpu_ctx.decode_int(c.cookie, torch.from_numpy(c.stream).cuda(), offsets_of(c), c.n, out=(batch[1, :, :frames - 1], ns, st))
    with pytest.raises(ValueError):
        gpu_ctx.decode_int(c.cookie, torch.from_numpy(c.stream).cuda(), offsets_of(c), c.n, dtype=torch.float32)


@pytest.mark.parametrize("depth,channels,cb,lj,planar,cs,fs", [(20, 2, 4, 1, True, None, 1), (16, 2, 2, 1, False, 1, 2),
                                                               (24, 6, 3, 1, False, 1, 7), (24, 2, 4, 0, True, None, 2)])
def test_host_form_equals_device_form(gpu_ctx, depth, channels, cb, lj, planar, cs, fs):
    c = encode_case(gpu_ctx, depth, channels, 2 * 4096 + 99, seed=13)
    fmt = c.fmt
    frames = c.n * 4096
    cs = frames * fs + PAD if cs is None else cs
    bits = 8 * cb if lj else 24
    lay = Layout("host", cb, lj=lj, bits=bits, planar=planar, cs=cs, fs=fs)
    got_dev, dns, dst_, view = decode_int(gpu_ctx, c, lay)
    span = ref.span_bytes(channels, frames, cb, cs, fs)
    out = np.full(span + TAIL, SENT, np.uint8)
    ns = np.zeros(c.n, np.uint32)
    st = np.full(c.n, 7, np.int32)
    sizes = c.sizes.astype(np.uint32)
    desc = alac_amd.capi.IntSource(cb, bits, lj, 0, cs, fs)
    rc = gpu_ctx.lib.alac_hip_decode_int_host(gpu_ctx.h, c.cookie.ctypes.data, c.cookie.size, c.stream.ctypes.data,
                                              sizes.ctypes.data, c.n, out.ctypes.data, C.byref(desc), ns.ctypes.data,
                                              st.ctypes.data)
    assert rc == 0
    assert (st == 0).all() and ns.tolist() == c.counts.tolist() and np.array_equal(dns, ns.astype(dns.dtype))
    # the containers decode writes equal the device form's; those it does not write are zero; the gaps are untouched
    want = got_dev.copy()
    dev_v = ref.load(got_dev, channels, frames, cb, cs, fs)
    live = np.broadcast_to(np.arange(frames) < c.counts.sum(), dev_v.shape)
    ref.store(want, np.where(live, dev_v, 0), cb, cs, fs)
    assert np.array_equal(out, want)
    assert (out == SENT).sum() >= TAIL


def test_bad_parameters_write_nothing(gpu_ctx):
    c = encode_case(gpu_ctx, 24, 2, 2 * 4096, seed=15)
    lib, fmt = gpu_ctx.lib, c.fmt
    T = c.n * fmt.frame_size
    d_stream, offs = torch.from_numpy(c.stream).cuda(), offsets_of(c)
    wsb = int(lib.alac_hip_decode_workspace_bytes_stream(C.byref(fmt), c.n, int(d_stream.numel())))
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    buf = torch.full((2 * T * 4 + 64,), SENT, dtype=torch.uint8, device="cuda")
    ns = torch.full((c.n,), 77, dtype=torch.int32, device="cuda")
    st = torch.full((c.n,), 77, dtype=torch.int32, device="cuda")
    base = buf.data_ptr()

    def call(ptr=base, cb=4, bits=32, lj=1, reserved=0, cs=T, fs=1, desc=True, wsbytes=wsb, cookie=c.cookie):
        d = alac_amd.capi.IntSource(cb, bits, lj, reserved, cs, fs)
        rc = lib.alac_hip_decode_int(gpu_ctx.h, cookie.ctypes.data, cookie.size, d_stream.data_ptr(), offs.data_ptr(), c.n,
                                     ws.data_ptr(), wsbytes, ptr, C.byref(d) if desc else None, ns.data_ptr(), st.data_ptr())
        gpu_ctx.synchronize()
        return rc

    assert call(ptr=None) == -50                      # null d_out
    assert call(desc=False) == -50                    # null descriptor
    for cb in (0, 1, 5, 8):
        assert call(cb=cb) == -50                     # container_bytes not 2, 3 or 4
    for bits in (0, 8, 23, 28, 33, 64):
        assert call(bits=bits) == -50                 # bits not 16, 20, 24 or 32
    assert call(cb=3, bits=32) == -50                 # bits above 8 * container_bytes
    assert call(cb=2, bits=24) == -50
    assert call(bits=20, lj=0) == -50                 # bits below D = 24
    assert call(bits=16, lj=0) == -50
    assert call(cb=2, bits=16) == -50                 # ... in a container narrower than the stream
    assert call(lj=2) == -50                          # left_justified > 1
    assert call(reserved=1) == -50                    # reserved != 0
    assert call(ptr=base + 2) == -50                  # d_out not aligned to a 4-byte container
    assert call(ptr=base + 1) == -50
    assert call(cs=1 << 62) == -50                    # the largest index overflows 64 bits as a byte offset
    assert call(cs=1, fs=1 << 52) == -50
    assert call(cs=T - 1) == -50                      # two samples can share a container
    assert call(cs=3 * T - 1, fs=3) == -50
    assert call(cs=1, fs=1) == -50
    assert call(cs=2, fs=3) == -50
    assert call(fs=0) == -50                          # zero strides
    assert call(cs=0, fs=2) == -50
    assert call(wsbytes=wsb - 1) == -50               # what alac_hip_decode refuses: a workspace below its own
    assert call(cookie=c.cookie[:10]) == -50          # ... a bad cookie
    assert (buf.cpu().numpy() == SENT).all()
    assert (ns.cpu().numpy() == 77).all() and (st.cpu().numpy() == 77).all()
    # a 2-byte container is refused at an odd address only; exactly the decode workspace suffices
    c16 = encode_case(gpu_ctx, 16, 2, 2 * 4096, seed=16)
    d16, o16 = torch.from_numpy(c16.stream).cuda(), offsets_of(c16)
    wsb16 = int(lib.alac_hip_decode_workspace_bytes_stream(C.byref(c16.fmt), c16.n, int(d16.numel())))
    ws16 = torch.empty(wsb16, dtype=torch.uint8, device="cuda")
    d = alac_amd.capi.IntSource(2, 16, 1, 0, T, 1)

    def call16(ptr):
        rc = lib.alac_hip_decode_int(gpu_ctx.h, c16.cookie.ctypes.data, c16.cookie.size, d16.data_ptr(), o16.data_ptr(), c16.n,
                                     ws16.data_ptr(), wsb16, ptr, C.byref(d), ns.data_ptr(), st.data_ptr())
        gpu_ctx.synchronize()
        return rc

    assert call16(base + 1) == -50
    assert (buf.cpu().numpy() == SENT).all() and (st.cpu().numpy() == 77).all()
    assert call16(base + 2) == 0
    assert (st.cpu().numpy() == 0).all()
    assert call() == 0 and call(cs=T, fs=1, bits=24, lj=0) == 0 and call(cs=1, fs=2) == 0
