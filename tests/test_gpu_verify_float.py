"""GPU: alac_hip_verify_float (Context.verify_float) and its host form.  Everything is bit-exact.  The expected answer always
comes from the host: the float source quantized by the numpy restatement of the rule (dither_ref.quantize_dithered; undithered,
quantize of test_gpu_encode_float), the stream decoded with Context.decode, the samples compared one by one — first
differing frame per packet, 0 for an undecodable packet, min(decoded, expected) for a frame count that differs — on every
decoder path of test_gpu_verify.VARIANTS."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import alac_amd
import dither_ref as dr
from test_gpu_encode_float import FAR, make_x, music, quantize, specials
from test_gpu_verify import CLEAN, GOLD, VARIANTS, golden_wav

pytestmark = pytest.mark.gpu
FS = 4096
FEW = ({}, {"dec_fused": 0}, {"decoder_lane": 1})  # where a case multiplies: automatic, separate launches, lane decoder


class Stream:
    def __init__(self, cookie, fmt, stream, sizes):
        self.cookie = np.ascontiguousarray(cookie, np.uint8)
        self.fmt = fmt
        self.stream = np.ascontiguousarray(stream, np.uint8)
        self.sizes = np.asarray(sizes, np.int64)

    @property
    def n(self):
        return len(self.sizes)

    @property
    def offsets(self):
        return np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)


def origin_tensor(origin):
    return None if origin is None else torch.from_numpy(np.asarray(origin, np.uint64).view(np.int64).copy()).cuda()


def counts_of(frames, n, fs):
    return [max(0, min(fs, frames - p * fs)) for p in range(n)]


def encode(ctx, fmt, xt, dither=None, seed=0, origin=None, counts=None, seg_first=None, **options):
    """encode_float of a cuda tensor [C, frames] -> Stream"""
    ns = None if counts is None else torch.tensor(counts, dtype=torch.int32, device="cuda")
    seg = None if seg_first is None else torch.tensor(seg_first, dtype=torch.int32, device="cuda")
    with ctx.options(**options):
        b = ctx.encode_float(fmt, xt, num_samples=ns, seg_first=seg, dither=dither, seed=seed,
                             packet_origin=origin_tensor(origin))
        ctx.synchronize()
    total = int(b["offsets"][-1].item())
    return Stream(ctx.magic_cookie(fmt), fmt, b["out"][:total].cpu().numpy(), b["sizes"].cpu().numpy())


def unpack(out, fmt, n):
    """the bytes alac_hip_decode wrote -> int64 samples [C, n * frame_size], sign-extended at the stream's depth"""
    ch, depth = fmt.num_channels, fmt.bit_depth
    if depth == 16:
        v = out.view("<i2").astype(np.int64)
    elif depth == 32:
        v = out.view("<i4").astype(np.int64)
    else:
        b = out.reshape(-1, 3).astype(np.int64)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        v = (v ^ 0x800000) - 0x800000
        if depth == 20:
            v >>= 4
    return v.reshape(n * fmt.frame_size, ch).T


def restate(x, fmt, n, dither, seed, origin):
    """the samples the float encode path stages for x [C, frames] (zero-padded to n packets: never compared behind a count)"""
    fs = fmt.frame_size
    full = np.zeros((x.shape[0], n * fs), np.float32)
    k = min(x.shape[1], n * fs)
    full[:, :k] = x[:, :k]
    if dither == "tpdf":
        return dr.quantize_dithered(full, fmt.bit_depth, seed, origin=dr.packet_frames(n, fs, origin))[0]
    return quantize(full, fmt.bit_depth)[0]


def host_reference(ctx, s, x, counts=None, dither=None, seed=0, origin=None):
    """Context.decode, then the comparison with the restated samples on the host -> (first mismatch, status)"""
    fs = s.fmt.frame_size
    out, ns, st, _ = ctx.decode(s.cookie, torch.from_numpy(s.stream).cuda(), torch.from_numpy(s.offsets).cuda(), s.n)
    ctx.synchronize()
    got = unpack(out.cpu().numpy(), s.fmt, s.n)
    ns, st = ns.cpu().numpy(), st.cpu().numpy()
    want = restate(x, s.fmt, s.n, dither, seed, origin)
    counts = [fs] * s.n if counts is None else counts
    fm = np.full(s.n, CLEAN, np.uint32)
    for p in range(s.n):
        if st[p] != 0:
            fm[p] = 0
            continue
        m = min(int(ns[p]), int(counts[p]))
        diff = np.nonzero((got[:, p * fs:p * fs + m] != want[:, p * fs:p * fs + m]).any(axis=0))[0]
        if diff.size:
            fm[p] = diff[0]
        elif int(ns[p]) != int(counts[p]):
            fm[p] = m
    return fm, st


def verify(ctx, s, xt, counts=None, dither=None, seed=0, origin=None, stream=None):
    ns = None if counts is None else torch.tensor(list(counts), dtype=torch.int32, device="cuda")
    stream = s.stream if stream is None else stream
    fm, st, bad = ctx.verify_float(s.cookie, torch.from_numpy(stream).cuda(), torch.from_numpy(s.offsets).cuda(), s.n, xt,
                                   num_samples=ns, dither=dither, seed=seed, packet_origin=origin_tensor(origin))
    ctx.synchronize()
    return fm.cpu().numpy().view(np.uint32), st.cpu().numpy(), int(bad.item())


def assert_clean(ctx, s, xt, what, variants=VARIANTS, **kw):
    for v in variants:
        with ctx.options(**v):
            fm, st, bad = verify(ctx, s, xt, **kw)
        assert bad == 0 and st.tolist() == [0] * s.n and (fm == CLEAN).all(), (what, v, np.nonzero(fm != CLEAN)[0][:8], fm[:8])


def assert_equals_host(ctx, s, x, xt, what, variants=VARIANTS, stream=None, **kw):
    ref = s if stream is None else Stream(s.cookie, s.fmt, stream, s.sizes)
    want_fm, want_st = host_reference(ctx, ref, x, **kw)
    for v in variants:
        with ctx.options(**v):
            fm, st, bad = verify(ctx, s, xt, stream=stream, **kw)
        assert np.array_equal(st, want_st), (what, v, st.tolist(), want_st.tolist())
        assert np.array_equal(fm, want_fm), (what, v, fm.tolist(), want_fm.tolist())
        assert bad == int((want_fm != CLEAN).sum()), (what, v)
    return want_fm, want_st


def layouts(x):
    """the same [C, frames] values behind every kind of strides; floats outside the view are FAR"""
    ch, frames = x.shape
    xt = torch.from_numpy(x).cuda()
    views = {"contiguous": xt}
    pad = torch.full((ch, frames + 37), FAR, device="cuda")  # a padded channel stride, not a 16-byte multiple
    pad[:, :frames] = xt
    views["padded"] = pad[:, :frames]
    odd = torch.full((ch, frames + 8), FAR, device="cuda")  # a base 4 but not 16 bytes aligned
    odd[:, 1:frames + 1] = xt
    views["odd_base"] = odd[:, 1:frames + 1]
    views["transposed"] = torch.from_numpy(np.ascontiguousarray(x.T)).cuda().t()
    wide = torch.full((ch, 3 * frames), FAR, device="cuda")  # a frame stride of 3
    wide[:, 0::3] = xt
    views["stride3"] = wide[:, 0::3]
    return views


# ---- 1 / 2: clean streams, every special value of the rule included (make_x) ----------------------------------------------

@pytest.mark.parametrize("channels", [1, 2, 3, 6, 8])
@pytest.mark.parametrize("depth", [16, 20, 24, 32])
def test_clean_depths_channels_layouts(gpu_ctx, depth, channels):
    fmt = alac_amd.make_format(FS, depth, channels, 44100)
    frames = 3 * FS + 777  # a short last packet
    x = make_x(depth, channels, frames, depth + channels)  # music past full scale, NaN, infinities, -0, denormals, ties
    counts = counts_of(frames, 4, FS)
    for dither in (None, "tpdf") if depth != 32 else (None,):
        key = dict(dither=dither, seed=0xABCDEF0123 + depth)
        views = layouts(x)
        s = encode(gpu_ctx, fmt, views["contiguous"], **key)
        assert s.n == 4
        for name, v in views.items():
            assert_clean(gpu_ctx, s, v, (depth, channels, dither, name), VARIANTS if name == "contiguous" else FEW, **key)
            assert_clean(gpu_ctx, s, v, (depth, channels, dither, name, "counts"), FEW, counts=counts, **key)
        assert_equals_host(gpu_ctx, s, x, views["contiguous"], "clean == host", FEW, counts=counts, **key)


@pytest.mark.parametrize("depth", [16, 20, 24, 32])
def test_special_values_dithered_and_not(gpu_ctx, depth):
    """a packet that is nothing but the special values, over and over"""
    fmt = alac_amd.make_format(FS, depth, 2, 44100)
    sp = specials(depth)
    x = np.stack([np.resize(sp, 2 * FS), np.resize(sp[::-1], 2 * FS)]).astype(np.float32)
    xt = torch.from_numpy(x).cuda()
    for dither in (None, "none", "tpdf") if depth != 32 else (None, "none"):
        s = encode(gpu_ctx, fmt, xt, dither=dither, seed=99)
        assert_clean(gpu_ctx, s, xt, (depth, dither), dither=dither, seed=99)
        assert_equals_host(gpu_ctx, s, x, xt, (depth, dither), FEW, dither=dither, seed=99)


@pytest.mark.parametrize("kind", ["odd_frame_size", "odd_origin", "lpc", "fast_mode", "segments"])
def test_clean_shapes_and_encode_options(gpu_ctx, kind):
    depth, ch = (24, 2) if kind in ("odd_origin", "segments") else (16, 2)
    fs = 1021 if kind == "odd_frame_size" else FS
    fmt = alac_amd.make_format(fs, depth, ch, 44100)
    n = 6
    frames = n * fs - 300
    x = make_x(depth, ch, frames, 17)
    xt = torch.from_numpy(x).cuda()
    origin = [1, 2 * fs + 3, 2 ** 32 + 5, 7, 2 ** 40 + 1, 12345] if kind == "odd_origin" else None
    opts = {"lpc": {"lpc": 1}, "fast_mode": {"fast_mode": 1}}.get(kind, {})
    seg = [0, 2, 5, n] if kind == "segments" else None
    for dither in (None, "tpdf"):
        key = dict(dither=dither, seed=4242, origin=origin)
        s = encode(gpu_ctx, fmt, xt, seg_first=seg, **key, **opts)
        assert s.n == n
        assert_clean(gpu_ctx, s, xt, (kind, dither), **key)
        assert_equals_host(gpu_ctx, s, x, xt, (kind, dither), FEW, counts=counts_of(frames, n, fs), **key)


# ---- 3: seeded differences --------------------------------------------------------------------------------------------------

def quiet(channels, frames, seed):
    """floats in [-0.5, 0.5]: every sample far from saturation"""
    return (music(channels, frames, seed) / 1.2 * 0.4).clip(-0.5, 0.5).astype(np.float32)


@pytest.mark.parametrize("depth,channels", [(16, 2), (20, 2), (24, 2), (32, 2), (16, 1), (24, 8), (16, 8), (20, 3)])
def test_one_seeded_difference(gpu_ctx, depth, channels):
    fmt = alac_amd.make_format(FS, depth, channels, 44100)
    n, last = 5, 1234
    frames = (n - 1) * FS + last  # packet 4 is short
    counts = counts_of(frames, n, FS)
    x = quiet(channels, frames, depth + channels)
    top = 2.0 ** (depth - 1)
    sites = [(0, 0, 0), (2, 1233, channels - 1), (1, 2, 0), (3, 4095, channels - 1), (4, last - 1, channels // 2), (1, 7, 0)]
    assert sorted({f % 4 for _, f, _ in sites}) == [0, 1, 2, 3]
    for dither in (None, "tpdf") if depth != 32 else (None,):
        key = dict(dither=dither, seed=31337)
        s = encode(gpu_ctx, fmt, torch.from_numpy(x).cuda(), **key)
        base = restate(x, fmt, n, dither, 31337, None)
        assert np.abs(base).max() <= top - 5  # at least 4 LSB away from saturation
        for packet, frame, c in sites:
            i = packet * FS + frame
            y = x.copy()
            step = max(2.5 / top, 4.0 * float(np.spacing(np.abs(x[c, i]) + np.float32(1e-30))))
            y[c, i] = np.float32(x[c, i] + (step if x[c, i] <= 0 else -step))
            changed = restate(y, fmt, n, dither, 31337, None)
            assert abs(int(changed[c, i]) - int(base[c, i])) >= 2, "the host restatement must see the change"
            assert np.array_equal(np.delete(changed.ravel(), c * changed.shape[1] + i),
                                  np.delete(base.ravel(), c * base.shape[1] + i))
            want = np.full(n, CLEAN, np.uint32)
            want[packet] = frame
            yt = torch.from_numpy(y).cuda()
            for v in VARIANTS:
                with gpu_ctx.options(**v):
                    fm, st, bad = verify(gpu_ctx, s, yt, counts=counts, **key)
                assert bad == 1 and (st == 0).all() and np.array_equal(fm, want), (v, dither, packet, frame, c, fm.tolist())


@pytest.mark.parametrize("depth", [16, 24])
def test_a_change_below_the_grid_is_no_difference(gpu_ctx, depth):
    fmt = alac_amd.make_format(FS, depth, 2, 44100)
    x = quiet(2, 2 * FS, 5)
    top = 2.0 ** (depth - 1)
    i = FS + 321
    x[1, i] = np.float32(3.25 / top)
    y = x.copy()
    y[1, i] = np.float32(x[1, i] + 2.0 ** -30)
    assert y[1, i] != x[1, i], "the float itself changed"
    for dither in (None, "tpdf"):
        key = dict(dither=dither, seed=8)
        assert np.array_equal(restate(x, fmt, 2, dither, 8, None), restate(y, fmt, 2, dither, 8, None))
        s = encode(gpu_ctx, fmt, torch.from_numpy(x).cuda(), **key)
        assert_clean(gpu_ctx, s, torch.from_numpy(y).cuda(), (depth, dither), **key)


# ---- 4: the wrong key -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("depth,channels", [(16, 2), (20, 2), (24, 2), (16, 1), (24, 6)])
def test_wrong_key_equals_host(gpu_ctx, depth, channels):
    fmt = alac_amd.make_format(FS, depth, channels, 44100)
    n = 4
    frames = n * FS - 1000
    counts = counts_of(frames, n, FS)
    x = quiet(channels, frames, 3 * depth + channels)
    xt = torch.from_numpy(x).cuda()
    origin = [0, FS, 2 * FS, 3 * FS]
    s = encode(gpu_ctx, fmt, xt, dither="tpdf", seed=1, origin=origin)
    assert_clean(gpu_ctx, s, xt, "right key", FEW, counts=counts, dither="tpdf", seed=1, origin=origin)
    for what, kw in (("other seed", dict(dither="tpdf", seed=2, origin=origin)),
                     ("dither off", dict(dither=None)),
                     ("dither none", dict(dither="none", seed=1, origin=origin)),
                     ("origin + 1", dict(dither="tpdf", seed=1, origin=[o + 1 for o in origin]))):
        fm, _ = assert_equals_host(gpu_ctx, s, x, xt, what, counts=counts, **kw)
        assert (fm != CLEAN).all() and (fm < 64).all(), (what, fm.tolist())  # these differ in most frames


# ---- 5: other streams -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fixture", ["forged.npz", "forged_mc.npz"])
def test_forged_foreign_packets_equal_host(gpu_ctx, fixture):
    z = np.load(os.path.join(GOLD, fixture))
    meta = json.loads(bytes(z["meta"]).decode())
    for m in meta:
        si = m["id"]
        fmt = alac_amd.make_format(m["frame"], m["depth"], m["channels"], 44100)
        s = Stream(z[f"s{si}_cookie"], fmt, z[f"s{si}_stream"], z[f"s{si}_sizes"])
        x = quiet(m["channels"], s.n * m["frame"], si)
        xt = torch.from_numpy(x).cuda()
        for dither in (None, "tpdf") if m["depth"] != 32 else (None,):
            assert_equals_host(gpu_ctx, s, x, xt, (m["id"], dither), dither=dither, seed=si)
        # the stream's own PCM as on-grid floats: what differs is what the host says differs (the lossy packets at most)
        out, ns, st, _ = gpu_ctx.decode(s.cookie, torch.from_numpy(s.stream).cuda(), torch.from_numpy(s.offsets).cuda(), s.n)
        gpu_ctx.synchronize()
        own = (unpack(out.cpu().numpy(), fmt, s.n) / 2.0 ** (m["depth"] - 1)).astype(np.float32)
        if m["depth"] <= 24:  # exact floats of the decoded samples
            assert_clean(gpu_ctx, s, torch.from_numpy(own).cuda(), (m["id"], "own"), counts=ns.cpu().tolist())


@pytest.mark.parametrize("depth,channels", [(16, 2), (24, 2), (16, 6), (20, 1)])
def test_damaged_packets_and_counts_equal_host(gpu_ctx, depth, channels):
    fmt = alac_amd.make_format(FS, depth, channels, 44100)
    n = 8
    x = quiet(channels, n * FS, depth + 7 * channels)
    xt = torch.from_numpy(x).cuda()
    key = dict(dither="tpdf", seed=5)
    s = encode(gpu_ctx, fmt, xt, **key)
    starts = s.offsets
    rng = np.random.default_rng(depth + channels)
    hit = [1, 4, 6]
    damaged = s.stream.copy()
    damaged[starts[1]] ^= 0x10      # a bit of the element header
    damaged[starts[4] + 2] ^= 0x01  # ... of the header's flags
    for _ in range(3):
        damaged[int(starts[6] + rng.integers(8, s.sizes[6]))] ^= np.uint8(1 << int(rng.integers(0, 8)))
    fm, st = assert_equals_host(gpu_ctx, s, x, xt, "flipped bits", stream=damaged, **key)
    untouched = [p for p in range(n) if p not in hit]
    assert (fm[untouched] == CLEAN).all() and (st[untouched] == 0).all() and (fm[hit] != CLEAN).any()
    # a truncated packet: packet 3 loses its second half, the packets behind it move up
    keep = int(s.sizes[3]) // 2
    cut = np.concatenate([s.stream[:starts[3] + keep], s.stream[starts[4]:]])
    sizes = s.sizes.copy()
    sizes[3] = keep
    t = Stream(s.cookie, fmt, cut, sizes)
    fm, st = assert_equals_host(gpu_ctx, t, x, xt, "truncated", **key)
    assert fm[3] != CLEAN and (np.delete(fm, 3) == CLEAN).all()
    # expected frame counts that differ from the decoded ones, in both directions
    short = encode(gpu_ctx, fmt, xt[:, :n * FS - 3000], **key)  # the last packet decodes 1096 frames
    counts = [FS] * n
    counts[0], counts[2], counts[5], counts[7] = 100, 0, 4095, FS
    fm, _ = assert_equals_host(gpu_ctx, short, x, xt, "counts", counts=counts, **key)
    assert fm.tolist() == [100, CLEAN, 0, CLEAN, CLEAN, 4095, CLEAN, 1096]
    fm, _ = assert_equals_host(gpu_ctx, short, x, xt, "null counts", **key)
    assert fm.tolist() == [CLEAN] * 7 + [1096]


# ---- 6: only the frames in front of the expected count are read ---------------------------------------------------------------

@pytest.mark.parametrize("depth,channels", [(16, 2), (24, 2), (16, 1), (20, 6)])
def test_a_packet_that_decodes_more_than_expected(gpu_ctx, depth, channels):
    """x is a view of exactly T frames inside an allocation whose other floats are 2.0; the stream's last packet holds a
    whole frame_size frames, of which T covers 1234.  (That no float behind T is loaded cannot be shown by a result —
    those frames are not compared either way — so the clamp is in the code of every site; DESIGN.md section 15 lists them.)"""
    fmt = alac_amd.make_format(FS, depth, channels, 44100)
    n = 4
    T = 3 * FS + 1234
    long = quiet(channels, n * FS, depth + channels)
    key = dict(dither="tpdf", seed=77)
    s = encode(gpu_ctx, fmt, torch.from_numpy(long).cuda(), **key)  # every packet decodes 4096 frames
    x = long[:, :T].copy()
    counts = counts_of(T, n, FS)
    flat = torch.full((channels * T + 64,), FAR, device="cuda")   # rows back to back: channel c + 1 starts where c ends
    apart = torch.full((channels, T + 4096), FAR, device="cuda")  # rows apart, 2.0 in front of and behind each
    for name, view in (("rows back to back", flat[:channels * T].view(channels, T)), ("rows apart", apart[:, 8:8 + T])):
        view.copy_(torch.from_numpy(x))
        fm, _ = assert_equals_host(gpu_ctx, s, x, view, name, counts=counts, **key)
        assert fm.tolist() == [CLEAN] * 3 + [1234]
    # the same through a frame stride (one load per sample) and with a difference in front of the count
    wide = torch.full((channels, 3 * T), FAR, device="cuda")
    y = x.copy()
    y[channels - 1, 3 * FS + 1233] += np.float32(0.01)
    wide[:, 0::3] = torch.from_numpy(y)
    fm, _ = assert_equals_host(gpu_ctx, s, y, wide[:, 0::3], "stride 3", counts=counts, **key)
    assert fm.tolist() == [CLEAN] * 3 + [1233]


# ---- 7: the golden audio ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["50.wav", "05.wav"])
def test_golden_audio_chained(gpu_ctx, name):
    """integers through the chained encode, verified against pcm / 32768 as float32: on-grid floats quantize to themselves"""
    ka, pcm = golden_wav(name)
    assert ka["bits"] == 16
    fmt = alac_amd.make_format(FS, 16, ka["channels"], ka["rate"])
    frames = pcm.size // fmt.bytes_per_frame
    stream, sizes, _ = gpu_ctx.encode_host(fmt, pcm, frames, segment_packets=0)
    s = Stream(gpu_ctx.magic_cookie(fmt), fmt, stream, sizes)
    x = (pcm.view("<i2").reshape(frames, ka["channels"]).T.astype(np.float32) / np.float32(32768.0))
    xt = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    assert_clean(gpu_ctx, s, xt, name)  # counts None: verify_float derives the short last packet from x
    assert_clean(gpu_ctx, s, xt, name, FEW, counts=counts_of(frames, s.n, FS), dither="none")


# ---- 8: host form and refusals ------------------------------------------------------------------------------------------------

def host_call(ctx, s, x, cs, fst, counts, dither, origin, want_arrays=True):
    fm = np.full(s.n, 0x5A5A5A5A, np.uint32)
    st = np.full(s.n, 0x5A5A5A5A, np.uint32).view(np.int32)
    sizes = s.sizes.astype(np.uint32)
    ns = None if counts is None else np.asarray(counts, np.uint32)
    org = None if origin is None else np.asarray(origin, np.uint64)
    ctx.lib.alac_hip_verify_float_host.restype = C.c_int32
    rc = ctx.lib.alac_hip_verify_float_host(
        ctx.h, s.cookie.ctypes.data, s.cookie.size, s.stream.ctypes.data, sizes.ctypes.data, s.n,
        x.ctypes.data, cs, fst, None if ns is None else ns.ctypes.data, None if dither is None else C.byref(dither),
        None if org is None else org.ctypes.data, fm.ctypes.data if want_arrays else None, st.ctypes.data if want_arrays else None)
    return rc, fm, st


@pytest.mark.parametrize("depth,channels", [(16, 2), (24, 2), (20, 6), (32, 1)])
def test_host_form_equals_device_form(gpu_ctx, depth, channels):
    fmt = alac_amd.make_format(FS, depth, channels, 44100)
    n = 5
    T = n * FS - 500
    counts = counts_of(T, n, FS)
    origin = [3, FS + 3, 2 ** 33, 9, 10 * FS]
    tpdf = depth != 32
    x = quiet(channels, T, depth)
    xt = torch.from_numpy(x).cuda()
    s = encode(gpu_ctx, fmt, xt, dither="tpdf" if tpdf else None, seed=6, origin=origin if tpdf else None)
    dz = alac_amd.capi.Dither(alac_amd.capi.DITHER_TPDF, 0, 6) if tpdf else None
    rc, fm, st = host_call(gpu_ctx, s, x, T, 1, counts, dz, origin if tpdf else None)
    assert rc == 0 and (fm == CLEAN).all() and (st == 0).all()
    assert host_call(gpu_ctx, s, x, T, 1, counts, dz, origin if tpdf else None, want_arrays=False)[0] == 0
    # the transposed source with two floats changed, and the wrong origin
    y = x.copy()
    y[channels - 1, 2 * FS + 77] += np.float32(0.01)
    y[0, 4 * FS + 5] -= np.float32(0.01)
    yt = np.ascontiguousarray(y.T)
    kw = dict(dither="tpdf", seed=6, origin=origin) if tpdf else {}
    dev_fm, dev_st, dev_bad = verify(gpu_ctx, s, torch.from_numpy(y).cuda(), counts=counts, **kw)
    rc, fm, st = host_call(gpu_ctx, s, yt, 1, channels, counts, dz, origin if tpdf else None)
    assert rc == dev_bad == 2 and np.array_equal(fm, dev_fm) and np.array_equal(st, dev_st)
    assert fm.tolist() == [CLEAN, CLEAN, 77, CLEAN, 5]
    if tpdf:
        rc, fm, st = host_call(gpu_ctx, s, x, T, 1, counts, dz, None)
        dev_fm, _, dev_bad = verify(gpu_ctx, s, xt, counts=counts, dither="tpdf", seed=6)
        assert rc == dev_bad and np.array_equal(fm, dev_fm) and fm[0] != CLEAN


def test_refusals_write_nothing(gpu_ctx):
    fmt = alac_amd.make_format(FS, 16, 2, 44100)
    n = 2
    x = quiet(2, n * FS, 1)
    xt = torch.from_numpy(x).cuda()
    s = encode(gpu_ctx, fmt, xt)
    fmt32 = alac_amd.make_format(FS, 32, 2, 44100)
    s32 = encode(gpu_ctx, fmt32, xt)
    lib = gpu_ctx.lib
    stream, offs = torch.from_numpy(s.stream).cuda(), torch.from_numpy(s.offsets).cuda()
    stream32, offs32 = torch.from_numpy(s32.stream).cuda(), torch.from_numpy(s32.offsets).cuda()
    wsb = int(lib.alac_hip_verify_workspace_bytes_stream(C.byref(fmt32), n, 0))
    ws = torch.zeros(wsb + 512, dtype=torch.uint8, device="cuda")
    base = ws.data_ptr() + (-ws.data_ptr() % 256)
    sentinel = 0x5A5A5A5A
    fm = torch.full((n,), sentinel, dtype=torch.int32, device="cuda")
    st = torch.full((n,), sentinel, dtype=torch.int32, device="cuda")
    bad = torch.full((1,), sentinel, dtype=torch.int32, device="cuda")
    origin = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    tpdf = alac_amd.capi.Dither(alac_amd.capi.DITHER_TPDF, 0, 1)

    def call(h=gpu_ctx.h, cookie=s.cookie, stream=stream.data_ptr(), offs=offs.data_ptr(), np_=n, x=xt.data_ptr(), cs=n * FS,
             fst=1, ns=None, dither=None, org=None, w=base, wb=wsb, fm_=fm.data_ptr(), st_=st.data_ptr(), bad_=bad.data_ptr()):
        return lib.alac_hip_verify_float(h, cookie.ctypes.data, cookie.size, stream, offs, np_, x, cs, fst, ns,
                                         None if dither is None else C.byref(dither), org, w, wb, fm_, st_, bad_)

    gpu_ctx.synchronize()
    refused = {
        "no context": dict(h=None),
        "bad cookie": dict(cookie=np.zeros(24, np.uint8)),
        "null stream": dict(stream=None), "null offsets": dict(offs=None), "null workspace": dict(w=None),
        "misaligned workspace": dict(w=base + 64), "workspace too small": dict(wb=1024),
        "null first_mismatch": dict(fm_=None), "null status": dict(st_=None), "null bad_packets": dict(bad_=None),
        "null d_in": dict(x=None), "misaligned d_in": dict(x=xt.data_ptr() + 2), "frame_stride 0": dict(fst=0),
        "channel_stride 0": dict(cs=0), "overflow": dict(cs=2 ** 63), "overflow frames": dict(fst=2 ** 62),
        "dither mode": dict(dither=alac_amd.capi.Dither(2, 0, 1)), "reserved": dict(dither=alac_amd.capi.Dither(1, 7, 1)),
        "reserved with mode none": dict(dither=alac_amd.capi.Dither(0, 1, 1)),
        "tpdf at 32 bits": dict(cookie=s32.cookie, stream=stream32.data_ptr(), offs=offs32.data_ptr(), dither=tpdf),
        "misaligned origin": dict(dither=tpdf, org=origin.data_ptr() + 4),
    }
    for what, kw in refused.items():
        assert call(**kw) == -50, what
        gpu_ctx.synchronize()
        for t in (fm, st, bad):
            assert (t == sentinel).all(), what
    # mode NONE ignores a misaligned origin table; and the call the refusals were variations of is accepted
    assert call(dither=alac_amd.capi.Dither(0, 0, 1), org=origin.data_ptr() + 4) == 0
    gpu_ctx.synchronize()
    assert fm.tolist() == [-1, -1] and st.tolist() == [0, 0] and bad.item() == 0
    # host form: the same checks
    dz_bad = alac_amd.capi.Dither(3, 0, 0)
    assert host_call(gpu_ctx, s, x, n * FS, 1, None, dz_bad, None)[0] == -50
    assert host_call(gpu_ctx, s, x, n * FS, 0, None, None, None)[0] == -50
    assert host_call(gpu_ctx, s, x, 0, 1, None, None, None)[0] == -50
    assert host_call(gpu_ctx, s32, x, n * FS, 1, None, tpdf, None)[0] == -50
    rc, hfm, hst = host_call(gpu_ctx, s, x, n * FS, 1, None, None, None)
    assert rc == 0 and (hfm == CLEAN).all() and (hst == 0).all()
