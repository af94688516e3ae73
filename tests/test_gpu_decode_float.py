"""GPU: alac_hip_decode_float (Context.decode_float) and its host form.  On every decoder path (tests/test_gpu_verify.py's
VARIANTS) the planar float32 output must equal, bit for bit, what the host makes of alac_hip_decode's bytes with numpy —
int16; the 3-byte container sign-extended, then >> 4 for 20 bits; the 3-byte container for 24 bits; int32 — scaled by
2^-(bit_depth - 1), at exactly the samples decode writes: a NaN sentinel written in front of the call must survive wherever
decode leaves a sample alone, the gap behind each channel's row included.  Frame counts and statuses equal decode's."""
import json
import os

import numpy as np
import pytest
import torch

import alac_amd
from test_gpu_verify import GOLD, VARIANTS, Case, encode_case, golden_wav, packed_case

pytestmark = pytest.mark.gpu
SENTINEL = np.uint32(0x7FC0DEAD)  # a quiet NaN no conversion produces
PAD = 37                          # floats of gap behind each channel's row


def offsets_of(c):
    return torch.from_numpy(np.concatenate([[0], np.cumsum(c.sizes)]).astype(np.int64)).cuda()


def to_float(raw, fmt):
    """decode's bytes -> float32 [channels, frames], the conversion a host caller writes"""
    d, ch = fmt.bit_depth, fmt.num_channels
    if d == 16:
        s = raw.view("<i2").astype(np.int32)
    elif d == 32:
        s = raw.view("<i4").astype(np.int32)
    else:
        b = raw.reshape(-1, 3).astype(np.int32)
        s = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        s = (s ^ 0x800000) - 0x800000
        if d == 20:
            s = s >> 4
    return (s.reshape(-1, ch).T.astype(np.float32) * np.float32(2.0 ** -(d - 1))).astype(np.float32)


def decode_reference(ctx, c, stream=None):
    """decode twice into buffers pre-filled with two different bytes: a sample decode wrote is equal in both.
    -> (float32 bits [channels, frames + PAD] with the sentinel where decode writes nothing, num_samples, status)"""
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
    frames = c.n * fmt.frame_size
    want = np.full((fmt.num_channels, frames + PAD), SENTINEL, np.uint32)
    want[:, :frames] = np.where(written, to_float(a, fmt).view(np.uint32), SENTINEL)
    return want, ns, st


def decode_float(ctx, c, stream=None, stride=None):
    """decode_float into a sentinel-filled [channels, stride] buffer -> (its bits, num_samples, status, pcm view)"""
    stream = c.stream if stream is None else stream
    fmt = c.fmt
    stride = c.n * fmt.frame_size + PAD if stride is None else stride
    buf = torch.from_numpy(np.full(fmt.num_channels * stride, SENTINEL, np.uint32).view(np.float32)).cuda()
    ns = torch.zeros(c.n, dtype=torch.int32, device="cuda")
    st = torch.zeros(c.n, dtype=torch.int32, device="cuda")
    pcm, ns, st, _ = ctx.decode_float(c.cookie, torch.from_numpy(stream).cuda(), offsets_of(c), c.n, out=(buf, ns, st),
                                      channel_stride=stride)
    ctx.synchronize()
    assert pcm.shape == (fmt.num_channels, c.n * fmt.frame_size) and pcm.stride() == (stride, 1)
    return buf.cpu().numpy().view(np.uint32).reshape(fmt.num_channels, stride), ns.cpu().numpy(), st.cpu().numpy(), pcm


def assert_float_equals_decode(ctx, c, what, stream=None, variants=VARIANTS):
    for v in variants:
        with ctx.options(**v):
            want, wns, wst = decode_reference(ctx, c, stream)
            got, ns, st, _ = decode_float(ctx, c, stream)
        assert np.array_equal(ns, wns) and np.array_equal(st, wst), (what, v)
        bad = np.argwhere(got != want)
        assert bad.size == 0, (what, v, bad[:4].tolist(), got[tuple(bad[0])] if bad.size else None)


# ---- streams of this library ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("depth", [16, 20, 24, 32])
@pytest.mark.parametrize("channels", [1, 2])
def test_mono_stereo_depths(gpu_ctx, depth, channels):
    c = encode_case(gpu_ctx, depth, channels, 3 * 4096 + 777, seed=depth + channels)  # a short last packet
    assert_float_equals_decode(gpu_ctx, c, (depth, channels))


@pytest.mark.parametrize("depth,channels", [(16, 3), (24, 6), (20, 6), (32, 8), (16, 8)])
def test_multichannel(gpu_ctx, depth, channels):
    c = encode_case(gpu_ctx, depth, channels, 2 * 4096 + 555, seed=depth * channels)
    assert_float_equals_decode(gpu_ctx, c, (depth, channels))


@pytest.mark.parametrize("depth,channels", [(16, 2), (24, 2), (24, 1)])
def test_odd_frame_size(gpu_ctx, depth, channels):
    c = encode_case(gpu_ctx, depth, channels, 7 * 333 + 100, seed=7, frame_size=333)
    assert_float_equals_decode(gpu_ctx, c, ("frame 333", depth, channels))


@pytest.mark.parametrize("kind", ["noise16", "noise24", "noise20_mono"])
def test_escaped_packets(gpu_ctx, kind):
    depth, channels = {"noise16": (16, 2), "noise24": (24, 2), "noise20_mono": (20, 1)}[kind]
    frames = 3 * 4096 + 100
    pcm = np.random.default_rng(9).integers(0, 256, frames * channels * alac_amd.capi.BPS[depth], dtype=np.uint8)
    if depth == 20:
        pcm[0::3] &= 0xF0
    c = encode_case(gpu_ctx, depth, channels, frames, pcm=pcm)
    assert_float_equals_decode(gpu_ctx, c, kind)


@pytest.mark.parametrize("kind", ["lpc", "fast_mode", "segments"])
def test_encode_modes(gpu_ctx, kind):
    frames = 9 * 4096 + 1234
    if kind == "lpc":
        c = encode_case(gpu_ctx, 16, 2, frames, seed=4, lpc=1)
    elif kind == "fast_mode":
        c = encode_case(gpu_ctx, 16, 2, frames, seed=5, fast_mode=1)
    else:
        c = encode_case(gpu_ctx, 24, 2, frames, seed=6, segment_packets=4)
    assert_float_equals_decode(gpu_ctx, c, kind)


def test_lpc_24bit(gpu_ctx):
    c = encode_case(gpu_ctx, 24, 2, 5 * 4096 + 3, seed=14, lpc=1)
    assert_float_equals_decode(gpu_ctx, c, "lpc 24")


@pytest.mark.parametrize("name", ["50.wav", "05.wav"])
def test_chained_reference_audio(gpu_ctx, name):
    ka, pcm = golden_wav(name)
    fmt = alac_amd.make_format(4096, ka["bits"], ka["channels"], ka["rate"])
    frames = pcm.size // fmt.bytes_per_frame
    stream, sizes, _ = gpu_ctx.encode_host(fmt, pcm, frames, segment_packets=0)
    c = packed_case(gpu_ctx, gpu_ctx.magic_cookie(fmt), fmt, stream, sizes, pcm, frames)
    assert_float_equals_decode(gpu_ctx, c, name)


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
        assert gpu_ctx.lib.alac_hip_format_from_cookie(np.ascontiguousarray(cookie).ctypes.data, cookie.size,
                                                       alac_amd.capi.C.byref(fmt)) == 0
        ends = np.cumsum(sizes)
        packets = [stream[e - s:e] for s, e in zip(sizes, ends)]
        c = Case(cookie, packets, fmt, np.zeros(0, np.uint8), np.zeros(len(packets), np.int32))
        assert_float_equals_decode(gpu_ctx, c, m)


# ---- damaged packets ------------------------------------------------------------------------------------------------------

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
    assert_float_equals_decode(gpu_ctx, c, (depth, channels), stream=s)


# ---- values at the edges --------------------------------------------------------------------------------------------------

def packed(x, depth):
    """int32 samples [frames, channels] -> the bytes decode writes"""
    x = np.ascontiguousarray(x, np.int64)
    if depth == 16:
        return x.astype("<i2").view(np.uint8).ravel()
    if depth == 32:
        return x.astype("<i4").view(np.uint8).ravel()
    v = (x << 4 if depth == 20 else x).ravel() & 0xFFFFFF
    return np.stack([v & 0xFF, (v >> 8) & 0xFF, v >> 16], axis=1).astype(np.uint8).ravel()


@pytest.mark.parametrize("depth", [16, 20, 24, 32])
def test_full_scale_values(gpu_ctx, depth):
    frames = 2 * 4096 + 9
    lo, hi = -(1 << (depth - 1)), (1 << (depth - 1)) - 1
    x = np.empty((frames, 2), np.int64)
    x[:, 0] = np.where(np.arange(frames) % 3 == 0, lo, hi)
    x[:, 1] = np.where(np.arange(frames) % 2 == 0, hi, lo)
    c = encode_case(gpu_ctx, depth, 2, frames, pcm=packed(x, depth))
    for v in VARIANTS:
        with gpu_ctx.options(**v):
            got, ns, st, _ = decode_float(gpu_ctx, c)
        f = got[:, :frames].view(np.float32).T
        assert (st == 0).all() and ns.sum() == frames, v
        assert (f[x == lo] == -1.0).all(), v
        top = np.float32(hi) * np.float32(2.0 ** -(depth - 1))
        assert (f[x == hi] == top).all(), v
        if depth == 32:
            assert (f[x == hi] == 1.0).all(), v  # 2^31 - 1 rounds to 2^31
        else:
            assert (f[x == hi] < 1.0).all(), v


# ---- the Python surface, the host form, bad parameters ---------------------------------------------------------------------

def test_default_call_returns_a_compact_zero_filled_tensor(gpu_ctx):
    c = encode_case(gpu_ctx, 24, 2, 3 * 4096 + 5, seed=12)
    pcm, ns, st, fmt = gpu_ctx.decode_float(c.cookie, torch.from_numpy(c.stream).cuda(), offsets_of(c), c.n)
    gpu_ctx.synchronize()
    assert pcm.dtype == torch.float32 and pcm.is_cuda and pcm.is_contiguous()
    assert tuple(pcm.shape) == (2, c.n * 4096)
    want, _, _ = decode_reference(gpu_ctx, c)
    want = want[:, :c.n * 4096]
    want[want == SENTINEL] = 0  # zero_fill: what decode leaves alone is 0.0
    assert np.array_equal(pcm.cpu().numpy().view(np.uint32), want)
    # the samples themselves, against the source
    src = to_float(c.expected, fmt)
    assert np.array_equal(pcm.cpu().numpy(), src)


def test_host_form_equals_device_form(gpu_ctx):
    c = encode_case(gpu_ctx, 20, 2, 4 * 4096 + 99, seed=13)
    frames = c.n * 4096
    stride = frames + PAD
    dev, _, _, _ = gpu_ctx.decode_float(c.cookie, torch.from_numpy(c.stream).cuda(), offsets_of(c), c.n)
    gpu_ctx.synchronize()
    out = np.full(2 * stride, SENTINEL, np.uint32)
    ns = np.zeros(c.n, np.uint32)
    st = np.full(c.n, 7, np.int32)
    sizes = c.sizes.astype(np.uint32)
    rc = gpu_ctx.lib.alac_hip_decode_float_host(gpu_ctx.h, c.cookie.ctypes.data, c.cookie.size, c.stream.ctypes.data,
                                                sizes.ctypes.data, c.n, out.ctypes.data, stride, ns.ctypes.data,
                                                st.ctypes.data)
    assert rc == 0
    out = out.reshape(2, stride)
    assert np.array_equal(out[:, :frames], dev.cpu().numpy().view(np.uint32))
    assert (out[:, frames:] == SENTINEL).all()
    assert (st == 0).all() and ns.tolist() == c.counts.tolist()


def test_bad_parameters_write_nothing(gpu_ctx):
    c = encode_case(gpu_ctx, 16, 2, 2 * 4096, seed=15)
    lib, fmt = gpu_ctx.lib, c.fmt
    frames = c.n * fmt.frame_size
    d_stream, offs = torch.from_numpy(c.stream).cuda(), offsets_of(c)
    wsb = int(lib.alac_hip_decode_workspace_bytes_stream(alac_amd.capi.C.byref(fmt), c.n, int(d_stream.numel())))
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    buf = torch.from_numpy(np.full(2 * frames + 8, SENTINEL, np.uint32).view(np.float32)).cuda()
    ns = torch.full((c.n,), 77, dtype=torch.int32, device="cuda")
    st = torch.full((c.n,), 77, dtype=torch.int32, device="cuda")

    def call(ptr, stride, wsbytes=wsb):
        rc = lib.alac_hip_decode_float(gpu_ctx.h, c.cookie.ctypes.data, c.cookie.size, d_stream.data_ptr(), offs.data_ptr(),
                                       c.n, ws.data_ptr(), wsbytes, ptr, stride, ns.data_ptr(), st.data_ptr())
        gpu_ctx.synchronize()
        return rc

    assert call(buf.data_ptr(), frames - 1) == -50          # channel_stride too small
    assert call(buf.data_ptr() + 2, frames) == -50          # d_out not 4-byte aligned
    assert call(None, frames) == -50                        # no d_out
    assert call(buf.data_ptr(), 1 << 62) == -50             # channel_stride * channels * 4 overflows
    assert call(buf.data_ptr(), frames, wsb - 1) == -50     # workspace below alac_hip_decode_workspace_bytes_stream
    assert (buf.cpu().numpy().view(np.uint32) == SENTINEL).all()
    assert (ns.cpu().numpy() == 77).all() and (st.cpu().numpy() == 77).all()
    # exactly the decode workspace suffices
    assert call(buf.data_ptr(), frames) == 0
    assert (st.cpu().numpy() == 0).all()
    with pytest.raises(ValueError):
        gpu_ctx.decode_float(c.cookie, d_stream, offs, c.n, out=(buf[:frames], ns, st))
