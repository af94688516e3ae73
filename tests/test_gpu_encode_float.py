"""GPU: alac_hip_encode_float (Context.encode_float) and its host form.  The stream, sizes, offsets and final state must equal,
byte for byte, what Context.encode gives for the PCM a numpy restatement of the quantization rule of include/alac_hip.h
makes (float64 product, np.rint, clip, NaN -> 0, << 4 into 3 bytes at 20 bits), over every layout the strides allow, short
packets, segment tables, state chains and the encode options.  Clip counts equal numpy's, floats the call must not read
(the gap between rows, the frames behind a short packet) are 2.0 and would clip if read, decode_float(encode_float(x)) == x
on the grid, and every refusal returns -50 with nothing written."""
import ctypes as C
import lzma
import os

import numpy as np
import pytest
import torch

import alac_amd

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
FS = 4096
FAR = 2.0  # a float the call must never read: it would clip


def quantize(x, depth):
    """the rule of include/alac_hip.h in numpy -> (int64 samples, clipped mask)"""
    top = 2 ** (depth - 1)
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.rint(x.astype(np.float64) * float(top))
        nan = np.isnan(x)
        hi, lo = r > top - 1, r < -top
        s = np.where(nan, 0, np.clip(np.nan_to_num(r, nan=0.0, posinf=top, neginf=-top - 1), -top, top - 1))
    return s.astype(np.int64), nan | hi | lo


def pack(s, depth, num_packets):
    """int samples [C, frames] -> packed little-endian interleaved PCM of num_packets whole packets (zeros behind)"""
    ch, frames = s.shape
    full = np.zeros((num_packets * FS, ch), np.int64)
    full[:frames] = s.T
    v = full.reshape(-1)
    if depth == 16:
        return v.astype("<i2").view(np.uint8).copy()
    if depth == 32:
        return v.astype("<i4").view(np.uint8).copy()
    c = (v << 4 if depth == 20 else v) & 0xFFFFFF
    out = np.empty((v.size, 3), np.uint8)
    out[:, 0], out[:, 1], out[:, 2] = c & 0xFF, (c >> 8) & 0xFF, (c >> 16) & 0xFF
    return out.reshape(-1)


def music(channels, frames, seed):
    """float32 [channels, frames] from the reference-audio fixture, scaled past full scale here and there"""
    with open(os.path.join(GOLD, "wav05_pcm.xz"), "rb") as f:
        pcm = np.frombuffer(lzma.decompress(f.read()), "<i2").astype(np.float64)
    rng = np.random.default_rng(seed)
    out = np.empty((channels, frames), np.float64)
    for c in range(channels):
        start = int(rng.integers(0, pcm.size - frames))
        out[c] = pcm[start:start + frames] / 32768.0 * 1.2 + rng.normal(0, 1e-4, frames)
    return out.astype(np.float32)


def specials(depth):
    """every edge of the rule: infinities, NaN, +-1, -0, denormals, far values and the ties (k + 0.5) / 2^(b-1)"""
    top = 2.0 ** (depth - 1)
    v = [np.inf, -np.inf, np.nan, 1.0, -1.0, -0.0, 0.0, 1e-40, -1e-40, 1e-45, -1e-45, 1.5, -1.5, 3e38, -3e38, 1.0000001,
         -1.0000001, 0.99999994, -0.99999994]
    ties = [(k + 0.5) / top for k in range(-9, 9)]
    if depth <= 24:
        ties += [(top - k - 0.5) / top for k in range(6)] + [-(top - k - 0.5) / top for k in range(6)]
        ties += [(top - k - 1.5) / top for k in range(3)]
    assert np.array_equal(np.array(ties, np.float32).astype(np.float64), np.array(ties)), "a tie is not a float32"
    out = np.array(v + ties, np.float32)
    return out


def make_x(depth, channels, frames, seed):
    x = music(channels, frames, seed)
    sp = specials(depth)
    rng = np.random.default_rng(seed + 100)
    for c in range(channels):
        pos = rng.choice(frames, sp.size, replace=False)
        x[c, pos] = rng.permutation(sp)
    return x


def reference(ctx, fmt, x, num_samples=None, **kw):
    """Context.encode of the numpy-quantized PCM -> (stream, sizes, offsets, bufs)"""
    ch, frames = x.shape
    n = (frames + FS - 1) // FS
    s, _ = quantize(x, fmt.bit_depth)
    if num_samples is not None:  # frames behind a packet's count are not read: they stage as zero
        for p, k in enumerate(num_samples.cpu().numpy()):
            s[:, p * FS + k:(p + 1) * FS] = 0
    elif frames % FS:
        num_samples = torch.tensor([FS] * (n - 1) + [frames % FS], dtype=torch.int32, device="cuda")
    pcm = torch.from_numpy(pack(s, fmt.bit_depth, n)).cuda()
    b = ctx.encode(fmt, pcm, n, num_samples=num_samples, **kw)
    return fetch(ctx, b)


def fetch(ctx, b):
    ctx.synchronize()
    total = int(b["offsets"][-1].item())
    return b["out"][:total].cpu().numpy(), b["sizes"].cpu().numpy(), b["offsets"].cpu().numpy(), b


def assert_same(got, want, what):
    assert np.array_equal(got[1], want[1]), (what, "sizes")
    assert np.array_equal(got[2], want[2]), (what, "offsets")
    assert np.array_equal(got[0], want[0]), (what, "stream")


@pytest.mark.parametrize("channels", [1, 2, 6])
@pytest.mark.parametrize("depth", [16, 20, 24, 32])
def test_bytes_equal_encode_of_numpy_quantized(gpu_ctx, depth, channels):
    fmt = alac_amd.make_format(FS, depth, channels, 44100)
    x = make_x(depth, channels, 3 * FS + 1000, depth * 10 + channels)
    got = fetch(gpu_ctx, gpu_ctx.encode_float(fmt, torch.from_numpy(x).cuda()))
    assert_same(got, reference(gpu_ctx, fmt, x), (depth, channels))


@pytest.mark.parametrize("depth,channels", [(16, 2), (24, 2), (16, 1), (20, 6)])
def test_layouts_give_identical_bytes(gpu_ctx, depth, channels):
    fmt = alac_amd.make_format(FS, depth, channels, 44100)
    frames = 2 * FS + 1236
    x = make_x(depth, channels, frames, 7 + depth)
    want = fetch(gpu_ctx, gpu_ctx.encode_float(fmt, torch.from_numpy(x).cuda()))
    assert_same(want, reference(gpu_ctx, fmt, x), "contiguous")
    views = {}
    for gap in (64, 37):  # a 16-byte multiple (vector loads) and not
        buf = torch.full((channels, frames + gap), FAR, device="cuda")
        buf[:, :frames] = torch.from_numpy(x).cuda()
        views[f"gap{gap}"] = buf[:, :frames]
    views["transposed"] = torch.from_numpy(np.ascontiguousarray(x.T)).cuda().t()
    wide = torch.full((channels, 2 * frames), FAR, device="cuda")
    wide[:, 0::2] = torch.from_numpy(x).cuda()
    views["every_other_frame"] = wide[:, 0::2]
    for name, v in views.items():
        assert tuple(v.shape) == (channels, frames)
        got = fetch(gpu_ctx, gpu_ctx.encode_float(fmt, v, clipped=True))
        assert_same(got, want, name)


@pytest.mark.parametrize("depth", [16, 24])
def test_short_packets_segments_and_state(gpu_ctx, depth):
    fmt = alac_amd.make_format(FS, depth, 2, 44100)
    n = 7
    counts = [FS, 1000, FS, 17, FS, FS, 2049]
    x = make_x(depth, 2, n * FS, 31 + depth)
    for p, k in enumerate(counts):
        x[:, p * FS + k:(p + 1) * FS] = FAR
    xt = torch.from_numpy(x).cuda()
    ns = torch.tensor(counts, dtype=torch.int32, device="cuda")
    seg = torch.tensor([0, 2, 5, n], dtype=torch.int32, device="cuda")
    for bound in (3, 0):
        st_ref = torch.zeros(3 * 64, dtype=torch.int16, device="cuda")
        st_got = torch.zeros(3 * 64, dtype=torch.int16, device="cuda")
        kw = dict(num_samples=ns, seg_first=seg, max_segment_packets=bound)
        want = reference(gpu_ctx, fmt, x, state=st_ref, **kw)
        got = fetch(gpu_ctx, gpu_ctx.encode_float(fmt, xt, state=st_got, **kw))
        assert_same(got, want, ("chained", bound))
        assert torch.equal(st_got, st_ref)
        # and on from that state
        want = reference(gpu_ctx, fmt, x, state=st_ref, state_in=True, **kw)
        got = fetch(gpu_ctx, gpu_ctx.encode_float(fmt, xt, state=st_got, state_in=True, **kw))
        assert_same(got, want, ("state in", bound))
        assert torch.equal(st_got, st_ref)
    # T not a multiple of frame_size, no explicit counts
    x2 = make_x(depth, 2, 4 * FS + 3, 5)
    got = fetch(gpu_ctx, gpu_ctx.encode_float(fmt, torch.from_numpy(x2).cuda()))
    assert_same(got, reference(gpu_ctx, fmt, x2), "T % frame_size")


@pytest.mark.parametrize("opts", [{"lpc": 1}, {"fast_mode": 1}, {"thru": 1}, {"encoder_lane": 1}, {"fused": 0}],
                         ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
@pytest.mark.parametrize("depth", [16, 24])
def test_options_bytes_equal_encode(gpu_ctx, depth, opts):
    fmt = alac_amd.make_format(FS, depth, 2, 44100)
    x = make_x(depth, 2, 5 * FS + 555, 11 + depth)
    with gpu_ctx.options(**opts):
        want = reference(gpu_ctx, fmt, x)
        got = fetch(gpu_ctx, gpu_ctx.encode_float(fmt, torch.from_numpy(x).cuda()))
    assert_same(got, want, opts)


@pytest.mark.parametrize("depth,channels", [(16, 2), (24, 2), (32, 1), (20, 3)])
def test_clip_counts_see_only_the_frames_read(gpu_ctx, depth, channels):
    fmt = alac_amd.make_format(FS, depth, channels, 44100)
    n = 5
    counts = np.array([FS, 999, FS, 4, FS], np.int32)
    frames = n * FS
    x = make_x(depth, channels, frames, 3 + depth)
    gap = 40
    buf = np.full((channels, frames + gap), FAR, np.float32)
    buf[:, :frames] = x
    for p, k in enumerate(counts):
        buf[:, p * FS + k:(p + 1) * FS] = FAR
    view = torch.from_numpy(buf).cuda()[:, :frames]
    b = gpu_ctx.encode_float(fmt, view, num_samples=torch.from_numpy(counts).cuda(), clipped=True)
    gpu_ctx.synchronize()
    _, clip = quantize(x, depth)
    want = [int(clip[:, p * FS:p * FS + k].sum()) for p, k in enumerate(counts)]
    assert b["clipped"].cpu().tolist() == want
    assert sum(want) > 0


@pytest.mark.parametrize("depth", [16, 20, 24, 32])
def test_round_trip_on_grid(gpu_ctx, depth):
    fmt = alac_amd.make_format(FS, depth, 2, 44100)
    rng = np.random.default_rng(depth)
    frames = 3 * FS + 100
    top = 2 ** (depth - 1)
    s = rng.integers(-top, top, (2, frames), dtype=np.int64)
    if depth == 32:
        s = (s >> 8) << 8  # x * 2^31 integral in float32
        s[:, :4] = [[-top, top - 128, 1, -1]] * 2
    x = (s.astype(np.float64) / top).astype(np.float32)
    assert np.array_equal(x.astype(np.float64) * top, s)
    b = gpu_ctx.encode_float(fmt, torch.from_numpy(x).cuda(), clipped=True)
    n = (frames + FS - 1) // FS
    pcm, ns, st, _ = gpu_ctx.decode_float(gpu_ctx.magic_cookie(fmt), b["out"], b["offsets"], n)
    gpu_ctx.synchronize()
    assert st.abs().sum().item() == 0 and int(b["clipped"].sum().item()) == 0
    assert np.array_equal(pcm[:, :frames].cpu().numpy().view(np.uint32), x.view(np.uint32))


def host_call(ctx, fmt, x, cs, fst, counts, seg, clipped=True):
    lib = ctx.lib
    n = len(counts)
    cap = int(lib.alac_hip_encode_max_output_bytes(C.byref(fmt), n))
    out = np.zeros(cap, np.uint8)
    sizes = np.zeros(n, np.uint32)
    clip = np.zeros(n, np.uint32)
    state = np.zeros((len(seg) - 1) * int(lib.alac_hip_state_int16(C.byref(fmt))), np.int16)
    total = C.c_uint64(0)
    ns = np.ascontiguousarray(counts, np.uint32)
    sg = np.ascontiguousarray(seg, np.uint32)
    rc = lib.alac_hip_encode_float_host(ctx.h, C.byref(fmt), x.ctypes.data, cs, fst, ns.ctypes.data, n, sg.ctypes.data,
                                        len(seg) - 1, state.ctypes.data, 0, out.ctypes.data, cap, sizes.ctypes.data,
                                        C.byref(total), clip.ctypes.data if clipped else None)
    assert rc == 0, lib.alac_hip_last_error(ctx.h)
    return out[:total.value], sizes, clip, state


@pytest.mark.parametrize("depth,channels", [(16, 2), (24, 1), (20, 6)])
def test_host_form_equals_device_form(gpu_ctx, depth, channels):
    fmt = alac_amd.make_format(FS, depth, channels, 44100)
    frames = 4 * FS + 321
    x = make_x(depth, channels, frames, 17)
    n = (frames + FS - 1) // FS
    counts = [FS] * (n - 1) + [frames % FS]
    seg = [0, 2, n]
    st = torch.zeros(2 * int(gpu_ctx.lib.alac_hip_state_int16(C.byref(fmt))), dtype=torch.int16, device="cuda")
    b = gpu_ctx.encode_float(fmt, torch.from_numpy(x).cuda(), seg_first=torch.tensor(seg, dtype=torch.int32, device="cuda"),
                             state=st, clipped=True)
    dev = fetch(gpu_ctx, b)
    want_state = st.cpu().numpy()
    want_clip = b["clipped"].cpu().numpy()
    for name, arr, cs, fst in (("planar", x, frames, 1), ("interleaved", np.ascontiguousarray(x.T), 1, channels)):
        stream, sizes, clip, state = host_call(gpu_ctx, fmt, arr, cs, fst, counts, seg)
        assert np.array_equal(sizes, dev[1]) and np.array_equal(stream, dev[0]), name
        assert np.array_equal(clip, want_clip), name
        assert np.array_equal(state, want_state), name


def test_refusals_write_nothing(gpu_ctx):
    ctx, lib = gpu_ctx, gpu_ctx.lib
    fmt = alac_amd.make_format(FS, 16, 2, 44100)
    n = 4
    x = torch.from_numpy(make_x(16, 2, n * FS, 2)).cuda()
    cap = int(lib.alac_hip_encode_max_output_bytes(C.byref(fmt), n))
    out = torch.full((cap,), 0xAB, dtype=torch.uint8, device="cuda")
    sizes = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    offs = torch.full((n + 1,), 9, dtype=torch.int64, device="cuda")
    clip = torch.full((n,), 5, dtype=torch.int32, device="cuda")
    wsb = int(lib.alac_hip_encode_float_workspace_bytes(C.byref(fmt), n, n))
    stage = wsb - int(lib.alac_hip_encode_workspace_bytes(C.byref(fmt), n, n))
    assert stage >= n * fmt.packet_bytes
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    bad_seg = torch.tensor([0, 3, 1, n], dtype=torch.int32, device="cuda")

    def call(ptr=x.data_ptr(), cs=n * FS, fst=1, f=fmt, seg=None, nseg=n, ws_bytes=wsb, capacity=cap):
        return lib.alac_hip_encode_float(ctx.h, C.byref(f), ptr, cs, fst, None, n,
                                         None if seg is None else seg.data_ptr(), nseg, 0, None, 0, ws.data_ptr(),
                                         ws_bytes, out.data_ptr(), capacity, sizes.data_ptr(), offs.data_ptr(),
                                         clip.data_ptr())

    cases = {
        "null d_in": dict(ptr=None),
        "misaligned d_in": dict(ptr=x.data_ptr() + 2),
        "frame_stride 0": dict(fst=0),
        "channel_stride 0": dict(cs=0),
        "index overflow": dict(cs=1 << 62),
        "workspace too small": dict(ws_bytes=stage + 4096),
        "workspace below the stage": dict(ws_bytes=1024),
        "output capacity": dict(capacity=cap - 1),
        "bad format": dict(f=alac_amd.make_format(FS, 18, 2, 44100)),
        "bad segment table": dict(seg=bad_seg, nseg=3),
        "segment count": dict(seg=bad_seg, nseg=n + 1),
    }
    for what, kw in cases.items():
        assert call(**kw) == -50, what
    with ctx.options(lpc=1, fast_mode=1):
        assert call() == -50, "lpc + fast_mode"
    ctx.synchronize()
    assert (out == 0xAB).all() and (sizes == 7).all() and (offs == 9).all() and (clip == 5).all()
    # the context is still usable
    assert call() == 0
    ctx.synchronize()
    want = reference(ctx, fmt, x.cpu().numpy())
    total = int(offs[-1].item())
    assert np.array_equal(out[:total].cpu().numpy(), want[0])
    assert clip.cpu().tolist() == [int(v) for v in quantize(x.cpu().numpy(), 16)[1].reshape(2, n, FS).sum(axis=(0, 2))]
