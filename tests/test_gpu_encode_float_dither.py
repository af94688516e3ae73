"""GPU: alac_hip_encode_float_dither (Context.encode_float(dither="tpdf")) and its host form.  The stream, sizes, offsets, final
state and clip counts must equal, byte for byte, what Context.encode gives for the PCM that tests/dither_ref.py (the numpy
restatement of the rule of include/alac_hip.h, pinned by tests/test_dither_rule.py) makes: over the bit depths, channel
counts and layouts, short packets, explicit packet origins (even, odd, above 2^32), segment tables and encode options.  The
quantized PCM does not depend on frame_size or on what else is in the batch; it does depend on the seed and the channel
index; without dither the new entry point is alac_hip_encode_float; floats the call must not read are 2.0 and would clip
if read; every refusal returns -50 with nothing written."""
import ctypes as C

import numpy as np
import pytest
import torch

import alac_amd
import dither_ref as dr
from test_gpu_encode_float import FAR, FS, assert_same, fetch, make_x, pack

pytestmark = pytest.mark.gpu


def restated(x, depth, seed, counts=None, origin=None, channels=None):
    """the samples and the per-packet clip counts of the rule for a call over x [C, frames] in packets of FS frames"""
    ch, frames = x.shape
    n = (frames + FS - 1) // FS
    if counts is None:
        counts = [FS] * (n - 1) + [frames - (n - 1) * FS]
    t = dr.packet_frames(n, FS, origin)[:frames]
    s, clip = dr.quantize_dithered(x, depth, seed, origin=t, channels=channels)
    clips = []
    for p, k in enumerate(counts):  # frames behind a packet's count are not read: they stage as zero, undithered
        s[:, p * FS + k:(p + 1) * FS] = 0
        clips.append(int(clip[:, p * FS:p * FS + k].sum()))
    return s, clips, n


def reference(ctx, fmt, x, seed, counts=None, origin=None, **kw):
    """Context.encode of the restatement's PCM -> (stream, sizes, offsets, bufs), and the clip counts"""
    s, clips, n = restated(x, fmt.bit_depth, seed, counts, origin)
    frames = x.shape[1]
    ns = None
    if counts is not None or frames % FS:
        ns = torch.tensor(counts or [FS] * (n - 1) + [frames % FS], dtype=torch.int32, device="cuda")
    pcm = torch.from_numpy(pack(s, fmt.bit_depth, n)).cuda()
    return fetch(ctx, ctx.encode(fmt, pcm, n, num_samples=ns, **kw)), clips


def origin_tensor(origin):
    return torch.from_numpy(np.asarray(origin, np.uint64).view(np.int64).copy()).cuda()


@pytest.mark.parametrize("channels", [1, 2, 6])
@pytest.mark.parametrize("depth", [16, 20, 24])
def test_bytes_equal_encode_of_restated_pcm(gpu_ctx, depth, channels):
    fmt = alac_amd.make_format(FS, depth, channels, 44100)
    seed = 0x0123456789ABCDEF + depth * 8 + channels
    x = make_x(depth, channels, 3 * FS + 1000, depth * 10 + channels)  # music past full scale and every special value
    b = gpu_ctx.encode_float(fmt, torch.from_numpy(x).cuda(), dither="tpdf", seed=seed, clipped=True)
    got = fetch(gpu_ctx, b)
    want, clips = reference(gpu_ctx, fmt, x, seed)
    assert_same(got, want, (depth, channels))
    assert b["clipped"].cpu().tolist() == clips and sum(clips) > 0


@pytest.mark.parametrize("depth,channels", [(16, 2), (24, 2), (16, 1), (20, 6)])
def test_layouts_give_identical_bytes(gpu_ctx, depth, channels):
    fmt = alac_amd.make_format(FS, depth, channels, 44100)
    frames = 2 * FS + 1236
    x = make_x(depth, channels, frames, 7 + depth)
    want, clips = reference(gpu_ctx, fmt, x, 5)
    xt = torch.from_numpy(x).cuda()
    views = {"contiguous": xt}
    for gap in (64, 37):  # a 16-byte multiple (vector loads) and not
        buf = torch.full((channels, frames + gap), FAR, device="cuda")
        buf[:, :frames] = xt
        views[f"gap{gap}"] = buf[:, :frames]
    odd = torch.full((channels, frames + 8), FAR, device="cuda")  # rows that start 4 bytes off a 16-byte boundary
    odd[:, 1:frames + 1] = xt
    views["odd_offset"] = odd[:, 1:frames + 1]
    views["transposed"] = torch.from_numpy(np.ascontiguousarray(x.T)).cuda().t()
    wide = torch.full((channels, 2 * frames), FAR, device="cuda")
    wide[:, 0::2] = xt
    views["every_other_frame"] = wide[:, 0::2]
    for name, v in views.items():
        assert tuple(v.shape) == (channels, frames)
        b = gpu_ctx.encode_float(fmt, v, dither="tpdf", seed=5, clipped=True)
        assert_same(fetch(gpu_ctx, b), want, name)
        assert b["clipped"].cpu().tolist() == clips, name


@pytest.mark.parametrize("depth,channels", [(16, 2), (24, 2), (20, 1)])
def test_short_packets_origins_segments_and_state(gpu_ctx, depth, channels):
    fmt = alac_amd.make_format(FS, depth, channels, 44100)
    n = 7
    counts = [FS, 1000, FS, 17, FS, FS, 2049]
    origin = [0, FS + 1, 2 ** 32 + 6, 2 ** 33 + 7, 12345, 2 ** 40, 3]  # even, odd and above 2^32
    x = make_x(depth, channels, n * FS, 31 + depth)
    for p, k in enumerate(counts):
        x[:, p * FS + k:(p + 1) * FS] = FAR
    xt = torch.from_numpy(x).cuda()
    ns = torch.tensor(counts, dtype=torch.int32, device="cuda")
    seg = torch.tensor([0, 2, 5, n], dtype=torch.int32, device="cuda")
    n16 = int(gpu_ctx.lib.alac_hip_state_int16(C.byref(fmt)))
    for org in (origin, None):
        ot = None if org is None else origin_tensor(org)
        for bound in (3, 0):
            st_ref = torch.zeros(3 * n16, dtype=torch.int16, device="cuda")
            st_got = torch.zeros(3 * n16, dtype=torch.int16, device="cuda")
            kw = dict(seg_first=seg, max_segment_packets=bound)
            want, clips = reference(gpu_ctx, fmt, x, 77, counts, org, state=st_ref, **kw)
            b = gpu_ctx.encode_float(fmt, xt, num_samples=ns, state=st_got, dither="tpdf", seed=77, packet_origin=ot,
                                     clipped=True, **kw)
            assert_same(fetch(gpu_ctx, b), want, ("chained", bound, org is None))
            assert torch.equal(st_got, st_ref)
            assert b["clipped"].cpu().tolist() == clips  # the 2.0 behind every short packet was not read
            want, _ = reference(gpu_ctx, fmt, x, 77, counts, org, state=st_ref, state_in=True, **kw)
            b = gpu_ctx.encode_float(fmt, xt, num_samples=ns, state=st_got, state_in=True, dither="tpdf", seed=77,
                                     packet_origin=ot, **kw)
            assert_same(fetch(gpu_ctx, b), want, ("state in", bound, org is None))
            assert torch.equal(st_got, st_ref)
    # T not a multiple of frame_size, no explicit counts
    x2 = make_x(depth, channels, 4 * FS + 3, 5)
    got = fetch(gpu_ctx, gpu_ctx.encode_float(fmt, torch.from_numpy(x2).cuda(), dither="tpdf", seed=1))
    assert_same(got, reference(gpu_ctx, fmt, x2, 1)[0], "T % frame_size")


@pytest.mark.parametrize("opts", [{"lpc": 1}, {"fast_mode": 1}], ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
@pytest.mark.parametrize("depth", [16, 24])
def test_options_bytes_equal_encode(gpu_ctx, depth, opts):
    fmt = alac_amd.make_format(FS, depth, 2, 44100)
    x = make_x(depth, 2, 5 * FS + 555, 11 + depth)
    with gpu_ctx.options(**opts):
        want, _ = reference(gpu_ctx, fmt, x, 3)
        got = fetch(gpu_ctx, gpu_ctx.encode_float(fmt, torch.from_numpy(x).cuda(), dither="tpdf", seed=3))
    assert_same(got, want, opts)


def decoded(ctx, fmt, b, n):
    pcm, ns, st, _ = ctx.decode(ctx.magic_cookie(fmt), b["out"], b["offsets"], n)
    ctx.synchronize()
    assert st.abs().sum().item() == 0
    return pcm.cpu().numpy()


@pytest.mark.parametrize("depth", [16, 24])
def test_pcm_does_not_depend_on_frame_size(gpu_ctx, depth):
    frames = 2 * FS
    x = make_x(depth, 2, frames, 40 + depth)
    xt = torch.from_numpy(x).cuda()
    pcms = []
    for fs in (4096, 1024):
        fmt = alac_amd.make_format(fs, depth, 2, 44100)
        pcms.append(decoded(gpu_ctx, fmt, gpu_ctx.encode_float(fmt, xt, dither="tpdf", seed=9), frames // fs))
    assert np.array_equal(pcms[0], pcms[1])
    s, _, n = restated(x, depth, 9)
    assert np.array_equal(pcms[0], pack(s, depth, n))


def test_a_file_in_a_batch_equals_the_file_alone(gpu_ctx):
    fmt = alac_amd.make_format(FS, 16, 2, 44100)
    xa, xb = make_x(16, 2, FS + 500, 1), make_x(16, 2, 3 * FS, 2)
    both = np.zeros((2, 5 * FS), np.float32)
    both[:, :FS + 500] = xa
    both[:, 2 * FS:] = xb
    dev = lambda v, dt=torch.int32: torch.tensor(v, dtype=dt, device="cuda")  # noqa: E731
    b = gpu_ctx.encode_float(fmt, torch.from_numpy(both).cuda(), num_samples=dev([FS, 500, FS, FS, FS]), seg_first=dev([0, 2, 5]),
                             dither="tpdf", seed=21, packet_origin=dev([0, FS, 0, FS, 2 * FS], torch.int64))
    got = fetch(gpu_ctx, b)
    alone = [fetch(gpu_ctx, gpu_ctx.encode_float(fmt, torch.from_numpy(v).cuda(), seg_first=dev([0, k]), dither="tpdf", seed=21))
             for v, k in ((xa, 2), (xb, 3))]
    assert np.array_equal(got[1], np.concatenate([alone[0][1], alone[1][1]]))
    assert np.array_equal(got[0], np.concatenate([alone[0][0], alone[1][0]]))
    # without the table the second file's frames count on from the first file's packets: other dither, other bytes
    b = gpu_ctx.encode_float(fmt, torch.from_numpy(both).cuda(), num_samples=dev([FS, 500, FS, FS, FS]), seg_first=dev([0, 2, 5]),
                             dither="tpdf", seed=21)
    assert not np.array_equal(fetch(gpu_ctx, b)[0], got[0])


def test_seed_and_channel_index_change_the_pcm(gpu_ctx):
    fmt = alac_amd.make_format(FS, 16, 2, 44100)
    x = make_x(16, 2, 2 * FS, 3)
    x[1] = x[0]  # the same signal on both channels: only the dither tells them apart

    def pcm(v, **kw):
        out = decoded(gpu_ctx, fmt, gpu_ctx.encode_float(fmt, torch.from_numpy(v).cuda(), dither="tpdf", **kw), 2)
        return out.view("<i2").reshape(-1, 2).T

    a, b = pcm(x, seed=1), pcm(x, seed=2)
    assert np.array_equal(a, pcm(x, seed=1))  # reproducible
    assert not np.array_equal(a, b)
    assert not np.array_equal(a[0], a[1])
    assert np.abs(a.astype(np.int64) - b).max() <= 2  # two dithers of the same samples: within +-1 LSB each
    s, _, _ = restated(x, 16, 1, channels=[1, 0])
    assert not np.array_equal(a, s) and np.array_equal(a, s[::-1])


@pytest.mark.parametrize("depth", [16, 32])
def test_without_dither_it_is_encode_float(gpu_ctx, depth):
    fmt = alac_amd.make_format(FS, depth, 2, 44100)
    frames = 3 * FS + 77
    x = make_x(depth, 2, frames, 8)
    buf = torch.full((2, frames + 64), FAR, device="cuda")
    buf[:, :frames] = torch.from_numpy(x).cuda()
    view = buf[:, :frames]
    b = gpu_ctx.encode_float(fmt, view, clipped=True)
    want, clips = fetch(gpu_ctx, b), b["clipped"].cpu().tolist()
    ot = origin_tensor([5, 6, 7, 8])
    b = gpu_ctx.encode_float(fmt, view, clipped=True, dither="none", seed=99, packet_origin=ot)  # mode NONE: origin ignored
    assert_same(fetch(gpu_ctx, b), want, "mode NONE")
    assert b["clipped"].cpu().tolist() == clips
    # a NULL struct through the new entry point
    lib, n = gpu_ctx.lib, 4
    bufs = gpu_ctx.encode_buffers(fmt, n)
    ns = torch.tensor([FS] * 3 + [77], dtype=torch.int32, device="cuda")
    wsb = int(lib.alac_hip_encode_float_workspace_bytes(C.byref(fmt), n, n))
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = lib.alac_hip_encode_float_dither(gpu_ctx.h, C.byref(fmt), view.data_ptr(), view.stride(0), 1, ns.data_ptr(), n, None, n, 0,
                                          None, 0, ws.data_ptr(), wsb, bufs["out"].data_ptr(), bufs["out"].numel(),
                                          bufs["sizes"].data_ptr(), bufs["offsets"].data_ptr(), None, None, ot.data_ptr() + 4)
    assert rc == 0, lib.alac_hip_last_error(gpu_ctx.h)
    assert_same(fetch(gpu_ctx, bufs), want, "dither NULL")


def host_call(ctx, fmt, x, cs, fst, counts, seg, dither, origin):
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
    org = None if origin is None else np.ascontiguousarray(origin, np.uint64)
    rc = lib.alac_hip_encode_float_dither_host(ctx.h, C.byref(fmt), x.ctypes.data, cs, fst, ns.ctypes.data, n, sg.ctypes.data,
                                               len(seg) - 1, state.ctypes.data, 0, out.ctypes.data, cap, sizes.ctypes.data,
                                               C.byref(total), clip.ctypes.data, C.byref(dither) if dither else None,
                                               None if org is None else org.ctypes.data)
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
    for origin in (None, [2 ** 32 + 1, 0, 7, FS, 2 * FS]):
        st = torch.zeros(2 * int(gpu_ctx.lib.alac_hip_state_int16(C.byref(fmt))), dtype=torch.int16, device="cuda")
        b = gpu_ctx.encode_float(fmt, torch.from_numpy(x).cuda(), seg_first=torch.tensor(seg, dtype=torch.int32, device="cuda"),
                                 state=st, clipped=True, dither="tpdf", seed=2 ** 63 + 5,
                                 packet_origin=None if origin is None else origin_tensor(origin))
        dev = fetch(gpu_ctx, b)
        assert_same(dev, reference(gpu_ctx, fmt, x, 2 ** 63 + 5, None, origin, seg_first=torch.tensor(seg, dtype=torch.int32,
                                                                                                   device="cuda"))[0], "device")
        want_state, want_clip = st.cpu().numpy(), b["clipped"].cpu().numpy()
        dz = alac_amd.Dither(1, 0, 2 ** 63 + 5)
        for name, arr, cs, fst in (("planar", x, frames, 1), ("interleaved", np.ascontiguousarray(x.T), 1, channels)):
            stream, sizes, clip, state = host_call(gpu_ctx, fmt, arr, cs, fst, counts, seg, dz, origin)
            assert np.array_equal(sizes, dev[1]) and np.array_equal(stream, dev[0]), name
            assert np.array_equal(clip, want_clip), name
            assert np.array_equal(state, want_state), name
    # the host form without dither is alac_hip_encode_float_host
    plain = fetch(gpu_ctx, gpu_ctx.encode_float(fmt, torch.from_numpy(x).cuda(),
                                                seg_first=torch.tensor(seg, dtype=torch.int32, device="cuda")))
    for dz in (None, alac_amd.Dither(0, 0, 4)):
        stream, sizes, _, _ = host_call(gpu_ctx, fmt, x, frames, 1, counts, seg, dz, None)
        assert np.array_equal(sizes, plain[1]) and np.array_equal(stream, plain[0])


def test_refusals_write_nothing(gpu_ctx):
    ctx, lib = gpu_ctx, gpu_ctx.lib
    fmt = alac_amd.make_format(FS, 16, 2, 44100)
    n = 4
    xn = make_x(16, 2, n * FS, 2)
    x = torch.from_numpy(xn).cuda()
    cap = int(lib.alac_hip_encode_max_output_bytes(C.byref(alac_amd.make_format(FS, 32, 2, 44100)), n))
    out = torch.full((cap,), 0xAB, dtype=torch.uint8, device="cuda")
    sizes = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    offs = torch.full((n + 1,), 9, dtype=torch.int64, device="cuda")
    clip = torch.full((n,), 5, dtype=torch.int32, device="cuda")
    wsb = int(lib.alac_hip_encode_float_workspace_bytes(C.byref(alac_amd.make_format(FS, 32, 2, 44100)), n, n))
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    origin = origin_tensor([0, FS, 2 * FS, 3 * FS, 0])
    torch.cuda.synchronize()

    def call(ptr=x.data_ptr(), fst=1, f=fmt, ws_bytes=wsb, capacity=cap, dz=alac_amd.Dither(1, 0, 3), org=origin.data_ptr()):
        return lib.alac_hip_encode_float_dither(ctx.h, C.byref(f), ptr, n * FS, fst, None, n, None, n, 0, None, 0, ws.data_ptr(),
                                                ws_bytes, out.data_ptr(), capacity, sizes.data_ptr(), offs.data_ptr(),
                                                clip.data_ptr(), None if dz is None else C.byref(dz), org)

    cases = {
        "mode 2": dict(dz=alac_amd.Dither(2, 0, 3)),
        "mode 0xffffffff": dict(dz=alac_amd.Dither(0xFFFFFFFF, 0, 3)),
        "reserved": dict(dz=alac_amd.Dither(1, 1, 3)),
        "reserved with mode NONE": dict(dz=alac_amd.Dither(0, 8, 3)),
        "32 bits with TPDF": dict(f=alac_amd.make_format(FS, 32, 2, 44100)),
        "misaligned origin": dict(org=origin.data_ptr() + 4),
        "null d_in": dict(ptr=None),
        "misaligned d_in": dict(ptr=x.data_ptr() + 2),
        "frame_stride 0": dict(fst=0),
        "workspace below the stage": dict(ws_bytes=1024),
        "output capacity": dict(capacity=100),
        "bad format": dict(f=alac_amd.make_format(FS, 18, 2, 44100)),
    }
    for what, kw in cases.items():
        assert call(**kw) == -50, what
    with ctx.options(lpc=1, fast_mode=1):
        assert call() == -50, "lpc + fast_mode"
    ctx.synchronize()
    assert (out == 0xAB).all() and (sizes == 7).all() and (offs == 9).all() and (clip == 5).all()
    # 32 bits is refused only with dither on; and the context is still usable
    assert call(f=alac_amd.make_format(FS, 32, 2, 44100), dz=alac_amd.Dither(0, 0, 3)) == 0
    assert call() == 0
    ctx.synchronize()
    want, clips = reference(ctx, fmt, xn, 3)
    total = int(offs[-1].item())
    assert np.array_equal(out[:total].cpu().numpy(), want[0]) and clip.cpu().tolist() == clips
    with pytest.raises(ValueError):
        ctx.encode_float(fmt, x, dither="rectangular")
