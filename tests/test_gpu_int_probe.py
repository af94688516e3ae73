"""GPU: alac_hip_int_probe.  The reports equal the numpy restatement of the rule (int_probe_ref.py) word for word, for every
container, justification and depth, in every layout the kernel reads, at frame counts around its group, wave and block sizes,
with single planted containers that move the fields they should and no other, and with segment tables whose boundaries fall
inside 4-frame groups and waves; a buffer probed twice gives the same reports; every refusal leaves d_reports alone; and the
depth the probe names is the one to which requantize() and back is exact, while the depth below it is not."""
import ctypes as C

import numpy as np
import pytest
import torch

import alac_amd
import int_probe_ref as ir
import pcm_requant_ref as pr

pytestmark = pytest.mark.gpu

COUNTS = [1, 3, 63, 64, 65, 255, 257, 1023, 1025, 4099]
# (container bytes, S, left_justified): every depth a container allows, both justifications
SOURCES = [(cb, S, lj) for cb, depths in ((2, (16,)), (3, (16, 20, 24)), (4, (16, 20, 24, 32))) for S in depths for lj in (1, 0)]
TENSOR_LAYOUTS = {  # name -> channels; int16 and int32 tensors
    "planar": 2, "planar_offset": 2, "planar_odd_stride": 2, "interleaved": 2, "transposed3": 3, "transposed8": 8, "mono": 1,
    "mono_offset": 1,
}
PACKED_LAYOUTS = {  # packed 3-byte containers in a uint8 tensor
    "packed_interleaved": 2, "packed_planar": 2, "packed_mono": 1, "packed_mono_offset": 1, "packed_transposed3": 3,
}
WORD = {"out_of_range": 0, "differing_frames": 2, "need_bits": 4, "peak": 5, "pad_bits": 6}


def channels_of(layout):
    return TENSOR_LAYOUTS.get(layout) or PACKED_LAYOUTS[layout]


def base_containers(src, channels, frames, seed, dual=False):
    """containers whose samples need at most 14 bits and stay far from full scale, no pad bit set, in range; every channel
    differs from channel 0 in every frame (dual: all channels identical): a planted container is the only one of its kind"""
    cb, S, lj = src
    rng = np.random.default_rng(seed)
    r = rng.integers(-3000, 3000, (1, frames), dtype=np.int64) + (0 if dual else 7) * np.arange(channels, dtype=np.int64)[:, None]
    r[:, min(2, frames - 1)] = 3001 + 7 * np.arange(channels) * (not dual)  # needs all 14 bits, and is the peak: frame 2 (no
    # container is planted there in 63 frames or more)
    s = r << (S - 14)
    return s << (8 * cb - S) if lj else s


def poison(cb):
    """what lies between the rows: a container that would move every field it can if it were read"""
    return {2: 0x7FFF, 3: 0x7F7F7F, 4: 0x7FFFFFFF}[cb]


def device_source(v, cb, layout):
    """containers v [channels, frames] (sign-extended, int64) as a cuda tensor in the named layout -> (tensor, probe_int's
    keyword arguments for it)"""
    c, t = v.shape
    if cb == 3:
        gap = np.full(5, poison(3), np.int64)
        if layout == "packed_interleaved" or layout == "packed_transposed3":
            flat, kw, lead = v.T.reshape(-1), dict(channel_stride=1, frame_stride=c), 0
        elif layout == "packed_planar":  # rows of t + 5 containers
            flat, kw, lead = np.concatenate([v[0], gap, v[1]]), dict(channel_stride=t + 5, frame_stride=1, num_channels=2), 0
        else:  # mono; _offset: the base one byte behind a 4-byte boundary
            flat, kw, lead = v[0], dict(channel_stride=t, frame_stride=1, num_channels=1), int(layout == "packed_mono_offset")
        data = np.concatenate([np.full(lead, 0x7F, np.uint8), pr.pack3(flat)])
        return torch.from_numpy(data).cuda()[lead:], dict(container_bytes=3, **kw)
    dt, tdt = (np.int16, torch.int16) if cb == 2 else (np.int32, torch.int32)
    x = v.astype(dt)
    assert np.array_equal(x, v)
    if layout in ("planar", "mono"):
        return torch.from_numpy(x).cuda(), {}
    if layout in ("planar_offset", "mono_offset"):  # base one container behind a 16-byte boundary
        buf = torch.full((c * t + 8,), poison(cb), dtype=tdt, device="cuda")
        view = buf[1:1 + c * t].view(c, t)
    elif layout == "planar_odd_stride":
        cs = (t + 3) // 4 * 4 + 1
        buf = torch.full((c * cs,), poison(cb), dtype=tdt, device="cuda")
        view = torch.as_strided(buf, (c, t), (cs, 1))
    else:  # interleaved stereo / the transposed view of [T, C]
        return torch.from_numpy(np.ascontiguousarray(x.T)).cuda().t(), {}
    view.copy_(torch.from_numpy(x))
    return view, {}


def probe(ctx, x, src, kw, table=None):
    r = ctx.probe_int(x, bits=src[1], left_justified=bool(src[2]), seg_first_frame=table, **kw)
    ctx.synchronize()
    return r.cpu().numpy().view(np.uint32)


def check(ctx, v, src, layout, table=None, what=""):
    x, kw = device_source(v, src[0], layout)
    got = probe(ctx, x, src, kw, table)
    want = ir.reports(v, src, table)
    assert got.shape == want.shape and np.array_equal(got, want), (src, layout, v.shape, table, what, got.tolist(), want.tolist())
    return got


def plants(src, channels):
    """(name, container as a function of the base container there, channel, fields that move) for one planted container"""
    cb, S, lj = src
    P, top = 8 * cb - S, 1 << (S - 1)
    put = (lambda s: s << P) if lj else (lambda s: s)
    out = [("an odd sample", lambda b: put(1), 0, {"need_bits"}), ("-2^(S-1)", lambda b: put(-top), channels - 1, {"peak"})]
    if P and not lj:  # a right-justified container one step out of range on each side: counted and saturated
        out += [("2^(S-1)", lambda b: top, 0, {"out_of_range", "need_bits", "peak"}),
                ("-2^(S-1) - 1", lambda b: -top - 1, channels - 1, {"out_of_range", "peak"})]
    if P and lj:
        out += [("a pad bit", lambda b: b | 1, channels - 1, {"pad_bits"}), ("the top pad bit", lambda b: b | (1 << (P - 1)), 0, {"pad_bits"})]
    return out


def moved(a, b):
    return {k for k, w in WORD.items() if a[w] != b[w] or (w < 4 and a[w + 1] != b[w + 1])}


def run_counts(ctx, layout, sources, counts):
    c = channels_of(layout)
    for i, t in enumerate(counts):
        src = sources[i % len(sources)]
        base = base_containers(src, c, t, t)
        split = [0, (t // 3) | 1, t] if t > 1 else [0, 0, 1]  # a boundary at an odd frame
        first = check(ctx, base, src, layout, None, "base")
        assert ir.report_depth(first[0]) == 16 and first[0, 4] == 14
        assert int(first[0, 2]) == (t if c > 1 else 0)
        check(ctx, base, src, layout, split, "base, split")
        for k, (name, value, ch, fields) in enumerate(plants(src, c)):
            v = base.copy()
            frame = (0, t - 1, t // 2, min(t - 1, 4 * (t // 8) + 1))[k % 4]
            v[ch, frame] = value(int(base[ch, frame]))
            got = check(ctx, v, src, layout, split if k % 2 else None, name)
            if t >= 63 and not k % 2:  # (in fewer frames the planted container may replace the one that needs 14 bits)
                assert moved(first[0], got[0]) == fields, (src, layout, t, name)
        if c > 1:  # one frame in which channel 1 differs, in material that is dual mono
            dual = base_containers(src, c, t, t, dual=True)
            assert check(ctx, dual, src, layout, None, "dual mono")[0, 2] == 0
            dual[1, t // 2] += 1 << (8 * src[0] - 14 if src[2] else src[1] - 14)
            got = check(ctx, dual, src, layout, split, "channel 1 differs in one frame")
            assert int(got[:, 2].sum()) == 1


@pytest.mark.parametrize("cb", [2, 4])
@pytest.mark.parametrize("layout", list(TENSOR_LAYOUTS))
def test_tensor_layouts_counts_and_planted_containers(gpu_ctx, layout, cb):
    run_counts(gpu_ctx, layout, [s for s in SOURCES if s[0] == cb], COUNTS)


@pytest.mark.parametrize("layout", list(PACKED_LAYOUTS))
def test_packed_layouts_counts_and_planted_containers(gpu_ctx, layout):
    run_counts(gpu_ctx, layout, [s for s in SOURCES if s[0] == 3], COUNTS)


@pytest.mark.parametrize("src", SOURCES, ids=["%dB-S%d-%s" % (cb, S, "left" if lj else "right") for cb, S, lj in SOURCES])
def test_every_source(gpu_ctx, src):
    """every (container, depth, justification) on a vector path and on the general one"""
    for layout in (("packed_interleaved", "packed_planar") if src[0] == 3 else ("planar", "transposed3")):
        run_counts(gpu_ctx, layout, [src], [257, 1025])


def sprinkled(src, channels, frames, seed):
    """the base signal with containers of every kind at random places, so that the segments' reports differ"""
    rng = np.random.default_rng(seed)
    v = base_containers(src, channels, frames, seed, dual=True)
    v[1:, rng.integers(0, frames, frames // 50)] += 1 << (8 * src[0] - 14 if src[2] else src[1] - 14)
    kinds = plants(src, channels) + plants(src, channels)[:2]
    for name, value, ch, _ in kinds:
        for _ in range(max(1, frames // 300)):
            f = rng.integers(frames)
            v[ch, f] = value(int(v[ch, f]))
    return v


SEG_CASES = [("planar", (4, 24, 1)), ("interleaved", (4, 20, 0)), ("transposed3", (2, 16, 1)), ("mono", (2, 16, 0)),
             ("planar_odd_stride", (4, 32, 1)), ("packed_interleaved", (3, 20, 1)), ("packed_planar", (3, 16, 0)),
             ("packed_mono", (3, 24, 1))]


@pytest.mark.parametrize("layout,src", SEG_CASES, ids=[c[0] for c in SEG_CASES])
def test_segment_tables(gpu_ctx, layout, src):
    c, t = channels_of(layout), 4099
    v = sprinkled(src, c, t, 5)
    tables = {
        "odd boundaries": [0, 1, 4, 7, 130, 1001, 2049, 3333, t],
        "empty at the start, in the middle and at the end": [0, 0, 5, 5, 5, 259, 1027, t, t],
        "length 1": [0, 1, 2, 3, 64, 65, 255, 256, 257, 1024, 1025, t - 1, t],
        "one wave, one segment each": [0, 256, 512, 768, 1024, 2048, 4096, t],
    }
    for what, table in tables.items():
        check(gpu_ctx, v, src, layout, table, what)
    # 300 segments of 1..7 frames: many fall inside one wave.  The table starts behind frame 0 and ends before total_frames;
    # what lies outside it is an odd sample at full scale, which must not be seen
    rng = np.random.default_rng(9)
    table = np.concatenate([[5], 5 + np.cumsum(rng.integers(1, 8, 300))])
    assert table[-1] < t - 8
    y = base_containers(src, c, t, 6)
    top = (1 << (src[1] - 1)) - 1
    y[0, :5] = y[c - 1, table[-1]:] = top << (8 * src[0] - src[1]) if src[2] else top
    got = check(gpu_ctx, y, src, layout, table, "300 short segments")
    assert got.shape == (300, 8) and int(got[:, 4].max()) <= 14 and int(got[:, 5].max()) < top
    # a planted container on each side of a boundary that splits a 4-frame group
    odd, low = plants(src, c)[:2]
    for b in (2, 258, 1027, 4097):
        z = base_containers(src, c, t, 6)
        z[c - 1, b - 1] = odd[1](0)
        z[0, b] = low[1](0)
        got = check(gpu_ctx, z, src, layout, [0, b, t], f"boundary {b}")
        assert got[0, 4] == src[1] and got[0, 5] < top and got[1, 4] <= 14 and got[1, 5] == top + 1


def raw_call(ctx, x, src, channels, total, table, nseg, ws, reports, ptr=None, ws_bytes=None, src_null=False):
    tab = None if table is None else np.ascontiguousarray(table, dtype=np.uint64)
    return ctx.lib.alac_hip_int_probe(
        ctx.h, x.data_ptr() if ptr is None else ptr, None if src_null else C.byref(src), channels, total,
        None if tab is None else tab.ctypes.data, nseg, None if ws is None else ws.data_ptr(),
        (0 if ws is None else ws.numel()) if ws_bytes is None else ws_bytes, None if reports is None else reports.data_ptr())


def test_probing_twice_does_not_accumulate(gpu_ctx):
    ctx = gpu_ctx
    for src in ((4, 24, 1), (4, 20, 0)):
        v = sprinkled(src, 2, 4099, 11)
        x, _ = device_source(v, 4, "planar")
        struct = alac_amd.IntSource(4, src[1], src[2], 0, 4099, 1)
        table = [0, 7, 7, 1000, 4099]
        ws = torch.empty(int(ctx.lib.alac_hip_int_probe_workspace_bytes(4)), dtype=torch.uint8, device="cuda")
        reports = torch.full((4, 8), 0x55555555, dtype=torch.int32, device="cuda")  # every word is written
        torch.cuda.synchronize()
        want = ir.reports(v, src, table)
        assert want[[0, 2, 3], 4].all() and want[:, 2].any() and want[:, 6 if src[2] else 0].any()
        for _ in range(2):
            assert raw_call(ctx, x, struct, 2, 4099, table, 4, ws, reports) == 0
            ctx.synchronize()
            assert np.array_equal(reports.cpu().numpy().view(np.uint32), want)
        # no table: one segment, and no workspace to speak of
        one = torch.full((1, 8), 0x55555555, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for _ in range(2):
            assert raw_call(ctx, x, struct, 2, 4099, None, 1, None, one, ws_bytes=256) == 0
            ctx.synchronize()
            assert np.array_equal(one.cpu().numpy().view(np.uint32), ir.reports(v, src))


def test_refusals_write_nothing(gpu_ctx):
    ctx = gpu_ctx
    t = 1000
    src = (4, 24, 1)
    v = base_containers(src, 2, t, 1)
    x, _ = device_source(v, 4, "planar")
    x16 = torch.zeros(2 * t + 8, dtype=torch.int16, device="cuda")
    nseg = 3
    table = [0, 10, 500, t]
    ws = torch.empty(int(ctx.lib.alac_hip_int_probe_workspace_bytes(nseg)) + 256, dtype=torch.uint8, device="cuda")
    reports = torch.full((nseg, 8), 0x55555555, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def source(cb=4, bits=24, lj=1, reserved=0, cs=t, fs=1):
        return alac_amd.IntSource(cb, bits, lj, reserved, cs, fs)

    ok = dict(ctx=ctx, x=x, src=source(), channels=2, total=t, table=table, nseg=nseg, ws=ws, reports=reports)
    cases = {
        # what alac_hip_pcm_requantize refuses in a source
        "null d_in": dict(ptr=0),
        "null src": dict(src_null=True),
        "container_bytes 1": dict(src=source(cb=1, bits=16)),
        "container_bytes 5": dict(src=source(cb=5)),
        "bits 18": dict(src=source(bits=18)),
        "bits 12": dict(src=source(bits=12)),
        "bits above the container": dict(src=source(cb=3, bits=32)),
        "24 bits in int16": dict(x=x16, src=source(cb=2, bits=24)),
        "reserved": dict(src=source(reserved=1)),
        "left_justified 2": dict(src=source(lj=2)),
        "misaligned int32 base": dict(ptr=x.data_ptr() + 2),
        "misaligned int16 base": dict(ptr=x16.data_ptr() + 1, src=source(cb=2, bits=16)),
        "frame_stride 0": dict(src=source(fs=0)),
        "channel_stride 0 with two channels": dict(src=source(cs=0)),
        "index overflow by the channel stride": dict(src=source(cs=1 << 62)),
        "index overflow by the frame stride": dict(src=source(fs=1 << 62)),
        "index overflow by the byte offset": dict(src=source(cs=(1 << 62) - 1), total=1, table=[0, 0, 1, 1]),
        # what alac_hip_float_probe refuses in channels, table, workspace and report pointer
        "no channels": dict(channels=0),
        "nine channels": dict(channels=9),
        "num_segments 0": dict(nseg=0),
        "table not ascending": dict(table=[0, 500, 10, t]),
        "table ends behind total_frames": dict(table=[0, 10, 500, t + 1]),
        "no table for three segments": dict(table=None),
        "workspace too small": dict(ws_bytes=(nseg + 1) * 8 - 1),
        "null workspace": dict(ws=None, ws_bytes=ws.numel()),
        "misaligned workspace": dict(ws=ws[4:], ws_bytes=ws.numel() - 4),
        "misaligned d_reports": dict(reports=reports.view(-1)[1:]),
    }
    for what, kw in cases.items():
        assert raw_call(**{**ok, **kw}) == -50, what
    assert raw_call(**{**ok, "reports": None}) == -50
    ctx.synchronize()
    assert bool((reports == 0x55555555).all())
    # the context is still usable
    assert raw_call(**ok) == 0
    ctx.synchronize()
    assert np.array_equal(reports.cpu().numpy().view(np.uint32), ir.reports(v, src, table))


@pytest.mark.parametrize("channels", [1, 2, 5])
def test_host_form_equals_the_rule(gpu_ctx, channels):
    ctx, t = gpu_ctx, 2051
    table = np.array([3, 64, 64, 1027, t - 2], dtype=np.uint64)
    for src in ((2, 16, 1), (3, 20, 1), (3, 24, 0), (4, 24, 0), (4, 32, 1)):
        v = sprinkled(src, channels, t, 21)
        want = ir.reports(v, src, table)
        for name, arr, cs, fs in (("planar", v, t, 1), ("interleaved", np.ascontiguousarray(v.T), 1, channels)):
            host = pr.pack3(arr) if src[0] == 3 else arr.astype(np.int16 if src[0] == 2 else np.int32).reshape(-1)
            struct = alac_amd.IntSource(src[0], src[1], src[2], 0, cs, fs)
            rep = (alac_amd.IntReport * 4)()
            rc = ctx.lib.alac_hip_int_probe_host(ctx.h, host.ctypes.data, C.byref(struct), channels, t, table.ctypes.data, 4, rep)
            assert rc == 0, ctx.lib.alac_hip_last_error(ctx.h)
            assert np.array_equal(np.frombuffer(bytes(rep), dtype=np.uint32).reshape(4, 8), want), (src, name)
            rep = (alac_amd.IntReport * 1)()
            assert ctx.lib.alac_hip_int_probe_host(ctx.h, host.ctypes.data, C.byref(struct), channels, t, None, 1, rep) == 0
            assert np.array_equal(np.frombuffer(bytes(rep), dtype=np.uint32).reshape(1, 8), ir.reports(v, src)), (src, name)


@pytest.mark.parametrize("channels", [1, 2, 8])
def test_no_frames(gpu_ctx, channels):
    """a tensor without frames: every segment is empty, an empty segment's report is all zero and its depth 16"""
    for dt in (torch.int16, torch.int32):
        x = torch.empty((channels, 0), dtype=dt, device="cuda")
        assert not probe(gpu_ctx, x, (0, None, 1), {}).any() and probe(gpu_ctx, x, (0, None, 1), {}).shape == (1, 8)
        assert not probe(gpu_ctx, x.t().contiguous().t(), (0, None, 0), {}, [0, 0, 0]).any()
        assert gpu_ctx.lossless_depth_int(x) == [16]
        assert gpu_ctx.lossless_depth_int(x, seg_first_frame=[0, 0, 0]) == [16, 16]
        with pytest.raises(alac_amd.AlacError):
            gpu_ctx.probe_int(x, seg_first_frame=[0, 1])
    empty = torch.empty(0, dtype=torch.uint8, device="cuda")
    assert gpu_ctx.lossless_depth_int(empty, bits=24, container_bytes=3, channel_stride=1, frame_stride=channels) == [16]
    rep = (alac_amd.IntReport * 2)()
    rep[0].need_bits = rep[1].peak = 77
    table = np.zeros(3, np.uint64)
    struct = alac_amd.IntSource(4, 32, 1, 0, 1, channels)
    host = np.zeros(4, np.int32)
    assert gpu_ctx.lib.alac_hip_int_probe_host(gpu_ctx.h, host.ctypes.data, C.byref(struct), channels, 0, table.ctypes.data, 2, rep) == 0
    assert not np.frombuffer(bytes(rep), dtype=np.uint32).any()


# ---- the depth the probe names ---------------------------------------------------------------------------------------------
FS = 1024


def exact_samples(need, frames, seed):
    """stereo 24-bit samples that need exactly `need` bits"""
    rng = np.random.default_rng(seed)
    s = rng.integers(-(1 << (need - 1)), 1 << (need - 1), (2, frames), dtype=np.int64) << (24 - need)
    s[0, 0], s[1, 0] = 1 << (24 - need), -(1 << 23)  # the lowest bit of the depth is in use, and full scale
    return s


def there_and_back(ctx, s, depth):
    """24-bit samples in packed 3-byte containers -> requantize to `depth` -> requantize that back to 24 bits: the bytes"""
    ch, frames = s.shape
    src = torch.from_numpy(pr.pack3(s.T.reshape(-1))).cuda()
    down = ctx.requantize(alac_amd.make_format(FS, depth, ch, 44100), src, bits=24, container_bytes=3, channel_stride=1, frame_stride=ch)
    packets = (frames + FS - 1) // FS
    up_fmt = alac_amd.make_format(FS, 24, ch, 44100)
    if depth == 16:
        back = ctx.requantize(up_fmt, down.view(torch.int16).view(packets * FS, ch).t(), bits=16)
    else:  # 20 bits come left-justified in their 3 bytes
        back = ctx.requantize(up_fmt, down, bits=depth, container_bytes=3, channel_stride=1, frame_stride=ch)
    ctx.synchronize()
    return np.array_equal(back[:frames * ch * 3].cpu().numpy(), src.cpu().numpy())


@pytest.mark.parametrize("need", [16, 20, 24])
def test_the_named_depth_is_the_lossless_one(gpu_ctx, need):
    frames = FS + 100
    s = exact_samples(need, frames, need)
    packed = dict(bits=24, container_bytes=3, channel_stride=1, frame_stride=2)
    x = torch.from_numpy(pr.pack3(s.T.reshape(-1))).cuda()
    assert gpu_ctx.lossless_depth_int(x, **packed) == [need]
    assert there_and_back(gpu_ctx, s, need)
    below = {20: 16, 24: 20}.get(need)
    if below:
        assert not there_and_back(gpu_ctx, s, below)  # the probe is what separates them
    # per segment: the first half alone is 16-bit material
    y = s.copy()
    y[:, :FS // 2] = exact_samples(16, FS // 2, 3)
    x = torch.from_numpy(pr.pack3(y.T.reshape(-1))).cuda()
    assert gpu_ctx.lossless_depth_int(x, seg_first_frame=[0, FS // 2, frames], **packed) == [16, need]
    # the same samples left-justified in int32, and as floats: the float probe names the same depth
    for v in (s, y):
        xi = torch.from_numpy((v << 8).astype(np.int32)).cuda()
        xf = torch.from_numpy((v.astype(np.float64) / (1 << 23)).astype(np.float32)).cuda()
        for table in (None, [0, FS // 2, frames], [5, 5, 300, frames - 1]):
            assert gpu_ctx.lossless_depth_int(xi, bits=24, seg_first_frame=table) == gpu_ctx.lossless_depth(xf, table)


def test_out_of_range_and_pad_bits_have_no_depth(gpu_ctx):
    s = exact_samples(16, 1000, 4)
    x = (s << 8).astype(np.int32)
    x[1, 777] |= 0x10
    xi = torch.from_numpy(x).cuda()
    assert gpu_ctx.lossless_depth_int(xi, bits=24) == [0]
    assert gpu_ctx.lossless_depth_int(xi, bits=24, seg_first_frame=[0, 777, 778, 1000]) == [16, 0, 16]
    assert gpu_ctx.lossless_depth_int(xi, bits=32) == [32]  # the bit is part of a 32-bit sample
    r = s.astype(np.int32)
    r[0, 5] = 1 << 23
    xr = torch.from_numpy(r).cuda()
    assert gpu_ctx.lossless_depth_int(xr, bits=24, left_justified=False, seg_first_frame=[0, 5, 6, 1000]) == [16, 0, 16]
    assert gpu_ctx.lossless_depth_int(xr, bits=32, left_justified=False) == [24]  # in range there: samples of 24 bits in 32
    assert gpu_ctx.lossless_depth_int(torch.zeros(2, 100, dtype=torch.int16, device="cuda")) == [16]


# ---- more than one pass of the grid-stride loop -------------------------------------------------------------------------------
# A launch has at most 1 024 blocks of 1 024 frames, so behind frame PASS = 1 024 * 1 024 every block takes a second and a
# third pass: its lanes' accumulators live across the passes and are flushed when the wave's segment changes between two of
# them.  LONG_T frames are three passes; what is planted differs from pass to pass, so every report depends on the later ones.
PASS = 1024 * 1024
LONG_T = 2 * PASS + 300001
INSIDE = PASS + 5 * 1024 + 2 * 256 + 77  # inside wave 2 of block 5 on its second pass
LONG_TABLES = {
    "one segment": None,
    "boundaries at the passes: every wave changes segment between two passes": [0, PASS, 2 * PASS, LONG_T],
    "boundaries beside the passes": [0, PASS - 1, PASS + 1, 2 * PASS - 3, 2 * PASS + 5, LONG_T],
    "a boundary inside a wave of the second pass": [0, INSIDE, LONG_T],
    "a first segment behind frame 0, empty segments, an end before total_frames":
        [1001, 1001, PASS + 1301, PASS + 1301, 2 * PASS + 999, LONG_T - 7],
}
# (layout, container bytes, the sources the same containers are read as)
LONG_CASES = {"mono": (2, [(2, 16, 1)]), "interleaved": (4, [(4, 24, 1), (4, 24, 0)])}


def long_containers(cb, channels):
    """16-bit material, dual mono, in the first pass; other things planted in every later pass"""
    rng = np.random.default_rng(77)
    W = 8 * cb
    v = np.repeat(rng.integers(-3000, 3000, (1, LONG_T), dtype=np.int64) << (W - 14), channels, axis=0)
    sh = lambda k: max(W - k, 1)  # noqa: E731  (the lowest bit of the container stays clear until the third pass)
    second = (3 << sh(20), 1 << sh(16), 3500 << (W - 14))  # needs more bits than the first pass; differing frames; a new peak
    third = (1 | (5 << (W - 15)), (1 << (W - 1)) - 1, 1 << (sh(24) - 1), -(1 << (W - 1)))  # the lowest bit, both ends of the range
    for a, b, values in ((PASS, 2 * PASS, second), (2 * PASS, LONG_T, third)):
        for k, x in enumerate(values):
            frames = np.concatenate([rng.integers(a, b, 40), [a + k, b - 1 - k]])
            v[rng.integers(0, channels, frames.size), frames] = x
    v[0, INSIDE - 1], v[channels - 1, INSIDE] = 1 << sh(22), 7 << sh(18)  # on each side of the boundary inside the wave
    v[channels - 1, LONG_T - 3] = -1  # behind the end of the last table
    return v


@pytest.mark.parametrize("layout", list(LONG_CASES))
def test_accumulators_across_passes_of_the_loop(gpu_ctx, layout):
    cb, sources = LONG_CASES[layout]
    c = channels_of(layout)
    v = long_containers(cb, c)
    x, kw = device_source(v, cb, layout)
    for src in sources:
        want = {what: ir.reports(v, src, table) for what, table in LONG_TABLES.items()}
        one = want["one segment"][0]
        first_pass = ir.report(v[:, :PASS], src)
        assert one[4] == src[1] and not np.array_equal(one, first_pass) and not np.array_equal(one, ir.report(v[:, :2 * PASS], src))
        if c > 1:
            assert 40 < one[2] < 400 and first_pass[2] == 0
        for what, table in LONG_TABLES.items():
            got = probe(gpu_ctx, x, src, kw, table)
            assert np.array_equal(got, want[what]), (layout, src, what, got.tolist(), want[what].tolist())
