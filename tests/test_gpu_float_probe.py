"""GPU: alac_hip_float_probe.  The reports equal the numpy restatement of the rule (float_probe_ref.py) word for word, in
every layout the kernel reads, at frame counts around its group, wave and block sizes, with single planted samples that move
one field each, and with segment tables whose boundaries fall inside 4-frame groups and waves; a buffer probed twice gives
the same reports; every refusal leaves d_reports alone; and the depth the probe names is the one at which
decode_float(encode_float(x)) == x, while the depth below it is not."""
import ctypes as C

import numpy as np
import pytest
import torch

import alac_amd
import float_probe_ref as fr

pytestmark = pytest.mark.gpu

FS = 4096
COUNTS = [1, 3, 63, 64, 65, 255, 257, 1023, 1025, 4099]
LAYOUTS = {  # name -> channels
    "planar": 2, "planar_offset": 2, "planar_odd_stride": 2, "interleaved": 2, "transposed3": 3, "transposed6": 6,
    "transposed8": 8, "mono": 1, "mono_offset": 1,
}
ONE = np.float32(1.0)
SPECIALS = [np.float32(v) for v in (
    -1.0, 1.0, np.nextafter(ONE, np.float32(0)), -np.nextafter(ONE, np.float32(2)), 0.0, -0.0, 2.0 ** -16, 3 * 2.0 ** -20,
    2.0 ** -23, 2.0 ** -31, 2.0 ** -32, 2.0 ** -140, np.nan, np.inf, -np.inf)]


def base_signal(channels, frames, seed):
    """on the 16-bit grid, away from full scale: a planted sample is the only one of its kind"""
    rng = np.random.default_rng(seed)
    return (rng.integers(-20000, 20000, (channels, frames)) / 32768.0).astype(np.float32)


def device_view(x, layout):
    """x [channels, frames] as a cuda tensor view in the named layout; what lies between the rows is 2.0 (over range if read)"""
    c, t = x.shape
    if layout in ("planar", "mono"):
        return torch.from_numpy(x).cuda()
    if layout in ("planar_offset", "mono_offset"):  # base 4 bytes behind a 16-byte boundary
        buf = torch.full((c * t + 8,), 2.0, dtype=torch.float32, device="cuda")
        v = buf[1:1 + c * t].view(c, t)
    elif layout == "planar_odd_stride":
        cs = (t + 3) // 4 * 4 + 1
        buf = torch.full((c * cs,), 2.0, dtype=torch.float32, device="cuda")
        v = torch.as_strided(buf, (c, t), (cs, 1))
    else:  # interleaved stereo / the transposed view of [T, C]
        return torch.from_numpy(np.ascontiguousarray(x.T)).cuda().t()
    v.copy_(torch.from_numpy(x))
    return v


def probe(ctx, v, table=None):
    r = ctx.probe_float(v, table)
    ctx.synchronize()
    return r.cpu().numpy().view(np.uint32)


def check(ctx, x, layout, table=None, what=""):
    got = probe(ctx, device_view(x, layout), table)
    want = fr.reports(x, table)
    assert got.shape == want.shape and np.array_equal(got, want), (layout, x.shape, table, what, got.tolist(), want.tolist())
    return got


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_layouts_counts_and_planted_samples(gpu_ctx, layout):
    c = LAYOUTS[layout]
    for t in COUNTS:
        base = base_signal(c, t, t)
        split = [0, (t // 3) | 1, t] if t > 1 else [0, 0, 1]  # a boundary at an odd frame
        first = check(gpu_ctx, base, layout, None, "base")
        assert fr.report_depth(first[0]) == 16
        check(gpu_ctx, base, layout, split, "base, split")
        for k, v in enumerate(SPECIALS):
            x = base.copy()
            frame = (0, t - 1, t // 2, min(t - 1, 4 * (t // 8) + 1))[k % 4]
            x[k % c, frame] = v
            check(gpu_ctx, x, layout, split if k % 2 else None, repr(v))


def sprinkled(channels, frames, seed):
    """the base signal with samples of every kind at random places, so that the segments' reports differ"""
    rng = np.random.default_rng(seed)
    x = base_signal(channels, frames, seed)
    more = [np.float32(v) for v in (5 * 2.0 ** -20, -3 * 2.0 ** -24, 2.0 ** -18, 0.75, -1.25, 7 * 2.0 ** -30)]
    for v in SPECIALS + more:
        for _ in range(max(1, frames // 300)):
            x[rng.integers(channels), rng.integers(frames)] = v
    return x


SEG_LAYOUTS = ["planar", "interleaved", "transposed3", "mono", "planar_odd_stride"]


@pytest.mark.parametrize("layout", SEG_LAYOUTS)
def test_segment_tables(gpu_ctx, layout):
    c, t = LAYOUTS[layout], 4099
    x = sprinkled(c, t, 5)
    tables = {
        "odd boundaries": [0, 1, 4, 7, 130, 1001, 2049, 3333, t],
        "empty at the start, in the middle and at the end": [0, 0, 5, 5, 5, 259, 1027, t, t],
        "length 1": [0, 1, 2, 3, 64, 65, 255, 256, 257, 1024, 1025, t - 1, t],
        "one wave, one segment each": [0, 256, 512, 768, 1024, 2048, 4096, t],
    }
    for what, table in tables.items():
        check(gpu_ctx, x, layout, table, what)
    # 300 segments of 1..7 frames: many fall inside one wave.  The table starts behind frame 0 and ends before total_frames
    rng = np.random.default_rng(9)
    table = np.concatenate([[5], 5 + np.cumsum(rng.integers(1, 8, 300))])
    assert table[-1] < t - 8
    y = x.copy()
    y[0, :5] = np.nan  # in front of the first segment
    y[c - 1, table[-1]:] = np.nan  # behind the last one: must not be seen
    y[:, table[0]:table[-1]][np.isnan(y[:, table[0]:table[-1]])] = 0.5
    got = check(gpu_ctx, y, layout, table, "300 short segments")
    assert got.shape == (300, 8) and int(got[:, 2].sum()) == 0
    # a planted sample on each side of a boundary that splits a 4-frame group
    for b in (2, 258, 1027, 4097):
        z = base_signal(c, t, 6)
        z[c - 1, b - 1] = np.float32(2.0 ** -23)
        z[0, b] = np.nan
        got = check(gpu_ctx, z, layout, [0, b, t], f"boundary {b}")
        assert got[0, 4] == 24 and got[0, 2] == 0 and got[1, 4] <= 16 and got[1, 2] == 1


def raw_call(ctx, v, channels, total, table, nseg, ws, reports, cs=None, fs=None, ptr=None, ws_bytes=None):
    tab = None if table is None else np.ascontiguousarray(table, dtype=np.uint64)
    return ctx.lib.alac_hip_float_probe(
        ctx.h, v.data_ptr() if ptr is None else ptr, channels, int(v.stride(0)) if cs is None else cs,
        int(v.stride(1)) if fs is None else fs, total, None if tab is None else tab.ctypes.data, nseg,
        None if ws is None else ws.data_ptr(), (0 if ws is None else ws.numel()) if ws_bytes is None else ws_bytes,
        None if reports is None else reports.data_ptr())


def test_probing_twice_does_not_accumulate(gpu_ctx):
    ctx = gpu_ctx
    x = sprinkled(2, 4099, 11)
    v = device_view(x, "planar")
    table = [0, 7, 7, 1000, 4099]
    ws = torch.empty(int(ctx.lib.alac_hip_float_probe_workspace_bytes(4)), dtype=torch.uint8, device="cuda")
    reports = torch.full((4, 8), 0x55555555, dtype=torch.int32, device="cuda")  # every word is written
    torch.cuda.synchronize()
    want = fr.reports(x, table)
    assert want[:, :4].any() and want[[0, 2, 3], 4].all()
    for _ in range(2):
        assert raw_call(ctx, v, 2, 4099, table, 4, ws, reports) == 0
        ctx.synchronize()
        assert np.array_equal(reports.cpu().numpy().view(np.uint32), want)
    # no table: one segment, and no workspace to speak of
    one = torch.full((1, 8), 0x55555555, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for _ in range(2):
        assert raw_call(ctx, v, 2, 4099, None, 1, None, one, ws_bytes=256) == 0
        ctx.synchronize()
        assert np.array_equal(one.cpu().numpy().view(np.uint32), fr.reports(x))


def test_refusals_write_nothing(gpu_ctx):
    ctx = gpu_ctx
    t = 1000
    v = torch.from_numpy(base_signal(2, t, 1)).cuda()
    nseg = 3
    table = [0, 10, 500, t]
    ws = torch.empty(int(ctx.lib.alac_hip_float_probe_workspace_bytes(nseg)) + 256, dtype=torch.uint8, device="cuda")
    reports = torch.full((nseg, 8), 0x55555555, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ok = dict(ctx=ctx, v=v, channels=2, total=t, table=table, nseg=nseg, ws=ws, reports=reports)
    cases = {
        "null d_in": dict(ptr=0),
        "misaligned d_in": dict(ptr=v.data_ptr() + 2),
        "no channels": dict(channels=0),
        "nine channels": dict(channels=9),
        "frame_stride 0": dict(fs=0),
        "channel_stride 0 with two channels": dict(cs=0),
        "index overflow by the channel stride": dict(cs=1 << 62),
        "index overflow by the frame stride": dict(fs=1 << 62),
        "index overflow by the byte offset": dict(cs=(1 << 62) - 1, total=1, table=[0, 0, 1, 1]),
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
    assert np.array_equal(reports.cpu().numpy().view(np.uint32), fr.reports(v.cpu().numpy(), table))


@pytest.mark.parametrize("channels", [1, 2, 5])
def test_host_form_equals_the_rule(gpu_ctx, channels):
    ctx, t = gpu_ctx, 2051
    x = sprinkled(channels, t, 21)
    table = np.array([3, 64, 64, 1027, t - 2], dtype=np.uint64)
    want = fr.reports(x, table)
    for name, arr, cs, fs in (("planar", x, t, 1), ("interleaved", np.ascontiguousarray(x.T), 1, channels)):
        rep = (alac_amd.FloatReport * 4)()
        rc = ctx.lib.alac_hip_float_probe_host(ctx.h, arr.ctypes.data, channels, cs, fs, t, table.ctypes.data, 4, rep)
        assert rc == 0, ctx.lib.alac_hip_last_error(ctx.h)
        assert np.array_equal(np.frombuffer(bytes(rep), dtype=np.uint32).reshape(4, 8), want), name
        rep = (alac_amd.FloatReport * 1)()
        assert ctx.lib.alac_hip_float_probe_host(ctx.h, arr.ctypes.data, channels, cs, fs, t, None, 1, rep) == 0
        assert np.array_equal(np.frombuffer(bytes(rep), dtype=np.uint32).reshape(1, 8), fr.reports(x)), name


def grid_tensor(depth, frames, seed):
    """stereo floats on the grid of `depth` bits that need all of them"""
    rng = np.random.default_rng(seed)
    top = 2 ** (depth - 1)
    mag = min(top, 2 ** 24)  # |s| < 2^24: every integer is a float32
    s = rng.integers(-mag, mag, (2, frames), dtype=np.int64)
    s[0, 0], s[1, 0] = 1, -mag  # an odd sample: the lowest bit of the depth is in use
    x = (s.astype(np.float64) / top).astype(np.float32)
    assert np.array_equal(x.astype(np.float64) * top, s)
    return x


def round_trip(ctx, x, depth):
    fmt = alac_amd.make_format(FS, depth, x.shape[0], 44100)
    b = ctx.encode_float(fmt, torch.from_numpy(x).cuda())
    n = (x.shape[1] + FS - 1) // FS
    pcm, ns, st, _ = ctx.decode_float(ctx.magic_cookie(fmt), b["out"], b["offsets"], n)
    ctx.synchronize()
    assert st.abs().sum().item() == 0
    return np.array_equal(pcm[:, :x.shape[1]].cpu().numpy().view(np.uint32), x.view(np.uint32))


@pytest.mark.parametrize("depth", [16, 20, 24, 32])
def test_the_named_depth_is_the_lossless_one(gpu_ctx, depth):
    frames = FS + 100
    x = grid_tensor(depth, frames, depth)
    if depth == 16:
        x = (np.random.default_rng(1).integers(-32768, 32768, (2, frames), dtype=np.int16) / np.float32(32768)).astype(np.float32)
    assert gpu_ctx.lossless_depth(torch.from_numpy(x).cuda()) == [depth]
    assert round_trip(gpu_ctx, x, depth)
    below = {20: 16, 24: 20, 32: 24}.get(depth)
    if below:
        assert not round_trip(gpu_ctx, x, below)  # the probe is what separates them
    # per segment: the first half alone is 16-bit material
    y = x.copy()
    y[:, :FS // 2] = base_signal(2, FS // 2, 3)
    assert gpu_ctx.lossless_depth(torch.from_numpy(y).cuda(), [0, FS // 2, frames]) == [16, depth]


def test_full_scale_has_no_lossless_depth(gpu_ctx):
    x = base_signal(2, 1000, 4)
    x[1, 777] = 1.0
    assert gpu_ctx.lossless_depth(torch.from_numpy(x).cuda()) == [0]
    assert gpu_ctx.lossless_depth(torch.from_numpy(x).cuda(), [0, 777, 778, 1000]) == [16, 0, 16]
    x[1, 777] = -1.0
    assert gpu_ctx.lossless_depth(torch.from_numpy(x).cuda()) == [16]
    assert gpu_ctx.lossless_depth(torch.zeros(2, 100, device="cuda")) == [16]


# ---- more than one pass of the grid-stride loop -------------------------------------------------------------------------------
# A launch has at most 1 024 blocks of 1 024 frames, so behind frame PASS = 1 024 * 1 024 every block takes a second and a
# third pass: its lanes' accumulators live across the passes and are flushed when the wave's segment changes between two of
# them.  LONG_T frames are three passes; what is planted differs from pass to pass, so every report depends on the later ones.
PASS = 1024 * 1024
LONG_T = 2 * PASS + 300001
LONG_LAYOUTS = ["planar", "interleaved", "planar_odd_stride"]
INSIDE = PASS + 5 * 1024 + 2 * 256 + 77  # inside wave 2 of block 5 on its second pass
LONG_TABLES = {
    "one segment": None,
    "boundaries at the passes: every wave changes segment between two passes": [0, PASS, 2 * PASS, LONG_T],
    "boundaries beside the passes": [0, PASS - 1, PASS + 1, 2 * PASS - 3, 2 * PASS + 5, LONG_T],
    "a boundary inside a wave of the second pass": [0, INSIDE, LONG_T],
    "a first segment behind frame 0, empty segments, an end before total_frames":
        [1001, 1001, PASS + 1301, PASS + 1301, 2 * PASS + 999, LONG_T - 7],
}


@pytest.fixture(scope="module")
def long_signal():
    """(x [2, LONG_T], {table name: reports of the rule}); computed once, the tests do not write to it"""
    rng = np.random.default_rng(77)
    x = base_signal(2, LONG_T, 77)
    plants = (  # (first frame, end frame, values): the first pass alone is 16-bit material
        (0, PASS, (0.75, -0.0)),
        (PASS, 2 * PASS, (2.0 ** -23, 1.0, 3 * 2.0 ** -20)),
        (2 * PASS, LONG_T, (np.nan, 2.0 ** -31, -1.25, np.inf)),
    )
    for a, b, values in plants:
        for k, v in enumerate(values):
            frames = np.concatenate([rng.integers(a, b, 40), [a + k, b - 1 - k]])
            x[rng.integers(0, 2, frames.size), frames] = np.float32(v)
    x[0, INSIDE - 1], x[1, INSIDE] = np.float32(2.0 ** -23), np.float32(1.0)  # on each side of the boundary inside the wave
    x[1, LONG_T - 3] = np.float32(2.0 ** -140)  # behind the end of the last table
    want = {what: fr.reports(x, table) for what, table in LONG_TABLES.items()}
    one = want["one segment"][0]
    assert fr.report_depth(fr.report(x[:, :PASS])) == 16 and one[4] == 141 and one[0] > 100 and one[2] > 30
    assert want["a boundary inside a wave of the second pass"][0, 4] == 24
    return x, want


@pytest.mark.parametrize("layout", LONG_LAYOUTS)
def test_accumulators_across_passes_of_the_loop(gpu_ctx, long_signal, layout):
    x, want = long_signal
    v = device_view(x, layout)
    for what, table in LONG_TABLES.items():
        got = probe(gpu_ctx, v, table)
        assert np.array_equal(got, want[what]), (layout, what, got.tolist(), want[what].tolist())


def test_the_table_is_done_with_when_the_call_returns(gpu_ctx, long_signal):
    """a table in pinned host memory, overwritten as soon as the call has returned"""
    ctx = gpu_ctx
    x, want = long_signal
    v = device_view(x, "planar")
    what = "boundaries beside the passes"
    nseg = len(LONG_TABLES[what]) - 1
    table = torch.tensor(LONG_TABLES[what], dtype=torch.int64).pin_memory()
    ws = torch.empty(int(ctx.lib.alac_hip_float_probe_workspace_bytes(nseg)), dtype=torch.uint8, device="cuda")
    reports = torch.empty((nseg, 8), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for _ in range(3):  # the later calls find the stream busy with the earlier ones
        assert ctx.lib.alac_hip_float_probe(ctx.h, v.data_ptr(), 2, LONG_T, 1, LONG_T, table.data_ptr(), nseg, ws.data_ptr(),
                                            ws.numel(), reports.data_ptr()) == 0
        table.zero_()
        table.copy_(torch.tensor(LONG_TABLES[what], dtype=torch.int64))
    assert ctx.lib.alac_hip_float_probe(ctx.h, v.data_ptr(), 2, LONG_T, 1, LONG_T, table.data_ptr(), nseg, ws.data_ptr(),
                                        ws.numel(), reports.data_ptr()) == 0
    table.zero_()
    ctx.synchronize()
    assert np.array_equal(reports.cpu().numpy().view(np.uint32), want[what])


@pytest.mark.parametrize("channels", [1, 2, 8])
def test_no_frames(gpu_ctx, channels):
    """a tensor without frames: every segment is empty, an empty segment's report is all zero and its depth 16"""
    x = torch.empty((channels, 0), dtype=torch.float32, device="cuda")
    assert not probe(gpu_ctx, x).any() and probe(gpu_ctx, x).shape == (1, 8)
    assert not probe(gpu_ctx, x.t().contiguous().t(), [0, 0, 0]).any()
    assert gpu_ctx.lossless_depth(x) == [16]
    assert gpu_ctx.lossless_depth(x, [0, 0, 0]) == [16, 16]
    with pytest.raises(alac_amd.AlacError):
        gpu_ctx.probe_float(x, [0, 1])
