"""GPU: alac_hip_loudness_int / alac_hip_loudness_float.  The rows equal the sequential numpy restatement of the rule
(loudness_ref.py) within |E - E_ref| <= 1e-9 E_ref + 1e-10 hop — about twenty times what reordering the restatement's own sums
moves them — and the peaks and counts equal it exactly, at chunk counts around what a wave and a scan group cover, with tables
whose boundaries fall anywhere, for every container, justification, depth and layout, at six sample rates; a segment gives the
same bits wherever it lies and whatever lies beside it; decode followed by a measurement equals the measurement of the source;
the host forms equal the device forms; every refusal leaves the outputs alone.
Inputs: seeded noise plus a full-scale 25 Hz tone, quantised to the source's depth.  Sample rate 8 000 (hop 800, chunks of 50
frames) unless a case says otherwise."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import alac_amd
import loudness_ref as lr

pytestmark = pytest.mark.gpu

FS = 8000
HOP = FS // 10
L = lr.chunk_frames(FS)
WAVE = 64  # chunks a wave of a vector layout covers
GROUP = lr.GROUP_CHUNKS


def signal(frames, channels, fs=FS, seed=1):
    """float64 [channels, frames] in [-1, 1): noise plus a full-scale 25 Hz tone, each channel its own phase and noise"""
    rng = np.random.default_rng(seed)
    t = np.arange(frames, dtype=np.float64)
    tone = np.sin(2.0 * math.pi * 25.0 * t[None, :] / fs + np.arange(channels)[:, None])
    return np.clip(tone + 0.05 * rng.standard_normal((channels, frames)), -1.0, 1.0 - 2.0 ** -15)


def quantise(x, bits):
    return np.clip(np.rint(x * 2.0 ** (bits - 1)), -(1 << (bits - 1)), (1 << (bits - 1)) - 1).astype(np.int64)


def check(energy, reports, x, fs, table=None, nonfinite=None, what=""):
    """the call's outputs against the restatement on x float64 [channels, frames] (the values of the rule)"""
    hop = fs // 10
    want, want_reports = lr.measure(x.T, fs, table, None if nonfinite is None else nonfinite.T)
    got = energy.cpu().numpy()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want)
    bound = 1e-9 * want + 1e-10 * hop
    if want.size:
        print(what, "rows", want.shape[0], "max err / bound", float((err / bound).max()), "max rel", float((err / np.maximum(want, 1e-300)).max()))
    assert (err <= bound).all(), (what, float((err / bound).max()))
    reps = alac_amd.Context.loudness_reports(reports)
    assert len(reps) == len(want_reports)
    for s, (r, (first, n, peak, bad)) in enumerate(zip(reps, want_reports)):
        assert (r.first_block, r.num_blocks, r.peak, r.nonfinite, r.reserved) == (first, n, peak, bad, 0), (what, s)
        a, b = alac_amd.integrated_loudness(got[first:first + n], hop), lr.integrated(want[first:first + n], hop)
        assert a == b if math.isinf(b) else abs(a - b) <= 1e-6, (what, s, a, b)


def int16_planar(gpu_ctx, s):
    return torch.from_numpy(s.astype(np.int16)).to(gpu_ctx.device)


# ---- chunk, wave and group geometry ----------------------------------------------------------------------------------------
GEOMETRY = sorted({k * L + HOP - 1 for k in (WAVE - 1, WAVE, WAVE + 1, 2 * WAVE + 1)} |
                  {k * L - 1 for k in (WAVE - 1, WAVE, WAVE + 1, 2 * WAVE + 1)} |
                  {k * L + 7 for k in (GROUP - 1, GROUP, GROUP + 1, 2 * GROUP + 1)})


@pytest.fixture(scope="module")
def long_signal():
    """one signal and its 16-bit samples for every geometry case: [3, frames]"""
    x = signal(max(GEOMETRY), 3, seed=11)
    s = quantise(x, 16)
    return s, s.astype(np.float64) * 2.0 ** -15


@pytest.mark.parametrize("frames", GEOMETRY)
def test_one_segment_around_the_wave_and_the_group(gpu_ctx, long_signal, frames):
    s, x = long_signal
    for channels in (1, 3):  # a vector layout (64 chunks per wave) and the general one (one lane per chunk and channel)
        energy, reports = gpu_ctx.loudness_int(int16_planar(gpu_ctx, s[:channels, :frames]), FS)
        gpu_ctx.synchronize()
        check(energy, reports, x[:channels, :frames], FS, what="frames %d channels %d" % (frames, channels))


def test_segments_of_every_small_size_in_one_table(gpu_ctx, long_signal):
    s, x = long_signal
    sizes = [0, 1, HOP - 1, HOP, 4 * HOP - 1, 4 * HOP, 0, 3]
    table = np.concatenate([[0], np.cumsum(sizes)])
    for channels in (2, 3):
        energy, reports = gpu_ctx.loudness_int(int16_planar(gpu_ctx, s[:channels, :table[-1]]), FS, seg_first_frame=table)
        gpu_ctx.synchronize()
        check(energy, reports, x[:channels, :table[-1]], FS, table, what="sizes channels %d" % channels)


# ---- tables ----------------------------------------------------------------------------------------------------------------
# odd boundaries, an empty segment, a start behind frame 0 and an end before total_frames
TABLE = [13, 13 + 4 * HOP + 1, 4001, 4001, 4002 + 5 * HOP + 3, 9107, 9107 + HOP]
TOTAL = TABLE[-1] + 37


def outside(table, total):
    m = np.ones(total, dtype=bool)
    m[table[0]:table[-1]] = False
    return m


def test_int_frames_outside_the_table_are_not_read(gpu_ctx):
    x = signal(TOTAL, 2, seed=3) * 0.5
    s = quantise(x, 16)
    table = TABLE
    dirty = s.copy()
    dirty[:, outside(table, TOTAL)] = -32768  # full scale: would be the peak of any segment that read it
    energy, reports = gpu_ctx.loudness_int(int16_planar(gpu_ctx, dirty), FS, seg_first_frame=table)
    gpu_ctx.synchronize()
    check(energy, reports, s.astype(np.float64) * 2.0 ** -15, FS, table, what="int table")
    assert max(r.peak for r in alac_amd.Context.loudness_reports(reports)) < 1.0


def test_float_frames_outside_the_table_are_not_read(gpu_ctx):
    x = (signal(TOTAL, 2, seed=4) * 0.5).astype(np.float32)
    table = TABLE
    dirty = x.copy()
    dirty[:, outside(table, TOTAL)] = np.nan
    energy, reports = gpu_ctx.loudness_float(torch.from_numpy(dirty).to(gpu_ctx.device), FS, seg_first_frame=table)
    gpu_ctx.synchronize()
    check(energy, reports, x.astype(np.float64), FS, table, np.zeros(x.shape, bool), what="float table")


# ---- sources ---------------------------------------------------------------------------------------------------------------
FRAMES = 4 * HOP + 2 * L + 3


def int_source(gpu_ctx, v, cb, layout, offset=0):
    """containers v [channels, frames] (int64, sign-extended) on the device in the named layout -> (tensor, keyword arguments);
    offset: containers in front of the first one (a base off the vector alignment)"""
    c, n = v.shape
    if cb == 3:
        flat = v.T.reshape(-1) if layout == "interleaved" else v.reshape(-1)
        kw = dict(container_bytes=3, num_channels=c, channel_stride=1 if layout == "interleaved" else n,
                  frame_stride=c if layout == "interleaved" else 1)
        b = np.zeros((offset + flat.size, 3), np.uint8)
        u = flat & 0xFFFFFF
        b[offset:, 0], b[offset:, 1], b[offset:, 2] = u & 255, (u >> 8) & 255, u >> 16
        return torch.from_numpy(b.reshape(-1)).to(gpu_ctx.device)[3 * offset:], kw
    dt = np.int16 if cb == 2 else np.int32
    if layout == "interleaved":
        buf = np.zeros(offset + n * c, dt)
        buf[offset:] = v.T.reshape(-1).astype(dt)
        return torch.from_numpy(buf).to(gpu_ctx.device)[offset:].view(n, c).t(), {}
    stride = n + 8 - n % 4  # rows a multiple of 4 containers apart, with room between them
    buf = np.zeros(offset + c * stride, dt)
    for ch in range(c):
        buf[offset + ch * stride: offset + ch * stride + n] = v[ch].astype(dt)
    return torch.as_strided(torch.from_numpy(buf).to(gpu_ctx.device), (c, n), (stride, 1), offset), {}


INT_CASES = [(2, 16, 1, "planar", 2, 0), (2, 16, 1, "interleaved", 2, 0), (2, 16, 0, "planar", 1, 0), (2, 16, 1, "planar", 2, 1),
             (2, 16, 1, "interleaved", 2, 3), (3, 24, 1, "interleaved", 2, 0), (3, 24, 1, "planar", 1, 0),
             (3, 20, 1, "interleaved", 2, 1), (3, 16, 0, "planar", 1, 1), (3, 24, 0, "interleaved", 3, 0),
             (4, 20, 1, "planar", 2, 0), (4, 20, 0, "planar", 2, 0), (4, 24, 1, "interleaved", 2, 0), (4, 24, 0, "planar", 1, 0),
             (4, 32, 1, "planar", 2, 0), (4, 32, 0, "interleaved", 2, 2), (4, 24, 1, "planar", 6, 0), (4, 16, 1, "interleaved", 8, 0),
             (2, 16, 1, "interleaved", 6, 0), (4, 32, 1, "planar", 3, 1)]


@pytest.mark.parametrize("cb,bits,lj,layout,channels,offset", INT_CASES)
def test_integer_sources(gpu_ctx, cb, bits, lj, layout, channels, offset):
    s = quantise(signal(FRAMES, channels, seed=bits + channels), bits)
    s[0, 5], s[channels - 1, FRAMES - 1] = -(1 << (bits - 1)), (1 << (bits - 1)) - 1  # both ends of the range
    v = s << (8 * cb - bits) if lj else s.copy()
    if lj and 8 * cb > bits:
        v |= np.random.default_rng(0).integers(0, 1 << (8 * cb - bits), v.shape)  # pad bits are not part of the sample
    if not lj and 8 * cb > bits:
        v[0, 9], v[channels - 1, 11] = (1 << (bits - 1)) + 5, -(1 << (bits - 1)) - 77  # out of range: saturated
    t, kw = int_source(gpu_ctx, v, cb, layout, offset)
    energy, reports = gpu_ctx.loudness_int(t, FS, bits=bits, left_justified=bool(lj), **kw)
    gpu_ctx.synchronize()
    check(energy, reports, lr.int_values(v, bits, lj, 8 * cb), FS, what=str((cb, bits, lj, layout, channels, offset)))


FLOAT_CASES = [("planar", 1, 0), ("planar", 2, 0), ("interleaved", 2, 0), ("padded", 2, 0), ("planar", 2, 1), ("interleaved", 2, 1),
               ("padded", 3, 0), ("interleaved", 6, 0), ("planar", 8, 0)]


def float_source(gpu_ctx, x, layout, offset=0):
    c, n = x.shape
    if layout == "interleaved":
        buf = np.full(offset + n * c, np.nan, np.float32)
        buf[offset:] = x.T.reshape(-1)
        return torch.from_numpy(buf).to(gpu_ctx.device)[offset:].view(n, c).t()
    stride, step = (n + 8 - n % 4, 1) if layout == "planar" else (3 * n + 5, 3)
    buf = np.full(offset + c * stride, np.nan, np.float32)
    for ch in range(c):
        buf[offset + ch * stride: offset + ch * stride + n * step: step] = x[ch]
    return torch.as_strided(torch.from_numpy(buf).to(gpu_ctx.device), (c, n), (stride, step), offset)


@pytest.mark.parametrize("layout,channels,offset", FLOAT_CASES)
def test_float_sources(gpu_ctx, layout, channels, offset):
    x = (signal(FRAMES, channels, seed=channels) * 1.5).astype(np.float32)  # over full scale: floats are not clipped
    energy, reports = gpu_ctx.loudness_float(float_source(gpu_ctx, x, layout, offset), FS)
    gpu_ctx.synchronize()
    check(energy, reports, x.astype(np.float64), FS, nonfinite=np.zeros(x.shape, bool), what=str((layout, channels, offset)))


def test_non_finite_floats_are_counted_and_read_as_zero(gpu_ctx):
    x = (signal(FRAMES, 2, seed=9) * 0.7).astype(np.float32)
    x[0, [3, 900, 901]] = [np.nan, np.inf, -np.inf]
    x[1, [0, FRAMES - 1]] = [-np.inf, np.nan]
    x[1, 50] = np.float32(1e-42)  # a denormal is finite
    table = [0, 850, 850, FRAMES]
    values, bad = lr.float_values(x)
    for layout in ("planar", "interleaved", "padded"):
        energy, reports = gpu_ctx.loudness_float(float_source(gpu_ctx, x, layout), FS, seg_first_frame=table)
        gpu_ctx.synchronize()
        check(energy, reports, values, FS, table, bad, what="non-finite " + layout)
        assert [r.nonfinite for r in alac_amd.Context.loudness_reports(reports)] == [2, 0, 3]


# ---- rates, decay ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs", [8000, 22050, 44100, 48000, 96000, 192000])
def test_rates(gpu_ctx, fs):
    frames = 4 * (fs // 10) + 321
    s = quantise(signal(frames, 2, fs, seed=fs), 16)
    energy, reports = gpu_ctx.loudness_int(int16_planar(gpu_ctx, s), fs)
    gpu_ctx.synchronize()
    check(energy, reports, s.astype(np.float64) * 2.0 ** -15, fs, what="rate %d" % fs)


def test_decay_into_digital_silence_and_back(gpu_ctx):
    """two seconds at full scale, three of digital zeros (the states decay through the whole double range of the high-pass's
    slow pole), then signal at 1e-4: the rows of the quiet part are compared at the same bound"""
    x = np.concatenate([signal(2 * FS, 2, seed=21), np.zeros((2, 3 * FS)), 1e-4 * signal(FS + 17, 2, seed=22)], axis=1)
    s = quantise(x, 24)
    t, kw = int_source(gpu_ctx, s << 8, 4, "planar")
    energy, reports = gpu_ctx.loudness_int(t, FS, bits=24, **kw)
    gpu_ctx.synchronize()
    check(energy, reports, s.astype(np.float64) * 2.0 ** -23, FS, what="decay")


# ---- determinism -----------------------------------------------------------------------------------------------------------
def raw_words(energy, reports):
    return energy.cpu().numpy().view(np.uint64), reports.cpu().numpy().view(np.uint32)


def test_a_segment_gives_the_same_bits_wherever_it_lies(gpu_ctx):
    n = 5 * HOP + 2 * L + 11
    s = quantise(signal(n, 2, seed=31), 16)
    alone = raw_words(*gpu_ctx.loudness_int(int16_planar(gpu_ctx, s), FS))
    # as the 3rd of 7 segments, at an odd offset, between segments of other sizes
    other = quantise(signal(9000, 2, seed=32), 16)
    sizes = [HOP + 1, 2 * HOP + 7, n, 0, 3 * HOP, 5, HOP - 1]
    parts, at = [], 3
    table = [at]
    for i, size in enumerate(sizes):
        parts.append(s if i == 2 else other[:, 100 * i:100 * i + size])
        at += size
        table.append(at)
    buf = np.concatenate([other[:, :3]] + parts + [other[:, :50]], axis=1)
    e7, r7 = raw_words(*gpu_ctx.loudness_int(int16_planar(gpu_ctx, buf), FS, seg_first_frame=table))
    first, rows = int(r7[2, 0]), int(r7[2, 1])
    assert rows == alone[1][0, 1] == 5 and first == (HOP + 1) // HOP + (2 * HOP + 7) // HOP
    assert np.array_equal(e7[first:first + rows], alone[0])
    assert np.array_equal(r7[2, 1:], alone[1][0, 1:])
    # at a different offset in a larger buffer
    big = np.concatenate([other[:, :1001], s, other[:, :7]], axis=1)
    e1, r1 = raw_words(*gpu_ctx.loudness_int(int16_planar(gpu_ctx, big), FS, seg_first_frame=[1001, 1001 + n]))
    assert np.array_equal(e1, alone[0]) and np.array_equal(r1[0, 1:], alone[1][0, 1:])
    # ... and interleaved at a base off the vector alignment: the general layout, one lane per chunk and channel
    t, _ = int_source(gpu_ctx, big, 2, "interleaved", offset=1)
    e2, r2 = raw_words(*gpu_ctx.loudness_int(t, FS, seg_first_frame=[1001, 1001 + n]))
    assert np.array_equal(e2, alone[0]) and np.array_equal(r2[0, 1:], alone[1][0, 1:])
    # ... and interleaved at an aligned base: the layout whose loads are staged through LDS (the planar ones above are not)
    t, _ = int_source(gpu_ctx, big, 2, "interleaved")
    e3, r3 = raw_words(*gpu_ctx.loudness_int(t, FS, seg_first_frame=[1001, 1001 + n]))
    assert np.array_equal(e3, alone[0]) and np.array_equal(r3[0, 1:], alone[1][0, 1:])
    gpu_ctx.synchronize()


def call_int(gpu_ctx, x, fs, table, energy, reports, ws=None, ws_bytes=None, rows=None, src=None, channels=None, frames=None,
             d_in=True):
    """alac_hip_loudness_int itself, into the caller's tensors"""
    lib = gpu_ctx.lib
    channels = x.shape[0] if channels is None else channels
    frames = x.shape[1] if frames is None else frames
    src = alac_amd.IntSource(2, 16, 1, 0, x.stride(0), x.stride(1)) if src is None else src
    tab = None if table is None else np.ascontiguousarray(table, dtype=np.uint64)
    nseg = 1 if tab is None else tab.size - 1
    if ws is None:
        ws = torch.empty(int(lib.alac_hip_loudness_workspace_bytes(fs, channels, frames, nseg)), dtype=torch.uint8, device=gpu_ctx.device)
    torch.cuda.synchronize()
    return lib.alac_hip_loudness_int(gpu_ctx.h, x.data_ptr() if d_in else None, C.byref(src) if src is not False else None, channels, fs,
                                     frames, None if tab is None else tab.ctypes.data, nseg,
                                     ws.data_ptr() if ws is not False else None, ws.numel() if ws_bytes is None else ws_bytes,
                                     energy.data_ptr() if energy is not False else None,
                                     energy.shape[0] if rows is None else rows, reports.data_ptr() if reports is not False else None)


def test_a_second_call_into_the_same_buffers_does_not_accumulate(gpu_ctx):
    n = 6 * HOP + 5
    x = int16_planar(gpu_ctx, quantise(signal(n, 2, seed=41), 16))
    table = [0, 2 * HOP + 3, n]
    energy = torch.full((6, 2), 7.0, dtype=torch.float64, device=gpu_ctx.device)
    reports = torch.full((2, 8), -1, dtype=torch.int32, device=gpu_ctx.device)
    assert call_int(gpu_ctx, x, FS, table, energy, reports) == 0
    gpu_ctx.synchronize()
    first = raw_words(energy, reports)
    assert call_int(gpu_ctx, x, FS, table, energy, reports) == 0
    gpu_ctx.synchronize()
    second = raw_words(energy, reports)
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1])
    fresh = raw_words(*gpu_ctx.loudness_int(x, FS, seg_first_frame=table))
    assert np.array_equal(first[0], fresh[0]) and np.array_equal(first[1], fresh[1])


# ---- composition with the decoder -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [16, 24])
def test_decode_then_loudness_equals_loudness_of_the_source(gpu_ctx, depth):
    fmt = alac_amd.make_format(4096, depth, 2, 44100)
    n = 3
    pcm = alac_amd.synth_pcm(0, n, fmt)
    d_pcm = torch.from_numpy(pcm).to(gpu_ctx.device)
    stream, sizes = gpu_ctx.encode_to_host(fmt, d_pcm, n)
    offs = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes.astype(np.int64))])).to(gpu_ctx.device)
    cookie = gpu_ctx.magic_cookie(fmt)
    d_stream = torch.from_numpy(stream).to(gpu_ctx.device)
    out, ns, st, _ = gpu_ctx.decode(cookie, d_stream, offs, n)
    gpu_ctx.synchronize()
    assert int(st.abs().sum()) == 0

    def measure(buf):
        if depth == 16:
            return gpu_ctx.loudness_int(buf.view(torch.int16).view(n * 4096, 2).t(), 44100)
        return gpu_ctx.loudness_int(buf, 44100, bits=24, container_bytes=3, num_channels=2, channel_stride=1, frame_stride=2)

    src, dec = raw_words(*measure(d_pcm)), raw_words(*measure(out))
    assert src[0].shape == (2, 2) and np.array_equal(src[0], dec[0]) and np.array_equal(src[1], dec[1])
    if depth == 16:
        f, _, st, _ = gpu_ctx.decode_float(cookie, d_stream, offs, n)
        flt = raw_words(*gpu_ctx.loudness_float(f, 44100))
        assert np.array_equal(src[0], flt[0]) and np.array_equal(src[1], flt[1])
    gpu_ctx.synchronize()


# ---- host forms -------------------------------------------------------------------------------------------------------------
def test_host_forms_equal_the_device_forms(gpu_ctx):
    n = 4 * HOP + 77
    s = quantise(signal(n + 100, 2, seed=51), 16).astype(np.int16)
    table = np.array([3, 2 * HOP + 9, n], dtype=np.uint64)
    lib = gpu_ctx.lib
    dev = raw_words(*gpu_ctx.loudness_int(torch.from_numpy(s).to(gpu_ctx.device), FS, seg_first_frame=table))
    gpu_ctx.synchronize()
    assert dev[0].shape == (4, 2)
    energy, reports = np.full((5, 2), 9.0), np.zeros((2, 8), np.uint32)
    src = alac_amd.IntSource(2, 16, 1, 0, s.shape[1], 1)
    assert lib.alac_hip_loudness_int_host(gpu_ctx.h, s.ctypes.data, C.byref(src), 2, FS, s.shape[1], table.ctypes.data, 2,
                                          energy.ctypes.data, 5, reports.ctypes.data) == 0
    assert np.array_equal(energy[:4].view(np.uint64), dev[0]) and np.array_equal(reports, dev[1]) and (energy[4] == 9.0).all()
    f = (s.astype(np.float32) / 32768.0)
    f[:, n:] = np.nan  # behind the last segment: not staged, not read
    dev = raw_words(*gpu_ctx.loudness_float(torch.from_numpy(f).to(gpu_ctx.device), FS, seg_first_frame=table))
    gpu_ctx.synchronize()
    energy, reports = np.full((4, 2), 9.0), np.zeros((2, 8), np.uint32)
    assert lib.alac_hip_loudness_float_host(gpu_ctx.h, f.ctypes.data, 2, f.shape[1], 1, FS, f.shape[1], table.ctypes.data, 2,
                                            energy.ctypes.data, 4, reports.ctypes.data) == 0
    assert np.array_equal(energy.view(np.uint64), dev[0]) and np.array_equal(reports, dev[1])
    assert lib.alac_hip_loudness_float_host(gpu_ctx.h, f.ctypes.data, 2, f.shape[1], 1, FS, f.shape[1], table.ctypes.data, 2,
                                            energy.ctypes.data, 3, reports.ctypes.data) == -50
    assert lib.alac_hip_loudness_int_host(gpu_ctx.h, s.ctypes.data, C.byref(src), 2, 44101, s.shape[1], table.ctypes.data, 2,
                                          energy.ctypes.data, 5, reports.ctypes.data) == -50


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone(gpu_ctx):
    n = 3 * HOP
    x = int16_planar(gpu_ctx, quantise(signal(n, 2, seed=61), 16))
    energy = torch.full((3, 2), 7.0, dtype=torch.float64, device=gpu_ctx.device)
    reports = torch.full((1, 8), -1, dtype=torch.int32, device=gpu_ctx.device)
    ws = torch.zeros(int(gpu_ctx.lib.alac_hip_loudness_workspace_bytes(FS, 2, n, 2)) + 64, dtype=torch.uint8, device=gpu_ctx.device)
    good = alac_amd.IntSource(2, 16, 1, 0, n, 1)
    assert call_int(gpu_ctx, x, FS, None, energy, reports, ws=ws) == 0
    gpu_ctx.synchronize()
    energy.fill_(7.0), reports.fill_(-1)
    S = alac_amd.IntSource
    cases = {
        "null d_in": dict(d_in=False),
        "null src": dict(src=False),
        "container bytes": dict(src=S(5, 16, 1, 0, n, 1)),
        "bits": dict(src=S(2, 24, 1, 0, n, 1)),
        "reserved": dict(src=S(2, 16, 1, 1, n, 1)),
        "left_justified": dict(src=S(2, 16, 2, 0, n, 1)),
        "frame_stride 0": dict(src=S(2, 16, 1, 0, n, 0)),
        "channel_stride 0": dict(src=S(2, 16, 1, 0, 0, 1)),
        "index overflow": dict(src=S(2, 16, 1, 0, 1 << 63, 1 << 62)),
        "channels 0": dict(channels=0),
        "channels 9": dict(channels=9),
        "rate not a multiple of 10": dict(fs=44101),
        "rate too low": dict(fs=7990),
        "rate too high": dict(fs=384010),
        "table not ascending": dict(table=[0, 900, 800]),
        "table behind total_frames": dict(table=[0, n + 1]),
        "null workspace": dict(ws=False, ws_bytes=1 << 20),
        "workspace too small": dict(ws_bytes=int(gpu_ctx.lib.alac_hip_loudness_workspace_bytes(FS, 2, n, 1)) - 1),
        "misaligned workspace": dict(ws=ws[4:]),
        "energy_rows too small": dict(rows=2),
        "null energy": dict(energy=False, rows=3),
        "misaligned energy": dict(energy=energy.view(torch.uint8)[4:], rows=3),
        "null reports": dict(reports=False),
        "misaligned reports": dict(reports=reports.view(torch.uint8)[4:]),
    }
    for name, kw in cases.items():
        args = dict(x=x, fs=FS, table=None, energy=energy, reports=reports, ws=ws, src=good)
        args.update(kw)
        rc = call_int(gpu_ctx, **args)
        gpu_ctx.synchronize()
        assert rc == -50, name
        assert bool((energy == 7.0).all()) and bool((reports == -1).all()), name
    # num_segments 0, and more than one segment without a table
    for nseg in (0, 2):
        rc = gpu_ctx.lib.alac_hip_loudness_int(gpu_ctx.h, x.data_ptr(), C.byref(good), 2, FS, n, None, nseg, ws.data_ptr(), ws.numel(),
                                               energy.data_ptr(), 3, reports.data_ptr())
        assert rc == -50
    # the float call: what alac_hip_float_probe refuses, and the same rates
    f = torch.zeros((2, n), dtype=torch.float32, device=gpu_ctx.device)
    lib = gpu_ctx.lib

    def call_float(d_in=f.data_ptr(), channels=2, cs=n, fst=1, fs=FS, frames=n, rows=3):
        return lib.alac_hip_loudness_float(gpu_ctx.h, d_in, channels, cs, fst, fs, frames, None, 1, ws.data_ptr(), ws.numel(),
                                           energy.data_ptr(), rows, reports.data_ptr())

    assert call_float() == 0
    gpu_ctx.synchronize()
    energy.fill_(7.0), reports.fill_(-1)
    for name, kw in {"null": dict(d_in=None), "misaligned": dict(d_in=f.data_ptr() + 2), "channels": dict(channels=9),
                     "frame_stride": dict(fst=0), "channel_stride": dict(cs=0), "rate": dict(fs=48001), "rows": dict(rows=2),
                     "overflow": dict(cs=1 << 63, fst=1 << 62)}.items():
        assert call_float(**kw) == -50, name
        gpu_ctx.synchronize()
        assert bool((energy == 7.0).all()) and bool((reports == -1).all()), name
