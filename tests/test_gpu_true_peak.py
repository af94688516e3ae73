"""GPU: alac_hip_true_peak_int / alac_hip_true_peak_float.  The channel peaks equal the numpy restatement of the rule
(true_peak_ref.py, with the library's own coefficients) within a bound that is derived, not measured: the device and the
restatement form the same K products in double and differ in fusing and order only, so an output moves by at most
    taps * 2^-52 * sum_k |h_p[k]| * sample peak          (the phase where that is largest: 12 x 1.864, 24 x 2.307)
and a maximum by no more than its elements.  The sample peak, the non-finite count and `reserved` are equal exactly, and
true_peak >= peak always.  Shapes: around what a lane's run (R frames), a wave and a block (B = 256 R frames) cover, segments
of every small size, peaks at the ends of segments and runs, tables whose boundaries fall anywhere; every container,
justification, depth and layout; a segment gives the same bits wherever it lies; decode followed by a measurement equals the
measurement of the source; the host forms equal the device forms; every refusal leaves the outputs alone.
Sample rate 8 000 (F = 4, K = 12) unless a case says otherwise.
Every check prints the share of the bound it used; the largest any case used on an MI355X is 9.5 %."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import alac_amd
import loudness_ref as lr
import true_peak_ref as tr
from alac_amd.capi import TRUE_PEAK_BLOCK_RUNS, TRUE_PEAK_RUN
from test_gpu_loudness import float_source, int16_planar, int_source, quantise, signal

pytestmark = pytest.mark.gpu

FS = 8000
R = TRUE_PEAK_RUN[4]
K = 12
B = TRUE_PEAK_BLOCK_RUNS * R
USED = [0.0]  # the largest share of the bound so far


def check(peaks, reports, x, fs, table=None, nonfinite=None, what=""):
    """the call's outputs against the restatement on x float64 [channels, frames] (the values of the rule)"""
    _, coefs = alac_amd.true_peak_filter(fs)
    want, want_reports = tr.measure(x.T, fs, table, None if nonfinite is None else nonfinite.T, coefs=coefs)
    got = peaks.cpu().numpy()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    tab = [0, x.shape[1]] if table is None else [int(t) for t in table]
    sample = np.array([np.abs(x[:, a:b]).max(axis=1) if b > a else np.zeros(x.shape[0]) for a, b in zip(tab, tab[1:])])
    err, bound = np.abs(got - want), tr.bound(coefs, sample)
    share = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    USED[0] = max(USED[0], share)
    print(what, "segments", want.shape[0], "share of the bound", share, "largest so far", USED[0])
    assert (err <= bound).all(), (what, share)
    assert (got >= sample).all(), what
    reps = alac_amd.Context.true_peak_reports(reports)
    assert len(reps) == len(want_reports)
    for s, (r, (true, peak, bad)) in enumerate(zip(reps, want_reports)):
        assert (r.peak, r.nonfinite, r.reserved) == (peak, bad, 0), (what, s)
        assert r.true_peak == got[s].max() and r.true_peak >= r.peak, (what, s)
    return got


def int16_interleaved(gpu_ctx, s):
    return int_source(gpu_ctx, s, 2, "interleaved")[0]


# ---- run, wave and block geometry --------------------------------------------------------------------------------------------
GEOMETRY = sorted({k * R + d for k in (63, 64, 65, 255, 256, 257) for d in (-1, 0, 1)} | {B - 1, B, B + 1, 2 * B + 1})


@pytest.fixture(scope="module")
def long_signal():
    """one signal and its 16-bit samples for every geometry case: [3, frames]"""
    x = signal(max(GEOMETRY), 3, seed=11)
    s = quantise(x, 16)
    return s, s.astype(np.float64) * 2.0 ** -15


@pytest.mark.parametrize("frames", GEOMETRY)
def test_one_segment_around_the_run_the_wave_and_the_block(gpu_ctx, long_signal, frames):
    s, x = long_signal
    for channels in (1, 2, 3):  # mono and interleaved stereo (staged through LDS), and the general layout
        src = int16_interleaved(gpu_ctx, s[:2, :frames]) if channels == 2 else int16_planar(gpu_ctx, s[:channels, :frames])
        peaks, reports = gpu_ctx.true_peak_int(src, FS)
        gpu_ctx.synchronize()
        check(peaks, reports, x[:channels, :frames], FS, what="frames %d channels %d" % (frames, channels))


def test_segments_of_every_small_size_in_one_table(gpu_ctx, long_signal):
    s, x = long_signal
    sizes = [0, 1, 2, K - 1, K, K + 1, R - 1, R, R + 1, 5, 0, 7]
    table = np.concatenate([[0], np.cumsum(sizes)])
    for channels in (1, 2, 3):
        part = s[:channels, :table[-1]]
        src = int16_interleaved(gpu_ctx, part) if channels == 2 else int16_planar(gpu_ctx, part)
        peaks, reports = gpu_ctx.true_peak_int(src, FS, seg_first_frame=table)
        gpu_ctx.synchronize()
        got = check(peaks, reports, x[:channels, :table[-1]], FS, table, what="sizes channels %d" % channels)
        assert (got[0] == 0).all() and (got[10] == 0).all()


# ---- where the peak lies -----------------------------------------------------------------------------------------------------
N_IMPULSE = 3 * R + 5
IMPULSE_AT = {"first frame": [0], "last frame": [N_IMPULSE - 1], "last frame of a run": [R - 1], "first frame of a run": [2 * R]}


@pytest.mark.parametrize("where", sorted(IMPULSE_AT))
def test_a_single_sample_gives_itself_exactly(gpu_ctx, where):
    """2^-3 in silence: every product is exact, no output exceeds the sample, true peak = sample peak = 0.125"""
    at = IMPULSE_AT[where][0]
    s = np.zeros((3, 7 + N_IMPULSE + 9), np.int64)
    s[:, 7 + at] = [1 << 12, -(1 << 12), 1 << 12]
    table = [7, 7 + N_IMPULSE]
    x = s.astype(np.float64) * 2.0 ** -15
    for channels in (1, 2, 3):
        src = int16_interleaved(gpu_ctx, s[:2]) if channels == 2 else int16_planar(gpu_ctx, s[:channels])
        peaks, reports = gpu_ctx.true_peak_int(src, FS, seg_first_frame=table)
        gpu_ctx.synchronize()
        got = check(peaks, reports, x[:channels], FS, table, what="impulse %s channels %d" % (where, channels))
        assert (got == 0.125).all()
        r = alac_amd.Context.true_peak_reports(reports)[0]
        assert r.true_peak == r.peak == 0.125


@pytest.mark.parametrize("at", [0, R - 2, R - 1, R, 2 * R - 1, N_IMPULSE - 2])
def test_a_crest_between_two_frames(gpu_ctx, at):
    """two equal samples: the crest lies half a frame behind the first — over a run's end the history carries it, and behind
    the segment's last but one frame the largest outputs lie in the flushed tail"""
    s = np.zeros((3, 7 + N_IMPULSE + 9), np.int64)
    s[:, 7 + at], s[:, 7 + at + 1] = 1 << 14, 1 << 14
    s[:, 7 + N_IMPULSE:] = 32767  # behind the segment: not read
    s[:, :7] = -32768
    table = [7, 7 + N_IMPULSE]
    x = s.astype(np.float64) * 2.0 ** -15
    for channels in (1, 2, 3):
        src = int16_interleaved(gpu_ctx, s[:2]) if channels == 2 else int16_planar(gpu_ctx, s[:channels])
        peaks, reports = gpu_ctx.true_peak_int(src, FS, seg_first_frame=table)
        gpu_ctx.synchronize()
        got = check(peaks, reports, x[:channels], FS, table, what="pair at %d channels %d" % (at, channels))
        assert (got > 0.6).all() and (got < 0.65).all()


def test_the_case_16_sine_cut_at_every_phase_of_the_run(gpu_ctx):
    """fs/4 at 0.5 FS sampled 45 degrees off its crests: the true peak lies 3 dB above the sample peak.  One segment per
    start offset 0 .. R-1, so that the run boundaries fall on every phase of the signal and of the run"""
    sizes = [2 * R + 9 + p for p in range(R)]
    table = np.concatenate([[3], 3 + np.cumsum(sizes)])
    n = np.arange(table[-1] + 4, dtype=np.float64)
    s = quantise(0.5 * np.sin(2.0 * math.pi * n / 4.0 + math.pi / 4.0)[None, :].repeat(3, axis=0), 16)
    x = s.astype(np.float64) * 2.0 ** -15
    for channels in (1, 2, 3):
        src = int16_interleaved(gpu_ctx, s[:2]) if channels == 2 else int16_planar(gpu_ctx, s[:channels])
        peaks, reports = gpu_ctx.true_peak_int(src, FS, seg_first_frame=table)
        gpu_ctx.synchronize()
        got = check(peaks, reports, x[:channels], FS, table, what="case 16 channels %d" % channels)
        for r in alac_amd.Context.true_peak_reports(reports):
            assert abs(tr.dbtp(r.peak) - (-9.03)) < 0.01 and tr.dbtp(r.true_peak) > -6.1


# ---- isolation -------------------------------------------------------------------------------------------------------------
# measured segments (even) between sacrificial ones (odd) that hold what must not leak: a start behind frame 0, an end before
# total_frames, odd boundaries, and K + 5 dirty frames directly in front of every measured segment
ISOLATION_SIZES = [2 * R + 7, K + 5, 1, K + 5, R, K + 5, 3 * R - 1, K + 5, K - 1]
ISOLATION_TABLE = np.concatenate([[K + 6], K + 6 + np.cumsum(ISOLATION_SIZES)])
ISOLATION_TOTAL = int(ISOLATION_TABLE[-1]) + 29


def isolation_mask():
    dirty = np.ones(ISOLATION_TOTAL, dtype=bool)
    for i in range(0, len(ISOLATION_SIZES), 2):
        dirty[ISOLATION_TABLE[i]:ISOLATION_TABLE[i + 1]] = False
    return dirty


def test_int_frames_outside_a_segment_are_not_read_not_even_as_history(gpu_ctx):
    s = quantise(signal(ISOLATION_TOTAL, 3, seed=3) * 0.5, 16)
    dirty = s.copy()
    dirty[:, isolation_mask()] = -32768
    x = s.astype(np.float64) * 2.0 ** -15
    want, _ = tr.measure(x.T, FS, ISOLATION_TABLE, coefs=alac_amd.true_peak_filter(FS)[1])
    for channels in (1, 2, 3):
        src = int16_interleaved(gpu_ctx, dirty[:2]) if channels == 2 else int16_planar(gpu_ctx, dirty[:channels])
        peaks, reports = gpu_ctx.true_peak_int(src, FS, seg_first_frame=ISOLATION_TABLE)
        gpu_ctx.synchronize()
        got = check(peaks, reports, dirty[:channels].astype(np.float64) * 2.0 ** -15, FS, ISOLATION_TABLE,
                    what="int isolation channels %d" % channels)
        clean, _ = gpu_ctx.true_peak_int(int16_interleaved(gpu_ctx, s[:2]) if channels == 2 else int16_planar(gpu_ctx, s[:channels]),
                                         FS, seg_first_frame=ISOLATION_TABLE)
        gpu_ctx.synchronize()
        assert np.array_equal(got[0::2].view(np.uint64), clean.cpu().numpy()[0::2].view(np.uint64))
        assert (got[0::2] < 0.9).all() and (got[1::2] >= 1.0).all()


def test_float_frames_outside_a_segment_are_not_read_not_even_as_history(gpu_ctx):
    x = (signal(ISOLATION_TOTAL, 3, seed=4) * 0.5).astype(np.float32)
    dirty = x.copy()
    dirty[:, isolation_mask()] = np.nan
    for layout, channels in (("planar", 1), ("interleaved", 2), ("padded", 3)):
        peaks, reports = gpu_ctx.true_peak_float(float_source(gpu_ctx, dirty[:channels], layout), FS, seg_first_frame=ISOLATION_TABLE)
        clean, _ = gpu_ctx.true_peak_float(float_source(gpu_ctx, x[:channels], layout), FS, seg_first_frame=ISOLATION_TABLE)
        gpu_ctx.synchronize()
        values, bad = lr.float_values(dirty[:channels])
        got = check(peaks, reports, values, FS, ISOLATION_TABLE, bad, what="float isolation " + layout)
        assert np.array_equal(got[0::2].view(np.uint64), clean.cpu().numpy()[0::2].view(np.uint64))
        reps = alac_amd.Context.true_peak_reports(reports)
        assert [r.nonfinite for r in reps[0::2]] == [0] * 5 and [r.nonfinite for r in reps[1::2]] == [(K + 5) * channels] * 4


# ---- sources ---------------------------------------------------------------------------------------------------------------
FRAMES = 5 * R + 17

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
    table = [0, 2 * R + 3, FRAMES]
    peaks, reports = gpu_ctx.true_peak_int(t, FS, bits=bits, left_justified=bool(lj), seg_first_frame=table, **kw)
    gpu_ctx.synchronize()
    check(peaks, reports, lr.int_values(v, bits, lj, 8 * cb), FS, table, what=str((cb, bits, lj, layout, channels, offset)))


FLOAT_CASES = [("planar", 1, 0), ("planar", 2, 0), ("interleaved", 2, 0), ("padded", 2, 0), ("planar", 2, 1), ("interleaved", 2, 1),
               ("padded", 3, 0), ("interleaved", 6, 0), ("planar", 8, 0)]


@pytest.mark.parametrize("layout,channels,offset", FLOAT_CASES)
def test_float_sources(gpu_ctx, layout, channels, offset):
    x = (signal(FRAMES, channels, seed=channels) * 1.5).astype(np.float32)  # over full scale: floats are not clipped
    table = [0, 2 * R + 3, FRAMES]
    peaks, reports = gpu_ctx.true_peak_float(float_source(gpu_ctx, x, layout, offset), FS, seg_first_frame=table)
    gpu_ctx.synchronize()
    check(peaks, reports, x.astype(np.float64), FS, table, np.zeros(x.shape, bool), what=str((layout, channels, offset)))


def test_non_finite_floats_are_counted_and_read_as_zero(gpu_ctx):
    x = (signal(FRAMES, 2, seed=9) * 0.7).astype(np.float32)
    x[0, [3, R - 1, R]] = [np.nan, np.inf, -np.inf]
    x[1, [0, FRAMES - 1]] = [-np.inf, np.nan]
    x[1, 50] = np.float32(1e-42)  # a denormal is finite
    table = [0, R + 20, R + 20, FRAMES]
    values, bad = lr.float_values(x)
    for layout in ("planar", "interleaved", "padded"):
        peaks, reports = gpu_ctx.true_peak_float(float_source(gpu_ctx, x, layout), FS, seg_first_frame=table)
        gpu_ctx.synchronize()
        check(peaks, reports, values, FS, table, bad, what="non-finite " + layout)
        assert [r.nonfinite for r in alac_amd.Context.true_peak_reports(reports)] == [4, 0, 1]


@pytest.mark.parametrize("fs", [44100, 48000, 96000, 192000])
def test_rates(gpu_ctx, fs):
    F, coefs = alac_amd.true_peak_filter(fs)
    run = TRUE_PEAK_RUN[F]
    frames = 257 * run + 3
    s = quantise(signal(frames, 3, fs, seed=fs), 16)
    x = s.astype(np.float64) * 2.0 ** -15
    table = [1, 64 * run + 1, 64 * run + 2, frames - 2]
    for channels in (1, 2, 3):
        src = int16_interleaved(gpu_ctx, s[:2]) if channels == 2 else int16_planar(gpu_ctx, s[:channels])
        peaks, reports = gpu_ctx.true_peak_int(src, fs, seg_first_frame=table)
        gpu_ctx.synchronize()
        got = check(peaks, reports, x[:channels], fs, table, what="rate %d channels %d" % (fs, channels))
        if F == 1:
            for r, g in zip(alac_amd.Context.true_peak_reports(reports), got):
                assert r.true_peak == r.peak == g.max()


# ---- determinism -----------------------------------------------------------------------------------------------------------
def raw_words(peaks, reports):
    return peaks.cpu().numpy().view(np.uint64), reports.cpu().numpy().view(np.uint32)


def test_a_segment_gives_the_same_bits_wherever_it_lies(gpu_ctx):
    n = 70 * R + 11
    s = quantise(signal(n, 2, seed=31), 16)
    alone = raw_words(*gpu_ctx.true_peak_int(int16_planar(gpu_ctx, s), FS))
    # as the 3rd of 7 segments, at an odd offset, between segments of other sizes
    other = quantise(signal(9000, 2, seed=32), 16)
    sizes = [R + 1, 2 * R + 7, n, 0, 3 * R, 5, R - 1]
    parts, at = [], 3
    table = [at]
    for i, size in enumerate(sizes):
        parts.append(s if i == 2 else other[:, 100 * i:100 * i + size])
        at += size
        table.append(at)
    buf = np.concatenate([other[:, :3]] + parts + [other[:, :50]], axis=1)
    p7, r7 = raw_words(*gpu_ctx.true_peak_int(int16_planar(gpu_ctx, buf), FS, seg_first_frame=table))
    assert np.array_equal(p7[2], alone[0][0]) and np.array_equal(r7[2], alone[1][0])
    # at a different offset in a larger buffer
    big = np.concatenate([other[:, :1001], s, other[:, :7]], axis=1)
    where = [1001, 1001 + n]
    p1, r1 = raw_words(*gpu_ctx.true_peak_int(int16_planar(gpu_ctx, big), FS, seg_first_frame=where))
    assert np.array_equal(p1, alone[0]) and np.array_equal(r1, alone[1])
    # ... interleaved at a base off the vector alignment: the general layout, one lane per run and channel
    t, _ = int_source(gpu_ctx, big, 2, "interleaved", offset=1)
    p2, r2 = raw_words(*gpu_ctx.true_peak_int(t, FS, seg_first_frame=where))
    assert np.array_equal(p2, alone[0]) and np.array_equal(r2, alone[1])
    # ... interleaved at an aligned base: staged through LDS (planar stereo above is not)
    t, _ = int_source(gpu_ctx, big, 2, "interleaved")
    p3, r3 = raw_words(*gpu_ctx.true_peak_int(t, FS, seg_first_frame=where))
    assert np.array_equal(p3, alone[0]) and np.array_equal(r3, alone[1])
    # ... and with any strides
    buf32 = np.zeros((2, 3 * big.shape[1] + 5), np.int16)
    buf32[:, ::3][:, :big.shape[1]] = big
    t = torch.from_numpy(buf32).to(gpu_ctx.device)[:, ::3][:, :big.shape[1]]
    p4, r4 = raw_words(*gpu_ctx.true_peak_int(t, FS, seg_first_frame=where))
    assert np.array_equal(p4, alone[0]) and np.array_equal(r4, alone[1])
    gpu_ctx.synchronize()


def call_int(gpu_ctx, x, fs, table, peaks, reports, ws=None, ws_bytes=None, src=None, channels=None, frames=None, d_in=True):
    """alac_hip_true_peak_int itself, into the caller's tensors"""
    lib = gpu_ctx.lib
    channels = x.shape[0] if channels is None else channels
    frames = x.shape[1] if frames is None else frames
    src = alac_amd.IntSource(2, 16, 1, 0, x.stride(0), x.stride(1)) if src is None else src
    tab = None if table is None else np.ascontiguousarray(table, dtype=np.uint64)
    nseg = 1 if tab is None else tab.size - 1
    if ws is None:
        ws = torch.empty(int(lib.alac_hip_true_peak_workspace_bytes(channels, nseg)), dtype=torch.uint8, device=gpu_ctx.device)
    torch.cuda.synchronize()
    return lib.alac_hip_true_peak_int(gpu_ctx.h, x.data_ptr() if d_in else None, C.byref(src) if src is not False else None, channels,
                                      fs, frames, None if tab is None else tab.ctypes.data, nseg,
                                      ws.data_ptr() if ws is not False else None, ws.numel() if ws_bytes is None else ws_bytes,
                                      peaks.data_ptr() if peaks is not False else None,
                                      reports.data_ptr() if reports is not False else None)


def test_a_second_call_into_the_same_buffers_does_not_accumulate(gpu_ctx):
    n = 6 * R + 5
    loud = int16_planar(gpu_ctx, quantise(signal(n, 2, seed=41), 16))
    quiet = int16_planar(gpu_ctx, quantise(signal(n, 2, seed=41) * 0.01, 16))
    table = [0, 2 * R + 3, n]
    peaks = torch.full((2, 2), 7.0, dtype=torch.float64, device=gpu_ctx.device)
    reports = torch.full((2, 8), -1, dtype=torch.int32, device=gpu_ctx.device)
    assert call_int(gpu_ctx, loud, FS, table, peaks, reports) == 0
    assert call_int(gpu_ctx, quiet, FS, table, peaks, reports) == 0
    gpu_ctx.synchronize()
    second = raw_words(peaks, reports)
    fresh = raw_words(*gpu_ctx.true_peak_int(quiet, FS, seg_first_frame=table))
    assert np.array_equal(second[0], fresh[0]) and np.array_equal(second[1], fresh[1])
    assert float(peaks.max()) < 0.05


# ---- composition with the decoder -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [16, 24])
def test_decode_then_true_peak_equals_true_peak_of_the_source(gpu_ctx, depth):
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
            return gpu_ctx.true_peak_int(buf.view(torch.int16).view(n * 4096, 2).t(), 44100)
        return gpu_ctx.true_peak_int(buf, 44100, bits=24, container_bytes=3, num_channels=2, channel_stride=1, frame_stride=2)

    src, dec = raw_words(*measure(d_pcm)), raw_words(*measure(out))
    assert src[0].shape == (1, 2) and np.array_equal(src[0], dec[0]) and np.array_equal(src[1], dec[1])
    assert src[0].view(np.float64).min() > 0
    if depth == 16:
        f, _, st, _ = gpu_ctx.decode_float(cookie, d_stream, offs, n)
        flt = raw_words(*gpu_ctx.true_peak_float(f, 44100))
        assert np.array_equal(src[0], flt[0]) and np.array_equal(src[1], flt[1])
    gpu_ctx.synchronize()


# ---- host forms -------------------------------------------------------------------------------------------------------------
def test_host_forms_equal_the_device_forms(gpu_ctx):
    n = 4 * R + 77
    s = quantise(signal(n + 100, 2, seed=51), 16).astype(np.int16)
    table = np.array([3, 2 * R + 9, n], dtype=np.uint64)
    lib = gpu_ctx.lib
    dev = raw_words(*gpu_ctx.true_peak_int(torch.from_numpy(s).to(gpu_ctx.device), FS, seg_first_frame=table))
    gpu_ctx.synchronize()
    assert dev[0].shape == (2, 2)
    peaks, reports = np.full((2, 2), 9.0), np.zeros((2, 8), np.uint32)
    src = alac_amd.IntSource(2, 16, 1, 0, s.shape[1], 1)
    assert lib.alac_hip_true_peak_int_host(gpu_ctx.h, s.ctypes.data, C.byref(src), 2, FS, s.shape[1], table.ctypes.data, 2,
                                           peaks.ctypes.data, reports.ctypes.data) == 0
    assert np.array_equal(peaks.view(np.uint64), dev[0]) and np.array_equal(reports, dev[1])
    f = (s.astype(np.float32) / 32768.0)
    f[:, n:] = np.nan  # behind the last segment: not staged, not read
    dev = raw_words(*gpu_ctx.true_peak_float(torch.from_numpy(f).to(gpu_ctx.device), FS, seg_first_frame=table))
    gpu_ctx.synchronize()
    peaks, reports = np.full((2, 2), 9.0), np.zeros((2, 8), np.uint32)
    assert lib.alac_hip_true_peak_float_host(gpu_ctx.h, f.ctypes.data, 2, f.shape[1], 1, FS, f.shape[1], table.ctypes.data, 2,
                                             peaks.ctypes.data, reports.ctypes.data) == 0
    assert np.array_equal(peaks.view(np.uint64), dev[0]) and np.array_equal(reports, dev[1])
    before = peaks.copy(), reports.copy()
    assert lib.alac_hip_true_peak_float_host(gpu_ctx.h, f.ctypes.data, 2, f.shape[1], 1, FS, f.shape[1], table.ctypes.data, 2,
                                             None, reports.ctypes.data) == -50
    assert lib.alac_hip_true_peak_int_host(gpu_ctx.h, s.ctypes.data, C.byref(src), 2, 44101, s.shape[1], table.ctypes.data, 2,
                                           peaks.ctypes.data, reports.ctypes.data) == -50
    assert np.array_equal(peaks, before[0]) and np.array_equal(reports, before[1])


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone(gpu_ctx):
    n = 3 * R
    x = int16_planar(gpu_ctx, quantise(signal(n, 2, seed=61), 16))
    peaks = torch.full((1, 2), 7.0, dtype=torch.float64, device=gpu_ctx.device)
    reports = torch.full((1, 8), -1, dtype=torch.int32, device=gpu_ctx.device)
    ws = torch.zeros(int(gpu_ctx.lib.alac_hip_true_peak_workspace_bytes(2, 2)) + 64, dtype=torch.uint8, device=gpu_ctx.device)
    good = alac_amd.IntSource(2, 16, 1, 0, n, 1)
    assert call_int(gpu_ctx, x, FS, None, peaks, reports, ws=ws) == 0
    gpu_ctx.synchronize()
    assert float(peaks.max()) <= 1.7 and int(reports[0, 6]) == 0
    peaks.fill_(7.0), reports.fill_(-1)
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
        "table not ascending": dict(table=[0, 90, 80]),
        "table behind total_frames": dict(table=[0, n + 1]),
        "null workspace": dict(ws=False, ws_bytes=1 << 20),
        "workspace too small": dict(ws_bytes=int(gpu_ctx.lib.alac_hip_true_peak_workspace_bytes(2, 1)) - 1),
        "misaligned workspace": dict(ws=ws[4:]),
        "null channel peaks": dict(peaks=False),
        "misaligned channel peaks": dict(peaks=peaks.view(torch.uint8)[4:]),
        "null reports": dict(reports=False),
        "misaligned reports": dict(reports=reports.view(torch.uint8)[4:]),
    }
    for name, kw in cases.items():
        args = dict(x=x, fs=FS, table=None, peaks=peaks, reports=reports, ws=ws, src=good)
        args.update(kw)
        rc = call_int(gpu_ctx, **args)
        gpu_ctx.synchronize()
        assert rc == -50, name
        assert bool((peaks == 7.0).all()) and bool((reports == -1).all()), name
    # num_segments 0, and more than one segment without a table
    for nseg in (0, 2):
        rc = gpu_ctx.lib.alac_hip_true_peak_int(gpu_ctx.h, x.data_ptr(), C.byref(good), 2, FS, n, None, nseg, ws.data_ptr(), ws.numel(),
                                                peaks.data_ptr(), reports.data_ptr())
        assert rc == -50
    # the float call: what alac_hip_float_probe refuses, and the same rates
    f = torch.zeros((2, n), dtype=torch.float32, device=gpu_ctx.device)
    lib = gpu_ctx.lib

    def call_float(d_in=f.data_ptr(), channels=2, cs=n, fst=1, fs=FS, frames=n, pk=peaks.data_ptr()):
        return lib.alac_hip_true_peak_float(gpu_ctx.h, d_in, channels, cs, fst, fs, frames, None, 1, ws.data_ptr(), ws.numel(),
                                            pk, reports.data_ptr())

    assert call_float() == 0
    gpu_ctx.synchronize()
    assert float(peaks.max()) == 0.0
    peaks.fill_(7.0), reports.fill_(-1)
    for name, kw in {"null": dict(d_in=None), "misaligned": dict(d_in=f.data_ptr() + 2), "channels": dict(channels=9),
                     "frame_stride": dict(fst=0), "channel_stride": dict(cs=0), "rate": dict(fs=48001), "peaks": dict(pk=None),
                     "overflow": dict(cs=1 << 63, fst=1 << 62)}.items():
        assert call_float(**kw) == -50, name
        gpu_ctx.synchronize()
        assert bool((peaks == 7.0).all()) and bool((reports == -1).all()), name


def test_python_level_refusals(gpu_ctx):
    f = torch.zeros((2, 100), dtype=torch.float32, device=gpu_ctx.device)
    with pytest.raises(ValueError):
        gpu_ctx.true_peak_float(f.double(), FS)
    with pytest.raises(ValueError):
        gpu_ctx.true_peak_float(f[0], FS)
    with pytest.raises(ValueError):
        gpu_ctx.true_peak_float(f.cpu(), FS)
    with pytest.raises(ValueError):
        gpu_ctx.true_peak_float(f, FS, seg_first_frame=[[0, 1], [2, 3]])
    with pytest.raises(ValueError):
        gpu_ctx.true_peak_int(f, FS)
    with pytest.raises(alac_amd.AlacError):
        gpu_ctx.true_peak_float(f, 44101)
