"""GPU: alac_hip_resample_int / alac_hip_resample_float.  The outputs equal the numpy restatement of the rule (resample_ref.py,
with the library's own coefficients, so that no libm bit enters) within a distance that is derived, not measured: the device
and the restatement form the same K products in double and differ in fusing and order only, so a sum moves by at most
    bound = K * 2^-52 * max_p sum_k |h_p[k]| * peak of the segment's samples
and the float32 the device writes is the correctly rounded value of a sum inside that bound:
    |device float - reference double| <= bound + half the float32 spacing at (|reference| + bound)
An impulse gives single products, which are equal as bits.  The reports are exact: out_first and out_frames are those of
alac_hip_resample_frames, nonfinite is the count, peak is the largest |float32| of the device's own output.  A segment gives
the same bits wherever it lies; refusals leave the outputs alone; every call stays inside the workspace its size query reports;
resample, encode_float and decode give the restatement pushed through the quantization rule.
T = 512 output frames is a block's tile at every ratio the tests use."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import alac_amd
import resample_ref as rr
from alac_amd.capi import RESAMPLE_TILE as T
from test_gpu_loudness import int_source
from test_gpu_workspace_bounds import confined, pair, refused  # noqa: F401  (pair: the fixture confined() and refused() use)

pytestmark = pytest.mark.gpu

# L / M = 160/147, 147/160, 2/1, 1/2, 1/4, 147/320, 441/80, 640/147
PAIRS = [(44100, 48000), (48000, 44100), (48000, 96000), (96000, 48000), (192000, 48000), (96000, 44100), (8000, 44100),
         (44100, 192000)]
USED = [0.0]  # the largest share of the accepted distance so far


@functools.lru_cache(maxsize=None)
def filt(rates):
    return alac_amd.resample_filter(*rates)


def check(y, reports, x, rates, table=None, nonfinite=None, what=""):
    """the call's outputs against the restatement on x float64 [channels, frames] (the values of the rule) -> y on the host"""
    L, M, coefs = filt(rates)
    tab = [0, x.shape[1]] if table is None else [int(t) for t in table]
    first = rr.out_table(tab, L, M)
    got = y.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (x.shape[0], first[-1]), (what, got.shape, first[-1])
    total, lib_first = alac_amd.resample_frames(rates[0], rates[1], x.shape[1], None if table is None else tab)
    assert total == first[-1] and list(lib_first) == first, what
    reps = alac_amd.Context.resample_reports(reports)
    assert len(reps) == len(tab) - 1
    for s, r in enumerate(reps):
        seg = x[:, tab[s]:tab[s + 1]]
        ref = rr.segment(seg.T, L, M, coefs).T
        out = got[:, first[s]:first[s + 1]]
        bnd = rr.bound(coefs, np.abs(seg).max() if seg.size else 0.0)
        err, acc = np.abs(out.astype(np.float64) - ref), rr.accepted(ref, bnd)
        share = float((err / acc).max()) if err.size else 0.0
        USED[0] = max(USED[0], share)
        assert (err <= acc).all(), (what, s, share)
        bad = 0 if nonfinite is None else int(nonfinite[:, tab[s]:tab[s + 1]].sum())
        assert (r.out_first, r.out_frames, r.nonfinite) == (first[s], first[s + 1] - first[s], bad), (what, s)
        own = float(np.abs(out).max()) if out.size else 0.0
        assert np.float64(r.peak).view(np.uint64) == np.float64(own).view(np.uint64), (what, s, r.peak, own)
        want_peak = float(np.abs(ref).max()) if ref.size else 0.0
        assert abs(r.peak - want_peak) <= rr.accepted(want_peak, bnd), (what, s)
    print(what, "segments", len(reps), "largest share of the accepted distance so far", USED[0])
    return got


# ---- sources ----------------------------------------------------------------------------------------------------------------
def noise(frames, channels, seed, scale=0.9):
    return np.random.default_rng(seed).uniform(-scale, scale, (channels, frames))


def make_source(gpu_ctx, name, frames, seed):
    """-> (call(rates, table) -> (y, reports), x float64 [channels, frames]: the values of the rule)"""
    if name in ("float contiguous", "float transposed"):
        f = noise(frames, 2, seed, 1.5).astype(np.float32)  # over full scale: floats are not clipped
        t = torch.from_numpy(f).to(gpu_ctx.device) if name == "float contiguous" else \
            torch.from_numpy(np.ascontiguousarray(f.T)).to(gpu_ctx.device).t()
        return (lambda rates, table: gpu_ctx.resample_float(t, rates[0], rates[1], seg_first_frame=table)), f.astype(np.float64)
    channels, cb, bits, layout, shift = {"int16 interleaved stereo": (2, 2, 16, "interleaved", 0),
                                         "int32 planar 24 bits left-justified": (2, 4, 24, "planar", 8),
                                         "packed 3-byte mono": (1, 3, 24, "planar", 0),
                                         "int32 general 3 channels": (3, 4, 32, "planar", 0)}[name]
    s = np.rint(noise(frames, channels, seed) * 2.0 ** (bits - 1)).astype(np.int64)
    t, kw = int_source(gpu_ctx, s << shift, cb, layout)
    return (lambda rates, table: gpu_ctx.resample_int(t, rates[0], rates[1], bits=bits, seg_first_frame=table, **kw)), \
        s.astype(np.float64) * 2.0 ** -(bits - 1)


SOURCES = ["int16 interleaved stereo", "int32 planar 24 bits left-justified", "packed 3-byte mono", "int32 general 3 channels",
           "float contiguous", "float transposed"]


def lengths(rates):
    """segment lengths in input frames: 1, K/2 - 1, K/2, K, K + 1, one frame into a third tile, and those around a tile's
    edge: the shortest ones that give T - 1, T and T + 1 output frames or the next count above (going up, not every count
    exists), and the centre frame of the second tile's first output with its neighbours"""
    L, M, coefs = filt(rates)
    K = coefs.shape[1]
    edge = T * M // L
    around = {edge - 1, edge, edge + 1} | {(o - 1) * M // L + 1 for o in (T - 1, T, T + 1)}
    return [1, K // 2 - 1, K // 2, K, K + 1, 2 * T * M // L + 1] + sorted(around)


# ---- noise, every source and ratio --------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("rates", PAIRS)
def test_noise_against_the_accepted_distance(gpu_ctx, rates, source):
    L, M, _ = filt(rates)
    sizes = lengths(rates)
    outs = [rr.out_frames(n, L, M) for n in sizes]
    assert min(outs[6:]) <= T < max(outs[6:]) and outs[5] > 2 * T  # the tile's edge is crossed
    table = np.concatenate([[0], np.cumsum(sizes)])
    call, x = make_source(gpu_ctx, source, int(table[-1]), seed=L * 1000 + M)
    y, reports = call(rates, table)
    gpu_ctx.synchronize()
    check(y, reports, x, rates, table, np.zeros(x.shape, bool), what="%s %d/%d table" % (source, L, M))
    # one segment without a table: the longest length
    call, x = make_source(gpu_ctx, source, sizes[5], seed=L * 1000 + M + 1)
    y, reports = call(rates, None)
    gpu_ctx.synchronize()
    check(y, reports, x, rates, None, np.zeros(x.shape, bool), what="%s %d/%d one segment" % (source, L, M))


# ---- impulse: single products, equal as bits -------------------------------------------------------------------------------
@pytest.mark.parametrize("rates", PAIRS[:4])
def test_an_impulse_gives_the_coefficients_as_bits(gpu_ctx, rates):
    L, M, coefs = filt(rates)
    K = coefs.shape[1]
    edge = T * M // L  # the centre frame of the second tile's first output, or the frame in front of it
    n = 2 * edge + 7
    for at in (0, n - 1, edge - 1, edge, edge + 1):
        x = np.zeros((2, n), np.float32)
        x[0, at] = 1.0
        x[1, n - 1 - at] = 1.0
        outs = rr.out_frames(n, L, M)
        m = np.arange(outs, dtype=np.int64)
        n0, p = m * M // L, m * M % L
        want = np.zeros((2, outs), np.float32)
        for c, pos in ((0, at), (1, n - 1 - at)):
            k = n0 + K // 2 - pos
            hit = (k >= 0) & (k < K)
            want[c, hit] = coefs[p[hit], k[hit]].astype(np.float32)
        for t in (torch.from_numpy(x).to(gpu_ctx.device), torch.from_numpy(np.ascontiguousarray(x.T)).to(gpu_ctx.device).t(),
                  torch.from_numpy(x[:1]).to(gpu_ctx.device)):
            y, reports = gpu_ctx.resample_float(t, rates[0], rates[1])
            gpu_ctx.synchronize()
            got = y.cpu().numpy()
            assert np.array_equal(got.view(np.uint32), want[:t.shape[0]].view(np.uint32)), (rates, at, tuple(t.stride()))
            r = alac_amd.Context.resample_reports(reports)[0]
            assert r.peak == float(np.abs(want[:t.shape[0]]).max()) and r.nonfinite == 0 and r.out_frames == outs


# ---- the same bits wherever a segment lies -------------------------------------------------------------------------------
def raw_call(gpu_ctx, x, rates, table, y, stride, out_frames, reports, ws=None, ws_bytes=None, src=None, channels=2, frames=None):
    """alac_hip_resample_int on an int16 tensor [2, frames] (planar) with every argument in the caller's hand; False: a null
    pointer"""
    lib = gpu_ctx.lib
    tab = None if table is None else np.ascontiguousarray(table, dtype=np.uint64)
    nseg = 1 if tab is None else tab.size - 1
    if ws is None:
        ws = gpu_ctx._workspace(int(lib.alac_hip_resample_workspace_bytes(rates[0], rates[1], 2, max(1, nseg))) or 4096)
    if src is None:
        src = alac_amd.IntSource(2, 16, 1, 0, int(x.stride(0)), int(x.stride(1)))
    return lib.alac_hip_resample_int(gpu_ctx.h, x.data_ptr() if x is not False else None, C.byref(src) if src is not False else None,
                                     channels, rates[0], rates[1], int(x.shape[1]) if frames is None else frames,
                                     None if tab is None else tab.ctypes.data, nseg,
                                     ws.data_ptr() if ws is not False else None, ws.numel() if ws_bytes is None else ws_bytes,
                                     y.data_ptr() if y is not False else None, stride, out_frames,
                                     reports.data_ptr() if reports is not False else None)


@pytest.mark.parametrize("rates", [(44100, 48000), (96000, 44100)])
def test_a_segment_gives_the_same_bits_wherever_it_lies(gpu_ctx, rates):
    L, M, _ = filt(rates)
    big = 2 * T * M // L + 13
    table = np.array([3, 3, 3 + big, 4 + big, 4 + big, 4 + big + 777], dtype=np.uint64)  # two empty ones, one of 1 frame
    total_in = int(table[-1]) + 11
    first = rr.out_table(table, L, M)
    for source in ("int16 interleaved stereo", "int32 general 3 channels"):
        channels, bits = (2, 16) if source.startswith("int16") else (3, 32)
        s = np.rint(noise(total_in, channels, 77) * 2.0 ** (bits - 1)).astype(np.int64)

        def run(v, tab):
            t, kw = int_source(gpu_ctx, v, bits // 8, "interleaved" if channels == 2 else "planar")
            y, rep = gpu_ctx.resample_int(t, rates[0], rates[1], bits=bits, seg_first_frame=tab, **kw)
            gpu_ctx.synchronize()
            return y.cpu().numpy(), alac_amd.Context.resample_reports(rep)

        whole, reps = run(s, table)
        check(torch.from_numpy(whole), torch.from_numpy(np.frombuffer(b"".join(bytes(r) for r in reps), np.int32).reshape(-1, 8).copy()),
              s.astype(np.float64) * 2.0 ** -(bits - 1), rates, table, what="five segments " + source)
        for i in range(5):
            a, b = int(table[i]), int(table[i + 1])
            alone, r1 = run(s[:, a:b], None)
            assert np.array_equal(alone.view(np.uint32), whole[:, first[i]:first[i + 1]].view(np.uint32)), (source, i)
            assert (r1[0].out_first, r1[0].out_frames) == (0, first[i + 1] - first[i]) == (0, reps[i].out_frames)
            assert (r1[0].peak, r1[0].nonfinite) == (reps[i].peak, reps[i].nonfinite), (source, i)
        assert reps[0].out_frames == reps[3].out_frames == 0 and reps[0].peak == 0.0 and reps[2].out_frames == -(-L // M)
    # the whole again with rows further apart than out_frames: the same bits, and nothing behind the rows' frames is written
    s = np.rint(noise(total_in, 2, 77) * 2.0 ** 15).astype(np.int16)
    x = torch.from_numpy(s).to(gpu_ctx.device)
    want, _ = gpu_ctx.resample_int(x, rates[0], rates[1], seg_first_frame=table)
    total = first[-1]
    out_frames, stride = total + 5, total + 37
    y = torch.full((2 * stride + 9,), -7.25, dtype=torch.float32, device=gpu_ctx.device)
    reports = torch.full((5, 8), -1, dtype=torch.int32, device=gpu_ctx.device)
    assert raw_call(gpu_ctx, x, rates, table, y, stride, out_frames, reports) == 0
    gpu_ctx.synchronize()
    got, want = y.cpu().numpy(), want.cpu().numpy()
    rows = np.stack([got[:total], got[stride:stride + total]])
    assert np.array_equal(rows.view(np.uint32), want.view(np.uint32))
    assert (got[total:stride] == -7.25).all() and (got[stride + total:] == -7.25).all()
    assert [r.out_first for r in alac_amd.Context.resample_reports(reports)] == first[:-1]


# ---- non-finite floats, DC ---------------------------------------------------------------------------------------------------
def test_non_finite_floats_are_counted_and_read_as_zero(gpu_ctx):
    rates = (44100, 48000)
    n = 3 * T
    x = noise(n, 2, 9, 0.7).astype(np.float32)
    x[0, [3, 900, 901]] = [np.nan, np.inf, -np.inf]
    x[1, [0, n - 1, T * 147 // 160, T * 147 // 160 + 1]] = [-np.inf, np.nan, np.inf, np.nan]  # ... and around a tile's edge
    x[1, 50] = np.float32(1e-42)  # a denormal is finite
    table = [0, 850, 850, n]
    bad = ~np.isfinite(x)
    values = np.where(bad, 0.0, x.astype(np.float64))
    for t in (torch.from_numpy(x).to(gpu_ctx.device), torch.from_numpy(np.ascontiguousarray(x.T)).to(gpu_ctx.device).t()):
        y, reports = gpu_ctx.resample_float(t, rates[0], rates[1], seg_first_frame=table)
        gpu_ctx.synchronize()
        got = check(y, reports, values, rates, table, bad, what="non-finite")
        assert np.isfinite(got).all()
        assert [r.nonfinite for r in alac_amd.Context.resample_reports(reports)] == [4, 0, 3]  # frames 0, 3, 470, 471; 900, 901, n - 1


@pytest.mark.parametrize("rates", [(44100, 48000), (96000, 44100)])
def test_dc_stays_dc_away_from_the_ends(gpu_ctx, rates):
    L, M, coefs = filt(rates)
    K = coefs.shape[1]
    n = 2 * T * M // L + 2 * K
    x = torch.full((1, n), 0.5, dtype=torch.float32, device=gpu_ctx.device)
    y, _ = gpu_ctx.resample_float(x, rates[0], rates[1])
    gpu_ctx.synchronize()
    got = y.cpu().numpy()[0].astype(np.float64)
    m = np.arange(got.size, dtype=np.int64)
    n0 = m * M // L
    inner = (n0 - K // 2 + 1 >= 0) & (n0 + K // 2 < n)  # every tap lies inside the segment
    assert inner.sum() > T
    ripple = 0.5 * float(np.abs(coefs.sum(axis=1) - 1.0).max())
    bnd = rr.bound(coefs, 0.5)
    assert (np.abs(got[inner] - 0.5) <= ripple + rr.accepted(0.5, bnd)).all()
    assert ripple < 2e-6


# ---- host forms --------------------------------------------------------------------------------------------------------------
def test_host_forms_equal_the_device_forms(gpu_ctx):
    rates = (96000, 44100)
    L, M, _ = filt(rates)
    n = 2500
    s = np.rint(noise(n + 100, 2, 51) * 2.0 ** 15).astype(np.int16)
    table = np.array([3, 1209, 1209, n], dtype=np.uint64)
    total, first = alac_amd.resample_frames(rates[0], rates[1], s.shape[1], table)
    lib = gpu_ctx.lib
    y, rep = gpu_ctx.resample_int(torch.from_numpy(s).to(gpu_ctx.device), rates[0], rates[1], seg_first_frame=table)
    gpu_ctx.synchronize()
    dev = y.cpu().numpy(), rep.cpu().numpy()
    stride = total + 3
    out, reports = np.full((2, stride), 9.0, np.float32), np.zeros((3, 8), np.int32)
    src = alac_amd.IntSource(2, 16, 1, 0, s.shape[1], 1)
    assert lib.alac_hip_resample_int_host(gpu_ctx.h, s.ctypes.data, C.byref(src), 2, rates[0], rates[1], s.shape[1],
                                          table.ctypes.data, 3, out.ctypes.data, stride, total, reports.ctypes.data) == 0
    assert np.array_equal(out[:, :total].view(np.uint32), dev[0].view(np.uint32)) and np.array_equal(reports, dev[1])
    assert (out[:, total:] == 9.0).all()
    f = (s.astype(np.float32) / 32768.0)
    f[:, n:] = np.nan  # behind the last segment: not staged, not read
    y, rep = gpu_ctx.resample_float(torch.from_numpy(f).to(gpu_ctx.device), rates[0], rates[1], seg_first_frame=table)
    gpu_ctx.synchronize()
    assert np.array_equal(y.cpu().numpy().view(np.uint32), dev[0].view(np.uint32))  # the same values, the same bits
    out, reports = np.full((2, stride), 9.0, np.float32), np.zeros((3, 8), np.int32)
    assert lib.alac_hip_resample_float_host(gpu_ctx.h, f.ctypes.data, 2, f.shape[1], 1, rates[0], rates[1], f.shape[1],
                                            table.ctypes.data, 3, out.ctypes.data, stride, total, reports.ctypes.data) == 0
    assert np.array_equal(out[:, :total].view(np.uint32), dev[0].view(np.uint32)) and np.array_equal(reports, dev[1])
    before = out.copy(), reports.copy()
    for kw in (dict(o=None), dict(r=None), dict(rate=44101), dict(frames=total - 1), dict(st=total - 1)):
        a = dict(o=out.ctypes.data, r=reports.ctypes.data, rate=rates[1], frames=total, st=stride)
        a.update(kw)
        assert lib.alac_hip_resample_float_host(gpu_ctx.h, f.ctypes.data, 2, f.shape[1], 1, rates[0], a["rate"], f.shape[1],
                                                table.ctypes.data, 3, a["o"], a["st"], a["frames"], a["r"]) == -50, kw
    assert np.array_equal(out, before[0]) and np.array_equal(reports, before[1])


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone(gpu_ctx):
    rates = (44100, 48000)
    n = 1000
    total = rr.out_frames(n, 160, 147)
    x = torch.from_numpy(np.rint(noise(n, 2, 61) * 2.0 ** 15).astype(np.int16)).to(gpu_ctx.device)
    y = torch.full((2 * total,), 7.0, dtype=torch.float32, device=gpu_ctx.device)
    reports = torch.full((1, 8), -1, dtype=torch.int32, device=gpu_ctx.device)
    need = int(gpu_ctx.lib.alac_hip_resample_workspace_bytes(rates[0], rates[1], 2, 2))
    ws = torch.zeros(need + 64, dtype=torch.uint8, device=gpu_ctx.device)
    good = alac_amd.IntSource(2, 16, 1, 0, n, 1)
    assert raw_call(gpu_ctx, x, rates, None, y, total, total, reports, ws=ws) == 0
    gpu_ctx.synchronize()
    assert float(y.abs().max()) <= 2.0 and alac_amd.Context.resample_reports(reports)[0].out_frames == total
    y.fill_(7.0), reports.fill_(-1)
    S = alac_amd.IntSource
    cases = {
        "null d_in": dict(x=False, frames=n, src=good),
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
        "in rate not a multiple of 10": dict(rates=(44101, 48000)),
        "out rate too low": dict(rates=(44100, 7990)),
        "out rate too high": dict(rates=(44100, 384010)),
        "equal rates": dict(rates=(44100, 44100)),
        "L above 640": dict(rates=(22050, 384000)),
        "M above 640": dict(rates=(384000, 11030)),
        "table not ascending": dict(table=[0, 90, 80]),
        "table behind total_frames": dict(table=[0, n + 1]),
        "null workspace": dict(ws=False, ws_bytes=1 << 20),
        "workspace too small": dict(ws_bytes=int(gpu_ctx.lib.alac_hip_resample_workspace_bytes(rates[0], rates[1], 2, 1)) - 1),
        "misaligned workspace": dict(ws=ws[8:]),
        "null d_out": dict(y=False),
        "misaligned d_out": dict(y=y.view(torch.uint8)[2:]),
        "out_frames too short": dict(out_frames=total - 1, stride=total),
        "out_channel_stride below out_frames": dict(out_frames=total, stride=total - 1),
        "null reports": dict(reports=False),
        "misaligned reports": dict(reports=reports.view(torch.uint8)[4:]),
    }
    for name, kw in cases.items():
        args = dict(x=x, rates=rates, table=None, y=y, stride=total, out_frames=total, reports=reports, ws=ws, src=good)
        args.update(kw)
        rc = raw_call(gpu_ctx, **args)
        gpu_ctx.synchronize()
        assert rc == -50, name
        assert bool((y == 7.0).all()) and bool((reports == -1).all()), name
    # num_segments 0, and more than one segment without a table
    for nseg in (0, 2):
        rc = gpu_ctx.lib.alac_hip_resample_int(gpu_ctx.h, x.data_ptr(), C.byref(good), 2, rates[0], rates[1], n, None, nseg,
                                               ws.data_ptr(), ws.numel(), y.data_ptr(), total, total, reports.data_ptr())
        assert rc == -50
    # the float call: what alac_hip_float_probe refuses, and the same rates and outputs
    f = torch.zeros((2, n), dtype=torch.float32, device=gpu_ctx.device)
    lib = gpu_ctx.lib

    def call_float(d_in=f.data_ptr(), channels=2, cs=n, fst=1, out_rate=48000, frames=n, out=y.data_ptr(), room=total):
        return lib.alac_hip_resample_float(gpu_ctx.h, d_in, channels, cs, fst, 44100, out_rate, frames, None, 1, ws.data_ptr(),
                                           ws.numel(), out, total, room, reports.data_ptr())

    assert call_float() == 0
    gpu_ctx.synchronize()
    assert float(y.abs().max()) == 0.0
    y.fill_(7.0), reports.fill_(-1)
    for name, kw in {"null": dict(d_in=None), "misaligned": dict(d_in=f.data_ptr() + 2), "channels": dict(channels=9),
                     "frame_stride": dict(fst=0), "channel_stride": dict(cs=0), "rate": dict(out_rate=48001),
                     "equal": dict(out_rate=44100), "out": dict(out=None), "room": dict(room=total - 1),
                     "overflow": dict(cs=1 << 63, fst=1 << 62)}.items():
        assert call_float(**kw) == -50, name
        gpu_ctx.synchronize()
        assert bool((y == 7.0).all()) and bool((reports == -1).all()), name


def test_python_level_refusals(gpu_ctx):
    f = torch.zeros((2, 100), dtype=torch.float32, device=gpu_ctx.device)
    with pytest.raises(ValueError):
        gpu_ctx.resample_float(f.double(), 44100, 48000)
    with pytest.raises(ValueError):
        gpu_ctx.resample_float(f[0], 44100, 48000)
    with pytest.raises(ValueError):
        gpu_ctx.resample_float(f.cpu(), 44100, 48000)
    with pytest.raises(ValueError):
        gpu_ctx.resample_float(f, 44100, 48000, seg_first_frame=[[0, 1], [2, 3]])
    with pytest.raises(ValueError):
        gpu_ctx.resample_int(f, 44100, 48000)
    with pytest.raises(alac_amd.AlacError):
        gpu_ctx.resample_float(f, 44100, 44100)


def test_a_second_call_into_the_same_buffers_does_not_accumulate(gpu_ctx):
    rates = (48000, 44100)
    n = 1500
    loud = torch.from_numpy(np.rint(noise(n, 2, 41) * 2.0 ** 15).astype(np.int16)).to(gpu_ctx.device)
    quiet = torch.from_numpy(np.rint(noise(n, 2, 41, 0.01) * 2.0 ** 15).astype(np.int16)).to(gpu_ctx.device)
    table = [0, 700, n]
    total, _ = alac_amd.resample_frames(rates[0], rates[1], n, table)
    y = torch.full((2 * total,), 7.0, dtype=torch.float32, device=gpu_ctx.device)
    reports = torch.full((2, 8), -1, dtype=torch.int32, device=gpu_ctx.device)
    assert raw_call(gpu_ctx, loud, rates, table, y, total, total, reports) == 0
    assert raw_call(gpu_ctx, quiet, rates, table, y, total, total, reports) == 0
    gpu_ctx.synchronize()
    fresh, rep = gpu_ctx.resample_int(quiet, rates[0], rates[1], seg_first_frame=table)
    gpu_ctx.synchronize()
    assert np.array_equal(y.cpu().numpy().view(np.uint32), fresh.cpu().numpy().reshape(-1).view(np.uint32))
    assert np.array_equal(reports.cpu().numpy(), rep.cpu().numpy())
    assert max(r.peak for r in alac_amd.Context.resample_reports(reports)) < 0.05


# ---- the workspace -----------------------------------------------------------------------------------------------------------
def resample_call(nseg, rates, kind, per=700):
    def call(c):
        rng = np.random.default_rng(nseg)
        table = np.arange(nseg + 1, dtype=np.uint64) * per
        if kind == "float":
            x = torch.from_numpy((rng.integers(-30000, 30000, (2, nseg * per)) / 32768.0).astype(np.float32)).cuda()
            y, rep = c.resample_float(x, rates[0], rates[1], seg_first_frame=table)
        else:
            x = torch.from_numpy(rng.integers(-30000, 30000, (nseg * per, 2)).astype(np.int16)).cuda().t()
            y, rep = c.resample_int(x, rates[0], rates[1], seg_first_frame=table)
        c.synchronize()
        return [y.cpu().numpy(), rep.cpu().numpy()]
    return call


@pytest.mark.parametrize("kind", ["int", "float"])
@pytest.mark.parametrize("nseg,rates", [(1, (44100, 48000)), (9, (96000, 44100)), (10, (44100, 48000))])
def test_inside_exactly_the_workspace_the_query_reports(pair, nseg, rates, kind):
    """3 (n + 1) x 8 bytes of tables: 9 segments leave 16 bytes of their 256 free, 10 begin the next 256; then the coefficients.
    The leftovers are those of a call with more segments and a larger filter."""
    out = confined(pair, resample_call(nseg, rates, kind), resample_call(21, (96000, 44100), kind) if nseg == 10 else None)
    L, M, _ = filt(rates)
    assert out[0].shape == (2, nseg * rr.out_frames(700, L, M)) and float(np.abs(out[0]).max()) > 0.5


@pytest.mark.parametrize("kind", ["int", "float"])
def test_the_reported_size_minus_one_is_refused(pair, kind):
    refused(pair[0], resample_call(3, (44100, 48000), kind))


# ---- end to end: resample, encode_float, decode --------------------------------------------------------------------------
# (rates, depth, seed, amplitude): exactly one sample of the restatement lies within the accepted distance of a rounding
# boundary (counted on the CPU when the seeds were chosen; the accepted distance is 2^-10 of a 16-bit step at -30 dBFS and
# 2^-13 of a 24-bit step at -60 dBFS, so louder signals have more of them)
END_TO_END = [((44100, 48000), 16, 3, 0.03), ((96000, 44100), 24, 2, 0.001)]


@pytest.mark.parametrize("rates,depth,seed,scale", END_TO_END)
def test_resample_encode_decode_equals_the_restatement_quantized(gpu_ctx, rates, depth, seed, scale):
    L, M, coefs = filt(rates)
    n = 3000
    bits = 16 if depth == 16 else 24
    s = np.rint(noise(n, 2, seed, scale) * 2.0 ** (bits - 1)).astype(np.int64)
    x = s.astype(np.float64) * 2.0 ** -(bits - 1)
    ref = rr.segment(x.T, L, M, coefs).T
    bnd = rr.bound(coefs, np.abs(x).max())
    excused = rr.near_boundary(ref, bnd, depth)
    print("samples near a rounding boundary:", int(excused.sum()), "of", excused.size)
    assert int(excused.sum()) <= 1
    t, kw = int_source(gpu_ctx, s << (32 - bits) if bits == 24 else s, 2 if bits == 16 else 4, "interleaved")
    y, reports = gpu_ctx.resample_int(t, rates[0], rates[1], bits=bits, **kw)
    fmt = alac_amd.make_format(4096, depth, 2, rates[1])
    bufs = gpu_ctx.encode_float(fmt, y, clipped=True)
    gpu_ctx.synchronize()
    check(y, reports, x, rates, what="end to end")
    frames = ref.shape[1]
    packets = -(-frames // 4096)
    assert int(bufs["clipped"].sum()) == 0
    total = int(bufs["offsets"][-1].item())
    f, ns, st, got_fmt = gpu_ctx.decode_float(gpu_ctx.magic_cookie(fmt), bufs["out"][:total], bufs["offsets"], packets)
    gpu_ctx.synchronize()
    assert int(st.abs().sum()) == 0 and int(ns.sum()) == frames and got_fmt.sample_rate == rates[1]
    got = np.rint(f.cpu().numpy()[:, :frames].astype(np.float64) * 2.0 ** (depth - 1)).astype(np.int64)
    want = rr.quantize(ref.astype(np.float32), depth)
    assert np.array_equal(got[~excused], want[~excused])
    assert np.abs(got - want).max() <= 1
