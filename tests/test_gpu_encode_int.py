"""GPU: alac_hip_pcm_requantize / alac_hip_encode_int (Context.requantize, Context.encode_int), their host forms and
ALACEncoder::EncodeSegmentsInt.  The requantized PCM and the per-packet clipped counts must equal, byte for byte, what the
numpy restatement of the integer rule of include/alac_hip.h gives (tests/pcm_requant_ref.py), over every container, both
justifications, all 16 (S, b) pairs with and without dither, every kernel path (1 / 2 channels planar and interleaved, 3 / 6
channels, frame sizes 4096, 1028 and 17, a misaligned base, a wide channel stride, a transposed view), short packets and odd
packet origins; encode_int's bytes must equal encode() of that PCM.  Every case is 3 packets; every input holds random
samples, all kinds of ties, both extremes and, right-justified, containers outside the range, and behind a packet's count
the largest containers there are, which would clip and leave non-zero bytes if they were read."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import alac_amd
import pcm_requant_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
NP = 3
SOURCES = [(2, 16), (3, 16), (3, 20), (3, 24), (4, 16), (4, 20), (4, 24), (4, 32)]  # (container bytes, S)


def containers(cb, bits, lj, depth, channels, fs, counts, seed):
    """int64 [channels, NP * fs] sign-extended containers: random samples, the edge samples of the pair, right-justified
    ones outside the range where the container has room; behind every packet's count the largest container"""
    rng = np.random.default_rng(seed)
    frames = NP * fs
    top, full = 1 << (bits - 1), 1 << (8 * cb - 1)
    s = rng.integers(-top, top, (channels, frames))
    edge = R.edge_samples(bits, depth)
    if not lj and full > top:  # and what a right-justified container can hold outside the range
        edge = np.concatenate([edge, [top, top + 1, full - 1, -top - 1, -full, min(top * 3 // 2, full - 1)]])
    for c in range(channels):
        for p, k in enumerate(counts):  # in every packet, in front of its count (a short packet: as many as fit)
            pos = rng.choice(k, min(edge.size, k), replace=False)
            s[c, p * fs + pos] = np.roll(edge, -(p + c))[::-1][:pos.size]
    v = (s << (8 * cb - bits)) | rng.integers(0, 1 << (8 * cb - bits), s.shape) if lj else s
    for p, k in enumerate(counts):
        v[:, p * fs + k:(p + 1) * fs] = full - 1
    return v


def as_tensor(v, cb, layout):
    """the containers [C, frames] as a cuda tensor in a layout -> (x, kwargs of requantize / encode_int)"""
    ch, frames = v.shape
    if cb == 3:
        pad = 5  # containers between two rows of the wide layout
        if layout in ("planar", "offset"):
            flat, cs, fst = v.reshape(-1), frames, 1
        elif layout in ("wide", "gap"):
            w = np.full((ch, frames + pad), (1 << 23) - 1, np.int64)
            w[:, :frames] = v
            flat, cs, fst = w.reshape(-1)[:(ch - 1) * (frames + pad) + frames], frames + pad, 1
        else:  # interleaved / transposed: frames contiguous
            flat, cs, fst = np.ascontiguousarray(v.T).reshape(-1), 1, ch
        b = R.pack3(flat)
        if layout == "offset":  # the base one container in: not dword aligned
            b = np.concatenate([np.zeros(3, np.uint8), b])
            return torch.from_numpy(b).cuda()[3:], dict(container_bytes=3, channel_stride=cs, frame_stride=fst)
        return torch.from_numpy(b).cuda(), dict(container_bytes=3, channel_stride=cs, frame_stride=fst)
    dt = np.int16 if cb == 2 else np.int32
    a = v.astype(dt)
    if layout == "planar":
        return torch.from_numpy(a).cuda(), {}
    if layout in ("interleaved", "transposed"):
        return torch.from_numpy(np.ascontiguousarray(a.T)).cuda().t(), {}
    if layout in ("wide", "gap"):  # channel_stride > frames: no multiple of 4, and one (the vector path still)
        w = np.full((ch, frames + (5 if layout == "wide" else 8)), np.iinfo(dt).max, dt)
        w[:, :frames] = a
        return torch.from_numpy(w).cuda()[:, :frames], {}
    assert layout == "offset"  # the base one container in
    flat = np.concatenate([np.zeros(1, dt), a.reshape(-1)])
    return torch.from_numpy(flat).cuda()[1:].view(ch, frames), {}


def want_of(v, cb, bits, lj, depth, fs, counts, seed=None, origin=None):
    s, clip = R.convert(v, bits, cb, lj, depth, fs, num_samples=counts, seed=seed, origin=origin)
    return R.pack(s, depth), clip.reshape(v.shape[0], NP, fs).sum(axis=(0, 2))


def check(ctx, cb, bits, lj, depth, channels, fs, counts, layout, dither, origin, seed):
    fmt = alac_amd.make_format(fs, depth, channels, 44100)
    v = containers(cb, bits, lj, depth, channels, fs, counts, seed)
    x, kw = as_tensor(v, cb, layout)
    ns = torch.tensor(counts, dtype=torch.int32, device="cuda")
    og = None if origin is None else torch.tensor(origin, dtype=torch.int64, device="cuda")
    pcm, clip = ctx.requantize(fmt, x, bits=bits, left_justified=lj, num_samples=ns, clipped=True,
                               dither="tpdf" if dither else None, seed=seed, packet_origin=og, **kw)
    ctx.synchronize()
    want, want_clip = want_of(v, cb, bits, lj, depth, fs, counts, seed if dither else None, origin)
    what = (cb, bits, lj, depth, channels, fs, layout, dither)
    assert np.array_equal(clip.cpu().numpy(), want_clip), (what, clip.cpu().tolist(), want_clip.tolist())
    assert np.array_equal(pcm.cpu().numpy(), want), what
    return want_clip


@pytest.mark.parametrize("cb,bits", SOURCES)
def test_every_depth_pair_and_justification(gpu_ctx, cb, bits):
    """all four targets from one source width: widening, identity and reduction, the latter with and without dither"""
    fs, counts = 4096, [4096, 4096, 2049]
    for lj in (True, False):
        for depth in R.DEPTHS:
            for dither in ((False, True) if depth < bits else (False,)):
                clips = check(gpu_ctx, cb, bits, lj, depth, 2, fs, counts, "planar", dither, [0, 4097, 8192] if dither else None,
                              cb * 1000 + bits * 10 + depth)
                if depth < bits or (not lj and bits < 8 * cb):  # the top tie clips; containers outside the range do
                    assert (clips > 0).all(), (cb, bits, lj, depth, clips)


@pytest.mark.parametrize("channels", [1, 2, 3, 6])
@pytest.mark.parametrize("fs", [4096, 1028, 17])
def test_every_path_layout_and_frame_size(gpu_ctx, fs, channels):
    """fs 4096 and 1028 (two blocks per packet, the second nearly empty) take the vector paths at 1 and 2 channels, 17 and
    3 / 6 channels the general one; so do a base one container in and (int16 / int32) a channel stride that is odd"""
    counts = [fs, fs, fs - 3 if fs > 17 else 6]
    origin = [0, fs + 1, 5 * fs]  # an odd entry: three Philox calls per lane and channel
    for cb, bits, lj, depth, dither in ((2, 16, True, 16, False), (2, 16, False, 24, False), (3, 24, True, 16, True),
                                        (3, 20, False, 20, False), (4, 32, True, 16, True), (4, 24, False, 20, False),
                                        (4, 24, True, 16, True)):
        for layout in ("planar", "interleaved", "wide", "gap", "offset"):
            check(gpu_ctx, cb, bits, lj, depth, channels, fs, counts, layout, dither, origin if dither else None,
                  fs + 10 * channels + cb)


def fetch(ctx, b):
    ctx.synchronize()
    total = int(b["offsets"][-1].item())
    return b["out"][:total].cpu().numpy(), b["sizes"].cpu().numpy(), b["offsets"].cpu().numpy()


def assert_same(got, want, what):
    assert np.array_equal(got[1], want[1]), (what, "sizes")
    assert np.array_equal(got[2], want[2]), (what, "offsets")
    assert np.array_equal(got[0], want[0]), (what, "stream")


@pytest.mark.parametrize("cb,bits,lj,depth,channels,dither", [(4, 24, True, 16, 2, True), (4, 32, True, 24, 2, False),
                                                              (2, 16, True, 16, 1, False), (3, 24, False, 20, 6, True),
                                                              (4, 16, False, 32, 2, False)])
def test_encode_int_equals_encode_of_the_requantized_pcm(gpu_ctx, cb, bits, lj, depth, channels, dither):
    ctx = gpu_ctx
    fs, counts = 4096, [4096, 1001, 4096]
    fmt = alac_amd.make_format(fs, depth, channels, 44100)
    v = containers(cb, bits, lj, depth, channels, fs, counts, 77 + cb + depth)
    x, kw = as_tensor(v, cb, "planar")
    kw.update(bits=bits, left_justified=lj, dither="tpdf" if dither else None, seed=5)
    want_pcm, want_clip = want_of(v, cb, bits, lj, depth, fs, counts, 5 if dither else None)
    pcm = torch.from_numpy(want_pcm).cuda()
    ns = torch.tensor(counts, dtype=torch.int32, device="cuda")
    got = ctx.encode_int(fmt, x, num_samples=ns, clipped=True, **kw)
    assert_same(fetch(ctx, got), fetch(ctx, ctx.encode(fmt, pcm, NP, num_samples=ns)), "default")
    assert np.array_equal(got["clipped"].cpu().numpy(), want_clip)
    if channels <= 2:
        with ctx.options(lpc=1):
            assert_same(fetch(ctx, ctx.encode_int(fmt, x, num_samples=ns, **kw)),
                        fetch(ctx, ctx.encode(fmt, pcm, NP, num_samples=ns)), "lpc")
    # a segment table with its bound, the state out and in again
    seg = torch.tensor([0, 2, NP], dtype=torch.int32, device="cuda")
    words = 2 * int(ctx.lib.alac_hip_state_int16(C.byref(fmt)))
    st_got = torch.zeros(words, dtype=torch.int16, device="cuda")
    st_ref = torch.zeros(words, dtype=torch.int16, device="cuda")
    for state_in in (False, True):
        skw = dict(num_samples=ns, seg_first=seg, max_segment_packets=2, state_in=state_in)
        assert_same(fetch(ctx, ctx.encode_int(fmt, x, state=st_got, **skw, **kw)),
                    fetch(ctx, ctx.encode(fmt, pcm, NP, state=st_ref, **skw)), ("segments", state_in))
        assert torch.equal(st_got, st_ref)


@pytest.mark.parametrize("bits,depth", [(20, 16), (24, 16), (24, 20)])
def test_undithered_equals_encode_float(gpu_ctx, bits, depth):
    ctx = gpu_ctx
    fs, counts = 4096, [4096, 4096, 4095]
    fmt = alac_amd.make_format(fs, depth, 2, 44100)
    v = containers(4, bits, False, depth, 2, fs, counts, bits + depth)
    top = 1 << (bits - 1)
    v = np.clip(v, -top, top - 1)  # a float has no container to be out of range in
    ns = torch.tensor(counts, dtype=torch.int32, device="cuda")
    xf = torch.from_numpy((v.astype(np.float64) * 2.0 ** -(bits - 1)).astype(np.float32)).cuda()
    a = ctx.encode_int(fmt, torch.from_numpy(v.astype(np.int32)).cuda(), bits=bits, left_justified=False, num_samples=ns, clipped=True)
    ga = fetch(ctx, a)
    b = ctx.encode_float(fmt, xf, num_samples=ns, clipped=True)
    assert_same(ga, fetch(ctx, b), (bits, depth))
    assert torch.equal(a["clipped"], b["clipped"]) and int(a["clipped"].sum()) > 0


@pytest.mark.parametrize("depth", R.DEPTHS)
def test_identity_equals_encode_of_the_source_bytes(gpu_ctx, depth):
    """S == b, interleaved, the stream's own container: the source bytes are the PCM"""
    ctx = gpu_ctx
    fs = 4096
    fmt = alac_amd.make_format(fs, depth, 2, 44100)
    src = alac_amd.synth_pcm(0, NP, fmt)
    want = fetch(ctx, ctx.encode(fmt, torch.from_numpy(src).cuda(), NP))
    if depth in (16, 32):
        x = torch.from_numpy(src.view("<i2" if depth == 16 else "<i4").reshape(NP * fs, 2)).cuda().t()
        got = ctx.encode_int(fmt, x)
    else:  # 20 bits sit left-justified in their 3 bytes
        got = ctx.encode_int(fmt, torch.from_numpy(src).cuda(), bits=depth, left_justified=True, container_bytes=3,
                             channel_stride=1, frame_stride=2)
    assert_same(fetch(ctx, got), want, depth)


def test_dither_repeats_and_does_not_depend_on_the_batch(gpu_ctx):
    ctx = gpu_ctx
    fs = 4096
    fmt = alac_amd.make_format(fs, 16, 2, 44100)
    rng = np.random.default_rng(12)
    files = [torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31, (2, k * fs), dtype=np.int64).astype(np.int32)).cuda() for k in (1, 2)]
    alone = [fetch(ctx, ctx.encode_int(fmt, f, bits=24, dither="tpdf", seed=3))[0] for f in files]
    again = fetch(ctx, ctx.encode_int(fmt, files[1], bits=24, dither="tpdf", seed=3))[0]
    other = fetch(ctx, ctx.encode_int(fmt, files[1], bits=24, dither="tpdf", seed=4))[0]
    assert np.array_equal(again, alone[1]) and not np.array_equal(other, alone[1])
    origin = torch.tensor([0, 0, fs], dtype=torch.int64, device="cuda")
    batch = fetch(ctx, ctx.encode_int(fmt, torch.cat(files, dim=1), bits=24, dither="tpdf", seed=3, packet_origin=origin))
    offs = batch[2]
    assert np.array_equal(batch[0][:offs[1]], alone[0]) and np.array_equal(batch[0][offs[1]:], alone[1])
    # without the table the second file's frames count on from the first one's: other dither, other bytes
    plain = fetch(ctx, ctx.encode_int(fmt, torch.cat(files, dim=1), bits=24, dither="tpdf", seed=3))
    assert np.array_equal(plain[0][:plain[2][1]], alone[0]) and not np.array_equal(plain[0][plain[2][1]:], alone[1])


@pytest.fixture(scope="module")
def harness(gpu_ctx):
    subprocess.check_call(["make", "-C", CPP, "-f", "encode_int.mk", "encode_int"], stdout=subprocess.DEVNULL)
    return os.path.join(CPP, "encode_int")


@pytest.mark.parametrize("cb,bits,lj,depth,channels,dither", [(4, 24, True, 16, 2, True), (3, 24, False, 20, 3, False),
                                                              (2, 16, True, 24, 1, False)])
def test_host_forms_and_the_class_equal_the_device_form(gpu_ctx, harness, tmp_path, cb, bits, lj, depth, channels, dither):
    ctx = gpu_ctx
    fs, counts, origin = 4096, [4096, 4096, 999], [0, 4097, 9000]
    fmt = alac_amd.make_format(fs, depth, channels, 44100)
    v = containers(cb, bits, lj, depth, channels, fs, counts, 200 + cb)
    # the host forms stage only what the counts cover: the file ends with the last frame of the last packet
    live = 2 * fs + counts[2]
    inter = np.ascontiguousarray(v[:, :live].T).reshape(-1)
    raw = R.pack3(inter) if cb == 3 else inter.astype("<i2" if cb == 2 else "<i4").view(np.uint8)
    (tmp_path / "in").write_bytes(raw.tobytes())
    (tmp_path / "counts").write_bytes(np.array(counts, np.uint32).tobytes())
    (tmp_path / "segs").write_bytes(np.array([0, 2, NP], np.uint32).tobytes())
    (tmp_path / "origin").write_bytes(np.array(origin, np.uint64).tobytes())
    p = subprocess.run([harness, str(tmp_path)] + [str(a) for a in (fs, depth, channels, cb, bits, int(lj), 1, channels,
                                                                    int(dither), 21)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    x, kw = as_tensor(v, cb, "interleaved")
    kw.update(bits=bits, left_justified=lj, dither="tpdf" if dither else None, seed=21,
              packet_origin=torch.tensor(origin, dtype=torch.int64, device="cuda"),
              num_samples=torch.tensor(counts, dtype=torch.int32, device="cuda"))
    pcm, clip = ctx.requantize(fmt, x, clipped=True, **kw)
    b = ctx.encode_int(fmt, x, seg_first=torch.tensor([0, 2, NP], dtype=torch.int32, device="cuda"), clipped=True, **kw)
    dev = fetch(ctx, b)
    read = lambda name, dt: np.frombuffer((tmp_path / name).read_bytes(), dt)  # noqa: E731
    assert np.array_equal(read("pcm", np.uint8), pcm.cpu().numpy())
    assert np.array_equal(read("pcm_clipped", np.uint32), clip.cpu().numpy())
    assert np.array_equal(read("sizes", np.uint32), dev[1]) and np.array_equal(read("stream", np.uint8), dev[0])
    assert np.array_equal(read("clipped", np.uint32), b["clipped"].cpu().numpy())
    want_pcm, want_clip = want_of(v, cb, bits, lj, depth, fs, counts, 21 if dither else None, origin)
    assert np.array_equal(pcm.cpu().numpy(), want_pcm) and np.array_equal(clip.cpu().numpy(), want_clip)


def test_refusals_write_nothing(gpu_ctx):
    ctx, lib = gpu_ctx, gpu_ctx.lib
    fs, n = 4096, NP
    fmt = alac_amd.make_format(fs, 16, 2, 44100)
    x = torch.zeros((2, n * fs), dtype=torch.int32, device="cuda")
    cap = int(lib.alac_hip_encode_max_output_bytes(C.byref(fmt), n))
    out = torch.full((cap,), 0xAB, dtype=torch.uint8, device="cuda")
    sizes = torch.full((n,), 7, dtype=torch.int32, device="cuda")
    offs = torch.full((n + 1,), 9, dtype=torch.int64, device="cuda")
    clip = torch.full((n,), 5, dtype=torch.int32, device="cuda")
    pcm = torch.full((n * fmt.packet_bytes,), 0xCD, dtype=torch.uint8, device="cuda")
    origin = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    wsb = int(lib.alac_hip_encode_int_workspace_bytes(C.byref(fmt), n, n))
    stage = wsb - int(lib.alac_hip_encode_workspace_bytes(C.byref(fmt), n, n))
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    bad_seg = torch.tensor([0, 3, 1, n], dtype=torch.int32, device="cuda")
    Src, Dz = alac_amd.capi.IntSource, alac_amd.capi.Dither
    good = dict(container_bytes=4, bits=24, left_justified=1, reserved=0, channel_stride=n * fs, frame_stride=1)

    def encode(ptr=x.data_ptr(), src=True, f=fmt, dz=None, og=None, seg=None, nseg=n, ws_bytes=wsb, capacity=cap, **s):
        st = Src(**dict(good, **s))
        return lib.alac_hip_encode_int(ctx.h, C.byref(f), ptr, C.byref(st) if src else None, None, n,
                                       None if seg is None else seg.data_ptr(), nseg, 0, None, 0, ws.data_ptr(), ws_bytes,
                                       out.data_ptr(), capacity, sizes.data_ptr(), offs.data_ptr(), clip.data_ptr(),
                                       None if dz is None else C.byref(dz), og)

    def requant(ptr=x.data_ptr(), src=True, f=fmt, dz=None, og=None, dst=pcm.data_ptr(), capacity=pcm.numel(), **s):
        st = Src(**dict(good, **s))
        return lib.alac_hip_pcm_requantize(ctx.h, C.byref(f), ptr, C.byref(st) if src else None, None, n, dst, capacity,
                                           clip.data_ptr(), None if dz is None else C.byref(dz), og)

    fmt24 = alac_amd.make_format(fs, 24, 2, 44100)
    shared = {
        "null d_in": dict(ptr=None),
        "null src": dict(src=False),
        "container_bytes 1": dict(container_bytes=1),
        "container_bytes 5": dict(container_bytes=5),
        "bits 18": dict(bits=18),
        "bits above the container": dict(container_bytes=2, bits=24),
        "reserved": dict(reserved=1),
        "left_justified 2": dict(left_justified=2),
        "misaligned int32": dict(ptr=x.data_ptr() + 2),
        "misaligned int16": dict(ptr=x.data_ptr() + 1, container_bytes=2, bits=16),
        "frame_stride 0": dict(frame_stride=0),
        "channel_stride 0": dict(channel_stride=0),
        "index overflow": dict(channel_stride=1 << 62),
        "dither where nothing is rounded": dict(f=fmt24, dz=Dz(1, 0, 1)),
        "dither when widening": dict(bits=16, dz=Dz(1, 0, 1)),
        "dither mode": dict(dz=Dz(2, 0, 1)),
        "dither reserved": dict(dz=Dz(1, 1, 1)),
        "misaligned origin": dict(dz=Dz(1, 0, 1), og=origin.data_ptr() + 4),
        "bad format": dict(f=alac_amd.make_format(fs, 18, 2, 44100)),
    }
    for what, kw in shared.items():
        assert encode(**kw) == -50, ("encode_int", what)
        assert requant(**kw) == -50, ("requantize", what)
    for what, kw in {"workspace too small": dict(ws_bytes=stage + 4096), "workspace below the stage": dict(ws_bytes=1024),
                     "output capacity": dict(capacity=cap - 1), "bad segment table": dict(seg=bad_seg, nseg=3),
                     "segment count": dict(seg=bad_seg, nseg=n + 1)}.items():
        assert encode(**kw) == -50, what
    for what, kw in {"null d_pcm_out": dict(dst=None), "misaligned d_pcm_out": dict(dst=pcm.data_ptr() + 8),
                     "pcm_capacity": dict(capacity=pcm.numel() - 1)}.items():
        assert requant(**kw) == -50, what
    with ctx.options(lpc=1, fast_mode=1):
        assert encode() == -50, "lpc + fast_mode"
    ctx.synchronize()
    assert (out == 0xAB).all() and (sizes == 7).all() and (offs == 9).all() and (clip == 5).all() and (pcm == 0xCD).all()
    # the context is still usable, and a packed 3-byte source needs no alignment at all
    assert encode() == 0 and requant() == 0 and requant(ptr=x.data_ptr() + 1, container_bytes=3, channel_stride=1, frame_stride=2) == 0
    ctx.synchronize()
    assert int(pcm.count_nonzero()) == 0 and int(clip.sum()) == 0
