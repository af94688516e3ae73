"""GPU: alac_hip_pcm_crc32.  The oracle is zlib.crc32 and every comparison is exact equality of both fields: one range at
every misalignment and at every size at which the kernel changes path (lane, wave and block chunk, one pass of the grid),
all-zero buffers (the length term), range tables with gaps, empty ranges and boundaries inside 16-byte groups, repeated calls,
every refusal, the host form, and the digest of what the codec decodes against the bytes it was encoded from."""
import lzma
import os
import subprocess
import zlib

import numpy as np
import pytest
import torch

import alac_amd
from alac_amd.capi import PCM_CRC_BLOCK_BYTES as BLOCK, PCM_CRC_LANE_BYTES as LANE, PCM_CRC_PASS_BYTES as PASS, PCM_CRC_WAVE_BYTES as WAVE

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
SENTINEL = 0x55555555


def want(host, ranges):
    return [(zlib.crc32(host[o:o + n].tobytes()), n) for o, n in ranges]


def check(ctx, dev, host, ranges, what=""):
    got = ctx.pcm_crc32(dev, ranges)
    exp = want(host, ranges)
    assert got == exp, (what, [(i, g, e) for i, (g, e) in enumerate(zip(got, exp)) if g != e][:4])
    return got


@pytest.fixture(scope="module")
def small():
    """random bytes for the one-range cases: two block chunks and a little"""
    host = np.random.default_rng(5).integers(0, 256, 2 * BLOCK + 64, dtype=np.uint8)
    return host, torch.from_numpy(host).cuda()


def test_one_range_at_every_length_and_misalignment(gpu_ctx, small):
    host, dev = small
    lengths = [0, 1, 2, 3, 4, 15, 16, 17, 31, 33]
    for chunk in (LANE, WAVE, BLOCK):
        lengths += [chunk - 1, chunk, chunk + 1]
    for n in lengths:
        for off in range(16):
            # as a range of the buffer (the chunks count from the buffer's start) ...
            check(gpu_ctx, dev, host, [(off, n)], f"range {off}+{n}")
            # ... and as a buffer of its own that starts at any address
            got = gpu_ctx.pcm_crc32(dev[off:off + n])
            assert got == [(zlib.crc32(host[off:off + n].tobytes()), n)], f"slice {off}+{n}"


def test_all_zero_buffers_and_leading_zeros(gpu_ctx):
    for n in (1, 4, 8, 4096, BLOCK + 1):
        z = torch.zeros(n, dtype=torch.uint8, device="cuda")
        assert gpu_ctx.pcm_crc32(z) == [(zlib.crc32(bytes(n)), n)], n
    assert gpu_ctx.pcm_crc32(torch.zeros(4, dtype=torch.uint8, device="cuda")) == [(0x2144df1c, 4)]
    assert gpu_ctx.pcm_crc32(torch.zeros(8, dtype=torch.uint8, device="cuda")) == [(0x6522df69, 8)]
    assert gpu_ctx.pcm_crc32(torch.zeros(0, dtype=torch.uint8, device="cuda")) == [(0, 0)]
    # a buffer whose first half is zero: a reduction must not lose what the zeros in front do to the length term
    for n in (2 * LANE, 2 * WAVE + 6, 4 * BLOCK + 10):
        host = np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8)
        host[:n // 2] = 0
        check(gpu_ctx, torch.from_numpy(host).cuda(), host, [(0, n)], f"half zero {n}")
        check(gpu_ctx, torch.from_numpy(host).cuda(), host, [(0, n // 2), (n // 2, n - n // 2)], f"half zero, two ranges {n}")


@pytest.fixture(scope="module")
def large():
    """three passes of the grid and a little more, different bytes in each pass"""
    n = 3 * PASS + 2 * BLOCK + 77
    g = torch.Generator(device="cuda")
    g.manual_seed(9)
    dev = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=g)
    for k in range(4):  # planted: a mark of its own at the same place of every pass
        dev[k * PASS + 5 * WAVE + 3:k * PASS + 5 * WAVE + 3 + 8] = 17 * (k + 1)
    host = dev.cpu().numpy()
    return host, dev


def test_range_larger_than_one_pass_of_the_grid(gpu_ctx, large):
    host, dev = large
    n = host.size
    check(gpu_ctx, dev, host, [(0, n)], "all of it")
    assert gpu_ctx.pcm_crc32(dev) == want(host, [(0, n)])
    # one range that starts beside a pass edge and ends inside a later pass
    check(gpu_ctx, dev, host, [(PASS - 1, PASS + WAVE + 2)], "from beside an edge")
    check(gpu_ctx, dev, host, [(7, 2 * PASS)], "two passes long, misaligned")
    # boundaries at, beside and inside the pass edges, no gaps
    cuts = [0, PASS - 1, PASS, PASS + 1, PASS + WAVE + 5, 2 * PASS - LANE, 2 * PASS + BLOCK, 3 * PASS - 3, 3 * PASS + BLOCK, n]
    check(gpu_ctx, dev, host, [(a, b - a) for a, b in zip(cuts, cuts[1:])], "cuts")
    # ... and with whole passes left out between the ranges
    check(gpu_ctx, dev, host, [(3, BLOCK), (PASS + BLOCK, 5), (2 * PASS + 9, PASS), (n - 1, 1)], "gaps of a pass")


def test_tables(gpu_ctx, small):
    host, dev = small
    rng = np.random.default_rng(6)
    # 300 ranges of 0..7 bytes, some of them touching, some behind gaps
    ranges, at = [], 0
    for _ in range(300):
        at += int(rng.integers(0, 3))
        n = int(rng.integers(0, 8))
        ranges.append((at, n))
        at += n
    check(gpu_ctx, dev, host, ranges, "300 small ranges")
    # a table that starts behind byte 0 and ends before total_bytes; empty first and last ranges
    check(gpu_ctx, dev, host, [(100, 50), (150, WAVE), (WAVE + 3000, 9)], "inner table")
    check(gpu_ctx, dev, host, [(5, 0), (5, 3 * WAVE + 1), (BLOCK + 100, 0)], "empty first and last")
    check(gpu_ctx, dev, host, [(0, 0), (0, 0), (host.size, 0)], "only empty ranges")
    # gaps whose bytes differ between two calls: the digests do not
    ranges = [(3, 61), (LANE + 10, WAVE), (2 * WAVE, 1), (BLOCK - 5, BLOCK + 11)]
    first = check(gpu_ctx, dev, host, ranges, "gaps")
    other = dev.clone()
    keep = torch.zeros(host.size, dtype=torch.bool, device="cuda")
    for o, n in ranges:
        keep[o:o + n] = True
    other[~keep] ^= 0xA5
    assert gpu_ctx.pcm_crc32(other, ranges) == first
    assert gpu_ctx.pcm_crc32(other) != gpu_ctx.pcm_crc32(dev)


def raw_call(ctx, dev, total, table, n, ws, digests, ptr=None, ws_bytes=None, table_ptr=None):
    tab = None if table is None else np.ascontiguousarray(table, dtype=np.uint64)
    return ctx.lib.alac_hip_pcm_crc32(
        ctx.h, dev.data_ptr() if ptr is None else ptr, total, (None if tab is None else tab.ctypes.data) if table_ptr is None else table_ptr,
        n, None if ws is None else ws.data_ptr(), (0 if ws is None else ws.numel()) if ws_bytes is None else ws_bytes,
        None if digests is None else digests.data_ptr())


def rows(host, ranges):
    return np.array([[n & 0xFFFFFFFF, n >> 32, zlib.crc32(host[o:o + n].tobytes()), 0] for o, n in ranges], dtype=np.uint32)


def test_two_calls_into_one_buffer_do_not_accumulate(gpu_ctx, small):
    ctx = gpu_ctx
    host, dev = small
    ranges = [(1, 0), (1, 70), (100, 2 * WAVE + 3), (BLOCK, BLOCK)]
    ws = torch.empty(int(ctx.lib.alac_hip_pcm_crc32_workspace_bytes(4)), dtype=torch.uint8, device="cuda")
    digests = torch.full((4, 4), SENTINEL, dtype=torch.int32, device="cuda")  # every field is written, reserved as 0
    torch.cuda.synchronize()
    for _ in range(2):
        assert raw_call(ctx, dev, host.size, ranges, 4, ws, digests) == 0
        ctx.synchronize()
        assert np.array_equal(digests.cpu().numpy().view(np.uint32), rows(host, ranges))
    # no table: one range, and no workspace to speak of
    one = torch.full((1, 4), SENTINEL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for _ in range(2):
        assert raw_call(ctx, dev, host.size, None, 1, None, one) == 0
        ctx.synchronize()
        assert np.array_equal(one.cpu().numpy().view(np.uint32), rows(host, [(0, host.size)]))


def test_pinned_table_overwritten_right_after_the_call(gpu_ctx, small):
    ctx = gpu_ctx
    host, dev = small
    ranges = [(o, 37) for o in range(0, 512 * 40, 40)]
    table = torch.tensor(ranges, dtype=torch.int64).pin_memory()
    ws = torch.empty(int(ctx.lib.alac_hip_pcm_crc32_workspace_bytes(len(ranges))), dtype=torch.uint8, device="cuda")
    digests = torch.empty((len(ranges), 4), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for _ in range(3):
        assert raw_call(ctx, dev, host.size, None, len(ranges), ws, digests, table_ptr=table.data_ptr()) == 0
        table.fill_(-1)  # the call has copied it out
        ctx.synchronize()
        assert np.array_equal(digests.cpu().numpy().view(np.uint32), rows(host, ranges))
        table.copy_(torch.tensor(ranges, dtype=torch.int64))


def test_refusals_write_nothing(gpu_ctx, small):
    ctx = gpu_ctx
    host, dev = small
    t = 1000
    table = [(0, 10), (10, 490), (600, 400)]
    ws = torch.empty(int(ctx.lib.alac_hip_pcm_crc32_workspace_bytes(3)) + 256, dtype=torch.uint8, device="cuda")
    digests = torch.full((3, 4), SENTINEL, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ok = dict(ctx=ctx, dev=dev, total=t, table=table, n=3, ws=ws, digests=digests)
    cases = {
        "null d_pcm with bytes": dict(ptr=0),
        "num_ranges 0": dict(n=0),
        "no table for three ranges": dict(table=None),
        "table not ascending": dict(table=[(10, 490), (0, 10), (600, 400)]),
        "ranges overlap": dict(table=[(0, 11), (10, 490), (600, 400)]),
        "a range's end overflows": dict(table=[(0, 10), (10, 490), (600, 2 ** 64 - 500)]),
        "table ends behind total_bytes": dict(table=[(0, 10), (10, 490), (600, 401)]),
        "workspace too small": dict(ws_bytes=3 * 16 - 1),
        "null workspace": dict(ws=None, ws_bytes=ws.numel()),
        "misaligned workspace": dict(ws=ws[4:], ws_bytes=ws.numel() - 4),
        "misaligned d_digests": dict(digests=digests.view(-1)[1:]),
    }
    for what, kw in cases.items():
        assert raw_call(**{**ok, **kw}) == -50, what
    assert raw_call(**{**ok, "digests": None}) == -50
    ctx.synchronize()
    assert bool((digests == SENTINEL).all())
    # the context is still usable
    assert raw_call(**ok) == 0
    ctx.synchronize()
    assert np.array_equal(digests.cpu().numpy().view(np.uint32), rows(host, table))
    with pytest.raises(alac_amd.AlacError):
        ctx.pcm_crc32(dev, [(0, host.size + 1)])


def test_host_form_on_an_unaligned_slice(gpu_ctx):
    ctx = gpu_ctx
    base = np.random.default_rng(8).integers(0, 256, 3 * WAVE + 50, dtype=np.uint8)
    arr = base[3:]  # an address that is no multiple of anything
    assert arr.ctypes.data % 2 == 1
    table = np.array([(1, 5), (6, 0), (9, WAVE + 7), (2 * WAVE, WAVE)], dtype=np.uint64)
    dig = (alac_amd.PcmDigest * 4)()
    rc = ctx.lib.alac_hip_pcm_crc32_host(ctx.h, arr.ctypes.data, arr.size, table.ctypes.data, 4, dig)
    assert rc == 0, ctx.lib.alac_hip_last_error(ctx.h)
    assert [(d.crc32, d.bytes, d.reserved) for d in dig] == [(zlib.crc32(arr[o:o + n].tobytes()), n, 0) for o, n in table.tolist()]
    one = (alac_amd.PcmDigest * 1)()
    assert ctx.lib.alac_hip_pcm_crc32_host(ctx.h, arr.ctypes.data, arr.size, None, 1, one) == 0
    assert (one[0].crc32, one[0].bytes) == (zlib.crc32(arr.tobytes()), arr.size)
    assert ctx.lib.alac_hip_pcm_crc32_host(ctx.h, arr.ctypes.data, arr.size, table.ctypes.data, 4, None) == -50


def source_pcm(frames, ch, bits, seed):
    """interleaved little-endian PCM, 20-bit samples left-justified in 3 bytes"""
    rng = np.random.default_rng(seed)
    t = np.arange(frames)
    full = (1 << (bits - 1)) - 1
    v = np.stack([np.round((0.3 * np.sin(2 * np.pi * (300.0 + 90 * c) * t / 44100.0) + 0.02 * rng.standard_normal(frames)) * full)
                  for c in range(ch)], axis=1).astype(np.int64)
    if bits == 16:
        return np.frombuffer(v.astype("<i2").tobytes(), np.uint8)
    v = (v << 4) if bits == 20 else v
    return np.ascontiguousarray((v & 0xffffff).astype("<u4").view(np.uint8).reshape(-1, 4)[:, :3]).reshape(-1)


@pytest.mark.parametrize("bits,ch", [(16, 2), (24, 2), (20, 1), (16, 6)])
def test_digest_of_a_decode_equals_the_crc_of_the_source(gpu_ctx, bits, ch):
    ctx = gpu_ctx
    fmt = alac_amd.make_format(4096, bits, ch, 44100)
    frames = 47 * 4096 + 1234  # 48 packets, the last one short
    pcm = source_pcm(frames, ch, bits, bits + ch)
    stream, sizes, _ = ctx.encode_host(fmt, pcm, frames, segment_packets=1)
    assert len(sizes) == 48
    offs = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes.astype(np.int64))])).cuda()
    out, ns, st, _ = ctx.decode(ctx.magic_cookie(fmt), torch.from_numpy(stream).cuda(), offs, 48, zero_fill=False)
    ctx.synchronize()
    assert int(st.abs().sum()) == 0 and int(ns.sum()) == frames
    valid = frames * fmt.bytes_per_frame
    assert valid == pcm.size
    assert ctx.pcm_crc32(out, [(0, valid)]) == [(zlib.crc32(pcm.tobytes()), valid)]
    # per packet, joined on the host without touching the PCM again
    per = ctx.pcm_crc32(out, [(p * fmt.packet_bytes, int(ns[p]) * fmt.bytes_per_frame) for p in range(48)])
    crc = 0
    for c, n in per:
        crc = alac_amd.crc32_combine(crc, c, n)
    assert crc == zlib.crc32(pcm.tobytes())


@pytest.fixture(scope="module")
def harness(gpu_ctx):
    subprocess.check_call(["make", "-C", CPP, "-f", "test_batch.mk", "test_batch"], stdout=subprocess.DEVNULL)
    return os.path.join(CPP, "test_batch")


def test_class_level_test_batch_on_a_chained_file(gpu_ctx, harness, tmp_path):
    """ALACDecoder::TestBatch over the chained encode of the reference's audio/50.wav (237 packets): as one file, as three
    files of which the middle one is empty, and with the short last packet moved into the middle of a file (one range per
    packet, joined with alac_hip_crc32_combine)."""
    with open(os.path.join(ROOT, "tests", "golden", "wav50_pcm.xz"), "rb") as f:
        pcm = np.frombuffer(lzma.decompress(f.read()), np.uint8)
    fmt = alac_amd.make_format(4096, 16, 2, 44100)
    total = pcm.size // fmt.bytes_per_frame
    stream, sizes, _ = gpu_ctx.encode_host(fmt, pcm, total, segment_packets=0)
    npk = len(sizes)
    offs = np.concatenate([[0], np.cumsum(sizes.astype(np.int64))])
    (tmp_path / "cookie").write_bytes(gpu_ctx.magic_cookie(fmt).tobytes())

    def run(order, first):
        (tmp_path / "stream").write_bytes(b"".join(stream[offs[p]:offs[p + 1]].tobytes() for p in order))
        (tmp_path / "sizes").write_bytes(np.array([sizes[p] for p in order], dtype=np.uint32).tobytes())
        (tmp_path / "first").write_bytes(np.array(first, dtype=np.uint32).tobytes())
        p = subprocess.run([harness] + [str(tmp_path / n) for n in ("cookie", "stream", "sizes", "first")], capture_output=True,
                           text=True, timeout=120)
        assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
        lines = p.stdout.split("\n")
        return [(int(a, 16), int(b)) for a, b in (ln.split() for ln in lines[:len(first) - 1])], lines[len(first) - 1:len(first) + 1]

    def pcm_of(packets):
        return b"".join(pcm[p * fmt.packet_bytes:(p + 1) * fmt.packet_bytes].tobytes() for p in packets)

    whole = list(range(npk))
    got, tail = run(whole, [0, npk])
    assert got == [(zlib.crc32(pcm.tobytes()), pcm.size)] and tail == [f"frames {total}", "bad 0"]
    got, tail = run(whole, [0, 100, 100, npk])
    parts = [pcm_of(range(100)), b"", pcm_of(range(100, npk))]
    assert got == [(zlib.crc32(x), len(x)) for x in parts] and tail == [f"frames {total}", "bad 0"]
    assert total % 4096  # the last packet is short: in the middle of a file its frames no longer sit back to back
    order = list(range(npk - 10, npk)) + list(range(10))
    got, tail = run(order, [0, 20])
    assert got == [(zlib.crc32(pcm_of(order)), len(pcm_of(order)))] and tail[1] == "bad 0"
