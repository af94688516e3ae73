"""A lone predictor wave decides with scalars, once per pass, which stretch of its 16-step block pairs is live in every lane
(run_tile, alac_encode_v1_impl.hpp: wave_max(jlo), wave_min(jhi)); that stretch runs the unmasked step in a loop without a
per-block test, every other pair runs the masked step, and the LDS operand pointers move once per pair.  What can go wrong
is where the stretch meets a masked pair or a tile that a packet ends in — and a batch in which every wave holds one short
packet never enters the stretch, so the batches here are built per wave: uniform ones (the stretch really runs, and ends at
every place a search row of N / 8 or N / 32 steps or a final pass of N steps can end relative to a 64-step tile and a 16-step
pair), one short packet in an otherwise full wave, neighbouring waves with different stretches, pad lanes and escapes.
Every packet byte for byte and size for size against the CPU oracle, in the regime that runs this loop ("narrow": 0) and in
the three that share run_tile / lms_pass ("narrow": 1, "fused": 0, "thru": 1)."""
import numpy as np
import pytest

import alac_amd

pytestmark = pytest.mark.gpu

OPTS = [{"narrow": 0}, {"narrow": 1}, {"fused": 0}, {"thru": 1}]
FORMATS = [(16, 2), (24, 2), (16, 1), (24, 1)]
UNIFORM = [4096, 4095, 4033, 4032, 4031, 2048, 1024, 576, 520, 512, 200, 193, 192, 191, 136, 128, 120, 80, 72, 64]

_REF = {}


def _id(v):
    return ",".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else None


def _packets(oracle, key, depth, channels, ns, first=0):
    """(format, pcm, num_samples, oracle packets, oracle infos) of independent packets of ns[p] samples; computed once and shared"""
    if key not in _REF:
        n = len(ns)
        fmt = alac_amd.make_format(4096, depth, channels)
        pcm = alac_amd.synth_pcm(first, n, fmt)
        ns = np.asarray(ns, np.int32).copy()
        enc = oracle.encoder(4096, depth, channels)
        packets, infos = [], []
        for p in range(n):
            enc.reset()
            packets.append(enc.encode_packet(pcm[p * fmt.packet_bytes:p * fmt.packet_bytes + int(ns[p]) * fmt.bytes_per_frame],
                                             int(ns[p])))
            infos.append(enc.last_info())
        pcm.setflags(write=False)
        ns.setflags(write=False)
        _REF[key] = (fmt, pcm, ns, packets, infos)
    return _REF[key]


def _check(gpu_ctx, opts, case):
    import torch
    fmt, pcm, ns, packets, _ = case
    n = len(packets)
    with gpu_ctx.options(**opts):
        stream, sizes = gpu_ctx.encode_to_host(fmt, torch.from_numpy(pcm.copy()).cuda(), n,
                                               num_samples=torch.from_numpy(ns.copy()).cuda())
    off = 0
    for p, pk in enumerate(packets):
        assert sizes[p] == len(pk), (p, int(ns[p]))
        assert np.array_equal(stream[off:off + len(pk)], pk), (p, int(ns[p]))
        off += len(pk)
    assert off == len(stream)


def _wave(channels):
    """packets of one two-lane predictor wave: 32 chains"""
    return 32 // channels


@pytest.mark.parametrize("opts", OPTS, ids=_id)
@pytest.mark.parametrize("size", UNIFORM)
@pytest.mark.parametrize("depth,channels", FORMATS)
def test_uniform_batch(gpu_ctx, oracle, depth, channels, size, opts):
    """32 packets of one size: every wave's live stretch is the packet's own.  The sizes give search rows (N / 8, N / 32
    steps) of exactly one tile, one tile and a step, half a tile, less than a pair, and final passes of whole tiles, whole
    tiles +- 1, a tile and one block, and packets shorter than a tile"""
    _check(gpu_ctx, opts, _packets(oracle, ("uniform", depth, channels, size), depth, channels, [size] * 32))


@pytest.mark.parametrize("opts", OPTS, ids=_id)
@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("short", [200, 64, 4031])
@pytest.mark.parametrize("depth,channels", FORMATS)
def test_one_short_packet_in_a_full_wave(gpu_ctx, oracle, depth, channels, short, where, opts):
    """One wave of 4096-sample packets but one: the wave's stretch ends where the short packet does, and the full packets
    go on through masked pairs and checked tiles with the history the plain ones left"""
    n = _wave(channels)
    ns = [4096] * n
    ns[{"first": 0, "middle": n // 2, "last": n - 1}[where]] = short
    _check(gpu_ctx, opts, _packets(oracle, ("short", depth, channels, short, where), depth, channels, ns, first=3))


@pytest.mark.parametrize("opts", OPTS, ids=_id)
@pytest.mark.parametrize("depth,channels", FORMATS)
def test_neighbouring_waves_with_different_stretches(gpu_ctx, oracle, depth, channels, opts):
    """64 packets in runs of 16 of 4096, 1024, 4095 and 136 samples"""
    ns = [s for s in (4096, 1024, 4095, 136) for _ in range(16)]
    _check(gpu_ctx, opts, _packets(oracle, ("runs", depth, channels), depth, channels, ns, first=5))


@pytest.mark.parametrize("opts", OPTS + [{"narrow": 0, "fold": 0}], ids=_id)
@pytest.mark.parametrize("n", [24, 40])
def test_pad_lanes_and_escapes(gpu_ctx, oracle, n, opts):
    """24 and 40 whole packets of all eight signal classes: the last wave has pad lanes, escaped packets idle in the final
    pass, and 4-tap rows (warm-up of 5 positions) share a wave with 8-tap rows (9)"""
    case = _packets(oracle, ("classes", n), 16, 2, [4096] * n)
    infos = case[4]
    coded = [i for i in infos if not i["escape"]]
    assert any(i["escape"] for i in infos), "no escaped packet in the batch"
    assert any(4 in (i["numU"], i["numV"]) for i in coded), "no 4-tap final row in the batch"
    assert any(8 in (i["numU"], i["numV"]) for i in coded), "no 8-tap final row in the batch"
    _check(gpu_ctx, opts, case)


@pytest.mark.parametrize("k", [2, 4])
def test_publish_cadence(gpu_ctx, oracle, k):
    """row publication every k tiles over a pass whose tiles all take the unmasked stretch"""
    _check(gpu_ctx, {"narrow": 0, "pub_every": k}, _packets(oracle, ("uniform", 16, 2, 4096), 16, 2, [4096] * 32))


@pytest.mark.parametrize("opts", OPTS, ids=_id)
def test_chained_segments_carry_the_coefficients(gpu_ctx, oracle, opts):
    """4 segments of 6 packets: the rows a packet leaves are the rows the next one starts from, and the state comes back"""
    import torch
    nseg, per = 4, 6
    n = nseg * per
    key = ("chain", nseg, per)
    if key not in _REF:
        fmt = alac_amd.make_format(4096, 16, 2)
        pcm = alac_amd.synth_pcm(7, n, fmt)
        enc = oracle.encoder(4096, 16, 2)
        refs = []
        for s in range(nseg):
            enc.reset()
            refs.append(enc.encode_stream(pcm[s * per * fmt.packet_bytes:(s + 1) * per * fmt.packet_bytes], per * 4096, 0)
                        + (enc.get_state(),))
        pcm.setflags(write=False)
        _REF[key] = (fmt, pcm, refs)
    fmt, pcm, refs = _REF[key]
    seg_first = torch.arange(0, n + 1, per, dtype=torch.int32).cuda()
    state = torch.zeros((nseg, 64), dtype=torch.int16).cuda()
    with gpu_ctx.options(**opts):
        stream, sizes = gpu_ctx.encode_to_host(fmt, torch.from_numpy(pcm.copy()).cuda(), n, seg_first=seg_first, state=state)
    offs = np.concatenate([[0], np.cumsum(sizes.astype(np.int64))])
    assert offs[-1] == len(stream)
    for s, (ref, rs, st) in enumerate(refs):
        a, b = s * per, (s + 1) * per
        assert np.array_equal(sizes[a:b], rs), s
        assert np.array_equal(stream[offs[a]:offs[b]], ref), s
        assert np.array_equal(state[s].cpu().numpy(), st), s
