"""The predictor -> coder hand-off in 16-byte groups (residual planes [sample / 4][stream][4], alac_plane_index.hpp) and the
publish cadence of the producer waves (option "pub_every": every 1 / 2 / 4 / 8 tiles, every tile at the end of a pass):
every lane mapping under every cadence, tile counts no cadence divides, groups cut by packet ends and mixed lengths inside a
wave for every sample format, search passes whose row count is no multiple of 4 and whose converge part (P2 rows) ends inside
a group, and chained segments with the split coder, whose second wave starts at v1_split_at.  Every packet byte for byte and
size for size against the CPU oracle; by the oracle's own escape flags at most half of each case's packets are escapes, so
no case can pass without its flush and its coder running."""
import numpy as np
import pytest

import alac_amd

pytestmark = pytest.mark.gpu

CUTS = [4096, 4095, 4094, 4093, 4035, 4034, 4033, 3970, 2051, 2050, 131, 130, 67, 66, 65, 11, 10, 9, 7, 5]

_REF = {}


def _case(oracle, frame, depth, channels, n, cuts):
    """(format, pcm, num_samples, oracle packets, oracle escape flags) of a case; computed once and shared"""
    key = (frame, depth, channels, n, cuts is not None)
    if key not in _REF:
        fmt = alac_amd.make_format(frame, depth, channels)
        pcm = alac_amd.synth_pcm(0, n, fmt)
        ns = np.array([cuts[p % len(cuts)] for p in range(n)] if cuts else [frame] * n, np.int32)
        enc = oracle.encoder(frame, depth, channels)
        packets, escapes = [], []
        for p in range(n):
            enc.reset()
            packets.append(enc.encode_packet(pcm[p * fmt.packet_bytes:p * fmt.packet_bytes + int(ns[p]) * fmt.bytes_per_frame],
                                             int(ns[p])))
            escapes.append(int(enc.last_info()["escape"]))
        pcm.setflags(write=False)
        ns.setflags(write=False)
        _REF[key] = (fmt, pcm, ns, packets, escapes)
    return _REF[key]


def _check(gpu_ctx, oracle, opts, frame, depth, channels, n, cuts=None):
    import torch
    fmt, pcm, ns, packets, escapes = _case(oracle, frame, depth, channels, n, cuts)
    assert 2 * sum(escapes) <= n, f"{sum(escapes)} of {n} packets are escapes: the flush would hardly run"
    with gpu_ctx.options(**opts):
        stream, sizes = gpu_ctx.encode_to_host(fmt, torch.from_numpy(pcm.copy()).cuda(), n,
                                               num_samples=torch.from_numpy(ns.copy()).cuda() if cuts else None)
    off = 0
    for p, pk in enumerate(packets):
        assert sizes[p] == len(pk), (p, int(ns[p]))
        assert np.array_equal(stream[off:off + len(pk)], pk), (p, int(ns[p]))
        off += len(pk)
    assert off == len(stream)


def _id(v):
    return ",".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else None


@pytest.mark.parametrize("every", [1, 2, 4, 8])
@pytest.mark.parametrize("opts", [{"narrow": 0}, {"narrow": 1}, {"fused": 0}, {"thru": 1}], ids=_id)
def test_mappings_and_cadences(gpu_ctx, oracle, opts, every):
    """33 stereo packets = 66 chains: two full two-lane predictor waves and one with 30 pad slots, two coder waves"""
    _check(gpu_ctx, oracle, dict(opts, pub_every=every), 4096, 16, 2, 33)


@pytest.mark.parametrize("every", [4, 8])
@pytest.mark.parametrize("narrow", [0, 1])
@pytest.mark.parametrize("frame", [704, 4104])
def test_tile_counts_no_cadence_divides(gpu_ctx, oracle, frame, narrow, every):
    """frame 704: 11 tiles, 88 search rows; frame 4104: 65 tiles, 513 search rows (no multiple of 4)"""
    _check(gpu_ctx, oracle, {"narrow": narrow, "pub_every": every}, frame, 16, 2, 33)


@pytest.mark.parametrize("narrow", [0, 1])
@pytest.mark.parametrize("depth,channels", [(16, 2), (24, 2), (20, 2), (32, 2), (16, 1)])
def test_groups_cut_by_packet_ends(gpu_ctx, oracle, depth, channels, narrow):
    """mixed lengths inside every wave: groups that a packet's end cuts at every position, tiles that end inside a wave,
    packets shorter than a tile, than a group's search rows, than eight samples"""
    _check(gpu_ctx, oracle, {"narrow": narrow, "pub_every": 4}, 4096, depth, channels, 40, CUTS)


@pytest.mark.parametrize("opts", [{"narrow": 0}, {"thru": 1}], ids=_id)
@pytest.mark.parametrize("frame", [100, 200, 264, 520])
def test_search_rows_and_converge_part_inside_a_group(gpu_ctx, oracle, frame, opts):
    """frame 100: 12 search rows, P2 = 5 / 9; 200: 25 rows, P2 = 6 / 9; 264: 33 rows, P2 = 8 / 9; 520: 65 rows"""
    _check(gpu_ctx, oracle, opts, frame, 16, 2, 40)


def test_chained_segments_with_the_split_coder(gpu_ctx, oracle):
    """8 segments of 6 packets: positions overlapped, the final coder on two waves, the second starting at v1_split_at"""
    import torch
    nseg, per = 8, 6
    n = nseg * per
    key = ("chain", nseg, per)
    if key not in _REF:
        fmt = alac_amd.make_format(4096, 16, 2)
        pcm = alac_amd.synth_pcm(0, n, fmt)
        enc = oracle.encoder(4096, 16, 2)
        refs, escapes = [], []
        for s in range(nseg):
            a, b = s * per, (s + 1) * per
            enc.reset()
            refs.append(enc.encode_stream(pcm[a * fmt.packet_bytes:b * fmt.packet_bytes], per * 4096, 0))
            enc.reset()
            for p in range(a, b):
                enc.encode_packet(pcm[p * fmt.packet_bytes:(p + 1) * fmt.packet_bytes], 4096)
                escapes.append(int(enc.last_info()["escape"]))
        pcm.setflags(write=False)
        _REF[key] = (fmt, pcm, refs, escapes)
    fmt, pcm, refs, escapes = _REF[key]
    assert 2 * sum(escapes) <= n, f"{sum(escapes)} of {n} packets are escapes"
    seg_first = torch.arange(0, n + 1, per, dtype=torch.int32).cuda()
    state = torch.zeros((nseg, 64), dtype=torch.int16).cuda()
    with gpu_ctx.options(overlap_pos=1, split_coder=1, pub_every=4):
        assert gpu_ctx.regime(fmt, nseg) == "tiny"
        stream, sizes = gpu_ctx.encode_to_host(fmt, torch.from_numpy(pcm.copy()).cuda(), n, seg_first=seg_first, state=state)
    offs = np.concatenate([[0], np.cumsum(sizes.astype(np.int64))])
    assert offs[-1] == len(stream)
    for s, (ref, rs) in enumerate(refs):
        a, b = s * per, (s + 1) * per
        assert np.array_equal(sizes[a:b], rs), s
        assert np.array_equal(stream[offs[a]:offs[b]], ref), s
