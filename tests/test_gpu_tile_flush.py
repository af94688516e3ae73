"""The residual tile flush of the predictor waves (lms_pass: LDS tile -> [sample][stream] plane), every variant at its smallest:
the batched unpredicated flush of the two- and four-lane mappings (write-through with and without the zig-zag, plain stores),
the grouped predicated flush of tiles that reach a packet's end, tiles cut inside a wave, passes shorter than a tile, and the
one-lane mapping that keeps the read-and-store form.  Every packet byte for byte and size for size against the CPU oracle; by
the oracle's own account at least half of each case's packets are compressed, so no case can pass without its flush running."""
import numpy as np
import pytest

import alac_amd

pytestmark = pytest.mark.gpu

CUTS = [4096, 4095, 4033, 4032, 2049, 129, 128, 65, 64, 63, 9, 1]

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


@pytest.mark.parametrize("opts", [{"narrow": 0}, {"narrow": 1}, {"fused": 0}, {"thru": 1}],
                         ids=["two-lane", "four-lane", "stagewise", "throughput"])
def test_full_tiles(gpu_ctx, oracle, opts):
    """33 stereo packets = 66 chains: two full two-lane predictor waves and one with 30 pad slots, two coder waves"""
    _check(gpu_ctx, oracle, opts, 4096, 16, 2, 33)


@pytest.mark.parametrize("opts", [{"narrow": 0}, {"narrow": 1}], ids=["two-lane", "four-lane"])
def test_tiles_cut_by_packet_ends(gpu_ctx, oracle, opts):
    """mixed lengths inside every wave: the predicated flush, tiles that end inside a wave, packets shorter than a tile"""
    _check(gpu_ctx, oracle, opts, 4096, 16, 2, 33, CUTS)


@pytest.mark.parametrize("frame", [192, 520])
def test_search_passes_around_one_tile(gpu_ctx, oracle, frame):
    """frame / 8 = 24 search positions (less than a tile) and 65 (a tile and one sample)"""
    _check(gpu_ctx, oracle, {"narrow": 0}, frame, 16, 2, 40)


@pytest.mark.parametrize("depth,channels", [(24, 2), (16, 1)])
def test_other_formats(gpu_ctx, oracle, depth, channels):
    _check(gpu_ctx, oracle, {"narrow": 0}, 4096, depth, channels, 33)
