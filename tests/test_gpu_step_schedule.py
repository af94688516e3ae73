"""The predictor step of the waves that own their SIMD runs in a fixed instruction order, with the operands of later steps
formed in the gaps of the serial chain (lms_step_lone, alac_lms.hpp; run_block_lone, alac_encode_v1_impl.hpp).  A re-ordered
step can go wrong where the order meets a boundary: blocks whose live mask is mixed (the warm-up positions at a packet's
start, the last block of a search pass), tiles cut by a packet's end, the operands prepared for a block that never runs, lanes
that hold no tap (a 4-tap row in the two-lane mapping), the 17- / 24- / 25-bit residual widths.  Every packet byte for byte and
size for size against the CPU oracle, in the regime that runs the fixed order ("narrow": 0) and in the three that keep the
compiler's ("narrow": 1, "fused": 0, "thru": 1)."""
import numpy as np
import pytest

import alac_amd

pytestmark = pytest.mark.gpu

OPTS = [{"narrow": 0}, {"narrow": 1}, {"fused": 0}, {"thru": 1}]
SIZES = [4096, 4095, 4089, 129, 128, 65, 64, 63, 17, 9, 8]

_REF = {}


def _id(v):
    return ",".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else None


def _packets(oracle, key, depth, channels, n, sizes, first=0):
    """(format, pcm, num_samples, oracle packets, oracle infos) of independent packets; computed once and shared"""
    if key not in _REF:
        fmt = alac_amd.make_format(4096, depth, channels)
        pcm = alac_amd.synth_pcm(first, n, fmt)
        ns = np.array([sizes[p % len(sizes)] for p in range(n)], np.int32)
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


@pytest.mark.parametrize("opts", OPTS, ids=_id)
@pytest.mark.parametrize("depth,channels", [(16, 2), (24, 2), (16, 1), (24, 1)])
def test_mixed_frame_sizes_in_one_batch(gpu_ctx, oracle, depth, channels, opts):
    """40 packets of 4096, 4095, 4089, 129, 128, 65, 64, 63, 17, 9 and 8 samples in turn: every wave holds packets that end in
    different tiles and blocks, packets shorter than a tile, than a block's eight steps' search rows, of exactly one block"""
    _check(gpu_ctx, opts, _packets(oracle, ("mixed", depth, channels), depth, channels, 40, SIZES))


@pytest.mark.parametrize("opts", OPTS + [{"narrow": 0, "fold": 0}], ids=_id)
def test_every_signal_class_both_row_widths_and_an_escape(gpu_ctx, oracle, opts):
    """24 whole packets, three of each of the synthetic generator's eight classes: the final pass walks 4-tap rows (the
    upper lane of the two-lane mapping holds no tap) and 8-tap rows, and at least one packet escapes"""
    case = _packets(oracle, "classes", 16, 2, 24, [4096])
    infos = case[4]
    coded = [i for i in infos if not i["escape"]]
    assert any(i["escape"] for i in infos), "no escaped packet in the batch"
    assert any(4 in (i["numU"], i["numV"]) for i in coded), "no 4-tap final row in the batch"
    assert any(8 in (i["numU"], i["numV"]) for i in coded), "no 8-tap final row in the batch"
    _check(gpu_ctx, opts, case)


@pytest.mark.parametrize("opts", OPTS, ids=_id)
def test_chained_segments_carry_the_coefficients(gpu_ctx, oracle, opts):
    """6 segments of 5 packets: the rows a packet leaves are the rows the next one starts from"""
    import torch
    nseg, per = 6, 5
    n = nseg * per
    key = ("chain", nseg, per)
    if key not in _REF:
        fmt = alac_amd.make_format(4096, 16, 2)
        pcm = alac_amd.synth_pcm(2, n, fmt)
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
