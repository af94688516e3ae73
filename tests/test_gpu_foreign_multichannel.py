"""GPU parity, decode direction, FOREIGN elements inside packets of 3..8 channels: what another legal ALAC encoder writes for
a 5.1 file.  oracle/forge.py `forge_batch_mc` appends to ONE bit buffer, per packet, the element sequence of the channel count
(sChannelMaps), every element chosen on its own: foreign header parameters (any numU / numV 0..31, denShift, pbFactor, mode
!= 0, any mix weights, shift-off bytes), own-shaped ones, UNCOMPRESSED ones (escape_element) and silent ones side by side —
so the element rounds (launch_decode_v1_elements: one mono / stereo pass per element, chained through elemBit[p], written
into the wider frame behind outFirst) meet the generic predictor, the any-tap one-lane predictor, the non-specialised
entropy rounds, both kinds of position hand-over (k_dec_header's for an uncompressed element, the entropy lane's for a coded
one) and short / odd frames.  Every test decodes once and compares every packet with the oracle decoder on status,
num_samples and the first n * bytes_per_frame bytes, and with the source where the forger guarantees losslessness; the
committed fixture tests/golden/forged_mc.npz carries the reference objects' own answers."""
import functools
import json
import os
import sys

import numpy as np
import pytest

import alac_amd
from oracle_lib import channel_elements, interleave_channels

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import forge  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def gpu_decode(ctx, cookie, packets):
    import torch
    stream = np.concatenate(packets)
    offs = np.concatenate([[0], np.cumsum([len(x) for x in packets])]).astype(np.int64)
    out, ns, st, fmt = ctx.decode(cookie, torch.from_numpy(stream).cuda(), torch.from_numpy(offs).cuda(), len(packets))
    ctx.synchronize()
    return out.cpu().numpy(), ns.cpu().numpy(), st.cpu().numpy(), fmt


def oracle_answers(oracle, ck, bpf, pk, pcm, ok, info):
    """[(status, pcm bytes, n)] of the oracle decoder; the forger / oracle round trip is asserted on the way"""
    dec = oracle.decoder(ck)
    want = []
    for p, a in enumerate(pk):
        ost, w, n = dec.decode_packet(a, bpf)
        assert ost == 0, (p, ost, info[p])
        if ok[p]:
            assert n * bpf == len(pcm[p]) and np.array_equal(w, pcm[p]), ("forger / oracle round trip", p, info[p])
        want.append((ost, w, n))
    return want


def assert_same(out, ns, st, fmt, want, ok, pcm, info, what=None):
    bpf = fmt.bytes_per_frame
    bad = []
    for p, (ost, w, n) in enumerate(want):
        got = out[p * fmt.packet_bytes:p * fmt.packet_bytes + n * bpf]
        if st[p] != ost or ns[p] != n or not np.array_equal(got, w) or (ok[p] and not np.array_equal(got, pcm[p][:n * bpf])):
            first = int(np.flatnonzero(got != w)[0]) if (len(got) == len(w) and (got != w).any()) else -1
            bad.append(dict(packet=p, status=int(st[p]), num_samples=int(ns[p]), want_n=n, first_frame=first // bpf,
                            first_channel=(first % bpf) // (bpf // fmt.num_channels), info=info[p]))
    assert not bad, (what, len(bad), bad[:3])


# ---- the committed fixture --------------------------------------------------------------------------------------------------

def test_forged_mc_golden_fixture(gpu_ctx):
    """the reference objects' own answers (no oracle in the loop)"""
    z = np.load(os.path.join(GOLD, "forged_mc.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    for m in meta:
        si = m["id"]
        sizes = z[f"s{si}_sizes"]
        ends = np.cumsum(sizes)
        stream = z[f"s{si}_stream"]
        pk = [stream[e - s:e] for s, e in zip(sizes, ends)]
        out, ns, st, fmt = gpu_decode(gpu_ctx, z[f"s{si}_cookie"], pk)
        assert fmt.num_channels == m["channels"] and st.tolist() == [0] * len(pk), (si, st.tolist())
        want, woff = z[f"s{si}_pcm"], 0
        for p in range(len(pk)):
            assert ns[p] == m["elements"][p][0]["n"], (si, p, m["elements"][p])
            nb = int(ns[p]) * fmt.bytes_per_frame
            a = p * fmt.packet_bytes
            assert np.array_equal(out[a:a + nb], want[woff:woff + nb]), (m["depth"], m["channels"], p, m["elements"][p])
            woff += nb
        assert woff == len(want)


# ---- foreign elements, element by element -------------------------------------------------------------------------------------

def own_shaped(c, taps):
    return c == (taps, 9, 4, 0)  # (num, denShift, pbFactor, mode): what this library's encoder writes


def coverage(info, ok, depth, frame):
    """what the batch must hold, from the forger's own record of every element -> the list of what is missing"""
    coded = [e for els in info for e in els if not e["escape"]]
    chans = [c for e in coded for c in e["chans"]]
    pairs = [(a["escape"], b["escape"]) for els in info for a, b in zip(els, els[1:])]
    have = {
        "escape directly before a coded element": (True, False) in pairs,
        "coded directly before an escape": (False, True) in pairs,
        "mode != 0": any(c[3] != 0 for c in chans),
        "order 0": any(c[0] == 0 for c in chans),
        "order >= 9": any(c[0] >= 9 for c in chans),
        "order 1..8, not own-shaped": any(1 <= c[0] <= 8 and not (own_shaped(c, 4) or own_shaped(c, 8)) for c in chans),
        "own-shaped 4-tap": any(own_shaped(c, 4) for c in chans),
        "own-shaped 8-tap": any(own_shaped(c, 8) for c in chans),
        "pbFactor != 4": any(c[2] != 4 for c in chans),
        "n < 16": any(e["n"] < 16 for e in coded) and any(e["n"] < 16 for els in info for e in els if e["escape"]),
        "n == frame": any(e["n"] == frame for e in coded),
        "half of the packets lossless": 2 * sum(ok) >= len(ok),
    }
    if depth >= 24:
        have["shifted 0"] = any(e["shifted"] == 0 and (depth < 32 or len(e["chans"]) == 1) for e in coded)
        have["shifted >= 1"] = any(e["shifted"] >= 1 for e in coded)
        if depth == 32:
            assert all(e["shifted"] >= 1 for e in coded if len(e["chans"]) == 2)  # a 33-bit chanBits does not exist
    if depth == 32:
        have["shifted == 2"] = any(e["shifted"] == 2 for e in coded)
    return [k for k, v in have.items() if not v]


def mixed_class_pcm(oracle, channels, depth, frame, packets):
    """synthetic PCM whose elements are of different signal classes in one packet (element k runs 19 * k + 1 frames ahead)"""
    return interleave_channels([(alac_amd.synth_pcm(19 * k + 1, packets, alac_amd.make_format(frame, depth, ech)), ech)
                                for k, (ci, ech) in enumerate(channel_elements(oracle, channels))], depth)


CASES = [  # channels, depth, frame, cookie (pb, mb, kb), seed: the first from 0 for which coverage() misses nothing
    (3, 16, 256, (40, 10, 14), 0), (6, 16, 256, (20, 5, 9), 0), (8, 16, 100, (40, 10, 14), 0), (4, 24, 256, (40, 10, 14), 0),
    (6, 24, 128, (255, 255, 8), 0), (5, 20, 200, (50, 8, 13), 0), (7, 32, 128, (40, 10, 14), 0), (8, 32, 64, (25, 10, 12), 0),
]
FORGED, OWN = 48, 16


@functools.lru_cache(maxsize=None)
def case_batch(oracle, channels, depth, frame, agp, seed):
    """(cookie, packets, source PCM, lossless, info, oracle answers) of one case: forged and decoded by the oracle once, shared
    by the option sets (nothing here is written to afterwards)"""
    pb, mb, kb = agp
    rng = np.random.default_rng(seed)
    pk, pcm, ok = forge.forge_batch_mc(forge.Forger(oracle), rng, FORGED, depth, channels, frame, pb, mb, kb)
    missing = coverage(ok.info, ok, depth, frame)
    info = list(ok.info)
    if agp == (40, 10, 14):
        # packets of the oracle's ENCODER (what this library writes) interleaved with the forged ones: the fast path and the
        # generic paths side by side in one round
        fmt = alac_amd.make_format(frame, depth, channels)
        own = mixed_class_pcm(oracle, channels, depth, frame, OWN)
        enc = oracle.encoder(frame, depth, channels)
        for i in range(OWN):
            enc.reset()
            src = own[i * fmt.packet_bytes:(i + 1) * fmt.packet_bytes]
            at = int(rng.integers(0, len(pk) + 1))
            pk.insert(at, enc.encode_packet(src, frame))
            pcm.insert(at, src)
            ok.insert(at, True)
            info.insert(at, "own")
    ck = forge.cookie(frame, depth, channels, pb, mb, kb)
    want = oracle_answers(oracle, ck, channels * forge.BPS[depth], pk, pcm, ok, info)
    return ck, pk, pcm, list(ok), info, want, missing


@pytest.mark.parametrize("opts", [{}, {"dec_fused": 0}, {"dec_fused": 0, "dec_pair": 0}], ids=["auto", "unfused", "unfused-unpaired"])
@pytest.mark.parametrize("channels,depth,frame,agp,seed", CASES)
def test_foreign_elements_in_multichannel_packets(gpu_ctx, oracle, channels, depth, frame, agp, seed, opts):
    ck, pk, pcm, ok, info, want, missing = case_batch(oracle, channels, depth, frame, agp, seed)
    assert not missing, missing  # on the CPU, before the GPU is touched: the batch holds every kind of element
    with gpu_ctx.options(**opts):
        out, ns, st, fmt = gpu_decode(gpu_ctx, ck, pk)
    assert fmt.num_channels == channels
    assert_same(out, ns, st, fmt, want, ok, pcm, info, opts)


# ---- another element sequence in the batch: the whole call goes to the lane decoder --------------------------------------------

@pytest.mark.parametrize("channels,depth", [(3, 16), (6, 24)])
def test_fallback_to_the_lane_decoder_with_foreign_elements(gpu_ctx, oracle, channels, depth):
    """packet 5 carries SCEs only: decode_impl finds the mismatch and decodes the whole call again with the lane decoder,
    foreign elements included; without that packet the element rounds decode the other 23 — to the same PCM"""
    frame, odd = 128, 5
    f = forge.Forger(oracle)
    pk, pcm, ok = forge.forge_batch_mc(f, np.random.default_rng(600 + channels), 24, depth, channels, frame)
    pk1, pcm1, ok1 = forge.forge_batch_mc(f, np.random.default_rng(700 + channels), 1, depth, channels, frame,
                                          sequence=[1] * channels)
    assert len(ok1.info[0]) == channels and any(e["escape"] for els in ok.info for e in els)
    pk[odd], pcm[odd], ok[odd], ok.info[odd] = pk1[0], pcm1[0], ok1[0], ok1.info[0]
    ck = forge.cookie(frame, depth, channels)
    bpf = channels * forge.BPS[depth]
    want = oracle_answers(oracle, ck, bpf, pk, pcm, ok, ok.info)
    out, ns, st, fmt = gpu_decode(gpu_ctx, ck, pk)
    assert_same(out, ns, st, fmt, want, ok, pcm, ok.info, "with the odd packet: lane decoder")
    rest = [p for p in range(len(pk)) if p != odd]
    out2, ns2, st2, _ = gpu_decode(gpu_ctx, ck, [pk[p] for p in rest])
    for q, p in enumerate(rest):
        n = want[p][2]
        assert st2[q] == st[p] == 0 and ns2[q] == ns[p] == n, (p, ok.info[p])
        assert np.array_equal(out2[q * fmt.packet_bytes:q * fmt.packet_bytes + n * bpf],
                              out[p * fmt.packet_bytes:p * fmt.packet_bytes + n * bpf]), (p, ok.info[p])


# ---- the hand-over behind an uncompressed element, where a wrong one is not caught by the fallback --------------------------------

@pytest.mark.parametrize("channels,depth,at", [(5, 16, 1), (7, 24, 3)])
def test_uncompressed_element_before_the_last_of_its_type(gpu_ctx, oracle, channels, depth, at):
    """A round that starts at a wrong bit usually finds another element type there, reports the mismatch, and the lane decoder
    decodes the call again — correctly, which hides the mistake from every comparison of PCM.  Not here: the only uncompressed
    element of each packet is the last but one, the last is of the same type (5 channels: CPE CPE, 7: SCE LFE), so a round
    that starts anywhere inside the packet's earlier elements and finds a header decodes it without a mismatch."""
    frame = 96
    seq = forge.element_sequence(oracle, channels)
    assert at + 2 == len(seq) and seq[at][0] == seq[at + 1][0]
    rng = np.random.default_rng(channels)
    f = forge.Forger(oracle)
    pk, pcm = [], []
    for i in range(8):
        n = frame if i % 2 == 0 else (37, 5, 95)[i // 2 % 3]
        buf, pos, parts = np.zeros(n * channels * 8 + 4096, np.uint8), forge.C.c_uint64(0), []
        for k, (ech, lfe) in enumerate(seq):
            part = forge.test_signal(rng, 1 + (i + k) % 2, n, depth, ech, headroom_bits=2)
            if k == at:
                f.escape_element(part, n, depth, ech, frame, lfe=lfe, end=False, buf=buf, pos=pos)
            else:
                params = [forge.ChannelParams(5, 8, 4, 0, forge.default_coefs(5, 8)) for _ in range(ech)]
                f.element(part, n, depth, ech, frame, params, mix_bits=2, mix_res=1, lfe=lfe, end=False, buf=buf, pos=pos)
            parts.append((part, ech))
        pk.append(f.finish(buf, pos))
        pcm.append(interleave_channels(parts, depth))
    ck = forge.cookie(frame, depth, channels)
    ok, info = [True] * len(pk), [f"escape at element {at}"] * len(pk)
    want = oracle_answers(oracle, ck, channels * forge.BPS[depth], pk, pcm, ok, info)
    out, ns, st, fmt = gpu_decode(gpu_ctx, ck, pk)
    assert_same(out, ns, st, fmt, want, ok, pcm, info)


# ---- elements of different lengths ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", ["cpe_sce", "sce_cpe"])
def test_later_element_shorter(gpu_ctx, oracle, order):
    """a partial first element of 100 frames, a partial second one of 60 (frame 128): the reference's loop reports the LAST
    element's count (codec/ALACDecoder.cu: numSamples is overwritten by every partial element), and the first 60 frames
    are whole.  cpe_sce is not the sequence of a 3-channel stream (lane decoder), sce_cpe is (element rounds).  The opposite
    order is not built: frames the shorter element never wrote are the caller's buffer, not a result."""
    depth, frame, channels = 16, 128, 3
    rng = np.random.default_rng(11)
    f = forge.Forger(oracle)
    buf, pos = np.zeros(8192, np.uint8), forge.C.c_uint64(0)
    src = []
    for ech, n in ((2, 100), (1, 60)) if order == "cpe_sce" else ((1, 100), (2, 60)):
        part = forge.test_signal(rng, 2, n, depth, ech, headroom_bits=2)
        params = [forge.ChannelParams(6, 8, 4, 0, forge.default_coefs(6, 8)) for _ in range(ech)]
        f.element(part, n, depth, ech, frame, params, mix_bits=2, mix_res=1, end=False, buf=buf, pos=pos)
        src.append((part[:60 * ech * 2], ech))
    pk = [f.finish(buf, pos)]
    ck = forge.cookie(frame, depth, channels)
    ost, want, n = oracle.decoder(ck).decode_packet(pk[0], 6)
    assert ost == 0 and n == 60 and np.array_equal(want, interleave_channels(src, depth))
    out, ns, st, fmt = gpu_decode(gpu_ctx, ck, pk)
    assert st[0] == 0 and ns[0] == 60
    assert np.array_equal(out[:60 * 6], want)


# ---- randomised ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(12))
def test_random_foreign_multichannel_streams(gpu_ctx, oracle, seed):
    """randomised: depth, 3..8 channels, frame size (odd and tiny ones too), cookie parameters, 24-40 forged packets decoded in
    one call — GPU == oracle (== source where the forger guarantees losslessness)"""
    rng = np.random.default_rng(9000 + seed)
    depth = int(rng.choice([16, 16, 24, 20, 32]))
    channels = int(rng.integers(3, 9))
    frame = int(rng.choice([512, 256, 100, 64, 17, 24, 8]))
    pb, mb, kb = int(rng.choice([40, 40, 20, 63, 255, 1])), int(rng.choice([10, 10, 1, 30, 255])), int(rng.choice([14, 14, 1, 8, 16]))
    count = int(rng.integers(24, 41))
    pk, pcm, ok = forge.forge_batch_mc(forge.Forger(oracle), rng, count, depth, channels, frame, pb, mb, kb)
    ck = forge.cookie(frame, depth, channels, pb, mb, kb)
    want = oracle_answers(oracle, ck, channels * forge.BPS[depth], pk, pcm, ok, ok.info)
    out, ns, st, fmt = gpu_decode(gpu_ctx, ck, pk)
    assert_same(out, ns, st, fmt, want, ok, pcm, ok.info, (seed, depth, channels, frame, pb, mb, kb))
