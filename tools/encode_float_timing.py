"""Cost of encoding straight from planar float32 (alac_hip_encode_float) against encoding PCM that is already integer and
against the conversion a torch user writes today:  python tools/encode_float_timing.py [--out result.json] [--channels N]
For 10 000 and 125 000 synthetic packets (BASELINE configs[1] / the configs[3] shard), 16-bit and 24-bit, stereo or --channels
N (3..8 channels are always the conversion's general layout), every packet independent, from a float32 [channels, T] device
tensor on the grid (the synthetic PCM scaled by 2^-(bit_depth - 1)):
  encode           alac_hip_encode on the integer PCM (interleaved packed bytes, already on the device)
  encode_float     alac_hip_encode_float on the float tensor (and on the same floats interleaved, a transposed [T, 2])
  torch+encode     nan_to_num / scale / round / clamp / cast / interleave / pack to 2 or 3 bytes in torch, then encode
  dither           alac_hip_encode_float_dither (TPDF, generated in the conversion kernel) on the float tensor
  torch dither+encode   the torch route with TPDF dither from two torch.rand draws added in front of the rounding
Times are device-synchronised wall times per call (best of 4 x 5 calls; inputs and outputs on the device, allocated once).
The conversion kernel's own time (k_float_to_pcm) comes from a rocprofv3 --kernel-trace --stats run of this script."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import alac_amd  # noqa: E402


def best_of(ctx, fn, reps=5, rounds=4):
    ctx.synchronize()
    best = 1e9
    for _ in range(rounds):
        t = time.perf_counter()
        for _ in range(reps):
            fn()
        ctx.synchronize()
        best = min(best, (time.perf_counter() - t) / reps)
    return best


def to_float(pcm, depth, channels):
    """interleaved integer bytes -> float32 [channels, frames] (the tool's input, not timed)"""
    if depth == 16:
        s = pcm.view(torch.int16).to(torch.int32)
    else:
        b = pcm.view(-1, 3).to(torch.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        s = v - ((v & 0x800000) << 1)
    return (s.float() * (2.0 ** -(depth - 1))).view(-1, channels).t().contiguous()


def synth_float(ctx, n, depth, channels):
    """float32 [channels, frames] on the grid: channel pairs from the stereo generator, a last odd channel from the mono one"""
    rows, c = [], 0
    while c < channels:
        w = 2 if c + 2 <= channels else 1
        rows.append(to_float(ctx.synth_pcm(len(rows) * n, n, alac_amd.make_format(4096, depth, w, 44100)), depth, w))
        c += w
    return torch.cat(rows).contiguous()


def torch_pack(x, depth):
    """float32 [channels, frames] -> the packed interleaved bytes alac_hip_encode reads: what a caller writes in torch"""
    top = float(2 ** (depth - 1))
    s = torch.nan_to_num(x, nan=0.0).mul(top).round().clamp(-top, top - 1).to(torch.int32).t().contiguous().view(-1)
    if depth == 16:
        return s.to(torch.int16).view(torch.uint8)
    return torch.stack([s & 0xFF, (s >> 8) & 0xFF, (s >> 16) & 0xFF], dim=1).to(torch.uint8).view(-1)


def torch_dither_pack(x, depth):
    """torch_pack with TPDF dither of +-1 LSB in front of the rounding: what a caller writes in torch to get a dithered master"""
    top = float(2 ** (depth - 1))
    d = torch.rand_like(x).sub_(torch.rand_like(x))
    s = torch.nan_to_num(x, nan=0.0).mul(top).add_(d).round().clamp(-top, top - 1).to(torch.int32).t().contiguous().view(-1)
    if depth == 16:
        return s.to(torch.int16).view(torch.uint8)
    return torch.stack([s & 0xFF, (s >> 8) & 0xFF, (s >> 16) & 0xFF], dim=1).to(torch.uint8).view(-1)


def measure(ctx, n, depth, channels=2):
    fmt = alac_amd.make_format(4096, depth, channels, 44100)
    r = {"packets": n, "bit_depth": depth, "channels": channels}
    with torch.cuda.stream(ctx.stream):
        x = synth_float(ctx, n, depth, channels)
        d_pcm = ctx.synth_pcm(0, n, fmt) if channels <= 2 else torch_pack(x, depth)
        bufs = ctx.encode_buffers(fmt, n)
        ref = ctx.encode(fmt, d_pcm, n, bufs=ctx.encode_buffers(fmt, n))
        got = ctx.encode_float(fmt, x, bufs=bufs)
        ctx.synchronize()
        total = int(ref["offsets"][-1].item())
        assert torch.equal(got["offsets"], ref["offsets"]) and torch.equal(got["out"][:total], ref["out"][:total]), \
            "encode_float differs from encode"
        assert torch.equal(torch_pack(x, depth), d_pcm[:n * fmt.packet_bytes]), "torch packing differs"
        r["encode_ms"] = best_of(ctx, lambda: ctx.encode(fmt, d_pcm, n, bufs=bufs)) * 1e3
        r["encode_float_ms"] = best_of(ctx, lambda: ctx.encode_float(fmt, x, bufs=bufs)) * 1e3
        xi = x.t().contiguous().t()  # the same floats interleaved: a [T, channels] tensor viewed as [channels, T]
        r["encode_float_interleaved_ms"] = best_of(ctx, lambda: ctx.encode_float(fmt, xi, bufs=bufs)) * 1e3
        r["torch_encode_ms"] = best_of(ctx, lambda: ctx.encode(fmt, torch_pack(x, depth), n, bufs=bufs)) * 1e3
        # the dithered samples differ from the grid by at most 1: same sizes of buffers, other bytes
        r["dither_ms"] = best_of(ctx, lambda: ctx.encode_float(fmt, x, bufs=bufs, dither="tpdf", seed=1)) * 1e3
        r["dither_interleaved_ms"] = best_of(ctx, lambda: ctx.encode_float(fmt, xi, bufs=bufs, dither="tpdf", seed=1)) * 1e3
        r["torch_dither_encode_ms"] = best_of(ctx, lambda: ctx.encode(fmt, torch_dither_pack(x, depth), n, bufs=bufs)) * 1e3
        # the encoder's share of the two dithered routes: encode of PCM that is already dithered (it compresses worse
        # than the grid input above, so it is not encode_ms)
        d_dith = torch_dither_pack(x, depth)
        r["encode_dithered_pcm_ms"] = best_of(ctx, lambda: ctx.encode(fmt, d_dith, n, bufs=bufs)) * 1e3
    r["float_minus_encode_ms"] = r["encode_float_ms"] - r["encode_ms"]
    r["dither_minus_float_ms"] = r["dither_ms"] - r["encode_float_ms"]
    r["dither_over_torch_dither"] = r["dither_ms"] / r["torch_dither_encode_ms"]
    r["float_over_torch"] = r["encode_float_ms"] / r["torch_encode_ms"]
    # bytes the conversion moves: 4 read + 2 or 3 written per sample
    r["conversion_bytes"] = n * 4096 * channels * (4 + alac_amd.capi.BPS[depth])
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--packets", default="10000,125000")
    ap.add_argument("--depths", default="16,24")
    ap.add_argument("--channels", type=int, default=2, help="3..8: the general layout of the conversion (k_float_to_pcm<.., 0, ..>)")
    a = ap.parse_args()
    ctx = alac_amd.Context(0)
    res = [measure(ctx, int(n), int(d), a.channels) for d in a.depths.split(",") for n in a.packets.split(",")]
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
