"""Cost of decoding straight to planar float32 (alac_hip_decode_float) against a decode followed by the conversion a torch
user writes today:  python tools/decode_float_timing.py [--out result.json]
For 10 000 and 125 000 synthetic packets (BASELINE configs[1] / the configs[3] shard), 16-bit and 24-bit stereo, every
packet independent:
  decode           alac_hip_decode into a device buffer (interleaved integer bytes)
  decode_float     alac_hip_decode_float into a float32 [2, T] device tensor
  decode+convert   alac_hip_decode, then view / unpack the bytes, scale, transpose to [C, T] and .contiguous() in torch
Times are device-synchronised wall times per call (best of 4 x 5 calls; inputs and outputs on the device, allocated once)."""
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


def convert(pcm, depth, channels):
    """decode's bytes -> float32 [channels, frames] in torch: what a caller of decode() writes"""
    if depth == 16:
        s = pcm.view(torch.int16).float()
    else:  # 3-byte containers: no 24-bit dtype, so unpack by hand
        b = pcm.view(-1, 3).to(torch.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        s = (v - ((v & 0x800000) << 1)).float()
    return (s * (2.0 ** -(depth - 1))).view(-1, channels).t().contiguous()


def measure(ctx, n, depth):
    fmt = alac_amd.make_format(4096, depth, 2, 44100)
    d_pcm = ctx.synth_pcm(0, n, fmt)
    cookie = ctx.magic_cookie(fmt)
    r = {"packets": n, "bit_depth": depth, "channels": 2}
    with torch.cuda.stream(ctx.stream):
        b = ctx.encode(fmt, d_pcm, n)
        ctx.synchronize()
        out = ctx.decode(cookie, b["out"], b["offsets"], n)
        ctx.synchronize()
        assert torch.equal(out[0], d_pcm), "round trip differs"
        fl = ctx.decode_float(cookie, b["out"], b["offsets"], n)
        ctx.synchronize()
        assert torch.equal(fl[0], convert(out[0], depth, 2)), "decode_float differs from decode + conversion"
        fout = (fl[0], fl[1], fl[2])
        r["decode_ms"] = best_of(ctx, lambda: ctx.decode(cookie, b["out"], b["offsets"], n, out=out[:3])) * 1e3
        r["decode_float_ms"] = best_of(ctx, lambda: ctx.decode_float(cookie, b["out"], b["offsets"], n, out=fout)) * 1e3

        def decode_convert():
            ctx.decode(cookie, b["out"], b["offsets"], n, out=out[:3])
            return convert(out[0], depth, 2)

        r["decode_convert_ms"] = best_of(ctx, decode_convert) * 1e3
    r["float_over_decode"] = r["decode_float_ms"] / r["decode_ms"]
    r["float_over_decode_convert"] = r["decode_float_ms"] / r["decode_convert_ms"]
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--packets", default="10000,125000")
    ap.add_argument("--depths", default="16,24")
    a = ap.parse_args()
    ctx = alac_amd.Context(0)
    res = [measure(ctx, int(n), int(d)) for d in a.depths.split(",") for n in a.packets.split(",")]
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
