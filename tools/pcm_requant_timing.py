"""Cost of encoding straight from a planar int32 tensor that holds 24-bit samples left-justified (alac_hip_encode_int, reduced
to 16 bits on the way) against the routes a caller has without it:  python tools/pcm_requant_timing.py [--out result.json]
For 10 000 and 125 000 stereo packets of 4096 frames, every packet independent, all inputs and outputs on the device and
allocated once:
  encode_int          alac_hip_encode_int on the int32 [2, T] tensor, 24 -> 16 bits, round half to even
  encode_int_dither   the same with TPDF dither generated in the conversion kernel
  encode              alac_hip_encode on PCM that is already packed 16-bit (what encode_int stages)
  torch+encode        shift, round half to even, clamp, transpose, cast to int16 in torch, then encode
  encode_float        alac_hip_encode_float on the same samples as float32 [2, T] (s * 2^-23), 16 bits
  encode_float_dither the same with the float path's TPDF dither
The routes run in one process in alternating repetitions: every round times each route once (3 calls, device-synchronised
wall time per call), and a route's figures are the minimum, the maximum and the spread (max - min) over the rounds.  Before
anything is timed the routes are checked against each other: the torch route and encode_float give encode_int's bytes.
--kernels runs only encode_int and encode_float with and without dither, alternating, for a rocprofv3 --kernel-trace --stats run: the conversion
kernels' own times (k_pcm_requantize against k_float_to_pcm) come from that trace."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import alac_amd  # noqa: E402

FS = 4096


def source(ctx, n):
    """int32 [2, n * FS]: the synthetic 16-bit PCM extended to 24 bits by 8 random bits, left-justified (<< 8)"""
    fmt16 = alac_amd.make_format(FS, 16, 2, 44100)
    s16 = ctx.synth_pcm(0, n, fmt16).view(torch.int16).view(-1, 2).t().to(torch.int32)
    g = torch.Generator(device=ctx.device).manual_seed(1)
    low = torch.randint(0, 256, s16.shape, generator=g, device=ctx.device, dtype=torch.int32)
    return ((s16 << 8) | low).contiguous() << 8


def torch_reduce(x):
    """the torch route: int32 [2, T], 24 bits left-justified -> packed interleaved 16-bit PCM, round half to even"""
    s = x >> 8
    q, rem = s >> 8, s & 255
    r = q + ((rem > 128) | ((rem == 128) & ((q & 1) == 1))).to(torch.int32)
    return r.clamp_(-32768, 32767).t().contiguous().to(torch.int16).view(-1).view(torch.uint8)


def timed(ctx, fn, calls=3):
    ctx.synchronize()
    t = time.perf_counter()
    for _ in range(calls):
        fn()
    ctx.synchronize()
    return (time.perf_counter() - t) / calls * 1e3


def measure(ctx, n, rounds, kernels_only):
    fmt = alac_amd.make_format(FS, 16, 2, 44100)
    r = {"packets": n, "frame_size": FS, "channels": 2, "source": "int32, 24 bits left-justified, planar", "bit_depth": 16}
    with torch.cuda.stream(ctx.stream):
        x = source(ctx, n)
        xf = (x >> 8).to(torch.float32) * (2.0 ** -23)
        bufs = ctx.encode_buffers(fmt, n)
        pcm = ctx.requantize(fmt, x, bits=24)
        routes = {
            "encode_int": lambda: ctx.encode_int(fmt, x, bits=24, bufs=bufs),
            "encode_int_dither": lambda: ctx.encode_int(fmt, x, bits=24, bufs=bufs, dither="tpdf", seed=1),
            "encode": lambda: ctx.encode(fmt, pcm, n, bufs=bufs),
            "torch_encode": lambda: ctx.encode(fmt, torch_reduce(x), n, bufs=bufs),
            "encode_float": lambda: ctx.encode_float(fmt, xf, bufs=bufs),
            "encode_float_dither": lambda: ctx.encode_float(fmt, xf, bufs=bufs, dither="tpdf", seed=1),
        }
        if kernels_only:
            routes = {k: routes[k] for k in ("encode_int", "encode_float", "encode_int_dither", "encode_float_dither")}
        else:
            assert torch.equal(torch_reduce(x), pcm), "the torch route differs from requantize"
            want = ctx.encode(fmt, pcm, n, bufs=ctx.encode_buffers(fmt, n))
            ctx.synchronize()
            total = int(want["offsets"][-1].item())
            for name in ("encode_int", "encode_float"):
                got = routes[name]()
                ctx.synchronize()
                assert torch.equal(got["offsets"], want["offsets"]) and torch.equal(got["out"][:total], want["out"][:total]), name
        for fn in routes.values():  # warm every route at this shape
            fn()
        ctx.synchronize()
        times = {k: [] for k in routes}
        for _ in range(rounds):
            for k, fn in routes.items():
                times[k].append(timed(ctx, fn))
    for k, t in times.items():
        r[k + "_ms"] = {"min": min(t), "max": max(t), "spread": max(t) - min(t), "rounds": t}
    if not kernels_only:
        r["int_over_torch"] = r["encode_int_ms"]["min"] / r["torch_encode_ms"]["min"]
        r["int_minus_encode_ms"] = r["encode_int_ms"]["min"] - r["encode_ms"]["min"]
        r["int_minus_float_ms"] = r["encode_int_ms"]["min"] - r["encode_float_ms"]["min"]
    # bytes either conversion moves: 4 read + 2 written per sample
    r["conversion_bytes"] = n * FS * 2 * (4 + 2)
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--packets", default="10000,125000")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args()
    ctx = alac_amd.Context(0)
    res = [measure(ctx, int(n), a.rounds, a.kernels) for n in a.packets.split(",")]
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
