"""Cost of probing integer PCM for its lossless bit depth (alac_hip_int_probe) against alac_hip_float_probe on a float tensor of
the same shape, against the conversion pass that reads the same containers (alac_hip_pcm_requantize), and against what a
caller does without it:
    python tools/int_probe_timing.py [--out result.json]
For 10 000 and 125 000 packets' worth of 4096 stereo frames of 16-bit material, one segment, all in one process:
  int32 / float32      alac_hip_int_probe on planar int32 [2, T] (24 bits left-justified) and alac_hip_float_probe on the float
                       tensor of the same samples: the same bytes and the same geometry.  The bar: the int32 probe is no slower
                       than the float probe beyond the spread the float probe shows in this run
  int16 / packed24     alac_hip_int_probe on planar int16 [2, T] and on interleaved packed 3-byte containers, in TB/s of
                       containers read, beside alac_hip_pcm_requantize on the same source (to the source's own depth: it reads
                       the same bytes and writes as many)
  torch                what decides the depth, written in torch on the device: the largest |s|, the lowest set bit over all
                       samples, whether a pad bit is set, the frames in which the channels differ (one host read)
  host                 the copy of the int32 tensor to the host and the numpy restatement of the rule's reductions (10 000
                       packets only)
Times are milliseconds between two events on the context's stream around one call, inputs on the device and allocated once.
A figure is the median over 7 rounds of the median of 10 calls (3 warm-up calls in front of the first round); "spread" is the
smallest and the largest round."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import alac_amd  # noqa: E402

ROUNDS = 7


def rounds_ms(ctx, fn, reps=10, warm=3, rounds=ROUNDS):
    for _ in range(warm):
        fn()
    ctx.synchronize()
    out = []
    for _ in range(rounds):
        times = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(ctx.stream)
            fn()
            b.record(ctx.stream)
            b.synchronize()
            times.append(a.elapsed_time(b))
        out.append(statistics.median(times))
    return {"ms": statistics.median(out), "spread_ms": [min(out), max(out)]}


def with_rate(r, nbytes):
    r["TBps"] = nbytes / r["ms"] / 1e9
    return r


def torch_reports(x, pad_bits):
    """what decides the depth of left-justified int32 [2, T] with `pad_bits` bits under the sample, in torch"""
    s = x >> pad_bits
    low = s & -s
    low = torch.where(low == 0, torch.full_like(low, 1 << 30), low)
    return (int(s.abs().max()), int(low.min()), bool((x & ((1 << pad_bits) - 1)).ne(0).any()), int((s[0] != s[1]).sum()))


def numpy_reports(x, pad_bits):
    s = x >> pad_bits
    low = s & -s
    return (int(np.abs(s).max()), int(low[low != 0].min(initial=1 << 30)), bool((x & ((1 << pad_bits) - 1)).any()),
            int((s[0] != s[1]).sum()))


def measure(ctx, n):
    t = n * 4096
    r = {"packets": n, "channels": 2, "frames": t}
    fmt16, fmt24 = alac_amd.make_format(4096, 16, 2, 44100), alac_amd.make_format(4096, 24, 2, 44100)
    with torch.cuda.stream(ctx.stream):
        pcm = ctx.synth_pcm(0, n, fmt16)
        x16 = pcm.view(torch.int16).view(-1, 2).t().contiguous()  # planar [2, T]
        del pcm
        x32 = x16.to(torch.int32) << 16                           # 24 bits left-justified in int32, 16 of them in use
        xf = x16.float() * (2.0 ** -15)
        assert ctx.lossless_depth_int(x32, bits=24) == [16] and ctx.lossless_depth(xf) == [16]
        r["int32_probe"] = with_rate(rounds_ms(ctx, lambda: ctx.probe_int(x32, bits=24)), t * 8)
        r["float_probe"] = with_rate(rounds_ms(ctx, lambda: ctx.probe_float(xf)), t * 8)
        r["int32_probe_again"] = with_rate(rounds_ms(ctx, lambda: ctx.probe_int(x32, bits=24)), t * 8)
        f = r["float_probe"]
        r["bar"] = {"float_spread_ms": f["spread_ms"][1] - f["spread_ms"][0], "gap_ms": r["int32_probe"]["ms"] - f["ms"],
                    "gap_again_ms": r["int32_probe_again"]["ms"] - f["ms"]}
        r["torch_ms"] = rounds_ms(ctx, lambda: torch_reports(x32, 8), reps=3, warm=1, rounds=3)["ms"]
        if n <= 10000:
            ctx.synchronize()
            t0 = time.perf_counter()
            host = x32.cpu().numpy()
            t1 = time.perf_counter()
            got = numpy_reports(host, 8)
            t2 = time.perf_counter()
            assert got == torch_reports(x32, 8)
            r["host_copy_ms"], r["host_numpy_ms"] = (t1 - t0) * 1e3, (t2 - t1) * 1e3
            del host
        del xf
        r["int16_probe"] = with_rate(rounds_ms(ctx, lambda: ctx.probe_int(x16)), t * 4)
        r["int16_requantize"] = with_rate(rounds_ms(ctx, lambda: ctx.requantize(fmt16, x16), reps=5, rounds=3), t * 4)
        # interleaved packed 3-byte containers of the same samples: requantize writes exactly that
        packed = ctx.requantize(fmt24, x32, bits=24)
        del x32, x16
        kw = dict(bits=24, container_bytes=3, channel_stride=1, frame_stride=2)
        assert ctx.lossless_depth_int(packed, **kw) == [16]
        r["packed24_probe"] = with_rate(rounds_ms(ctx, lambda: ctx.probe_int(packed, **kw)), t * 6)
        r["packed24_requantize"] = with_rate(rounds_ms(ctx, lambda: ctx.requantize(fmt24, packed, **kw), reps=5, rounds=3), t * 6)
        del packed
    torch.cuda.empty_cache()
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--packets", default="10000,125000")
    a = ap.parse_args()
    ctx = alac_amd.Context(0)
    res = [measure(ctx, int(n)) for n in a.packets.split(",")]
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
