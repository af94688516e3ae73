"""Cost of probing float32 PCM for its lossless bit depth (alac_hip_float_probe) against the conversion pass of
alac_hip_encode_float, which reads the same floats, and against the test a torch user writes today:
    python tools/float_probe_timing.py [--out result.json]
For 10 000 and 125 000 packets of 4096 stereo frames on the 16-bit grid, planar [2, T] and interleaved (a [T, 2] tensor
viewed as [2, T]), one segment:
  probe            alac_hip_float_probe; with its achieved bytes per second (4 bytes read per sample)
  probe_1024seg    the same call with a table of 1 024 equal segments (10 000 packets only)
  encode_float     alac_hip_encode_float at 16 bits, the WHOLE call, for scale only.  The probe's bar is the undithered
                   conversion pass inside it (k_float_to_pcm), which has no call of its own: this table does not hold the bar
                   comparison.  It is read from a kernel trace of this script (rocprofv3 --kernel-trace -- python
                   tools/float_probe_timing.py), which lists k_float_probe and k_float_to_pcm dispatch by dispatch
  torch_16         isnan().any(), the range test and (x * 2^15 == round(x * 2^15)).all(): what answers "is it 16-bit?"
  torch_all        the same with three depths that miss in front (13, 14, 15, then 16): the cost of "which depth?" for material
                   that needs the fourth depth tried
Times are milliseconds between two events on the context's stream around one call, the median of 20 calls after 3 warm-up
calls; inputs are on the device and allocated once."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import alac_amd  # noqa: E402


def median_ms(ctx, fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    ctx.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(ctx.stream)
        fn()
        b.record(ctx.stream)
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def torch_depth_test(x, depths):
    """the chain a caller writes today; returns the first depth that passes, 0 for none (one host read per reduction)"""
    if bool(torch.isnan(x).any()) or bool((x >= 1.0).any()) or bool((x < -1.0).any()):
        return 0
    for b in depths:
        y = x * float(2 ** (b - 1))
        if bool((y == y.round()).all()):
            return b
    return 0


def measure(ctx, n, layout):
    fmt = alac_amd.make_format(4096, 16, 2, 44100)
    r = {"packets": n, "layout": layout, "channels": 2, "float_bytes": n * 4096 * 2 * 4}
    with torch.cuda.stream(ctx.stream):
        pcm = ctx.synth_pcm(0, n, fmt)
        x = (pcm.view(torch.int16).float() * (2.0 ** -15)).view(-1, 2)  # [T, 2]
        x = x.t() if layout == "interleaved" else x.t().contiguous()
        del pcm
        bufs = ctx.encode_buffers(fmt, n)
        assert ctx.lossless_depth(x) == [16]
        r["probe_ms"] = median_ms(ctx, lambda: ctx.probe_float(x))
        r["probe_GBps"] = r["float_bytes"] / r["probe_ms"] / 1e6
        if n <= 10000:
            table = [s * (n * 4096) // 1024 for s in range(1025)]
            assert ctx.lossless_depth(x, table) == [16] * 1024
            r["probe_1024seg_ms"] = median_ms(ctx, lambda: ctx.probe_float(x, table))
        r["encode_float_ms"] = median_ms(ctx, lambda: ctx.encode_float(fmt, x, bufs=bufs), reps=5, warm=1)
        assert torch_depth_test(x, (16, 20, 24, 32)) == 16
        r["torch_16_ms"] = median_ms(ctx, lambda: torch_depth_test(x, (16,)), reps=5, warm=1)
        r["torch_all_ms"] = median_ms(ctx, lambda: torch_depth_test(x, (13, 14, 15, 16)), reps=5, warm=1)  # three misses first
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--packets", default="10000,125000")
    a = ap.parse_args()
    ctx = alac_amd.Context(0)
    res = [measure(ctx, int(n), layout) for n in a.packets.split(",") for layout in ("planar", "interleaved")]
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
