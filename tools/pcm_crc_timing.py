"""Cost of fingerprinting decoded PCM where it lies (alac_hip_pcm_crc32) against the route a caller had before it: the output
of alac_hip_decode copied to the host and zlib.crc32 there.
    python tools/pcm_crc_timing.py [--out result.json]
For 10 000 and 125 000 packets of 4096 16-bit stereo frames (the synthetic PCM, in the layout alac_hip_decode writes):
  crc              alac_hip_pcm_crc32 over the whole buffer as one range; with its achieved bytes per second
  crc_1024         the same call with a table of 1 024 equal ranges
  host_route       the PCM copied to pinned host memory and zlib.crc32 over it, wall clock, same process: the bar
  host_copy        the copy alone
The digests of both routes are compared before anything is timed.  GPU times are milliseconds between two events on the
context's stream around one call, the median of 20 calls after 3 warm-up calls; the host route is the median of 3 runs."""
import argparse
import json
import os
import statistics
import sys
import time
import zlib

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


def wall_ms(fn, reps=3):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def measure(ctx, n):
    fmt = alac_amd.make_format(4096, 16, 2, 44100)
    nbytes = n * fmt.packet_bytes
    r = {"packets": n, "pcm_bytes": nbytes}
    with torch.cuda.stream(ctx.stream):
        pcm = ctx.synth_pcm(0, n, fmt)
        ctx.synchronize()
        host = torch.empty(nbytes, dtype=torch.uint8).pin_memory()

        def copy():
            host.copy_(pcm, non_blocking=True)
            ctx.synchronize()

        def host_route():
            copy()
            return zlib.crc32(host.numpy())

        table = [(s * nbytes // 1024, (s + 1) * nbytes // 1024 - s * nbytes // 1024) for s in range(1024)]
        want = host_route()
        assert ctx.pcm_crc32(pcm) == [(want, nbytes)]
        parts = ctx.pcm_crc32(pcm, table)
        crc = 0
        for c, m in parts:
            crc = alac_amd.crc32_combine(crc, c, m)
        assert crc == want and sum(m for _, m in parts) == nbytes
        r["crc_ms"] = median_ms(ctx, lambda: ctx.pcm_crc32_device(pcm))
        r["crc_GBps"] = nbytes / r["crc_ms"] / 1e6
        r["crc_1024_ms"] = median_ms(ctx, lambda: ctx.pcm_crc32_device(pcm, table))
        r["host_copy_ms"] = wall_ms(copy)
        r["host_route_ms"] = wall_ms(host_route)
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
