"""Cost of measuring BS.1770 loudness where the PCM lies (alac_hip_loudness_int) against reading the same source once
(alac_hip_int_probe) and against the route a caller had before it: the PCM copied to the host and the K-weighting filter run
there (scipy.signal.lfilter, the restatement's recurrence in C).
    python tools/loudness_timing.py [--out result.json] [--packets 10000,125000] [--host-packets 10000]
For 10 000 and 125 000 packets of 4096 16-bit stereo frames at 44.1 kHz (the synthetic PCM, in the layout alac_hip_decode
writes), in one process:
  loudness_1024    alac_hip_loudness_int with a table of 1 024 equal segments
  loudness_1024_direct  the same under ALAC_HIP_LOUDNESS_DIRECT=1: every lane loads its own chunk, nothing is staged through
                   LDS; direct_equals_staged says whether both ways gave the same bytes
  loudness_1       the same call with one segment: the state scan over the groups of the one segment is one lane's serial
                   loop, and scan_serial = loudness_1 - loudness_1024 is what that loop costs (both calls filter the same
                   frames twice and move the same states)
  probe_1024 / _1  alac_hip_int_probe on the same source and tables: the cost of reading it once
  host_route       (up to --host-packets) the plane copied to pinned host memory, converted to double and filtered by two
                   lfilter calls, squared and summed per 100 ms, wall clock; host_copy is the copy alone
The rows of the device call are compared with the host route's before anything is timed (where the host route runs).  GPU
times are milliseconds between two events on the context's stream around 10 calls, divided by 10: the median of 7 such
rounds after one warm-up round, with [min, max]."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import alac_amd  # noqa: E402
import loudness_ref as lr  # noqa: E402

FS = 44100


def rounds_ms(ctx, fn, rounds=7, calls=10):
    times = []
    for r in range(rounds + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(ctx.stream)
        for _ in range(calls):
            fn()
        b.record(ctx.stream)
        b.synchronize()
        if r:
            times.append(a.elapsed_time(b) / calls)
    return {"median": statistics.median(times), "min": min(times), "max": max(times)}


def host_rows(host, frames):
    from scipy.signal import lfilter
    c = lr.coefficients(FS)
    x = host.numpy().view(np.int16).reshape(frames, 2).astype(np.float64) * 2.0 ** -15
    y = lfilter(c[5:8], np.r_[1.0, c[8:]], lfilter(c[:3], np.r_[1.0, c[3:5]], x, axis=0), axis=0)
    hop = FS // 10
    n = frames // hop
    y = y[:n * hop]
    return (y * y).reshape(n, hop, 2).sum(axis=1)


def measure(ctx, n, host_packets):
    fmt = alac_amd.make_format(4096, 16, 2, FS)
    frames = n * 4096
    r = {"packets": n, "frames": frames, "pcm_bytes": n * fmt.packet_bytes, "chunk_frames": lr.chunk_frames(FS)}
    with torch.cuda.stream(ctx.stream):
        pcm = ctx.synth_pcm(0, n, fmt)
        x = pcm.view(torch.int16).view(frames, 2).t()
        table = [s * frames // 1024 for s in range(1025)]
        ctx.synchronize()
        if n <= host_packets:
            host = torch.empty(pcm.numel(), dtype=torch.uint8).pin_memory()

            def copy():
                host.copy_(pcm, non_blocking=True)
                ctx.synchronize()

            def host_route():
                copy()
                return host_rows(host, frames)

            want = host_route()
            energy, _ = ctx.loudness_int(x, FS)
            ctx.synchronize()
            got = energy.cpu().numpy()
            assert got.shape == want.shape and (np.abs(got - want) <= 1e-9 * want + 1e-10 * (FS // 10)).all()
            r["lufs"] = alac_amd.integrated_loudness(got, FS // 10)
            t0 = time.perf_counter()
            copy()
            r["host_copy_ms"] = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            host_route()
            r["host_route_ms"] = (time.perf_counter() - t0) * 1e3
        r["loudness_1024_ms"] = rounds_ms(ctx, lambda: ctx.loudness_int(x, FS, seg_first_frame=table))
        # the same call with every lane loading its own chunk (no staging through LDS): the library reads the switch per call
        staged = [t.cpu().numpy().tobytes() for t in ctx.loudness_int(x, FS, seg_first_frame=table)]
        os.environ["ALAC_HIP_LOUDNESS_DIRECT"] = "1"
        try:
            direct = [t.cpu().numpy().tobytes() for t in ctx.loudness_int(x, FS, seg_first_frame=table)]
            r["direct_equals_staged"] = direct == staged
            r["loudness_1024_direct_ms"] = rounds_ms(ctx, lambda: ctx.loudness_int(x, FS, seg_first_frame=table))
        finally:
            del os.environ["ALAC_HIP_LOUDNESS_DIRECT"]
        r["loudness_1_ms"] = rounds_ms(ctx, lambda: ctx.loudness_int(x, FS))
        r["probe_1024_ms"] = rounds_ms(ctx, lambda: ctx.probe_int(x, seg_first_frame=table))
        r["probe_1_ms"] = rounds_ms(ctx, lambda: ctx.probe_int(x))
        r["scan_serial_ms"] = r["loudness_1_ms"]["median"] - r["loudness_1024_ms"]["median"]
        r["loudness_1024_GBps"] = r["pcm_bytes"] / r["loudness_1024_ms"]["median"] / 1e6
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--packets", default="10000,125000")
    ap.add_argument("--host-packets", type=int, default=10000)
    a = ap.parse_args()
    ctx = alac_amd.Context(0)
    res = [measure(ctx, int(n), a.host_packets) for n in a.packets.split(",")]
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
