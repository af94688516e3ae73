"""Cost of measuring the BS.1770 true peak where the PCM lies (alac_hip_true_peak_int) against the loudness call on the same
plane (alac_hip_loudness_int, two filter passes and a scan where this is one pass) and against reading the source once
(alac_hip_int_probe).
    python tools/true_peak_timing.py [--out result.json] [--packets 10000,125000]
For 10 000 and 125 000 packets of 4096 16-bit stereo frames at 44.1 kHz (the synthetic PCM, in the layout alac_hip_decode
writes), in one process:
  true_peak_1024         alac_hip_true_peak_int with a table of 1 024 equal segments
  true_peak_1024_direct  the same under ALAC_HIP_TRUE_PEAK_DIRECT=1: every lane loads its own run, nothing is staged through
                         LDS; direct_equals_staged says whether both ways gave the same bytes
  true_peak_1            the same call with one segment: every block's maximum goes to the same words
  loudness_1024          alac_hip_loudness_int on the same plane and table
  probe_1024             alac_hip_int_probe on the same source and table: the cost of reading it once
The bars (each widened by the two spreads, max - min of the 7 rounds of either side):
  bar_loudness           true_peak_1024 <= loudness_1024
  bar_one_segment        true_peak_1 <= true_peak_1024
The channel peaks of the first 64 packets are compared with the restatement (tests/true_peak_ref.py) before anything is timed.
GPU times are milliseconds between two events on the context's stream around 10 calls, divided by 10: the median of 7 such
rounds after one warm-up round, with [min, max]."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import alac_amd  # noqa: E402
import true_peak_ref as tr  # noqa: E402

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


def bar(got, limit):
    """got <= limit, widened by the two spreads"""
    slack = (got["max"] - got["min"]) + (limit["max"] - limit["min"])
    return {"met": got["median"] <= limit["median"] + slack, "got_ms": got["median"], "limit_ms": limit["median"], "slack_ms": slack}


def measure(ctx, n):
    fmt = alac_amd.make_format(4096, 16, 2, FS)
    frames = n * 4096
    r = {"packets": n, "frames": frames, "pcm_bytes": n * fmt.packet_bytes, "run_frames": alac_amd.capi.TRUE_PEAK_RUN[4]}
    with torch.cuda.stream(ctx.stream):
        pcm = ctx.synth_pcm(0, n, fmt)
        x = pcm.view(torch.int16).view(frames, 2).t()
        table = [s * frames // 1024 for s in range(1025)]
        ctx.synchronize()
        head = min(n, 64) * 4096
        peaks, _ = ctx.true_peak_int(x[:, :head], FS)
        ctx.synchronize()
        _, coefs = alac_amd.true_peak_filter(FS)
        values = x[:, :head].cpu().numpy().astype(np.float64).T * 2.0 ** -15
        want, reports = tr.measure(values, FS, coefs=coefs)
        assert (np.abs(peaks.cpu().numpy() - want) <= tr.bound(coefs, np.abs(values).max(axis=0))).all()
        r["true_peak_dbtp_head"], r["peak_dbfs_head"] = tr.dbtp(reports[0][0]), tr.dbtp(reports[0][1])
        r["true_peak_1024_ms"] = rounds_ms(ctx, lambda: ctx.true_peak_int(x, FS, seg_first_frame=table))
        # the same call with every lane loading its own run (no staging through LDS): the library reads the switch per call
        staged = [t.cpu().numpy().tobytes() for t in ctx.true_peak_int(x, FS, seg_first_frame=table)]
        os.environ["ALAC_HIP_TRUE_PEAK_DIRECT"] = "1"
        try:
            direct = [t.cpu().numpy().tobytes() for t in ctx.true_peak_int(x, FS, seg_first_frame=table)]
            r["direct_equals_staged"] = direct == staged
            r["true_peak_1024_direct_ms"] = rounds_ms(ctx, lambda: ctx.true_peak_int(x, FS, seg_first_frame=table))
        finally:
            del os.environ["ALAC_HIP_TRUE_PEAK_DIRECT"]
        r["true_peak_1_ms"] = rounds_ms(ctx, lambda: ctx.true_peak_int(x, FS))
        r["loudness_1024_ms"] = rounds_ms(ctx, lambda: ctx.loudness_int(x, FS, seg_first_frame=table))
        r["probe_1024_ms"] = rounds_ms(ctx, lambda: ctx.probe_int(x, seg_first_frame=table))
        r["bar_loudness"] = bar(r["true_peak_1024_ms"], r["loudness_1024_ms"])
        r["bar_one_segment"] = bar(r["true_peak_1_ms"], r["true_peak_1024_ms"])
        r["true_peak_1024_GBps"] = r["pcm_bytes"] / r["true_peak_1024_ms"]["median"] / 1e6
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
